// eval_kernels.hip -- the SI-SDR of every (estimate, reference) pair of a ragged batch of samples on the device, in
// float64 and in the two passes of the host statement hostdsp.si_sdr (include/asw_hip.h: asw_cross_sisdr; DESIGN.md
// section 7o).
//
// Pass A sums rr = sum ref^2 and sum ref est of every pair (xs_pass<0>, xs_coef), pass B sums te = sum (a ref)^2 and
// ne = sum (est - a ref)^2 element by element with a = sum ref est / rr known (xs_pass<1>, xs_value); xs_status folds
// the per-tile flags into status.  The house rules of bss_kernels.hip hold: every launch is a grid over host-built
// lists, workgroups hand nothing to each other inside a launch, there are no atomics and no device-side asserts, every
// address has one writer and every sum has one fixed order.  Compiled with -ffp-contract=off (native.EXTRA_FLAGS): the
// statement rounds a * ref before it subtracts.
#include "asw_common.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int TE = 8, TS = 8;          // a tile: estimate rows x reference rows of one item, a lane per pair
constexpr int NPAIR = TE * TS;         // 64: one wave
constexpr int TC = 512;                // samples per chunk; wave w of the four sums samples [128 w, 128 w + 128) of it
constexpr int LD = TC + 1;             // LDS row pitch: lanes of different rows read different banks
constexpr int MAX_SPLIT = 8;           // partial sums per pair (each a run of whole chunks)
constexpr int MAX_K = 65535, MAX_P = 4096, MAX_S = 64;
constexpr int MAX_T = 1 << 25;
constexpr double MIN_ERR = 1e-8;       // hostdsp.MIN_ERR

struct Item {                          // one sample of the batch
  int64_t e0, r0, out_off;             // first estimate row, first reference row, first output slot
  int32_t P, S, tile0, ntiles;
};
struct Tile { int32_t item, pe, rs, pad; };      // estimate rows pe .. pe + TE, reference rows rs .. rs + TS of the item

struct Plan {
  int K, T;
  long NE, NR, NP, ntiles;
  int nchunk, cps, nsplit;
  size_t tab_bytes, o_items, o_tiles, o_coef, o_part, o_bad, total;
};

// null on success, else the refusal.  Sizes only: no pointer but the counts is looked at.
const char* make_plan(const int32_t* ec, const int32_t* rc, int K, int T, Plan& p, char* msg, size_t msg_len) {
  if (K < 0 || K > MAX_K) { snprintf(msg, msg_len, "K = %d outside 0..%d", K, MAX_K); return msg; }
  if (T < 1 || T > MAX_T) { snprintf(msg, msg_len, "T = %d outside 1..%d", T, MAX_T); return msg; }
  if (K > 0 && !(ec && rc)) { snprintf(msg, msg_len, "null counts"); return msg; }
  p = Plan{};
  p.K = K, p.T = T;
  for (int k = 0; k < K; ++k) {
    const long P = ec[k], S = rc[k];
    if (P < 0 || S < 0) { snprintf(msg, msg_len, "item %d: negative count (%ld estimates, %ld references)", k, P, S); return msg; }
    if (P > MAX_P || S > MAX_S) {
      snprintf(msg, msg_len, "item %d: %ld estimates (at most %d) or %ld references (at most %d)", k, P, MAX_P, S, MAX_S);
      return msg;
    }
    p.NE += P, p.NR += S, p.NP += P * S;
    if (P > 0 && S > 0) p.ntiles += (long)asw::cdiv(P, TE) * asw::cdiv(S, TS);
  }
  p.nchunk = asw::cdiv(T, TC);
  const int split = p.nchunk < MAX_SPLIT ? p.nchunk : MAX_SPLIT;
  p.cps = asw::cdiv(p.nchunk, split);
  p.nsplit = asw::cdiv(p.nchunk, p.cps);
  size_t o = 0;
  p.o_items = o, o += (size_t)K * sizeof(Item);
  p.o_tiles = o, o += (size_t)p.ntiles * sizeof(Tile);
  p.tab_bytes = o;
  p.o_coef = o, o += (size_t)p.NP * 2 * sizeof(double);                              // (a, rr) per pair
  p.o_part = o, o += (size_t)p.ntiles * p.nsplit * NPAIR * 2 * sizeof(double);       // both passes, one after the other
  p.o_bad = o, o += (size_t)((p.ntiles + 1) / 2) * 8;                                // int32 per tile
  p.total = o < 8 ? 8 : o;
  return nullptr;
}

// ---- passes A and B: part[tile][split][pair] = the two sums of the pair over the split's samples.
// PASS 0: (sum ref^2, sum ref est).  PASS 1: (sum (a ref)^2, sum (est - a ref)^2), a = coef[pair].
// The rows of a tile are staged chunk by chunk in LDS, once per pass for all its pairs; a row beyond the item's own
// (the ragged edge of a tile) and the samples beyond T are staged as zeros and never read from memory.
template <int PASS>
__global__ __launch_bounds__(256) void xs_pass_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                      const Item* __restrict__ items, const Tile* __restrict__ tiles, int T,
                                                      int cps, int nchunk, int nsplit, const double* __restrict__ coef,
                                                      double* __restrict__ part) {
  __shared__ float es[TE * LD], rs[TS * LD];
  __shared__ double red[4][NPAIR][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Tile tl = tiles[blockIdx.x];
  const Item it = items[tl.item];
  const int ne = it.P - tl.pe < TE ? it.P - tl.pe : TE, nr = it.S - tl.rs < TS ? it.S - tl.rs : TS;
  const int le = lane / TS, lr = lane % TS;
  const bool live = le < ne && lr < nr;
  const float* ebase = est + (size_t)(it.e0 + tl.pe) * T;
  const float* rbase = ref + (size_t)(it.r0 + tl.rs) * T;
  double a = 0.0;
  if (PASS == 1 && live) a = coef[2 * (it.out_off + (int64_t)(tl.pe + le) * it.S + tl.rs + lr)];
  double s0 = 0.0, s1 = 0.0;
  const int c0 = blockIdx.y * cps, c1 = c0 + cps < nchunk ? c0 + cps : nchunk;
  for (int c = c0; c < c1; ++c) {
    const int t0 = c * TC, len = T - t0 < TC ? T - t0 : TC;
    __syncthreads();
    for (int row = 0; row < TE; ++row)
      for (int u = tid; u < TC; u += 256) es[row * LD + u] = row < ne && u < len ? ebase[(size_t)row * T + t0 + u] : 0.0f;
    for (int row = 0; row < TS; ++row)
      for (int u = tid; u < TC; u += 256) rs[row * LD + u] = row < nr && u < len ? rbase[(size_t)row * T + t0 + u] : 0.0f;
    __syncthreads();
    const float* ep = es + le * LD + w * (TC / 4);
    const float* rp = rs + lr * LD + w * (TC / 4);
    for (int u = 0; u < TC / 4; ++u) {
      const double e = (double)ep[u], r = (double)rp[u];
      if (PASS == 0) {
        s0 += r * r;
        s1 += r * e;
      } else {
        const double tg = a * r, d = e - tg;
        s0 += tg * tg;
        s1 += d * d;
      }
    }
  }
  red[w][lane][0] = s0, red[w][lane][1] = s1;
  __syncthreads();
  if (w == 0 && live) {
    double f0 = red[0][lane][0], f1 = red[0][lane][1];
    for (int q = 1; q < 4; ++q) f0 += red[q][lane][0], f1 += red[q][lane][1];
    double* out = part + (((size_t)blockIdx.x * nsplit + blockIdx.y) * NPAIR + lane) * 2;
    out[0] = f0, out[1] = f1;
  }
}

// coef[pair] = (a, rr): the runs of pass A folded left to right, a = sum ref est / rr as the statement divides
__global__ __launch_bounds__(NPAIR) void xs_coef_kernel(const Item* __restrict__ items, const Tile* __restrict__ tiles, int nsplit,
                                                        const double* __restrict__ part, double* __restrict__ coef) {
  const int lane = threadIdx.x;
  const Tile tl = tiles[blockIdx.x];
  const Item it = items[tl.item];
  const int le = lane / TS, lr = lane % TS;
  if (tl.pe + le >= it.P || tl.rs + lr >= it.S) return;
  const double* in = part + ((size_t)blockIdx.x * nsplit * NPAIR + lane) * 2;
  double rr = in[0], dot = in[1];
  for (int q = 1; q < nsplit; ++q) rr += in[(size_t)q * NPAIR * 2], dot += in[(size_t)q * NPAIR * 2 + 1];
  double* out = coef + 2 * (it.out_off + (int64_t)(tl.pe + le) * it.S + tl.rs + lr);
  out[0] = dot / rr, out[1] = rr;
}

// out[pair] = 10 log10(te / (ne + 1e-8)); bad[tile] = 1 when a pair of the tile has rr == 0, te == 0 or a value that
// is not finite (the flags of the tile's lanes folded in LDS by one thread)
__global__ __launch_bounds__(NPAIR) void xs_value_kernel(const Item* __restrict__ items, const Tile* __restrict__ tiles, int nsplit,
                                                         const double* __restrict__ part, const double* __restrict__ coef,
                                                         double* __restrict__ out, int32_t* __restrict__ bad) {
  __shared__ int32_t flag[NPAIR];
  const int lane = threadIdx.x;
  const Tile tl = tiles[blockIdx.x];
  const Item it = items[tl.item];
  const int le = lane / TS, lr = lane % TS;
  int32_t f = 0;
  if (tl.pe + le < it.P && tl.rs + lr < it.S) {
    const double* in = part + ((size_t)blockIdx.x * nsplit * NPAIR + lane) * 2;
    double te = in[0], ne = in[1];
    for (int q = 1; q < nsplit; ++q) te += in[(size_t)q * NPAIR * 2], ne += in[(size_t)q * NPAIR * 2 + 1];
    const int64_t slot = it.out_off + (int64_t)(tl.pe + le) * it.S + tl.rs + lr;
    const double v = 10.0 * log10(te / (ne + MIN_ERR));
    out[slot] = v;
    f = coef[2 * slot + 1] == 0.0 || te == 0.0 || !(fabs(v) <= 1.7976931348623157e308);
  }
  flag[lane] = f;
  __syncthreads();
  if (lane == 0) {
    int32_t any = 0;
    for (int q = 0; q < NPAIR; ++q) any |= flag[q];
    bad[blockIdx.x] = any;
  }
}

// status[k] = 1 when a tile of item k is flagged, 0 otherwise (also for an item without pairs): a workgroup per item
__global__ __launch_bounds__(256) void xs_status_kernel(const Item* __restrict__ items, const int32_t* __restrict__ bad,
                                                        int32_t* __restrict__ status) {
  __shared__ int32_t flag[256];
  const int tid = threadIdx.x;
  const Item it = items[blockIdx.x];
  int32_t f = 0;
  for (int q = tid; q < it.ntiles; q += 256) f |= bad[it.tile0 + q];
  flag[tid] = f;
  for (int s = 128; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) flag[tid] |= flag[tid + s];
  }
  if (tid == 0) status[blockIdx.x] = flag[0] != 0;
}

}  // namespace

extern "C" size_t asw_cross_sisdr_workspace_bytes(const int32_t* est_counts, const int32_t* ref_counts, int K, int T) {
  Plan p;
  char msg[160];
  if (make_plan(est_counts, ref_counts, K, T, p, msg, sizeof msg)) {
    asw::set_error(ASW_ERR_ARG, "cross_sisdr_workspace_bytes: %s", msg);
    return 0;
  }
  return p.total;
}

extern "C" int asw_cross_sisdr(const float* est, const float* ref, const int32_t* est_counts, const int32_t* ref_counts, int K,
                               int T, double* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  Plan p;
  char msg[160];
  if (make_plan(est_counts, ref_counts, K, T, p, msg, sizeof msg)) return asw::set_error(ASW_ERR_ARG, "cross_sisdr: %s", msg);
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(status && workspace, "cross_sisdr: null status or workspace");
  ASW_CHECK_ARG((est || p.NE == 0) && (ref || p.NR == 0) && (out || p.NP == 0), "cross_sisdr: null pointer");
  ASW_CHECK_ARG(workspace_bytes >= p.total, "cross_sisdr: workspace of %zu bytes too small, %zu needed", workspace_bytes, p.total);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "cross_sisdr: workspace not 8-byte aligned");
  hipStream_t s = asw::as_stream(stream);

  // the lists every launch is a grid over
  std::vector<unsigned char> blob(p.tab_bytes);
  Item* hi = reinterpret_cast<Item*>(blob.data() + p.o_items);
  Tile* ht = reinterpret_cast<Tile*>(blob.data() + p.o_tiles);
  int64_t e0 = 0, r0 = 0, o0 = 0;
  long nt = 0;
  for (int k = 0; k < K; ++k) {
    const int P = est_counts[k], S = ref_counts[k];
    const long first = nt;
    if (P > 0 && S > 0)
      for (int pe = 0; pe < P; pe += TE)
        for (int rs = 0; rs < S; rs += TS) ht[nt++] = Tile{k, pe, rs, 0};
    hi[k] = Item{e0, r0, o0, P, S, (int32_t)first, (int32_t)(nt - first)};
    e0 += P, r0 += S, o0 += (int64_t)P * S;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const Item* di = reinterpret_cast<const Item*>(ws + p.o_items);
  const Tile* dt = reinterpret_cast<const Tile*>(ws + p.o_tiles);
  double* coef = reinterpret_cast<double*>(ws + p.o_coef);
  double* part = reinterpret_cast<double*>(ws + p.o_part);
  int32_t* bad = reinterpret_cast<int32_t*>(ws + p.o_bad);
  // pageable source: the runtime has taken the table before the call returns
  ASW_HIP(hipMemcpyAsync(ws, blob.data(), p.tab_bytes, hipMemcpyHostToDevice, s));
  if (p.ntiles > 0) {
    const dim3 grid((unsigned)p.ntiles, (unsigned)p.nsplit);
    const double bytes = (double)p.ntiles * (TE + TS) * T * 4;
    {
      asw::ProfScope prof(s, "xs_pass_a", 4.0 * (double)p.NP * T, bytes);
      hipLaunchKernelGGL(xs_pass_kernel<0>, grid, dim3(256), 0, s, est, ref, di, dt, T, p.cps, p.nchunk, p.nsplit,
                         (const double*)nullptr, part);
      ASW_LAUNCH_CHECK();
    }
    {
      asw::ProfScope prof(s, "xs_coef", 0.0, 0.0);
      hipLaunchKernelGGL(xs_coef_kernel, dim3((unsigned)p.ntiles), dim3(NPAIR), 0, s, di, dt, p.nsplit, part, coef);
      ASW_LAUNCH_CHECK();
    }
    {
      asw::ProfScope prof(s, "xs_pass_b", 6.0 * (double)p.NP * T, bytes);
      hipLaunchKernelGGL(xs_pass_kernel<1>, grid, dim3(256), 0, s, est, ref, di, dt, T, p.cps, p.nchunk, p.nsplit,
                         (const double*)coef, part);
      ASW_LAUNCH_CHECK();
    }
    {
      asw::ProfScope prof(s, "xs_value", 0.0, 0.0);
      hipLaunchKernelGGL(xs_value_kernel, dim3((unsigned)p.ntiles), dim3(NPAIR), 0, s, di, dt, p.nsplit, part, coef, out, bad);
      ASW_LAUNCH_CHECK();
    }
  }
  asw::ProfScope prof(s, "xs_status", 0.0, 0.0);
  hipLaunchKernelGGL(xs_status_kernel, dim3((unsigned)K), dim3(256), 0, s, di, bad, status);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
