// stft_kernels.hip -- the STFT / inverse STFT of scipy.signal.stft(x, nperseg=2048) / istft on the device in float64,
// and on top of them the oracle mask baselines of the evaluation, the ideal ratio mask and the ideal binary mask
// (include/asw_hip.h: asw_stft, asw_istft, asw_oracle_masks; the statements are oracle_masks.stft_f64, istft_f64,
// irm_f64 and ibm_f64).
//
// A workgroup of 256 threads owns one frame.  The 2048 real samples of a windowed frame are read as 1024 complex values
// z[m] = x[2m] + i x[2m+1], transformed by a 1024-point radix-2 Stockham FFT that ping-pongs between two LDS buffers
// (self-sorting: no bit reversal), and split into the 1025 one-sided bins; the inverse runs the same three steps
// backwards.  Real and imaginary parts live in separate arrays, so that consecutive lanes read consecutive 8-byte words.
// A thread owns the bin pairs (k, 1024 - k) of k = tid, tid + 256 (and 512 for thread 0) in every split: what it keeps
// per bin between transforms -- the mixture's spectrum, the ratio mask's denominator -- is written and read by it alone.
// The house rules of eval_kernels.hip hold: grids over host-built tables, no atomics, no cross-lane operations, no
// device-side assert, one writer per address, every sum in one fixed order.
#include "asw_common.h"
#include "fft1024.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

namespace {

using namespace asw::fft;              // NFFT, HOP, NB, NH, THREADS; Lds, fft1024, the split and merge steps (fft1024.h)
constexpr int MAX_K = 65535, MAX_S = 64, MAX_ROWS = 65535;
constexpr int MAX_T = 1 << 25;
constexpr long MAX_GRID = 1L << 30;
constexpr double EPS = 2.220446049250313e-16;                  // np.finfo(np.float64).eps

// the tables of a device, float64, built on the host once: tw[t] = exp(-2 pi i t / 2048) for t < 1024 as (cos, -sin)
// pairs, the analysis window w, the synthesis factor w * sum(w), the divisor of the overlap-add and sum(w)
constexpr int O_TW = 0, O_WIN = 2 * NH, O_SYN = O_WIN + NFFT, O_NORM = O_SYN + NFFT, O_WSUM = O_NORM + HOP, N_TAB = O_WSUM + 1;

struct DeviceTables {
  static constexpr int kMaxDev = 64;
  std::mutex mu;
  double* tab[kMaxDev] = {};
};
DeviceTables g_tables;

int device_tables(const double** out) {
  int dev = 0;
  ASW_HIP(hipGetDevice(&dev));
  ASW_CHECK_ARG(dev >= 0 && dev < DeviceTables::kMaxDev, "stft: device %d beyond the %d this library keeps tables for", dev,
                DeviceTables::kMaxDev);
  std::lock_guard<std::mutex> lk(g_tables.mu);
  if (!g_tables.tab[dev]) {
    std::vector<double> h(N_TAB);
    const double pi = 3.14159265358979323846;
    fill_twiddles(&h[O_TW]);
    double wsum = 0.0;
    for (int n = 0; n < NFFT; ++n) {
      h[O_WIN + n] = 0.5 - 0.5 * std::cos(2.0 * pi * n / NFFT);
      wsum += h[O_WIN + n];
    }
    for (int n = 0; n < NFFT; ++n) h[O_SYN + n] = h[O_WIN + n] * wsum;
    for (int r = 0; r < HOP; ++r) {
      const double nr = h[O_WIN + HOP + r] * h[O_WIN + HOP + r] + h[O_WIN + r] * h[O_WIN + r];
      h[O_NORM + r] = nr > 1e-10 ? nr : 1.0;
    }
    h[O_WSUM] = wsum;
    double* d = nullptr;
    if (hipMalloc(&d, N_TAB * sizeof(double)) != hipSuccess) return asw::set_error(ASW_ERR_NOMEM, "stft: hipMalloc of the tables");
    if (hipMemcpy(d, h.data(), N_TAB * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return asw::set_error(ASW_ERR_HIP, "stft: copy of the tables");
    }
    g_tables.tab[dev] = d;
  }
  *out = g_tables.tab[dev];
  return ASW_OK;
}

inline int frames_of(int N) { return (N + HOP - 1) / HOP + 1; }          // oracle_masks.frame_count

struct Item {                          // one (mixture row, reference rows) group; for asw_istft the one group of all rows
  int64_t row0, slot0;                 // first row of ref / out; first frame slot (2048 doubles each) of the workspace
  int32_t S, N, F, pad;
};

// ---- device pieces -----------------------------------------------------------------------------------------------
// frame f of a row of N float32 samples, windowed, into buffer 0: padded sample p = 1024 f + n is x[p - 1024] or 0
__device__ __forceinline__ void load_frame(Lds& L, const float* __restrict__ row, int N, int f, const double* __restrict__ win,
                                           int tid) {
  __syncthreads();
  for (int m = tid; m < NH; m += THREADS) {
    const int64_t t = (int64_t)f * HOP - HOP + 2 * m;
    const double a = t >= 0 && t < N ? (double)row[t] : 0.0, b = t + 1 >= 0 && t + 1 < N ? (double)row[t + 1] : 0.0;
    L.re[0][m] = a * win[2 * m], L.im[0][m] = b * win[2 * m + 1];
  }
}

// the time frame in buffer 0 (after the inverse transform), times w * sum(w), to its slot of the workspace
__device__ __forceinline__ void store_frame(const Lds& L, const double* __restrict__ syn, double* __restrict__ slot, int tid) {
  for (int m = tid; m < NH; m += THREADS)
    *reinterpret_cast<double2*>(slot + 2 * m) = make_double2(L.re[0][m] * syn[2 * m], L.im[0][m] * syn[2 * m + 1]);
}

__device__ __forceinline__ double mag_pow(Cx v, double alpha) {
  const double m = hypot(v.r, v.i);
  return alpha == 1.0 ? m : pow(m, alpha);
}

// ---- asw_stft: grid (F, R) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void stft_kernel(const float* __restrict__ x, int N, int F, const double* __restrict__ tab,
                                                       double2* __restrict__ z) {
  __shared__ Lds L;
  const int tid = threadIdx.x, f = blockIdx.x;
  const int64_t row = blockIdx.y;
  const double* tw = tab + O_TW;
  const double wsum = tab[O_WSUM];
  load_frame(L, x + row * N, N, f, tab + O_WIN, tid);
  fft1024<false>(L, tw, tid);
  double2* out = z + row * NB * F + f;                                  // bin k at out[k F]
  for (int k = tid; k <= NH / 2; k += THREADS) {
    Cx a, b;
    if (k == 0) split_ends(L, wsum, a, b); else split_pair(L, tw, k, wsum, a, b);
    out[(int64_t)k * F] = make_double2(a.r, a.i);
    out[(int64_t)(NH - k) * F] = make_double2(b.r, b.i);
  }
}

// ---- asw_istft, first launch: grid (F, R); the windowed time frames go to the workspace ----------------------------
__global__ __launch_bounds__(THREADS) void istft_frames_kernel(const double2* __restrict__ z, int F, const double* __restrict__ tab,
                                                               double* __restrict__ frames) {
  __shared__ Lds L;
  const int tid = threadIdx.x, f = blockIdx.x;
  const int64_t row = blockIdx.y;
  const double* tw = tab + O_TW;
  const double2* in = z + row * NB * F + f;
  for (int k = tid; k <= NH / 2; k += THREADS) {
    const double2 a = in[(int64_t)k * F], b = in[(int64_t)(NH - k) * F];
    if (k == 0) merge_ends(L, a.x, b.x); else merge_pair(L, tw, k, Cx{a.x, a.y}, Cx{b.x, b.y});
  }
  fft1024<true>(L, tw, tid);
  store_frame(L, tab + O_SYN, frames + (row * F + f) * NFFT, tid);
}

// ---- the overlap-add: grid (chunks of 1024 samples of the stride, row of the item, item) ----------------------------
// out[row][t] = (frame f-1 at r + 1024, then frame f at r) / divisor[r] with t + 1024 = 1024 f + r, for t < N; 0 from N
// up to the stride.  One thread per sample: it gathers its two frames, nothing is accumulated in memory.
__global__ __launch_bounds__(THREADS) void overlap_add_kernel(const Item* __restrict__ items, const double* __restrict__ frames,
                                                              const double* __restrict__ tab, int stride,
                                                              double* __restrict__ out) {
  const Item it = items[blockIdx.z];
  if ((int)blockIdx.y >= it.S) return;
  const double* fr = frames + (it.slot0 + (int64_t)blockIdx.y * it.F) * NFFT;
  double* o = out + (it.row0 + blockIdx.y) * stride;
  const int f = blockIdx.x + 1;                                          // the later of the two frames of this chunk
  for (int r = threadIdx.x; r < HOP; r += THREADS) {
    const int64_t t = (int64_t)blockIdx.x * HOP + r;
    if (t >= stride) break;
    double v = 0.0;
    if (t < it.N) v = (fr[(int64_t)(f - 1) * NFFT + HOP + r] + fr[(int64_t)f * NFFT + r]) / tab[O_NORM + r];
    o[t] = v;
  }
}

// ---- asw_oracle_masks, first launch: grid (max F, K).  A workgroup transforms frame f of the item's mixture and keeps
// the spectrum; for the ratio mask a first pass over the sources sums |S_k|^alpha per bin, starting from eps and in
// source order; then source after source is transformed (again), masked, merged and transformed back, and its windowed
// time frame goes to the workspace.  No spectrum leaves the workgroup.
__global__ __launch_bounds__(THREADS) void oracle_frames_kernel(const float* __restrict__ mix, const float* __restrict__ ref,
                                                                const Item* __restrict__ items, int stride, int ibm, double alpha,
                                                                double theta, const double* __restrict__ tab,
                                                                double* __restrict__ frames) {
  __shared__ Lds L;
  __shared__ double Xr[NB], Xi[NB], den[NB];
  const int tid = threadIdx.x, f = blockIdx.x;
  const Item it = items[blockIdx.y];
  if (f >= it.F) return;
  const double* tw = tab + O_TW;
  const double* win = tab + O_WIN;
  const double wsum = tab[O_WSUM];
  load_frame(L, mix + (int64_t)blockIdx.y * stride, it.N, f, win, tid);
  fft1024<false>(L, tw, tid);
  for (int k = tid; k <= NH / 2; k += THREADS) {
    Cx a, b;
    if (k == 0) split_ends(L, wsum, a, b); else split_pair(L, tw, k, wsum, a, b);
    Xr[k] = a.r, Xi[k] = a.i, Xr[NH - k] = b.r, Xi[NH - k] = b.i;
    if (ibm) den[k] = EPS + mag_pow(a, alpha), den[NH - k] = EPS + mag_pow(b, alpha);
    else den[k] = EPS, den[NH - k] = EPS;
  }
  if (!ibm)
    for (int j = 0; j < it.S; ++j) {
      load_frame(L, ref + (it.row0 + j) * stride, it.N, f, win, tid);
      fft1024<false>(L, tw, tid);
      for (int k = tid; k <= NH / 2; k += THREADS) {
        Cx a, b;
        if (k == 0) split_ends(L, wsum, a, b); else split_pair(L, tw, k, wsum, a, b);
        const double pa = mag_pow(a, alpha), pb = mag_pow(b, alpha);
        den[k] += pa;
        if (k != NH - k) den[NH - k] += pb;
      }
    }
  for (int j = 0; j < it.S; ++j) {
    load_frame(L, ref + (it.row0 + j) * stride, it.N, f, win, tid);
    fft1024<false>(L, tw, tid);
    for (int k = tid; k <= NH / 2; k += THREADS) {
      Cx a, b;
      if (k == 0) split_ends(L, wsum, a, b); else split_pair(L, tw, k, wsum, a, b);
      const int km = NH - k;
      double ma = mag_pow(a, alpha) / den[k], mb = mag_pow(b, alpha) / den[km];
      if (ibm) {                                                         // the reference's two assignments, in its order
        ma = ma >= theta ? 1.0 : ma, ma = ma < theta ? 0.0 : ma;
        mb = mb >= theta ? 1.0 : mb, mb = mb < theta ? 0.0 : mb;
      }
      const Cx ya{Xr[k] * ma, Xi[k] * ma}, yb{Xr[km] * mb, Xi[km] * mb};
      if (k == 0) merge_ends(L, ya.r, yb.r); else merge_pair(L, tw, k, ya, yb);
    }
    fft1024<true>(L, tw, tid);
    store_frame(L, tab + O_SYN, frames + (it.slot0 + (int64_t)j * it.F + f) * NFFT, tid);
  }
}

// ---- plans -------------------------------------------------------------------------------------------------------
struct Plan {
  long rows, slots;
  int maxF, maxS;
  size_t tab_bytes, o_frames, total;
};

const char* make_plan(const int32_t* counts, const int32_t* lengths, int K, Plan& p, char* msg, size_t msg_len) {
  if (K < 0 || K > MAX_K) { snprintf(msg, msg_len, "K = %d outside 0..%d", K, MAX_K); return msg; }
  if (K > 0 && !(counts && lengths)) { snprintf(msg, msg_len, "null counts or lengths"); return msg; }
  p = Plan{};
  for (int k = 0; k < K; ++k) {
    const long S = counts[k], N = lengths[k];
    if (S < 0 || S > MAX_S) { snprintf(msg, msg_len, "item %d: %ld references outside 0..%d", k, S, MAX_S); return msg; }
    if (N < NFFT || N > MAX_T) { snprintf(msg, msg_len, "item %d: %ld samples outside %d..%d", k, N, NFFT, MAX_T); return msg; }
    const int F = frames_of((int)N);
    p.rows += S, p.slots += S * F;
    if (F > p.maxF) p.maxF = F;
    if (S > p.maxS) p.maxS = (int)S;
  }
  p.tab_bytes = (size_t)K * sizeof(Item);
  p.o_frames = p.tab_bytes;
  p.total = p.o_frames + (size_t)p.slots * NFFT * sizeof(double);
  if (p.total < 8) p.total = 8;
  return nullptr;
}

}  // namespace

extern "C" int asw_stft(const float* x, int R, int N, double* z, void* stream) {
  ASW_CHECK_ARG(R >= 0 && R <= MAX_ROWS && N >= NFFT && N <= MAX_T, "stft: bad shape (R=%d within 0..%d, N=%d within %d..%d)", R,
                MAX_ROWS, N, NFFT, MAX_T);
  if (R == 0) return ASW_OK;
  ASW_CHECK_ARG(x && z, "stft: null pointer");
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(z) & 15) == 0, "stft: z not 16-byte aligned");
  const double* tab = nullptr;
  if (int rc = device_tables(&tab)) return rc;
  hipStream_t s = asw::as_stream(stream);
  const int F = frames_of(N);
  asw::ProfScope prof(s, "stft", 5.0 * NH * 10 * (double)R * F, (double)R * F * (NFFT * 4.0 + NB * 16.0));
  hipLaunchKernelGGL(stft_kernel, dim3(F, R), dim3(THREADS), 0, s, x, N, F, tab, reinterpret_cast<double2*>(z));
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" size_t asw_istft_workspace_bytes(int R, int F) {
  if (R < 0 || R > MAX_ROWS || F < 2 || F > frames_of(MAX_T)) {
    asw::set_error(ASW_ERR_ARG, "istft_workspace_bytes: R=%d outside 0..%d or F=%d outside 2..%d", R, MAX_ROWS, F, frames_of(MAX_T));
    return 0;
  }
  return sizeof(Item) + (size_t)R * F * NFFT * sizeof(double);
}

extern "C" int asw_istft(const double* z, int R, int F, int N, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  ASW_CHECK_ARG(R >= 0 && R <= MAX_ROWS && F >= 2 && F <= frames_of(MAX_T), "istft: bad shape (R=%d within 0..%d, F=%d within 2..%d)",
                R, MAX_ROWS, F, frames_of(MAX_T));
  ASW_CHECK_ARG(N >= 0 && N <= (F - 1) * HOP, "istft: N=%d outside 0..%d, what %d frames cover", N, (F - 1) * HOP, F);
  if (R == 0 || N == 0) return ASW_OK;
  ASW_CHECK_ARG(z && out && workspace, "istft: null pointer");
  const size_t need = sizeof(Item) + (size_t)R * F * NFFT * sizeof(double);
  ASW_CHECK_ARG(workspace_bytes >= need, "istft: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0,
                "istft: z or workspace not 16-byte aligned");
  const double* tab = nullptr;
  if (int rc = device_tables(&tab)) return rc;
  hipStream_t s = asw::as_stream(stream);
  const Item item{0, 0, R, N, F, 0};
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double* frames = reinterpret_cast<double*>(ws + sizeof(Item));
  ASW_HIP(hipMemcpyAsync(ws, &item, sizeof item, hipMemcpyHostToDevice, s));      // pageable: taken before the call returns
  {
    asw::ProfScope prof(s, "istft_frames", 5.0 * NH * 10 * (double)R * F, (double)R * F * (NFFT * 8.0 + NB * 16.0));
    hipLaunchKernelGGL(istft_frames_kernel, dim3(F, R), dim3(THREADS), 0, s, reinterpret_cast<const double2*>(z), F, tab, frames);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "stft_overlap_add", 0.0, (double)R * N * 24.0);
  hipLaunchKernelGGL(overlap_add_kernel, dim3(asw::cdiv(N, HOP), R, 1), dim3(THREADS), 0, s, reinterpret_cast<const Item*>(ws),
                     frames, tab, N, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" size_t asw_oracle_masks_workspace_bytes(const int32_t* counts, const int32_t* lengths, int K) {
  Plan p;
  char msg[160];
  if (make_plan(counts, lengths, K, p, msg, sizeof msg)) {
    asw::set_error(ASW_ERR_ARG, "oracle_masks_workspace_bytes: %s", msg);
    return 0;
  }
  return p.total;
}

extern "C" int asw_oracle_masks(const float* mix, const float* ref, const int32_t* counts, const int32_t* lengths, int K, int stride,
                                int kind, double alpha, double theta, double* out, void* workspace, size_t workspace_bytes,
                                void* stream) {
  Plan p;
  char msg[160];
  if (make_plan(counts, lengths, K, p, msg, sizeof msg)) return asw::set_error(ASW_ERR_ARG, "oracle_masks: %s", msg);
  ASW_CHECK_ARG(kind == ASW_ORACLE_IRM || kind == ASW_ORACLE_IBM, "oracle_masks: kind = %d is neither IRM (0) nor IBM (1)", kind);
  ASW_CHECK_ARG(alpha == alpha && theta == theta, "oracle_masks: alpha or theta is not a number");
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(stride >= NFFT && stride <= MAX_T, "oracle_masks: stride = %d outside %d..%d", stride, NFFT, MAX_T);
  for (int k = 0; k < K; ++k)
    ASW_CHECK_ARG(lengths[k] <= stride, "oracle_masks: item %d: %d samples exceed the stride of %d", k, lengths[k], stride);
  ASW_CHECK_ARG(mix && workspace, "oracle_masks: null mix or workspace");
  ASW_CHECK_ARG((ref && out) || p.rows == 0, "oracle_masks: null pointer");
  ASW_CHECK_ARG(workspace_bytes >= p.total, "oracle_masks: workspace of %zu bytes too small, %zu needed", workspace_bytes, p.total);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "oracle_masks: workspace not 16-byte aligned");
  const long chunks = asw::cdiv(stride, HOP);
  ASW_CHECK_ARG((long)p.maxF * K <= MAX_GRID && chunks * p.maxS * K <= MAX_GRID,
                "oracle_masks: %d items of up to %d references and %d samples outgrow one launch", K, p.maxS, stride);
  if (p.rows == 0) return ASW_OK;
  const double* tab = nullptr;
  if (int rc = device_tables(&tab)) return rc;
  hipStream_t s = asw::as_stream(stream);

  std::vector<Item> hi(K);
  int64_t row0 = 0, slot0 = 0;
  for (int k = 0; k < K; ++k) {
    const int F = frames_of(lengths[k]);
    hi[k] = Item{row0, slot0, counts[k], lengths[k], F, 0};
    row0 += counts[k], slot0 += (int64_t)counts[k] * F;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const Item* di = reinterpret_cast<const Item*>(ws);
  double* frames = reinterpret_cast<double*>(ws + p.o_frames);
  ASW_HIP(hipMemcpyAsync(ws, hi.data(), p.tab_bytes, hipMemcpyHostToDevice, s));  // pageable: taken before the call returns
  const int ibm = kind == ASW_ORACLE_IBM;
  {
    const double ffts = (double)p.slots * (ibm ? 2.0 : 3.0) + (double)p.maxF * K;
    asw::ProfScope prof(s, ibm ? "oracle_frames_ibm" : "oracle_frames_irm", 5.0 * NH * 10 * ffts,
                        (double)p.slots * NFFT * (8.0 + (ibm ? 4.0 : 8.0)));
    hipLaunchKernelGGL(oracle_frames_kernel, dim3(p.maxF, K), dim3(THREADS), 0, s, mix, ref, di, stride, ibm, alpha, theta, tab,
                       frames);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "stft_overlap_add", 0.0, (double)p.rows * stride * 24.0);
  hipLaunchKernelGGL(overlap_add_kernel, dim3((unsigned)chunks, p.maxS, K), dim3(THREADS), 0, s, di, frames, tab, stride, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
