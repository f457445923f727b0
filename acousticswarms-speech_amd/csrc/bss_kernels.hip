// bss_kernels.hip -- BSS-eval SDR, SIR and SAR (the "mtifilt" decomposition of evalkit._project / evalkit.bss_eval_sdr /
// evalkit.bss_eval_sources) of a ragged batch of samples on the device, float64 throughout (include/asw_hip.h:
// asw_bss_eval_sources and its view asw_bss_eval_sdr; DESIGN.md sections 7j and 7p).
//
// Per item (S references, R estimate sets) the work is: direct correlations of every reference against every reference
// and every estimate (bss_corr, bss_fold), the block-Toeplitz Gram matrix of the S references and the S single-reference
// Toeplitz matrices (bss_gram), one blocked Cholesky over that whole ragged list of symmetric systems (bss_potrf,
// bss_trsm, bss_update per 64-wide step), forward and backward substitution of every right-hand side (bss_solve), the
// two projections as direct flen-tap FIRs with the energies of the decomposition (bss_project) and the ratios (bss_sdr).
// Matched mode scores estimate j against reference j; all-pairs mode every estimate against every reference, which adds
// single-reference right-hand sides (they are rows of corr already) and rows of the projection, nothing else.
// Every launch is a grid over list entries; workgroups hand nothing to each other inside a launch, there are no
// atomics, no cross-lane operations and no device-side asserts, and every sum has one fixed order.
#include "asw_common.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int NB = 64;                 // Cholesky tile
constexpr int TC = 1024;               // samples per correlation / projection chunk
constexpr int MAX_SPLIT = 8;           // partial sums per correlation (each a run of whole chunks)
constexpr int MAX_FLEN = 1024, MAX_S = 16, MAX_ORDER = 8192;
constexpr int MAX_T = 1 << 25;         // chunk index rides on grid.y
// a pivot must exceed this fraction of its row's original diagonal entry r_ii[0]: below it the factor has lost the
// digits the decomposition needs (and a duplicated reference leaves pivots of a few ulp of either sign, not zeros)
constexpr double PIVOT_GUARD = 0x1p-40;

struct Item {                          // one sample of the batch
  int64_t corr_off;                    // corr + corr_off: [(R + 1) S][S][flen], (b row, reference, lag)
  int64_t x_off;                       // xsol + x_off: x1 [rows of the item][flen], then (S > 1) xF [R S][S flen]
  int32_t n0, S, sys0, out0;           // first row, talkers, first system (S singles, then the full one when S > 1),
};                                     // first output column (n0 matched, the sum of the earlier S^2 all pairs)
struct System {
  int64_t g_off;                       // gram + g_off: order x order, row-major, lower triangle in use
  int32_t order, item, src, nt;        // src = the reference of a single system, -1 for the full one; nt = tiles
};
struct Pair { int32_t item, brow, i, pad; };        // b row (reference < S <= estimate S + r S + j) against reference i
struct Solve {                         // estimate row e = r S + e' of the item against the full system or that of reference j
  int64_t x_off;                       // xsol + x_off: the solution, order doubles
  int32_t item, e, full, j;            // j = -1 with the full system
};
struct Row { int32_t item, ej; };      // ej = e S + j: estimate row e of the item scored against its reference j

struct Plan {
  int K, R, T, flen, N, all_pairs, nw;                                   // nw: sums per row and chunk, 2 (SDR) or 5
  long P, nsys, nsolve, E, Q;                                            // E rows; Q = sum S^2
  int nchunk, nsplit, cps, nchunk_p, ntmax;
  size_t tab_bytes, o_items, o_sys, o_pairs, o_solves, o_rows;           // inside the table blob
  size_t o_part, o_corr, o_gram, o_x, o_proj, total;                     // byte offsets in the workspace
};

// null on success, else the refusal.  Sizes only: no pointer is looked at.
const char* make_plan(const int32_t* counts, int K, int R, int T, int flen, int all_pairs, int nw, Plan& p, char* msg,
                      size_t msg_len) {
  if (K < 0 || R < 1) { snprintf(msg, msg_len, "K = %d < 0 or R = %d < 1", K, R); return msg; }
  if (flen < 1 || flen > MAX_FLEN) { snprintf(msg, msg_len, "flen = %d outside 1..%d", flen, MAX_FLEN); return msg; }
  if (T < flen || T > MAX_T) { snprintf(msg, msg_len, "T = %d outside flen = %d .. %d", T, flen, MAX_T); return msg; }
  if (K > 0 && !counts) { snprintf(msg, msg_len, "null counts"); return msg; }
  p = Plan{};
  p.K = K, p.R = R, p.T = T, p.flen = flen, p.all_pairs = all_pairs, p.nw = nw;
  size_t gram = 0, x = 0;
  for (int k = 0; k < K; ++k) {
    const long S = counts[k];
    if (S < 0 || S > MAX_S) { snprintf(msg, msg_len, "counts[%d] = %ld outside 0..%d", k, S, MAX_S); return msg; }
    if (S * flen > MAX_ORDER) {
      snprintf(msg, msg_len, "item %d: %ld references of %d taps make a system of order %ld > %d", k, S, flen, S * flen, MAX_ORDER);
      return msg;
    }
    const long rows = (long)R * S * (all_pairs ? S : 1);                 // single-reference solves = rows of the projection
    p.N += (int)S;
    p.Q += S * S;
    p.E += rows;
    p.P += (long)(R + 1) * S * S;
    p.nsys += S > 1 ? S + 1 : S;
    p.nsolve += rows + (S > 1 ? (long)R * S : 0);
    gram += (size_t)S * flen * flen + (S > 1 ? (size_t)(S * flen) * (S * flen) : 0);
    x += (size_t)rows * flen + (S > 1 ? (size_t)R * S * S * flen : 0);
    const int nt = asw::cdiv(S * flen, NB);
    if (S > 0 && nt > p.ntmax) p.ntmax = nt;
  }
  if (p.P > (1L << 30) || p.nsolve > (1L << 30)) { snprintf(msg, msg_len, "R = %d sets of %d rows are too many", R, p.N); return msg; }
  p.nchunk = asw::cdiv(T, TC);
  const int split = p.nchunk < MAX_SPLIT ? p.nchunk : MAX_SPLIT;
  p.cps = asw::cdiv(p.nchunk, split);
  p.nsplit = asw::cdiv(p.nchunk, p.cps);
  p.nchunk_p = asw::cdiv((long)T + flen - 1, TC);
  size_t o = 0;
  p.o_items = o, o += (size_t)K * sizeof(Item);
  p.o_sys = o, o += (size_t)p.nsys * sizeof(System);
  p.o_pairs = o, o += (size_t)p.P * sizeof(Pair);
  p.o_solves = o, o += (size_t)p.nsolve * sizeof(Solve);
  p.o_rows = o, o += (size_t)p.E * sizeof(Row);
  p.tab_bytes = o;
  p.o_part = o, o += (size_t)p.P * p.nsplit * flen * sizeof(double);
  p.o_corr = o, o += (size_t)p.P * flen * sizeof(double);
  p.o_gram = o, o += gram * sizeof(double);
  p.o_x = o, o += x * sizeof(double);
  p.o_proj = o, o += (size_t)p.E * p.nchunk_p * nw * sizeof(double);
  p.total = o;
  return nullptr;
}

__device__ __forceinline__ const float* b_row(const Item& it, int brow, const float* ref, const float* est, int N, int T) {
  if (brow < it.S) return ref + (size_t)(it.n0 + brow) * T;
  const int e = brow - it.S;                                             // r S + j
  return est + ((size_t)(e / it.S) * N + it.n0 + e % it.S) * T;
}

// ---- 1. correlations: part[pair][split][p] = sum over the split's samples t of a[t - p] * b[t], p = 0 .. flen - 1
__global__ __launch_bounds__(256) void bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                       const Item* __restrict__ items, const Pair* __restrict__ pairs, int N,
                                                       int T, int flen, int cps, int nchunk, int nsplit,
                                                       double* __restrict__ part) {
  __shared__ double bs[TC];
  __shared__ double as[TC + MAX_FLEN - 1];                               // a[t0 - (flen - 1) .. t0 + TC)
  const int tid = threadIdx.x;
  const Pair pr = pairs[blockIdx.x];
  const Item it = items[pr.item];
  const float* a = ref + (size_t)(it.n0 + pr.i) * T;
  const float* b = b_row(it, pr.brow, ref, est, N, T);
  const int nq = (flen + 255) / 256;
  int back[4];                                                           // flen - 1 - lag, clamped into the window
  for (int q = 0; q < 4; ++q) {
    const int p = tid + 256 * q;
    back[q] = flen - 1 - (p < flen ? p : flen - 1);
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int c0 = blockIdx.y * cps, c1 = c0 + cps < nchunk ? c0 + cps : nchunk;
  for (int c = c0; c < c1; ++c) {
    const int t0 = c * TC, len = T - t0 < TC ? T - t0 : TC;
    __syncthreads();
    for (int u = tid; u < TC; u += 256) bs[u] = u < len ? (double)b[t0 + u] : 0.0;
    for (int u = tid; u < TC + flen - 1; u += 256) {
      const int t = t0 - (flen - 1) + u;
      as[u] = t >= 0 && t < T ? (double)a[t] : 0.0;
    }
    __syncthreads();
    for (int u = 0; u < len; ++u) {
      const double bv = bs[u];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nq) acc[q] += as[u + back[q]] * bv;
    }
  }
  double* out = part + ((size_t)blockIdx.x * nsplit + blockIdx.y) * flen;
  for (int q = 0; q < nq; ++q)
    if (tid + 256 * q < flen) out[tid + 256 * q] = acc[q];
}

// corr[pair][p] = the splits of part[pair] folded left to right
__global__ __launch_bounds__(256) void bss_fold_kernel(const double* __restrict__ part, int flen, int nsplit,
                                                       double* __restrict__ corr) {
  const double* in = part + (size_t)blockIdx.x * nsplit * flen;
  for (int p = threadIdx.x; p < flen; p += 256) {
    double s = in[p];
    for (int k = 1; k < nsplit; ++k) s += in[(size_t)k * flen + p];
    corr[(size_t)blockIdx.x * flen + p] = s;
  }
}

// (row, col) of entry idx of a lower triangle stored row after row; the same for every thread of a workgroup
__device__ __forceinline__ void tri_decode(int idx, int& row, int& col) {
  int r = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > idx) --r;
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  row = r, col = idx - r * (r + 1) / 2;
}

// G[(i, a)][(j, b)] = sum_u ref_i[u - a] ref_j[u - b]: lag a - b of (b row j, reference i), or lag b - a of (i, j)
__device__ __forceinline__ double gram_entry(const double* __restrict__ c, int S, int flen, int i, int a, int j, int b) {
  return a >= b ? c[((size_t)j * S + i) * flen + (a - b)] : c[((size_t)i * S + j) * flen + (b - a)];
}

// ---- 2. Gram matrices: every tile on or below the diagonal of every system
__global__ __launch_bounds__(256) void bss_gram_kernel(const Item* __restrict__ items, const System* __restrict__ systems,
                                                       const double* __restrict__ corr, int flen, double* __restrict__ gram) {
  const System sy = systems[blockIdx.x];
  int ti, tl;
  tri_decode(blockIdx.y, ti, tl);
  if (ti >= sy.nt) return;
  const Item it = items[sy.item];
  const double* c = corr + it.corr_off;
  double* G = gram + sy.g_off;
  const int M = sy.order;
  for (int idx = threadIdx.x; idx < NB * NB; idx += 256) {
    const int m = ti * NB + idx / NB, n = tl * NB + idx % NB;
    if (m >= M || n >= M) continue;
    const double v = sy.src >= 0 ? gram_entry(c, it.S, flen, sy.src, m, sy.src, n)
                                 : gram_entry(c, it.S, flen, m / flen, m % flen, n / flen, n % flen);
    G[(size_t)m * M + n] = v;
  }
}

// ---- 3. blocked Cholesky, step j.  Diagonal tile in LDS; rows past the order behave as rows of the identity.
__global__ __launch_bounds__(256) void bss_potrf_kernel(const Item* __restrict__ items, const System* __restrict__ systems,
                                                        const double* __restrict__ corr, int flen, int j,
                                                        double* __restrict__ gram, int32_t* __restrict__ status) {
  __shared__ double Ts[NB][NB + 1];
  __shared__ double dg[NB], scale[NB];
  const System sy = systems[blockIdx.x];
  if (j >= sy.nt) return;
  const Item it = items[sy.item];
  const int M = sy.order, tid = threadIdx.x, base = j * NB;
  const int nr = M - base < NB ? M - base : NB;
  double* G = gram + sy.g_off;
  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int r = idx / NB, q = idx % NB;
    double v = r == q ? 1.0 : 0.0;
    if (r < nr && q <= r) v = G[(size_t)(base + r) * M + base + q];
    Ts[r][q] = v;
  }
  if (tid < NB) {
    double s = 0.0;                                                      // identity rows: 1 > 0 always passes
    if (tid < nr) {
      const int i = sy.src >= 0 ? sy.src : (base + tid) / flen;
      s = corr[it.corr_off + ((size_t)i * it.S + i) * flen] * PIVOT_GUARD;
    }
    scale[tid] = s;
  }
  const int r = tid & (NB - 1), qg = tid >> 6;
  for (int c = 0; c < NB; ++c) {
    __syncthreads();
    double piv = Ts[c][c];
    if (!(piv > scale[c])) {                                             // NaN included
      piv = 1.0;
      if (tid == 0) status[sy.item] = 1;
    }
    const double l = sqrt(piv);
    if (tid == 0) dg[c] = l;
    if (tid < NB && tid > c) Ts[tid][c] = Ts[tid][c] / l;
    __syncthreads();
    const double lr = Ts[r][c];
    for (int q = c + 1 + qg; q <= r; q += 4) Ts[r][q] -= lr * Ts[q][c];
  }
  __syncthreads();
  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int rr = idx / NB, q = idx % NB;
    if (rr < nr && q <= rr) G[(size_t)(base + rr) * M + base + q] = q == rr ? dg[rr] : Ts[rr][q];
  }
}

// panel: X = A[i][j] <- X L_jj^-T, a row per lane.  Tile j is whole whenever a tile lies below it.
__global__ __launch_bounds__(64) void bss_trsm_kernel(const System* __restrict__ systems, int j, double* __restrict__ gram) {
  __shared__ double Ls[NB][NB];
  __shared__ double Xs[NB][NB + 1];
  const System sy = systems[blockIdx.x];
  const int i = j + 1 + blockIdx.y;
  if (i >= sy.nt) return;
  const int M = sy.order, tid = threadIdx.x;
  const int nr = M - i * NB < NB ? M - i * NB : NB;
  double* G = gram + sy.g_off;
  for (int idx = tid; idx < NB * NB; idx += 64) {
    const int r = idx / NB, q = idx % NB;
    Ls[r][q] = q <= r ? G[(size_t)(j * NB + r) * M + j * NB + q] : 0.0;
    Xs[r][q] = r < nr ? G[(size_t)(i * NB + r) * M + j * NB + q] : 0.0;
  }
  __syncthreads();
  for (int q = 0; q < NB; ++q) {
    double s = Xs[tid][q];
    for (int c = 0; c < q; ++c) s -= Xs[tid][c] * Ls[q][c];
    Xs[tid][q] = s / Ls[q][q];
  }
  __syncthreads();
  for (int idx = tid; idx < NB * NB; idx += 64) {
    const int r = idx / NB, q = idx % NB;
    if (r < nr) G[(size_t)(i * NB + r) * M + j * NB + q] = Xs[r][q];
  }
}

// trailing update: A[ti][tl] -= A[ti][j] A[tl][j]^T for j < tl <= ti, a 4 x 4 patch per thread
__global__ __launch_bounds__(256) void bss_update_kernel(const System* __restrict__ systems, int j, double* __restrict__ gram) {
  constexpr int KH = 32, LD = NB + 2;                                    // half the k range at a time, k-major
  __shared__ __attribute__((aligned(16))) double As[KH][LD];
  __shared__ __attribute__((aligned(16))) double Bs[KH][LD];
  const System sy = systems[blockIdx.x];
  int a, b;
  tri_decode(blockIdx.y, a, b);
  const int ti = j + 1 + a, tl = j + 1 + b;
  if (ti >= sy.nt) return;
  const int M = sy.order, tid = threadIdx.x;
  double* G = gram + sy.g_off;
  const int ty = tid >> 4, tx = tid & 15;
  double acc[4][4] = {};
  for (int h = 0; h < NB / KH; ++h) {
    __syncthreads();
    for (int idx = tid; idx < NB * KH; idx += 256) {
      const int r = idx / KH, k = idx % KH;
      const int ra = ti * NB + r, rb = tl * NB + r, col = j * NB + h * KH + k;
      As[k][r] = ra < M ? G[(size_t)ra * M + col] : 0.0;
      Bs[k][r] = rb < M ? G[(size_t)rb * M + col] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < KH; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) av[u] = As[k][ty * 4 + u], bv[u] = Bs[k][tx * 4 + u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += av[u] * bv[v];
    }
  }
  for (int u = 0; u < 4; ++u)
    for (int v = 0; v < 4; ++v) {
      const int m = ti * NB + ty * 4 + u, n = tl * NB + tx * 4 + v;
      if (m < M && n < M && n <= m) G[(size_t)m * M + n] -= acc[u][v];
    }
}

// ---- 4. L y = d, L^T x = y for one right-hand side; y and x live in LDS, a 64-wide tile of L at a time
__global__ __launch_bounds__(256) void bss_solve_kernel(const Item* __restrict__ items, const System* __restrict__ systems,
                                                        const Solve* __restrict__ solves, const double* __restrict__ corr,
                                                        const double* __restrict__ gram, int flen, double* __restrict__ xsol) {
  __shared__ double yl[MAX_ORDER];
  __shared__ double Lt[NB][NB + 1];
  __shared__ double red[NB][NB + 1];
  __shared__ double accv[NB];
  __shared__ double pv;
  const Solve so = solves[blockIdx.x];
  const Item it = items[so.item];
  const int S = it.S, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const System sy = systems[it.sys0 + (so.full ? S : so.j)];
  const int M = sy.order, nt = sy.nt;
  const double* G = gram + sy.g_off;
  // d: the lags of estimate row e against every reference (full) or against reference j (single)
  const double* d = corr + it.corr_off + ((size_t)(S + so.e) * S + (so.full ? 0 : so.j)) * flen;
  for (int t = 0; t < nt; ++t) {                                         // forward
    const int base = t * NB, nr = M - base < NB ? M - base : NB;
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 256) {
      const int r = idx / NB, q = idx % NB;
      double v = r == q ? 1.0 : 0.0;
      if (r < nr && q <= r) v = G[(size_t)(base + r) * M + base + q];
      Lt[r][q] = v;
    }
    for (int rr = 0; rr < 16; ++rr) {                                    // rows of the tile against everything solved so far
      const int r = w * 16 + rr;
      double s = 0.0;
      if (r < nr)
        for (int c = lane; c < base; c += 64) s += G[(size_t)(base + r) * M + c] * yl[c];
      red[r][lane] = s;
    }
    __syncthreads();
    if (tid < NB) {
      double s = 0.0;
      for (int c = 0; c < NB; ++c) s += red[tid][c];
      accv[tid] = tid < nr ? d[base + tid] - s : 0.0;
    }
    for (int c = 0; c < NB; ++c) {
      __syncthreads();
      if (tid == 0) pv = accv[c] / Lt[c][c], yl[base + c] = pv;
      __syncthreads();
      if (tid < NB && tid > c) accv[tid] -= Lt[tid][c] * pv;
    }
  }
  for (int t = nt - 1; t >= 0; --t) {                                    // backward
    const int base = t * NB, nr = M - base < NB ? M - base : NB;
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 256) {
      const int r = idx / NB, q = idx % NB;
      double v = r == q ? 1.0 : 0.0;
      if (r < nr && q <= r) v = G[(size_t)(base + r) * M + base + q];
      Lt[r][q] = v;
    }
    {
      double s = 0.0;                                                    // column base + lane over the rows below the tile
      for (int r = base + NB + w; r < M; r += 4) s += G[(size_t)r * M + base + lane] * yl[r];
      red[w][lane] = s;
    }
    __syncthreads();
    if (tid < NB) accv[tid] = tid < nr ? yl[base + tid] - ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) : 0.0;
    for (int c = NB - 1; c >= 0; --c) {
      __syncthreads();
      if (tid == 0) {
        pv = accv[c] / Lt[c][c];
        if (c < nr) yl[base + c] = pv;
      }
      __syncthreads();
      if (tid < c) accv[tid] -= Lt[c][tid] * pv;
    }
  }
  __syncthreads();
  double* out = xsol + so.x_off;
  for (int m = tid; m < M; m += 256) out[m] = yl[m];
}

// ---- 5. projections and energies of one row (estimate row e against reference j) over one chunk of the T + flen - 1
// output samples: sp1 = x1 * ref_j, spF = sum_i xF_i * ref_i (S = 1: spF is sp1), then the decomposition as
// evalkit.bss_eval_sdr forms it.  FULL adds the three sums SIR and SAR need to the two of the SDR.  In all-pairs mode the
// S rows of an estimate each form its spF again.
template <bool FULL>
__global__ __launch_bounds__(256) void bss_project_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                          const Item* __restrict__ items, const Row* __restrict__ rows,
                                                          const double* __restrict__ xsol, int N, int R, int T, int flen,
                                                          int all_pairs, int nchunk_p, double* __restrict__ proj) {
  constexpr int NW = FULL ? 5 : 2;
  __shared__ double rs[TC + MAX_FLEN - 1];                               // ref_i[t0 - (flen - 1) .. t0 + TC)
  __shared__ double cf[MAX_FLEN], c1[MAX_FLEN];
  __shared__ double red[NW][256];
  const int tid = threadIdx.x;
  const Row rw = rows[blockIdx.x];
  const Item it = items[rw.item];
  const int S = it.S, e = rw.ej / S, j = rw.ej % S, t0 = blockIdx.y * TC;
  const int nrow = R * S * (all_pairs ? S : 1);                          // x1 of the item: one per row
  const double* x1 = xsol + it.x_off + (size_t)(all_pairs ? rw.ej : e) * flen;
  const double* xF = xsol + it.x_off + (size_t)nrow * flen + (size_t)e * S * flen;
  double spF[4] = {0.0, 0.0, 0.0, 0.0}, sp1[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < S; ++i) {
    const float* a = ref + (size_t)(it.n0 + i) * T;
    __syncthreads();
    for (int u = tid; u < TC + flen - 1; u += 256) {
      const int t = t0 - (flen - 1) + u;
      rs[u] = t >= 0 && t < T ? (double)a[t] : 0.0;
    }
    for (int p = tid; p < flen; p += 256) {
      if (S > 1) cf[p] = xF[(size_t)i * flen + p];
      if (i == j) c1[p] = x1[p];
    }
    __syncthreads();
    if (S > 1)
      for (int p = 0; p < flen; ++p) {
        const double cv = cf[p];
#pragma unroll
        for (int q = 0; q < 4; ++q) spF[q] += cv * rs[tid + 256 * q + flen - 1 - p];
      }
    if (i == j)
      for (int p = 0; p < flen; ++p) {
        const double cv = c1[p];
#pragma unroll
        for (int q = 0; q < 4; ++q) sp1[q] += cv * rs[tid + 256 * q + flen - 1 - p];
      }
  }
  const float* rj = ref + (size_t)(it.n0 + j) * T;
  const float* ev = est + ((size_t)(e / S) * N + it.n0 + e % S) * T;
  double num = 0.0, den = 0.0, si = 0.0, sn = 0.0, sa = 0.0;
  for (int q = 0; q < 4; ++q) {
    const int t = t0 + tid + 256 * q;
    if (t >= T + flen - 1) continue;
    const double s_true = t < T ? (double)rj[t] : 0.0;
    const double e_spat = sp1[q] - s_true;
    const double e_interf = (S > 1 ? spF[q] : sp1[q]) - s_true - e_spat;
    double e_artif = -s_true - e_spat - e_interf;
    if (t < T) e_artif += (double)ev[t];
    const double u = s_true + e_spat, v = e_interf + e_artif;
    num += u * u, den += v * v;
    if constexpr (FULL) {
      const double w = u + e_interf;
      si += e_interf * e_interf, sn += w * w, sa += e_artif * e_artif;
    }
  }
  red[0][tid] = num, red[1][tid] = den;
  if constexpr (FULL) red[2][tid] = si, red[3][tid] = sn, red[4][tid] = sa;
  for (int s = 128; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s)
#pragma unroll
      for (int k = 0; k < NW; ++k) red[k][tid] += red[k][tid + s];
  }
  if (tid == 0) {
    double* out = proj + ((size_t)blockIdx.x * nchunk_p + blockIdx.y) * NW;
#pragma unroll
    for (int k = 0; k < NW; ++k) out[k] = red[k][0];
  }
}

__device__ __forceinline__ double ratio_db(double num, double den) { return den == 0.0 ? HUGE_VAL : 10.0 * log10(num / den); }

// the ratios of every row, the chunks folded left to right, +inf when a denominator is 0: sdr = sum u^2 / sum (e_i + e_a)^2
// and with FULL sir = sum u^2 / sum e_i^2, sar = sum (u + e_i)^2 / sum e_a^2.  Row (e, j) of an item lands in column
// out0 + j (matched) or out0 + e' S + j (all pairs) of set r's line of ncol entries, e = r S + e'.
template <bool FULL>
__global__ __launch_bounds__(256) void bss_sdr_kernel(const Item* __restrict__ items, const Row* __restrict__ rows,
                                                      const double* __restrict__ proj, long E, long ncol, int all_pairs,
                                                      int nchunk_p, double* __restrict__ sdr, double* __restrict__ sir,
                                                      double* __restrict__ sar) {
  constexpr int NW = FULL ? 5 : 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= E) return;
  const Row rw = rows[q];
  const Item it = items[rw.item];
  const double* in = proj + (size_t)q * nchunk_p * NW;
  double s[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) s[k] = in[k];
  for (int c = 1; c < nchunk_p; ++c)
#pragma unroll
    for (int k = 0; k < NW; ++k) s[k] += in[NW * c + k];
  const int e = rw.ej / it.S, j = rw.ej % it.S;
  const size_t o = (size_t)(e / it.S) * ncol + it.out0 + (all_pairs ? (e % it.S) * it.S + j : j);
  sdr[o] = ratio_db(s[0], s[1]);
  if constexpr (FULL) sir[o] = ratio_db(s[0], s[2]), sar[o] = ratio_db(s[3], s[4]);
}

// the general call: matched or all pairs, one output (sir and sar null) or three
int run(const char* who, const float* ref, const float* est, const int32_t* counts, int K, int R, int T, int flen, int all_pairs,
        double* sdr, double* sir, double* sar, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  Plan p;
  char msg[160];
  ASW_CHECK_ARG(all_pairs == 0 || all_pairs == 1, "%s: all_pairs = %d is neither 0 nor 1", who, all_pairs);
  ASW_CHECK_ARG((sir == nullptr) == (sar == nullptr), "%s: sir and sar go together: one of them alone is null", who);
  const bool full = sir != nullptr;
  if (make_plan(counts, K, R, T, flen, all_pairs, full ? 5 : 2, p, msg, sizeof msg)) return asw::set_error(ASW_ERR_ARG, "%s: %s", who, msg);
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(status, "%s: null status", who);
  hipStream_t s = asw::as_stream(stream);
  if (p.N > 0) {
    ASW_CHECK_ARG(ref && est && sdr && workspace, "%s: null pointer", who);
    ASW_CHECK_ARG(workspace_bytes >= p.total, "%s: workspace of %zu bytes too small, %zu needed", who, workspace_bytes, p.total);
    ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace not 8-byte aligned", who);
  }
  ASW_HIP(hipMemsetAsync(status, 0, (size_t)K * sizeof(int32_t), s));
  if (p.N == 0) return ASW_OK;

  // the lists every launch is a grid over
  std::vector<unsigned char> blob(p.tab_bytes);
  Item* hi = reinterpret_cast<Item*>(blob.data() + p.o_items);
  System* hs = reinterpret_cast<System*>(blob.data() + p.o_sys);
  Pair* hp = reinterpret_cast<Pair*>(blob.data() + p.o_pairs);
  Solve* hv = reinterpret_cast<Solve*>(blob.data() + p.o_solves);
  Row* hr = reinterpret_cast<Row*>(blob.data() + p.o_rows);
  long n0 = 0, q0 = 0, np = 0, ns = 0, nv = 0, nr = 0;
  int64_t g = 0, x = 0;
  for (int k = 0; k < K; ++k) {
    const int S = counts[k], E = R * S;
    const int64_t rows = (int64_t)E * (all_pairs ? S : 1);
    hi[k] = Item{(int64_t)np * flen, x, (int32_t)n0, S, (int32_t)ns, (int32_t)(all_pairs ? q0 : n0)};
    for (int b = 0; b < (R + 1) * S; ++b)
      for (int i = 0; i < S; ++i) hp[np++] = Pair{k, b, i, 0};
    for (int i = 0; i < S; ++i) {
      hs[ns++] = System{g, flen, k, i, asw::cdiv(flen, NB)};
      g += (int64_t)flen * flen;
    }
    if (S > 1) {
      hs[ns++] = System{g, S * flen, k, -1, asw::cdiv(S * flen, NB)};
      g += (int64_t)S * flen * S * flen;
    }
    for (int e = 0; e < E; ++e) {
      for (int j = all_pairs ? 0 : e % S; j < (all_pairs ? S : e % S + 1); ++j) {
        const int64_t row = all_pairs ? (int64_t)e * S + j : e;          // of the item: where its x1 lies
        hv[nv++] = Solve{x + row * flen, k, e, 0, j};
        hr[nr++] = Row{k, e * S + j};
      }
      if (S > 1) hv[nv++] = Solve{x + rows * flen + (int64_t)e * S * flen, k, e, 1, -1};
    }
    x += rows * flen + (S > 1 ? (int64_t)E * S * flen : 0);
    n0 += S, q0 += S * S;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const Item* di = reinterpret_cast<const Item*>(ws + p.o_items);
  const System* ds = reinterpret_cast<const System*>(ws + p.o_sys);
  const Pair* dp = reinterpret_cast<const Pair*>(ws + p.o_pairs);
  const Solve* dv = reinterpret_cast<const Solve*>(ws + p.o_solves);
  const Row* dr = reinterpret_cast<const Row*>(ws + p.o_rows);
  double* part = reinterpret_cast<double*>(ws + p.o_part);
  double* corr = reinterpret_cast<double*>(ws + p.o_corr);
  double* gram = reinterpret_cast<double*>(ws + p.o_gram);
  double* xsol = reinterpret_cast<double*>(ws + p.o_x);
  double* proj = reinterpret_cast<double*>(ws + p.o_proj);
  // pageable source: the runtime has taken the table before the call returns
  ASW_HIP(hipMemcpyAsync(ws, blob.data(), p.tab_bytes, hipMemcpyHostToDevice, s));
  const int N = p.N;
  {
    asw::ProfScope prof(s, "bss_corr", 2.0 * (double)p.P * flen * T, 0.0);
    hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)p.P, (unsigned)p.nsplit), dim3(256), 0, s, ref, est, di, dp, N, T, flen,
                       p.cps, p.nchunk, p.nsplit, part);
    ASW_LAUNCH_CHECK();
  }
  {
    asw::ProfScope prof(s, "bss_fold", 0.0, (double)p.P * (p.nsplit + 1) * flen * 8);
    hipLaunchKernelGGL(bss_fold_kernel, dim3((unsigned)p.P), dim3(256), 0, s, part, flen, p.nsplit, corr);
    ASW_LAUNCH_CHECK();
  }
  const int nt = p.ntmax;
  {
    asw::ProfScope prof(s, "bss_gram", 0.0, (double)g * 8);
    hipLaunchKernelGGL(bss_gram_kernel, dim3((unsigned)p.nsys, (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, di, ds, corr, flen,
                       gram);
    ASW_LAUNCH_CHECK();
  }
  for (int j = 0; j < nt; ++j) {
    const int rem = nt - j - 1;
    {
      asw::ProfScope prof(s, "bss_potrf", 0.0, 0.0);
      hipLaunchKernelGGL(bss_potrf_kernel, dim3((unsigned)p.nsys), dim3(256), 0, s, di, ds, corr, flen, j, gram, status);
      ASW_LAUNCH_CHECK();
    }
    if (rem == 0) break;
    {
      asw::ProfScope prof(s, "bss_trsm", 0.0, 0.0);
      hipLaunchKernelGGL(bss_trsm_kernel, dim3((unsigned)p.nsys, (unsigned)rem), dim3(64), 0, s, ds, j, gram);
      ASW_LAUNCH_CHECK();
    }
    asw::ProfScope prof(s, "bss_update", 0.0, 0.0);
    hipLaunchKernelGGL(bss_update_kernel, dim3((unsigned)p.nsys, (unsigned)(rem * (rem + 1) / 2)), dim3(256), 0, s, ds, j, gram);
    ASW_LAUNCH_CHECK();
  }
  {
    asw::ProfScope prof(s, "bss_solve", 0.0, 0.0);
    hipLaunchKernelGGL(bss_solve_kernel, dim3((unsigned)p.nsolve), dim3(256), 0, s, di, ds, dv, corr, gram, flen, xsol);
    ASW_LAUNCH_CHECK();
  }
  const dim3 gp((unsigned)p.E, (unsigned)p.nchunk_p), gr((unsigned)asw::cdiv(p.E, 256));
  const long ncol = all_pairs ? p.Q : (long)N;
  {
    asw::ProfScope prof(s, "bss_project", 0.0, 0.0);
    if (full)
      hipLaunchKernelGGL(bss_project_kernel<true>, gp, dim3(256), 0, s, ref, est, di, dr, xsol, N, R, T, flen, all_pairs,
                         p.nchunk_p, proj);
    else
      hipLaunchKernelGGL(bss_project_kernel<false>, gp, dim3(256), 0, s, ref, est, di, dr, xsol, N, R, T, flen, all_pairs,
                         p.nchunk_p, proj);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "bss_sdr", 0.0, 0.0);
  if (full)
    hipLaunchKernelGGL(bss_sdr_kernel<true>, gr, dim3(256), 0, s, di, dr, proj, p.E, ncol, all_pairs, p.nchunk_p, sdr, sir, sar);
  else
    hipLaunchKernelGGL(bss_sdr_kernel<false>, gr, dim3(256), 0, s, di, dr, proj, p.E, ncol, all_pairs, p.nchunk_p, sdr, sir, sar);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

size_t plan_bytes(const char* who, const int32_t* counts, int K, int R, int T, int flen, int all_pairs, int nw) {
  Plan p;
  char msg[160];
  if (all_pairs != 0 && all_pairs != 1) {
    asw::set_error(ASW_ERR_ARG, "%s: all_pairs = %d is neither 0 nor 1", who, all_pairs);
    return 0;
  }
  if (make_plan(counts, K, R, T, flen, all_pairs, nw, p, msg, sizeof msg)) {
    asw::set_error(ASW_ERR_ARG, "%s: %s", who, msg);
    return 0;
  }
  return p.total;
}

}  // namespace

// the size with sir and sar wanted; a call without them needs the 3/5 smaller energy partials and accepts this size too
extern "C" size_t asw_bss_eval_sources_workspace_bytes(const int32_t* counts, int K, int R, int T, int flen, int all_pairs) {
  return plan_bytes("bss_eval_sources_workspace_bytes", counts, K, R, T, flen, all_pairs, 5);
}

extern "C" int asw_bss_eval_sources(const float* ref, const float* est, const int32_t* counts, int K, int R, int T, int flen,
                                    int all_pairs, double* sdr, double* sir, double* sar, int32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return run("bss_eval_sources", ref, est, counts, K, R, T, flen, all_pairs, sdr, sir, sar, status, workspace, workspace_bytes,
             stream);
}

// the SDR alone, matched: the general call with all_pairs = 0 and neither sir nor sar
extern "C" size_t asw_bss_eval_sdr_workspace_bytes(const int32_t* counts, int K, int R, int T, int flen) {
  return plan_bytes("bss_eval_sdr_workspace_bytes", counts, K, R, T, flen, 0, 2);
}

extern "C" int asw_bss_eval_sdr(const float* ref, const float* est, const int32_t* counts, int K, int R, int T, int flen,
                                double* sdr, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  return run("bss_eval_sdr", ref, est, counts, K, R, T, flen, 0, sdr, nullptr, nullptr, status, workspace, workspace_bytes, stream);
}
