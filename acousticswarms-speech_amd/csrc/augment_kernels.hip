// augment_kernels.hip -- the training batches of train_data.py on the device: power-law noise from
// a counter-based generator (asw_colored_noise), the rolled and perturbed mixtures (asw_train_batch) and the per-row
// terms of the training losses (asw_train_losses).  All arithmetic is float64.  The house rules of room_kernels.hip hold:
// grids over host-built tables, no atomics, one writer per address, every sum in a fixed order, so two runs give
// identical bytes.
//
// asw_colored_noise is an inverse real transform of any length T: row r is irfft(s_r, n = T) / sigma with s_r the scaled
// Philox normals of train_data.philox_normals.  Two real rows share one complex transform: rows 2p and 2p + 1 go in as
// X = X_a + i X_b (each the Hermitian extension of its one-sided spectrum) and come out as the real and the imaginary part,
// which serves odd and even T alike and needs no merge step.  The T-point transform is Bluestein's:
//     y[t] = w[t] sum_k (X[k] w[k]) conj(w[t - k]),    w[n] = exp(i pi n^2 / T),
// a circular convolution of length L = 1024 R >= 2 T - 1 (R a power of two), and n^2 is reduced modulo 2 T in 64-bit
// integers before any trigonometry.  The L-point transform is a four-step over the array seen as R rows of 1024:
//   cols_fwd   R-point Stockham transforms down the columns (a workgroup takes TC adjacent columns, so that a row of its
//              tile is TC * 16 contiguous bytes), then the twiddles exp(-2 pi i n2 k1 / L) from sincospi of an exact
//              argument;
//   rows       fft1024 along each row.  Bin k1 + R k2 of the spectrum lands at [k1][k2]; the chirp's spectrum is
//              prepared once per call by the same two kernels and so lies in the same order, and the product, the inverse
//              fft1024 and the conjugate twiddles follow in the same launch with the row still in LDS;
//   cols_inv   the inverse R-point transforms, the product with w[t] and the scale, and the two real rows are written.
// No transpose anywhere.  Rows are processed in passes of at most max_rows_per_pass, which bounds the workspace; the
// pairing of rows does not depend on the pass size, so neither do the bytes.
#include "asw_common.h"
#include "fft1024.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {

using namespace asw::fft;              // NH (1024), THREADS (256), Lds, fft1024, fill_twiddles

constexpr int MAX_T = 524288, MAX_ROWS = 1 << 20, MAX_GRID_YZ = 65535;
constexpr int COL_ELEMS = 2048;        // complex values of a column tile: R * TC; re/im ping-pong pairs of it are 64 KB
constexpr size_t DEFAULT_PASS_BYTES = size_t(256) << 20;
constexpr uint32_t STREAM_PINK = 0, STREAM_WHITE = 1;

// ---- Philox4x32-10 and the normals (train_data.philox_normals) --------------------------------------------------------
struct Normals { double z0, z1; };

__device__ __forceinline__ double words_to_uniform(uint32_t hi, uint32_t lo) {      // (2 m + 1) / 2^53, m the top 52 bits
  const uint64_t m = ((uint64_t)hi << 20) | (lo >> 12);
  return (double)(2 * m + 1) * 0x1p-53;
}

__device__ __forceinline__ Normals philox_normals(uint64_t key, uint32_t row, uint32_t index, uint32_t stream) {
  uint32_t c0 = index, c1 = row, c2 = stream, c3 = 0, k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  const double u1 = words_to_uniform(c0, c1), u2 = words_to_uniform(c2, c3);
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  return Normals{r * c, r * s};
}

// ---- asw_colored_noise ----------------------------------------------------------------------------------------------------
struct NoiseArgs {
  const int64_t* row_key;              // [rows]
  const int32_t* row_id;               // [rows]
  const double* tw;                    // fft1024.h's table
  double2* chirp;                      // [L]: the chirp's spectrum, at [k1][k2]
  double2* work;                       // [pairs per pass][L]
  double* out;                         // [rows][T]
  double exponent, norm;               // norm = 1 / (L T sigma)
  int rows, T, L, R, TC, log_tc, pair0;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// exp(sign i pi n^2 / T)
__device__ __forceinline__ double2 chirp_value(int64_t n, int T, double sign) {
  const uint64_t r = (uint64_t)(n * n) % (uint64_t)(2 * (int64_t)T);
  double s, c;
  sincospi((double)r / (double)T, &s, &c);
  return make_double2(c, sign * s);
}

// exp(sign 2 pi i (n2 k1) / L), L a power of two: the argument 2 (n2 k1 mod L) / L is exact
__device__ __forceinline__ double2 step_twiddle(int n2, int k1, int L, double sign) {
  const int64_t q = ((int64_t)n2 * k1) & (L - 1);
  double s, c;
  sincospi(2.0 * (double)q / (double)L, &s, &c);
  return make_double2(c, sign * s);
}

// bin n (0 <= n < T) of the Hermitian extension of row r's one-sided spectrum
__device__ __forceinline__ double2 spectrum_bin(const NoiseArgs& a, int r, int n) {
  const int T = a.T, k = n <= T / 2 ? n : T - n;
  const Normals z = philox_normals((uint64_t)a.row_key[r], (uint32_t)a.row_id[r], (uint32_t)k, STREAM_PINK);
  const double f = (double)(k > 0 ? k : 1) / (double)T;                 // the cutoff: bin 0 takes bin 1's frequency
  const double scale = a.exponent == 1.0 ? 1.0 / sqrt(f) : pow(f, -0.5 * a.exponent);
  const bool real_bin = k == 0 || 2 * k == T;
  const double re = z.z0 * scale * (real_bin ? 1.4142135623730951 : 1.0);
  const double im = real_bin ? 0.0 : z.z1 * scale;
  return make_double2(re, n <= T / 2 ? im : -im);
}

struct ColLds {
  double re[2][COL_ELEMS], im[2][COL_ELEMS];
};

// R-point Stockham transforms of the TC columns of a tile, element (j, c) at j * TC + c of buffer 0; returns the buffer
// the result is in.  The twiddle exp(-+ 2 pi i k / (2 ns)) is entry k * (1024 / ns) of the 2048-point table.
template <bool INV>
__device__ __forceinline__ int column_fft(ColLds& S, const double* __restrict__ tw, int R, int log_tc, int tid) {
  const int TC = 1 << log_tc, half = R >> 1;
  int src = 0;
#pragma unroll 1
  for (int ns = 1; ns < R; ns <<= 1) {
    __syncthreads();
    const int step = NH / ns;
    for (int i = tid; i < half * TC; i += THREADS) {
      const int j = i >> log_tc, c = i & (TC - 1), k = j & (ns - 1);
      const double tc = tw[2 * (k * step)], ts0 = tw[2 * (k * step) + 1];
      const double ts = INV ? -ts0 : ts0;
      const int ia = j * TC + c, ix = (j + half) * TC + c;
      const double ar = S.re[src][ia], ai = S.im[src][ia], xr = S.re[src][ix], xi = S.im[src][ix];
      const double br = xr * tc - xi * ts, bi = xr * ts + xi * tc;
      const int j0 = ((j - k) << 1) + k, o0 = j0 * TC + c, o1 = (j0 + ns) * TC + c;
      S.re[src ^ 1][o0] = ar + br, S.im[src ^ 1][o0] = ai + bi;
      S.re[src ^ 1][o1] = ar - br, S.im[src ^ 1][o1] = ai - bi;
    }
    src ^= 1;
  }
  __syncthreads();
  return src;
}

// grid (1024 / TC, pairs of this pass; 1 for the chirp).  CHIRP: the input is b[n] = conj(w[m]) at n = m and n = L - m for
// m < T, zero between; otherwise (X_a[n] + i X_b[n]) w[n] for n < T and zero beyond.
template <bool CHIRP>
__global__ __launch_bounds__(THREADS) void cols_fwd_kernel(NoiseArgs a) {
  __shared__ ColLds S;
  const int tid = threadIdx.x, TC = a.TC, n2_0 = blockIdx.x * TC, T = a.T, L = a.L;
  const int ra = 2 * (a.pair0 + (int)blockIdx.y), rb = ra + 1;
  for (int i = tid; i < a.R * TC; i += THREADS) {
    const int n1 = i >> a.log_tc, c = i & (TC - 1);
    const int64_t n = (int64_t)n1 * NH + n2_0 + c;
    double2 v = make_double2(0.0, 0.0);
    if (CHIRP) {
      const int64_t m = n < T ? n : L - n;
      if (m < T) v = chirp_value(m, T, -1.0);
    } else if (n < T) {
      double2 x = spectrum_bin(a, ra, (int)n);
      if (rb < a.rows) {
        const double2 xb = spectrum_bin(a, rb, (int)n);
        x.x -= xb.y, x.y += xb.x;
      }
      v = cmul(x, chirp_value(n, T, 1.0));
    }
    S.re[0][i] = v.x, S.im[0][i] = v.y;
  }
  const int buf = column_fft<false>(S, a.tw, a.R, a.log_tc, tid);
  double2* dst = CHIRP ? a.chirp : a.work + (int64_t)blockIdx.y * L;
  for (int i = tid; i < a.R * TC; i += THREADS) {
    const int k1 = i >> a.log_tc, n2 = n2_0 + (i & (TC - 1));
    dst[(int64_t)k1 * NH + n2] = cmul(make_double2(S.re[buf][i], S.im[buf][i]), step_twiddle(n2, k1, L, -1.0));
  }
}

// grid (R, pairs of this pass; 1 for the chirp): row k1 through fft1024; CHIRP keeps the spectrum, otherwise the product
// with the chirp's, the inverse fft1024 and the conjugate twiddles follow, in place
template <bool CHIRP>
__global__ __launch_bounds__(THREADS) void rows_kernel(NoiseArgs a) {
  __shared__ Lds S;
  const int tid = threadIdx.x, k1 = blockIdx.x;
  double2* row = (CHIRP ? a.chirp : a.work + (int64_t)blockIdx.y * a.L) + (int64_t)k1 * NH;
  for (int j = tid; j < NH; j += THREADS) {
    const double2 v = row[j];
    S.re[0][j] = v.x, S.im[0][j] = v.y;
  }
  fft1024<false>(S, a.tw, tid);
  if (CHIRP) {
    for (int j = tid; j < NH; j += THREADS) row[j] = make_double2(S.re[0][j], S.im[0][j]);
    return;
  }
  const double2* b = a.chirp + (int64_t)k1 * NH;
  for (int j = tid; j < NH; j += THREADS) {
    const double2 v = cmul(make_double2(S.re[0][j], S.im[0][j]), b[j]);
    S.re[0][j] = v.x, S.im[0][j] = v.y;
  }
  fft1024<true>(S, a.tw, tid);
  for (int j = tid; j < NH; j += THREADS)
    row[j] = cmul(make_double2(S.re[0][j], S.im[0][j]), step_twiddle(j, k1, a.L, 1.0));
}

// grid (1024 / TC, pairs of this pass): the inverse column transforms, y[t] = w[t] c[t] norm, real part to row 2p and
// imaginary part to row 2p + 1
__global__ __launch_bounds__(THREADS) void cols_inv_kernel(NoiseArgs a) {
  __shared__ ColLds S;
  const int tid = threadIdx.x, TC = a.TC, n2_0 = blockIdx.x * TC, T = a.T;
  const int ra = 2 * (a.pair0 + (int)blockIdx.y), rb = ra + 1;
  const double2* src = a.work + (int64_t)blockIdx.y * a.L;
  for (int i = tid; i < a.R * TC; i += THREADS) {
    const int k1 = i >> a.log_tc, n2 = n2_0 + (i & (TC - 1));
    const double2 v = src[(int64_t)k1 * NH + n2];
    S.re[0][i] = v.x, S.im[0][i] = v.y;
  }
  const int buf = column_fft<true>(S, a.tw, a.R, a.log_tc, tid);
  for (int i = tid; i < a.R * TC; i += THREADS) {
    const int n1 = i >> a.log_tc;
    const int64_t n = (int64_t)n1 * NH + n2_0 + (i & (TC - 1));
    if (n >= T) continue;
    const double2 y = cmul(make_double2(S.re[buf][i], S.im[buf][i]), chirp_value(n, T, 1.0));
    a.out[(int64_t)ra * T + n] = y.x * a.norm;
    if (rb < a.rows) a.out[(int64_t)rb * T + n] = y.y * a.norm;
  }
}

struct NoisePlan {
  int L, R, TC, log_tc, pairs_per_pass;
  size_t o_key, o_id, o_chirp, o_work, total;
};

const char* noise_plan(int rows, int T, int max_rows_per_pass, NoisePlan& p) {
  if (rows < 0 || rows > MAX_ROWS) return "rows outside 0..2^20";
  if (T < 2 || T > MAX_T) return "T outside 2..524288";
  if (max_rows_per_pass < 0 || max_rows_per_pass == 1) return "max_rows_per_pass must be 0 (the default) or at least 2";
  int L = NH;
  while (L < 2 * T - 1) L <<= 1;
  p.L = L, p.R = L / NH;
  p.TC = COL_ELEMS / p.R < NH ? COL_ELEMS / p.R : NH;
  p.log_tc = 0;
  while ((1 << p.log_tc) < p.TC) ++p.log_tc;
  const int pairs = (rows + 1) / 2;
  long ppp = max_rows_per_pass ? max_rows_per_pass / 2 : (long)(DEFAULT_PASS_BYTES / (sizeof(double2) * (size_t)L));
  if (ppp < 1) ppp = 1;
  if (ppp > MAX_GRID_YZ) ppp = MAX_GRID_YZ;
  if (ppp > pairs) ppp = pairs > 0 ? pairs : 1;
  p.pairs_per_pass = (int)ppp;
  auto up = [](size_t v) { return (v + 15) & ~size_t(15); };
  p.o_key = up(2 * NH * sizeof(double));                      // the twiddle table comes first
  p.o_id = up(p.o_key + (size_t)rows * sizeof(int64_t));
  p.o_chirp = up(p.o_id + (size_t)rows * sizeof(int32_t));
  p.o_work = p.o_chirp + (size_t)L * sizeof(double2);
  p.total = p.o_work + (size_t)p.pairs_per_pass * L * sizeof(double2);
  return nullptr;
}

// the theoretical standard deviation of powerlaw_psd_gaussian, summed in bin order
double noise_sigma(int T, double exponent) {
  const int K = T / 2 + 1;
  double sum = 0.0;
  for (int k = 1; k < K; ++k) {
    double w = std::pow((double)k / (double)T, -0.5 * exponent);
    if (k == K - 1) w *= (1 + T % 2) / 2.0;
    sum += w * w;
  }
  return 2.0 * std::sqrt(sum) / T;
}

// ---- asw_train_batch ----------------------------------------------------------------------------------------------------
struct ItemRec {
  double pink_level, white_level;
  uint64_t white_key;
  int32_t mix, count;
};

// grid (ceil(T / 256), S_max * M, items): one sample each
template <typename OUT>
__global__ __launch_bounds__(THREADS) void train_batch_kernel(const float* __restrict__ mix, const ItemRec* __restrict__ items,
                                                              const int32_t* __restrict__ shifts, const double* __restrict__ pink,
                                                              int M, int T, OUT* __restrict__ out) {
  const int t = blockIdx.x * THREADS + threadIdx.x, c = blockIdx.y, i = blockIdx.z, C = gridDim.y;
  if (t >= T) return;
  const ItemRec it = items[i];
  const int s = c / M, m = c - s * M;
  double x = 0.0;
  if (s < it.count) {
    const int64_t sh = shifts[(int64_t)i * C + c];
    if (sh >= -(int64_t)T && sh <= (int64_t)T) {
      const int64_t q = ((int64_t)t - sh + T) % T;                       // t - sh lies in [-T, 2T)
      x = (double)mix[((int64_t)it.mix * M + m) * T + q];
    }
  }
  const int64_t o = ((int64_t)i * C + c) * T + t;
  // x + white_level w + pink_level p, each product and sum rounded on its own, as the statement's numpy does
  if (it.white_level != 0.0) x = __dadd_rn(x, __dmul_rn(it.white_level, philox_normals(it.white_key, (uint32_t)c, (uint32_t)t, STREAM_WHITE).z0));
  if (it.pink_level != 0.0) x = __dadd_rn(x, __dmul_rn(it.pink_level, pink[o]));
  out[o] = (OUT)x;
}

// ---- asw_train_losses ---------------------------------------------------------------------------------------------------
struct RedLds {
  double v[4][THREADS];
};

// the sums (or maxima) of the threads' NV values, to all threads, by a fixed tree
template <int NV, bool MAXLAST>
__device__ __forceinline__ void block_reduce(RedLds& S, double (&v)[NV], int tid) {
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) S.v[q][tid] = v[q];
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double x = S.v[q][tid], y = S.v[q][tid + w];
        S.v[q][tid] = (MAXLAST && q == NV - 1) ? (x > y ? x : y) : x + y;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = S.v[q][0];
}

// grid (rows): out[row] = (mean |e - g|, -SNR, -SI-SDR, max |g|) of train_data.row_losses_f64.  Three passes over the
// row: the means; the centred energies and the dot; the residual against the scaled target.
__global__ __launch_bounds__(THREADS) void train_losses_kernel(const float* __restrict__ est, const float* __restrict__ gt, int T,
                                                               double* __restrict__ out) {
  __shared__ RedLds S;
  const int tid = threadIdx.x;
  const float* e = est + (int64_t)blockIdx.x * T;
  const float* g = gt + (int64_t)blockIdx.x * T;
  const double EPS = 1e-8;
  double a[4] = {0.0, 0.0, 0.0, 0.0};                              // sum e, sum g, sum |e - g|, max |g|
  for (int t = tid; t < T; t += THREADS) {
    const double ev = e[t], gv = g[t];
    a[0] += ev, a[1] += gv, a[2] += fabs(ev - gv);
    a[3] = fabs(gv) > a[3] ? fabs(gv) : a[3];
  }
  block_reduce<4, true>(S, a, tid);
  const double me = a[0] / T, mg = a[1] / T;
  double b[3] = {0.0, 0.0, 0.0};                                   // sum gc^2, sum (ec - gc)^2, sum ec gc
  for (int t = tid; t < T; t += THREADS) {
    const double ec = (double)e[t] - me, gc = (double)g[t] - mg, d = ec - gc;
    b[0] += gc * gc, b[1] += d * d, b[2] += ec * gc;
  }
  block_reduce<3, false>(S, b, tid);
  const double alpha = b[2] / (b[0] + EPS);
  double c[2] = {0.0, 0.0};                                        // sum (alpha gc)^2, sum (ec - alpha gc)^2
  for (int t = tid; t < T; t += THREADS) {
    const double ec = (double)e[t] - me, st = alpha * ((double)g[t] - mg), d = ec - st;
    c[0] += st * st, c[1] += d * d;
  }
  block_reduce<2, false>(S, c, tid);
  if (tid == 0) {
    double* o = out + (int64_t)blockIdx.x * 4;
    o[0] = a[2] / T;
    o[1] = -10.0 * log10(b[0] / (b[1] + EPS) + EPS);
    o[2] = -10.0 * log10(c[0] / (c[1] + EPS) + EPS);
    o[3] = a[3];
  }
}

}  // namespace

extern "C" size_t asw_colored_noise_workspace_bytes(int rows, int T, int max_rows_per_pass) {
  NoisePlan p;
  if (const char* msg = noise_plan(rows, T, max_rows_per_pass, p)) {
    asw::set_error(ASW_ERR_ARG, "colored_noise_workspace_bytes: %s", msg);
    return 0;
  }
  return p.total;
}

extern "C" int asw_colored_noise(const int64_t* row_key, const int32_t* row_id, int rows, int T, double exponent,
                                 int max_rows_per_pass, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  NoisePlan p;
  if (const char* msg = noise_plan(rows, T, max_rows_per_pass, p)) return asw::set_error(ASW_ERR_ARG, "colored_noise: %s", msg);
  ASW_CHECK_ARG(std::isfinite(exponent) && exponent >= 0.0 && exponent <= 8.0, "colored_noise: exponent = %g outside 0..8", exponent);
  if (rows == 0) return ASW_OK;
  ASW_CHECK_ARG(row_key && row_id && out && workspace, "colored_noise: null pointer");
  ASW_CHECK_ARG(workspace_bytes >= p.total, "colored_noise: workspace of %zu bytes too small, %zu needed", workspace_bytes, p.total);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "colored_noise: workspace not 16-byte aligned");
  hipStream_t s = asw::as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  std::vector<double> tw(2 * NH);
  fill_twiddles(tw.data());
  ASW_HIP(hipMemcpyAsync(ws, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, s));   // pageable: taken before the call returns
  ASW_HIP(hipMemcpyAsync(ws + p.o_key, row_key, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, s));
  ASW_HIP(hipMemcpyAsync(ws + p.o_id, row_id, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
  NoiseArgs a;
  a.row_key = reinterpret_cast<const int64_t*>(ws + p.o_key);
  a.row_id = reinterpret_cast<const int32_t*>(ws + p.o_id);
  a.tw = reinterpret_cast<const double*>(ws);
  a.chirp = reinterpret_cast<double2*>(ws + p.o_chirp);
  a.work = reinterpret_cast<double2*>(ws + p.o_work);
  a.out = out;
  a.exponent = exponent;
  a.norm = 1.0 / ((double)p.L * (double)T * noise_sigma(T, exponent));
  a.rows = rows, a.T = T, a.L = p.L, a.R = p.R, a.TC = p.TC, a.log_tc = p.log_tc, a.pair0 = 0;
  const int tiles = NH / p.TC, pairs = (rows + 1) / 2;
  const double fft_flops = 5.0 * p.L * std::log2((double)p.L);
  {
    asw::ProfScope prof(s, "noise_chirp", fft_flops, 48.0 * p.L);
    hipLaunchKernelGGL(cols_fwd_kernel<true>, dim3(tiles, 1), dim3(THREADS), 0, s, a);
    ASW_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_kernel<true>, dim3(p.R, 1), dim3(THREADS), 0, s, a);
    ASW_LAUNCH_CHECK();
  }
  for (int p0 = 0; p0 < pairs; p0 += p.pairs_per_pass) {
    const int n = pairs - p0 < p.pairs_per_pass ? pairs - p0 : p.pairs_per_pass;
    a.pair0 = p0;
    {
      asw::ProfScope prof(s, "noise_spectrum_cols", 0.5 * fft_flops * n, 16.0 * p.L * n);
      hipLaunchKernelGGL(cols_fwd_kernel<false>, dim3(tiles, n), dim3(THREADS), 0, s, a);
      ASW_LAUNCH_CHECK();
    }
    {
      asw::ProfScope prof(s, "noise_rows_product", fft_flops * n, 48.0 * p.L * n);
      hipLaunchKernelGGL(rows_kernel<false>, dim3(p.R, n), dim3(THREADS), 0, s, a);
      ASW_LAUNCH_CHECK();
    }
    asw::ProfScope prof(s, "noise_cols_inv", 0.5 * fft_flops * n, (16.0 * p.L + 16.0 * T) * n);
    hipLaunchKernelGGL(cols_inv_kernel, dim3(tiles, n), dim3(THREADS), 0, s, a);
    ASW_LAUNCH_CHECK();
  }
  return ASW_OK;
}

extern "C" size_t asw_train_batch_workspace_bytes(int items, int S_max, int M) {
  if (items < 0 || items > MAX_GRID_YZ || S_max < 1 || M < 1 || (long)S_max * M > MAX_GRID_YZ) {
    asw::set_error(ASW_ERR_ARG, "train_batch_workspace_bytes: items = %d outside 0..%d or S_max * M = %d * %d outside 1..%d", items,
                   MAX_GRID_YZ, S_max, M, MAX_GRID_YZ);
    return 0;
  }
  return 16 + (size_t)items * sizeof(ItemRec) + (size_t)items * S_max * M * sizeof(int32_t);
}

extern "C" int asw_train_batch(const float* mix, int K, int M, int T, int items, int S_max, const int32_t* item_mix, const int32_t* shifts,
                               const int32_t* counts, const double* pink_level, const double* white_level, const int64_t* white_key,
                               const double* pink, void* out, int out_f64, void* workspace, size_t workspace_bytes, void* stream) {
  ASW_CHECK_ARG(items >= 0 && items <= MAX_GRID_YZ, "train_batch: items = %d outside 0..%d", items, MAX_GRID_YZ);
  ASW_CHECK_ARG(K >= 0 && M >= 1 && S_max >= 1 && (long)S_max * M <= MAX_GRID_YZ, "train_batch: K = %d, M = %d or S_max = %d out of range", K, M,
                S_max);
  ASW_CHECK_ARG(T >= 1 && T <= (1 << 25), "train_batch: T = %d outside 1..2^25", T);
  if (items == 0) return ASW_OK;
  ASW_CHECK_ARG(item_mix && shifts && counts && pink_level && white_level && white_key, "train_batch: null host table");
  ASW_CHECK_ARG(out && workspace && (mix || K == 0), "train_batch: null pointer");
  const size_t rec_bytes = (size_t)items * sizeof(ItemRec), sh_bytes = (size_t)items * S_max * M * sizeof(int32_t);
  ASW_CHECK_ARG(workspace_bytes >= rec_bytes + sh_bytes, "train_batch: workspace of %zu bytes too small, %zu needed", workspace_bytes,
                rec_bytes + sh_bytes);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "train_batch: workspace not 8-byte aligned");
  std::vector<ItemRec> rec(items);
  for (int i = 0; i < items; ++i) {
    ASW_CHECK_ARG(counts[i] >= 0 && counts[i] <= S_max, "train_batch: counts[%d] = %d outside 0..%d", i, counts[i], S_max);
    ASW_CHECK_ARG(counts[i] == 0 || (item_mix[i] >= 0 && item_mix[i] < K), "train_batch: item_mix[%d] = %d outside 0..%d", i, item_mix[i], K - 1);
    ASW_CHECK_ARG(std::isfinite(pink_level[i]) && std::isfinite(white_level[i]), "train_batch: level of item %d not finite", i);
    ASW_CHECK_ARG(pink || pink_level[i] == 0.0, "train_batch: pink_level[%d] = %g without the pink rows", i, pink_level[i]);
    rec[i] = ItemRec{pink_level[i], white_level[i], (uint64_t)white_key[i], item_mix[i], counts[i]};
  }
  hipStream_t s = asw::as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  ASW_HIP(hipMemcpyAsync(ws, rec.data(), rec_bytes, hipMemcpyHostToDevice, s));                   // pageable: taken before the call returns
  ASW_HIP(hipMemcpyAsync(ws + rec_bytes, shifts, sh_bytes, hipMemcpyHostToDevice, s));
  const ItemRec* d_rec = reinterpret_cast<const ItemRec*>(ws);
  const int32_t* d_sh = reinterpret_cast<const int32_t*>(ws + rec_bytes);
  const dim3 grid(asw::cdiv(T, THREADS), S_max * M, items);
  const double n = (double)items * S_max * M * T;
  asw::ProfScope prof(s, "train_batch", 0.0, n * (4.0 + 8.0 + (out_f64 ? 8.0 : 4.0)));
  if (out_f64)
    hipLaunchKernelGGL(train_batch_kernel<double>, grid, dim3(THREADS), 0, s, mix, d_rec, d_sh, pink, M, T, static_cast<double*>(out));
  else
    hipLaunchKernelGGL(train_batch_kernel<float>, grid, dim3(THREADS), 0, s, mix, d_rec, d_sh, pink, M, T, static_cast<float*>(out));
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_train_losses(const float* est, const float* gt, int N, int T, double* out, void* stream) {
  ASW_CHECK_ARG(N >= 0 && N <= (1 << 24), "train_losses: N = %d outside 0..2^24", N);
  ASW_CHECK_ARG(T >= 1 && T <= (1 << 25), "train_losses: T = %d outside 1..2^25", T);
  if (N == 0) return ASW_OK;
  ASW_CHECK_ARG(est && gt && out, "train_losses: null pointer");
  hipStream_t s = asw::as_stream(stream);
  asw::ProfScope prof(s, "train_losses", 0.0, 24.0 * N * (double)T);
  hipLaunchKernelGGL(train_losses_kernel, dim3(N), dim3(THREADS), 0, s, est, gt, T, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
