// voice_kernels.hip -- corpus voices on the device: the polyphase resampler and the silence trim of voiceprep.py
// (resample_poly_f64, trim_f64), equal to those float64 statements bit for bit.  Both entry points take a ragged batch
// through host-built row tables that are validated before the first launch; no atomics, one writer per address, every
// output element written, so two calls give identical bytes.  The file is compiled with -ffp-contract=off and every
// product and sum of the statements is written with __dmul_rn / __dadd_rn: no fused multiply-add may replace them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/asw_hip.h"
#include "asw_common.h"

namespace {

// one row of a call: where the input row lies in the packed x, and (resampler only) the window of its output
struct VoiceRow {
  int64_t off, win_begin;
  int32_t len, win_len;
};

constexpr int RS_THREADS = 1024;         // outputs per workgroup of the resampler
constexpr int64_t MAX_SAMPLES = (int64_t)1 << 40;

// voice_resample_kernel: a workgroup per (row, 1024 outputs of its window).  The filter table is staged once into dynamic
// LDS (a thread's taps h[phase + j * up] are scattered over it; the input samples x[q - j] of neighbouring outputs are
// neighbours in memory and come through the caches).  Each thread sums one output serially in ascending j; the terms
// whose sample lies outside the row are left out by the loop bounds.
template <typename OutT>
__global__ __launch_bounds__(RS_THREADS) void voice_resample_kernel(const float* __restrict__ x, const VoiceRow* __restrict__ rows,
                                                                     const double* __restrict__ h, int hlen, int up, int down,
                                                                     int T_out, OutT* __restrict__ out) {
  extern __shared__ double hs[];
  for (int i = threadIdx.x; i < hlen; i += RS_THREADS) hs[i] = h[i];
  __syncthreads();
  const int t = blockIdx.x * RS_THREADS + threadIdx.x;
  if (t >= T_out) return;                                       // no barrier below
  const VoiceRow r = rows[blockIdx.y];
  const int64_t N = r.len, n_out = (N * up + down - 1) / down, n = r.win_begin + t;
  double acc = 0.0;
  if (t < r.win_len && n < n_out) {
    const float* __restrict__ xr = x + r.off;
    const int64_t m = n * down + (hlen - 1) / 2, q = m / up;
    const int phase = (int)(m - q * up);
    const int64_t j_first = q - (N - 1) > 0 ? q - (N - 1) : 0;  // sample index q - j < N
    int64_t j_last = (hlen - 1 - phase) / up;                   // tap index phase + j * up <= hlen - 1
    j_last = q < j_last ? q : j_last;                           // sample index q - j >= 0
    for (int64_t j = j_first; j <= j_last; ++j)
      acc = __dadd_rn(acc, __dmul_rn(hs[phase + (int)j * up], (double)xr[q - j]));
  }
  out[(int64_t)blockIdx.y * T_out + t] = (OutT)acc;
}

// voice_block_sums_kernel: one wavefront per 512-sample block of a row.  Lane l sums the squares of samples 8l .. 8l+7 left
// to right (samples past the row count as 0; a float32 squared is exact in double), then the statement's butterfly
// p[l] += p[l+s], s = 32 .. 1; lane 0 holds the block sum.  Rows are packed at any offset, so the loads are scalar.
__global__ __launch_bounds__(256) void voice_block_sums_kernel(const float* __restrict__ x, const VoiceRow* __restrict__ rows,
                                                               int nblk_max, double* __restrict__ bsum) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const VoiceRow r = rows[blockIdx.y];
  const int T = r.len, nblk = (T + 511) / 512;
  if (j >= nblk) return;                                        // whole wavefronts leave; no barrier below
  const float* __restrict__ row = x + r.off;
  const int t0 = j * 512 + lane * 8;
  double p = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double v = t0 + i < T ? (double)row[t0 + i] : 0.0;
    const double q = __dmul_rn(v, v);
    p = i == 0 ? q : __dadd_rn(p, q);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) p = __dadd_rn(p, __shfl_down(p, s, 64));   // lanes < s hold the statement's p[:s]
  if (lane == 0) bsum[(int64_t)blockIdx.y * nblk_max + j] = p;
}

// ms[f] of the statement from one row's block sums; blocks outside [0, nblk) are 0
__device__ __forceinline__ double trim_frame_ms(const double* __restrict__ b, int nblk, int f) {
  const double b0 = (f >= 2 && f - 2 < nblk) ? b[f - 2] : 0.0, b1 = (f >= 1 && f - 1 < nblk) ? b[f - 1] : 0.0;
  const double b2 = f < nblk ? b[f] : 0.0, b3 = f + 1 < nblk ? b[f + 1] : 0.0;
  return __dadd_rn(__dadd_rn(__dadd_rn(b0, b1), b2), b3) / 2048.0;
}

// the statement's _span_sum over the 256 partial sums of a workgroup: p[:s] + p[s:2s], s = 128 .. 1; all threads call
__device__ __forceinline__ double span_butterfly(double partial, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                                              // the previous use of red is over
  red[tid] = partial;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = __dadd_rn(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// voice_trim_kernel: one workgroup per row.  The frame values and their maximum (exact in any order), the first and the
// last non-silent frame (a minimum and a maximum, exact in any order), then the two passes of the variance over the kept
// span: thread t adds elements t, t + 256, ... in ascending order and the partial sums go through the butterfly.
__global__ __launch_bounds__(256) void voice_trim_kernel(const float* __restrict__ x, const VoiceRow* __restrict__ rows,
                                                         const double* __restrict__ bsum, int nblk_max, double thr,
                                                         int* __restrict__ bounds, double* __restrict__ stats) {
  constexpr double A2 = 1e-10;
  __shared__ double red[256];
  __shared__ int ired[2][256];
  const int tid = threadIdx.x;
  const VoiceRow r = rows[blockIdx.x];
  const int T = r.len, nblk = (T + 511) / 512, nfr = 1 + T / 512;
  const double* __restrict__ b = bsum + (int64_t)blockIdx.x * nblk_max;

  double peak = 0.0;                                            // ms >= 0
  for (int f = tid; f < nfr; f += 256) {
    const double v = trim_frame_ms(b, nblk, f);
    peak = v > peak ? v : peak;
  }
  red[tid] = peak;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  peak = red[0];
  const double level = __dmul_rn(thr, A2 > peak ? A2 : peak);

  int first = INT32_MAX, last = -1;
  for (int f = tid; f < nfr; f += 256) {
    const double v = trim_frame_ms(b, nblk, f);
    if ((A2 > v ? A2 : v) > level) {
      first = f < first ? f : first;
      last = f;                                                 // ascending f
    }
  }
  ired[0][tid] = first;
  ired[1][tid] = last;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      ired[0][tid] = ired[0][tid + s] < ired[0][tid] ? ired[0][tid + s] : ired[0][tid];
      ired[1][tid] = ired[1][tid + s] > ired[1][tid] ? ired[1][tid + s] : ired[1][tid];
    }
    __syncthreads();
  }
  first = ired[0][0];
  last = ired[1][0];
  // the peak frame is non-silent whatever thr <= 1 is; with thr > 1 (top_db < 0) or NaN samples none may be: (0, 0) then
  int begin = 0, end = 0;
  if (last >= 0) {
    const int64_t e = (int64_t)(last + 1) * 512;
    begin = first * 512;
    end = (int)(e < T ? e : T);
    if (begin > end) begin = end;
  }
  const int n = end - begin;
  const float* __restrict__ row = x + r.off + begin;
  double acc = 0.0;
  for (int i = tid; i < n; i += 256) acc = __dadd_rn(acc, (double)row[i]);
  const double total = span_butterfly(acc, red);
  double var = 0.0;
  if (n > 0) {                                                  // uniform over the workgroup
    const double mean = __ddiv_rn(total, (double)n);
    acc = 0.0;
    for (int i = tid; i < n; i += 256) {
      const double d = __dsub_rn((double)row[i], mean);
      acc = __dadd_rn(acc, __dmul_rn(d, d));
    }
    var = __ddiv_rn(span_butterfly(acc, red), (double)n);
  }
  if (tid == 0) {
    bounds[2 * blockIdx.x] = begin;
    bounds[2 * blockIdx.x + 1] = end;
    stats[2 * blockIdx.x] = peak;
    stats[2 * blockIdx.x + 1] = var;
  }
}

int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the row tables of both entry points, checked and packed; `what` names the entry point in the message
int pack_rows(const char* what, int64_t x_len, const int64_t* row_offset, const int32_t* row_len, int n, int64_t max_len,
              const int64_t* win_begin, const int32_t* win_len, int T_out, std::vector<VoiceRow>& rows) {
  ASW_CHECK_ARG(n == 0 || (row_offset && row_len), "%s: null row table", what);
  rows.resize(n);
  for (int r = 0; r < n; ++r) {
    ASW_CHECK_ARG(row_len[r] >= 0 && row_len[r] <= max_len, "%s: row_len[%d] = %d outside 0..%lld", what, r, row_len[r],
                  (long long)max_len);
    ASW_CHECK_ARG(row_offset[r] >= 0 && row_offset[r] <= x_len - row_len[r], "%s: row %d = [%lld, +%d) leaves x of %lld samples",
                  what, r, (long long)row_offset[r], row_len[r], (long long)x_len);
    rows[r] = VoiceRow{row_offset[r], 0, row_len[r], 0};
    if (win_begin) {
      ASW_CHECK_ARG(win_begin[r] >= 0 && win_begin[r] <= MAX_SAMPLES, "%s: win_begin[%d] = %lld outside 0..2^40", what, r,
                    (long long)win_begin[r]);
      ASW_CHECK_ARG(win_len[r] >= 0 && win_len[r] <= T_out, "%s: win_len[%d] = %d outside 0..T_out = %d", what, r, win_len[r],
                    T_out);
      rows[r].win_begin = win_begin[r];
      rows[r].win_len = win_len[r];
    }
  }
  return ASW_OK;
}

}  // namespace

extern "C" size_t asw_voice_resample_workspace_bytes(int n) {
  if (n < 0 || n > 65535) {
    asw::set_error(ASW_ERR_ARG, "voice_resample_workspace_bytes: n = %d outside 0..65535", n);
    return 0;
  }
  return (size_t)(n > 0 ? n : 1) * sizeof(VoiceRow);
}

extern "C" int asw_voice_resample(const float* x, int64_t x_len, const int64_t* row_offset, const int32_t* row_len, int n, int up,
                                  int down, const double* h, int h_len, const int64_t* win_begin, const int32_t* win_len,
                                  int T_out, void* out, int out_f64, void* workspace, size_t workspace_bytes, void* stream) {
  ASW_CHECK_ARG(n >= 0 && n <= 65535, "voice_resample: n = %d outside 0..65535", n);
  ASW_CHECK_ARG(up >= 1 && down >= 1, "voice_resample: up = %d and down = %d must be positive", up, down);
  const int g = gcd_int(up, down);
  up /= g;
  down /= g;
  const int big = up > down ? up : down;
  ASW_CHECK_ARG(big <= ASW_VOICE_MAX_RATIO, "voice_resample: the ratio %d/%d is beyond max(up, down) <= %d", up, down,
                ASW_VOICE_MAX_RATIO);
  const int want_h = big == 1 ? 1 : 20 * big + 1;
  ASW_CHECK_ARG(h_len == want_h, "voice_resample: the filter of %d/%d has %d taps, got %d", up, down, want_h, h_len);
  ASW_CHECK_ARG(T_out >= 1 && T_out <= (1 << 30), "voice_resample: T_out = %d outside 1..2^30", T_out);
  ASW_CHECK_ARG(x_len >= 0 && x_len <= MAX_SAMPLES, "voice_resample: x_len = %lld outside 0..2^40", (long long)x_len);
  ASW_CHECK_ARG(n == 0 || (win_begin && win_len), "voice_resample: null window table");
  std::vector<VoiceRow> rows;
  if (int rc = pack_rows("voice_resample", x_len, row_offset, row_len, n, INT32_MAX, win_begin, win_len, T_out, rows)) return rc;
  if (n == 0) return ASW_OK;
  ASW_CHECK_ARG(x && h && out && workspace, "voice_resample: null pointer");
  const size_t need = (size_t)n * sizeof(VoiceRow);
  ASW_CHECK_ARG(workspace_bytes >= need, "voice_resample: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "voice_resample: workspace not 8-byte aligned");
  hipStream_t s = asw::as_stream(stream);
  const size_t lds = (size_t)h_len * sizeof(double);            // 102,408 bytes at the limit: beyond the default 64 KB
  static asw::SmemAttr attr[2];
  const void* kern = out_f64 ? reinterpret_cast<const void*>(voice_resample_kernel<double>)
                             : reinterpret_cast<const void*>(voice_resample_kernel<float>);
  if (int rc = attr[out_f64 ? 1 : 0].ensure(kern, (size_t)(20 * ASW_VOICE_MAX_RATIO + 1) * sizeof(double))) return rc;
  ASW_HIP(hipMemcpyAsync(workspace, rows.data(), need, hipMemcpyHostToDevice, s));   // pageable: taken before the call returns
  const VoiceRow* drows = static_cast<const VoiceRow*>(workspace);
  const dim3 grid(asw::cdiv(T_out, RS_THREADS), n);
  const double taps = (double)(h_len - 1) / up + 1.0;
  asw::ProfScope prof(s, "voice_resample", 2.0 * taps * (double)n * T_out, (double)n * T_out * (out_f64 ? 8.0 : 4.0) + (double)x_len * 4.0);
  if (out_f64)
    hipLaunchKernelGGL(voice_resample_kernel<double>, grid, dim3(RS_THREADS), lds, s, x, drows, h, h_len, up, down, T_out,
                       static_cast<double*>(out));
  else
    hipLaunchKernelGGL(voice_resample_kernel<float>, grid, dim3(RS_THREADS), lds, s, x, drows, h, h_len, up, down, T_out,
                       static_cast<float*>(out));
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" size_t asw_voice_trim_workspace_bytes(int n, int max_len) {
  if (n < 0 || n > 65535 || max_len < 0) {
    asw::set_error(ASW_ERR_ARG, "voice_trim_workspace_bytes: n = %d outside 0..65535 or max_len = %d < 0", n, max_len);
    return 0;
  }
  const size_t nblk = (size_t)asw::cdiv(max_len, 512);
  return (size_t)(n > 0 ? n : 1) * (sizeof(VoiceRow) + (nblk > 0 ? nblk : 1) * sizeof(double));
}

extern "C" int asw_voice_trim(const float* x, int64_t x_len, const int64_t* row_offset, const int32_t* row_len, int n, int max_len,
                              double thr, int32_t* bounds, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  ASW_CHECK_ARG(n >= 0 && n <= 65535, "voice_trim: n = %d outside 0..65535", n);
  ASW_CHECK_ARG(max_len >= 0, "voice_trim: max_len = %d < 0", max_len);
  ASW_CHECK_ARG(x_len >= 0 && x_len <= MAX_SAMPLES, "voice_trim: x_len = %lld outside 0..2^40", (long long)x_len);
  ASW_CHECK_ARG(thr == thr, "voice_trim: the threshold is not a number");
  std::vector<VoiceRow> rows;
  if (int rc = pack_rows("voice_trim", x_len, row_offset, row_len, n, max_len, nullptr, nullptr, 0, rows)) return rc;
  if (n == 0) return ASW_OK;
  ASW_CHECK_ARG(x && bounds && stats && workspace, "voice_trim: null pointer");
  const int nblk_raw = asw::cdiv(max_len, 512), nblk_max = nblk_raw > 0 ? nblk_raw : 1;
  const size_t o_sums = (size_t)n * sizeof(VoiceRow), need = o_sums + (size_t)n * nblk_max * sizeof(double);
  ASW_CHECK_ARG(workspace_bytes >= need, "voice_trim: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "voice_trim: workspace not 8-byte aligned");
  hipStream_t s = asw::as_stream(stream);
  ASW_HIP(hipMemcpyAsync(workspace, rows.data(), o_sums, hipMemcpyHostToDevice, s));   // pageable: taken before the call returns
  const VoiceRow* drows = static_cast<const VoiceRow*>(workspace);
  double* bsum = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + o_sums);
  double samples = 0.0;
  for (const VoiceRow& r : rows) samples += r.len;
  if (nblk_raw > 0) {
    asw::ProfScope prof(s, "voice_block_sums", 2.0 * samples, samples * 4.0);
    hipLaunchKernelGGL(voice_block_sums_kernel, dim3(asw::cdiv(nblk_raw, 4), n), dim3(256), 0, s, x, drows, nblk_max, bsum);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "voice_trim", 5.0 * samples, samples * 8.0);
  hipLaunchKernelGGL(voice_trim_kernel, dim3(n), dim3(256), 0, s, x, drows, bsum, nblk_max, thr, bounds, stats);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
