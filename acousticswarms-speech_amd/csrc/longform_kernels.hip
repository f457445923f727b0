// longform_kernels.hip -- a recording of any length as overlapping blocks: the gather that frames the blocks and the
// normalised overlap-add that stitches the separated blocks back together (include/asw_hip.h: asw_frame_blocks,
// asw_stitch_blocks; the statements are longform.frame_f64 and longform.stitch_f64).
//
// Both kernels only move data: a thread owns four consecutive samples of one row and reads and writes them as 16-byte
// accesses (the vector type below asks for dword alignment only, which is all a global access of gfx950 needs, so a
// block that starts at any sample takes the same path).  Every output sample has one writer, there are no atomics and
// nothing is accumulated in memory.  The host tables (block starts, the row of every (block, track)) travel as kernel
// arguments, TABLE_INTS per launch; a longer table is cut into launches that each own a range of the output (a run of
// blocks, and for the stitch a run of tracks), so there is no device table, no copy and nothing to synchronise.
#include "asw_common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int TABLE_INTS = 960;        // 3840 bytes of the 4 KB of kernel arguments
constexpr int THREADS = 256;
constexpr int MAX_GRID_X = 2048;       // grid-stride beyond: a memory-bound pass gains nothing from more workgroups
constexpr int MAX_GRID_Y = 65535;
constexpr int MAX_SAMPLES = 1 << 30;   // T and Ttot: a sample index plus one grid stride stays inside int32

typedef float f32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef double f64x4 __attribute__((ext_vector_type(4), aligned(8)));

struct Table {
  int32_t v[TABLE_INTS];
};

// out[k][m][j] = mix[m][a_k + j], 0 past Ttot, for the nb blocks whose starts are tab.v[0 .. nb); blockIdx.y = kl * M + m
__global__ __launch_bounds__(THREADS) void frame_blocks_kernel(const float* __restrict__ mix, int M, int Ttot, int T, Table tab,
                                                               float* __restrict__ out) {
  const int kl = blockIdx.y / M, m = blockIdx.y - kl * M;
  const int a = tab.v[kl];
  const float* src = mix + (size_t)m * Ttot + a;
  float* dst = out + (size_t)blockIdx.y * T;
  const int left = Ttot - a;                                 // samples of the recording from a on (>= 1)
  for (int j = (blockIdx.x * THREADS + threadIdx.x) * 4; j < T; j += gridDim.x * THREADS * 4) {
    if (j + 3 < T && j + 3 < left) {
      *reinterpret_cast<f32x4*>(dst + j) = *reinterpret_cast<const f32x4*>(src + j);
    } else {
      for (int i = 0; i < 4 && j + i < T; ++i) dst[j + i] = j + i < left ? src[j + i] : 0.f;
    }
  }
}

// out[s][t] for t in [t0, t1) and s = s0 + blockIdx.y, from the nb blocks that cover that range: tab.v[0 .. nb) their
// starts (ascending), tab.v[nb + kl * gridDim.y + blockIdx.y] the row of track s in block kl (-1: absent)
__global__ __launch_bounds__(THREADS) void stitch_blocks_kernel(const float* __restrict__ rows, const double* __restrict__ taper,
                                                                Table tab, int nb, int s0, int T, int Ttot, int t0, int t1,
                                                                float* __restrict__ out) {
  float* dst = out + (size_t)(s0 + blockIdx.y) * Ttot;
  for (int t = t0 + (blockIdx.x * THREADS + threadIdx.x) * 4; t < t1; t += gridDim.x * THREADS * 4) {
    // first block that ends after t: the blocks before it cover none of t .. t + 3
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tab.v[mid] + T > t) hi = mid; else lo = mid + 1;
    }
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kl = lo; kl < nb && tab.v[kl] <= t + 3; ++kl) {         // ascending k: the order of the statement's sums
      const int j = t - tab.v[kl];                                    // -3 .. T - 1
      const int r = tab.v[nb + kl * gridDim.y + blockIdx.y];
      const float* x = r >= 0 ? rows + (size_t)r * T : nullptr;
      if (j >= 0 && j + 3 < T) {
        const f64x4 w = *reinterpret_cast<const f64x4*>(taper + j);
        f32x4 xv = {0.f, 0.f, 0.f, 0.f};
        if (x) xv = *reinterpret_cast<const f32x4*>(x + j);
        for (int i = 0; i < 4; ++i) den[i] += w[i], num[i] += w[i] * (double)xv[i];
      } else {
        for (int i = 0; i < 4; ++i) {
          if (j + i < 0 || j + i >= T) continue;
          const double w = taper[j + i];
          den[i] += w;
          if (x) num[i] += w * (double)x[j + i];
        }
      }
    }
    if (t + 3 < t1) {
      f32x4 o;
      for (int i = 0; i < 4; ++i) o[i] = (float)(num[i] / den[i]);
      *reinterpret_cast<f32x4*>(dst + t) = o;
    } else {
      for (int i = 0; i < 4 && t + i < t1; ++i) dst[t + i] = (float)(num[i] / den[i]);
    }
  }
}

int grid_x(long samples) { return std::max(1, std::min(MAX_GRID_X, asw::cdiv(samples, THREADS * 4))); }

constexpr int STITCH_TRACKS = 63;     // tracks per launch at most, which leaves its table 15 blocks

// The launches that begin at block k0 of a stitch, ns tracks each: they own the output from starts[k0] to starts[k1] (to
// Ttot when k1 == K) and read the blocks lo .. k1 - 1, lo being the first block that reaches past starts[k0].  False when
// not even block k0 fits the table beside the earlier blocks that cover its first samples.
bool stitch_range(const int32_t* starts, int K, int ns, int T, int k0, int& lo, int& k1) {
  lo = k0;
  while (lo > 0 && (int64_t)starts[lo - 1] + T > starts[k0]) --lo;
  k1 = std::min(K, lo + TABLE_INTS / (ns + 1));
  return k1 > k0;
}

}  // namespace

extern "C" int asw_frame_blocks(const float* mix, int M, int Ttot, const int32_t* starts, int K, int T, float* out,
                                void* stream) {
  ASW_CHECK_ARG(mix && starts && out, "frame_blocks: null pointer");
  ASW_CHECK_ARG(M >= 1 && M <= MAX_GRID_Y && Ttot >= 1 && Ttot <= MAX_SAMPLES && K >= 1 && T >= 1 && T <= MAX_SAMPLES,
                "frame_blocks: bad shape (M=%d Ttot=%d K=%d T=%d)", M, Ttot, K, T);
  for (int k = 0; k < K; ++k)
    ASW_CHECK_ARG(starts[k] >= 0 && starts[k] < Ttot, "frame_blocks: block %d starts at %d, outside the %d samples", k, starts[k],
                  Ttot);
  hipStream_t s = asw::as_stream(stream);
  const int per = std::min(TABLE_INTS, MAX_GRID_Y / M);
  for (int k0 = 0; k0 < K; k0 += per) {
    const int nb = std::min(per, K - k0);
    Table tab;
    std::copy(starts + k0, starts + k0 + nb, tab.v);
    asw::ProfScope prof(s, "frame_blocks", 0.0, 8.0 * nb * M * T);
    hipLaunchKernelGGL(frame_blocks_kernel, dim3(grid_x(T), nb * M), dim3(THREADS), 0, s, mix, M, Ttot, T, tab,
                       out + (size_t)k0 * M * T);
    ASW_LAUNCH_CHECK();
  }
  return ASW_OK;
}

extern "C" int asw_stitch_blocks(const float* rows, int N, const double* taper, const int32_t* starts, const int32_t* row_of,
                                 int K, int S, int T, int Ttot, float* out, void* stream) {
  ASW_CHECK_ARG(rows && taper && starts && row_of && out, "stitch_blocks: null pointer");
  ASW_CHECK_ARG(N >= 1 && K >= 1 && S >= 1 && T >= 1 && T <= MAX_SAMPLES && Ttot >= 1 && Ttot <= MAX_SAMPLES,
                "stitch_blocks: bad shape (N=%d K=%d S=%d T=%d Ttot=%d)", N, K, S, T, Ttot);
  // every sample has a cover: the blocks begin at 0, leave no gap and reach the end
  ASW_CHECK_ARG(starts[0] == 0, "stitch_blocks: block 0 starts at %d, not at 0", starts[0]);
  for (int k = 1; k < K; ++k)
    ASW_CHECK_ARG(starts[k] > starts[k - 1] && (int64_t)starts[k] - starts[k - 1] <= T && starts[k] < Ttot,
                  "stitch_blocks: block %d starts at %d after %d (ascending, at most T=%d apart, inside the %d samples)", k,
                  starts[k], starts[k - 1], T, Ttot);
  ASW_CHECK_ARG((int64_t)starts[K - 1] + T >= Ttot, "stitch_blocks: the last block ends at %ld, before the %d samples end",
                (long)starts[K - 1] + T, Ttot);
  for (long i = 0; i < (long)K * S; ++i)
    ASW_CHECK_ARG(row_of[i] >= -1 && row_of[i] < N, "stitch_blocks: row_of[%ld][%ld] = %d outside -1..%d", i / S, i % S, row_of[i],
                  N - 1);
  const int ns = std::min(S, STITCH_TRACKS);
  int lo, k1;
  for (int k0 = 0; k0 < K; k0 = k1)
    ASW_CHECK_ARG(stitch_range(starts, K, ns, T, k0, lo, k1), "stitch_blocks: the %d blocks that cover sample %d outgrow one launch's table",
                  k0 - lo + 1, starts[k0]);
  hipStream_t s = asw::as_stream(stream);
  for (int k0 = 0; k0 < K; k0 = k1) {
    stitch_range(starts, K, ns, T, k0, lo, k1);
    const int nb = k1 - lo, t0 = starts[k0], t1 = k1 == K ? Ttot : starts[k1];
    for (int s0 = 0; s0 < S; s0 += ns) {
      const int n = std::min(ns, S - s0);
      Table tab;
      std::copy(starts + lo, starts + k1, tab.v);
      for (int kl = 0; kl < nb; ++kl)
        std::copy(row_of + (size_t)(lo + kl) * S + s0, row_of + (size_t)(lo + kl) * S + s0 + n, tab.v + nb + kl * n);
      // per output sample: the float written, and a float and a double read for each of its (one to two, rarely three) covers
      asw::ProfScope prof(s, "stitch_blocks", 0.0, (double)n * (t1 - t0) * 4.0 + (double)n * (k1 - k0) * T * 12.0);
      hipLaunchKernelGGL(stitch_blocks_kernel, dim3(grid_x(t1 - t0), n), dim3(THREADS), 0, s, rows, taper, tab, nb, s0, T, Ttot, t0,
                         t1, out);
      ASW_LAUNCH_CHECK();
    }
  }
  return ASW_OK;
}
