// room_kernels.hip -- the shoebox room simulator of the dataset generator on the device in float64 (include/asw_hip.h:
// asw_room_rir, asw_room_convolve; the statements are roomsim.rir_f64 and convolve_f64).
//
// asw_room_rir builds image-source impulse responses.  A workgroup of 256 threads owns one (source, microphone) pair and
// one segment of 1024 samples, four samples per thread in registers.  It walks the (nx, ny) columns of the image lattice
// in canonical order, 256 columns a batch; a thread solves its column for the short nz ranges whose distance can reach
// the segment's window widened by the 81 taps, decides every candidate by the exact delay, and the hits of a batch are
// compacted in canonical order through a prefix sum in LDS.  Then every thread adds, hit after hit, the one tap that
// falls on each of its samples.  The distance and delay arithmetic is written as roomsim.image_delays_f64 writes it and
// the file is compiled with -ffp-contract=off: floor(t) and t - floor(t) come out bit for bit as in the statement.
//
// asw_room_convolve is uniformly partitioned overlap-save, hop 1024 and frame 2048, on the transform of fft1024.h:
// one launch transforms every frame of the dry signals and every zero-padded 1024-tap partition of the responses to
// 1025 bins, a second one accumulates X[s, b - p] H[s, m, p] over p ascending per (scene, microphone, block) with the
// bins in registers, inverts, keeps the second half, writes premix and adds the sources in order into mix.
//
// The house rules of bss_kernels.hip / eval_kernels.hip hold: grids over host-built tables, no atomics, no device-side
// assert, one writer per address, every sum in one fixed order; two runs give identical bytes.
#include "asw_common.h"
#include "fft1024.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

namespace {

using namespace asw::fft;              // NFFT, HOP, NB, NH, THREADS; Lds, fft1024, the split and merge steps

constexpr int MAX_K = 65535, MAX_S = 64, MAX_M = 1024, MAX_ROWS = 65535;
constexpr int MAX_T = 1 << 25;
constexpr int MAX_ORDER = 150;
constexpr long MAX_GRID = 1L << 30;
constexpr double SOUND = 343.0;                                // patch.SPEED_OF_SOUND
constexpr double PI = 3.141592653589793;
constexpr double FOUR_PI = 4.0 * PI;

// ---- asw_room_rir ------------------------------------------------------------------------------------------------
constexpr int SEG = 1024, SPT = SEG / THREADS;                 // samples of a segment, samples per thread
constexpr int TAPS = 81, LEAD = 40;                            // the Hann-windowed sinc and its lead-in
constexpr int CAP = 1024;                                      // hits that one accumulation round holds in LDS
constexpr int NPOW = MAX_ORDER + 1;

struct SceneRec {
  double L[3];
  int32_t order, pad;
};
struct SrcRec {
  double p[3];
  int32_t scene, pad;
};

// the host-built table at the head of the workspace: scenes, sources, microphones [K][M][3], r^n [K][151], window [81]
struct RirPlan {
  size_t o_scene, o_src, o_mic, o_pow, o_win, total;
};
RirPlan rir_plan(long K, long M, long n_src) {
  RirPlan p;
  p.o_scene = 0;
  p.o_src = p.o_scene + (size_t)K * sizeof(SceneRec);
  p.o_mic = p.o_src + (size_t)n_src * sizeof(SrcRec);
  p.o_pow = p.o_mic + (size_t)K * M * 3 * sizeof(double);
  p.o_win = p.o_pow + (size_t)K * NPOW * sizeof(double);
  p.total = p.o_win + TAPS * sizeof(double);
  return p;
}

// image coordinate n along one axis of length L for a source at s (roomsim.shoebox_images)
__device__ __forceinline__ double image_coord(int n, double L, double s) {
  return (n & 1) ? (double)(n + 1) * L - s : (double)n * L + s;
}

__device__ __forceinline__ double clamp_to(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

struct Column {                      // one (nx, ny) column as a thread sees it
  double rxy2, sz, mz, Lz;             // dx dx + dy dy; the z coordinates of source and microphone; the room's height
  int nxy, lo1, hi1, lo2, hi2;         // |nx| + |ny|; the two candidate nz ranges (empty when hi < lo)
};

struct Hits {
  int ip[CAP];
  double f[CAP], g[CAP], sp[CAP];      // fraction of the delay, gain, sin(pi f)
};

// The candidates of a column decided by the exact delay, in nz order.  WRITE = false counts the hits; WRITE = true
// stores hit number i at slot first + i where that lies inside 0..CAP-1.  lo..hi: the integer delays that reach the
// segment.
template <bool WRITE>
__device__ __forceinline__ int walk(const Column& c, double fs, double lo, double hi, const double* __restrict__ rpow, Hits& H,
                                    int first) {
  int n = 0;
  for (int r = 0; r < 2; ++r) {
    const int a = r ? c.lo2 : c.lo1, b = r ? c.hi2 : c.hi1;
    for (int nz = a; nz <= b; ++nz) {
      const double dz = image_coord(nz, c.Lz, c.sz) - c.mz;
      const double d = sqrt(c.rxy2 + dz * dz);
      const double t = d / SOUND * fs;
      const double ipd = floor(t);
      if (ipd < lo || ipd > hi) continue;
      if (WRITE) {
        const int slot = first + n;
        if (slot >= 0 && slot < CAP) {
          const double f = t - ipd;
          // sin(pi f) through the smaller of f and 1 - f (exact from 0.5 up): a delay a few ulps below an integer keeps
          // its relative precision, which the tap next to it divides by an equally small number
          H.ip[slot] = (int)ipd, H.f[slot] = f, H.sp[slot] = sin(PI * (f > 0.5 ? 1.0 - f : f));
          H.g[slot] = rpow[c.nxy + (nz < 0 ? -nz : nz)] / (FOUR_PI * d);
        }
      }
      ++n;
    }
  }
  return n;
}

// grid (segments, M, sources)
__global__ __launch_bounds__(THREADS) void room_rir_kernel(const SceneRec* __restrict__ scenes, const SrcRec* __restrict__ srcs,
                                                           const double* __restrict__ mics, const double* __restrict__ rpow_all,
                                                           const double* __restrict__ win_tab, int M, double fs, int length,
                                                           double* __restrict__ out) {
  __shared__ Hits H;
  __shared__ int cnt[THREADS], gsum[THREADS / 16];
  __shared__ double win[TAPS];
  const int tid = threadIdx.x, m = blockIdx.y;
  const int t0 = blockIdx.x * SEG;
  const SrcRec src = srcs[blockIdx.z];
  const SceneRec sc = scenes[src.scene];
  const double* mic = mics + ((int64_t)src.scene * M + m) * 3;
  const double mx = mic[0], my = mic[1], mz = mic[2];
  const double* rpow = rpow_all + (int64_t)src.scene * NPOW;
  if (tid < TAPS) win[tid] = win_tab[tid];

  const int N = sc.order, W = 2 * N + 1;
  // integer delays that reach the segment, and the distances that can have them: a sample of margin on either side
  const double lo = (double)t0 - (TAPS - 1), hi = (double)(min(t0 + SEG, length) - 1);
  const double dlo = (lo - 2.0) * (SOUND / fs), dhi = (hi + 3.0) * (SOUND / fs);
  double acc[SPT];
#pragma unroll
  for (int q = 0; q < SPT; ++q) acc[q] = 0.0;

  for (int col0 = 0; col0 < W * W; col0 += THREADS) {
    __syncthreads();                                            // the tables of the batch before are read out
    Column c{};
    c.lo1 = c.lo2 = 0, c.hi1 = c.hi2 = -1;
    const int col = col0 + tid;
    if (col < W * W) {
      const int nx = col / W - N, ny = col % W - N;
      const int rem = N - (nx < 0 ? -nx : nx) - (ny < 0 ? -ny : ny);
      if (rem >= 0) {
        const double dx = image_coord(nx, sc.L[0], src.p[0]) - mx, dy = image_coord(ny, sc.L[1], src.p[1]) - my;
        c.rxy2 = dx * dx + dy * dy, c.sz = src.p[2], c.mz = mz, c.Lz = sc.L[2], c.nxy = N - rem;
        const double hi2 = dhi * dhi - c.rxy2;
        if (hi2 >= 0.0) {
          // |dz| within a..b; the image lies in [nz Lz, (nz + 1) Lz], so dz within [nz Lz - mz, (nz + 1) Lz - mz]
          const double lo2 = dlo > 0.0 ? dlo * dlo - c.rxy2 : -1.0;
          const double a = lo2 > 0.0 ? sqrt(lo2) : 0.0, b = sqrt(hi2);
          const double bound = (double)rem;                    // every limit is clamped before it becomes an int
          const double l1 = clamp_to(floor((mz - b) / c.Lz) - 2.0, -bound, bound + 1.0);
          const double h1 = clamp_to(ceil((mz - a) / c.Lz) + 1.0, -bound - 1.0, bound);
          const double l2 = clamp_to(floor((mz + a) / c.Lz) - 2.0, -bound, bound + 1.0);
          const double h2 = clamp_to(ceil((mz + b) / c.Lz) + 1.0, -bound - 1.0, bound);
          c.lo1 = (int)l1, c.hi1 = (int)h1, c.hi2 = (int)h2;
          c.lo2 = max((int)l2, c.hi1 + 1);                      // the two ranges never share an image
        }
      }
    }
    const int mine = walk<false>(c, fs, lo, hi, rpow, H, 0);
    cnt[tid] = mine;
    __syncthreads();
    if (tid < THREADS / 16) {
      int s = 0;
      for (int i = 0; i < 16; ++i) s += cnt[16 * tid + i];
      gsum[tid] = s;
    }
    __syncthreads();
    int before = 0, total = 0;
    for (int g = 0; g < THREADS / 16; ++g) {
      if (g < tid / 16) before += gsum[g];
      total += gsum[g];
    }
    for (int i = 16 * (tid / 16); i < tid; ++i) before += cnt[i];

    for (int w0 = 0; w0 < total; w0 += CAP) {                   // total is the same in every thread
      if (w0 > 0) __syncthreads();                              // the round before is summed
      if (mine > 0 && before < w0 + CAP && before + mine > w0) walk<true>(c, fs, lo, hi, rpow, H, before - w0);
      __syncthreads();
      const int n = min(CAP, total - w0);
      const int tb = t0 + tid;
      for (int e = 0; e < n; ++e) {
        const int base = tb - H.ip[e];                          // tap index of this thread's first sample
        const int q = base >= 0 ? 0 : (-base + THREADS - 1) / THREADS;
        const int j = base + q * THREADS;
        if (j < TAPS && q < SPT) {
          const int k = j - LEAD;
          const double x = (double)k - H.f[e];
          const double sv = (k & 1) ? H.sp[e] : -H.sp[e];       // sin(pi (k - f)) = -(-1)^k sin(pi f)
          const double sinc = x == 0.0 ? 1.0 : sv / (PI * x);
          const double v = H.g[e] * win[j] * sinc;
#pragma unroll
          for (int qq = 0; qq < SPT; ++qq)
            if (qq == q) acc[qq] += v;
        }
      }
    }
  }
  double* row = out + ((int64_t)blockIdx.z * M + m) * length;
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int t = t0 + tid + q * THREADS;
    if (t < length) row[t] = acc[q];
  }
}

// ---- asw_room_convolve -------------------------------------------------------------------------------------------
struct TwiddleTables {
  static constexpr int kMaxDev = 64;
  std::mutex mu;
  double* tab[kMaxDev] = {};
};
TwiddleTables g_tw;

int device_twiddles(const double** out) {
  int dev = 0;
  ASW_HIP(hipGetDevice(&dev));
  ASW_CHECK_ARG(dev >= 0 && dev < TwiddleTables::kMaxDev, "room_convolve: device %d beyond the %d this library keeps tables for", dev,
                TwiddleTables::kMaxDev);
  std::lock_guard<std::mutex> lk(g_tw.mu);
  if (!g_tw.tab[dev]) {
    std::vector<double> h(2 * NH);
    fill_twiddles(h.data());
    double* d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(double)) != hipSuccess) return asw::set_error(ASW_ERR_NOMEM, "room_convolve: hipMalloc of the twiddles");
    if (hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return asw::set_error(ASW_ERR_HIP, "room_convolve: copy of the twiddles");
    }
    g_tw.tab[dev] = d;
  }
  *out = g_tw.tab[dev];
  return ASW_OK;
}

// the 1025 bins of the frame in buffer 0 to spec[0..1024]
__device__ __forceinline__ void store_bins(const Lds& L, const double* __restrict__ tw, double2* __restrict__ spec, int tid) {
  for (int k = tid; k <= NH / 2; k += THREADS) {
    Cx a, b;
    if (k == 0) split_ends(L, 1.0, a, b); else split_pair(L, tw, k, 1.0, a, b);
    spec[k] = make_double2(a.r, a.i);
    spec[NH - k] = make_double2(b.r, b.i);
  }
}

// grid (blocks, rows): frame b of a dry row holds the samples 1024 (b - 1) .. 1024 (b + 1) - 1, zero outside 0..T-1
__global__ __launch_bounds__(THREADS) void dry_spectra_kernel(const float* __restrict__ dry, int T, int nblk, const double* __restrict__ tw,
                                                              double2* __restrict__ X) {
  __shared__ Lds L;
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* row = dry + (int64_t)blockIdx.y * T;
  for (int m = tid; m < NH; m += THREADS) {
    const int64_t t = (int64_t)(b - 1) * HOP + 2 * m;
    L.re[0][m] = t >= 0 && t < T ? (double)row[t] : 0.0;
    L.im[0][m] = t + 1 >= 0 && t + 1 < T ? (double)row[t + 1] : 0.0;
  }
  fft1024<false>(L, tw, tid);
  store_bins(L, tw, X + ((int64_t)blockIdx.y * nblk + b) * NB, tid);
}

// grid (partitions, rows): partition p of a response row holds its taps 1024 p .. 1024 p + 1023, then 1024 zeros
__global__ __launch_bounds__(THREADS) void rir_spectra_kernel(const double* __restrict__ rir, int length, int parts,
                                                              const double* __restrict__ tw, double2* __restrict__ Hs) {
  __shared__ Lds L;
  const int tid = threadIdx.x, p = blockIdx.x;
  const double* row = rir + (int64_t)blockIdx.y * length;
  for (int m = tid; m < NH; m += THREADS) {
    const int64_t t = (int64_t)p * HOP + 2 * m;
    const bool head = m < NH / 2;
    L.re[0][m] = head && t < length ? row[t] : 0.0;
    L.im[0][m] = head && t + 1 < length ? row[t + 1] : 0.0;
  }
  fft1024<false>(L, tw, tid);
  store_bins(L, tw, Hs + ((int64_t)blockIdx.y * parts + p) * NB, tid);
}

struct ConvItem {                      // one scene
  int64_t row0;                        // its first source row
  int32_t S, pad;
};

constexpr int KPT = 3;                 // bin pairs (k, 1024 - k) per thread: k = tid, tid + 256 (and 512 for thread 0)

// grid (blocks, M, K)
__global__ __launch_bounds__(THREADS) void room_convolve_kernel(const ConvItem* __restrict__ items, const double2* __restrict__ X,
                                                                const double2* __restrict__ Hs, const double* __restrict__ tw, int M,
                                                                int T, int nblk, int parts, double* __restrict__ premix,
                                                                double* __restrict__ mix) {
  __shared__ Lds L;
  const int tid = threadIdx.x, b = blockIdx.x, m = blockIdx.y;
  const ConvItem it = items[blockIdx.z];
  const int plast = min(b, parts - 1);
  double mr[2] = {0.0, 0.0}, mi[2] = {0.0, 0.0};                // the mixture at the two complex samples this thread keeps
  for (int j = 0; j < it.S; ++j) {
    const int64_t s = it.row0 + j;
    Cx ya[KPT], yb[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) ya[i] = Cx{0.0, 0.0}, yb[i] = Cx{0.0, 0.0};
    for (int p = 0; p <= plast; ++p) {
      const double2* xs = X + (s * nblk + (b - p)) * NB;
      const double2* hs = Hs + ((s * M + m) * parts + p) * NB;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = tid + i * THREADS;
        if (k <= NH / 2) {
          const double2 xa = xs[k], ha = hs[k], xb = xs[NH - k], hb = hs[NH - k];
          ya[i].r += xa.x * ha.x - xa.y * ha.y, ya[i].i += xa.x * ha.y + xa.y * ha.x;
          yb[i].r += xb.x * hb.x - xb.y * hb.y, yb[i].i += xb.x * hb.y + xb.y * hb.x;
        }
      }
    }
    __syncthreads();                                            // the samples of the source before are read out
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int k = tid + i * THREADS;
      if (k <= NH / 2) {
        if (k == 0) merge_ends(L, ya[i].r, yb[i].r); else merge_pair(L, tw, k, ya[i], yb[i]);
      }
    }
    fft1024<true>(L, tw, tid);
    double* row = premix + (s * M + m) * T;
#pragma unroll
    for (int i = 0; i < 2; ++i) {                               // the second half of the frame: complex samples 512..1023
      const int z = NH / 2 + tid + i * THREADS;
      const int64_t t = (int64_t)b * HOP + 2 * (z - NH / 2);
      const double vr = L.re[0][z], vi = L.im[0][z];
      if (t < T) row[t] = vr;
      if (t + 1 < T) row[t + 1] = vi;
      mr[i] += vr, mi[i] += vi;
    }
  }
  double* row = mix + ((int64_t)blockIdx.z * M + m) * T;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t t = (int64_t)b * HOP + 2 * (tid + i * THREADS);
    if (t < T) row[t] = mr[i];
    if (t + 1 < T) row[t + 1] = mi[i];
  }
}

struct ConvPlan {
  long rows;
  int nblk, parts;
  size_t tab_bytes, o_x, o_h, total;
};

const char* conv_plan(const int32_t* counts, int K, int M, int length, int T, ConvPlan& p, char* msg, size_t msg_len) {
  if (K < 0 || K > MAX_K) { snprintf(msg, msg_len, "K = %d outside 0..%d", K, MAX_K); return msg; }
  if (M < 1 || M > MAX_M) { snprintf(msg, msg_len, "M = %d outside 1..%d", M, MAX_M); return msg; }
  if (length < 1 || length > MAX_T) { snprintf(msg, msg_len, "length = %d outside 1..%d", length, MAX_T); return msg; }
  if (T < 1 || T > MAX_T) { snprintf(msg, msg_len, "T = %d outside 1..%d", T, MAX_T); return msg; }
  if (K > 0 && !counts) { snprintf(msg, msg_len, "null counts"); return msg; }
  p = ConvPlan{};
  for (int k = 0; k < K; ++k) {
    if (counts[k] < 0 || counts[k] > MAX_S) { snprintf(msg, msg_len, "scene %d: %d sources outside 0..%d", k, counts[k], MAX_S); return msg; }
    p.rows += counts[k];
  }
  p.nblk = asw::cdiv(T, HOP), p.parts = asw::cdiv(length, HOP);
  if (p.rows > MAX_ROWS || p.rows * M > MAX_ROWS) {
    snprintf(msg, msg_len, "%ld sources times %d microphones outgrow one launch (%d rows)", p.rows, M, MAX_ROWS);
    return msg;
  }
  p.tab_bytes = (((size_t)K * sizeof(ConvItem)) + 15) / 16 * 16;
  p.o_x = p.tab_bytes;
  p.o_h = p.o_x + (size_t)p.rows * p.nblk * NB * sizeof(double2);
  p.total = p.o_h + (size_t)p.rows * M * p.parts * NB * sizeof(double2);
  if (p.total < 16) p.total = 16;
  return nullptr;
}

}  // namespace

extern "C" size_t asw_room_rir_workspace_bytes(int K, int M, int n_src) {
  if (K < 0 || K > MAX_K || M < 1 || M > MAX_M || n_src < 0 || n_src > MAX_ROWS) {
    asw::set_error(ASW_ERR_ARG, "room_rir_workspace_bytes: K=%d outside 0..%d, M=%d outside 1..%d or %d sources outside 0..%d", K, MAX_K,
                   M, MAX_M, n_src, MAX_ROWS);
    return 0;
  }
  return rir_plan(K, M, n_src).total;
}

extern "C" int asw_room_rir(const double* rooms, const double* absorption, const int32_t* max_orders, const double* src,
                            const double* mics, const int32_t* counts, int K, int M, double fs, int length, double* rir,
                            void* workspace, size_t workspace_bytes, void* stream) {
  ASW_CHECK_ARG(K >= 0 && K <= MAX_K, "room_rir: K = %d outside 0..%d", K, MAX_K);
  ASW_CHECK_ARG(M >= 1 && M <= MAX_M, "room_rir: M = %d outside 1..%d", M, MAX_M);
  ASW_CHECK_ARG(length >= 1 && length <= MAX_T, "room_rir: length = %d outside 1..%d", length, MAX_T);
  ASW_CHECK_ARG(fs > 0.0 && fs <= 1e9, "room_rir: fs = %g outside (0, 1e9]", fs);
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(rooms && absorption && max_orders && mics && counts, "room_rir: null host table");
  long n_src = 0;
  for (int k = 0; k < K; ++k) {
    ASW_CHECK_ARG(counts[k] >= 0 && counts[k] <= MAX_S, "room_rir: scene %d: %d sources outside 0..%d", k, counts[k], MAX_S);
    n_src += counts[k];
  }
  ASW_CHECK_ARG(n_src <= MAX_ROWS, "room_rir: %ld sources (at most %d)", n_src, MAX_ROWS);
  ASW_CHECK_ARG(src || n_src == 0, "room_rir: null src");
  const RirPlan p = rir_plan(K, M, n_src);
  std::vector<unsigned char> tab(p.total);
  SceneRec* hs = reinterpret_cast<SceneRec*>(tab.data() + p.o_scene);
  SrcRec* hr = reinterpret_cast<SrcRec*>(tab.data() + p.o_src);
  double* hm = reinterpret_cast<double*>(tab.data() + p.o_mic);
  double* hp = reinterpret_cast<double*>(tab.data() + p.o_pow);
  double* hw = reinterpret_cast<double*>(tab.data() + p.o_win);
  long row = 0;
  for (int k = 0; k < K; ++k) {
    const double* L = rooms + 3 * k;
    ASW_CHECK_ARG(L[0] > 0.0 && L[1] > 0.0 && L[2] > 0.0 && L[0] <= 1e6 && L[1] <= 1e6 && L[2] <= 1e6,
                  "room_rir: scene %d: room %g x %g x %g is no box of sides within (0, 1e6]", k, L[0], L[1], L[2]);
    ASW_CHECK_ARG(absorption[k] > 0.0 && absorption[k] <= 1.0, "room_rir: scene %d: absorption %g outside (0, 1]", k, absorption[k]);
    ASW_CHECK_ARG(max_orders[k] >= 0 && max_orders[k] <= MAX_ORDER, "room_rir: scene %d: max_order %d outside 0..%d", k, max_orders[k],
                  MAX_ORDER);
    for (int m = 0; m < M; ++m)
      for (int a = 0; a < 3; ++a) {
        const double v = mics[((size_t)k * M + m) * 3 + a];
        ASW_CHECK_ARG(v > 0.0 && v < L[a], "room_rir: scene %d: microphone %d lies outside the room (axis %d: %g not inside 0..%g)", k, m,
                      a, v, L[a]);
        hm[((size_t)k * M + m) * 3 + a] = v;
      }
    for (int j = 0; j < counts[k]; ++j, ++row) {
      const double* s = src + 3 * row;
      for (int a = 0; a < 3; ++a)
        ASW_CHECK_ARG(s[a] > 0.0 && s[a] < L[a], "room_rir: scene %d: source %d lies outside the room (axis %d: %g not inside 0..%g)", k, j,
                      a, s[a], L[a]);
      for (int m = 0; m < M; ++m) {
        const double* q = mics + ((size_t)k * M + m) * 3;
        ASW_CHECK_ARG(!(s[0] == q[0] && s[1] == q[1] && s[2] == q[2]), "room_rir: scene %d: source %d sits at microphone %d", k, j, m);
      }
      hr[row] = SrcRec{{s[0], s[1], s[2]}, k, 0};
    }
    hs[k] = SceneRec{{L[0], L[1], L[2]}, max_orders[k], 0};
    const double r = std::sqrt(1.0 - absorption[k]);
    for (int n = 0; n < NPOW; ++n) hp[(size_t)k * NPOW + n] = std::pow(r, (double)n);
  }
  for (int j = 0; j < TAPS; ++j) hw[j] = 0.5 - 0.5 * std::cos(2.0 * PI * j / (TAPS - 1));
  if (n_src == 0) return ASW_OK;
  ASW_CHECK_ARG(rir && workspace, "room_rir: null pointer");
  ASW_CHECK_ARG(workspace_bytes >= p.total, "room_rir: workspace of %zu bytes too small, %zu needed", workspace_bytes, p.total);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "room_rir: workspace not 8-byte aligned");
  const long segs = asw::cdiv(length, SEG);
  ASW_CHECK_ARG(segs * M * n_src <= MAX_GRID, "room_rir: %ld sources, %d microphones and %d samples outgrow one launch", n_src, M, length);
  hipStream_t s = asw::as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  ASW_HIP(hipMemcpyAsync(ws, tab.data(), p.total, hipMemcpyHostToDevice, s));     // pageable: taken before the call returns
  asw::ProfScope prof(s, "room_rir", 0.0, (double)n_src * M * length * 8.0);
  hipLaunchKernelGGL(room_rir_kernel, dim3((unsigned)segs, M, (unsigned)n_src), dim3(THREADS), 0, s,
                     reinterpret_cast<const SceneRec*>(ws + p.o_scene), reinterpret_cast<const SrcRec*>(ws + p.o_src),
                     reinterpret_cast<const double*>(ws + p.o_mic), reinterpret_cast<const double*>(ws + p.o_pow),
                     reinterpret_cast<const double*>(ws + p.o_win), M, fs, length, rir);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" size_t asw_room_convolve_workspace_bytes(const int32_t* counts, int K, int M, int length, int T) {
  ConvPlan p;
  char msg[160];
  if (conv_plan(counts, K, M, length, T, p, msg, sizeof msg)) {
    asw::set_error(ASW_ERR_ARG, "room_convolve_workspace_bytes: %s", msg);
    return 0;
  }
  return p.total;
}

extern "C" int asw_room_convolve(const float* dry, const double* rir, const int32_t* counts, int K, int M, int length, int T,
                                 double* premix, double* mix, void* workspace, size_t workspace_bytes, void* stream) {
  ConvPlan p;
  char msg[160];
  if (conv_plan(counts, K, M, length, T, p, msg, sizeof msg)) return asw::set_error(ASW_ERR_ARG, "room_convolve: %s", msg);
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(mix && workspace, "room_convolve: null mix or workspace");
  ASW_CHECK_ARG((dry && rir && premix) || p.rows == 0, "room_convolve: null pointer");
  ASW_CHECK_ARG(workspace_bytes >= p.total, "room_convolve: workspace of %zu bytes too small, %zu needed", workspace_bytes, p.total);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "room_convolve: workspace not 16-byte aligned");
  ASW_CHECK_ARG((long)p.nblk * M * K <= MAX_GRID && (long)p.parts * p.rows * M <= MAX_GRID,
                "room_convolve: %d scenes of %d microphones and %d samples outgrow one launch", K, M, T);
  const double* tw = nullptr;
  if (int rc = device_twiddles(&tw)) return rc;
  hipStream_t s = asw::as_stream(stream);
  std::vector<ConvItem> hi(K);
  int64_t row0 = 0;
  for (int k = 0; k < K; ++k) {
    hi[k] = ConvItem{row0, counts[k], 0};
    row0 += counts[k];
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  double2* X = reinterpret_cast<double2*>(ws + p.o_x);
  double2* Hs = reinterpret_cast<double2*>(ws + p.o_h);
  ASW_HIP(hipMemcpyAsync(ws, hi.data(), (size_t)K * sizeof(ConvItem), hipMemcpyHostToDevice, s));   // pageable: taken before the call returns
  if (p.rows > 0) {
    {
      asw::ProfScope prof(s, "room_dry_spectra", 5.0 * NH * 10 * (double)p.rows * p.nblk, (double)p.rows * p.nblk * (NFFT * 4.0 + NB * 16.0));
      hipLaunchKernelGGL(dry_spectra_kernel, dim3(p.nblk, (unsigned)p.rows), dim3(THREADS), 0, s, dry, T, p.nblk, tw, X);
      ASW_LAUNCH_CHECK();
    }
    asw::ProfScope prof(s, "room_rir_spectra", 5.0 * NH * 10 * (double)p.rows * M * p.parts, (double)p.rows * M * p.parts * (HOP * 8.0 + NB * 16.0));
    hipLaunchKernelGGL(rir_spectra_kernel, dim3(p.parts, (unsigned)(p.rows * M)), dim3(THREADS), 0, s, rir, length, p.parts, tw, Hs);
    ASW_LAUNCH_CHECK();
  }
  const double pairs = (double)p.rows * M * p.nblk * (p.parts + 1) / 2.0;
  asw::ProfScope prof(s, "room_convolve", 8.0 * NB * pairs, 32.0 * NB * pairs);
  hipLaunchKernelGGL(room_convolve_kernel, dim3(p.nblk, M, K), dim3(THREADS), 0, s, reinterpret_cast<const ConvItem*>(ws), X, Hs, tw, M, T,
                     p.nblk, p.parts, premix, mix);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
