// resconv.hip -- the dilated residual layers (DilatedResidualLayer, sep/training/SpeakerLocalization/network.py:57-68)
// as one halo-staged f16x3 kernel per layer, reached from the dispatcher of convgemm.hip through asw::try_resconv.
// Activations channels-last [B][T][C] fp32, weights in MFMA-fragment order (asw_pack_fragments_f16); the two
// arithmetic modes and the layout are described at the head of convgemm.hip, the epilogue in gemm_epilogue.h.
// (The epilogue is instantiated with LayerNorm only, so its range guard is constant false here: this file's copy
// of g_f16x3_overflow is never written and asw_f16x3_overflow_count does not read it.)
#include "gemm_epilogue.h"

namespace {
using namespace asw_mfma;

#ifdef ASW_PHASE_TIMING
// Diagnostic build only (tests/micro/phase_timing.py): cycles wave 0 of every workgroup spends in
// each phase of a residual-layer tile, summed over workgroups.  [0] staging (global loads, split,
// LDS writes, barrier), [1] taps x k-steps, [2] epilogue, [3] workgroups counted.
__device__ unsigned long long g_phase_cycles[4] = {0, 0, 0, 0};
#endif

// ------------------------------------------------------------------ halo-staged residual conv
// DilatedResidualLayer (network.py:57-68) in f16x3 arithmetic: out = LN(ReLU(conv_d(x)+b) + x).
// The workgroup owns BM output rows x all C channels.  For each 64-channel slice of the
// input it stages the rows its taps touch ONCE into LDS, already split into fp16 hi/lo
// (row = 128 B hi + 128 B lo + 16 B pad: the per-lane 16-byte fragment reads of 32
// consecutive rows are bank-conflict free); every tap reads that image at a row offset, so
// the input is fetched and converted once per workgroup instead of once per tap.
//
// Row sets.  PH == 1: BM consecutive rows, image = rows [m0 - pad, m0 + BM + pad), tap step
// = dil rows.  PH > 1 (large dilation, 49): a dilated convolution is `dil` independent
// dilation-1 convolutions on the polyphase sub-sequences x[phase + dil*j]; the workgroup
// takes PH phases x BM/PH consecutive j, image = PH x (BM/PH + taps-1) rows, tap step = 1
// row.  The halo is then K-1 rows per phase instead of (K-1)*dil, which keeps the image at
// ~40 KB and lets 3-4 workgroups share a CU (the kernel is latency-bound otherwise).
//
// Weights never touch LDS: they are pre-packed in MFMA-fragment order, so each wave pulls
// its B operand with one coalesced 1 KiB load per fragment, one k-step ahead of the MFMAs
// (they are L2/L1-resident: a layer's weights are at most 7.3 MB and shared by every
// workgroup).  No barrier inside the taps x k-steps of a slice.
template <int BM, int PH, bool POLY>
struct ResRows {
  static constexpr int BMJ = BM / PH;
  int m0, jb, pb, dil, T;                    // contiguous tiles use m0; polyphase tiles (jb, pb)
  __device__ __forceinline__ int operator()(int trow) const {
    if (!POLY) { const int t = m0 + trow; return t < T ? t : -1; }
    const int ph = pb * PH + trow / BMJ;
    const int t = dil * (jb * BMJ + trow % BMJ) + ph;
    return (ph < dil && t < T) ? t : -1;
  }
};

template <int BM, int C, int WM, int WN, int PH, int QD = 4, bool POLY = (PH > 1), bool GLU = false, int NTERM = 3>
__global__ __launch_bounds__(64 * WM * WN)
__attribute__((amdgpu_waves_per_eu(C == 64 ? 4 : WM * WN == 8 ? 2 : (QD == 2 ? (C >= 512 || (C == 256 && BM == 128) ? 2 : 3) : (C == 64 && WM * WN == 4 ? 4 : 1)))))
void resconv16_kernel(const asw_convgemm_args p) {
  static_assert(QD == 2 || QD == 4, "B prefetch depth in k-steps");
  static_assert(!GLU || (PH == 1 && !POLY), "GroupNorm + GLU on load: contiguous tiles only");
  static_assert(WM * WN == 2 || WM * WN == 4 || WM * WN == 8, "2, 4 or 8 waves per workgroup");
  constexpr int NTHR = 64 * WM * WN;
  constexpr int TM = BM / WM / 32, TN = C / WN / 32;
  constexpr int NT = C / 32;                 // 32-column fragments across N
  constexpr int BMJ = BM / PH;
  constexpr int SU = (GLU && C > 64) ? 4 : 8;   // staging rows per thread in flight
  static_assert(BMJ % 32 == 0, "an MFMA row tile must stay inside one phase");

  extern __shared__ __align__(16) float smem[];
  char* img = reinterpret_cast<char*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int b = blockIdx.z;
  const int taps = p.taps, dil = p.dil, pad = p.pad;
  const int T = p.M_out;
  // contiguous: blockIdx.x = row tile.  polyphase: blockIdx.x = jb * n_pb + pb (PH phases per workgroup).
  const int n_pb = (dil + PH - 1) / PH;
  const int jb = !POLY ? 0 : blockIdx.x / n_pb, pb = !POLY ? 0 : blockIdx.x % n_pb;
  const int m0 = blockIdx.x * BM;
  const int RJ = BMJ + (!POLY ? (taps - 1) * dil : taps - 1);      // image rows per phase
  const int R = PH * RJ;
  const int tapstep = !POLY ? dil : 1;
  // GLU: the input row g is GLU(GroupNorm(raw row g)), raw = [T][value half C | gate half C]
  const __amdgpu_buffer_rsrc_t rX = GLU ? act_rsrc(p.glu_raw + (long)b * T * 2 * C, (long)T * 2 * C)
                                        : act_rsrc(p.A + (long)b * p.a_batch_stride, (long)T * C);
  const half8* __restrict__ Wh = reinterpret_cast<const half8*>(p.Wf_hi);
  const half8* __restrict__ Wl = reinterpret_cast<const half8*>(p.Wf_lo);

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int sc4 = tid & 15;                           // staging: 16 threads per row
  int a_base[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int trow = wm * (BM / WM) + i * 32;          // first row of this MFMA tile
    a_base[i] = ((trow / BMJ) * RJ + trow % BMJ + (lane & 31)) * RS + (lane >> 5) * 16;
  }
  const int nt0 = wn * TN;                            // first N fragment of this wave

  GluCoef gc;
  if (GLU) gc.stats(p.glu_mr, b);
  ASW_PHASE_MARK(t_begin);
#ifdef ASW_PHASE_TIMING
  unsigned long long t_stage = 0, t_loop = 0;
#endif
  // (the two slices at C = 128 are unrolled -- not in the one-term kernels without GLU -- and no others: what hipcc
  // chose on its own while the staging loop was written out here)
#pragma unroll(C == 128 && (NTERM == 3 || GLU) ? 2 : 1)
  for (int cc = 0; cc < C / 64; ++cc) {
    ASW_PHASE_MARK(t_s0);
    if (GLU) gc.affine(p.glu_gamma, p.glu_beta, C, cc * 64 + sc4 * 4);
    __syncthreads();                                   // previous slice fully consumed
    // ---- stage + split the image of this channel slice (8 loads per thread in flight: 8 rows, or 4 rows of value + gate
    // halves where the accumulators leave no room for more)
    stage_image<NTHR, C, SU, GLU, NTERM, C == 64>(
        img, R, rX, cc * 64, gc,
        [&](int row) __attribute__((always_inline)) {
          int g;
          bool ok = row < R;
          if (!POLY) {
            g = m0 - pad + row;
          } else {
            const int ph = pb * PH + row / RJ;
            g = dil * (jb * BMJ + row % RJ - (taps - 1) / 2) + ph;
            ok = ok && ph < dil && (jb * BMJ + row % RJ - (taps - 1) / 2) >= 0;
          }
          return ImgSrc{g, ok && g >= 0 && g < T};
        },
        // the normalised rows of the tile's own output range go out once as well: the skip connection of an
        // encoder block, and (C > 64, where the image holds one channel slice at a time) this layer's residual
        [&](int g, bool ok, const float4& o) __attribute__((always_inline)) {
          if (p.glu_out && ok && g >= m0 && g < m0 + BM)
            *reinterpret_cast<float4*>(p.glu_out + ((long)b * T + g) * C + cc * 64 + sc4 * 4) = o;
        });
    __syncthreads();
    // ---- taps x k-steps, B fragments double-buffered in registers
    auto bload = [&](int tap, int ks, half8 (&bh)[TN], half8 (&bl)[TN]) {
      const long kg = (long)tap * (C / 16) + cc * 4 + ks;          // global k-step
#pragma unroll
      for (int j = 0; j < TN; ++j) frag_load<NTERM>(Wh, Wl, kg * NT + nt0 + j, lane, bh[j], bl[j]);
    };
    // A fragments are double buffered in registers, one k-step ahead: left to itself the compiler
    // keeps ONE fragment register and waits for every ds_read right before its MFMA
    // (ds_read -> s_waitcnt lgkmcnt(0) -> mfma, four times per k-step), i.e. no LDS read of a wave
    // ever overlaps its own MFMAs.
    auto aload = [&](int tap, int ks, half8 (&ah)[TM], half8 (&al)[TM]) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const char* q = img + a_base[i] + tap * tapstep * RS + ks * 32;
        ah[i] = *reinterpret_cast<const half8*>(q + IMG_HI);
        if (NTERM == 3) al[i] = *reinterpret_cast<const half8*>(q + IMG_LO);
      }
    };
    auto mma = [&](const half8 (&ah)[TM], const half8 (&al)[TM], const half8 (&bh)[TN], const half8 (&bl)[TN]) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma3<NTERM>(acc[i][j], ah[i], al[i], bh[j], bl[j]);
    };
    // One B register buffer per k-step of a tap: the fragment for (tap+1, ks) is requested
    // right after (tap, ks) has been multiplied, i.e. three k-steps (600-1200 MFMA cycles)
    // before its use -- enough to cover an L2 hit without the register cost of a second
    // whole-tap set (which halves occupancy; measured slower for C <= 128).
    // (measured, T = 48 000 batch 64: C = 64 268 -> 280 TFLOP/s, C = 512 361 -> 368, C = 256 unchanged;
    // at C = 128 the 32 extra registers cost more than the overlap gains, 305 -> 301, so it keeps
    // the single buffer)
    constexpr bool ADB = C != 128;
    half8 qh[QD][TN], ql[QD][TN];
    half8 ah[ADB ? 2 : 1][TM], al[ADB ? 2 : 1][TM];
    ASW_PHASE_MARK(t_s1);
#pragma unroll
    for (int ks = 0; ks < QD; ++ks) bload(0, ks, qh[ks], ql[ks]);
    if (ADB) aload(0, 0, ah[0], al[0]);
    // (Measured in round 3 and dropped here: the same loop with every load unconditional -- clamped past-the-end
    // taps -- and the k-steps pinned by sched_barrier, which lifts the transposed C = 64 kernel of resstack.hip by
    // 5-8 %: C = 128 +0.7 %, C = 256 +-0, C = 512 -2 %; unconditional loads without the pinning -3...-10 %.)
    for (int tap = 0; tap < taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ADB) {                          // next k-step's A fragments
          const int nks = (ks + 1) & 3, ntp = tap + (ks == 3 ? 1 : 0);
          if (ntp < taps) aload(ntp, nks, ah[(ks + 1) & 1], al[(ks + 1) & 1]);
        } else {
          aload(tap, ks, ah[0], al[0]);
        }
        mma(ah[ADB ? (ks & 1) : 0], al[ADB ? (ks & 1) : 0], qh[ks % QD], ql[ks % QD]);
        const int nk = ks + QD, ntap = tap + nk / 4;               // QD k-steps ahead
        if (ntap < taps) bload(ntap, nk % 4, qh[ks % QD], ql[ks % QD]);
      }
    }
#ifdef ASW_PHASE_TIMING
    {
      // make the timestamp wait for the MFMAs: read one accumulator lane
      float sink = acc[0][0][0];
      asm volatile("" ::"v"(sink));
      const unsigned long long t_s2 = __builtin_readcyclecounter();
      t_stage += t_s1 - t_s0;
      t_loop += t_s2 - t_s1;
    }
#endif
  }
  ASW_PHASE_MARK(t_epi0);
  if constexpr (C == 64) {
    // The residual of this layer is its own input, and at C = 64 the whole input row of every
    // output row still sits in the LDS image (one channel slice) as fp16 hi + lo.  Taking it from
    // there (x = hi + lo, 2^-22 relative) instead of re-loading it from global memory removes the
    // load latency from the epilogue, which is 44 % of a workgroup's time at this width
    // (tests/micro/phase_timing.py).  Read before the first slab barrier: the slab aliases the image.
    using G = EpiGeom<C, WM, WN>;
    float4 rpre[TM * G::NSTEP * G::VPL];
    const int sub = lane / G::LPR, lc = lane % G::LPR;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int st = 0; st < G::NSTEP; ++st) {
        const int sr = (st * G::NW + wid) * G::RPI + sub;
        const int trow = (sr >> 5) * (BM / WM) + tm * 32 + (sr & 31);
        const int irow = POLY ? (trow / BMJ) * RJ + trow % BMJ + (taps - 1) / 2 : trow + pad;
#pragma unroll
        for (int q = 0; q < G::VPL; ++q) {
          const int col = (lc + q * G::LPR) * 4;
          const half4 hi = *reinterpret_cast<const half4*>(img + irow * RS + IMG_HI + col * 2);
          const half4 lo = *reinterpret_cast<const half4*>(img + irow * RS + IMG_LO + col * 2);
          rpre[(tm * G::NSTEP + st) * G::VPL + q] = make_float4((float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1],
                                                                (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]);
        }
      }
    epilogue<BM, C, WM, WN, true, false, true, false, ResRows<BM, PH, POLY>, true>(
        acc, p, smem, __builtin_ldexpf(1.0f, -p.w_shift), ResRows<BM, PH, POLY>{m0, jb, pb, dil, T}, blockIdx, gridDim.y, rpre);
  } else {
    epilogue<BM, C, WM, WN, true, false, true, false>(acc, p, smem, __builtin_ldexpf(1.0f, -p.w_shift),
                                                      ResRows<BM, PH, POLY>{m0, jb, pb, dil, T}, blockIdx, gridDim.y);
  }
#ifdef ASW_PHASE_TIMING
  {
    const unsigned long long t_end = __builtin_readcyclecounter();
    if (threadIdx.x == 0) {
      atomicAdd(&g_phase_cycles[0], t_stage);
      atomicAdd(&g_phase_cycles[1], t_loop);
      atomicAdd(&g_phase_cycles[2], t_end - t_epi0);
      atomicAdd(&g_phase_cycles[3], 1ull);
    }
    (void)t_begin;
  }
#endif
}

template <int BM, int C, int WM, int WN, int PH, int QD = 4, bool POLY = (PH > 1), bool GLU = false>
int launch_res(const asw_convgemm_args& a, hipStream_t s) {
  constexpr int BMJ = BM / PH;
  const int RJ = BMJ + (!POLY ? (a.taps - 1) * a.dil : a.taps - 1);
  const size_t img = (size_t)PH * RJ * RS;
  const size_t slab = (size_t)(WM * 32) * (C + 4) * sizeof(float);
  const size_t smem = img > slab ? img : slab;
  if (smem > 160 * 1024) return 1;                     // caller falls back to the generic kernel
  const int gx = !POLY ? asw::cdiv(a.M_out, BM)
                       : asw::cdiv(asw::cdiv(a.M_out, a.dil), BMJ) * asw::cdiv(a.dil, PH);
  char nm[96];
  snprintf(nm, sizeof nm, "resconv16<%d,%d,%s%d%s%s>", BM, C, POLY ? "poly" : "ph", PH, QD == 2 ? ",q2" : "", GLU ? ",glu" : "");
  asw_convgemm_args k = a;
  // C > 64: the image holds one 64-channel slice at a time, so the residual (= the normalised input) is read back
  // from glu_out: the rows a workgroup reads in its epilogue are the ones it stored while staging (same CU, after
  // the barriers of the k-loop)
  if (GLU && C > 64) k.resid = a.glu_out;
  return asw::launch_pair<resconv16_kernel<BM, C, WM, WN, PH, QD, POLY, GLU, 1>, resconv16_kernel<BM, C, WM, WN, PH, QD, POLY, GLU, 3>>(
      a.precision, dim3(gx, 1, a.B), dim3(64 * WM * WN), smem, 160 * 1024, nm, asw::ShapeTag(a, 'd', a.dil).s,
      2.0 * a.B * (double)a.M_out * a.N * (double)a.taps * a.Cin, 0.0, s, k);
}

}  // namespace

#ifdef ASW_PHASE_TIMING
extern "C" int asw_debug_phase_cycles(unsigned long long* out4, int reset) {
  ASW_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_phase_cycles), 4 * sizeof(unsigned long long)));
  if (reset) {
    const unsigned long long z[4] = {0, 0, 0, 0};
    ASW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof z));
  }
  return ASW_OK;
}
#endif

namespace asw {
// returns 1 when the layer is not a halo-kernel case (or does not fit LDS)
int try_resconv(const asw_convgemm_args& a, hipStream_t s) {
  const bool shape = a.precision >= 1 && a.Wf_hi && a.Wf_lo && a.ln_gamma && a.stride == 1 && a.taps > 1 &&
                     a.taps % 2 == 1 && a.Cin == a.N && a.a_row_stride == a.Cin && a.resid == a.A && !a.A2 &&
                     !a.mul && !a.stats && a.pad * 2 == (a.taps - 1) * a.dil &&
                     a.a_len == (int64_t)a.M_out * a.Cin && a.a_batch_stride == a.a_len;
  if (!shape) return 1;
  if (a.glu_raw) {
    ASW_CHECK_ARG(a.dil == 1 && a.glu_mr && a.glu_gamma && a.glu_beta,
                  "convgemm: GroupNorm + GLU on load needs dilation 1 and the statistics / affine arrays");
    ASW_CHECK_ARG(a.N == 64 || a.glu_out, "convgemm: GroupNorm + GLU on load at %d channels takes the residual from glu_out", a.N);
  }
  // large dilation: polyphase row sets -- but only while every phase still fills a 32-row
  // MFMA tile; on short sequences (T/dil < 32, e.g. T = 752 at dil 49) most of each tile
  // would be empty (measured: 141 vs 243 TFLOP/s), so those stay contiguous
  const int rows_per_phase = a.M_out / a.dil;
  const bool poly = a.dil >= 16 && rows_per_phase >= 32;
  // Tile / prefetch choices are measured (tests/perf_layers.py, T = 48 000, batch 64):
  //  C = 64  : waves 2x2 (64 rows x 32 columns each) halves the weight fragments every wave
  //            pulls through L1 compared with 4x1 -> 222 -> 257 TFLOP/s.  (A persistent variant
  //            with the weights stationary in registers, 224 VGPRs per wave, was tried: one wave
  //            per SIMD leaves the LDS reads of the A operand exposed -> 160 TFLOP/s.);
  //  C = 128 : B prefetch depth 2 fits 3 waves/SIMD -> 294 -> 312 TFLOP/s (dil 49: 259 -> 279);
  //  C = 256 : depth 4 and depth 2 tied in round 1; with the A fragments double buffered depth 2
  //            (3 waves/SIMD) is 1-2 % ahead (322 -> 325, dilation 49: 298 -> 305);
  //  C = 512 : depth 2 fits 2 workgroups per CU -> 346 -> 366 TFLOP/s, except dilation 49 whose
  //            contiguous halo image (294 extra rows) leaves room for one workgroup anyway.
  // Also measured and dropped: 8-wave 128-row tiles for C >= 256 (305 vs 368), and a persistent
  // variant that double-buffers the image slices (prefetch under the MFMAs, one barrier per
  // slice): 338 vs 330 at C = 256 but 146 vs 239 where the doubled image costs a resident
  // workgroup.  With the epilogue removed the same loops run at 355-385 TFLOP/s, the level of an
  // idealised k-step loop fed from L2 on random data (tests/micro/cu_probe.hip: 400).
  switch (a.N) {
    // Dilation 49 as polyphase dilation-1 convolutions, PH phases per workgroup (measured at
    // T = 48 000, batch 64, TFLOP/s for PH = 1 / 2 / 4): C = 64: 243 / 238 / 205; C = 128: 292 / 307 /
    // 282; C = 256: 300 / 301 / -.  Fewer phases per workgroup mean fewer halo rows in the image
    // (134 / 140 / 152 rows for 128 outputs) and longer runs of one phase -- as long as a phase
    // (M_out / dil rows) still fills the BM / PH rows the workgroup gives it.
    // Round 2 also measured, for C = 64: 256-row tiles with 4 x 1 waves (221 vs 262 TFLOP/s at
    // dilation 1), 2 waves of 128 x 64 (155) and 8 waves 4 x 2 on 256 rows (same wave tile, weight
    // fragments shared by four waves through L1: 266 vs 268): neither LDS, L2 nor the weight path
    // is the limit.  Cycle counters per phase (tests/micro/phase_timing.py): a workgroup spends 16 %
    // staging, 40 % in the k-loop, 44 % in the epilogue; taking the residual from the LDS image
    // instead of global memory and budgeting registers for 4 waves per SIMD gave +3 %.
    case 64:
      // at C = 64 even dilation 7 is better off as 7 single-phase tiles (halo 6 instead of 42 rows per
      // 128 outputs, image 36 instead of 46 KB -> 4 resident workgroups): 238 -> 257 TFLOP/s
      if (a.glu_raw) return launch_res<128, 64, 2, 2, 1, 4, false, true>(a, s);
      if (a.dil >= 7 && a.dil < 16 && rows_per_phase >= 96) return launch_res<128, 64, 2, 2, 1, 4, true>(a, s);
      if (!poly) return launch_res<128, 64, 2, 2, 1>(a, s);
      if (rows_per_phase >= 96) return launch_res<128, 64, 2, 2, 1, 4, true>(a, s);
      return rows_per_phase >= 48 ? launch_res<128, 64, 2, 2, 2>(a, s) : launch_res<128, 64, 2, 2, 4>(a, s);
    case 128:
      if (a.glu_raw) return launch_res<128, 128, 2, 2, 1, 2, false, true>(a, s);
      if (!poly) return launch_res<128, 128, 2, 2, 1, 2>(a, s);
      return rows_per_phase >= 48 ? launch_res<128, 128, 2, 2, 2, 2>(a, s) : launch_res<128, 128, 2, 2, 4, 2>(a, s);
    case 256: {
      // 128-row tiles (wave tile 128 x 64: half the weight-fragment traffic per MFMA, two waves per SIMD
      // instead of three) once they still fill the chip twice over: 313 -> 335 TFLOP/s at T = 48 000,
      // batch 64 (same box).  The same step at C = 128 (256-row tiles) loses, 300 -> 292.
      if (a.glu_raw)
        return (long)asw::cdiv(a.M_out, 128) * a.B >= 512 ? launch_res<128, 256, 1, 4, 1, 2, false, true>(a, s)
                                                          : launch_res<64, 256, 1, 4, 1, 2, false, true>(a, s);
      if (!poly && (long)asw::cdiv(a.M_out, 128) * a.B >= 512) return launch_res<128, 256, 1, 4, 1, 2>(a, s);
      // (polyphase, two phases of 64 rows: 302 -> 307)
      if (poly && rows_per_phase >= 48 && (long)asw::cdiv(a.M_out, 128) * a.B >= 512) return launch_res<128, 256, 1, 4, 2, 2>(a, s);
      return poly ? launch_res<64, 256, 1, 4, 2, 2>(a, s) : launch_res<64, 256, 1, 4, 1, 2>(a, s);
    }
    case 512:
      // polyphase at C = 512 pays only for long phases: 45 rows per phase (T = 144 000) measured 243
      // TFLOP/s against 307 for the contiguous halo image on the same layer shape at T = 48 000
      if (a.glu_raw) return launch_res<64, 512, 1, 4, 1, 2, false, true>(a, s);
      if (poly && a.M_out / a.dil >= 64) return launch_res<64, 512, 1, 4, 2>(a, s);
      return a.dil >= 16 ? launch_res<64, 512, 1, 4, 1>(a, s) : launch_res<64, 512, 1, 4, 1, 2>(a, s);
    default: return 1;
  }
}
}  // namespace asw
