// convgemm.hip -- 1-D conv / transposed conv / linear as implicit GEMM on the gfx950
// matrix cores, with the layer's element-wise tail fused into the epilogue.
//
// Replaces (reference file:line): DilatedResidualLayer conv+ReLU+residual+LayerNorm
// (sep/training/SpeakerLocalization/network.py:57-68), EncoderBlock.conv1
// (:105-108), UpsamplerBlock ConvTranspose1d (:158-165,190), mask_encoder /
// reference_bypass / output_decoder contraction (:327-349,397-402) and the
// transformer linears (:254).
//
// Layout: activations channels-last [B][T][C] fp32, weights Wt[N][K] with
// K = tap*Cin + c.  One workgroup (4 waves, 8 for the 256-row f16x3 tiles) owns a BM x BN
// output tile of one batch item; K is walked in chunks of BK channels of one tap.  A and W
// chunks are staged global -> registers -> LDS (activations through a buffer descriptor, so
// padding costs no branch), the next chunk's global loads are in flight while the MFMAs of
// the current chunk run.  The 30 dilated residual layers have their own halo-staged kernel
// (resconv16_kernel, resconv.hip).
//
// Two arithmetic modes share the tiling and the epilogue:
//  * precision 0: v_mfma_f32_32x32x2_f32 -- an exact fp32 fmaf chain (64 FLOP/clk/SIMD).
//    Lane l supplies A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31]; a lane reads 4 consecutive
//    k (one ds_read_b128) and step s of 4 uses element s of both operands, i.e. the k
//    order is permuted identically for A and B.  LDS rows are padded to BK+4 floats so
//    those reads are bank-conflict free.
//  * precision 1 ("f16x3"): every fp32 operand is split into two halves hi = fp16(x),
//    lo = fp16(x - hi) and the product is lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_f16
//    with fp32 accumulation: operands carry ~21 bits, the dropped lo*lo term is 2^-22 of the
//    product, and the pipe nominally runs 16/3 = 5.3x the f32 MFMA rate (measured on random
//    operands: 1.63 PFLOP/s of f16 MFMA sustained, tests/micro/cu_probe.hip).  Activations are split while
//    they are staged to LDS (saturating at +-65504); weights are split once on the host,
//    pre-scaled by a power of two (undone in the epilogue) so their lo parts stay out of the
//    fp16 subnormal range.  Lane l supplies A[l&31][8(l>>5)+j], j<8: one ds_read_b128 per
//    operand half per k-step; rows padded to BK+8 halves (conflict free).
//
// The epilogue all kernels share is in gemm_epilogue.h.
#include "gemm_epilogue.h"

namespace {
using namespace asw_mfma;

#ifdef ASW_PHASE_TIMING
// Diagnostic build only (tests/micro/phase_timing.py), cycles of wave 0 summed over workgroups:
// generic 256x256 f16x3 GEMM: [0] waiting at the first barrier of a chunk, [1] register -> LDS deposit
// + second barrier, [2] global loads of the next chunk + fragment reads + MFMAs, [3] epilogue, [4] workgroups
__device__ unsigned long long g_gemm_cycles[5] = {0, 0, 0, 0, 0};
#endif

// address of the float4 of A this thread stages for chunk kc (or -1 when it is padding)
template <int BM, int BK>
__device__ __forceinline__ long a_elem(const asw_convgemm_args& p, int idx, int kc, int cpb, int m0) {
  constexpr int KV = BK / 4;
  const int tap = kc / cpb;
  const int c0 = (kc - tap * cpb) * BK;
  const int row = idx / KV, cv = idx - row * KV;
  const int t_out = m0 + row;
  const long e = ((long)t_out * p.stride + (long)tap * p.dil - p.pad) * p.a_row_stride + c0 + cv * 4;
  const bool ok = (idx < BM * KV) && (t_out < p.M_out) && (e >= 0) && (e + 3 < p.a_len);
  return ok ? e : -1;
}

// ------------------------------------------------------------------ exact fp32 MFMA
template <int BM, int BN, int BK, int WM, int WN, bool LN, bool STATS, bool MUL, bool A2F>
__global__ __launch_bounds__(256) void convgemm_kernel(const asw_convgemm_args p) {
  static_assert(WM * WN == 4, "4 waves per workgroup");
  constexpr int LDK = BK + 4;
  constexpr int KV = BK / 4;                 // float4 per staged row
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int A_VEC = (BM * KV + 255) / 256, B_VEC = (BN * KV + 255) / 256;

  extern __shared__ __align__(16) float smem[];
  float* As = smem;
  float* Bs = smem + BM * LDK;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int b = blockIdx.z, m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int K = p.taps * p.Cin;
  const int cpb = p.Cin / BK;                // chunks per tap
  const int nk = p.taps * cpb;
  const float* __restrict__ Ab = p.A + (long)b * p.a_batch_stride;
  const float* __restrict__ A2b = p.A2 ? p.A2 + (long)b * p.a_batch_stride : nullptr;

  float4 ra[A_VEC], rb[B_VEC];
  const __amdgpu_buffer_rsrc_t rA = act_rsrc(Ab, p.a_len);
  const __amdgpu_buffer_rsrc_t rA2 = act_rsrc(A2F ? A2b : Ab, p.a_len);

  // The skip-connection operand is a compile-time variant (no runtime "load or zero" branch).
  auto gload = [&](int kc) {
#pragma unroll
    for (int v = 0; v < A_VEC; ++v) {
      const long e = a_elem<BM, BK>(p, tid + v * 256, kc, cpb, m0);
      float4 x = act_load4(rA, e, e >= 0);
      if (A2F) {
        const float4 y = act_load4(rA2, e, e >= 0);
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
      }
      ra[v] = x;
    }
#pragma unroll
    for (int v = 0; v < B_VEC; ++v) {
      const int idx = tid + v * 256;
      const int row = idx / KV, cv = idx - row * KV;
      const bool ok = idx < BN * KV;
      const float4 x = *reinterpret_cast<const float4*>(p.Wt + (long)(n0 + (ok ? row : 0)) * K + (long)kc * BK + cv * 4);
      rb[v] = ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int v = 0; v < A_VEC; ++v) {
      const int idx = tid + v * 256;
      const int row = idx / KV, cv = idx - row * KV;
      if (idx < BM * KV) *reinterpret_cast<float4*>(As + row * LDK + cv * 4) = ra[v];
    }
#pragma unroll
    for (int v = 0; v < B_VEC; ++v) {
      const int idx = tid + v * 256;
      const int row = idx / KV, cv = idx - row * KV;
      if (idx < BN * KV) *reinterpret_cast<float4*>(Bs + row * LDK + cv * 4) = rb[v];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const float* a_rd = As + (wm * (BM / WM) + (lane & 31)) * LDK + (lane >> 5) * 4;
  const float* b_rd = Bs + (wn * (BN / WN) + (lane & 31)) * LDK + (lane >> 5) * 4;

  gload(0);
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();                  // previous chunk's fragment reads are done
    lstore();
    __syncthreads();
    if (kc + 1 < nk) gload(kc + 1);   // in flight under the MFMAs below
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(a_rd + i * 32 * LDK + kk * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(b_rd + j * 32 * LDK + kk * 8);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float a = s == 0 ? af[i].x : s == 1 ? af[i].y : s == 2 ? af[i].z : af[i].w;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float bb = s == 0 ? bf[j].x : s == 1 ? bf[j].y : s == 2 ? bf[j].z : bf[j].w;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }
  epilogue<BM, BN, WM, WN, LN, STATS, LN, MUL>(acc, p, smem, 1.0f, RowsContig{m0, p.M_out}, blockIdx, gridDim.y);
}

// ------------------------------------------------------------------ f16x3 split MFMA
// Four-wave tiles whose LDS footprint lets three workgroups share a CU get a register budget for
// three waves per SIMD (hipcc otherwise spends ~180 VGPRs -> two): these are the small-K, write- and
// latency-bound layers, which gain from the third resident workgroup (128x128 tiles: strided conv
// 211 -> 242, transformer linears 232 -> 269 TFLOP/s, K = 64 / 128 transposed convs +15-20 %).
// (The 8-wave 256x128 tile squeezed into 128 VGPRs for two workgroups per CU spills and loses:
// mask encoder 293 vs 312 TFLOP/s on 256x256; 128x256 with four waves, i.e. two independent
// workgroups per CU whose deposit phases could overlap the other's MFMAs: 314 vs 310, a tie.
// Cycle counters on the 256x256 mask-encoder tile (tests/micro/phase_timing.py): per 32-wide chunk
// wave 0 spends 1900 cycles waiting at the first barrier (its SIMD mate is still multiplying), 1150
// depositing the next chunk and 2240 on loads + fragment reads + 48 MFMAs; epilogue 11 % of the tile.)
template <int BM, int BN, int BK, int WM, int WN>
constexpr int g16_waves_per_eu() {
  constexpr long stage = (long)(BM + BN) * (BK + 8) * 2 * 2, slab = (long)(WM * 32) * (BN + 4) * 4;
  if (WM * WN == 4 && (stage > slab ? stage : slab) <= 80 * 1024 && (stage > slab ? stage : slab) > 53 * 1024) return 2;
  return (WM * WN == 4 && (stage > slab ? stage : slab) <= 53 * 1024) ? 3 : 1;
}
template <int BM, int BN, int BK, int WM, int WN, bool LN, bool STATS, bool MUL, bool A2F, int NTERM = 3>
__global__ __launch_bounds__(64 * WM * WN)
__attribute__((amdgpu_waves_per_eu(g16_waves_per_eu<BM, BN, BK, WM, WN>())))
void convgemm16_kernel(const asw_convgemm_args p) {
  static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 waves per workgroup");
  static_assert(BK % 16 == 0, "k-step of the f16 MFMA");
  constexpr int NT = 64 * WM * WN;           // threads
  constexpr int LDH = BK + 8;                // halves per staged row
  constexpr int KH = BK / 8;                 // 16-byte vectors (B, fp16) per row
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int B_VEC = (BN * KH + NT - 1) / NT;

  extern __shared__ __align__(16) float smem[];
  _Float16* Ah = reinterpret_cast<_Float16*>(smem);
  _Float16* Al = Ah + BM * LDH;
  _Float16* Bh = Al + BM * LDH;
  _Float16* Bl = Bh + BN * LDH;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int ncol = p.N / BN, nrt = (p.M_out + BM - 1) / BM;
  uint3 tl;
  if (!xcd_tile_groups(p.B, nrt, ncol, tl)) return;           // XCD-aware order, groups of 8
  const dim3 tile(tl.x, tl.y, tl.z);
  const int b = tile.z, m0 = tile.x * BM, n0 = tile.y * BN;
  const int K = p.taps * p.Cin;
  const int nk = p.taps * (p.Cin / BK);
  const _Float16* __restrict__ Wh = reinterpret_cast<const _Float16*>(p.Wt_hi);
  const _Float16* __restrict__ Wl = reinterpret_cast<const _Float16*>(p.Wt_lo);

  // One staging register set (a second set, i.e. loads two chunks ahead, was measured: no
  // gain, and its 64 extra VGPRs cost a resident workgroup per CU).
  ChunkedA<BM, BK, NT, A2F> A(p, b, m0, tid);
  half8 rbh0[B_VEC], rbl0[B_VEC];

  // per-thread invariants of the weight staging addresses
  long b_row[B_VEC];
  bool b_ok[B_VEC];
#pragma unroll
  for (int v = 0; v < B_VEC; ++v) {
    const int idx = tid + v * NT;
    const int row = idx / KH, cv = idx - row * KH;
    b_row[v] = (long)(n0 + row) * K + cv * 8;
    b_ok[v] = (idx < BN * KH) && (n0 + row < p.N);
  }

  auto gload = [&](int kc, half8 (&rbh)[B_VEC], half8 (&rbl)[B_VEC]) {
    A.load(kc);
#pragma unroll
    for (int v = 0; v < B_VEC; ++v) {
      const long o = (b_ok[v] ? b_row[v] : 0) + (long)kc * BK;
      rbh[v] = *reinterpret_cast<const half8*>(Wh + o);   // rows past BN*KH are never stored to LDS
      if (NTERM == 3) rbl[v] = *reinterpret_cast<const half8*>(Wl + o);
    }
  };
  auto lstore = [&](const half8 (&rbh)[B_VEC], const half8 (&rbl)[B_VEC]) {
    A.template deposit<NTERM>(Ah, Al);
#pragma unroll
    for (int v = 0; v < B_VEC; ++v) {
      const int idx = tid + v * NT;
      const int row = idx / KH, cv = idx - row * KH;
      if (idx < BN * KH) {
        *reinterpret_cast<half8*>(Bh + row * LDH + cv * 8) = rbh[v];
        if (NTERM == 3) *reinterpret_cast<half8*>(Bl + row * LDH + cv * 8) = rbl[v];
      }
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int a_off = (wm * (BM / WM) + (lane & 31)) * LDH + (lane >> 5) * 8;
  const int b_off = (wn * (BN / WN) + (lane & 31)) * LDH + (lane >> 5) * 8;

  auto compute = [&]() {
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      half8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const half8*>(Ah + a_off + i * 32 * LDH + ks * 16);
        if (NTERM == 3) al[i] = *reinterpret_cast<const half8*>(Al + a_off + i * 32 * LDH + ks * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const half8*>(Bh + b_off + j * 32 * LDH + ks * 16);
        if (NTERM == 3) bl[j] = *reinterpret_cast<const half8*>(Bl + b_off + j * 32 * LDH + ks * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma3<NTERM>(acc[i][j], ah[i], al[i], bh[j], bl[j]);
    }
  };

#ifdef ASW_PHASE_TIMING
  unsigned long long tg_wait = 0, tg_store = 0, tg_comp = 0;
#endif
  gload(0, rbh0, rbl0);
  for (int kc = 0; kc < nk; ++kc) {
    ASW_PHASE_MARK(g0);
    __syncthreads();
    ASW_PHASE_MARK(g1);
    lstore(rbh0, rbl0);
    __syncthreads();
    ASW_PHASE_MARK(g2);
    if (kc + 1 < nk) gload(kc + 1, rbh0, rbl0);
    compute();
#ifdef ASW_PHASE_TIMING
    {
      float sink = acc[0][0][0];
      asm volatile("" ::"v"(sink));
      const unsigned long long g3 = __builtin_readcyclecounter();
      tg_wait += g1 - g0; tg_store += g2 - g1; tg_comp += g3 - g2;
    }
#endif
  }
  ASW_PHASE_MARK(ge0);
  epilogue<BM, BN, WM, WN, LN, STATS, LN, MUL>(acc, p, smem, __builtin_ldexpf(1.0f, -p.w_shift), RowsContig{m0, p.M_out}, tile, ncol);
#ifdef ASW_PHASE_TIMING
  if (threadIdx.x == 0 && BM == 256 && BN == 256) {
    const unsigned long long ge1 = __builtin_readcyclecounter();
    atomicAdd(&g_gemm_cycles[0], tg_wait);
    atomicAdd(&g_gemm_cycles[1], tg_store);
    atomicAdd(&g_gemm_cycles[2], tg_comp);
    atomicAdd(&g_gemm_cycles[3], ge1 - ge0);
    atomicAdd(&g_gemm_cycles[4], 1ull);
  }
#endif
}

template <int BM, int BN, int BK, int WM, int WN, bool LN, bool STATS, bool MUL, bool F16, bool A2F = false>
int launch(const asw_convgemm_args& a, hipStream_t s) {
  constexpr size_t stage = F16 ? (size_t)(BM + BN) * (BK + 8) * 2 * sizeof(_Float16)
                               : (size_t)(BM + BN) * (BK + 4) * sizeof(float);
  constexpr size_t slab = (size_t)(WM * 32) * (BN + 4) * sizeof(float);
  constexpr size_t smem = stage > slab ? stage : slab;
  static_assert(smem <= 160 * 1024, "LDS budget");
  ASW_CHECK_ARG(A2F == (a.A2 != nullptr), "convgemm: the skip operand is fused only in the 128-wide statistics tile");
  ASW_CHECK_ARG(a.Cin % BK == 0, "convgemm: Cin=%d not a multiple of BK=%d", a.Cin, BK);
  ASW_CHECK_ARG(a.N % BN == 0, "convgemm: N=%d not a multiple of BN=%d", a.N, BN);
  const int nrt = asw::cdiv(a.M_out, BM), ncol = a.N / BN;
  const std::string pn = asw::prof_name(F16 ? (MUL ? "convgemm16m" : "convgemm16") : (MUL ? "convgemm_m" : "convgemm"),
                                        BM, BN, BK, LN, STATS);
  const asw::ShapeTag tag(a, 's', a.stride);
  const double flops = 2.0 * a.B * (double)a.M_out * a.N * (double)a.taps * a.Cin;
  if constexpr (F16)
    return asw::launch_pair<convgemm16_kernel<BM, BN, BK, WM, WN, LN, STATS, MUL, A2F, 1>,
                            convgemm16_kernel<BM, BN, BK, WM, WN, LN, STATS, MUL, A2F, 3>>(
        a.precision, dim3(xcd_grid_groups((long)nrt * a.B, ncol)), dim3(64 * WM * WN), smem, smem, pn, tag.s, flops, 0.0, s, a);
  else   // exact fp32: one instantiation
    return asw::launch_pair<convgemm_kernel<BM, BN, BK, WM, WN, LN, STATS, MUL, A2F>, convgemm_kernel<BM, BN, BK, WM, WN, LN, STATS, MUL, A2F>>(
        0, dim3(nrt, ncol, a.B), dim3(256), smem, smem, pn, tag.s, flops, 0.0, s, a);
}

template <int BM, int BN, int BK, int WM, int WN, bool LN, bool STATS, bool MUL = false>
int launch_prec(const asw_convgemm_args& a, hipStream_t s) {
  return a.precision >= 1 ? launch<BM, BN, BK, WM, WN, LN, STATS, MUL, true>(a, s)
                          : launch<BM, BN, BK, WM, WN, LN, STATS, MUL, false>(a, s);
}

template <int BM, int BN, int WM, int WN, bool F16>
struct GemmTile {                        // two-barrier kernels: convgemm16 / convgemm, 32-wide chunks
  template <bool STATS, bool MUL, bool A2F>
  static int run(const asw_convgemm_args& a, hipStream_t s) { return launch<BM, BN, 32, WM, WN, false, STATS, MUL, F16, A2F>(a, s); }
};

// tile choice for the non-LayerNorm variants; must match asw_convgemm_stats_tiles
inline bool wide_tile(int N) { return N % 128 == 0; }
// f16x3 only: 2 = 256x256 (8 waves), 0 = 128x128.  The big tile halves the bytes pulled per
// MAC but needs a grid of >= 2 workgroups per CU to stay balanced (measured: mask encoder
// 242 -> 267 TFLOP/s, deep down/up convs 169 -> 201, but the 288-workgroup QKV GEMM is
// faster on 128x128).
// 3 = 192x256: the same 8-wave kernel with three MFMA row tiles per wave, for sequence lengths
// that leave a 256-row tile a quarter or more empty (the bottleneck-side convolutions: 188 rows at
// T = 48 000, 563 at T = 144 000 -> 2 % instead of 27 % of the MFMAs on padding rows).
inline int wide_tile_kind(int B, int M_out, int N, int K) {
  if (M_out <= 128 || N % 256 != 0 || K < 256) return 0;
  const long blocks = (long)asw::cdiv(M_out, 256) * (N / 256) * B;
  if (blocks < 512) return 0;
  const long pad256 = (long)asw::cdiv(M_out, 256) * 256, pad192 = (long)asw::cdiv(M_out, 192) * 192;
  return pad192 * 10 <= pad256 * 9 ? 3 : 2;                  // at least 10 % fewer padded rows
}

}  // namespace

#ifdef ASW_PHASE_TIMING
extern "C" int asw_debug_gemm_cycles(unsigned long long* out5, int reset) {
  ASW_HIP(hipMemcpyFromSymbol(out5, HIP_SYMBOL(g_gemm_cycles), 5 * sizeof(unsigned long long)));
  if (reset) {
    const unsigned long long z[5] = {0, 0, 0, 0, 0};
    ASW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_cycles), z, sizeof z));
  }
  return ASW_OK;
}
#endif

namespace asw {
int try_resconv(const asw_convgemm_args& a, hipStream_t s);          // resconv.hip
int pipe_gemm(const asw_convgemm_args& a, hipStream_t s);            // pipegemm.hip
int try_downconv64(const asw_convgemm_args& a, hipStream_t s);       // downconv.hip
int pipegemm_f16x3_overflow(int reset, unsigned int* count);
int convgemm_f16x3_overflow(int reset, unsigned int* count) { return f16x3_overflow_read(reset, count); }
}  // namespace asw

// the two translation units that write a range-guard counter (gemm_epilogue.h)
extern "C" int asw_f16x3_overflow_count(int reset, uint32_t* count) {
  ASW_CHECK_ARG(count != nullptr, "f16x3_overflow_count: null pointer");
  unsigned int here = 0, pipe = 0;
  if (int rc = asw::convgemm_f16x3_overflow(reset, &here)) return rc;
  if (int rc = asw::pipegemm_f16x3_overflow(reset, &pipe)) return rc;
  *count = here + pipe;
  return ASW_OK;
}

extern "C" int asw_convgemm_stats_tiles(int M_out, int N) {
  // upper bound over the tile choices of both precisions (the smallest tiles)
  if (wide_tile(N)) return asw::cdiv(M_out, 128) * (N / 128);
  return asw::cdiv(M_out, 256) * (N / 64);
}

extern "C" int asw_convgemm_f32(const asw_convgemm_args* args, void* stream) {
  ASW_CHECK_ARG(args != nullptr, "convgemm: null args");
  asw_convgemm_args a = *args;
  hipStream_t s = asw::as_stream(stream);
  if (a.stats) {
    a.stats_stride = asw_convgemm_stats_tiles(a.M_out, a.N);
    ASW_HIP(hipMemsetAsync(a.stats, 0, (size_t)a.B * a.stats_stride * 4 * sizeof(float), s));
  }
  ASW_CHECK_ARG(a.A && a.out, "convgemm: null tensor");
  ASW_CHECK_ARG(a.precision >= 0 && a.precision <= 3, "convgemm: precision %d", a.precision);
  if (a.precision >= 1) ASW_CHECK_ARG(a.Wt_hi && a.Wt_lo, "convgemm: the f16 modes need Wt_hi/Wt_lo");
  else ASW_CHECK_ARG(a.Wt != nullptr, "convgemm: null weights");
  ASW_CHECK_ARG(a.B > 0 && a.M_out > 0 && a.N > 0 && a.Cin > 0 && a.taps > 0, "convgemm: bad dims");
  ASW_CHECK_ARG(a.a_len > 0 && a.a_len < (int64_t)1 << 29, "convgemm: a_len=%lld per batch item exceeds the 2 GiB buffer descriptor",
                (long long)a.a_len);
  ASW_CHECK_ARG(a.a_row_stride % 4 == 0 && a.a_batch_stride % 4 == 0 && a.a_len % 4 == 0 && a.Cin % 8 == 0,
                "convgemm: strides must be multiples of 4 floats, Cin of 8");
  ASW_CHECK_ARG(a.B <= 65535, "convgemm: batch %d exceeds grid.z", a.B);
  const bool stats = a.stats != nullptr;
  if (stats) ASW_CHECK_ARG(a.chan_mod >= 2 && a.chan_mod % 2 == 0, "convgemm: stats need even chan_mod");
  ASW_CHECK_ARG(!(a.resid && !a.ln_gamma), "convgemm: a residual is fused only together with LayerNorm");
  ASW_CHECK_ARG(!(a.mul && (a.ln_gamma || stats || !wide_tile(a.N))),
                "convgemm: the gate tensor is fused only in the plain 128-wide tile");
  if (a.ln_gamma) {
    ASW_CHECK_ARG(a.ln_beta != nullptr && a.resid != nullptr, "convgemm: LayerNorm needs beta and a residual");
    ASW_CHECK_ARG(!stats, "convgemm: LayerNorm + stats epilogue is not a reference layer");
    {
      const int rc = asw::try_resconv(a, s);             // the halo-staged residual layer (resconv.hip)
      if (rc != 1) return rc;
    }
    ASW_CHECK_ARG(!a.glu_raw, "convgemm: GroupNorm + GLU on load exists only in the halo-staged f16x3 layer "
                              "(C_in == N == 64, dilation 1, fragment-order weights)");
    switch (a.N) {
      case 64: return launch_prec<256, 64, 32, 4, 1, true, false>(a, s);
      case 128: return launch_prec<128, 128, 32, 2, 2, true, false>(a, s);
      case 256: return launch_prec<64, 256, 32, 1, 4, true, false>(a, s);
      case 512: return launch_prec<64, 512, 16, 1, 4, true, false>(a, s);
      case 1024: return launch_prec<32, 1024, 16, 1, 4, true, false>(a, s);
      default:
        return asw::set_error(ASW_ERR_ARG, "convgemm: LayerNorm width %d unsupported (64..1024, power of 2)", a.N);
    }
  }
  ASW_CHECK_ARG(!a.glu_raw, "convgemm: GroupNorm + GLU on load belongs to a residual layer (LayerNorm + residual)");
  {
    const int rc = asw::try_downconv64(a, s);          // stride-2 convolutions of a 64-channel input (downconv.hip)
    if (rc != 1) return rc;
  }
  if (wide_tile(a.N)) {
    if (a.precision >= 1) {
      // f16x3 is bound by the bytes each CU can pull per cycle, so take the largest tile the
      // shape fills: 256x256 or 192x256 (8 waves, 1/32 B per MAC), else 128x128 (1/16 B per MAC)
      const int t = wide_tile_kind(a.B, a.M_out, a.N, a.taps * a.Cin);
      // (192-row tiles, i.e. a single row tile per item and a long K, stay on the two-barrier kernel:
      // with so little reuse of a weight fragment the global B path loses, 296 vs 322 TFLOP/s)
      if (a.Wf_hi && a.Wf_lo && t == 2 && (a.taps * a.Cin) % 16 == 0 && a.N % 32 == 0 && asw::pipe_offsets_ok(a))
        return asw::pipe_gemm(a, s);                                                                  // pipegemm.hip
      if (t == 3) return launch_variant<GemmTile<192, 256, 2, 4, true>>(a, s);
      if (t == 2) return launch_variant<GemmTile<256, 256, 2, 4, true>>(a, s);
      return launch_variant<GemmTile<128, 128, 2, 2, true>>(a, s);
    }
    return launch_variant<GemmTile<128, 128, 2, 2, false>>(a, s);
  }
  ASW_CHECK_ARG(a.N % 64 == 0, "convgemm: N=%d must be a multiple of 64", a.N);
  return stats ? launch_prec<256, 64, 32, 4, 1, false, true>(a, s) : launch_prec<256, 64, 32, 4, 1, false, false>(a, s);
}
