// gemm_epilogue.h -- what the row-major GEMM kernels of convgemm.hip, pipegemm.hip and resconv.hip share.
//
// Epilogue: the accumulators of one 32-row slab are written to LDS (C/D map:
// col = lane&31, row = acc_row(r, lane>>5), mfma_util.h), then each wave owns whole
// rows: + residual, * gate tensor, LayerNorm over the row (two-pass, wave shuffles),
// GroupNorm partial sums, coalesced row stores.
#pragma once
#include "asw_common.h"
#include "f16x3_tile.h"

namespace asw_mfma {

// f16x3 range guard.  In the f16x3 mode activations are split into fp16 halves while they are
// staged, which saturates at +-65504.  Every tensor a GEMM reads is either normalised
// (LayerNorm / GroupNorm output, bounded by |gamma| sqrt(C) + |beta|) or the un-normalised output
// of a plain epilogue (the masked latent, the feed-forward intermediate).  The plain epilogue
// therefore counts, in f16x3 mode, the threads that wrote a value beyond the fp16 range;
// asw_f16x3_overflow_count() reads the counter.  Zero on every test and bench run with seeded
// weights; a non-zero count means the next GEMM clipped its input and the f32 or the f16x3_safe mode must be used.
// In the f16x3_safe mode (model_common.h, Trunk::site) the un-normalised tensors are read by exact f32 kernels only;
// its split GEMMs run under per-call precision 3, where the guard counts non-finite values alone.
//
// There is no relocatable device code, so every translation unit that includes this header has a counter of its
// own.  convgemm.hip and pipegemm.hip write theirs and export an accessor over f16x3_overflow_read();
// asw_f16x3_overflow_count() adds the two.  resconv.hip instantiates the epilogue with LayerNorm only, where `guard`
// is constant false: its copy is never written and is not part of the sum.
static __device__ unsigned int g_f16x3_overflow = 0;

// this translation unit's count; `reset` clears it
[[maybe_unused]] static int f16x3_overflow_read(int reset, unsigned int* count) {
  unsigned int v = 0;
  ASW_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_f16x3_overflow), sizeof v));      // waits for the device
  if (reset && v) {
    const unsigned int z = 0;
    ASW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_f16x3_overflow), &z, sizeof z));
  }
  *count = v;
  return ASW_OK;
}

// ASW_PHASE_TIMING: diagnostic builds only (tests/micro/phase_timing.py); the cycle counters live with their kernels
#ifdef ASW_PHASE_TIMING
#define ASW_PHASE_MARK(var) const unsigned long long var = __builtin_readcyclecounter()
#else
#define ASW_PHASE_MARK(var)
#endif
// ------------------------------------------------------------------ shared epilogue
// tile row -> output row of the batch item (or -1): contiguous tiles
struct RowsContig {
  int m0, M;
  __device__ __forceinline__ int operator()(int trow) const { const int t = m0 + trow; return t < M ? t : -1; }
};

// Row-phase geometry of the epilogue: a row is BN/4 float4; LPR lanes share a row (RPI rows per
// wave instruction, VPL float4 per lane); each wave walks its share of a WM*32-row slab in NSTEP steps.
template <int BN, int WM, int WN>
struct EpiGeom {
  static constexpr int NW = WM * WN;
  static constexpr int LPR = (BN / 4 < 64) ? BN / 4 : 64;
  static constexpr int RPI = 64 / LPR;
  static constexpr int VPL = BN / 4 / LPR;
  static constexpr int NSTEP = WM * 32 / (NW * RPI);
};

template <int BM, int BN, int WM, int WN, bool LN, bool STATS, bool RESID, bool MUL, typename RowMap, bool RESPRE = false>
__device__ __forceinline__ void epilogue(  // WM*WN waves (4 or 8)
floatx16 (&acc)[BM / WM / 32][BN / WN / 32], const asw_convgemm_args& p,
                                         float* smem, float acc_scale, const RowMap& rowmap, const dim3 tile, const int ncol,
                                         const float4* rpre = nullptr) {
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int LDC = BN + 4;
  float* Ct = smem;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int b = tile.z, n0 = tile.y * BN;
  float st0 = 0.f, sq0 = 0.f, st1 = 0.f, sq1 = 0.f;
  const int half_mod = p.chan_mod >> 1;
  const bool guard = !LN && !STATS && p.precision >= 1;       // un-normalised output that a later f16 GEMM may read
  float amax = 0.f;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int col = wn * (BN / WN) + tn * 32 + (lane & 31);
      const float bv = p.bias ? p.bias[n0 + col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 + acc_row(r, lane >> 5);
        float v = acc[tm][tn][r] * acc_scale + bv;
        if (p.relu == 1) v = fmaxf(v, 0.f);
        else if (p.relu == 2) v = v / (1.0f + expf(-v));             // Swish (Conformer feed-forward)
        Ct[row * LDC + col] = v;
      }
    }
    __syncthreads();
    // Row phase.  A row is BN/4 float4; LPR lanes share a row (RPI rows per wave
    // instruction, VPL float4 per lane), so each wave walks its 8*WM slab rows in 8 steps.
    // Steps are processed four at a time with every global load (residual / gate tensor)
    // issued before the first use: the loads of four steps overlap instead of serialising.
    using G = EpiGeom<BN, WM, WN>;
    constexpr int NW = G::NW, LPR = G::LPR, RPI = G::RPI, VPL = G::VPL;
    constexpr int NSTEP = G::NSTEP;                    // steps each wave needs for its slab rows
    constexpr int UNR = NSTEP < 4 ? NSTEP : 4;
    static_assert(NSTEP >= 1 && NSTEP % UNR == 0 && WM * 32 == NSTEP * NW * RPI, "slab rows must split evenly");
    const int sub = lane / LPR, lc = lane % LPR;
#pragma unroll
    for (int it0 = 0; it0 < NSTEP; it0 += UNR) {
      float4 v[UNR][VPL];
      long obase[UNR];
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int sr = ((it0 + u) * NW + wid) * RPI + sub;
        const int trow = (sr >> 5) * (BM / WM) + tm * 32 + (sr & 31);
        const int t_out = rowmap(trow);
        ok[u] = t_out >= 0;
        // rows past the end read row 0 (always valid) and are simply not stored: the loads
        // stay unconditional, so the compiler issues the whole batch before the first wait
        obase[u] = ((long)b * p.M_out + (ok[u] ? t_out : 0)) * p.N + n0;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int col = (lc + q * LPR) * 4;
          if (RESID && RESPRE) v[u][q] = rpre[(tm * NSTEP + it0 + u) * VPL + q];     // residual taken from the LDS image
          else if (RESID) v[u][q] = *reinterpret_cast<const float4*>(p.resid + obase[u] + col);
          if (MUL) v[u][q] = *reinterpret_cast<const float4*>(p.mul + obase[u] + col);
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int sr = ((it0 + u) * NW + wid) * RPI + sub;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
          const int col = (lc + q * LPR) * 4;
          const float4 x = *reinterpret_cast<const float4*>(Ct + sr * LDC + col);
          if (RESID) { v[u][q].x += x.x; v[u][q].y += x.y; v[u][q].z += x.z; v[u][q].w += x.w; }
          else if (MUL) { v[u][q].x *= x.x; v[u][q].y *= x.y; v[u][q].z *= x.z; v[u][q].w *= x.w; }
          else v[u][q] = x;
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (LN) {
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < VPL; ++q) s += (v[u][q].x + v[u][q].y) + (v[u][q].z + v[u][q].w);
#pragma unroll
          for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
          const float mean = s * (1.0f / BN);
          float d = 0.f;
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            const float cx = v[u][q].x - mean, cy = v[u][q].y - mean, cz = v[u][q].z - mean, cw = v[u][q].w - mean;
            d += (cx * cx + cy * cy) + (cz * cz + cw * cw);
          }
#pragma unroll
          for (int o = LPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
          const float rstd = 1.0f / sqrtf(d * (1.0f / BN) + p.ln_eps);
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            const int col = (lc + q * LPR) * 4;
            const float4 g = *reinterpret_cast<const float4*>(p.ln_gamma + col);
            const float4 be = *reinterpret_cast<const float4*>(p.ln_beta + col);
            v[u][q].x = (v[u][q].x - mean) * rstd * g.x + be.x;
            v[u][q].y = (v[u][q].y - mean) * rstd * g.y + be.y;
            v[u][q].z = (v[u][q].z - mean) * rstd * g.z + be.z;
            v[u][q].w = (v[u][q].w - mean) * rstd * g.w + be.w;
          }
        }
        if (ok[u]) {
#pragma unroll
          for (int q = 0; q < VPL; ++q) {
            const int col = (lc + q * LPR) * 4;
            if (STATS) {
              const float4 x = v[u][q];
              const float s1 = (x.x + x.y) + (x.z + x.w), s2 = (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
              if (((n0 + col) % p.chan_mod) >= half_mod) { st1 += s1; sq1 += s2; } else { st0 += s1; sq0 += s2; }
            }
            if (!LN && !STATS) {
              const float4 x = v[u][q];
              amax = fmaxf(amax, fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w))));
            }
            *reinterpret_cast<float4*>(p.out + obase[u] + col) = v[u][q];
          }
        }
      }
    }
  }
  // (precision 3: no split GEMM reads this output, only a non-finite value is an error)
  if (guard && !(amax <= (p.precision == 3 ? 3.402823466e38f : 65504.f))) atomicAdd(&g_f16x3_overflow, 1u);      // also catches NaN
  if (STATS) {
    __syncthreads();
    st0 = wave_sum(st0); sq0 = wave_sum(sq0); st1 = wave_sum(st1); sq1 = wave_sum(sq1);
    float* red = smem;                           // Ct is dead after the barrier above
    if (lane == 0) { red[wid * 4 + 0] = st0; red[wid * 4 + 1] = sq0; red[wid * 4 + 2] = st1; red[wid * 4 + 3] = sq1; }
    __syncthreads();
    if (tid < 4) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < WM * WN; ++w) s += red[w * 4 + tid];
      // slot layout is independent of the tile shape: stats_stride slots per batch item (the
      // launcher zero-fills the buffer, smaller grids simply leave slots at zero)
      const long part = (long)b * p.stats_stride + (long)tile.x * ncol + tile.y;
      p.stats[part * 4 + tid] = s;
    }
  }
}

// The epilogue variants of a non-LayerNorm tile: gate tensor (MUL), GroupNorm partial sums with the skip operand added
// on load (STATS + A2F), partial sums alone, plain.  A tile is a type with run<STATS, MUL, A2F>(a, s).
template <typename Tile, bool HAS_MUL = true>
int launch_variant(const asw_convgemm_args& a, hipStream_t s) {
  const bool stats = a.stats != nullptr;
  if constexpr (HAS_MUL)
    if (a.mul) return Tile::template run<false, true, false>(a, s);
  if (stats && a.A2) return Tile::template run<true, false, true>(a, s);
  return stats ? Tile::template run<true, false, false>(a, s) : Tile::template run<false, false, false>(a, s);
}

}  // namespace asw_mfma
