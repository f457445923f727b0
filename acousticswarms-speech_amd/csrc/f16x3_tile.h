// f16x3_tile.h -- the building blocks the split-fp16 ("f16x3") matrix kernels share (convgemm.hip, pipegemm.hip,
// resconv.hip, resstack.hip, downconv.hip): the three-term product, the fragment-order weight load, the halo-image row layout with its staging
// loop, the pinned transposed k-loop, the A operands of the row-major GEMMs (ChunkedA of the two-barrier kernel, ResidueA
// of the pipelined tiles, one deposit) and the XCD-aware tile orders.
// Everything is inlined into its caller; a kernel experiment changes one of these instead of a copy per kernel.
#pragma once
#include "mfma_util.h"

namespace asw_mfma {

// ------------------------------------------------------------------ three-term product
// acc += x . w for an activation (xh, xl) and a weight (wh, wl) fragment pair, as
//   x_lo * w_hi,  x_hi * w_lo,  x_hi * w_hi      (NTERM == 1: the last term only)
// in THIS order in every kernel: fp32 accumulation is not associative, and the kernels that compute the same layer
// (generic GEMM, halo kernel, fused stack, stride-2 kernel) agree to the bit only because their terms arrive alike.
// W_IS_A says which side is the MFMA A operand: the row-major kernels pass the activation as A (a lane holds 16
// rows of one column), the transposed kernels (resstack64, downconv64) the weight (16 channels of one row).  It
// swaps the operands of each MFMA, never the order of the terms.
template <int NTERM, bool W_IS_A = false>
__device__ __forceinline__ void mma3(floatx16& acc, const half8& xh, const half8& xl, const half8& wh, const half8& wl) {
  auto term = [&](const half8& x, const half8& w) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W_IS_A ? w : x, W_IS_A ? x : w, acc, 0, 0, 0);
  };
  if (NTERM == 3) {
    term(xl, wh);
    term(xh, wl);
  }
  term(xh, wh);
}

// ------------------------------------------------------------------ fragment-order weights
// asw_pack_fragments_f16 stores the 32-column x 16-k fragment (k-step kg, column fragment nt of NT) as 64 lanes x
// 16 bytes: one coalesced 1 KiB load per wave, hi and (three-term mode) lo.  `frag` = kg * NT + nt, formed by the
// caller: which part of that sum is loop-invariant differs per kernel, and the association decides what hipcc folds
// into the load's immediate offset (nt0 + j added before the widening cost resconv16 ten VGPRs at C = 128).
template <int NTERM>
__device__ __forceinline__ void frag_load(const half8* Wh, const half8* Wl, long frag, int lane, half8& h, half8& l) {
  const long o = frag * 64 + lane;
  h = Wh[o];
  if (NTERM == 3) l = Wl[o];
}

// ------------------------------------------------------------------ halo image
// One image row = 64 channels as 128 B of fp16 hi + 128 B of fp16 lo + 16 B pad: the per-lane 16-byte fragment
// reads of 32 consecutive rows are bank-conflict free.
constexpr int RS = 272;                  // bytes per image row
constexpr int IMG_HI = 0, IMG_LO = 128;  // byte offsets of the two halves in a row

// GroupNorm(2) statistics of one batch item and the affine vectors of this thread's four channels (value | gate half)
struct GluCoef {
  float m0 = 0.f, r0 = 0.f, m1 = 0.f, r1 = 0.f;
  float4 ga, ba, gg, bg;
  __device__ __forceinline__ void stats(const float* mr, int b) {
    m0 = mr[b * 4 + 0]; r0 = mr[b * 4 + 1]; m1 = mr[b * 4 + 2]; r1 = mr[b * 4 + 3];
  }
  __device__ __forceinline__ void affine(const float* gamma, const float* beta, int C, int c) {
    ga = *reinterpret_cast<const float4*>(gamma + c);
    ba = *reinterpret_cast<const float4*>(beta + c);
    gg = *reinterpret_cast<const float4*>(gamma + C + c);
    bg = *reinterpret_cast<const float4*>(beta + C + c);
  }
};
// the arithmetic of gn_glu_kernel, expression for expression; rows outside the sequence stay zero (computed
// unconditionally and then selected: a branch around the arithmetic would split the staging loop per component)
__device__ __forceinline__ float4 gn_glu4(const float4& a, const float4& g, const GluCoef& c, bool ok) {
  const float x = asw::gn_glu_value(a.x, g.x, c.m0, c.r0, c.m1, c.r1, c.ga.x, c.ba.x, c.gg.x, c.bg.x);
  const float y = asw::gn_glu_value(a.y, g.y, c.m0, c.r0, c.m1, c.r1, c.ga.y, c.ba.y, c.gg.y, c.bg.y);
  const float z = asw::gn_glu_value(a.z, g.z, c.m0, c.r0, c.m1, c.r1, c.ga.z, c.ba.z, c.gg.z, c.bg.z);
  const float w = asw::gn_glu_value(a.w, g.w, c.m0, c.r0, c.m1, c.r1, c.ga.w, c.ba.w, c.gg.w, c.bg.w);
  return make_float4(ok ? x : 0.f, ok ? y : 0.f, ok ? z : 0.f, ok ? w : 0.f);
}

struct ImgSrc { int g; bool ok; };       // global row of an image row, and whether it exists

// Stage R image rows of one 64-channel slice, split to fp16 hi / lo: NTHR threads, 16 per row, SU rows per thread in
// flight (every load of a round is issued before the first conversion).  The source is [T][C] fp32 behind the
// buffer descriptor rX, or with GLU the raw [T][value C | gate C] tensor, normalised and gated on the way
// (`side(g, ok, v)` then sees every row's float4 once: the optional glu_out store).  `src(row)` maps an image
// row to its global row; `coff` is the slice's first channel.  LO1: write the lo half in the one-term mode too (a
// kernel that takes its residual from the image needs it).
template <int NTHR, int C, int SU, bool GLU, int NTERM, bool LO1, typename Src, typename Side>
__device__ __forceinline__ void stage_image(char* img, int R, const __amdgpu_buffer_rsrc_t rX, int coff,
                                            const GluCoef& gc, const Src& src, const Side& side) {
  constexpr int SROWS = NTHR / 16;
  const int tid = threadIdx.x, srow = tid >> 4, sc4 = tid & 15;
  for (int r0 = 0; r0 < R; r0 += SROWS * SU) {
    float4 buf[SU];
    float4 gate[GLU ? SU : 1];
    bool okr[GLU ? SU : 1];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const ImgSrc f = src(r0 + u * SROWS + srow);
      if (GLU) {
        buf[u] = act_load4(rX, (long)f.g * 2 * C + coff + sc4 * 4, f.ok);
        gate[u] = act_load4(rX, (long)f.g * 2 * C + C + coff + sc4 * 4, f.ok);
        okr[u] = f.ok;
      } else {
        buf[u] = act_load4(rX, (long)f.g * C + coff + sc4 * 4, f.ok);
      }
    }
    if (GLU) {
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        buf[u] = gn_glu4(buf[u], gate[u], gc, okr[u]);
        side(src(r0 + u * SROWS + srow).g, okr[u], buf[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int row = r0 + u * SROWS + srow;
      if (row < R) {
        half4 hi, lo;
        split4t<NTERM>(buf[u], hi, lo);
        *reinterpret_cast<half4*>(img + row * RS + IMG_HI + sc4 * 8) = hi;
        if (NTERM == 3 || LO1) *reinterpret_cast<half4*>(img + row * RS + IMG_LO + sc4 * 8) = lo;
      }
    }
  }
}

// ------------------------------------------------------------------ pinned transposed k-loop
// taps x 4 k-steps of a 64-channel image for NF row fragments x CB 32-channel blocks of this wave, weight = MFMA A
// operand: acc[i][cb] += W(cb) . X(i)^T.  `xrow(tap, i)` is the image address of this lane's row of fragment i at tap
// `tap` (downconv64 picks its even or odd image there).  Weights are fragment-order, prefetched QD k-steps ahead;
// `wfrag(kg, cb)` is the fragment index kg * NT + nt of channel block cb at k-step kg.
// (Both are functors, not plain integers, so that a caller's compile-time constants and its order of address
// arithmetic reach the loops before they are unrolled: passed as arguments they cost resstack64 four VGPRs and its
// third wave per SIMD.)
template <int NF, int CB, int QD, int NTERM, typename XRow, typename WFrag>
__device__ __forceinline__ void kloop(floatx16 (&acc)[NF][CB], int taps, const XRow& xrow, const half8* __restrict__ Wh,
                                      const half8* __restrict__ Wl, const WFrag& wfrag, int lane) {
  auto wload = [&](int kg, half8 (&h)[CB], half8 (&l)[CB]) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) frag_load<NTERM>(Wh, Wl, wfrag(kg, cb), lane, h[cb], l[cb]);
  };
  auto xload = [&](int tap, int ks, half8 (&h)[NF], half8 (&l)[NF]) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const char* q = xrow(tap, i) + ks * 32;
      h[i] = *reinterpret_cast<const half8*>(q + IMG_HI);
      if (NTERM == 3) l[i] = *reinterpret_cast<const half8*>(q + IMG_LO);
    }
  };
  half8 wh[QD][CB], wl[QD][CB];
  half8 xh[2][NF], xl[2][NF];
#pragma unroll
  for (int q = 0; q < QD; ++q) wload(q, wh[q], wl[q]);
  xload(0, 0, xh[0], xl[0]);
  // Every load in the loop body is UNCONDITIONAL (past-the-end indices are clamped to the last fragment, which
  // is simply fetched again): a load inside an `if` sits in its own basic block, and at the join hipcc waits
  // vmcnt(0) -- i.e. for the weight fragments requested one k-step earlier -- once per tap, instead of counting.
  const int nks = taps * 4;
  for (int tap = 0; tap < taps; ++tap) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int nk = (ks + 1) & 3;
      int nt = tap + (ks == 3 ? 1 : 0);
      nt = nt < taps ? nt : taps - 1;
      xload(nt, nk, xh[(ks + 1) & 1], xl[(ks + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);       // (the next k-step's LDS reads go out BEFORE this k-step's MFMAs, not after)
      const int s = ks % QD, xbuf = ks & 1;
#pragma unroll
      for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) mma3<NTERM, true>(acc[i][cb], xh[xbuf][i], xl[xbuf][i], wh[s][cb], wl[s][cb]);
      int kg = tap * 4 + ks + QD;
      kg = kg < nks ? kg : nks - 1;
      wload(kg, wh[s], wl[s]);
      // pin the k-step order: left alone, hipcc sinks the four k-steps' weight loads to the end of the tap body and
      // waits for them at the top of the next one -- the L2 latency of the weight stream exposed once per tap
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ------------------------------------------------------------------ A operands of the row-major f16 GEMMs
// Both feeds hold a tile's fp32 rows as float4 v of thread tid = element tid + v * NT of a [ROWS][BK / 4] image, and
// deposit them split to fp16 hi / lo in rows of LDH = BK + 8 halves.  ROWS bounds the image: only the last float4 of a
// thread can fall outside it.
template <int NTERM, int ROWS, int BK, int NT, int NV>
__device__ __forceinline__ void deposit_rows(const float4 (&ra)[NV], int tid, _Float16* Ah, _Float16* Al) {
  constexpr int KV = BK / 4, LDH = BK + 8;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int idx = tid + v * NT;
    const int row = idx / KV, cv = idx - row * KV;
    if ((v + 1) * NT <= ROWS * KV || idx < ROWS * KV) {
      half4 hi, lo;
      split4t<NTERM>(ra[v], hi, lo);
      *reinterpret_cast<half4*>(Ah + row * LDH + cv * 4) = hi;
      if (NTERM == 3) *reinterpret_cast<half4*>(Al + row * LDH + cv * 4) = lo;
    }
  }
}

// ---- chunked A operand (convgemm16_kernel)
// The fp32 activation rows of a BM-row tile, walked in chunks of BK channels of one tap by NT threads: fetched to
// registers through the buffer descriptor (padding and rows past the end read as zeros; A2F adds the skip operand on
// load -- a compile-time variant, no runtime "load or zero" branch), then split and deposited.
template <int BM, int BK, int NT, bool A2F>
struct ChunkedA {
  static constexpr int KV = BK / 4;                // float4 per row
  static constexpr int LDH = BK + 8;               // halves per staged row
  static constexpr int A_VEC = (BM * KV + NT - 1) / NT;
  float4 ra[A_VEC];
  // per-thread invariants of the staging addresses
  long a_row[A_VEC];                               // element offset of (row, tap 0, c 0) + this thread's column
  bool a_ok[A_VEC];
  long tap_step;
  int cpb;                                         // chunks per tap
  __amdgpu_buffer_rsrc_t rA, rA2;
  // the kernel's own thread index, by reference: with a copy in this struct hipcc allocates six more VGPRs in the
  // variants that add the skip operand, and two of them lose a wave per SIMD
  const int& tid;

  __device__ __forceinline__ ChunkedA(const asw_convgemm_args& p, int b, int m0, const int& tid) : tid(tid) {
    const float* __restrict__ Ab = p.A + (long)b * p.a_batch_stride;
    const float* __restrict__ A2b = p.A2 ? p.A2 + (long)b * p.a_batch_stride : nullptr;
#pragma unroll
    for (int v = 0; v < A_VEC; ++v) {
      const int idx = tid + v * NT;
      const int row = idx / KV, cv = idx - row * KV;
      a_row[v] = ((long)(m0 + row) * p.stride - p.pad) * p.a_row_stride + cv * 4;
      a_ok[v] = (idx < BM * KV) && (m0 + row < p.M_out);
    }
    tap_step = (long)p.dil * p.a_row_stride;
    cpb = p.Cin / BK;
    rA = act_rsrc(Ab, p.a_len);
    rA2 = act_rsrc(A2F ? A2b : Ab, p.a_len);
  }
  __device__ __forceinline__ void load(int kc) {
    const int tap = kc / cpb;
    const long koff = tap * tap_step + (kc - tap * cpb) * BK;
#pragma unroll
    for (int v = 0; v < A_VEC; ++v) {
      const long e = a_row[v] + koff;                   // padding / past-the-end offsets read as zeros
      float4 x = act_load4(rA, e, a_ok[v]);
      if (A2F) {
        const float4 y = act_load4(rA2, e, a_ok[v]);
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
      }
      ra[v] = x;
    }
  }
  template <int NTERM>
  __device__ __forceinline__ void deposit(_Float16* Ah, _Float16* Al) const {
    deposit_rows<NTERM, BM, BK, NT>(ra, tid, Ah, Al);
  }
};

// ---- residue-image A operand (the pipelined tiles of pipegemm.hip: every stage of their main loop is one image)
// An image is the BM + shift input rows that ONE residue r = tap mod W of the walk and one BK-channel chunk c need:
// image row i is input row (m0 + i) * stride - pad + r * dil, and tap r + q * W of tile row i reads image row i + q
// (asw::ResidueFeed, include/asw_hip.h: asw_residue_schedule).  Two walks:
//  * SHIFTS == 0, W = taps, the chunk walk: one tap per image, every (tap, chunk) fetched, split and deposited for
//    its BM rows, as ChunkedA does;
//  * SHIFTS == ASW_RESIDUE_MAX_SHIFT, W = stride, the residue walk (asw::residue_feed_ok; dil == 1): with
//    taps > stride, tap j of frame f and tap j + stride of frame f - 1 are the same input row -- a 33-tap stride-16
//    tile handles every row 2.05 times in the chunk walk, once here.  An image has BM + (taps - 1 - r) / stride rows.
// The ring stage is sized for ROWS = BM + SHIFTS.  The BM rows every image has are FULL float4 per thread; the rows
// beyond them are one more float4 in the first threads only (the other lanes' loads are disabled: no traffic).
// Loads stay on the buffer descriptor: padding, rows past a_len and disabled lanes read as zeros and no index can
// fault.  A2F adds the skip operand on load (a second descriptor, compile-time, as in ChunkedA).
// Rows of frames past M_out ARE fetched where a valid frame reads them through a shift (only rows from
// M_out + SHIFTS on are left zero), so the phantom frames of a ragged tile accumulate real data in the residue walk:
// the caller clears their accumulators after the K loop.
template <int BM, int BK, int NT, bool A2F, int SH>
struct ResidueA {
  static constexpr int KV = BK / 4;                // float4 per row
  static constexpr int LDH = BK + 8;               // halves per staged row
  static constexpr int SHIFTS = SH, ROWS = BM + SHIFTS;
  // the k-step of a stage after which the stage loop deposits the next image: the middle of a one-tap stage, the end
  // of the first tap where more taps follow -- where each walk was measured, and the one place where the loop's
  // schedule differs between the walks
  static constexpr int DEPOSIT_AFTER = SH ? BK / 16 - 1 : BK / 32 - 1;
  static constexpr int FULL = BM * KV / NT;
  static constexpr int A_VEC = (ROWS * KV + NT - 1) / NT;
  static_assert(BM * KV % NT == 0 && A_VEC == FULL + (SHIFTS > 0), "BM rows split evenly; the shifted rows fit one more float4");
  float4 ra[A_VEC];
  // The staging addresses are ONE per-thread element offset plus uniform terms (float4 v of a thread is NT / KV rows
  // below float4 v - 1): an offset and a flag per float4, as ChunkedA keeps them, cost the three-term mask path its
  // last VGPRs and eight bytes of scratch.  32-bit: offsets stay below a_len + (BM + shift) rows + the tap term,
  // a_len < 2^29 (asw::pipe_offsets_ok bounds the terms at every launch).
  int a_base;                                      // element offset of (image row tid / KV, residue 0, c 0) + column
  int blk_step;                                    // NT / KV rows
  int row_lim;                                     // image rows from here on serve phantom frames only: left zero
  int row_step;                                    // from a residue's image to the next one's
  __amdgpu_buffer_rsrc_t rA, rA2;
  const int& tid;                                  // (by reference: see ChunkedA)

  // the walk of a launch: the residue walk steps by the stride, the chunk walk is its case of one tap per image
  static __device__ __forceinline__ asw::ResidueFeed walk(const asw_convgemm_args& p) {
    return asw::ResidueFeed{p.taps, SHIFTS ? p.stride : p.taps, p.Cin / BK};
  }
  __device__ __forceinline__ ResidueA(const asw_convgemm_args& p, int b, int m0, const int& tid) : tid(tid) {
    const int row = tid / KV, cv = tid - row * KV;
    a_base = (int)(((long)(m0 + row) * p.stride - p.pad) * p.a_row_stride) + cv * 4;
    blk_step = (NT / KV) * p.stride * (int)p.a_row_stride;
    row_lim = p.M_out + SHIFTS - m0;
    row_step = p.dil * (int)p.a_row_stride;
    rA = act_rsrc(p.A + (long)b * p.a_batch_stride, p.a_len);
    rA2 = act_rsrc((A2F ? p.A2 : p.A) + (long)b * p.a_batch_stride, p.a_len);
  }
  // image of residue r, chunk c; `shifts` = its rows beyond BM (-BM: no row at all, every lane disabled)
  __device__ __forceinline__ void load(int r, int c, int shifts) {
    const int koff = r * row_step + c * BK;
    const int rows = min(BM + shifts, row_lim);
#pragma unroll
    for (int v = 0; v < A_VEC; ++v) {                   // padding / past-the-end offsets read as zeros
      const int e = a_base + v * blk_step + koff;
      const bool ok = tid / KV + v * (NT / KV) < rows;
      float4 x = act_load4(rA, e, ok);
      if (A2F) {
        const float4 y = act_load4(rA2, e, ok);
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
      }
      ra[v] = x;
    }
  }
  // (rows an image does not have are deposited as the zeros their disabled loads returned: no tap reads them)
  template <int NTERM>
  __device__ __forceinline__ void deposit(_Float16* Ah, _Float16* Al) const {
    deposit_rows<NTERM, ROWS, BK, NT>(ra, tid, Ah, Al);
  }
};

// ------------------------------------------------------------------ XCD-aware tile orders
// The grids are 1-D; workgroup L goes to XCD L % 8 (the dispatcher deals consecutive workgroups round-robin over
// the 8 XCDs, each with its own L2).  Both orders pad the grid so that every XCD gets the same number of slots;
// padded slots exit.
//
// "Groups of 8" (convgemm16, pipe_mainloop of pipegemm.hip): slot s = L / 8 of one XCD walks the column tiles of a row tile first:
// the ncol workgroups that read the same activation rows run back to back on ONE L2, so those rows come from HBM
// once instead of once per column tile.  The (batch item, row tile) pairs are dealt to the XCDs in groups of 8, so
// every XCD gets the same share whatever the number of row tiles per item.
// tile = (row tile, column tile, batch item)
__device__ __forceinline__ bool xcd_tile_groups(int B, int nrt, int ncol, uint3& tile) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int R = (slot / ncol) * 8 + xcd;                      // (batch item, row tile) index
  tile = make_uint3(R % nrt, slot % ncol, R / nrt);
  return R < B * nrt;
}
inline unsigned xcd_grid_groups(long row_tiles, int ncol) { return (unsigned)(((row_tiles + 7) / 8) * 8 * ncol); }
// "Contiguous run" (resstack64, downconv64): XCD x walks a contiguous run of the `total` tiles, so the halo rows two
// neighbouring tiles share meet in one L2.  False for a padded slot.
__device__ __forceinline__ bool xcd_tile_run(int total, int& idx) {
  const int per = (total + 7) >> 3;
  idx = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  return idx < total;
}
inline unsigned xcd_grid_run(int total) { return (unsigned)(((total + 7) / 8) * 8); }

}  // namespace asw_mfma
