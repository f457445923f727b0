// pipegemm.hip -- the pipelined 256-column f16x3 GEMM (convgemm16p) and the mask path built on its main loop, reached
// from the dispatcher of convgemm.hip through asw::pipe_gemm and from asw_mask_path_f16x3.  Layout and arithmetic
// are described at the head of convgemm.hip, the epilogue in gemm_epilogue.h.  ONE main loop (pipe_mainloop) walks the
// stages of a ResidueA feed (f16x3_tile.h) in both of its walks; the mask path kernel is that loop plus named phases.
#include <type_traits>

#include "gemm_epilogue.h"

namespace {
using namespace asw_mfma;

// ------------------------------------------------------------------ pipelined wide-tile GEMM
// The 8-wave 256-column tiles (mask encoder, strided / transposed convolutions, big linears) as a
// software pipeline with ONE barrier per 32-wide chunk instead of two (cycle counters on the
// two-barrier kernel of convgemm.hip, mask-encoder shape: per chunk wave 0 spent 1150 cycles depositing the
// next chunk with every MFMA pipe of the workgroup idle, tests/micro/phase_timing.py):
//  * B never touches LDS: the weights are pre-packed in MFMA-fragment order (asw_pack_fragments_f16,
//    the layout of the residual kernel), each wave pulls its two column fragments per k-step with
//    coalesced 1 KiB loads, QDB k-steps ahead of their use (L2-resident: one column tile of the
//    largest matrix is 2.1 MB);
//  * A (fp32 activations) is split to fp16 hi / lo while it is deposited, into a two-stage LDS ring:
//    the rows of image k+1 are fetched before, and deposited after, the MFMAs of image k, so the
//    deposit of one wave overlaps the MFMAs of the others and only the ring hand-over needs a barrier.
// Same tiling (wave tile BM/2 x 64), same epilogue, same XCD-aware tile order as the two-barrier kernel.
// Measured (T = 48 000, batch 64): mask encoder 312 -> 332 TFLOP/s, strided / transposed convolutions
// +3-6 %.  64-wide chunks (half the barriers, 147 KB ring) spill and lose: 304 -- BK is the constant 32 here.
constexpr int BN = 256, WN = 4, LDC = BN + 4;
constexpr int BK = 32, KS = BK / 16;             // a chunk of one tap is KS k-steps (16 K each)
constexpr int QDB = 2;                           // B fragments in flight, in k-steps
static_assert(KS == QDB, "a tap is QDB k-steps: the B buffer of a k-step is its index within the tap");

// the A feed of a tile: the residue walk where asw::residue_feed_ok says so at the launch site (RES), else the chunk walk
template <int BM, int WM, bool A2F, bool RES>
using PipeFeed = ResidueA<BM, BK, 64 * WM * WN, A2F, RES ? ASW_RESIDUE_MAX_SHIFT : 0>;
// bytes of the two-stage A ring: hi + lo image of Feed::ROWS rows per stage
template <typename Feed>
constexpr size_t pipe_ring_bytes() { return (size_t)2 * 2 * Feed::ROWS * Feed::LDH * sizeof(_Float16); }

// Main loop of one 256-column tile: picks the tile of this workgroup (false: none, the whole workgroup
// leaves), runs the K loop and returns the accumulators (wave (wm, wn) of WM x 4 holds rows
// wm*BM/WM + 32*i.., columns wn*64 + 32*j..).  Ends on a barrier: the ring is free for the epilogue.
// WM = 2: eight waves on a 256-row tile, one workgroup per CU.  WM = 1: four waves on a 128-row tile with the
// SAME wave tile (128 x 64), two independent workgroups per CU -- one's epilogue under the other's main loop.
//
// The loop walks STAGES.  A stage is one LDS image of the feed -- one (residue, chunk) -- plus the taps that read it
// (tap r + q * W at row shift q); ONE barrier per stage; the next image is fetched at the top of the stage and
// deposited DEP k-steps into it.  Chunk walk (W = taps): one tap per image, stage r * cpb + c is chunk kc of the tap-major
// K order and its k-steps are kc * KS + ks.  Residue walk (W = stride, strided convolutions with taps > stride): every
// input row deposited once per tile instead of once per tap.  Mask encoder (33 taps, stride 16): 32 deposits and
// barriers per tile instead of 66, 4 k-steps (6 for residue 0) between barriers instead of 2.  The fragment index of a
// k-step is the same in both walks, only the order of the visit differs; every tap contributes KS == QDB k-steps, so
// the B slot of a k-step is static.
// Frames past M_out: an image row serves up to three frames, so the phantom frames of a ragged tile have
// accumulated real rows in the residue walk.  That is undone HERE, by clearing their accumulators after the loop -- the
// state the chunk walk's disabled loads leave, where the clearing changes nothing -- and not in the epilogues: outputs,
// GroupNorm partial sums, the mask path's bypass gating, decoder contraction and range guard all see zeros.
template <int BM, typename Feed, int NTERM, int WM>
__device__ __forceinline__ bool pipe_mainloop(const asw_convgemm_args& p, float* smem, floatx16 (&acc)[BM / WM / 32][2],
                                              dim3& tile_out, int& ncol_out) {
  constexpr int LDH = Feed::LDH, ROWS = Feed::ROWS;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int STAGE = 2 * ROWS * LDH;            // halves per ring stage (hi image + lo image)
  constexpr int DEP = Feed::DEPOSIT_AFTER;         // the k-step of a stage after which the next image is deposited

  _Float16* ring = reinterpret_cast<_Float16*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int ncol = p.N / BN, nrt = (p.M_out + BM - 1) / BM;
  uint3 tl;
  if (!xcd_tile_groups(p.B, nrt, ncol, tl)) return false;     // XCD-aware order, groups of 8
  const dim3 tile(tl.x, tl.y, tl.z);
  tile_out = tile;
  ncol_out = ncol;
  const int b = tile.z, m0 = tile.x * BM, n0 = tile.y * BN;
  const asw::ResidueFeed rf = Feed::walk(p);
  const int nst = rf.stages();
  const int tap_ks = rf.stride * rf.cpb * KS;      // k-steps from a tap to the next tap of the same image
  const half8* __restrict__ Wh = reinterpret_cast<const half8*>(p.Wf_hi);
  const half8* __restrict__ Wl = reinterpret_cast<const half8*>(p.Wf_lo);
  const int NTF = p.N / 32;                        // column fragments across N
  const int nt0 = n0 / 32 + wn * TN;

  Feed A(p, b, m0, tid);
  auto deposit = [&](int stage) {
    _Float16* Ah = ring + stage * STAGE;
    A.template deposit<NTERM>(Ah, Ah + ROWS * LDH);
  };
  auto bload = [&](int kg, half8 (&bh)[TN], half8 (&bl)[TN]) {          // kg = global k-step (16 K each)
#pragma unroll
    for (int j = 0; j < TN; ++j) frag_load<NTERM>(Wh, Wl, (long)kg * NTF + nt0 + j, lane, bh[j], bl[j]);
  };

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int a_off = (wm * (BM / WM) + (lane & 31)) * LDH + (lane >> 5) * 8;
  half8 qh[QDB][TN], ql[QDB][TN];                  // B fragments of the next tap's k-steps
  int r = 0, c = 0, sh = rf.shifts(0);             // the stage being multiplied: residue, chunk, largest row shift
#pragma unroll
  for (int q = 0; q < QDB; ++q) bload(rf.kstep(rf.tap(0, 0), 0, KS) + q, qh[q], ql[q]);
  A.load(r, c, sh);
  deposit(0);
  __syncthreads();
  // One stage; PAR = stage parity, compile-time so that the ring stage index is static (the loop below is
  // unrolled by two).
  auto stage = [&](int s, auto par) {
    constexpr int PAR = decltype(par)::value;
    const bool more = s + 1 < nst;
    int rn = r, cn = c + 1, shn = sh;              // residue-major, chunk inner
    if (cn == rf.cpb) { cn = 0; rn = r + 1; shn = rf.shifts(rn); }
    // Every load of the loop is UNCONDITIONAL (f16x3_tile.h, kloop): after the last stage the A lanes are all disabled
    // (no traffic) and the B index is the fragment already held -- a load under an `if` costs a vmcnt(0) at the join
    A.load(rn, cn, more ? shn : -BM);              // in flight under the MFMAs of this stage
    const _Float16* Ah = ring + PAR * STAGE;
    const _Float16* Al = Ah + ROWS * LDH;
#pragma unroll
    for (int q = 0; q <= Feed::SHIFTS; ++q) {
      if (q == 0 || q <= sh) {                     // tap r + q * W: tile row i reads image row i + q
        const bool last = q == Feed::SHIFTS || q == sh;
        // the fragments QDB k-steps ahead: the same k-steps of the image's next tap, or of the next image's first
        const int kb = rf.kstep(rf.tap(r, q), c, KS);
        const int kn = !last ? kb + tap_ks : more ? rf.kstep(rf.tap(rn, 0), cn, KS) : kb;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          half8 ah[TM], al[TM];
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            ah[i] = *reinterpret_cast<const half8*>(Ah + a_off + (i * 32 + q) * LDH + ks * 16);
            if (NTERM == 3) al[i] = *reinterpret_cast<const half8*>(Al + a_off + (i * 32 + q) * LDH + ks * 16);
          }
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) mma3<NTERM>(acc[i][j], ah[i], al[i], qh[ks][j], ql[ks][j]);
          bload(kn + ks, qh[ks], ql[ks]);
          // deposit of the next image between the k-steps: its conversions and LDS writes issue in the shadow of
          // this wave's own MFMAs (the other stage was last read one stage ago, before the previous barrier).
          // Eight waves: unconditional like the loads (after the last stage: zeros into the stage nobody reads again);
          // under `if (more)` hipcc sinks the A loads of a one-tap stage down to this block and waits for them on the
          // spot (plain 256-row tile 3.51 -> 3.92 ms per step, mask path 17.17 -> 17.57).  Four waves: the second
          // workgroup of the CU hides that wait, and the extra deposit in front of the epilogue of a tile of 8-16
          // stages costs more (3.58 -> 3.66).  (A switch on the TILE, WM; the feeds differ in DEP alone.)
          if (q == 0 && ks == DEP && (more || WM == 2)) deposit(PAR ^ 1);
        }
      }
    }
    __syncthreads();
    r = rn; c = cn; sh = shn;
  };
  for (int s = 0; s < nst; s += 2) {
    stage(s, std::integral_constant<int, 0>{});
    if (s + 1 < nst) stage(s + 1, std::integral_constant<int, 1>{});
  }
  if (m0 + BM > p.M_out) {                         // ragged tile: frames past M_out contribute nothing (see above)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (m0 + wm * (BM / WM) + i * 32 + acc_row(e, lane >> 5) >= p.M_out) {
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j][e] = 0.f;
        }
      }
  }
  return true;
}

template <int BM, bool STATS, bool MUL, bool A2F, int NTERM, int WM, bool RES>
__global__ __launch_bounds__(256 * WM) __attribute__((amdgpu_waves_per_eu(2)))
void convgemm16p_kernel(const asw_convgemm_args p) {
  extern __shared__ __align__(16) float smem[];
  floatx16 acc[BM / WM / 32][2];
  dim3 tile;
  int ncol;
  if (!pipe_mainloop<BM, PipeFeed<BM, WM, A2F, RES>, NTERM, WM>(p, smem, acc, tile, ncol)) return;
  epilogue<BM, BN, WM, WN, false, STATS, false, MUL>(acc, p, smem, __builtin_ldexpf(1.0f, -p.w_shift),
                                                     RowsContig{(int)tile.x * BM, p.M_out}, tile, ncol);
}

// ------------------------------------------------------------------ mask path in one kernel
// reference_bypass, mask_encoder and the output_decoder taps (network.py:327-349,397-405) without the
// 2048-channel latents ever reaching memory:
//   taps[f][j] = sum_e relu(mask_enc(x)[f][e] + b_e) * relu(bypass(ref)[f][e] + c_e) * D[e][j]
// The main loop is the pipelined GEMM above (mask encoder, K = taps*Cin).  Epilogue, per 256 x 256 tile, in the
// phases below: A. bypass tile and gating in registers (mask_gate); B. the gated latent through an LDS slab, 128 rows
// at a time (mask_slab_store), back in A-fragment order for the decoder contraction (mask_contract) and out as a
// PARTIAL tap product (mask_store_taps: this column tile's share of the sum over e; the overlap-add kernel adds the
// N/256 partials).
// Per candidate (T = 48 000) this writes 8 x 3008 x 33 floats instead of writing the bypass latent,
// reading it, writing the gated latent and reading that again (4 x 24.6 MB).
//
// SCALED (asw_mask_path_f16x3_scaled, the f16x3_safe mode): the gated latent is the one un-normalised tensor that is
// split to fp16 inside a kernel, and split4 saturates at 65504.  This variant gives every latent row of a pass (one
// frame, the tile's 256 channels) a power-of-two scale of its own (mask_row_scale) before the split and takes it off
// the frame's taps after the contraction.  Both steps are exact (v_ldexp_f32), so the kernel is exactly
// homogeneous per frame: scaling a frame's latent by 2^k scales its taps by 2^k, bit for bit.
constexpr int MASK_BINADE = 12;
constexpr int MASK_KSB = 3;                      // k-steps of the bypass kernel: 33 taps padded to 48

// Phase A: each wave computes the bypass tile of its own 32 x 32 accumulator blocks with nine more MFMAs (K = 33 padded
// to 48; the frames of the reference channel are read straight from global memory in A-fragment order) and gates
// the accumulators in registers.  The latent is split to fp16 halves in mask_contract: same range guard as a latent
// written for a later GEMM (SCALED: every row is brought into range first, a finite magnitude is no error; the row
// maxima of mask_row_scale find the rest).
template <int TM, int KSB, int NTERM, bool SCALED>
__device__ __forceinline__ void mask_gate(floatx16 (&acc)[TM][2], const asw_convgemm_args& p, const asw_maskpath_args& mf,
                                          int b, int m0, int n0, int lane, int wm, int wn) {
  constexpr int TN = 2;
  const float acc_scale = __builtin_ldexpf(1.0f, -p.w_shift), byp_scale = __builtin_ldexpf(1.0f, -mf.byp_shift);
  const __amdgpu_buffer_rsrc_t rR = act_rsrc(mf.ref + (long)b * mf.ref_batch_stride, mf.ref_len);
  const half8* __restrict__ Bh = reinterpret_cast<const half8*>(mf.byp_hi);
  const half8* __restrict__ Bl = reinterpret_cast<const half8*>(mf.byp_lo);
  const int NTF = p.N / 32;
  float amax = 0.f;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int nt = n0 / 32 + wn * TN + tn;
    const int col = nt * 32 + (lane & 31);
    const float bm = p.bias ? p.bias[col] : 0.f, bb = mf.byp_bias ? mf.byp_bias[col] : 0.f;
    half8 wh[KSB], wl[KSB];
#pragma unroll
    for (int ks = 0; ks < KSB; ++ks) frag_load<NTERM>(Bh, Bl, (long)ks * NTF + nt, lane, wh[ks], wl[ks]);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int f = m0 + wm * (TM * 32) + tm * 32 + (lane & 31);
      const bool ok = f < p.M_out;
      floatx16 bp;
#pragma unroll
      for (int r = 0; r < 16; ++r) bp[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KSB; ++ks) {
        const long e = (long)f * mf.ref_hop + ks * 16 + (lane >> 5) * 8;
        const float4 x0 = act_load4(rR, e, ok), x1 = act_load4(rR, e + 4, ok);
        half4 h0, l0, h1, l1;
        split4t<NTERM>(x0, h0, l0);
        split4t<NTERM>(x1, h1, l1);
        const half8 ah = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        const half8 al = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
        mma3<NTERM>(bp, ah, al, wh[ks], wl[ks]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = fmaxf(acc[tm][tn][r] * acc_scale + bm, 0.f) * fmaxf(bp[r] * byp_scale + bb, 0.f);
        if constexpr (!SCALED) amax = fmaxf(amax, v);
        acc[tm][tn][r] = v;
      }
    }
    // one column block after the other (only loads may move up across this line): with both blocks' bypass tiles
    // scheduled together the three-term kernels, which sit at the 256 VGPRs of two waves per SIMD, spill (248 bytes
    // of scratch without it)
    if (tn == 0) __builtin_amdgcn_sched_barrier(0x20);
  }
  if (!SCALED && !(amax <= 65504.f)) atomicAdd(&g_f16x3_overflow, 1u);
}

// Phase B, slab store: the 128 rows of this wave row's gated accumulators into the slab
template <int TM>
__device__ __forceinline__ void mask_slab_store(float* Ct, const floatx16 (&acc)[TM][2], int lane, int wn) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int col = wn * 64 + tn * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) Ct[(tm * 32 + acc_row(r, lane >> 5)) * LDC + col] = acc[tm][tn][r];
    }
}

// Phase B, row scale of SCALED.  A lane owns one slab row in A-fragment order (`src`: its 128 values of the 256): with
// 2^e <= max|row| < 2^(e+1) the row is split as row * 2^rsh, rsh = MASK_BINADE - e, which puts its largest magnitude into
// [2^12, 2^13) whatever it was -- up as well as down, so small rows keep their lo halves out of the fp16 subnormals
// too.  The row maximum is a pre-pass over the lane's own values and one exchange with lane ^ 32.  A row of zeros (or
// of fp32 subnormals) keeps scale 1.  The range guard counts non-finite latents only.
__device__ __forceinline__ int mask_row_scale(const float* src) {
  // magnitudes order like their bit patterns, and a NaN (which fmaxf would drop) sorts above every number
  unsigned mb = 0;
  auto mag = [](float v) { return __builtin_bit_cast(unsigned, v) & 0x7fffffffu; };
#pragma unroll 4
  for (int ks = 0; ks < BN / 16; ++ks) {
    const float4 x0 = *reinterpret_cast<const float4*>(src + ks * 16);
    const float4 x1 = *reinterpret_cast<const float4*>(src + ks * 16 + 4);
    mb = max(max(max(mb, mag(x0.x)), max(mag(x0.y), mag(x0.z))), max(max(mag(x0.w), mag(x1.x)), mag(x1.y)));
    mb = max(mb, max(mag(x1.z), mag(x1.w)));
  }
  const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);   // the other half of the row: lane ^ 32
  const int ef = (int)(max(sw[0], sw[1]) >> 23);                            // biased exponent of the row maximum
  if (ef == 255) atomicAdd(&g_f16x3_overflow, 1u);                          // range guard: inf or NaN in the latent
  return (ef == 0 || ef == 255) ? 0 : MASK_BINADE + 127 - ef;
}

// Phase B, decoder contraction over the tile's 256 latent channels: eight waves = four 32-row blocks x two 32-tap
// blocks (tt), 48 MFMAs each; the lane's row comes back from the slab in A-fragment order, times 2^rsh if SCALED
template <int NTERM, bool SCALED>
__device__ __forceinline__ floatx16 mask_contract(const float* src, int rsh, const asw_maskpath_args& mf, int n0, int tt, int lane) {
  const half8* __restrict__ Dh = reinterpret_cast<const half8*>(mf.dec_hi);
  const half8* __restrict__ Dl = reinterpret_cast<const half8*>(mf.dec_lo);
  floatx16 tp;
#pragma unroll
  for (int r = 0; r < 16; ++r) tp[r] = 0.f;
#pragma unroll 4
  for (int ks = 0; ks < BN / 16; ++ks) {
    float4 x0 = *reinterpret_cast<const float4*>(src + ks * 16);
    float4 x1 = *reinterpret_cast<const float4*>(src + ks * 16 + 4);
    if constexpr (SCALED) {
      x0 = make_float4(__builtin_ldexpf(x0.x, rsh), __builtin_ldexpf(x0.y, rsh), __builtin_ldexpf(x0.z, rsh), __builtin_ldexpf(x0.w, rsh));
      x1 = make_float4(__builtin_ldexpf(x1.x, rsh), __builtin_ldexpf(x1.y, rsh), __builtin_ldexpf(x1.z, rsh), __builtin_ldexpf(x1.w, rsh));
    }
    half8 dh, dl;
    frag_load<NTERM>(Dh, Dl, (long)(n0 / 16 + ks) * 2 + tt, lane, dh, dl);
    half4 h0, l0, h1, l1;
    split4t<NTERM>(x0, h0, l0);
    split4t<NTERM>(x1, h1, l1);
    const half8 ah = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    const half8 al = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    mma3<NTERM>(tp, ah, al, dh, dl);
  }
  return tp;
}

// Phase B, tap store of the block whose first frame is f0.  SCALED: register r holds row acc_row(r, lane >> 5) of the
// block, another row than the lane's A row, so that row's exponent comes back through a bpermute and its scale is
// undone first (every lane takes part in the exchange, whatever it stores below)
template <bool SCALED>
__device__ __forceinline__ void mask_store_taps(floatx16 tp, int rsh, const asw_maskpath_args& mf, float* __restrict__ outp,
                                                int f0, int M_out, int tt, int lane) {
  if constexpr (SCALED) {
#pragma unroll
    for (int r = 0; r < 16; ++r) tp[r] = __builtin_ldexpf(tp[r], -__shfl(rsh, acc_row(r, lane >> 5), 64));
  }
  const float dec_scale = __builtin_ldexpf(1.0f, -mf.dec_shift);
  const int j = tt * 32 + (lane & 31);
  if (j < mf.dec_taps) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = f0 + acc_row(r, lane >> 5);
      if (f < M_out) outp[(long)f * 64 + j] = tp[r] * dec_scale;
    }
  }
}

template <int BM, int KSB, int NTERM, bool RES, bool SCALED>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2)))
void maskpath16p_kernel(const asw_convgemm_args p, const asw_maskpath_args mf) {
  constexpr int TM = BM / 64;
  static_assert(BM == 256, "slab passes are written for 2 x 128 rows");
  extern __shared__ __align__(16) float smem[];
  floatx16 acc[TM][2];
  dim3 tile;
  int ncol;
  if (!pipe_mainloop<BM, PipeFeed<BM, 2, false, RES>, NTERM, 2>(p, smem, acc, tile, ncol)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  // (the wave index as a scalar: wm, ft and tt live across every phase, and as vector registers they are the ones
  // that go to scratch)
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int b = tile.z, m0 = tile.x * BM, n0 = tile.y * BN;
  mask_gate<TM, KSB, NTERM, SCALED>(acc, p, mf, b, m0, n0, lane, wm, wn);
  // rows [pass*128, pass*128 + 128) of the tile per pass
  float* Ct = smem;
  const int ft = wid & 3, tt = wid >> 2;                       // 32-row block, 32-tap block of this wave
  float* __restrict__ outp = mf.taps + ((long)tile.y * p.B + b) * p.M_out * 64;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) __syncthreads();                                 // (pass 0: the main loop ended on a barrier)
    if (wm == pass) mask_slab_store<TM>(Ct, acc, lane, wn);
    __syncthreads();
    const float* src = Ct + (ft * 32 + (lane & 31)) * LDC + (lane >> 5) * 8;
    int rsh = 0;                                               // SCALED: this lane's row is split as row * 2^rsh
    if constexpr (SCALED) rsh = mask_row_scale(src);
    const floatx16 tp = mask_contract<NTERM, SCALED>(src, rsh, mf, n0, tt, lane);
    mask_store_taps<SCALED>(tp, rsh, mf, outp, m0 + pass * 128 + ft * 32, p.M_out, tt, lane);
  }
}

// mask encoder + bypass + decoder taps; the encoder's rows through the residue walk where it applies
template <bool RES, bool SCALED>
int launch_mask(const asw_convgemm_args& a, const asw_maskpath_args& m, hipStream_t s) {
  constexpr int BM = 256, KSB = MASK_KSB;
  constexpr size_t ring = pipe_ring_bytes<PipeFeed<BM, 2, false, true>>();     // (the larger of the two feeds' rings)
  constexpr size_t slab = (size_t)128 * LDC * sizeof(float);
  constexpr size_t smem = ring > slab ? ring : slab;
  static_assert(smem <= 160 * 1024, "LDS budget");
  const dim3 grid(xcd_grid_groups((long)asw::cdiv(a.M_out, BM) * a.B, a.N / BN));
  const double flops = 2.0 * a.B * (double)a.M_out * a.N * ((double)a.taps * a.Cin + m.byp_taps + m.dec_taps);
  const asw::ShapeTag tag(a, 's', a.stride, RES ? " res" : "");     // the detailed profile says which feed ran
  return asw::launch_pair<maskpath16p_kernel<BM, KSB, SCALED ? 3 : 1, RES, SCALED>, maskpath16p_kernel<BM, KSB, 3, RES, SCALED>>(
      a.precision, grid, dim3(512), smem, smem, SCALED ? "maskpath16ps<256,256,32>" : "maskpath16p<256,256,32>", tag.s, flops,
      0.0, s, a, m);
}

int launch_mask_path(const asw_maskpath_args* args, void* stream, bool scaled = false) {
  ASW_CHECK_ARG(args, "mask_path: null argument block");
  const asw_maskpath_args& m = *args;
  asw_convgemm_args a = m.enc;
  ASW_CHECK_ARG(a.A && a.Wf_hi && a.Wf_lo && m.ref && m.byp_hi && m.byp_lo && m.dec_hi && m.dec_lo && m.taps,
                "mask_path: null pointer (fragment-order weights are required)");
  ASW_CHECK_ARG(a.B > 0 && a.M_out > 0 && a.N % BN == 0 && a.Cin % BK == 0 && a.taps > 0 && a.stride > 0,
                "mask_path: shape (N %% 256 == 0, Cin %% 32 == 0)");
  ASW_CHECK_ARG(a.a_len > 0 && a.a_len < ((int64_t)1 << 29) && asw::pipe_offsets_ok(a),
                "mask_path: input rows beyond the 32-bit offsets of the pipelined tile");
  ASW_CHECK_ARG(a.A2 == nullptr && a.mul == nullptr && a.resid == nullptr && a.ln_gamma == nullptr && a.stats == nullptr,
                "mask_path: the encoder block takes A, weights and bias only");
  ASW_CHECK_ARG(m.byp_k == 16 * MASK_KSB, "mask_path: bypass kernel padded to %d taps, %d given", 16 * MASK_KSB, m.byp_k);
  ASW_CHECK_ARG(m.dec_taps > 0 && m.dec_taps <= 64 && m.ref_hop > 0 && m.ref_hop % 4 == 0 && m.ref_len > 0,
                "mask_path: decoder taps 1..64, reference hop a multiple of 4 samples");
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(m.ref) & 15) == 0 && m.ref_batch_stride % 4 == 0,
                "mask_path: reference rows must be 16-byte aligned");
  ASW_CHECK_ARG(a.precision == 1 || a.precision == 2, "mask_path: precision 1 (f16x3) or 2 (single-pass f16)");
  ASW_CHECK_ARG(!scaled || a.precision == 1, "mask_path: the per-frame scale exists for precision 1 (f16x3) only");
  a.relu = 1;
  const bool res = asw::residue_feed_ok(a, BK);
  const auto launch = scaled ? (res ? launch_mask<true, true> : launch_mask<false, true>)
                             : (res ? launch_mask<true, false> : launch_mask<false, false>);
  return launch(a, m, asw::as_stream(stream));
}

template <int BM, bool STATS, bool MUL, bool A2F, int WM, bool RES>
int launch_pipe(const asw_convgemm_args& a, hipStream_t s) {
  constexpr size_t ring = pipe_ring_bytes<PipeFeed<BM, WM, A2F, RES>>();
  constexpr size_t slab = (size_t)(WM * 32) * LDC * sizeof(float);
  constexpr size_t smem = ring > slab ? ring : slab;
  static_assert(smem <= 160 * 1024, "LDS budget");
  static_assert(BM == 128 * WM, "wave tile 128 x 64");
  ASW_CHECK_ARG(A2F == (a.A2 != nullptr), "convgemm: skip operand variant mismatch");
  ASW_CHECK_ARG(a.Cin % BK == 0 && a.N % BN == 0, "convgemm: pipelined tile needs Cin %% 32 == 0 and N %% 256 == 0");
  return asw::launch_pair<convgemm16p_kernel<BM, STATS, MUL, A2F, 1, WM, RES>, convgemm16p_kernel<BM, STATS, MUL, A2F, 3, WM, RES>>(
      a.precision, dim3(xcd_grid_groups((long)asw::cdiv(a.M_out, BM) * a.B, a.N / BN)), dim3(256 * WM), smem, smem,
      asw::prof_name(MUL ? "convgemm16pm" : "convgemm16p", BM, BN, BK, false, STATS),
      asw::ShapeTag(a, 's', a.stride, RES ? " res" : "").s,
      2.0 * a.B * (double)a.M_out * a.N * (double)a.taps * a.Cin, 0.0, s, a);
}

template <int BM, int WM>
struct PipeTile {                        // pipelined 256-column kernel: convgemm16p
  template <bool STATS, bool MUL, bool A2F>
  static int run(const asw_convgemm_args& a, hipStream_t s) {
    // strided convolutions with taps > stride: every input row deposited once per tile (plain and statistics forms)
    if constexpr (!MUL && !A2F)
      if (asw::residue_feed_ok(a, BK)) return launch_pipe<BM, STATS, MUL, A2F, WM, true>(a, s);
    return launch_pipe<BM, STATS, MUL, A2F, WM, false>(a, s);
  }
};

}  // namespace

namespace asw {
int pipegemm_f16x3_overflow(int reset, unsigned int* count) { return f16x3_overflow_read(reset, count); }

// The wide f16x3 tile with fragment-order weights (the caller has checked both, and asw::pipe_offsets_ok).
int pipe_gemm(const asw_convgemm_args& a, hipStream_t s) {
  // Short K (the decoder's transposed convolutions): two independent 4-wave workgroups of 128 rows per CU, same
  // wave tile -- one drains its tile while the other computes (K = 512: 234 -> 260 TFLOP/s, K = 256: 186 -> 193;
  // at K >= 896 and in the mask path the 8-wave tile is 2-4 % ahead).
  if (a.taps * a.Cin <= 512 && !a.mul) return launch_variant<PipeTile<128, 1>, false>(a, s);
  return launch_variant<PipeTile<256, 2>>(a, s);
}
}  // namespace asw

extern "C" int asw_mask_path_f16x3(const asw_maskpath_args* args, void* stream) { return launch_mask_path(args, stream); }
extern "C" int asw_mask_path_f16x3_scaled(const asw_maskpath_args* args, void* stream) {
  return launch_mask_path(args, stream, true);
}
