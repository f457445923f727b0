// resstack.hip -- a stack of 64-channel DilatedResidualLayers in ONE launch on the gfx950 matrix cores
// (f16x3 split-operand arithmetic), the layers' intermediate tensors never leaving LDS.
//
// Replaces (reference file:line): DilatedResidualLayer / DilatedResidualSequence
// (sep/training/SpeakerLocalization/network.py:50-82, sep/training/SpeakerSeparation/network.py, same
// classes): out_i = LayerNorm(ReLU(conv_{d_i}(x_i) + b_i) + x_i), x_{i+1} = out_i.
//
// Why a second residual kernel.  At C = 64 the halo-staged layer of resconv.hip (resconv16_kernel)
// moves 112 FLOP per byte of HBM traffic -- exactly the ridge of this chip -- and spends 44 % of a
// workgroup's time in its epilogue (accumulators -> LDS slab -> row-wise LayerNorm -> store).  Two changes:
//
//  * The accumulators are TRANSPOSED: the weight fragment is the A operand of v_mfma_f32_32x32x16_f16
//    and the activation rows are the B operand, so a lane holds, for ONE time row (lane & 31), 16
//    channels of each 32-channel block: (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  A wave owns all 64
//    channels of its rows, hence LayerNorm is 32 in-lane adds + ONE cross-lane shuffle, bias / ReLU /
//    residual are applied in registers, four consecutive channels of a row are one float4 (global
//    store) or one 8-byte hi / lo pair (LDS image): no slab, no barriers inside the epilogue.
//  * Consecutive layers with small dilation are FUSED: the workgroup stages the rows the whole stack
//    needs (output rows + the summed halos) once, layer i writes its output -- already split to fp16
//    hi / lo -- over the LDS image it has just consumed, layer i + 1 reads it from there.  With
//    R0 = 256 rows computed by layer 0 the pair (dilation 1, dilation 7; halo 3 + 21) produces
//    256 - 42 = 214 finished rows from a tile that stands alone: half the HBM round trips.  The
//    42 layer-0 rows two neighbouring tiles share are computed once all the same: a workgroup
//    walks a run of consecutive tiles of an item and carries them from tile to tile, so every
//    tile after a run's first finishes 256 rows (resstack64_carry_kernel, the pair's one kernel:
//    runs of one tile are the stand-alone tiling; three layers and UpFeed keep resstack64_kernel).
//
// Large dilations (49) cannot be fused (the halo would be the tile); they run through the same
// kernel as single layers on polyphase row sets (x[phase + dil * j] is a dilation-1 convolution in j),
// which in the transposed layout costs nothing extra: every lane stores its own row anyway.
//
// Image layout (as resconv16_kernel): one row = 64 channels as 128 B of fp16 hi + 128 B of fp16 lo +
// 16 B pad (272 B: the 16-byte fragment reads of 32 consecutive rows are bank-conflict free).  Weights
// never touch LDS: MFMA-fragment order (asw_pack_fragments_f16), one coalesced 1 KiB load per fragment,
// QD k-steps ahead.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "asw_common.h"
#include "f16x3_tile.h"

namespace {
using namespace asw_mfma;

constexpr int C = 64;
constexpr int MAXL = 3;
// The one tile shape: NW waves, each owning TM 32-row fragments x all 64 channels (two waves per SIMD), weights
// prefetched QD k-steps ahead.
constexpr int NW = 4, TM = 2, QD = 4;
constexpr int NTHR = 64 * NW, SROWS = NTHR / 16;
constexpr int R0 = 32 * NW * TM;         // rows layer 0 computes

// The runs of the fused pair.  An item's rows are cut into `nrun` runs, each a head tile of BM rows followed by steady
// tiles of R0 rows (n tiles cover BM + (n - 1) R0 rows); the item's tiles are dealt to the runs as evenly as they go,
// the runs with one tile more last, so that only the item's very last tile is ragged and none is empty.
struct RunPlan {
  int nrun, q, long0;                    // runs per item; tiles of a short run; index of the first run with q + 1 tiles
  ASW_HOST_DEVICE int tiles(int run) const { return q + (run >= long0 ? 1 : 0); }
  ASW_HOST_DEVICE int start(int run, int BM) const { return run * (BM + (q - 1) * R0) + (run - long0 > 0 ? run - long0 : 0) * R0; }
};

struct LayerDev {
  const half8* Wh;
  const half8* Wl;
  const float* bias;
  const float* gamma;
  const float* beta;
  int dil, pad;
  int halo;                              // rows of halo still needed AFTER this layer (sum of later pads)
  int nfrag;                             // 32-row fragments this layer computes
  float scale;                           // 2^-w_shift
};

struct KArgs {
  const float* x;
  float* out;
  const float* glu_raw;
  const float* glu_mr;
  const float* glu_gamma;
  const float* glu_beta;
  float* glu_out;                        // optional: the GroupNorm + GLU rows of this tile's own output range, fp32
  const half8* src_h;                    // SRC: the 8-channel source rows [B][T][8], fp16 hi / lo planes (16 B per row each)
  const half8* src_l;
  const half8* Pre_h;                    // SRC: the 1x1 weight [64][16] that rebuilds layer 0's residual, fragment order
  const half8* Pre_l;
  float pre_up, pre_down;                // SRC: 2^pre_shift and its inverse
  int B, T, taps, ntile, BM, img_rows;
  RunPlan runs;                          // the fused pair: the runs of an item
  float eps;
  LayerDev L[MAXL];
};

// UpFeed (asw_resstack_args.up_hi): the transposed convolution of the next decoder block, applied by the last layer
constexpr int UPN = 256;                 // its GEMM width: stride 2 x (64 value + 64 gate) channels
struct UpArgs {
  const half8* Wh;                       // Wt[256][64] with the K order of asw_up_feed_kperm, fragment order
  const half8* Wl;
  const float* bias;                     // [256]
  const float* skip;                     // [B][T][64], added to the stack's output before the GEMM
  float* out;                            // [B][T][256] == [B][2 T][128] raw rows
  float* stats;                          // [B][ntile][4]: sum, sum of squares of the value half, then of the gate half
  float scale;                           // 2^-w_shift
};
struct KArgsUp : KArgs { UpArgs u; };    // the kernel argument of the UpFeed instantiations

// Diagnostic build only (-DASW_PHASE_TIMING, tests/micro/resstack_phases.py): cycles wave 0 of every workgroup spends
// per phase, summed over workgroups: [0] staging, [1] layer-0 k-loop, [2] layer-0 epilogue + hand-over, [3] layer-1
// k-loop, [4] layer-1 epilogue + stores, [5] workgroups (the carried-halo kernel: tiles).  Stamps: 0 start, 1 staged, 2 + 2 li after layer li's
// k-loop, 3 + 2 li after layer li.
#ifdef ASW_PHASE_TIMING
__device__ unsigned long long g_rs_cycles[6] = {0, 0, 0, 0, 0, 0};
struct PhaseClock {
  unsigned long long t[2 * MAXL + 2];
  __device__ __forceinline__ void mark(int i) { t[i] = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void mark_after(int i, float sink) {
    asm volatile("" ::"v"(sink));                           // the stamp waits for the MFMAs
    mark(i);
  }
  template <int NL>
  __device__ __forceinline__ void report() const {
    if (threadIdx.x != 0 || NL > 2) return;
    atomicAdd(&g_rs_cycles[0], t[1] - t[0]);
    atomicAdd(&g_rs_cycles[1], t[2] - t[1]);
    if (NL == 2) {
      atomicAdd(&g_rs_cycles[2], t[3] - t[2]);
      atomicAdd(&g_rs_cycles[3], t[4] - t[3]);
    }
    atomicAdd(&g_rs_cycles[4], t[2 * NL + 1] - t[2 * NL]);
    atomicAdd(&g_rs_cycles[5], 1ull);
  }
};
#else
struct PhaseClock {
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void mark_after(int, float) {}
  template <int NL>
  __device__ __forceinline__ void report() const {}
};
#endif

// One 16-byte row of a source plane through its buffer descriptor: rows outside [0, T) read as zeros.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t src_rsrc(const half8* base, long rows) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<half8*>(base), 0, (int)(rows * 16), 0x00020000);
}
__device__ __forceinline__ half8 src_load(__amdgpu_buffer_rsrc_t r, int row) {
  return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(r, row >= 0 ? row * 16 : (int)0x80000000, 0, 0));
}

// ------------------------------------------------------------------ the row map
// The three kinds of row of a workgroup's tile, contiguous or polyphase (POLY: PH phases of R0 / PH rows of j each,
// a fragment inside one phase), and every conversion between them:
//   image row     a row of the LDS image (layer 0's input, later each layer's output in its place)
//   fragment row  row (wave * TM + i) * 32 + (lane & 31) of the R0 rows a layer computes
//   sequence row  a row t of the [T][64] tensors in memory
template <bool POLY, int PH, bool CARRY = false>
struct RowMap {
  static constexpr int BMJ = R0 / PH;                   // polyphase: rows of j per phase
  static_assert(BMJ % 32 == 0, "a row fragment must stay inside one phase");
  int T, taps, dil0, pad0, jb, pb, m0, BM, n_img, halo0;
  // CARRY only:
  int shift;                             // rows by which layer 0's rows lie later than m0 - halo0 (a steady tile)
  int glu_lo, glu_hi;                    // (GLU on load) the sequence rows whose normalised form this tile writes out

  __device__ __forceinline__ RowMap(int tile, const KArgs& p) : T(p.T), taps(p.taps), dil0(p.L[0].dil), pad0(p.L[0].pad) {
    const int n_pb = POLY ? (dil0 + PH - 1) / PH : 1;
    jb = POLY ? tile / n_pb : 0;
    pb = POLY ? tile - jb * n_pb : 0;
    m0 = tile * p.BM;
    BM = p.BM;
    n_img = POLY ? PH * rj() : R0 + 2 * pad0;
    halo0 = p.L[0].halo;
  }
  // Tile `j` of a carried-halo run that starts at sequence row s (contiguous tiles, two layers).  The head tile (j == 0)
  // is the tile above: layer 0 computes rows m0 - halo0 .. and BM = R0 - 2 halo0 rows are delivered.  A steady tile
  // delivers R0 rows: its first 2 halo0 layer-0 rows are the previous tile's last, so layer 0 starts at m0 + halo0.
  // The normalised input rows (GLU side output) go out with the layer-0 rows a tile computes, clipped to the run.
  __device__ __forceinline__ RowMap(int s, int j, bool last, const KArgs& p) : T(p.T), taps(p.taps), dil0(p.L[0].dil), pad0(p.L[0].pad) {
    static_assert(CARRY && !POLY, "carried halo: contiguous tiles");
    const bool head = j == 0;
    jb = pb = 0;
    halo0 = p.L[0].halo;
    m0 = head ? s : s + p.BM + (j - 1) * R0;
    BM = head ? p.BM : R0;
    n_img = R0 + 2 * pad0;
    shift = head ? 0 : 2 * halo0;
    glu_lo = head ? m0 : m0 + halo0;
    glu_hi = last ? m0 + BM : m0 + BM + halo0;
  }
  __device__ __forceinline__ int rj() const { return BMJ + taps - 1; }          // polyphase: image rows per phase

  // ---- image row -> the sequence row it is staged from, and whether that row exists
  __device__ __forceinline__ ImgSrc staged_from(int irow) const {
    int g;
    bool ok = irow < n_img;
    if (!POLY) {
      g = m0 - halo0 - pad0 + (CARRY ? shift : 0) + irow;
    } else {
      const int ph = pb * PH + irow / rj();
      const int jj = jb * BMJ + irow % rj() - (taps - 1) / 2;
      g = dil0 * jj + ph;
      ok = ok && ph < dil0 && jj >= 0;
    }
    return {g, ok && g >= 0 && g < T};
  }
  // (GLU on load) is sequence row g one of the rows this tile delivers
  __device__ __forceinline__ bool delivers(int g) const { return CARRY ? g >= glu_lo && g < glu_hi : g >= m0 && g < m0 + BM; }

  // ---- fragment row -> image row at tap 0; image rows between two taps; from tap 0 to the centre tap (the residual)
  __device__ __forceinline__ int image_row(int frow) const { return POLY ? (frow / BMJ) * rj() + frow % BMJ : frow; }
  __device__ __forceinline__ int tap_rows(const LayerDev& Ld) const { return POLY ? 1 : Ld.dil; }
  __device__ __forceinline__ int centre_rows(const LayerDev& Ld, bool first) const { return POLY ? (taps - 1) / 2 : first ? pad0 : Ld.pad; }

  // ---- fragment row -> sequence row
  // a layer with `halo` rows still to come after it (contiguous tiles only): is the row inside the sequence
  __device__ __forceinline__ bool handed_on(int frow, int halo) const {
    const int t = m0 - halo + (CARRY ? shift : 0) + frow;
    return t >= 0 && t < T;
  }
  // the last layer (`ok`: a row this tile delivers)
  __device__ __forceinline__ int phase(int frow) const { return pb * PH + frow / BMJ; }
  __device__ __forceinline__ int seq_row(int frow) const { return POLY ? dil0 * (jb * BMJ + frow % BMJ) + phase(frow) : m0 + frow; }
  __device__ __forceinline__ ImgSrc delivered(int frow) const {
    const int t = seq_row(frow);
    return {t, (POLY ? phase(frow) < dil0 : frow < BM) && t < T};
  }
  // sequence rows between two rows of a fragment; the delivered rows of the fragment that starts at fragment row f0
  // are a prefix of it: their number, not yet clamped to [0, 32]
  __device__ __forceinline__ int row_step() const { return POLY ? dil0 : 1; }
  __device__ __forceinline__ int run_rows(int f0) const {
    if (!POLY) return min(BM, T - m0) - f0;
    const int t0 = seq_row(f0);
    return (phase(f0) < dil0 && t0 < T) ? (T - 1 - t0) / dil0 + 1 : 0;
  }
};

// this lane's row of its wave's fragment i, as a fragment row
__device__ __forceinline__ int frag_row(int wid, int i, int lane) { return (wid * TM + i) * 32 + (lane & 31); }

// This wave's fragments that exist in a layer, f(i) for i < nf.  Written out, not a loop over i: each phase is
// optimised on its own before it is inlined, its channel walks unrolled by then, and from a loop the per-channel table
// and image addresses of all fragments were hoisted in front of the first one (+8 VGPRs, the single-pass kernels' fourth
// wave per SIMD).
template <typename F>
__device__ __forceinline__ void for_each_fragment(int nf, const F& f) {
  static_assert(TM == 2, "one line per fragment");
  if (0 < nf) f(0);
  if (1 < nf) f(1);
}

// ------------------------------------------------------------------ the channel walk
// A lane (half h = lane >> 5) holds sixteen groups of four consecutive channels of its row: group q of the 32-channel
// block cb is registers 4 q .. 4 q + 3 of acc[cb] and channels c0 .. c0 + 3.  f(cb, q, c0), in register order.
template <typename F>
__device__ __forceinline__ void for_each_group(int h, const F& f) {
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) f(cb, q, cb * 32 + q * 8 + h * 4);
}
__device__ __forceinline__ float4 group4(const floatx16& a, int q) { return make_float4(a[q * 4 + 0], a[q * 4 + 1], a[q * 4 + 2], a[q * 4 + 3]); }

// ------------------------------------------------------------------ the phases
// The per-layer vectors in LDS, tab[NL][bias | gamma | beta][64], as float4 groups STRIDE bytes apart: one array behind
// the image (STRIDE 16), or -- the carried-halo form, whose image leaves no room behind it -- group i in the 16 pad
// bytes of image row i (STRIDE RS), which no staging, hand-over or fragment read touches.
template <int STRIDE>
struct Tab {
  static_assert(STRIDE % 16 == 0, "float4 groups");
  float* p;
  __device__ __forceinline__ float4& at(int word) const { return *reinterpret_cast<float4*>(p + word * (STRIDE / 16)); }
  __device__ __forceinline__ Tab layer(int li) const { return {p + li * 192 * (STRIDE / 16)}; }
};

// per-layer vectors -> LDS
template <int NL, typename TabT>
__device__ __forceinline__ void load_layer_vectors(const KArgs& p, TabT tab, int tid) {
  for (int i = tid; i < NL * 3 * 16; i += NTHR) {
    const int li = i / 48, w = (i - li * 48) / 16, c4 = i & 15;
    const float* src = w == 0 ? p.L[li].bias : w == 1 ? p.L[li].gamma : p.L[li].beta;
    tab.at(i * 4) = *reinterpret_cast<const float4*>(src + c4 * 4);
  }
}

// stage + split the input rows of layer 0 (16 threads per row, 8 rows per thread in flight)
template <bool GLU, int NTERM, typename Map>
__device__ __forceinline__ void stage_rows(const KArgs& p, const Map& map, int b, char* img, int tid) {
  const int T = map.T;
  const __amdgpu_buffer_rsrc_t rX = GLU ? act_rsrc(p.glu_raw + (long)b * T * 2 * C, (long)T * 2 * C)
                                        : act_rsrc(p.x + (long)b * T * C, (long)T * C);
  const int srow = tid >> 4, sc4 = tid & 15;
  const int R_img = map.n_img;
  GluCoef gc;
  if (GLU) {
    gc.stats(p.glu_mr, b);
    gc.affine(p.glu_gamma, p.glu_beta, C, sc4 * 4);
  }
  // (This loop stays here instead of calling stage_image of f16x3_tile.h, which resconv16 and downconv64 use: through
  // the shared routine the GLU variant of the fused pair measured 0.7 % slower, 11.11 -> 11.21 ms per bench step.)
  // the whole image is requested before the first row is converted: one exposed memory latency per tile (with 8
  // rows per thread in flight the three rounds of a 262-row image took 17 % of a workgroup's time)
  constexpr int SU = GLU ? 9 : 18;
  for (int r0 = 0; r0 < R_img; r0 += SROWS * SU) {
    float4 buf[SU];
    float4 gate[GLU ? SU : 1];
    bool okr[GLU ? SU : 1];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const ImgSrc f = map.staged_from(r0 + u * SROWS + srow);
      if (GLU) {
        buf[u] = act_load4(rX, (long)f.g * 2 * C + sc4 * 4, f.ok);
        gate[u] = act_load4(rX, (long)f.g * 2 * C + C + sc4 * 4, f.ok);
        okr[u] = f.ok;
        // (each row's two loads go out as soon as their address is there: left alone, the scheduler computed all nine
        // addresses first and the GLU pair measured 0.65 % slower, 10.92 -> 10.99 ms per bench step)
        __builtin_amdgcn_sched_barrier(0);
      } else {
        buf[u] = act_load4(rX, (long)f.g * C + sc4 * 4, f.ok);
      }
    }
    if (GLU) {
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const float4 o = gn_glu4(buf[u], gate[u], gc, okr[u]);
        buf[u] = o;
        // the normalised tensor is also a skip connection: each tile writes the rows of its own output range once
        if (p.glu_out && okr[u]) {
          const int g = map.staged_from(r0 + u * SROWS + srow).g;
          if (map.delivers(g)) *reinterpret_cast<float4*>(p.glu_out + ((long)b * T + g) * C + sc4 * 4) = o;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int row = r0 + u * SROWS + srow;
      if (row < R_img) {
        half4 hi, lo;
        split4t<NTERM>(buf[u], hi, lo);
        *reinterpret_cast<half4*>(img + row * RS + IMG_HI + sc4 * 8) = hi;
        *reinterpret_cast<half4*>(img + row * RS + IMG_LO + sc4 * 8) = lo;      // (the residual reads it in every mode)
      }
    }
  }
}

// SRC: layer 0 on the source planes, up to and including its residual; also brings the per-layer vectors to LDS.
// (Every wave owns TM whole fragments here: nfrag == NW * TM, checked by the host.)
// Lane (row r, half h) holds, for k-step ks, the 8 source channels of row r + tap, tap = 2 ks + h: one 16-byte
// load per plane.  Tap 7 does not exist -- its weights are zero -- but its rows are read and are finite (data or
// the descriptor's zeros).  Everything is requested before the first MFMA: one exposed latency per tile.
// (load_tab: false on the later tiles of a carried-halo run, whose vectors are in LDS already; the barrier stays, and
// there it also keeps the hand-over behind the previous tile's last reads of the image.  wofs: as in conv_layer.)
template <int NL, typename Map, typename TabT>
__device__ __forceinline__ void source_layer0(const KArgs& p, const Map& map, int b, TabT tab, bool load_tab, int wofs, int tid,
                                              floatx16 (&acc)[TM][2]) {
  const LayerDev& Ld = p.L[0];
  const int T = map.T, lane = tid & 63, wid = tid >> 6, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t rH = src_rsrc(p.src_h + (long)b * T, T), rL = src_rsrc(p.src_l + (long)b * T, T);
  const int g0 = map.staged_from(frag_row(wid, 0, lane)).g;                     // global row of this lane's row at tap 0
  half8 xh[4][TM], xl[4][TM], rh[TM], rl[TM];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      xh[ks][i] = src_load(rH, g0 + i * 32 + 2 * ks + h);
      xl[ks][i] = src_load(rL, g0 + i * 32 + 2 * ks + h);
    }
#pragma unroll
  for (int i = 0; i < TM; ++i) {                        // the residual's rows (centre tap); the half h == 1 meets zero weights
    rh[i] = src_load(rH, g0 + i * 32 + map.centre_rows(Ld, true));
    rl[i] = src_load(rL, g0 + i * 32 + map.centre_rows(Ld, true));
  }
  // weight stream: k-steps 0..3 of the composed weight, then the 1x1 weight as "k-step 4"; two slots
  half8 wh[2][2], wl[2][2];
  auto wload = [&](auto kgc, int slot) {
    constexpr int kg = decltype(kgc)::value;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      if constexpr (kg < 4) frag_load<3>(Ld.Wh, Ld.Wl, (long)kg * 2 + cb + wofs, lane, wh[slot][cb], wl[slot][cb]);
      else frag_load<3>(p.Pre_h, p.Pre_l, (long)cb + wofs, lane, wh[slot][cb], wl[slot][cb]);
    }
  };
  wload(std::integral_constant<int, 0>{}, 0);
  wload(std::integral_constant<int, 1>{}, 1);
  if (load_tab) load_layer_vectors<NL>(p, tab, tid);    // (here: after layer 0's operand loads are out, under the same wait)
  __syncthreads();
  auto kstep = [&](auto ksc) {
    constexpr int ks = decltype(ksc)::value;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) mma3<3, true>(acc[i][cb], xh[ks][i], xl[ks][i], wh[ks & 1][cb], wl[ks & 1][cb]);
    if constexpr (ks + 2 <= 4) wload(std::integral_constant<int, ks + 2>{}, ks & 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  kstep(std::integral_constant<int, 0>{});
  kstep(std::integral_constant<int, 1>{});
  kstep(std::integral_constant<int, 2>{});
  kstep(std::integral_constant<int, 3>{});
  // + bias, ReLU -- brought to the units of the 1x1 weight (both weights carry a power-of-two pre-scale, so the
  // rescaling is exact) -- then the residual x0 = Wpre~ u~ accumulated on top: no second accumulator set
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    for_each_group(h, [&](int cb, int q, int c0) __attribute__((always_inline)) {
      const float4 bi = tab.at(c0);
      const float bv[4] = {bi.x, bi.y, bi.z, bi.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][cb][q * 4 + j] = fmaxf(acc[i][cb][q * 4 + j] * Ld.scale + bv[j], 0.f) * p.pre_up;
    });
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) mma3<3, true>(acc[i][cb], rh[i], rl[i], wh[0][cb], wl[0][cb]);
  }
}

// the convolution of one layer from the image: this wave's first nf (<= TM) fragments, one k-loop instantiation per
// count (wave-uniform choice; nf <= 0: none).  WOFS: wofs is added to every weight fragment's index (the carried-halo
// kernel's opaque zero).
template <int NTERM, bool WOFS, typename Map>
__device__ __forceinline__ void conv_layer(const KArgs& p, const LayerDev& Ld, const Map& map, const char* img, int nf, int wofs,
                                           int lane, int wid, floatx16 (&acc)[TM][2]) {
  const int taps = map.taps, h = lane >> 5;
  const int tapstep = map.tap_rows(Ld) * RS;
  auto run = [&](auto nfc) {
    constexpr int NF = decltype(nfc)::value;
    int xb[NF];
    floatx16 a[NF][2];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      xb[i] = (map.image_row((wid * TM + i) * 32) + (lane & 31)) * RS + h * 16;
      a[i][0] = acc[i][0];
      a[i][1] = acc[i][1];
    }
    if constexpr (WOFS)
      kloop<NF, 2, QD, NTERM>(
          a, taps, [&](int tap, int i) __attribute__((always_inline)) { return img + xb[i] + tap * tapstep; }, Ld.Wh, Ld.Wl,
          [wofs](int kg, int cb) __attribute__((always_inline)) { return (long)kg * 2 + cb + wofs; }, lane);
    else
      kloop<NF, 2, QD, NTERM>(
          a, taps, [&](int tap, int i) __attribute__((always_inline)) { return img + xb[i] + tap * tapstep; }, Ld.Wh, Ld.Wl,
          [](int kg, int cb) __attribute__((always_inline)) { return (long)kg * 2 + cb; }, lane);
#pragma unroll
    for (int i = 0; i < NF; ++i) { acc[i][0] = a[i][0]; acc[i][1] = a[i][1]; }
  };
  if (nf >= TM) run(std::integral_constant<int, TM>{});
  else if (nf == 1) run(std::integral_constant<int, 1>{});
}

// the epilogue in registers: + bias, ReLU, + residual (the layer's own input, from the image), LayerNorm.
// IN_ACC (the source-fed layer 0): bias, ReLU and residual are in the accumulators already.
template <bool IN_ACC, bool FUSED_VAR, typename Map, typename TabT>
__device__ __forceinline__ void finish_rows(const KArgs& p, const LayerDev& Ld, const Map& map, const char* img, const TabT tb,
                                            bool first, int nf, int lane, int wid, floatx16 (&acc)[TM][2]) {
  const int h = lane >> 5;
  const int cpad = map.centre_rows(Ld, first);                 // image row of the residual = tap-0 row + centre tap
  for_each_fragment(nf, [&](int i) __attribute__((always_inline)) {
    const char* rrow = img + (map.image_row(frag_row(wid, i, lane)) + cpad) * RS;
    float s = 0.f;
    for_each_group(h, [&](int cb, int q, int c0) __attribute__((always_inline)) {
      const float4 bi = tb.at(c0);
      const half4 rh = *reinterpret_cast<const half4*>(rrow + IMG_HI + c0 * 2);
      const half4 rl = *reinterpret_cast<const half4*>(rrow + IMG_LO + c0 * 2);
      const float bv[4] = {bi.x, bi.y, bi.z, bi.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v;
        if constexpr (IN_ACC) {
          v = acc[i][cb][q * 4 + j] * p.pre_down;
        } else {
          v = fmaxf(acc[i][cb][q * 4 + j] * Ld.scale + bv[j], 0.f);
          v += (float)rh[j] + (float)rl[j];
        }
        acc[i][cb][q * 4 + j] = v;
        s += v;
      }
    });
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.0f / C);
    float d = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float cx = acc[i][cb][r] - mean;
        // (Said term by term, not left to contraction, so that every form keeps the bits it has always produced: the
        // compiler used to round each product and then add -- packed multiplies -- except in the UpFeed
        // instantiations, where it fused the first 26 terms into multiply-adds and rounded the last 6 products.)
        if (FUSED_VAR && cb * 16 + r < 26) {
          d = __builtin_fmaf(cx, cx, d);
        } else {
#pragma clang fp contract(off)
          d += cx * cx;
        }
      }
    d += __shfl_xor(d, 32, 64);
    const float rstd = 1.0f / sqrtf(d * (1.0f / C) + p.eps);
    for_each_group(h, [&](int cb, int q, int c0) __attribute__((always_inline)) {
      const float4 g4 = tb.at(64 + c0);
      const float4 b4 = tb.at(128 + c0);
      const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, be[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][cb][q * 4 + j] = (acc[i][cb][q * 4 + j] - mean) * rstd * gv[j] + be[j];
    });
  });
}

// the next layer's input replaces this layer's in the image, from image row `row0` on (0, or the carried rows of a
// steady tile): rows outside the sequence are its zero padding
template <int NTERM, typename Map>
__device__ __forceinline__ void hand_over(const LayerDev& Ld, const Map& map, char* img, int row0, int nf, int lane, int wid,
                                          const floatx16 (&acc)[TM][2]) {
  for_each_fragment(nf, [&](int i) __attribute__((always_inline)) {
    const int frow = frag_row(wid, i, lane);
    const bool inside = map.handed_on(frow, Ld.halo);
    char* wrow = img + (row0 + frow) * RS;
    for_each_group(lane >> 5, [&](int cb, int q, int c0) __attribute__((always_inline)) {
      float4 v = group4(acc[i][cb], q);
      if (!inside) v = make_float4(0.f, 0.f, 0.f, 0.f);
      half4 hi, lo;
      split4t<NTERM>(v, hi, lo);
      *reinterpret_cast<half4*>(wrow + IMG_HI + c0 * 2) = hi;
      *reinterpret_cast<half4*>(wrow + IMG_LO + c0 * 2) = lo;
    });
  });
}

// UpFeed.  The GEMM runs with the activation as the MFMA A operand (the same registers serve either side:
// lane = row, 8 k per lane half), so a result block has its output CHANNEL on the lane and 16 rows in registers:
// one store instruction writes two whole 128-byte lines, and a lane's 16 values share a GroupNorm group.
template <int NTERM, typename Map>
__device__ __forceinline__ void up_feed(const KArgs& p, const UpArgs& u, const LayerDev& Ld, const Map& map, int b, int tile,
                                        char* smem, int tid, const floatx16 (&acc)[TM][2]) {
  const int T = map.T, lane = tid & 63, wid = tid >> 6, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t rS = act_rsrc(u.skip + (long)b * T * C, (long)T * C);
  const int tstep = map.row_step();                     // sequence rows between two rows of a fragment
  const int widu = __builtin_amdgcn_readfirstlane(wid); // (the row bookkeeping and the store bases stay scalar)
  half8 xh[TM][4], xl[TM][4];
  int t0[TM], nv[TM];                                   // sequence row of a fragment's row 0; its rows that exist (a prefix)
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int f0 = (widu * TM + i) * 32;
    t0[i] = map.seq_row(f0);
    const int lim = map.run_rows(f0);
    nv[i] = i < Ld.nfrag - widu * TM ? min(max(lim, 0), 32) : 0;
    const bool ok = (lane & 31) < nv[i];
    const long e0 = ((long)t0[i] + (long)(lane & 31) * tstep) * C + h * 4;
    float4 sk[8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) sk[c8] = act_load4(rS, e0 + c8 * 8, ok);
    for_each_group(h, [&](int cb, int q, int) __attribute__((always_inline)) {
      const float4 s4 = sk[cb * 4 + q];
      const float4 v = make_float4(acc[i][cb][q * 4 + 0] + s4.x, acc[i][cb][q * 4 + 1] + s4.y,
                                   acc[i][cb][q * 4 + 2] + s4.z, acc[i][cb][q * 4 + 3] + s4.w);
      half4 hi, lo;
      split4t<NTERM>(v, hi, lo);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xh[i][cb * 2 + (q >> 1)][(q & 1) * 4 + j] = hi[j];
        xl[i][cb * 2 + (q >> 1)][(q & 1) * 4 + j] = lo[j];
      }
    });
  }
  float st0 = 0.f, sq0 = 0.f, st1 = 0.f, sq1 = 0.f;
  // Stores go through one buffer descriptor per fragment that covers exactly its rows that exist: the address is one
  // 32-bit offset, and a row past the end (of the sequence, or of this tile's share) is dropped by the bounds
  // check instead of by a branch.
  __amdgpu_buffer_rsrc_t rO[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
    rO[i] = __builtin_amdgcn_make_buffer_rsrc(u.out + ((long)b * T + t0[i]) * UPN, 0,
                                              nv[i] > 0 ? ((nv[i] - 1) * tstep + 1) * UPN * 4 : 0, 0x00020000);
  const int voff = (4 * h * tstep * UPN + (lane & 31)) * 4; // this lane's part of a store address: its first row, its channel
  const int rstep = tstep * UPN * 4;
  half8 wh[2][2], wl[2][2];
  auto wload = [&](int ks, int nb2, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 2; ++e) frag_load<NTERM>(u.Wh, u.Wl, (long)ks * (UPN / 32) + nb2 * 2 + e, lane, wh[slot][e], wl[slot][e]);
  };
  wload(0, 0, 0);
#pragma unroll 1
  for (int nb2 = 0; nb2 < UPN / 64; ++nb2) {            // two 32-channel blocks at a time: 0, 2 the value half, 1, 3 the gate half
    floatx16 y[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[i][e][r] = 0.f;
    const float bv[2] = {u.bias[nb2 * 64 + (lane & 31)], u.bias[nb2 * 64 + 32 + (lane & 31)]};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // the next k-step's weights (after the last one: the next pair's first, the last pair fetching its own again)
      if (ks < 3) wload(ks + 1, nb2, (ks + 1) & 1);
      else wload(0, nb2 + 1 < UPN / 64 ? nb2 + 1 : nb2, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) mma3<NTERM, false>(y[i][e], xh[i][ks], xl[i][ks], wh[ks & 1][e], wl[ks & 1][e]);
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const bool whole = nv[i] == 32;                   // (wave-uniform) every row of the fragment exists
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = y[i][e][r] * u.scale + bv[e];
          // (the whole offset in the vector operand: that is the one the bounds check compares)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rO[i],
                                                voff + ((r & 3) + 8 * (r >> 2)) * rstep + (nb2 * 64 + e * 32) * 4, 0, 0);
          const float m = (whole || acc_row(r, h) < nv[i]) ? v : 0.f;
          s1 += m;
          s2 += m * m;
        }
    }
    if (nb2 & 1) { st1 += s1; sq1 += s2; } else { st0 += s1; sq0 += s2; }
  }
  // GroupNorm partial sums of this tile: lanes, then waves, in a fixed order; one slot per (item, tile), no atomics
  st0 = wave_sum(st0); sq0 = wave_sum(sq0); st1 = wave_sum(st1); sq1 = wave_sum(sq1);
  __syncthreads();                                      // every wave is done with the image
  float* red = reinterpret_cast<float*>(smem);
  if (lane == 0) { red[wid * 4 + 0] = st0; red[wid * 4 + 1] = sq0; red[wid * 4 + 2] = st1; red[wid * 4 + 3] = sq1; }
  __syncthreads();
  if (tid < 4) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w * 4 + tid];
    u.stats[((long)b * p.ntile + tile) * 4 + tid] = s;
  }
}

// the stack's output: the rows of this tile that it delivers, one float4 per group
template <typename Map>
__device__ __forceinline__ void store_rows(const KArgs& p, const Map& map, int b, int nf, int lane, int wid,
                                           const floatx16 (&acc)[TM][2]) {
  float* __restrict__ ob = p.out + (long)b * map.T * C;
  for_each_fragment(nf, [&](int i) __attribute__((always_inline)) {
    const ImgSrc o = map.delivered(frag_row(wid, i, lane));
    if (o.ok) {
      float* orow = ob + (long)o.g * C;
      for_each_group(lane >> 5, [&](int cb, int q, int c0) __attribute__((always_inline)) {
        *reinterpret_cast<float4*>(orow + c0) = group4(acc[i][cb], q);
      });
    }
  });
}

// ------------------------------------------------------------------ the kernel
// NL fused layers (contiguous row tiles) or one layer on polyphase row sets (POLY, NL == 1).
// NW waves, each owning TM 32-row fragments x all 64 channels.  The pair comes here as UpFeed only: without it, it is
// resstack64_carry_kernel's.
//
// UP ("UpFeed", f16x3): the stack is the last of a decoder block and the next block is a 64 -> 64 channel stride-2
// transposed convolution.  That convolution is a one-tap GEMM over channels of (x + skip), and a finished LayerNorm
// row fragment already sits in registers in an MFMA operand layout (lane = time row; registers 8s .. 8s+7 of the
// 32-channel block cb are k-step 2 cb + s, up to a fixed order of the 16 channels inside the step that the host
// folds into the packed weight, asw_up_feed_kperm).  So the last layer adds the skip rows, splits the sum, runs
// W_up (x + skip) + bias for the 256 output channels from registers and writes the raw rows and their GroupNorm
// partial sums (UpArgs).  x is never stored: one write and one read of it and one launch less.
template <int NL, int PH, bool POLY, bool GLU, int NTERM, bool UP = false>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2)))
void resstack64_kernel(const std::conditional_t<UP, KArgsUp, KArgs> p) {
  static_assert(!UP || NTERM == 3, "UpFeed: f16x3");
  static_assert(!POLY || NL == 1, "polyphase row sets: single layers only");
  static_assert(NL != 2 || UP, "the pair without UpFeed: resstack64_carry_kernel");

  extern __shared__ __align__(16) char smem[];
  char* img = smem;
  const Tab<16> tab = {reinterpret_cast<float*>(smem + (size_t)p.img_rows * RS)};    // [NL][bias | gamma | beta][64]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int idx;
  if (!xcd_tile_run(p.B * p.ntile, idx)) return;        // XCD-aware order: a contiguous run of (item, row tile) pairs
  const int b = idx / p.ntile, tile = idx - b * p.ntile;
  const RowMap<POLY, PH> map(tile, p);

  PhaseClock clk;
  clk.mark(0);
  load_layer_vectors<NL>(p, tab, tid);
  stage_rows<GLU, NTERM>(p, map, b, img, tid);
  __syncthreads();
  clk.mark(1);

  floatx16 acc[TM][2];
  auto layer = [&](auto lic) {
    constexpr int li = decltype(lic)::value;
    const LayerDev& Ld = p.L[li];
    const int nf = Ld.nfrag - wid * TM;                 // fragments of this wave that exist in this layer (<= 0: none)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][cb][r] = 0.f;        // (all of acc defined on every path: it stays in registers)
    conv_layer<NTERM, false>(p, Ld, map, img, nf, 0, lane, wid, acc);
    clk.mark_after(2 + 2 * li, acc[0][0][0]);
    finish_rows<false, UP>(p, Ld, map, img, tab.layer(li), li == 0, nf, lane, wid, acc);
    if constexpr (li < NL - 1) {
      __syncthreads();                                  // every wave is done reading the old image
      hand_over<NTERM>(Ld, map, img, 0, nf, lane, wid, acc);
      __syncthreads();
    } else if constexpr (UP) {
      up_feed<NTERM>(p, p.u, Ld, map, b, tile, smem, tid, acc);
    } else {
      store_rows(p, map, b, nf, lane, wid, acc);
    }
    clk.mark(3 + 2 * li);
  };
  layer(std::integral_constant<int, 0>{});
  if constexpr (NL > 1) layer(std::integral_constant<int, 1>{});
  if constexpr (NL > 2) layer(std::integral_constant<int, 2>{});
  clk.report<NL>();
}

// The fused pair (contiguous tiles, never UpFeed), its halo carried.  A workgroup owns a RUN (RunPlan) of consecutive row
// tiles of one item and walks them in time order.  The first tile of a run is the tile of the kernel above: R0 layer-0
// rows, of which layer 1 can finish BM = R0 - 2 halo.  Every later tile finishes R0 rows: the 2 halo layer-0 rows in
// front of its own are the previous tile's last -- split to fp16 hi / lo as hand_over left them -- and travel in
// registers (CQ 16-byte pieces per thread) across the staging and layer 0 of the new tile, whose hand-over puts them in
// front of the R0 new rows.  Both layers then run NW * TM whole fragments and no layer-0 row is computed twice inside
// a run.  The image of layer 1 is R0 + 2 halo rows, which leaves no room behind it at two workgroups per CU: the
// per-layer vectors live in the rows' pad bytes (Tab), loaded once per run.  A row's arithmetic does not depend on the
// tile that computes it: a plan of one tile per run IS the recomputed-halo tiling (the host's, on request or where
// nothing can be carried; the image is then the rows a head tile needs) and gives the same results bit for bit.
//
// SRC: layer 0's input x0 is itself a 1x1 convolution of an 8-channel source u~ = (u_0 .. u_6, 1) (zero outside the
// sequence), x0[t] = Wpre~ u~[t], which nothing non-linear separates from layer 0's convolution.  Layer 0 then runs
// on u~ with the composed weights Wc_k Wpre~ (k index = tap * 8 + channel: 4 k-steps of two taps each instead of
// taps x 4), its B operand loaded straight from the two fp16 planes of u~ -- a fragment is 32 consecutive 16-byte
// rows -- with no LDS image and no staging pass; the residual x0 is one more k-step with Wpre~ (K = 8 padded to 16)
// accumulated onto the ReLU'd accumulators.  x0 is never materialised.
constexpr int CQ = 3;                    // 16-byte pieces of carried rows per thread: 2 halo <= CQ * NTHR / 16 = 48 rows
template <bool GLU, int NTERM, bool SRC>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2)))
void resstack64_carry_kernel(const KArgs p) {
  static_assert(!SRC || (!GLU && NTERM == 3), "source-fed layer 0: f16x3");
  constexpr int NL = 2;
  static_assert(R0 >= NL * 3 * 16, "one float4 group of the per-layer vectors per image row");
  using Map = RowMap<false, 1, true>;

  extern __shared__ __align__(16) char smem[];
  char* img = smem;
  const Tab<RS> tab = {reinterpret_cast<float*>(smem + IMG_LO + C * 2)};       // [NL][bias | gamma | beta][64] in the rows' pad bytes

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int idx;
  if (!xcd_tile_run(p.B * p.runs.nrun, idx)) return;    // XCD-aware order: a contiguous run of (item, run) pairs
  const int b = idx / p.runs.nrun, run = idx - b * p.runs.nrun;
  const int s = p.runs.start(run, p.BM), n = p.runs.tiles(run);
  const int crows = 2 * p.L[0].halo;                    // rows carried from tile to tile

  PhaseClock clk;
  floatx16 acc[TM][2];
  half8 carry[CQ];                                      // this thread's pieces of the carried rows
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    const bool steady = j > 0;
    const Map map(s, j, j == n - 1, p);
    if (map.m0 >= p.T) break;                           // (the planner leaves no such tile)
    // The weight addresses are made opaque tile by tile.  Left as loop invariants, the first QD k-steps of both
    // layers' weights were loaded once in front of the loop and held across it: 256 VGPRs and scratch.
    // (wofs: a zero the compiler cannot see through, uniform, added to every weight fragment's index.)
    int wofs = 0;
    asm volatile("" : "+v"(wofs));
    wofs = __builtin_amdgcn_readfirstlane(wofs);

    clk.mark(0);
    if constexpr (!SRC) {                               // (SRC: source_layer0 loads the vectors and has nothing to stage)
      if (steady) __syncthreads();                      // every wave is done with the previous tile's image
      else load_layer_vectors<NL>(p, tab, tid);
      stage_rows<GLU, NTERM>(p, map, b, img, tid);
      __syncthreads();
    }
    clk.mark(1);

    auto layer = [&](auto lic) __attribute__((always_inline)) {
      constexpr int li = decltype(lic)::value;
      constexpr bool fed = SRC && li == 0;
      const LayerDev& Ld = p.L[li];
      // fragments of this wave in this layer: all of them, but for layer 1 of the head tile
      const int nf = (li == 0 || steady ? NW * TM : Ld.nfrag) - wid * TM;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][cb][r] = 0.f;
      if constexpr (fed) source_layer0<NL>(p, map, b, tab, !steady, wofs, tid, acc);
      else conv_layer<NTERM, true>(p, Ld, map, img, nf, wofs, lane, wid, acc);
      clk.mark_after(2 + 2 * li, acc[0][0][0]);
      finish_rows<fed, false>(p, Ld, map, img, tab.layer(li), li == 0, nf, lane, wid, acc);
      if constexpr (li == 0) {
        if constexpr (!fed) __syncthreads();            // every wave is done reading the old image
        hand_over<NTERM>(Ld, map, img, steady ? crows : 0, nf, lane, wid, acc);
        if (steady) {                                   // the carried rows in front of the new ones
#pragma unroll
          for (int k = 0; k < CQ; ++k) {
            const int c = tid + k * NTHR;
            if (c < crows * 16) *reinterpret_cast<half8*>(img + (c >> 4) * RS + (c & 15) * 16) = carry[k];
          }
        }
        __syncthreads();
      } else {
        store_rows(p, map, b, nf, lane, wid, acc);
      }
      clk.mark(3 + 2 * li);
    };
    layer(std::integral_constant<int, 0>{});
    layer(std::integral_constant<int, 1>{});
    clk.report<NL>();                                   // (diagnostic build: per tile)

    if (j + 1 < n) {                                    // the next tile starts from the last `crows` layer-0 rows of this image
#pragma unroll
      for (int k = 0; k < CQ; ++k) {
        const int c = tid + k * NTHR;
        if (c < crows * 16) carry[k] = *reinterpret_cast<const half8*>(img + (map.BM + (c >> 4)) * RS + (c & 15) * 16);
      }
    }
  }
}

// ------------------------------------------------------------------ launch
template <bool GLU, bool SRC, bool UP>
double stack_bytes(const KArgs& k) {
  const double rows = (double)k.B * k.T;
  // f16x3 only; algorithmic bytes: the two source planes read once, the output written once
  if (SRC) return rows * (32 + C * 4);
  // algorithmic bytes: the stack's input and the skip rows read once, the raw rows written once
  if (UP) return rows * 4 * ((GLU ? 3 : 2) * C + UPN);
  // algorithmic bytes: the stack's input read once, its output written once
  return rows * C * 4 * (GLU ? 3 : 2);
}

template <int NL, int PH, bool POLY, bool GLU, int NTERM, bool SRC, bool UP>
constexpr auto stack_kernel() {
  static_assert(!SRC || (NL == 2 && !UP), "source-fed layer 0: the pair without UpFeed");
  if constexpr (NL == 2 && !UP) return &resstack64_carry_kernel<GLU, NTERM, SRC>;
  else return &resstack64_kernel<NL, PH, POLY, GLU, NTERM, UP>;
}

// One form of the kernel: its single-pass and its f16x3 instantiation (SRC and UP are f16x3 only: the host has
// checked the precision).  carry (the pair without UpFeed): the plan hands rows from tile to tile, and the name says so.
template <int NL, int PH, bool POLY, bool GLU, bool SRC, bool UP>
int launch_stack(const KArgs& k, const UpArgs* up, int precision, size_t smem, double flops, hipStream_t s, bool carry = false) {
  const bool say_carry = carry && asw::prof_form();
  char nm[128], detail[48] = "";
  snprintf(nm, sizeof nm, "resstack64<%d,%dx%d%s%s%s%s%s>", NL, NW, TM, POLY ? (PH == 1 ? ",poly1" : PH == 2 ? ",poly2" : ",poly4") : "",
           say_carry ? ",carry" : "", GLU ? ",glu" : "", SRC ? ",src" : "", UP ? ",up" : "");
  if (asw::prof_detail()) {
    if (say_carry) snprintf(detail, sizeof detail, "[B%d M%d d%d r%d]", k.B, k.T, k.L[0].dil, k.runs.nrun);
    else snprintf(detail, sizeof detail, "[B%d M%d d%d]", k.B, k.T, k.L[0].dil);
  }
  std::conditional_t<UP, KArgsUp, KArgs> ka;
  static_cast<KArgs&>(ka) = k;
  if constexpr (UP) {
    ka.u = *up;
    flops += 2.0 * k.B * (double)k.T * C * UPN;
  }
  return asw::launch_pair<stack_kernel<NL, PH, POLY, GLU, (SRC || UP) ? 3 : 1, SRC, UP>(),
                          stack_kernel<NL, PH, POLY, GLU, 3, SRC, UP>()>(
      precision, dim3(xcd_grid_run(k.B * (NL == 2 && !UP ? k.runs.nrun : k.ntile))), dim3(NTHR), smem, 160 * 1024, nm, detail,
      flops, stack_bytes<GLU, SRC, UP>(k), s, ka);                // (the pair without UpFeed: a workgroup per run, not per tile)
}

// the staged forms of a tiling: GroupNorm + GLU on load (contiguous tiles only) or not, UpFeed or not (the pair comes
// here as UpFeed only: dispatch)
template <int NL, int PH, bool POLY>
int launch_staged(const KArgs& k, const UpArgs* up, bool glu, int precision, size_t smem, double flops, hipStream_t s) {
  auto form = [&](auto gluc) {
    constexpr bool GLU = decltype(gluc)::value;
    if constexpr (NL != 2) {
      if (!up) return launch_stack<NL, PH, POLY, GLU, false, false>(k, up, precision, smem, flops, s);
    }
    return launch_stack<NL, PH, POLY, GLU, false, true>(k, up, precision, smem, flops, s);
  };
  if constexpr (!POLY) {
    if (glu) return form(std::true_type{});
  }
  return form(std::false_type{});
}

// The row tiling of a launch whose layer 0 computes R0 rows (asw_resstack_tiles reports ntile to a caller that sizes
// the UpFeed statistics).
struct TilePlan { bool poly; int PH, BM, ntile; };
TilePlan plan_tiles(int T, int n_layers, int dil0, int halo0, bool glu) {
  // one layer of large dilation: polyphase row sets while every phase still fills its share of the tile
  const int rpp = T / dil0;                              // rows per phase
  if (n_layers == 1 && dil0 >= 7 && rpp >= 48 && !glu) {
    const int PH = rpp >= R0 - 32 ? 1 : rpp >= R0 / 2 - 32 ? 2 : 4;
    return {true, PH, R0, asw::cdiv(asw::cdiv(T, dil0), R0 / PH) * asw::cdiv(dil0, PH)};
  }
  // contiguous tiles: layer 0 computes R0 rows, the stack delivers BM = R0 - 2 * (halo after layer 0)
  const int BM = R0 - 2 * halo0;
  return {false, 1, BM, BM > 0 ? asw::cdiv(T, BM) : 0};
}

// The runs of an item of T rows (RunPlan) when `want` are asked for: never more than the item has head tiles.  INT_MAX
// (dispatch, where nothing is carried) makes every tile a run of its own, at run * BM: the recomputed-halo tiling.
RunPlan plan_runs(int T, int BM, int want) {
  const int nrun = std::max(1, std::min(want, asw::cdiv(T, BM)));
  const int ntile = nrun + asw::cdiv(std::max(T - nrun * BM, 0), R0);
  return {nrun, ntile / nrun, nrun - ntile % nrun};
}
// Runs per item when the caller leaves them to the library: about four workgroups per CU in the grid (two resident
// rounds of two per CU) while B is small, and no run shorter than a head and a steady tile.
int auto_runs(int T, int BM, int B, int n_cu) {
  return std::max(1, std::min(asw::cdiv(4 * n_cu, B), T / (BM + R0)));
}
int device_cus() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus[dev] = 256;
  return cus[dev];
}
// Does the fused pair (without UpFeed) carry its halo: it is not asked to recompute it (runs_per_item < 0), there is
// more than one tile of rows, the carried rows fit the registers that hold them, and the image of a steady tile --
// R0 + 2 halo rows for layer 1 -- admits two workgroups per CU.
bool carry_applies(int T, int BM, int pad0, int halo0, int runs_per_item) {
  const int rows = R0 + 2 * std::max(pad0, halo0);
  return runs_per_item >= 0 && T > BM && halo0 > 0 && 2 * halo0 * 16 <= CQ * NTHR && (size_t)rows * RS <= 80 * 1024;
}

int dispatch(const asw_resstack_args& a, KArgs& k, const UpArgs* up, bool glu, double flops, hipStream_t s) {
  const int dil0 = k.L[0].dil;
  const TilePlan tp = plan_tiles(a.T, a.n_layers, dil0, k.L[0].halo, glu);
  k.BM = tp.BM;
  k.ntile = tp.ntile;
  if (tp.poly) {
    const int PH = tp.PH, BMJ = R0 / PH;
    k.L[0].nfrag = NW * TM;
    k.img_rows = PH * (BMJ + a.taps - 1);
    const size_t smem = (size_t)k.img_rows * RS + 3 * 64 * sizeof(float);
    switch (PH) {
      case 1: return launch_staged<1, 1, true>(k, up, false, a.precision, smem, flops, s);
      case 2: return launch_staged<1, 2, true>(k, up, false, a.precision, smem, flops, s);
      default: return launch_staged<1, 4, true>(k, up, false, a.precision, smem, flops, s);
    }
  }
  ASW_CHECK_ARG(k.BM >= R0 / 2, "resstack: the later layers' halo (%d rows per side) leaves %d of %d rows; fuse fewer layers",
                k.L[0].halo, k.BM, R0);
  int rows = 0;                                          // of the image of a tile that stands alone
  for (int i = 0; i < a.n_layers; ++i) {
    k.L[i].nfrag = asw::cdiv(k.BM + 2 * k.L[i].halo, 32);
    const int r = 32 * k.L[i].nfrag + 2 * k.L[i].pad;
    rows = r > rows ? r : rows;
  }
  const bool pair = a.n_layers == 2 && !up;              // runs of tiles, the per-layer vectors in the rows' pad bytes
  const bool carry = pair && carry_applies(a.T, k.BM, k.L[0].pad, k.L[0].halo, a.runs_per_item);
  k.img_rows = carry ? R0 + 2 * std::max(k.L[0].pad, k.L[0].halo) : rows;
  const size_t smem = (size_t)k.img_rows * RS + (pair ? 0 : (size_t)a.n_layers * 3 * 64 * sizeof(float));
  ASW_CHECK_ARG(smem <= 160 * 1024, "resstack: image of %d rows exceeds LDS (dilation %d x %d taps too wide for a contiguous tile)",
                k.img_rows, dil0, a.taps);
  if (pair) {
    k.runs = plan_runs(a.T, k.BM, !carry ? INT_MAX : a.runs_per_item > 0 ? a.runs_per_item : auto_runs(a.T, k.BM, a.B, device_cus()));
    if (k.src_h) return launch_stack<2, 1, false, false, true, false>(k, nullptr, a.precision, smem, flops, s, carry);
    return glu ? launch_stack<2, 1, false, true, false, false>(k, nullptr, a.precision, smem, flops, s, carry)
               : launch_stack<2, 1, false, false, false, false>(k, nullptr, a.precision, smem, flops, s, carry);
  }
  switch (a.n_layers) {
    case 1: return launch_staged<1, 1, false>(k, up, glu, a.precision, smem, flops, s);
    case 2: return launch_staged<2, 1, false>(k, up, glu, a.precision, smem, flops, s);
    default: return launch_staged<3, 1, false>(k, up, glu, a.precision, smem, flops, s);
  }
}

}  // namespace

#ifdef ASW_PHASE_TIMING
extern "C" int asw_debug_resstack_cycles(unsigned long long* out6, int reset) {
  ASW_HIP(hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_rs_cycles), 6 * sizeof(unsigned long long)));
  if (reset) {
    const unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
    ASW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_rs_cycles), z, sizeof z));
  }
  return ASW_OK;
}
#endif

extern "C" int asw_compose_source_weights(const float* wc, const float* wpre, const float* bpre, int M, int taps, float* comp,
                                          float* pre16) {
  ASW_CHECK_ARG(wc && wpre && bpre && comp && pre16, "compose_source_weights: null pointer");
  ASW_CHECK_ARG(M >= 1 && M <= 7 && taps >= 1 && taps <= 7, "compose_source_weights: M=%d taps=%d (at most 7 each)", M, taps);
  for (int i = 0; i < C * 16; ++i) pre16[i] = 0.f;
  for (int i = 0; i < C * 64; ++i) comp[i] = 0.f;
  for (int c = 0; c < C; ++c) {
    for (int m = 0; m < M; ++m) pre16[c * 16 + m] = wpre[c * M + m];
    pre16[c * 16 + 7] = bpre[c];                         // the channel that is 1 on every row carries the bias
  }
  for (int n = 0; n < C; ++n)
    for (int k = 0; k < taps; ++k)
      for (int j = 0; j < 8; ++j) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc += (double)wc[((size_t)n * C + c) * taps + k] * (double)pre16[c * 16 + j];
        comp[n * 64 + k * 8 + j] = (float)acc;
      }
  return ASW_OK;
}

extern "C" int asw_resstack_tiles(int T, int taps, int n_layers, const int32_t* dil, int glu) {
  ASW_CHECK_ARG(T > 0 && taps >= 3 && taps % 2 == 1 && n_layers >= 1 && n_layers <= MAXL && dil, "resstack_tiles: bad argument");
  int halo0 = 0;
  for (int i = 1; i < n_layers; ++i) halo0 += dil[i] * (taps - 1) / 2;
  const TilePlan t = plan_tiles(T, n_layers, dil[0], halo0, glu != 0);
  ASW_CHECK_ARG(t.BM >= R0 / 2, "resstack_tiles: the later layers' halo (%d rows per side) is too wide", halo0);
  return t.ntile;
}

extern "C" int asw_resstack_runs(int T, int B, int taps, const int32_t* dil, int runs_per_item, int n_cu, int32_t* head_rows,
                                 int32_t* steady_rows, int32_t* run_start, int32_t* run_tiles, int max_runs) {
  ASW_CHECK_ARG(T > 0 && B > 0 && taps >= 3 && taps % 2 == 1 && dil && n_cu > 0 && max_runs >= 0, "resstack_runs: bad argument");
  const int pad0 = dil[0] * (taps - 1) / 2, halo0 = dil[1] * (taps - 1) / 2, BM = R0 - 2 * halo0;
  if (BM < R0 / 2 || !carry_applies(T, BM, pad0, halo0, runs_per_item)) return 0;
  const RunPlan rp = plan_runs(T, BM, runs_per_item > 0 ? runs_per_item : auto_runs(T, BM, B, n_cu));
  if (head_rows) *head_rows = BM;
  if (steady_rows) *steady_rows = R0;
  for (int r = 0; r < rp.nrun && r < max_runs; ++r) {
    if (run_start) run_start[r] = rp.start(r, BM);
    if (run_tiles) run_tiles[r] = rp.tiles(r);
  }
  return rp.nrun;
}

extern "C" int asw_resstack64_f16x3(const asw_resstack_args* args, void* stream) {
  ASW_CHECK_ARG(args != nullptr, "resstack: null args");
  const asw_resstack_args& a = *args;
  hipStream_t s = asw::as_stream(stream);
  ASW_CHECK_ARG(a.C == C, "resstack: C=%d (64 only)", a.C);
  ASW_CHECK_ARG(a.n_layers >= 1 && a.n_layers <= MAXL, "resstack: 1..%d layers", MAXL);
  ASW_CHECK_ARG(a.taps >= 3 && a.taps <= 15 && a.taps % 2 == 1, "resstack: taps=%d (odd, 3..15)", a.taps);
  ASW_CHECK_ARG(a.precision == 1 || a.precision == 2, "resstack: precision 1 (f16x3) or 2 (single-pass f16)");
  ASW_CHECK_ARG(a.B > 0 && a.B <= (1 << 20) && a.T > 0 && (int64_t)a.T * 2 * C < ((int64_t)1 << 29), "resstack: bad B / T");
  ASW_CHECK_ARG((a.out || a.up_hi) && (a.x || a.glu_raw || a.src_hi), "resstack: null tensor");
  const bool glu = a.glu_raw != nullptr;
  if (glu) ASW_CHECK_ARG(a.glu_mr && a.glu_gamma && a.glu_beta, "resstack: GroupNorm + GLU on load needs the statistics / affine arrays");
  KArgs k = {};
  k.x = a.x; k.out = a.out; k.glu_raw = a.glu_raw; k.glu_mr = a.glu_mr; k.glu_gamma = a.glu_gamma; k.glu_beta = a.glu_beta;
  k.glu_out = glu ? a.glu_out : nullptr;
  k.B = a.B; k.T = a.T; k.taps = a.taps; k.eps = a.ln_eps;
  int halo = 0;
  for (int i = a.n_layers - 1; i >= 0; --i) {
    const asw_reslayer_desc& d = a.layer[i];
    ASW_CHECK_ARG(d.Wf_hi && d.Wf_lo && d.bias && d.ln_gamma && d.ln_beta && d.dil >= 1, "resstack: layer %d incomplete", i);
    LayerDev& L = k.L[i];
    L.Wh = reinterpret_cast<const half8*>(d.Wf_hi); L.Wl = reinterpret_cast<const half8*>(d.Wf_lo);
    L.bias = d.bias; L.gamma = d.ln_gamma; L.beta = d.ln_beta;
    L.dil = d.dil; L.pad = d.dil * (a.taps - 1) / 2; L.halo = halo;
    L.scale = ldexpf(1.0f, -d.w_shift);
    halo += L.pad;
  }
  double flops = 2.0 * a.B * (double)a.T * C * C * a.taps * a.n_layers;
  if (a.src_hi) {
    ASW_CHECK_ARG(a.src_lo && a.pre_hi && a.pre_lo && !a.x && !glu, "resstack: the source-fed form takes src_hi / src_lo / pre_hi / pre_lo and no x");
    ASW_CHECK_ARG(a.precision == 1 && a.n_layers == 2 && a.taps <= 7 && a.layer[0].dil == 1,
                  "resstack: source-fed layer 0 is f16x3, two layers, dilation 1, at most 7 taps");
    k.src_h = reinterpret_cast<const half8*>(a.src_hi); k.src_l = reinterpret_cast<const half8*>(a.src_lo);
    k.Pre_h = reinterpret_cast<const half8*>(a.pre_hi); k.Pre_l = reinterpret_cast<const half8*>(a.pre_lo);
    k.pre_up = ldexpf(1.0f, a.pre_shift); k.pre_down = ldexpf(1.0f, -a.pre_shift);
    // the FLOPs executed: layer 0 is K = 64 (8 taps x 8 channels) plus the K = 16 residual step, layer 1 as always
    flops = 2.0 * a.B * (double)a.T * C * (64 + 16 + C * a.taps);
  }
  UpArgs up = {};
  if (a.up_hi) {
    ASW_CHECK_ARG(a.up_lo && a.up_bias && a.up_skip && a.up_out && a.up_stats, "resstack: UpFeed needs up_lo / up_bias / up_skip / up_out / up_stats");
    ASW_CHECK_ARG(a.precision == 1 && !a.src_hi, "resstack: UpFeed is f16x3 and never source-fed");
    up.Wh = reinterpret_cast<const half8*>(a.up_hi); up.Wl = reinterpret_cast<const half8*>(a.up_lo);
    up.bias = a.up_bias; up.skip = a.up_skip; up.out = a.up_out; up.stats = a.up_stats;
    up.scale = ldexpf(1.0f, -a.up_shift);
  }
  return dispatch(a, k, a.up_hi ? &up : nullptr, glu, flops, s);   // 4 waves x 2 row fragments: 256 rows computed by layer 0
}
