// attention.hip -- self-attention over the time axis of both bottlenecks, ctx = softmax(Q K^T [+ rel-pos term]) V:
// every kernel, its launcher and the C entry points asw_attention, asw_attention_prec and asw_relpos_attention.
//   spot network: nn.MultiheadAttention core inside nn.TransformerEncoderLayer
//     (sep/training/SpeakerLocalization/network.py:254), sequence L = T/256 (188 at T = 48 000, 563 at T = 144 000),
//     head_dim 128, scale 1/sqrt(hd);
//   separation network: speechbrain RelPosMHAXL as published (SpeakerSeparation/network.py:270-321; the library itself
//     is absent, see oracle/sep_ref.py), L = T/64 (750 at T = 48 000), head_dim 64.
// Which kernel runs (asw_attention_prec / asw_relpos_attention at the end of the file decide, nothing else does):
//   head_dim 128, f16x3 / f16, L <= 320   attention_mfma16_kernel       f16x3 MFMA, whole score row in LDS
//   head_dim 128, L <= 320                attention_mfma64_kernel       f32 MFMA, whole score row in LDS
//   head_dim 128, longer                  attention_mfma_flash_kernel   f32 MFMA, key-tiled, two passes
//   any other head_dim <= 128, or a sequence of 2^31 bytes and more     attention_valu_kernel<0, 128, false>
//   rel-pos, head_dim 64                  relpos_attention_mfma_kernel  f32 MFMA, online softmax, rel-pos skew
//   rel-pos, head_dim 16 / 32             attention_valu_kernel<HD, 64, true>
// The MFMA kernels run one workgroup (4 waves) per (batch item, head, 64-query tile) on 64-key tiles; the f32 ones are
// exact fp32 arithmetic (v_mfma_f32_32x32x2_f32 is an fmaf chain) and are put together from the tile steps below.
// The inter-speaker attention attends over speakers, not time, shares nothing with these and lives in sep_kernels.hip.
#include <cstdlib>

#include "asw_common.h"
#include "mfma_util.h"

namespace {

using asw::cdiv;
using asw::ProfScope;
using asw::SmemAttr;
using asw_mfma::acc_row;
using asw_mfma::floatx16;
using asw_mfma::mma_row;

// ---------------------------------------------------------------------------------------
// VALU kernel: per (batch item, head, 16-query tile) a flash-style sweep over KT-key tiles held in LDS with an online
// softmax, exact fp32 arithmetic, written for exactness and bounded LDS rather than MFMA rate.
// thread = (query q = tid/16, sub-lane sl = tid%16): scores for keys sl + 16 jj, output dims sl + 16 i.
//   HD   head_dim at compile time, or 0: any multiple of 16 up to 128, passed in `hd_rt`
//   KT   keys per tile
//   REL  the relative-position term of RelPosMHAXL:
//          score[i][j] = scale * ( (q_i + u_h) . k_j  +  (q_i + v_h) . P_h[(L-1) + j - i] ),   P = linear_pos(sinusoid table),
//        P [2L-1][d], bu / bv [d] (flat, head-major as pos_bias_*.view(1,1,H,hd) reads them); the P rows a tile needs
//        are the KT + 15 consecutive rows (L-1) + k0 - q0 - 15 ...  Without REL, P / bu / bv are not read.
// qkv [B][L][3d] in the standard layout (Q | K | V, head h at columns h*hd; the rel-pos caller permutes speechbrain's
// per-head (q,k,v) interleave when packing in_proj_weight).
// ---------------------------------------------------------------------------------------
constexpr int VA_BQ = 16;

template <int HD, int KT, bool REL>
__global__ __launch_bounds__(256) void attention_valu_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                             const float* __restrict__ bu, const float* __restrict__ bv,
                                                             int L, int d, int hd_rt, float scale, float* __restrict__ ctx) {
  constexpr int MAXD = HD ? HD / 16 : 8, PR = KT + VA_BQ - 1;
  const int hd = HD ? HD : hd_rt;
  const int ldk = hd + 1, ldq = REL ? hd : ldk;
  const int nd = hd >> 4;                 // output dims per thread
  extern __shared__ __align__(16) float smem[];
  float* Qs = smem;                       // [BQ][ldq]   q * scale; REL: (q + u) * scale
  float* Qv = Qs + VA_BQ * ldq;           // [BQ][ldq]   REL: (q + v) * scale
  float* Ks = REL ? Qv + VA_BQ * ldq : Qv;   // [KT][hd+1]
  float* Vs = Ks + KT * ldk;              // [KT][hd]
  float* Pw = Vs + KT * hd;               // [PR][hd+1]  REL: window of P rows for this (query tile, key tile)
  float* Ps = REL ? Pw + PR * ldk : Pw;   // [BQ][KT] probabilities
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * VA_BQ;
  const int tid = threadIdx.x, q = tid >> 4, sl = tid & 15;
  const float* base = qkv + (long)b * L * 3 * d;

  for (int i = tid; i < VA_BQ * hd; i += 256) {
    const int r = i / hd, c = i - r * hd;
    const float qq = (q0 + r < L) ? base[(long)(q0 + r) * 3 * d + h * hd + c] : 0.f;
    if constexpr (REL) {
      Qs[r * ldq + c] = (qq + bu[h * hd + c]) * scale;
      Qv[r * ldq + c] = (qq + bv[h * hd + c]) * scale;
    } else {
      Qs[r * ldq + c] = qq * scale;
    }
  }
  float acc[MAXD];
#pragma unroll
  for (int i = 0; i < MAXD; ++i) acc[i] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < L; k0 += KT) {
    const int kn = L - k0 < KT ? L - k0 : KT;
    __syncthreads();                      // previous tile fully consumed (also covers Qs / Qv)
    for (int i = tid; i < KT * hd; i += 256) {
      const int r = i / hd, c = i - r * hd;
      float kv = 0.f, vv = 0.f;
      if (r < kn) {
        const float* row = base + (long)(k0 + r) * 3 * d + h * hd + c;
        kv = row[d];
        vv = row[2 * d];
      }
      Ks[r * ldk + c] = kv;
      Vs[r * hd + c] = vv;
    }
    if constexpr (REL) {
      const int pbase = (L - 1) + k0 - q0 - (VA_BQ - 1);
      for (int i = tid; i < PR * hd; i += 256) {
        const int r = i / hd, c = i - r * hd;
        const int m = pbase + r;
        Pw[r * ldk + c] = (m >= 0 && m <= 2 * L - 2) ? P[(long)m * d + h * hd + c] : 0.f;
      }
    }
    __syncthreads();
    // scores for this thread's keys: one fmaf chain over c ascending
    float sc[KT / 16];
    float tmax = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < KT / 16; ++jj) {
      const int j = sl + 16 * jj;
      const float* qr = Qs + q * ldq;
      const float* kr = Ks + j * ldk;
      float s = 0.f;
      if constexpr (REL) {
        const float* qv = Qv + q * ldq;
        const float* pr = Pw + (j - q + VA_BQ - 1) * ldk;
#pragma unroll 8
        for (int c = 0; c < hd; ++c) s = fmaf(qr[c], kr[c], fmaf(qv[c], pr[c], s));
      } else {
        for (int c = 0; c < hd; ++c) s = fmaf(qr[c], kr[c], s);
      }
      sc[jj] = (j < kn) ? s : -INFINITY;
      tmax = fmaxf(tmax, sc[jj]);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o, 64));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int jj = 0; jj < KT / 16; ++jj) {
      const float pv = (sc[jj] == -INFINITY) ? 0.f : expf(sc[jj] - m_new);
      Ps[q * KT + sl + 16 * jj] = pv;
      psum += pv;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) psum += __shfl_xor(psum, o, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXD; ++i) acc[i] *= alpha;
    for (int j = 0; j < kn; ++j) {
      const float pv = Ps[q * KT + j];
#pragma unroll
      for (int i = 0; i < MAXD; ++i)
        if (i < nd) acc[i] = fmaf(pv, Vs[j * hd + sl + 16 * i], acc[i]);
    }
  }
  if (q0 + q < L) {
    const float inv = 1.0f / l_run;
    float* o = ctx + ((long)b * L + q0 + q) * d + h * hd;
#pragma unroll
    for (int i = 0; i < MAXD; ++i)
      if (i < nd) o[sl + 16 * i] = acc[i] * inv;
  }
}

// ---------------------------------------------------------------------------------------
// Tile steps of the f32 MFMA kernels.  A workgroup is 4 waves; lane = (lr = lane & 31, lh = lane >> 5); in the score
// products wave w owns the 32 x 32 tile (query half qi = w >> 1, key half kj = w & 1); register r of a 32 x 32
// accumulator is row acc_row(r, lh), column lr.
// ---------------------------------------------------------------------------------------
constexpr int BQ = 64;            // queries per workgroup
constexpr int BK = 64;            // keys per staged tile

// asw_mfma::act_load4 without its `elem >= 0` test (no offset here is negative).  Kept apart from it: with the test the
// three kernels below take more registers (attention_mfma16_kernel 208 -> 220 VGPRs, 4 to 8 SGPRs in the other two).
__device__ __forceinline__ float4 row_load4(__amdgpu_buffer_rsrc_t r, long elem, bool ok) {
  // rows past the sequence end read as zeros through the descriptor's range check (no branch)
  const asw_mfma::intx4 v = __builtin_amdgcn_raw_buffer_load_b128(r, ok ? (int)(elem * 4) : (int)0x80000000, 0, 0);
  const asw_mfma::floatx4v f = __builtin_bit_cast(asw_mfma::floatx4v, v);
  return make_float4(f[0], f[1], f[2], f[3]);
}

// dst[ROWS][HD + 4] = mul * rows row0 .. of the sequence behind descriptor rs (row stride 3d floats), HD columns from
// `col`; rows from L on read as zeros
template <int ROWS, int HD>
__device__ __forceinline__ void stage_tile(float* dst, __amdgpu_buffer_rsrc_t rs, int row0, int L, int d, int col, int tid,
                                           float mul = 1.0f) {
  for (int i = tid; i < ROWS * (HD / 4); i += 256) {
    const int r = i / (HD / 4), c4 = i - r * (HD / 4);
    float4 v = row_load4(rs, (long)(row0 + r) * 3 * d + col + c4 * 4, row0 + r < L);
    v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
    *reinterpret_cast<float4*>(dst + r * (HD + 4) + c4 * 4) = v;
  }
}

// one wave's 32 x 32 tile of S = Q K^T to dst[acc_row][0], row stride ldd: qa / kb as mma_row takes them, dst = (first query
// row, this lane's key) of the tile; a key that is not `valid` gets -inf
template <int HD>
__device__ __forceinline__ void score_tile(const float* qa, const float* kb, float* dst, int ldd, int lh, bool valid = true) {
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  acc = mma_row<HD / 8>(qa, kb, acc);
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[acc_row(r, lh) * ldd] = valid ? acc[r] : -INFINITY;
}

// maximum / sum over the 4 lanes that share a query row (tid >> 2)
__device__ __forceinline__ float quad_max(float m) {
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  return fmaxf(m, __shfl_xor(m, 2, 64));
}
__device__ __forceinline__ float quad_sum(float s) {
  s += __shfl_xor(s, 1, 64);
  return s + __shfl_xor(s, 2, 64);
}

// One online-softmax step of query row `row` over the BK scores pr[] of a key tile (4 lanes per row, this one is `sub`):
// rm / rl [BQ] are the running maximum and sum.  WRITE: pr[] becomes exp(s - m_new) and ra[row] the factor that rescales
// what was accumulated before.  exp(-inf) = 0 for padded keys, and for the factor of the first step (m_old = -inf).
template <bool WRITE>
__device__ __forceinline__ void online_softmax_row(float* pr, int row, int sub, float* rm, float* rl, float* ra) {
  float m = -INFINITY;
  for (int j = sub; j < BK; j += 4) m = fmaxf(m, pr[j]);
  m = quad_max(m);
  const float m_old = rm[row], m_new = fmaxf(m_old, m);
  float sum = 0.f;
  for (int j = sub; j < BK; j += 4) {
    const float e = expf(pr[j] - m_new);
    if constexpr (WRITE) pr[j] = e;
    sum += e;
  }
  sum = quad_sum(sum);
  if (sub == 0) {
    const float alpha = expf(m_old - m_new);
    if constexpr (WRITE) ra[row] = alpha;
    rl[row] = rl[row] * alpha + sum;
    rm[row] = m_new;
  }
}

// o[t] += P_t V over one BK-key tile on v_mfma_f32_32x32x2_f32, NQ query tiles against one 32-column block of V:
// pa = probability row of this lane's query in tile 0, + 4 * lh (tile t is t * pq floats on); vb = V[key 4 * lh][this
// lane's column] of the row-major tile, row stride ldv: the B operand is four ds_read_b32 per four MFMAs (no transposition)
template <int NQ>
__device__ __forceinline__ void pv_f32(const float* pa, int pq, const float* vb, int ldv, floatx16 (&o)[NQ]) {
#pragma unroll 4
  for (int kk = 0; kk < BK / 8; ++kk) {
    float a[NQ][4];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      const float4 v = *reinterpret_cast<const float4*>(pa + t * pq + kk * 8);
      a[t][0] = v.x; a[t][1] = v.y; a[t][2] = v.z; a[t][3] = v.w;
    }
    const float bb[4] = {vb[(kk * 8 + 0) * ldv], vb[(kk * 8 + 1) * ldv], vb[(kk * 8 + 2) * ldv], vb[(kk * 8 + 3) * ldv]};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < NQ; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][i], bb[i], o[t], 0, 0, 0);
  }
}

// NQ 32 x 32 accumulators (query tiles 32 rows apart) to rows q0 + 32 t + acc_row, those below L, of the sequence that
// starts at row bL of ctx [..][d], this lane's column `col`; times mul, or divided by rdiv[32 t + acc_row] where given
template <int NQ>
__device__ __forceinline__ void ctx_store(float* ctx, long bL, int col, int d, int q0, int L, int lh, const floatx16 (&o)[NQ],
                                          float mul = 1.0f, const float* rdiv = nullptr) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      const int row = 32 * t + acc_row(r, lh), q = q0 + row;
      if (q < L) ctx[(bL + q) * d + col] = rdiv ? o[t][r] / rdiv[row] : o[t][r] * mul;
    }
  }
}

constexpr int AD = 128;           // head_dim of the spot network's kernels
constexpr int LDQ = AD + 4;       // Q / K / V row stride (floats)

// ---- short sequences (L <= 320: T = 48 000 gives L = 188): whole score row in LDS ----------
// The 64 x LP score rows of the workgroup's queries stay in LDS beside Q and one K / V tile: exact softmax, one Q K^T.
__global__ __launch_bounds__(256) void attention_mfma64_kernel(const float* __restrict__ qkv, int L, int LP, int d,
                                                               float* __restrict__ ctx) {
  extern __shared__ __align__(16) float smem[];
  const int LDP = LP + 4;
  float* Qs = smem;                          // [BQ][LDQ]
  float* KV = Qs + BQ * LDQ;                 // K tile [BK][LDQ], then V tile [BK][LDQ] (row-major)
  float* Ps = KV + BK * LDQ;                 // [BQ][LDP]
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * BQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qkv + (long)b * L * 3 * d), 0, L * 3 * d * 4, 0x00020000);

  stage_tile<BQ, AD>(Qs, rs, q0, L, d, h * AD, tid, 1.0f / sqrtf((float)AD));
  // ---- phase 1: S = (Q/sqrt(hd)) K^T; wave w owns score tile (query tile w>>1, key tile w&1)
  const int qi = wid >> 1, kj = wid & 1;
  for (int k0 = 0; k0 < LP; k0 += BK) {
    __syncthreads();
    stage_tile<BK, AD>(KV, rs, k0, L, d, d + h * AD, tid);
    __syncthreads();
    score_tile<AD>(Qs + (qi * 32 + lr) * LDQ + lh * 4, KV + (kj * 32 + lr) * LDQ + lh * 4, Ps + qi * 32 * LDP + k0 + kj * 32 + lr,
                   LDP, lh);
  }
  __syncthreads();
  // ---- row softmax over the L valid keys: 4 lanes per query row, padded keys -> 0
  {
    const int row = tid >> 2, sub = tid & 3;
    float* pr = Ps + row * LDP;
    float m = -INFINITY;
    for (int j = sub; j < L; j += 4) m = fmaxf(m, pr[j]);
    m = quad_max(m);
    float s = 0.f;
    for (int j = sub; j < LP; j += 4) {
      const float e = j < L ? expf(pr[j] - m) : 0.f;
      pr[j] = e;
      s += e;
    }
    s = quad_sum(s);
    const float inv = 1.0f / s;
    for (int j = sub; j < LP; j += 4) pr[j] *= inv;
  }
  // ---- phase 2: O = P V; wave w owns output columns [32w, 32w+32) of both query tiles
  floatx16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  for (int k0 = 0; k0 < LP; k0 += BK) {
    __syncthreads();                                   // softmax done / previous V tile consumed
    // not stage_tile: written out, the compiler opens this loop up (8 loads per thread, each waited for) and keeps the
    // other staging loops closed, and the kernel's time follows that: through stage_tile it is 1 % slower
    for (int i = tid; i < BK * (AD / 4); i += 256) {
      const int r = i / (AD / 4), c4 = i - r * (AD / 4);
      *reinterpret_cast<float4*>(KV + r * LDQ + c4 * 4) =
          row_load4(rs, (long)(k0 + r) * 3 * d + 2 * d + h * AD + c4 * 4, k0 + r < L);
    }
    __syncthreads();
    pv_f32<2>(Ps + lr * LDP + k0 + lh * 4, 32 * LDP, KV + (lh * 4) * LDQ + wid * 32 + lr, LDQ, o);
  }
  ctx_store(ctx, (long)b * L, h * AD + wid * 32 + lr, d, q0, L, lh, o);
}


// ---- short sequences on the f16 matrix pipe (f16x3 split operands) --------------------------
// Same structure as attention_mfma64_kernel (64 queries per workgroup, exact fp32 softmax over a score
// row that stays in LDS), with both products on v_mfma_f32_32x32x16_f16: every fp32 operand x is
// hi = fp16(x) + lo = fp16(x - hi) and a product is lo*hi + hi*lo + hi*hi with fp32 accumulation
// (operands good to 2^-21; the f32 MFMA runs at 1/16 of this pipe's rate, i.e. 3/16 of it per product).
//   * Q and the K tile are staged as fp16 hi / lo images, row = 128 hi + 128 lo halves + 16 B pad
//     (528 B: the 16-byte fragment reads of 32 consecutive rows are bank-conflict free);
//   * S = (Q / sqrt(hd)) K^T goes to LDS in fp32, the softmax runs there as before, and each row is
//     then REPLACED by its probabilities as fp16 hi | lo (same bytes: 2 + 2 per element), read back as
//     the A operand of O = P V;
//   * V stays row-major [key][hd] (coalesced staging): the B operand of O = P V needs, per hd column,
//     8 consecutive KEYS, which ds_read_b64_tr_b16 delivers from the row-major image (per 16-lane
//     group a 4-row x 16-column block, column-major); V rows are 256 B of hi (or lo) + 64 B pad
//     = 320 B, which keeps those reads conflict-free (bank of row q, 8-byte chunk p: 16 q + 2 p + 8 g).
// This is the kernel the benchmark runs and it is register-bound (208 + 32 VGPRs): of the tile steps above it takes
// acc_row, the 4-lane reductions and the context store, which inline to the code it had.
typedef _Float16 ahalf8 __attribute__((ext_vector_type(8)));
typedef _Float16 ahalf4 __attribute__((ext_vector_type(4)));
typedef __fp16 afp16x2 __attribute__((ext_vector_type(2)));
typedef __fp16 afp16x4 __attribute__((ext_vector_type(4)));

constexpr int QRS = 528;          // bytes per Q / K image row (hi 256 | lo 256 | pad 16)
constexpr int VRS = 320;          // bytes per V image row (256 + 64 pad); hi image, then lo image

// hi by packed round-toward-zero conversion, lo = the remainder ROUNDED TO NEAREST (|x - hi - lo| <= 2^-23 |x|, no
// one-sided bias): the softmax exponentiates the score error, so the attention products keep the extra bit that
// the truncating split of the convolution kernels (convgemm.hip split4) gives up
__device__ __forceinline__ void split4h(const float4 x, ahalf4& hi, ahalf4& lo) {
  const afp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(x.x, x.y), h23 = __builtin_amdgcn_cvt_pkrtz(x.z, x.w);
  union { afp16x2 v[2]; ahalf4 h; } uh;
  uh.v[0] = h01; uh.v[1] = h23;
  hi = uh.h;
  lo = ahalf4{(_Float16)(x.x - (float)h01[0]), (_Float16)(x.y - (float)h01[1]), (_Float16)(x.z - (float)h23[0]),
              (_Float16)(x.w - (float)h23[1])};
}

// transposed fragment: 8 consecutive k (rows of the row-major image) of this lane's column
__device__ __forceinline__ ahalf8 tr_frag(const char* blk_lo4, const char* blk_hi4) {
  typedef __attribute__((address_space(3))) afp16x4 lds_h4;
  const afp16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(blk_lo4));
  const afp16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(blk_hi4));
  union { afp16x4 v[2]; ahalf8 h; } u;
  u.v[0] = a; u.v[1] = b;
  return u.h;
}

__global__ __launch_bounds__(256) void attention_mfma16_kernel(const float* __restrict__ qkv, int L, int LP, int d,
                                                               float* __restrict__ ctx, int pf) {
  extern __shared__ __align__(16) float smem[];
  const int RSP = LP * 4 + 16;               // bytes per score / probability row
  char* Qi = reinterpret_cast<char*>(smem);  // [BQ] x QRS
  char* KV = Qi + BQ * QRS;                  // K tile [BK] x QRS, then V tile: hi [BK] x VRS | lo [BK] x VRS
  char* Pb = KV + 2 * BK * VRS;              // [BQ] x RSP: fp32 scores, then fp16 hi | lo probabilities
  static_assert(2 * BK * VRS >= BK * QRS, "the V images cover the K tile");
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * BQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const float scale = 1.0f / sqrtf((float)AD);
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qkv + (long)b * L * 3 * d), 0, L * 3 * d * 4, 0x00020000);
  // Tiles of 64 rows x 128 floats travel global -> registers -> (split) -> LDS; the loads of the NEXT tile are issued
  // before the MFMAs of the current one (8 float4 per thread in flight), so with one workgroup per CU the memory
  // latency of a tile hides behind the products of the previous one (and the first V tile behind the softmax).
  constexpr int TV = BK * (AD / 4) / 256;               // float4 per thread and tile
  auto issue = [&](float4 (&r)[TV], int row0, int which) {
#pragma unroll
    for (int u = 0; u < TV; ++u) {
      const int i = tid + u * 256;
      const int rr = i / (AD / 4), c4 = i - rr * (AD / 4);
      r[u] = row_load4(rs, (long)(row0 + rr) * 3 * d + which * d + h * AD + c4 * 4, row0 + rr < L);
    }
  };
  auto deposit = [&](const float4 (&r)[TV], char* hi_img, char* lo_img, int rstride, float mul) {
#pragma unroll
    for (int u = 0; u < TV; ++u) {
      const int i = tid + u * 256;
      const int rr = i / (AD / 4), c4 = i - rr * (AD / 4);
      float4 v = r[u];
      v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
      ahalf4 hi, lo;
      split4h(v, hi, lo);
      *reinterpret_cast<ahalf4*>(hi_img + rr * rstride + c4 * 8) = hi;
      *reinterpret_cast<ahalf4*>(lo_img + rr * rstride + c4 * 8) = lo;
    }
  };
  float4 stg[TV];
  issue(stg, q0, 0);
  deposit(stg, Qi, Qi + 256, QRS, scale);
  // pf: bit 0 = K tiles, bit 1 = V tiles requested one tile ahead (3 in production; the launcher's ASW_ATTN_PF
  // selects other combinations for measurements).  The flags are RUNTIME values on purpose: with the two prefetches
  // as straight-line code hipcc (ROCm 7.2) produced a kernel that returned wrong values for every shape, while each
  // of the four flag combinations of this form is correct (test_attention covers pf = 3, the production value).
  if (pf & 1) issue(stg, 0, 1);
  // ---- phase 1: S = (Q/sqrt(hd)) K^T; wave w owns score tile (query tile w>>1, key tile w&1)
  const int qi = wid >> 1, kj = wid & 1;
  for (int k0 = 0; k0 < LP; k0 += BK) {
    __syncthreads();                                   // previous K tile consumed
    if (!(pf & 1)) issue(stg, k0, 1);
    deposit(stg, KV, KV + 256, QRS, 1.0f);
    __syncthreads();
    if (k0 + BK < LP) { if (pf & 1) issue(stg, k0 + BK, 1); }      // next K tile
    else if (pf & 2) issue(stg, 0, 2);                 // first V tile: in flight under the softmax
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const char* qa = Qi + (qi * 32 + lr) * QRS + lh * 16;
    const char* kb = KV + (kj * 32 + lr) * QRS + lh * 16;
#pragma unroll
    for (int ks = 0; ks < AD / 16; ++ks) {
      const ahalf8 qh = *reinterpret_cast<const ahalf8*>(qa + ks * 32), ql = *reinterpret_cast<const ahalf8*>(qa + 256 + ks * 32);
      const ahalf8 kh = *reinterpret_cast<const ahalf8*>(kb + ks * 32), kl = *reinterpret_cast<const ahalf8*>(kb + 256 + ks * 32);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql, kh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh, kl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh, kh, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = qi * 32 + acc_row(r, lh);
      *reinterpret_cast<float*>(Pb + (size_t)row * RSP + (k0 + kj * 32 + lr) * 4) = acc[r];
    }
  }
  __syncthreads();
  // ---- row softmax over the L valid keys (fp32, 4 lanes per query row), then the row is rewritten in place as
  //      fp16 hi | lo probabilities: every lane first pulls its share of the row into registers
  {
    const int row = tid >> 2, sub = tid & 3;
    char* pr = Pb + (size_t)row * RSP;
    constexpr int MAXV = 352 / 16;                       // float4 groups per lane (LP <= 352)
    float4 v[MAXV];
    const int nv = LP / 16;                               // LP is a multiple of 64
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (i < nv) {
        v[i] = *reinterpret_cast<const float4*>(pr + (i * 4 + sub) * 16);
        const int j = (i * 4 + sub) * 4;
        if (j + 0 < L) m = fmaxf(m, v[i].x);
        if (j + 1 < L) m = fmaxf(m, v[i].y);
        if (j + 2 < L) m = fmaxf(m, v[i].z);
        if (j + 3 < L) m = fmaxf(m, v[i].w);
      }
    }
    m = quad_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (i < nv) {
        const int j = (i * 4 + sub) * 4;
        v[i].x = j + 0 < L ? expf(v[i].x - m) : 0.f;
        v[i].y = j + 1 < L ? expf(v[i].y - m) : 0.f;
        v[i].z = j + 2 < L ? expf(v[i].z - m) : 0.f;
        v[i].w = j + 3 < L ? expf(v[i].w - m) : 0.f;
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      }
    }
    s = quad_sum(s);
    // probabilities are stored times 2^12 (undone in the output): the lo half of a small probability would otherwise
    // fall into the fp16 subnormals (p = 1/300 has lo ~ 1e-6) and lose the bits it is there to carry
    const float inv = 4096.0f / s;
    // the four lanes of a row have read all of it (same wave: the shuffles above order the reads before these writes)
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (i < nv) {
        const float4 pv = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
        ahalf4 hi, lo;
        split4h(pv, hi, lo);
        const int j = (i * 4 + sub) * 4;
        *reinterpret_cast<ahalf4*>(pr + j * 2) = hi;
        *reinterpret_cast<ahalf4*>(pr + LP * 2 + j * 2) = lo;
      }
    }
  }
  // ---- phase 2: O = P V; wave w owns output columns [32w, 32w+32) of both query tiles
  floatx16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  char* Vh = KV;
  char* Vl = KV + BK * VRS;
  // transposed reads: 16-lane group g = lane >> 4 covers columns 16 (g & 1) .. +15 of this wave's 32, k half (g >> 1);
  // lane 4q + p of a group addresses row q, 8-byte chunk p of the 4-row x 16-column block
  const int g = lane >> 4, gq = (lane & 15) >> 2, gp = lane & 3;
  const int tr_off = (8 * (g >> 1) + gq) * VRS + (wid * 32 + 16 * (g & 1) + 4 * gp) * 2;
  for (int k0 = 0; k0 < LP; k0 += BK) {
    __syncthreads();                                   // probabilities written / previous V tile consumed
    if (!(pf & 2)) issue(stg, k0, 2);
    deposit(stg, Vh, Vl, VRS, 1.0f);
    __syncthreads();
    // The two image bases go through an opaque asm placed after the barrier: the transposed reads cannot be scheduled
    // before it, and every read keeps a small immediate offset from its own base register.
    const char* vh_base = Vh + tr_off;
    const char* vl_base = Vl + tr_off;
    asm volatile("" : "+v"(vh_base), "+v"(vl_base));
    if ((pf & 2) && k0 + BK < LP) issue(stg, k0 + BK, 2);          // next V tile
    const char* p0 = Pb + (size_t)lr * RSP + (k0 + lh * 8) * 2;
    const char* p1 = p0 + (size_t)32 * RSP;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const ahalf8 a0h = *reinterpret_cast<const ahalf8*>(p0 + ks * 32), a0l = *reinterpret_cast<const ahalf8*>(p0 + LP * 2 + ks * 32);
      const ahalf8 a1h = *reinterpret_cast<const ahalf8*>(p1 + ks * 32), a1l = *reinterpret_cast<const ahalf8*>(p1 + LP * 2 + ks * 32);
      const int ro = ks * 16 * VRS;                    // rows 16 ks + 8 (g >> 1) + {0..3}, then + 4
      const ahalf8 vh = tr_frag(vh_base + ro, vh_base + ro + 4 * VRS);
      const ahalf8 vl = tr_frag(vl_base + ro, vl_base + ro + 4 * VRS);
      o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, vh, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, vh, o[1], 0, 0, 0);
      o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, vl, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, vl, o[1], 0, 0, 0);
      o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, vh, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, vh, o[1], 0, 0, 0);
    }
  }
  ctx_store(ctx, (long)b * L, h * AD + wid * 32 + lr, d, q0, L, lh, o, 1.0f / 4096.0f);
}

// ---- long sequences (L > 320: T = 144 000 gives L = 563): key-tiled, two passes ------------
// The score row of 64 queries no longer fits LDS beside Q, K and V, so the row statistics are
// taken first and the scores recomputed: pass A walks the key tiles keeping each query's
// running maximum m and sum l = sum exp(s - m) (rescaled when m grows); pass B recomputes the
// same score tiles, turns them into probabilities exp(s - m) / l and accumulates O = P V.
// Costs one extra Q K^T (a third more MFMAs) but stages K and V row-major with float4 stores,
// keeps all four waves busy and reuses every K / V tile for 64 queries instead of 32.
__global__ __launch_bounds__(256) void attention_mfma_flash_kernel(const float* __restrict__ qkv, int L, int d,
                                                                   float* __restrict__ ctx) {
  extern __shared__ __align__(16) float smem[];
  constexpr int LDS_P = BK + 4;
  float* Qs = smem;                          // [BQ][LDQ]
  float* KV = Qs + BQ * LDQ;                 // K tile / V tile [BK][LDQ]
  float* Pt = KV + BK * LDQ;                 // score / probability tile [BQ][BK + 4]
  float* rm = Pt + BQ * LDS_P;               // [BQ] running max
  float* rl = rm + BQ;                       // [BQ] running sum
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * BQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int LPk = (L + BK - 1) / BK * BK;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qkv + (long)b * L * 3 * d), 0, L * 3 * d * 4, 0x00020000);
  stage_tile<BQ, AD>(Qs, rs, q0, L, d, h * AD, tid, 1.0f / sqrtf((float)AD));
  if (tid < BQ) { rm[tid] = -INFINITY; rl[tid] = 0.f; }
  const int qi = wid >> 1, kj = wid & 1;
  const int row = tid >> 2, sub = tid & 3;   // softmax: 4 lanes per query row
  float* pr = Pt + row * LDS_P;
  auto scores = [&](int k0) {                // Pt = (Q/sqrt(hd)) K^T for this key tile; padded keys -> -inf; ends on a barrier
    __syncthreads();
    stage_tile<BK, AD>(KV, rs, k0, L, d, d + h * AD, tid);
    __syncthreads();
    score_tile<AD>(Qs + (qi * 32 + lr) * LDQ + lh * 4, KV + (kj * 32 + lr) * LDQ + lh * 4, Pt + qi * 32 * LDS_P + kj * 32 + lr, LDS_P, lh,
                   k0 + kj * 32 + lr < L);
    __syncthreads();
  };
  // ---- pass A: running max / sum per query row
  for (int k0 = 0; k0 < LPk; k0 += BK) {
    scores(k0);
    online_softmax_row<false>(pr, row, sub, rm, rl, nullptr);
  }
  // ---- pass B: probabilities and O = P V; wave w owns output columns [32w, 32w+32)
  floatx16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
  for (int k0 = 0; k0 < LPk; k0 += BK) {
    scores(k0);
    {
      const float m = rm[row], inv = 1.0f / rl[row];
      for (int j = sub; j < BK; j += 4) pr[j] = expf(pr[j] - m) * inv;
    }
    stage_tile<BK, AD>(KV, rs, k0, L, d, 2 * d + h * AD, tid);   // the K tile is consumed (barrier at the end of scores)
    __syncthreads();
    pv_f32<2>(Pt + lr * LDS_P + lh * 4, 32 * LDS_P, KV + (lh * 4) * LDQ + wid * 32 + lr, LDQ, o);
  }
  ctx_store(ctx, (long)b * L, h * AD + wid * 32 + lr, d, q0, L, lh, o);
}

// ---------------------------------------------------------------------------------------
// Relative-position attention on the f32 matrix cores (head_dim 64, the full separation network's shape): online
// softmax over 64-key tiles.
//   AC  = (Q+u) K^T            4 MFMA tiles (2 query x 2 key halves), one per wave
//   BD: the relative-position term needs, for query i and key j of the tile, row (L-1)+j-i of P --
//       127 consecutive rows per (query tile, key tile).  Wave (qi, kj) multiplies its 32 queries
//       with the 64 P rows its block can touch (2 MFMA tiles), parks the 32 x 64 product in LDS
//       and reads it back skewed: bd[i][j] = G[i][(j - i) + 31].
//   O   = O * alpha + P V      wave (qi, dj) owns a 32 x 32 block of the 64 x 64 output tile.
// K, V and the P window are staged with guarded pointer loads, not stage_tile: this entry point has no 2^31-byte
// refusal for a descriptor to rest on.  The K and the V loop stay two loops: as one lambda called twice the kernel was
// 2 % slower.
// ---------------------------------------------------------------------------------------
constexpr int RM_HD = 64, RM_LD = RM_HD + 4;     // row stride 68 floats: conflict-free b128 reads

__global__ __launch_bounds__(256) void relpos_attention_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                                    const float* __restrict__ bu, const float* __restrict__ bv,
                                                                    int L, int d, float scale, float* __restrict__ ctx) {
  extern __shared__ __align__(16) float smem[];
  float* Qu = smem;                          // [64][68]
  float* Qv = Qu + BQ * RM_LD;               // [64][68]
  float* KV = Qv + BQ * RM_LD;               // [64][68] K tile, then V tile
  float* Pw = KV + BK * RM_LD;               // [128][68] window of P rows; later 4 x [32][68] skew buffers
  float* Sc = Pw + 2 * BK * RM_LD;           // [64][68] scores, then probabilities
  float* rm = Sc + BQ * RM_LD;               // [64] running max
  float* rl = rm + BQ;                       // [64] running sum
  float* ra = rl + BQ;                       // [64] rescale factor of this step
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * BQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int qi = wid >> 1, kj = wid & 1;
  const float* base = qkv + (long)b * L * 3 * d;

  for (int i = tid; i < BQ * (RM_HD / 4); i += 256) {
    const int r = i / (RM_HD / 4), c4 = (i - r * (RM_HD / 4)) * 4;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + r < L) q = *reinterpret_cast<const float4*>(base + (long)(q0 + r) * 3 * d + h * RM_HD + c4);
    const float4 u = *reinterpret_cast<const float4*>(bu + h * RM_HD + c4);
    const float4 v = *reinterpret_cast<const float4*>(bv + h * RM_HD + c4);
    *reinterpret_cast<float4*>(Qu + r * RM_LD + c4) = make_float4((q.x + u.x) * scale, (q.y + u.y) * scale, (q.z + u.z) * scale, (q.w + u.w) * scale);
    *reinterpret_cast<float4*>(Qv + r * RM_LD + c4) = make_float4((q.x + v.x) * scale, (q.y + v.y) * scale, (q.z + v.z) * scale, (q.w + v.w) * scale);
  }
  if (tid < BQ) { rm[tid] = -INFINITY; rl[tid] = 0.f; }
  floatx16 o[1];
#pragma unroll
  for (int r = 0; r < 16; ++r) o[0][r] = 0.f;
  float* G = Pw + wid * 32 * RM_LD;          // this wave's skew buffer (aliases the P window once it is consumed)
  const int rt0 = kj - qi + 1;               // first of the two 32-row blocks of the P window this wave needs

  for (int k0 = 0; k0 < L; k0 += BK) {
    __syncthreads();                         // previous step fully consumed (also covers Qu / Qv / rm / rl)
    for (int i = tid; i < BK * (RM_HD / 4); i += 256) {
      const int r = i / (RM_HD / 4), c4 = (i - r * (RM_HD / 4)) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k0 + r < L) kv = *reinterpret_cast<const float4*>(base + (long)(k0 + r) * 3 * d + d + h * RM_HD + c4);
      *reinterpret_cast<float4*>(KV + r * RM_LD + c4) = kv;
    }
    const int pbase = (L - 1) + k0 - q0 - (BQ - 1);
    for (int i = tid; i < 2 * BK * (RM_HD / 4); i += 256) {
      const int r = i / (RM_HD / 4), c4 = (i - r * (RM_HD / 4)) * 4;
      const int m = pbase + r;
      float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m >= 0 && m <= 2 * L - 2) pv = *reinterpret_cast<const float4*>(P + (long)m * d + h * RM_HD + c4);
      *reinterpret_cast<float4*>(Pw + r * RM_LD + c4) = pv;
    }
    __syncthreads();
    floatx16 ac, g0, g1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { ac[r] = 0.f; g0[r] = 0.f; g1[r] = 0.f; }
    const float* qa = Qu + (qi * 32 + lr) * RM_LD + lh * 4;
    const float* qb = Qv + (qi * 32 + lr) * RM_LD + lh * 4;
    ac = mma_row<RM_HD / 8>(qa, KV + (kj * 32 + lr) * RM_LD + lh * 4, ac);
    g0 = mma_row<RM_HD / 8>(qb, Pw + (rt0 * 32 + lr) * RM_LD + lh * 4, g0);
    g1 = mma_row<RM_HD / 8>(qb, Pw + ((rt0 + 1) * 32 + lr) * RM_LD + lh * 4, g1);
    __syncthreads();                         // every wave is done with the P window and the K tile
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, lh);
      G[row * RM_LD + lr] = g0[r];
      G[row * RM_LD + 32 + lr] = g1[r];
    }
    // V tile (the K tile is consumed) while the skew buffers settle
    for (int i = tid; i < BK * (RM_HD / 4); i += 256) {
      const int r = i / (RM_HD / 4), c4 = (i - r * (RM_HD / 4)) * 4;
      float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k0 + r < L) vv = *reinterpret_cast<const float4*>(base + (long)(k0 + r) * 3 * d + 2 * d + h * RM_HD + c4);
      *reinterpret_cast<float4*>(KV + r * RM_LD + c4) = vv;
    }
    __syncthreads();
    {
      const bool valid = k0 + kj * 32 + lr < L;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lh);
        const float s = ac[r] + G[row * RM_LD + (lr - row + 31)];            // bd[i][j] = G[i][(j - i) + 31]
        Sc[(qi * 32 + row) * RM_LD + kj * 32 + lr] = valid ? s : -INFINITY;
      }
    }
    __syncthreads();
    online_softmax_row<true>(Sc + (tid >> 2) * RM_LD, tid >> 2, tid & 3, rm, rl, ra);
    __syncthreads();
    // O = O * alpha + P V : wave (qi, dj = kj) owns a 32 x 32 block
#pragma unroll
    for (int r = 0; r < 16; ++r) o[0][r] *= ra[qi * 32 + acc_row(r, lh)];
    pv_f32<1>(Sc + (qi * 32 + lr) * RM_LD + lh * 4, 0, KV + (lh * 4) * RM_LD + kj * 32 + lr, RM_LD, o);
  }
  __syncthreads();
  ctx_store(ctx, (long)b * L, h * RM_HD + kj * 32 + lr, d, q0 + qi * 32, L, lh, o, 1.0f, rl + qi * 32);
}

// ---- launchers: the shared-memory opt-in (per device and kernel), the profiler scope, the launch ----------------------
template <int HD, int KT, bool REL>
int launch_valu(const char* scope, double flops_per_term, const float* qkv, const float* P, const float* bu, const float* bv,
                int B, int L, int d, int nhead, float scale, float* ctx, hipStream_t s) {
  const int hd = d / nhead;
  const size_t smem = sizeof(float) * ((size_t)(REL ? 2 * VA_BQ * hd : VA_BQ * (hd + 1)) + (size_t)KT * (hd + 1) + (size_t)KT * hd +
                                       (size_t)(REL ? (KT + VA_BQ - 1) * (hd + 1) : 0) + (size_t)VA_BQ * KT);
  static SmemAttr attr;
  if (int rc = attr.ensure(reinterpret_cast<const void*>(attention_valu_kernel<HD, KT, REL>), smem)) return rc;
  ProfScope prof(s, scope, flops_per_term * B * nhead * (double)L * L * hd);
  hipLaunchKernelGGL((attention_valu_kernel<HD, KT, REL>), dim3(cdiv(L, VA_BQ), nhead, B), dim3(256), smem, s, qkv, P, bu, bv,
                     L, d, hd, scale, ctx);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

template <typename... KArgs, typename... Args>
int launch_mfma(void (*kern)(KArgs...), SmemAttr& attr, size_t smem, const char* scope, double flops, int B, int L, int nhead,
                hipStream_t s, Args... args) {
  if (int rc = attr.ensure(reinterpret_cast<const void*>(kern), smem)) return rc;
  ProfScope prof(s, scope, flops);
  hipLaunchKernelGGL(kern, dim3(cdiv(L, BQ), nhead, B), dim3(256), smem, s, args...);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

}  // namespace

extern "C" int asw_attention(const float* qkv, int B, int L, int d, int nhead, float* ctx, void* stream) {
  return asw_attention_prec(qkv, B, L, d, nhead, 0, ctx, stream);
}

extern "C" int asw_attention_prec(const float* qkv, int B, int L, int d, int nhead, int precision, float* ctx, void* stream) {
  ASW_CHECK_ARG(qkv && ctx, "attention: null pointer");
  ASW_CHECK_ARG(precision >= 0 && precision <= 2, "attention: precision %d", precision);
  ASW_CHECK_ARG(B > 0 && L > 0 && nhead > 0 && d % nhead == 0, "attention: bad shape");
  ASW_CHECK_ARG(B <= 65535 && nhead <= 65535, "attention: grid too large");
  hipStream_t s = asw::as_stream(stream);
  const int hd = d / nhead;
  if (hd == AD && (long)L * 3 * d * 4 < (1L << 31)) {          // the MFMA kernels read rows through a buffer descriptor
    const int LP = cdiv(L, BK) * BK;
    const size_t lds_max = 160 * 1024;
    const double flops = 4.0 * B * nhead * (double)L * L * AD;
    static const bool no16 = getenv("ASW_NO_ATTN16") != nullptr;          // A/B switch for measurements
    // f16x3 arithmetic: short sequences only (the probability rows replace the score rows in LDS)
    const size_t smem16 = (size_t)BQ * QRS + (size_t)2 * BK * VRS + (size_t)BQ * (LP * 4 + 16);
    if (precision >= 1 && !no16 && LP <= 352 && smem16 <= lds_max) {
      static SmemAttr attr16;
      static const int pf = getenv("ASW_ATTN_PF") ? atoi(getenv("ASW_ATTN_PF")) & 3 : 3;
      return launch_mfma(attention_mfma16_kernel, attr16, smem16, "attention_mfma16", flops, B, L, nhead, s, qkv, L, LP, d, ctx, pf);
    }
    // short sequences: the score rows of the 64 queries must fit beside Q and one K / V tile
    const size_t smem64 = sizeof(float) * ((size_t)BQ * LDQ + (size_t)BK * LDQ + (size_t)BQ * (LP + 4));
    if (smem64 <= lds_max) {
      static SmemAttr attr64;
      return launch_mfma(attention_mfma64_kernel, attr64, smem64, "attention_mfma64", flops, B, L, nhead, s, qkv, L, LP, d, ctx);
    }
    // long sequences: key-tiled two-pass kernel (any L)
    constexpr size_t smemf = sizeof(float) * ((size_t)BQ * LDQ + (size_t)BK * LDQ + (size_t)BQ * (BK + 4) + 2 * BQ);
    static SmemAttr attrf;
    return launch_mfma(attention_mfma_flash_kernel, attrf, smemf, "attention_mfma_flash", flops, B, L, nhead, s, qkv, L, d, ctx);
  }
  ASW_CHECK_ARG(hd % 16 == 0 && hd <= 128, "attention: head_dim %d must be a multiple of 16, <= 128", hd);
  return launch_valu<0, 128, false>("attention_valu", 4.0, qkv, nullptr, nullptr, nullptr, B, L, d, nhead, 1.0f / sqrtf((float)hd),
                                    ctx, s);
}

extern "C" int asw_relpos_attention(const float* qkv, const float* P, const float* bias_u, const float* bias_v, int BS, int L,
                                    int d, int nhead, float scale, float* ctx, void* stream) {
  ASW_CHECK_ARG(qkv && P && bias_u && bias_v && ctx, "relpos_attention: null pointer");
  ASW_CHECK_ARG(BS > 0 && BS <= 65535 && L > 0 && nhead > 0 && nhead <= 65535 && d % nhead == 0, "relpos_attention: bad shape");
  hipStream_t s = asw::as_stream(stream);
  static const bool valu_only = getenv("ASW_RELPOS_VALU") != nullptr;          // A/B switch for measurements
  if (d / nhead == RM_HD && d % 4 == 0 && !valu_only) {
    constexpr size_t smem = sizeof(float) * ((size_t)(3 * BQ + 2 * BK + BQ) * RM_LD + 3 * BQ);
    static SmemAttr attr;
    return launch_mfma(relpos_attention_mfma_kernel, attr, smem, "relpos_attention_mfma", 6.0 * BS * nhead * (double)L * L * RM_HD,
                       BS, L, nhead, s, qkv, P, bias_u, bias_v, L, d, scale, ctx);
  }
  switch (d / nhead) {
    case 16: return launch_valu<16, 64, true>("relpos_attention", 6.0, qkv, P, bias_u, bias_v, BS, L, d, nhead, scale, ctx, s);
    case 32: return launch_valu<32, 64, true>("relpos_attention", 6.0, qkv, P, bias_u, bias_v, BS, L, d, nhead, scale, ctx, s);
    case 64: return launch_valu<64, 64, true>("relpos_attention", 6.0, qkv, P, bias_u, bias_v, BS, L, d, nhead, scale, ctx, s);
    default: return asw::set_error(ASW_ERR_ARG, "relpos_attention: head_dim %d unsupported (16, 32, 64)", d / nhead);
  }
}
