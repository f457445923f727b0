// sep_kernels.hip -- the small (memory / latency bound, VALU) kernels of the joint separation
// network: joint normalisation statistics of the S x M zero-fill-shifted channels
// (sep/training/SpeakerSeparation/network.py:510-534 with :28-40) and the pieces of its
// bottleneck (:270-321) that are neither GEMMs nor attention over time -- row LayerNorms with
// fused residual adds, GLU, depthwise convolution + LayerNorm + Swish, and the inter-speaker
// attention over the S speakers of one time step (nn.TransformerEncoderLayer, :290-291,311-316).
// The relative-position self-attention over time is in attention.hip.
//
// The bottleneck tensors are [S][L][d] fp32 channels-last with L = T/64 (750 at T = 48 000),
// d = 512: a few MB, so every kernel here is one short pass and the stage is launch-latency
// bound; the GEMMs between them run on the MFMA kernels of convgemm.hip.
#include "asw_common.h"
#include "wave_util.h"

namespace {

using asw::quant16;
using asw::wave_max;
using asw::wave_sum;

__device__ __forceinline__ float swishf(float v) { return v / (1.0f + expf(-v)); }

// ---------------------------------------------------------------------------------------
// Joint statistics: ref[t] = mean over the S*M channels of the int16-quantised, zero-fill
// shifted mixture (channel (s,m) = mix[m] advanced by offsets[s][m-1], mic 0 unshifted);
// mean = mean_t ref, std = unbiased std_t ref.  Pass 1: per-block partial (sum, sum of
// squares) in double over a strided set of samples; pass 2: one wave reduces the partials and
// writes S copies (the preproc / un-normalise kernels take per-sequence arrays).
// ---------------------------------------------------------------------------------------
constexpr int JS_MAXCH = 2048;
constexpr int JS_BLOCKS = 128;

// Sequence groups of a ragged call, passed to the kernels by value (a few hundred bytes of kernel arguments: no device
// buffer, no copy): group g is the sequences bounds[g] .. bounds[g+1]-1 and, for the statistics, reads mixture item[g].
constexpr int RG_MAXG = 64;
struct GroupTable { int32_t bounds[RG_MAXG + 1]; int32_t item[RG_MAXG]; };

// blocks blockIdx.x of gridDim.x over the T samples of one item
__device__ __forceinline__ void joint_stats_partial(const float* __restrict__ mix, int M, int T,
                                                    const int32_t* __restrict__ offsets, int S, double* __restrict__ part) {
  __shared__ int off[JS_MAXCH];
  __shared__ double red[4][2];
  const int SM = S * M;
  for (int i = threadIdx.x; i < SM; i += 256) {
    const int s = i / M, m = i - s * M;
    off[i] = m == 0 ? 0 : offsets[(long)s * (M - 1) + m - 1];
  }
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
    float acc = 0.f;
    for (int s = 0; s < S; ++s)
      for (int m = 0; m < M; ++m) {
        const int i = t + off[s * M + m];
        const float x = (i >= 0 && i < T) ? mix[(long)m * T + i] : 0.f;
        acc += quant16(x);
      }
    const float r = acc / (float)SM;
    a0 += (double)r;
    a1 += (double)r * (double)r;
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[wid][0] = a0; red[wid][1] = a1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2 + 0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    part[blockIdx.x * 2 + 1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
  }
}

__device__ __forceinline__ void joint_stats_final(const double* __restrict__ part, int nblocks, int T, int S,
                                                  float* __restrict__ mean_out, float* __restrict__ std_out) {
  double a0 = 0.0, a1 = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) { a0 += part[i * 2]; a1 += part[i * 2 + 1]; }
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  const double mean = a0 / (double)T;
  double var = (a1 - a0 * a0 / (double)T) / (double)(T - 1);      // Bessel, torch.std default
  if (var < 0) var = 0;
  const float mu = (float)mean, sg = (float)sqrt(var);
  for (int s = threadIdx.x; s < S; s += 64) { mean_out[s] = mu; std_out[s] = sg; }
}

// The two passes for the G items of a call, item g = blockIdx.y: its own mixture, offsets, S_g, partials
// (2 * JS_BLOCKS doubles each) and rows of mean / std.  mix [K][M][T], offsets / mean / std over all N sequences.
// asw_joint_shift_stats is the call with one group.
__global__ __launch_bounds__(256) void joint_stats_partial_groups_kernel(const float* __restrict__ mix, int M, int T,
                                                                         const int32_t* __restrict__ offsets, GroupTable tab,
                                                                         double* __restrict__ part) {
  const int g = blockIdx.y, n0 = tab.bounds[g];
  joint_stats_partial(mix + (long)tab.item[g] * M * T, M, T, offsets + (long)n0 * (M - 1), tab.bounds[g + 1] - n0,
                      part + (long)g * 2 * JS_BLOCKS);
}

__global__ __launch_bounds__(64) void joint_stats_final_groups_kernel(const double* __restrict__ part, int nblocks, int T,
                                                                      GroupTable tab, float* __restrict__ mean_out,
                                                                      float* __restrict__ std_out) {
  const int g = blockIdx.x, n0 = tab.bounds[g];
  joint_stats_final(part + (long)g * 2 * JS_BLOCKS, nblocks, T, tab.bounds[g + 1] - n0, mean_out + n0, std_out + n0);
}

// ---------------------------------------------------------------------------------------
// Row kernel: s = x + alpha * y (y optional); sum_out = s (optional);
// ln_out = act(LayerNorm(s) * gamma + beta) (optional; act 0 = none, 2 = Swish).
// One wave per row, the row in registers (NV float4 per lane, N <= 256 * NV, N % 4 == 0),
// two-pass statistics by wave shuffles -- the arithmetic of the GEMM epilogue's LayerNorm.
// ---------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void add_ln2_kernel(const float* __restrict__ x, const float* __restrict__ y, float alpha,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int rows, int N, float eps, int act, float* __restrict__ sum_out,
                                                      float* __restrict__ ln_out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int n4 = N >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + (long)row * N);
  const float4* yr = y ? reinterpret_cast<const float4*>(y + (long)row * N) : nullptr;
  float4 v[NV];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c4 = i * 64 + lane;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < n4) {
      a = xr[c4];
      if (yr) { const float4 b = yr[c4]; a.x += alpha * b.x; a.y += alpha * b.y; a.z += alpha * b.z; a.w += alpha * b.w; }
      if (sum_out) reinterpret_cast<float4*>(sum_out + (long)row * N)[c4] = a;
    }
    v[i] = a;
    sum += (a.x + a.y) + (a.z + a.w);
  }
  if (!ln_out) return;
  const float mu = wave_sum(sum) / (float)N;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i * 64 + lane < n4) {
      const float dx = v[i].x - mu, dy = v[i].y - mu, dz = v[i].z - mu, dw = v[i].w - mu;
      sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)N + eps);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  float4* orow = reinterpret_cast<float4*>(ln_out + (long)row * N);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c4 = i * 64 + lane;
    if (c4 < n4) {
      const float4 g = g4[c4], b = b4[c4];
      float4 o = make_float4((v[i].x - mu) * rstd * g.x + b.x, (v[i].y - mu) * rstd * g.y + b.y,
                             (v[i].z - mu) * rstd * g.z + b.z, (v[i].w - mu) * rstd * g.w + b.w);
      if (act == 2) { o.x = swishf(o.x); o.y = swishf(o.y); o.z = swishf(o.z); o.w = swishf(o.w); }
      orow[c4] = o;
    }
  }
}

// out[r][c] = raw[r][c] * sigmoid(raw[r][C + c])   (nn.GLU over channels-last rows of 2C)
__global__ __launch_bounds__(256) void glu_rows_kernel(const float* __restrict__ raw, long rows, int C, float* __restrict__ out) {
  const int c4n = C >> 2;
  const long total = rows * c4n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / c4n;
    const int c = (int)(i - r * c4n) * 4;
    const float4 a = *reinterpret_cast<const float4*>(raw + r * 2 * C + c);
    const float4 g = *reinterpret_cast<const float4*>(raw + r * 2 * C + C + c);
    float4 o;
    o.x = a.x / (1.0f + expf(-g.x)); o.y = a.y / (1.0f + expf(-g.y));
    o.z = a.z / (1.0f + expf(-g.z)); o.w = a.w / (1.0f + expf(-g.w));
    *reinterpret_cast<float4*>(out + r * C + c) = o;
  }
}

// Depthwise Conv1d(d, d, k, padding (k-1)/2, groups = d) over time within each sequence,
// + bias, then LayerNorm over channels and Swish (ConvolutionModule: conv -> after_conv[0..1]).
// u, out: [BS][L][d]; wT: [K][d] (tap-major so a wave reads contiguous channel rows).
// One wave per (sequence, time) row.
template <int NV>
__global__ __launch_bounds__(256) void dwconv_ln_swish_kernel(const float* __restrict__ u, const float* __restrict__ wT,
                                                              const float* __restrict__ bias, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int BS, int L, int d, int K,
                                                              float eps, float* __restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (long)BS * L) return;
  const int seq = (int)(row / L), t = (int)(row - (long)seq * L);
  const int n4 = d >> 2, pad = (K - 1) / 2;
  float4 acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c4 = i * 64 + lane;
    acc[i] = c4 < n4 ? reinterpret_cast<const float4*>(bias)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int k = 0; k < K; ++k) {
    const int tt = t + k - pad;
    if (tt < 0 || tt >= L) continue;                     // wave-uniform: zero padding
    const float4* ur = reinterpret_cast<const float4*>(u + ((long)seq * L + tt) * d);
    const float4* wr = reinterpret_cast<const float4*>(wT + (long)k * d);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c4 = i * 64 + lane;
      if (c4 < n4) {
        const float4 a = ur[c4], w = wr[c4];
        acc[i].x = fmaf(a.x, w.x, acc[i].x); acc[i].y = fmaf(a.y, w.y, acc[i].y);
        acc[i].z = fmaf(a.z, w.z, acc[i].z); acc[i].w = fmaf(a.w, w.w, acc[i].w);
      }
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) sum += (acc[i].x + acc[i].y) + (acc[i].z + acc[i].w);     // lanes past the row hold zeros
  const float mu = wave_sum(sum) / (float)d;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i * 64 + lane < n4) {
      const float dx = acc[i].x - mu, dy = acc[i].y - mu, dz = acc[i].z - mu, dw = acc[i].w - mu;
      sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
  float4* orow = reinterpret_cast<float4*>(out + row * d);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c4 = i * 64 + lane;
    if (c4 < n4) {
      const float4 g = reinterpret_cast<const float4*>(gamma)[c4], b = reinterpret_cast<const float4*>(beta)[c4];
      orow[c4] = make_float4(swishf((acc[i].x - mu) * rstd * g.x + b.x), swishf((acc[i].y - mu) * rstd * g.y + b.y),
                             swishf((acc[i].z - mu) * rstd * g.z + b.z), swishf((acc[i].w - mu) * rstd * g.w + b.w));
    }
  }
}

// ---------------------------------------------------------------------------------------
// Inter-speaker attention: at every (item n, time step t, head h) the S speakers are the
// sequence (nn.MultiheadAttention inside nn.TransformerEncoderLayer(batch_first), applied to
// x.reshape(N*T, S, F), SpeakerSeparation/network.py:311-316).  qkv [N][S][L][3d] standard
// layout with in_proj bias already added; ctx [N][S][L][d].
// One wave per (n, t, head): the S x hd blocks of q, k, v are staged once into LDS (rows padded
// to hd+1 floats so the per-lane row walks are conflict free); lane s2 computes the scores
// (s1, s2) for every s1 with an in-lane dot product, the softmax runs across lanes, and for the
// output lane = head dimension.  S <= 64, hd <= 64.  IA_WAVES waves (units) per workgroup: 4 while their
// regions fit the CU's LDS (S <= 39 at hd = 64), else 2 (any S <= 64: 2 x 66 KB at S = 64, hd = 64) or 1.
// ---------------------------------------------------------------------------------------
// One unit on one wave: the S sequences n0 .. n0+S-1 at time step t, head h, in the wave's LDS region
// (3 * S * (hd+1) + S * 64 floats).  Every wave of the workgroup reaches both barriers; an inactive one does nothing else.
__device__ __forceinline__ void inter_attention_unit(const float* __restrict__ qkv, int n0, int S, int t, int h, int L, int d,
                                                     int hd, bool active, float* __restrict__ Qs, int lane,
                                                     float* __restrict__ ctx) {
  const int ldk = hd + 1;
  float* Ks = Qs + S * ldk;                                       // per-wave region: Q, K, V [S][hd+1], P [S][64]
  float* Vs = Ks + S * ldk;
  float* Ps = Vs + S * ldk;
  const float scale = 1.0f / sqrtf((float)hd);
  for (int i = lane; active && i < S * hd; i += 64) {
    const int s = i / hd, c = i - s * hd;
    const float* row = qkv + ((long)(n0 + s) * L + t) * 3 * d + h * hd + c;
    Qs[s * ldk + c] = row[0] * scale;
    Ks[s * ldk + c] = row[d];
    Vs[s * ldk + c] = row[2 * d];
  }
  __syncthreads();
  for (int s1 = 0; active && s1 < S; ++s1) {
    float sc = -INFINITY;
    if (lane < S) {
      float acc = 0.f;
      const float* qr = Qs + s1 * ldk;
      const float* kr = Ks + lane * ldk;
      for (int c = 0; c < hd; ++c) acc = fmaf(qr[c], kr[c], acc);
      sc = acc;
    }
    const float mx = wave_max(sc);
    const float e = lane < S ? expf(sc - mx) : 0.f;
    const float p = e / wave_sum(e);
    Ps[s1 * 64 + lane] = p;
  }
  __syncthreads();
  if (active && lane < hd) {
    for (int s1 = 0; s1 < S; ++s1) {
      float acc = 0.f;
      for (int s2 = 0; s2 < S; ++s2) acc = fmaf(Ps[s1 * 64 + s2], Vs[s2 * ldk + lane], acc);
      ctx[((long)(n0 + s1) * L + t) * d + h * hd + lane] = acc;
    }
  }
}

// The units of one call: unit (g, t, h) attends over the sequences of group g only.  qkv [N][L][3d], ctx [N][L][d].
// The groups are either all S_uniform > 0 sequences wide -- group g is the sequences g * S_uniform ..., any number of
// groups, the table is not read -- or, with S_uniform == 0, the G <= RG_MAXG groups of `tab`, of different sizes
// (N = tab.bounds[G]).  The LDS regions are S_max = max S_g wide.
template <int IA_WAVES>
__global__ __launch_bounds__(64 * IA_WAVES) void inter_attention_groups_kernel(const float* __restrict__ qkv, GroupTable tab,
                                                                               int G, int S_uniform, int S_max, int L, int d,
                                                                               int nhead, float* __restrict__ ctx) {
  extern __shared__ __align__(16) float smem[];
  const int hd = d / nhead;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long unit = (long)blockIdx.x * IA_WAVES + wid;                  // (g, t, h)
  const bool active = unit < (long)G * L * nhead;                 // wave-uniform
  if (!active) unit = 0;
  const int h = (int)(unit % nhead);
  const long gt = unit / nhead;
  const int g = (int)(gt / L), t = (int)(gt - (long)g * L);
  const int n0 = S_uniform ? g * S_uniform : tab.bounds[g];
  const int S = S_uniform ? S_uniform : tab.bounds[g + 1] - n0;
  inter_attention_unit(qkv, n0, S, t, h, L, d, hd, active, smem + (size_t)wid * (3 * S_max * (hd + 1) + S_max * 64), lane, ctx);
}

// host: the groups of a ragged call.  bounds [G+1] non-decreasing from 0, every group 1..64 sequences.
int fill_group_table(const char* who, const int32_t* bounds, int G, GroupTable& tab, int* s_max) {
  if (G < 1 || G > RG_MAXG) return asw::set_error(ASW_ERR_ARG, "%s: G=%d groups (1..%d per call)", who, G, RG_MAXG);
  if (bounds[0] != 0) return asw::set_error(ASW_ERR_ARG, "%s: bounds[0]=%d, must be 0", who, bounds[0]);
  *s_max = 0;
  for (int g = 0; g < G; ++g) {
    const long sg = (long)bounds[g + 1] - bounds[g];
    if (sg < 1 || sg > 64)
      return asw::set_error(ASW_ERR_ARG, "%s: group %d holds %ld sequences (1..64; empty groups are left out)", who, g, sg);
    *s_max = (int)sg > *s_max ? (int)sg : *s_max;
  }
  for (int g = 0; g <= RG_MAXG; ++g) tab.bounds[g] = bounds[g <= G ? g : G];
  for (int g = 0; g < RG_MAXG; ++g) tab.item[g] = 0;
  return ASW_OK;
}

// waves (units) per workgroup of the inter-speaker attention and the LDS bytes of one: 4 regions while they fit, else 2, 1
int inter_attention_waves(const char* who, int S, int hd, size_t* per_wave) {
  *per_wave = sizeof(float) * (3 * (size_t)S * (hd + 1) + (size_t)S * 64);
  const size_t lds_max = 160 * 1024;
  if (*per_wave > lds_max) {
    asw::set_error(ASW_ERR_ARG, "%s: S=%d x head_dim %d needs %zu bytes of LDS per wave", who, S, hd, *per_wave);
    return 0;
  }
  return 4 * *per_wave <= lds_max ? 4 : 2 * *per_wave <= lds_max ? 2 : 1;
}

// the two passes of the joint statistics over the G groups of `tab`; scratch holds 2 * JS_BLOCKS doubles per group
int launch_joint_stats(const float* mix, int M, int T, const int32_t* offsets, const GroupTable& tab, int G, double* scratch,
                       float* mean, float* std, hipStream_t s) {
  const int nb = asw::cdiv(T, 256) < JS_BLOCKS ? asw::cdiv(T, 256) : JS_BLOCKS;
  hipLaunchKernelGGL(joint_stats_partial_groups_kernel, dim3(nb, G), dim3(256), 0, s, mix, M, T, offsets, tab, scratch);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(joint_stats_final_groups_kernel, dim3(G), dim3(64), 0, s, scratch, nb, T, tab, mean, std);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

}  // namespace

// The one launcher of the inter-speaker attention (internal; sep_model.hip calls it for every kind of call): G groups,
// either all S_uniform > 0 wide (bounds unused, any G) or the host bounds [G+1] of a ragged call (S_uniform == 0).
// The shape (L, d, nhead, head_dim <= 64, S_uniform <= 64) is the caller's to check.
namespace asw {
int inter_attention_launch(const char* who, const float* qkv, const int32_t* bounds, int G, int S_uniform, int L, int d,
                           int nhead, float* ctx, hipStream_t st) {
  GroupTable tab = {};
  int s_max = S_uniform;
  if (!S_uniform)
    if (int rc = fill_group_table(who, bounds, G, tab, &s_max)) return rc;
  size_t per_wave;
  const int waves = inter_attention_waves(who, s_max, d / nhead, &per_wave);
  if (!waves) return ASW_ERR_ARG;
  const size_t smem = per_wave * waves;
  const int v = waves == 4 ? 0 : waves == 2 ? 1 : 2;
  using Kern = void (*)(const float*, GroupTable, int, int, int, int, int, int, float*);
  static const Kern kern[3] = {inter_attention_groups_kernel<4>, inter_attention_groups_kernel<2>, inter_attention_groups_kernel<1>};
  static SmemAttr attr[3];                                     // per device and instantiation
  if (int rc = attr[v].ensure(reinterpret_cast<const void*>(kern[v]), smem)) return rc;
  asw::ProfScope prof(st, who, 4.0 * G * L * nhead * (double)s_max * s_max * (d / nhead));   // s_max: an upper bound when ragged
  hipLaunchKernelGGL(kern[v], dim3(cdiv((long)G * L * nhead, waves)), dim3(64 * waves), smem, st, qkv, tab, G, S_uniform, s_max,
                     L, d, nhead, ctx);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
}  // namespace asw

extern "C" int asw_joint_shift_stats(const float* mix, int M, int T, const int32_t* offsets, int S, double* scratch,
                                     float* mean, float* std, void* stream) {
  ASW_CHECK_ARG(mix && offsets && scratch && mean && std, "joint_shift_stats: null pointer");
  ASW_CHECK_ARG(M >= 1 && S >= 1 && S * M <= JS_MAXCH && T >= 2, "joint_shift_stats: S=%d M=%d T=%d unsupported (S*M <= %d)", S,
                M, T, JS_MAXCH);
  // one group: every sequence, mixture 0.  Built here, not by fill_group_table: S is bounded by S * M alone
  GroupTable tab = {};
  for (int g = 1; g <= RG_MAXG; ++g) tab.bounds[g] = S;
  return launch_joint_stats(mix, M, T, offsets, tab, 1, scratch, mean, std, asw::as_stream(stream));
}

extern "C" int asw_joint_shift_stats_scratch_doubles(void) { return 2 * JS_BLOCKS; }

extern "C" int asw_joint_shift_stats_groups(const float* mix, int M, int T, const int32_t* offsets, const int32_t* bounds,
                                            int G, const int32_t* item_of_group, double* scratch, float* mean, float* std,
                                            void* stream) {
  ASW_CHECK_ARG(G >= 0, "joint_shift_stats_groups: G=%d", G);
  if (G == 0) return ASW_OK;
  ASW_CHECK_ARG(mix && offsets && bounds && item_of_group && scratch && mean && std, "joint_shift_stats_groups: null pointer");
  ASW_CHECK_ARG(M >= 1 && T >= 2, "joint_shift_stats_groups: M=%d T=%d unsupported", M, T);
  GroupTable tab;
  int s_max;
  if (int rc = fill_group_table("joint_shift_stats_groups", bounds, G, tab, &s_max)) return rc;
  ASW_CHECK_ARG((long)s_max * M <= JS_MAXCH, "joint_shift_stats_groups: an item of %d sequences x %d channels (S*M <= %d)", s_max,
                M, JS_MAXCH);
  for (int g = 0; g < G; ++g) {
    ASW_CHECK_ARG(item_of_group[g] >= 0, "joint_shift_stats_groups: group %d reads mixture %d", g, item_of_group[g]);
    tab.item[g] = item_of_group[g];
  }
  return launch_joint_stats(mix, M, T, offsets, tab, G, scratch, mean, std, asw::as_stream(stream));
}

extern "C" int asw_add_layernorm2(const float* x, const float* y, float alpha, const float* gamma, const float* beta,
                                  int rows, int N, float eps, int act, float* sum_out, float* ln_out, void* stream) {
  ASW_CHECK_ARG(x && (sum_out || ln_out), "add_layernorm2: null pointer");
  ASW_CHECK_ARG(!ln_out || (gamma && beta), "add_layernorm2: LayerNorm needs gamma and beta");
  ASW_CHECK_ARG(rows >= 0 && N > 0 && N % 4 == 0 && N <= 2048, "add_layernorm2: N=%d must be a multiple of 4, <= 2048", N);
  ASW_CHECK_ARG(act == 0 || act == 2, "add_layernorm2: act must be 0 (none) or 2 (Swish)");
  if (rows == 0) return ASW_OK;
  hipStream_t s = asw::as_stream(stream);
  dim3 grid(asw::cdiv(rows, 4));
  switch ((N + 255) / 256) {
#define ASW_ALN2(NV) case NV: hipLaunchKernelGGL(add_ln2_kernel<NV>, grid, dim3(256), 0, s, x, y, alpha, gamma, beta, rows, N, eps, act, sum_out, ln_out); break;
    ASW_ALN2(1) ASW_ALN2(2) ASW_ALN2(3) ASW_ALN2(4) ASW_ALN2(5) ASW_ALN2(6) ASW_ALN2(7) ASW_ALN2(8)
#undef ASW_ALN2
  }
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_glu_rows(const float* raw, long rows, int C, float* out, void* stream) {
  ASW_CHECK_ARG(raw && out, "glu_rows: null pointer");
  ASW_CHECK_ARG(rows >= 0 && C > 0 && C % 4 == 0, "glu_rows: C=%d must be a multiple of 4", C);
  if (rows == 0) return ASW_OK;
  const long total = rows * (C / 4);
  const int blocks = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
  hipLaunchKernelGGL(glu_rows_kernel, dim3(blocks), dim3(256), 0, asw::as_stream(stream), raw, rows, C, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_dwconv_ln_swish(const float* u, const float* wT, const float* bias, const float* gamma, const float* beta,
                                   int BS, int L, int d, int K, float eps, float* out, void* stream) {
  ASW_CHECK_ARG(u && wT && bias && gamma && beta && out, "dwconv_ln_swish: null pointer");
  ASW_CHECK_ARG(BS > 0 && L > 0 && d > 0 && d % 4 == 0 && d <= 1024 && K >= 1 && K % 2 == 1,
                "dwconv_ln_swish: bad shape (d %% 4, d <= 1024, odd K)");
  hipStream_t s = asw::as_stream(stream);
  dim3 grid(asw::cdiv((long)BS * L, 4));
  switch ((d + 255) / 256) {
#define ASW_DW(NV) case NV: hipLaunchKernelGGL(dwconv_ln_swish_kernel<NV>, grid, dim3(256), 0, s, u, wT, bias, gamma, beta, BS, L, d, K, eps, out); break;
    ASW_DW(1) ASW_DW(2) ASW_DW(3) ASW_DW(4)
#undef ASW_DW
  }
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_inter_attention(const float* qkv, int NB, int S, int L, int d, int nhead, float* ctx, void* stream) {
  ASW_CHECK_ARG(qkv && ctx, "inter_attention: null pointer");
  ASW_CHECK_ARG(NB > 0 && S > 0 && S <= 64 && L > 0 && nhead > 0 && d % nhead == 0 && d / nhead <= 64,
                "inter_attention: bad shape (S <= 64, head_dim <= 64)");
  return asw::inter_attention_launch("inter_attention", qkv, nullptr, NB, S, L, d, nhead, ctx, asw::as_stream(stream));
}

extern "C" int asw_inter_attention_groups(const float* qkv, const int32_t* bounds, int G, int L, int d, int nhead, float* ctx,
                                          void* stream) {
  ASW_CHECK_ARG(G >= 0, "inter_attention_groups: G=%d", G);
  if (G == 0) return ASW_OK;
  ASW_CHECK_ARG(qkv && bounds && ctx, "inter_attention_groups: null pointer");
  ASW_CHECK_ARG(L > 0 && nhead > 0 && d > 0 && d % nhead == 0 && d / nhead <= 64,
                "inter_attention_groups: bad shape (head_dim <= 64)");
  return asw::inter_attention_launch("inter_attention_groups", qkv, bounds, G, 0, L, d, nhead, ctx, asw::as_stream(stream));
}
