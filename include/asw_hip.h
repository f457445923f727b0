/*
 * asw_hip.h -- C ABI of libasw_hip.so: the MI355X (gfx950) implementation of the
 * Spotforming localization-by-separation hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes (device
 * pointers unless a parameter says "host"), enqueues its work on the given HIP
 * stream (hipStream_t passed as void*; NULL = default stream) and returns 0 or a
 * negative asw_status.  No exception crosses the ABI; asw_last_error() returns a
 * thread-local message for the last failure.  Inputs are borrowed and never
 * mutated; outputs are caller-owned buffers.
 *
 * Each function cites the reference interface (file:line under the upstream
 * repo) it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 */
#ifndef ASW_HIP_H
#define ASW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum asw_status {
  ASW_OK = 0,
  ASW_ERR_ARG = -1,       /* bad shape / null pointer / unsupported configuration */
  ASW_ERR_HIP = -2,       /* a HIP runtime call failed                             */
  ASW_ERR_NOMEM = -3,     /* device allocation failed                              */
  ASW_ERR_STATE = -4      /* handle used before weights were loaded                */
} asw_status;

const char* asw_last_error(void);
int asw_abi_version(void);

/* Optional launch profiler: while enabled, every GEMM-class launch is bracketed by HIP
 * events on its own stream.  asw_profile_enable(on) also clears earlier records
 * (on = 2: launch names carry their shape, "name[B.. M.. ..]", and stand for the arithmetic of
 * the launch alone; on = 3: the shape and, as with on = 1, the tiling form where several
 * compute the same bits, such as resstack64's ",carry");
 * asw_profile_report() waits for the recorded events and writes a JSON object
 * {"kernel<tile>": {"launches": n, "ms": total, "work": flops}, ...} into buf. */
int asw_profile_enable(int on);
int asw_profile_report(char* buf, size_t cap);

/* ------------------------------------------------------------------------
 * Spot-network hyper-parameters.  Mirrors Network.__init__
 * (sep/training/SpeakerLocalization/network.py:268-292).
 * ---------------------------------------------------------------------- */
typedef struct asw_spot_config {
  int32_t n_mics;                 /* 7 */
  int32_t kernel_size;            /* 7 */
  int32_t depth;                  /* len(stride_list) <= 8 */
  int32_t stride_list[8];         /* 2,2,4,4,4 */
  int32_t channels;               /* 64 */
  int32_t growth;                 /* 2 */
  int32_t encoder_channels;       /* 2048 */
  int32_t encoder_kernel_size;    /* 33 */
  int32_t encoder_stride;         /* 16 */
  int32_t residual_layers;        /* 3 */
  int32_t residual_dilation_factor; /* 7 */
  int32_t num_head;               /* 8 */
  int32_t ffw_dim;                /* 1024 */
  int32_t num_transformer_layers; /* 2 */
} asw_spot_config;

typedef struct asw_spot asw_spot;   /* opaque: device-resident weights + workspace */

/* Create a model for `cfg` on the current HIP device.  Replaces Network(**model_params)
 * + .to(device) (sep/helpers/utils.py:176-183, sep/training/base_network.py:41-45). */
int asw_spot_create(const asw_spot_config* cfg, asw_spot** out);
void asw_spot_destroy(asw_spot* m);

/* Upload one tensor of a reference-format state dict (host float32, contiguous, in the
 * reference's own layout and key name, SURVEY.md §8 a-N).  Replaces
 * model.load_state_dict(..., strict=True) (sep/helpers/utils.py:196-198).
 * asw_spot_finalize() checks that every key arrived (strict) and packs the weights
 * into the kernels' layouts. */
int asw_spot_set_param(asw_spot* m, const char* key, const float* host_data, size_t numel);
int asw_spot_finalize(asw_spot* m);

/* Maximum number of candidates processed per internal batch (the reference's
 * spot_batch_size, sep/training/JointModel/network.py:28,75). */
int asw_spot_set_batch(asw_spot* m, int batch);

/* Number of execution lanes (1 or 2, default 1).  With 2, consecutive internal batches of one
 * asw_spot_shift_and_sep call run on two HIP streams (the caller's stream and a library-owned
 * side stream, forked and joined with events inside the call) with one workspace each, so the
 * memory-bound passes and the launch tails of one batch overlap the MFMA kernels of the other.
 * Results are identical; the call still only depends on, and is ordered by, the caller's stream. */
int asw_spot_set_lanes(asw_spot* m, int lanes);

/* Arithmetic of the GEMM-class layers: 0 = exact fp32 MFMA (default), 1 = "f16x3"
 * split-operand half MFMA with fp32 accumulation, 2 = optional single-pass f16 (reduced
 * precision; see asw_convgemm_args.precision), 3 = "f16x3_safe": f16x3 without its fp16 range limit.
 * In mode 3 a GEMM runs the f16x3 kernels exactly as in mode 1 if and only if its A operand is bounded by
 * construction -- the output of a LayerNorm, of GroupNorm + GLU or of the input normalisation, Swish of such an
 * output, or the skip-add of two of them: the whole U-Net trunk, in_proj, the first feed-forward linears, the
 * Conformer's pointwise convolutions, the mask encoder and the bypass.  The sites that read an un-normalised tensor
 * run on the exact f32 MFMA: the attention core, out_proj (reads the context), the second feed-forward linears (read
 * the hidden layer), and the output_decoder tap GEMM of the three-GEMM mask path (reads the masked latent); the
 * one-launch mask path becomes asw_mask_path_f16x3_scaled.  asw_f16x3_overflow_count then reads 0 for any finite
 * weights.  What remains assumed: a normalised tensor is bounded by its affine parameters, roughly
 * sqrt(n) * max|gamma| + max|beta| for n channels, and that bound is below 65504. */
int asw_spot_set_precision(asw_spot* m, int precision);

/* The hot loop: replaces DataParallelSpotModel.shift_and_sep
 * (sep/training/JointModel/network.py:37-104): for each of the N candidates,
 * circularly advance channel m>=1 of `mix` by offsets[n][m-1] samples, int16-quantise
 * and normalise (network.py:28-40), run the spot network with the window one-hot
 * selected by `strict` (1 -> [1,0], else [0,1]), un-normalise (network.py:42-47).
 *   mix      [M][T] float32 device
 *   offsets  [N][M-1] int32 device (already rounded, JointModel/network.py:81-82)
 *   out_wave [N][T] float32 device, or NULL
 *   out_energy [N][2] float64 device, or NULL: (power, power2) of the mean-removed
 *              output as computed by the stage loops (sep/helpers/local_utils_3d.py:13-17,
 *              349-354; sep/Mic_Array.py:290-295) with window `energy_window` samples. */
int asw_spot_shift_and_sep(asw_spot* m, const float* mix, int M, int T,
                           const int32_t* offsets, int N, int strict, int circular,
                           float* out_wave, double* out_energy, int energy_window,
                           void* stream);

/* The same call over the candidates of SEVERAL mixtures in one stream (the reference fills its 128-wide
 * batches from one mixture at a time, sep/training/JointModel/network.py:75-96; a batch of mixtures --
 * BASELINE configs[3] -- keeps the internal batches full when its searches are interleaved):
 *   mix [K][M][T] float32 device, mix_index [N] int32 device (candidate n reads mixture mix_index[n], values in
 *   [0, K); may be NULL when K == 1).  The mix_index values are NOT range-checked on the device: the caller
 *   guarantees them.  Everything else as asw_spot_shift_and_sep; each candidate's result is the one it has in a
 *   single-mixture call of the same internal batch size. */
int asw_spot_shift_and_sep_multi(asw_spot* m, const float* mix, int K, int M, int T, const int32_t* offsets,
                                 const int32_t* mix_index, int N, int strict, int circular, float* out_wave,
                                 double* out_energy, int energy_window, void* stream);

/* Network.forward (sep/training/SpeakerLocalization/network.py:363-405) on already
 * normalised input: mix [B][M][t], window_embedding host [2] shared by the batch ->
 * out [B][t]. */
int asw_spot_forward(asw_spot* m, const float* mix_norm, int B, int M, int t,
                     const float* window_embedding_host, float* out, void* stream);

/* f16x3 mode runs the mask path (reference_bypass, mask_encoder, product, output_decoder taps) as ONE
 * launch (asw_mask_path_f16x3) when the shapes fit (encoder_channels % 256 == 0, channels % 32 == 0,
 * kernel <= 48): the latent is then never written and the "latent" tap does not exist; and the
 * 64-channel decoder blocks apply GroupNorm + GLU while their first residual layer loads its rows
 * (asw_convgemm_args.glu_raw).  on = 0 selects the three-GEMM mask path and the separate GroupNorm + GLU
 * pass everywhere (default: on). */
int asw_spot_set_fused_mask(asw_spot* m, int on);

/* f16x3 mode, 64 channels at level 0, n_mics <= 7, kernel_size <= 7: asw_spot_shift_and_sep[_multi] folds the 1x1
 * preproc convolution into the first residual layer of encoder block 0 (no non-linearity separates them): the front end
 * writes the 8-channel network input (asw_shift_norm_src_multi) instead of the 64-channel preproc output, and the
 * block's first fused pair runs source-fed (asw_resstack_args.src_hi).  The preproc output is then never written and
 * the "preproc" tap does not exist after such a call.  on = 0 selects the separate preproc pass (default: on).
 * asw_spot_forward, the f32 and the single-pass f16 modes always take the separate pass. */
int asw_spot_set_source_stack(asw_spot* m, int on);

/* f16x3 mode: in asw_spot_shift_and_sep[_multi] the residual stack of the decoder block in front of a 64 -> 64 channel
 * stride-2 block applies that block's transposed convolution from its registers (asw_resstack_args.up_hi): its own
 * output is never written, the separate GEMM launch and one round trip of that tensor disappear, and the tap "dec<j>"
 * of the block in front does not exist after such a call ("no activation named dec<j>").  on = 0 selects the
 * separate launch (default: on).  asw_spot_forward, the f32 and the single-pass f16 modes always take the separate
 * launch; f16x3_safe takes the fused one as f16x3 does (the site reads a normalised tensor, which that mode runs on the
 * same kernels, so the two modes' launch plans keep differing in the exact-f32 sites only). */
int asw_spot_set_up_fusion(asw_spot* m, int on);

/* Debug/parity tap: copy an intermediate activation of the LAST forward to `dst`
 * (channels-last [B][T_l][C] float32).  names: "preproc", "enc0".., "bottleneck",
 * "dec0".., "latent" (three-GEMM mask path only); "preproc" does not exist after a
 * shift_and_sep call that took the source-fed path (asw_spot_set_source_stack): the call then fails with "no
 * activation named preproc".  Returns the element count through *numel (dst may be NULL). */
int asw_spot_get_tap(asw_spot* m, const char* name, float* dst, size_t capacity, size_t* numel,
                     void* stream);

/* ------------------------------------------------------------------------
 * Joint separation network ("separation by localization").  Mirrors Network.__init__
 * (sep/training/SpeakerSeparation/network.py:323-416; experiments/separation/
 * description.json:4-10).  The bottleneck's Conformer follows the published speechbrain
 * definitions (the library is absent from the build image: parity of that part is pinned to
 * this repository's restatement only, see oracle/sep_ref.py).
 * ---------------------------------------------------------------------- */
typedef struct asw_sep_config {
  int32_t n_mics;                 /* 7 */
  int32_t max_speakers;           /* 5 (constructor default 6): forward() pads its rows to this */
  int32_t kernel_size;            /* 5 */
  int32_t depth;                  /* len(stride_list) <= 8 */
  int32_t stride_list[8];         /* 2,2,4,4 */
  int32_t channels;               /* 64 */
  int32_t growth;                 /* 2 */
  int32_t encoder_channels;       /* 4096 */
  int32_t encoder_kernel_size;    /* 33 */
  int32_t encoder_stride;         /* 16 */
  int32_t residual_layers;        /* 3 */
  int32_t residual_dilation_factor; /* 2 */
  int32_t num_head;               /* 8 */
  int32_t ffw_dim;                /* 1024 */
  int32_t bottleneck_layers;      /* 3 */
  int32_t bottleneck_ksize;       /* 31 */
} asw_sep_config;

typedef struct asw_sep asw_sep;     /* opaque: device-resident weights + workspace */

/* Network(**model_params).to(device) + load_state_dict(strict=True)
 * (sep/helpers/utils.py:176-198); same protocol as the asw_spot_* calls above. */
int asw_sep_create(const asw_sep_config* cfg, asw_sep** out);
void asw_sep_destroy(asw_sep* m);
int asw_sep_set_param(asw_sep* m, const char* key, const float* host_data, size_t numel);
int asw_sep_finalize(asw_sep* m);
int asw_sep_set_precision(asw_sep* m, int precision);   /* 0..3, as asw_spot_set_precision */

/* Network.infer_sample (SpeakerSeparation/network.py:496-548): for each of the S speakers
 * advance channel m>=1 of `mix` by offsets[s][m-1] samples with ZERO fill (:510-522), stack to
 * S*M channels, int16-quantise and normalise with ONE mean / std over all of them (:534),
 * run the network and un-normalise.
 *   mix [M][T] float32 device; offsets [S][M-1] int32 device (already rounded, :507);
 *   out [S][T] float32 device.  S <= 64. */
int asw_sep_infer(asw_sep* m, const float* mix, int M, int T, const int32_t* offsets, int S, float* out,
                  void* stream);

/* asw_sep_infer for K mixtures of one shape in ONE call, each with its own number of talkers: sequence n of item k is
 * exactly what asw_sep_infer(mix[k], the offsets of item k) computes for it.  The talkers of an item are normalised with
 * that item's joint statistics and attend only to each other in the inter-speaker layers; the N = sum counts sequences
 * are packed item after item with no padding, so the rest of the network runs once with batch N.
 *   mix [K][M][T] float32 device; offsets [N][M-1] int32 device, item after item, already rounded;
 *   counts host int32 [K], each 0..64 (an item with none contributes no rows); out [N][T] float32 device.  N <= 64.
 * K = 0 or N = 0 succeeds and launches nothing.  Refused on the host, before any launch: a null pointer, M other than
 * the model's, T < 2, K < 0, a count outside 0..64, N > 64. */
int asw_sep_infer_batch(asw_sep* m, const float* mix, int K, int M, int T, const int32_t* offsets,
                        const int32_t* counts, float* out, void* stream);

/* Network.forward (:418-490) on already normalised input, every item with the same number of
 * speakers: mix_norm [B][S*M][t] -> out [B][max(S, max_speakers)][t] (rows beyond S are zeros,
 * :486-488).  B*S <= 64. */
int asw_sep_forward(asw_sep* m, const float* mix_norm, int B, int S, int M, int t, float* out, void* stream);
/* Network.forward with DIFFERENT speaker counts per item (speakers_to_batches / batches_to_speakers, :236-268):
 * mix_norm [B][S*M][t] with S = the largest count; counts host int32 [B], 1 <= counts[b] <= S (NULL: S everywhere).
 * A missing speaker enters every inter-speaker layer as a zero sequence and leaves as the bare output_decoder bias; the
 * channels of its block in mix_norm are ignored. */
int asw_sep_forward_counts(asw_sep* m, const float* mix_norm, int B, int S, int M, int t, const int32_t* counts,
                           float* out, void* stream);
/* The hyper-parameters the handle was created with (a caller that sizes `out` of asw_sep_forward from
 * max_speakers must use the handle's value, not its own). */
int asw_sep_get_config(const asw_sep* m, asw_sep_config* out);

/* Debug/parity tap of the LAST call (channels-last [B*S][T_l][C] float32): "enc0".., "intra0"..,
 * "inter0".., "bottleneck", "dec0".. */
int asw_sep_get_tap(asw_sep* m, const char* name, float* dst, size_t capacity, size_t* numel, void* stream);

/* Joint normalisation statistics of the S*M zero-fill-shifted, int16-quantised channels
 * (SpeakerSeparation/network.py:510-534 with :28-35): mean / unbiased std over time of the
 * all-channel average.  scratch: asw_joint_shift_stats_scratch_doubles() doubles (device).
 * mean, std: [S] float32 (the same value S times, the layout the preproc kernel takes). */
int asw_joint_shift_stats(const float* mix, int M, int T, const int32_t* offsets, int S, double* scratch,
                          float* mean, float* std, void* stream);
int asw_joint_shift_stats_scratch_doubles(void);
/* The same statistics for the G items of a ragged call (asw_sep_infer_batch), each over its own S_g*M channels:
 * mix [K][M][T]; offsets [N][M-1], mean / std [N] over all sequences; bounds host int32 [G+1], non-decreasing from 0
 * with bounds[G] = N: item g is the sequences bounds[g] .. bounds[g+1]-1 (1..64 of them, S_g*M <= 2048) and reads
 * mixture item_of_group[g] (host int32 [G], values in [0, K): not range-checked).  G <= 64; the two tables travel as
 * kernel arguments.  Same partition of the samples and same order of the sums as asw_joint_shift_stats: a one-item
 * call writes the same bytes.  scratch: G * asw_joint_shift_stats_scratch_doubles() doubles (device). */
int asw_joint_shift_stats_groups(const float* mix, int M, int T, const int32_t* offsets, const int32_t* bounds, int G,
                                 const int32_t* item_of_group, double* scratch, float* mean, float* std, void* stream);

/* Row kernel of the Conformer layer: s = x + alpha*y (y may be NULL); sum_out = s (may be NULL);
 * ln_out = act(LayerNorm(s)*gamma + beta) (may be NULL; act 0 none, 2 Swish).  rows x N floats,
 * N % 4 == 0, N <= 2048.  Replaces the residual adds and LayerNorms of ConformerEncoderLayer. */
int asw_add_layernorm2(const float* x, const float* y, float alpha, const float* gamma, const float* beta,
                       int rows, int N, float eps, int act, float* sum_out, float* ln_out, void* stream);

/* nn.GLU over channels-last rows: raw [rows][2C] -> out [rows][C] = raw[:, :C] * sigmoid(raw[:, C:]). */
int asw_glu_rows(const float* raw, long rows, int C, float* out, void* stream);

/* ConvolutionModule tail: depthwise Conv1d(d, d, K, padding (K-1)/2, groups d) over time within
 * each of the BS sequences + bias, LayerNorm over channels, Swish.  u, out [BS][L][d];
 * wT [K][d] (tap-major copy of the [d][1][K] weight). */
int asw_dwconv_ln_swish(const float* u, const float* wT, const float* bias, const float* gamma, const float* beta,
                        int BS, int L, int d, int K, float eps, float* out, void* stream);

/* Relative-position multi-head self-attention core (speechbrain RelPosMHAXL as published):
 * score[i][j] = scale*((q_i+u).k_j + (q_i+v).P[(L-1)+j-i]); ctx = softmax(score) V.
 * qkv [BS][L][3d] in Q|K|V layout (head h at columns h*hd), P [2L-1][d] = linear_pos(table),
 * bias_u / bias_v [d] head-major; ctx [BS][L][d].  head_dim in {16, 32, 64}. */
int asw_relpos_attention(const float* qkv, const float* P, const float* bias_u, const float* bias_v, int BS, int L,
                         int d, int nhead, float scale, float* ctx, void* stream);

/* Inter-speaker attention core: for every (item, time step, head) softmax(QK^T/sqrt(hd))V over the
 * S speakers (nn.TransformerEncoderLayer on x.reshape(N*T, S, F), :311-316).
 * qkv [NB][S][L][3d] (in_proj bias included) -> ctx [NB][S][L][d].  S <= 64, head_dim <= 64. */
int asw_inter_attention(const float* qkv, int NB, int S, int L, int d, int nhead, float* ctx, void* stream);
/* The same core over G groups of DIFFERENT sizes: qkv [N][L][3d] -> ctx [N][L][d]; bounds host int32 [G+1],
 * non-decreasing from 0 with bounds[G] = N; group g is the sequences bounds[g] .. bounds[g+1]-1 (1..64 of them) and its
 * members attend only to each other.  G <= 64 (the table travels as a kernel argument); G = 0 launches nothing.  The
 * arithmetic of a unit is that of asw_inter_attention: groups of one size give the same bytes. */
int asw_inter_attention_groups(const float* qkv, const int32_t* bounds, int G, int L, int d, int nhead, float* ctx,
                               void* stream);

/* ------------------------------------------------------------------------
 * Individual kernels (unit-testable; the model above is built from these).
 * ---------------------------------------------------------------------- */

/* Shift + quantise + per-candidate mean / unbiased std of the mic-average
 * (JointModel/network.py:80-83 + network.py:28-35).  mean,std: [N] float32. */
int asw_shift_stats(const float* mix, int M, int T, const int32_t* offsets, int N,
                    int circular, float* mean, float* std, void* stream);

/* Shift + quantise + normalise + left zero-pad to T_pad + 1x1 preproc conv
 * (network.py:36-38,377-378,385).  w [C][M], b [C];
 * x0 [N][T_pad][C] channels-last, refn [N][refn_stride] (normalised padded mic 0; the
 * first T_pad entries of each row are written). */
int asw_shift_norm_preproc(const float* mix, int M, int T, int T_pad, const int32_t* offsets,
                           int N, int circular, const float* mean, const float* std,
                           const float* w, const float* b, int C, float* x0, float* refn,
                           long refn_stride, void* stream);

/* The two calls above over candidates of several mixtures: mix [K][M][T], candidate n reads mixture
 * mix_index[n] (int32 device [N], values in [0, K), not range-checked; NULL = mixture 0 for every candidate). */
int asw_shift_stats_multi(const float* mix, int M, int T, const int32_t* offsets, const int32_t* mix_index, int N,
                          int circular, float* mean, float* std, void* stream);
int asw_shift_norm_preproc_multi(const float* mix, int M, int T, int T_pad, const int32_t* offsets,
                                 const int32_t* mix_index, int N, int circular, const float* mean, const float* std,
                                 const float* w, const float* b, int C, float* x0, float* refn, long refn_stride,
                                 void* stream);

/* asw_shift_norm_preproc_multi without the 1x1 convolution, for the source-fed first residual pair
 * (asw_resstack_args.src_hi): the same shift, quantisation, normalisation and left pad, the same refn, and instead of
 * x0 the network input itself as u~ [N][T_pad][8] = (u_0 .. u_{M-1}, 0 .., 1) -- the last channel is 1 on every row and
 * carries the preproc bias -- already split into the two fp16 halves of the f16x3 operands (saturating at +-65504 like
 * every activation split): src_hi / src_lo, 16 bytes per row each.  M <= 7. */
int asw_shift_norm_src_multi(const float* mix, int M, int T, int T_pad, const int32_t* offsets,
                             const int32_t* mix_index, int N, int circular, const float* mean, const float* std,
                             void* src_hi, void* src_lo, float* refn, long refn_stride, void* stream);

/* Normalised input variant used by asw_spot_forward: x [B][M][t] -> x0, refn. */
int asw_pad_preproc(const float* x, int B, int M, int t, int T_pad, const float* w,
                    const float* b, int C, float* x0, float* refn, long refn_stride,
                    void* stream);

/* 1-D convolution / transposed convolution / linear layer as an implicit GEMM on the
 * f32 MFMA pipe with a fused epilogue.  Activations are channels-last.
 *   out[b][r][n] = epi( sum_{tap,c} A[b][(r*stride + tap*dil - pad)*a_row_stride + c]
 *                                    * Wt[n][tap*Cin + c] )
 * epi: +bias[n]; activation (relu: 0 none, 1 ReLU, 2 Swish x*sigmoid(x)); +resid; *mul; LayerNorm over n (ln_gamma!=NULL,
 * requires N in {64,128,256,512,1024}); group statistics partials (stats!=NULL).
 * Replaces nn.Conv1d / nn.ConvTranspose1d / nn.Linear + ReLU / residual / LayerNorm of
 * network.py:57-68,105-113,190-198 and the transformer linears.
 * Zero-initialise the block (memset / = {}) before filling it: every optional pointer is tested against NULL,
 * and the struct only ever grows at its end. */
typedef struct asw_convgemm_args {
  const float* A;         /* [B][a_batch_stride] */
  const float* A2;        /* optional tensor added to A while loading (skip connection) */
  const float* Wt;        /* [N][taps*Cin] */
  const float* bias;      /* [N] or NULL */
  const float* resid;     /* [B][M_out][N] or NULL */
  const float* mul;       /* [B][M_out][N] or NULL */
  const float* ln_gamma;  /* [N] or NULL */
  const float* ln_beta;   /* [N] */
  float* out;             /* [B][M_out][N] */
  float* stats;           /* [B][tiles_m*tiles_n][4] or NULL: (sum0,sumsq0,sum1,sumsq1) */
  int32_t B, M_out, N, Cin, taps, stride, dil, pad;
  int32_t a_row_stride;   /* floats between consecutive input rows (normally Cin) */
  int64_t a_batch_stride; /* floats between batch items of A */
  int64_t a_len;          /* valid floats per batch item (bounds for zero padding) */
  int32_t chan_mod;       /* stats: group = ((n % chan_mod) >= chan_mod/2) */
  int32_t relu;
  float ln_eps;
  /* precision 0: Wt is fp32 and the products run on the exact f32 MFMA.
   * precision 1 ("f16x3"): every fp32 operand x is split into two halves
   *   hi = fp16(x), lo = fp16(x - hi) and the product is hi*hi + hi*lo + lo*hi on the f16
   *   MFMA with fp32 accumulation (operands good to ~2^-21, 5.3x the f32 MFMA rate).
   *   Weights arrive pre-split: Wt_hi / Wt_lo are fp16 [N][taps*Cin] of (w * 2^w_shift);
   *   activations are split on the fly (saturated at +-65504).
   * precision 2 ("f16", optional, reduced precision): the same kernels with ONE MFMA per product, hi * hi on
   *   round-to-nearest halves (same weight arrays; the lo halves are ignored): ~2e-4 per layer, 47-48 dB
   *   end to end against the reference, 1.5x the f16x3 throughput.  Never the default.
   * precision 3: the kernels and the arithmetic of precision 1, for a GEMM whose output no split GEMM reads (every
   *   f16x3 site of the "f16x3_safe" model precision): the range guard of the plain epilogue counts non-finite
   *   outputs only (asw_f16x3_overflow_count).  asw_convgemm_f32 only. */
  int32_t precision;
  int32_t w_shift;
  const void* Wt_hi;
  const void* Wt_lo;
  /* Optional (precision 1): the same split weights in MFMA-fragment order (see
   * asw_pack_fragments_f16).  When given and the layer is a stride-1 "same" convolution
   * with C_in == N <= 512, a residual that is the input itself and a LayerNorm epilogue
   * (the reference's DilatedResidualLayer), the halo-staged kernel is used: each input row
   * is fetched and split once per workgroup instead of once per tap. */
  const void* Wf_hi;
  const void* Wf_lo;
  int32_t stats_stride;   /* set by the library: partial-statistics slots per batch item */
  /* Optional (precision >= 1, the halo-staged residual layer with C_in == N in {64, 128, 256, 512}, dilation 1,
   * i.e. the first layer of a block's residual stack): take the layer's input -- and residual -- from the
   * un-normalised output of the preceding transposed convolution instead of A, applying GroupNorm(2) + GLU
   * while the rows are staged (the arithmetic of asw_gn_glu, bit for bit), so that tensor is neither written
   * nor read back.  glu_raw [B][M_out][2N] (value half | gate half of every output row), glu_mr [B][4] =
   * (mean0, rstd0, mean1, rstd1) from asw_gn_finalize, glu_gamma / glu_beta [2N].  A is ignored. */
  const float* glu_raw;
  const float* glu_mr;
  const float* glu_gamma;
  const float* glu_beta;
  /* [B][M_out][N]: receives GLU(GroupNorm(glu_raw)), the layer's input, as a tensor (an encoder block's skip
   * connection).  Optional at N == 64; required at N = 128 / 256 / 512, where the layer also reads its residual
   * from it (each workgroup the rows it wrote itself). */
  float* glu_out;
} asw_convgemm_args;
/* Host helper: fp32 Wt[N][K] -> fragment-major fp16 hi/lo [K/16][N/32][64 lanes][8]:
 * lane l of fragment (ks, nt) holds Wt[nt*32 + (l&31)][ks*16 + 8*(l>>5) + j], j < 8, i.e.
 * exactly the B operand of v_mfma_f32_32x32x16_f16, so a wave fetches a fragment with one
 * coalesced 1 KiB load.  Pre-scaled by 2^w_shift like asw_split_weights_f16.  N % 32 == 0,
 * K % 16 == 0; hi/lo: N*K uint16 each (host). */
int asw_pack_fragments_f16(const float* Wt, int N, int K, uint16_t* hi, uint16_t* lo, int32_t* w_shift);
int asw_convgemm_f32(const asw_convgemm_args* args, void* stream);
/* The mask path of the spot / separation network in ONE launch (f16x3 arithmetic), replacing
 * reference_bypass -> ReLU, mask_encoder -> ReLU, their product and the output_decoder tap products
 * (SpeakerLocalization/network.py:327-349,397-405; SpeakerSeparation/network.py:385-416) without the
 * E-channel latents ever being written:
 *   taps[c][b][f][j] = sum_{e in column tile c} relu(enc(x)[b][f][e] + bias_e) * relu(byp(ref)[b][f][e] + byp_bias_e) * D[e][j]
 * `enc` describes the mask_encoder GEMM exactly as for asw_convgemm_f32 (A, Wf_hi / Wf_lo fragment-order
 * weights, w_shift, bias, B, M_out = frames, N = E, Cin, taps, stride, pad, a_*; out / mul / stats unused;
 * N % 256 == 0, Cin % 32 == 0).  Frame f of item b reads the bypass window
 * ref[b*ref_batch_stride + f*ref_hop + k], k < byp_k (zero beyond ref_len); byp_hi / byp_lo: bypass weights
 * [E][byp_k = 48] (taps beyond byp_taps zero) packed by asw_pack_fragments_f16 (shift byp_shift); dec_hi /
 * dec_lo: decoder weights Wt[64][E] (row j = tap j, rows >= dec_taps zero) packed likewise (dec_shift).
 * Output: N/256 partial tap tensors [N/256][B][M_out][64] (columns < dec_taps written) to be summed by
 * asw_overlap_add_parts. */
typedef struct asw_maskpath_args {
  asw_convgemm_args enc;
  const float* ref;
  int64_t ref_batch_stride;
  int64_t ref_len;
  int32_t ref_hop;
  int32_t byp_k;          /* padded bypass kernel length (48) */
  int32_t byp_taps;       /* true bypass kernel length (33), for the FLOP count only */
  int32_t byp_shift;
  const void* byp_hi;
  const void* byp_lo;
  const float* byp_bias;  /* [E] or NULL */
  const void* dec_hi;
  const void* dec_lo;
  int32_t dec_shift;
  int32_t dec_taps;       /* 33 */
  float* taps;            /* [N/256][B][M_out][64] */
} asw_maskpath_args;
int asw_mask_path_f16x3(const asw_maskpath_args* args, void* stream);
/* The same launch without the fp16 range limit (the mask path of the "f16x3_safe" model precision; enc.precision 1
 * only).  asw_mask_path_f16x3 splits the gated latent relu(..) * relu(..) to fp16 halves for the decoder
 * contraction, which saturates at +-65504.  Here every latent row (one frame, the 256 channels of a column tile)
 * is first multiplied by the power of two that brings its largest magnitude into [2^12, 2^13) -- up as well as
 * down -- and the frame's partial taps by the inverse afterwards; both steps are exact.  The result is what
 * asw_mask_path_f16x3 gives wherever that is in range (up to the rounding of the lo halves, which small rows no
 * longer lose to fp16 subnormals), the kernel is exactly homogeneous per frame (latent row * 2^k -> taps * 2^k, bit
 * for bit, short of fp32 overflow / underflow), and asw_f16x3_overflow_count counts non-finite latents only.  A row
 * whose largest magnitude is zero or an fp32 subnormal keeps scale 1.  Profile name "maskpath16ps<256,256,32>". */
int asw_mask_path_f16x3_scaled(const asw_maskpath_args* args, void* stream);
/* A stack of 1..3 consecutive 64-channel DilatedResidualLayers (DilatedResidualSequence,
 * sep/training/SpeakerLocalization/network.py:50-82; the separation network uses the same classes) in
 * ONE launch, f16x3 arithmetic: out_i = LayerNorm(ReLU(conv_{dil_i}(x_i) + bias_i) + x_i), x_{i+1} = out_i.
 * The workgroup stages the rows the whole stack needs once; the intermediate tensors live in LDS only
 * (halo recomputation: a tile of 256 rows of layer 0 yields 256 - 2 * sum_{i>0} dil_i (taps-1)/2 finished
 * rows, so the later layers' dilations must be small: the call fails when fewer than 128 would be left).
 * A single layer of dilation >= 7 runs on polyphase row sets.  Results agree with n_layers calls of
 * asw_convgemm_f32 to fp32 rounding (the residual is taken from the fp16 hi + lo image: 2^-22 relative).
 *   x / out [B][T][64] float32 (out must not alias x); layer[i]: weights Wt[64][taps*64] in fragment order
 *   (asw_pack_fragments_f16), their shift, conv bias, LayerNorm affine.  glu_raw (optional, instead of x):
 *   as asw_convgemm_args.glu_raw -- GroupNorm(2) + GLU applied while layer 0 stages its rows. */
typedef struct asw_reslayer_desc {
  const void* Wf_hi;
  const void* Wf_lo;
  const float* bias;
  const float* ln_gamma;
  const float* ln_beta;
  int32_t dil;
  int32_t w_shift;
} asw_reslayer_desc;
typedef struct asw_resstack_args {
  const float* x;
  float* out;
  int32_t B, T, C, taps, n_layers;
  int32_t precision;      /* 1 = f16x3, 2 = single-pass f16 */
  float ln_eps;
  asw_reslayer_desc layer[3];
  const float* glu_raw;
  const float* glu_mr;
  const float* glu_gamma;
  const float* glu_beta;
  float* glu_out;         /* optional with glu_raw: [B][T][64], receives GLU(GroupNorm(glu_raw)) -- the stack's input --
                             for a caller that needs it as a tensor as well (the encoder's skip connection) */
  /* Optional, instead of x (precision 1, n_layers == 2, layer 0 of dilation 1, taps <= 7): the stack's input is
   * x[t] = Wpre~ u~[t], a 1x1 convolution of the 8-channel source u~ = (u_0 .. u_6, 1) written by
   * asw_shift_norm_src_multi, and is never materialised.  src_hi / src_lo: [B][T][8] fp16 planes of u~;
   * layer[0].Wf_hi / Wf_lo / w_shift: the COMPOSED weight Wt[64][64], column tap*8 + j = sum_c Wc[n][c][tap] Wpre~[c][j]
   * (tap 7 zero), in fragment order; pre_hi / pre_lo / pre_shift: Wpre~ as Wt[64][16] (columns 8..15 zero), fragment
   * order.  Layer 0's bias and LayerNorm and all of layer 1 as above.  Launch name resstack64<2,4x2,src>. */
  const void* src_hi;
  const void* src_lo;
  const void* pre_hi;
  const void* pre_lo;
  int32_t pre_shift;
  /* Optional ("UpFeed", precision 1, not with src_hi): the stack is the last of a decoder block and the next block
   * upsamples 64 -> 64 channels with stride 2.  The last layer then applies that transposed convolution itself,
   * up_out[b][t][r*128 + n] = up_bias[r*128 + n] + sum_c Wt[r*128 + n][c] (stack(x)[b][t][c] + up_skip[b][t][c]),
   * from the registers that hold the finished LayerNorm rows, and the stack's own output is not written (out may be
   * NULL).  up_hi / up_lo / up_shift: Wt[256][64] (pack_conv_transpose layout) packed by asw_pack_up_feed_f16;
   * up_skip [B][T][64]; up_out [B][T][256], i.e. the raw rows [B][2T][128]; up_stats [B][tiles][4], tiles =
   * asw_resstack_tiles(...): per (item, row tile) the sum and the sum of squares of the value half (n < 64) and of
   * the gate half, every slot written, for asw_gn_finalize / asw_gn_glu with n_partials = tiles.  Deterministic (no
   * atomics).  Launch names end in ",up>", e.g. resstack64<1,4x2,poly1,up>. */
  const void* up_hi;
  const void* up_lo;
  int32_t up_shift;
  const float* up_bias;
  const float* up_skip;
  float* up_out;
  float* up_stats;
  /* The fused pair (n_layers == 2, not UpFeed) on more than one tile of rows runs in its carried-halo form: a
   * workgroup walks a run of consecutive row tiles of one item and hands the layer-0 rows two neighbouring tiles share
   * from tile to tile instead of computing them twice (same results, bit for bit).  Runs per item: 0 = chosen by the
   * library from B, T and the device's CU count; > 0 = this many (clamped to the tiles there are); < 0 = the
   * recomputed-halo tiling: every tile a run of its own, by the same kernel (also where nothing can be carried: one
   * tile of rows, or more shared rows than the registers hold).  Launch names of a carrying plan carry ",carry",
   * e.g. resstack64<2,4x2,carry,glu>, and with asw_profile_enable(3) the runs per item, "[B.. M.. d.. r<runs>]";
   * asw_profile_enable(2) shows the launch under the name of the recomputed-halo form, whose bits it computes. */
  int32_t runs_per_item;
} asw_resstack_args;
int asw_resstack64_f16x3(const asw_resstack_args* args, void* stream);
/* Host helper: the runs asw_resstack64_f16x3 cuts an item into for the fused pair of dilations dil[2] with these T, B,
 * taps and runs_per_item on a device of n_cu compute units.  Returns the runs per item (0: the launch does not take the
 * carried-halo form; negative asw_status on a bad argument) and, for the first max_runs of them, the first row and the
 * number of tiles of each run.  The first tile of a run delivers *head_rows rows, every later one *steady_rows; the
 * last tile of the last run ends at or after T. */
int asw_resstack_runs(int T, int B, int taps, const int32_t* dil, int runs_per_item, int n_cu, int32_t* head_rows,
                      int32_t* steady_rows, int32_t* run_start, int32_t* run_tiles, int max_runs);
/* Row tiles per batch item of the asw_resstack64_f16x3 launch with these T, taps, n_layers, dilations dil[n_layers] and
 * GroupNorm + GLU on load or not: the number of UpFeed statistics slots per item.  Negative asw_status on a bad argument. */
int asw_resstack_tiles(int T, int taps, int n_layers, const int32_t* dil, int glu);
/* UpFeed hands the LayerNorm rows to the MFMA as they sit in the accumulator registers: position k of a 16-channel
 * k-step holds channel asw_up_feed_kperm(k) of that step (k = 0..15; bits 2 and 3 of k exchanged).
 * asw_pack_up_feed_f16 applies that order to the columns of Wt[N][K] (K % 16 == 0, N % 32 == 0) and packs the result
 * with asw_pack_fragments_f16 (same split, same shift). */
int asw_up_feed_kperm(int k);
int asw_pack_up_feed_f16(const float* Wt, int N, int K, uint16_t* hi, uint16_t* lo, int32_t* w_shift);
/* Host helper: the weights of the source-fed form (asw_resstack_args.src_hi) from the torch-layout parameters, composed
 * in double: wc [64][64][taps] (the first layer's Conv1d weight), wpre [64][M] and bpre [64] (the 1x1 convolution in
 * front of it), M <= 7, taps <= 7 -> comp Wt[64][64] (column tap*8 + j; j == 7 multiplies the constant channel and
 * carries the bias; tap 7 zero) and pre16 Wt[64][16] = [wpre | 0 | bpre | 0 x 8], both to be packed with
 * asw_pack_fragments_f16. */
int asw_compose_source_weights(const float* wc, const float* wpre, const float* bpre, int M, int taps, float* comp,
                               float* pre16);
/* Host helper: split n fp32 weights into the fp16 hi/lo pair used by precision 1 with the
 * power-of-two pre-scale that keeps the lo parts out of the fp16 subnormal range; returns
 * the shift through *w_shift.  hi/lo: n uint16 each (host). */
int asw_split_weights_f16(const float* w, size_t n, uint16_t* hi, uint16_t* lo, int32_t* w_shift);
/* f16x3 range guard: activations are split to fp16 halves (saturating at +-65504) when a GEMM
 * stages them.  Normalised tensors are bounded; the un-normalised ones (outputs of epilogues
 * without LayerNorm / GroupNorm statistics: masked latent, feed-forward intermediate, attention
 * projections) are checked where they are produced.  Returns through *count how many threads
 * of f16x3 launches on the current device wrote a value beyond the fp16 range (or a NaN) since
 * the last reset; waits for the device.  Non-zero means a later GEMM clipped its input: rerun in
 * precision 0 or 3.  (In model precision 3 nothing un-normalised is split unscaled, and only non-finite values
 * count.)  The device must be the one the launches ran on. */
int asw_f16x3_overflow_count(int reset, uint32_t* count);
/* Number of stats partials per batch item the call above will write. */
int asw_convgemm_stats_tiles(int M_out, int N);
/* The residue-image A feed of the pipelined f16x3 tiles (convgemm16p, the mask path).  In a strided convolution
 * with taps > stride, tap j of frame f and tap j + stride of frame f - 1 are the same input row.  The rows
 * {(m0 + i) * stride - pad + r}, r = tap mod stride, of one BK-channel chunk c form ONE LDS image; it serves tap
 * r + q * stride of frame m0 + i at image row i + q.  The image is fetched, split and deposited once and all of its
 * taps' k-steps run before the next barrier.  Stage order: residue-major, channel chunk inner (stage = r * Cin/BK + c).
 * The weight packing is untouched: the first k-step of (tap, chunk c) is index (tap * Cin/BK + c) * (BK/16) of
 * asw_pack_fragments_f16, whatever the order of the visit.
 * asw_residue_schedule enumerates that schedule for a tile whose first frame is m0: *n_stages = stride * Cin/BK and up
 * to `cap` entries of `out` (may be NULL with cap 0), or *n_stages = 0 when the feed does not apply: it needs dil == 1,
 * stride >= 2, taps > stride, Cin % BK == 0, BK % 16 == 0 and no skip operand.  *max_shift (optional) receives
 * (taps - 1) / stride, the largest row shift; the kernels take the feed up to ASW_RESIDUE_MAX_SHIFT (their ring has
 * that many rows beyond BM per image) and ASW_NO_RESIDUE_FEED=1 in the environment keeps them on the chunk-per-tap
 * feed (A/B measurements). */
#define ASW_RESIDUE_MAX_TAPS 8
#define ASW_RESIDUE_MAX_SHIFT 2
typedef struct asw_residue_stage {
  int32_t residue;                        /* r: tap mod stride of every tap of this stage */
  int32_t chunk;                          /* c: channels [c * BK, (c + 1) * BK) */
  int32_t rows;                           /* image rows: BM + (taps - 1 - r) / stride */
  int32_t first_row;                      /* input row of image row 0: m0 * stride - pad + r (image row i: + i * stride) */
  int32_t ntaps;                          /* taps served by the image, in the order of the visit */
  int32_t tap[ASW_RESIDUE_MAX_TAPS];      /* r + q * stride */
  int32_t shift[ASW_RESIDUE_MAX_TAPS];    /* q: frame m0 + i reads image row i + q */
  int32_t kstep[ASW_RESIDUE_MAX_TAPS];    /* first of the tap's BK/16 consecutive k-step indices */
} asw_residue_stage;
int asw_residue_schedule(int taps, int stride, int dil, int pad, int Cin, int BK, int BM, int m0, int has_skip,
                         asw_residue_stage* out, int cap, int* n_stages, int* max_shift);

/* GroupNorm(2 groups) + GLU over channels-last raw [B][T][2C] using the partial
 * statistics written by asw_convgemm_f32 (network.py:107-113,194-197). */
int asw_gn_glu(const float* raw, const float* stats, int n_partials, const float* gamma,
               const float* beta, int B, int T, int C, float eps, float* out, void* stream);
/* The statistics half of asw_gn_glu alone: reduces the same partial sums the same way and writes
 * mr [B][4] = (mean0, rstd0, mean1, rstd1) (float32), for a consumer that normalises while it loads
 * (asw_convgemm_args.glu_raw). */
int asw_gn_finalize(const float* stats, int n_partials, int B, int T, int C, float eps, float* mr, void* stream);

/* Multi-head self-attention core: qkv [B][L][3*d] (in_proj output) -> ctx [B][L][d]
 * (softmax(QK^T/sqrt(hd))V per head); nn.MultiheadAttention inside
 * nn.TransformerEncoderLayer (network.py:254). */
int asw_attention(const float* qkv, int B, int L, int d, int nhead, float* ctx, void* stream);
/* The same with the arithmetic of the two products chosen like asw_convgemm_args.precision: 0 = exact f32 MFMA
 * (asw_attention), 1 / 2 = f16x3 split operands on the f16 MFMA (head_dim 128 and L <= 320; the softmax stays
 * fp32; other shapes run as precision 0). */
int asw_attention_prec(const float* qkv, int B, int L, int d, int nhead, int precision, float* ctx, void* stream);

/* output_decoder ConvTranspose1d overlap-add + trim + un-normalise
 * (network.py:346-349,400-405; JointModel/network.py:96).
 * D [B][F][ldd] (per-frame tap products); the transposed convolution has
 * (F-1)*hop + taps samples, of which [trim_left : -trim_right] and then the last t are
 * kept; out [B][t]. */
int asw_overlap_add_unnorm(const float* D, int B, int F, int ldd, int taps, int hop,
                           int t, int trim_left, int trim_right, float bias, const float* mean,
                           const float* std, float* out, void* stream);
/* Same with the tap products given as `nparts` partial tensors [nparts][B][F][ldd] that are added
 * first (asw_mask_path_f16x3 writes one per 256-channel column tile of the latent). */
int asw_overlap_add_parts(const float* D, int nparts, int B, int F, int ldd, int taps, int hop,
                          int t, int trim_left, int trim_right, float bias, const float* mean,
                          const float* std, float* out, void* stream);

/* Per-candidate energies: mean removal, power = sum x^2, power2 = max windowed RMS
 * (local_utils_3d.py:13-17,349-354).  out [B][2] float64.  T <= 4096 * 256 samples when T and window are
 * multiples of 4 and y is 16-byte aligned, T <= 4096 * 64 otherwise.  scratch is ignored (the prefix sums stay in
 * registers / LDS; the argument is kept for the ABI): pass NULL, nothing needs to be allocated for it. */
int asw_energies(const float* y, int B, int T, int window, double* scratch, double* out,
                 void* stream);

/* out = LayerNorm(x + resid) * gamma + beta over rows of N floats (N % 256 == 0, N <= 2048):
 * norm1 / norm2 of the post-norm nn.TransformerEncoderLayer
 * (sep/training/SpeakerLocalization/network.py:254) when the row is too wide to fuse into the
 * producing GEMM's tile.  out may alias x. */
int asw_add_layernorm(const float* x, const float* resid, const float* gamma, const float* beta,
                      int rows, int N, float eps, float* out, void* stream);

/* In-place mean removal of every row (sep/Mic_Array.py:291, local_utils_3d.py:350): the
 * stage loops centre each candidate output before comparing waveforms. */
int asw_center_rows(float* y, int B, int T, void* stream);

/* SI-SDR of every ordered pair (est=i, ref=j) of n waveforms (eval_utils.py:11-39;
 * call sites Mic_Array.py:353,432).  out [n][n] float64. */
int asw_pair_sisdr(const float* y, int n, int T, double* out, void* stream);

/* Segment-wise SI-SDR of every ordered pair (split_wise_sisdr, eval_utils.py:73-82; call site
 * Mic_Array.py:432-458): segments [n][kmax][2] int32 = the [start,end) voiced segments of
 * waveform i (split_wav), seg_count [n]; out [n][n][kmax] float64, entry (i,j,k) = SI-SDR of
 * est = y[i][seg k of i] against ref = y[j][same samples]; entries k >= seg_count[i] are left
 * untouched.  Segment bounds must lie in [0,T] (device arrays). */
int asw_segment_sisdr(const float* y, int n, int T, const int32_t* segments, const int32_t* seg_count,
                      int kmax, double* out, void* stream);

/* Voiced segments of n waveforms on the device (split_wav, eval_utils.py:43-70; call sites Mic_Array.py:399-500), as
 * hostdsp.voiced_segments_f64 states them and equal to that statement bit for bit: y [n][T] float32, any T >= 1 (a
 * row need not be 16-byte aligned).  The mean square of librosa's centred, zero-padded 1024 / 256 frames is formed in
 * float64 in one fixed order -- per 256-sample block 64 partial sums of 4 consecutive squares, a six-step butterfly
 * over them, a frame = its four blocks left to right, / 1024 -- and frame f of nfr = 1 + T/256 is voiced iff
 * max(1e-10, ms[f]) > thr * ref2, ref2 = max(1e-10, Q) when the peak max_f ms[f] < Q and max(1e-10, peak) otherwise.
 * thr = 10^(-top_db/10) and Q = 0.04 * 0.04 are the caller's doubles.  Maximal voiced runs [f0, f1) give the
 * intervals [min(256 f0, T), min(256 f1, T)); one shorter than 1000 samples is dropped, one longer than 4000 is cut
 * into len / 4000 pieces of 4000 of which the last takes the remainder.  segments int32 [n][kcap][2] receives the
 * [start, end) pairs of waveform i in ascending order and [0, 0] in every slot from counts[i] on (so every slot is
 * written), counts int32 [n]; kcap >= max(1, T / 1000) always suffices and is required.  ms [n][nfr] float64 receives
 * the frame values, or NULL.  workspace: asw_voiced_segments_workspace_bytes(n, T) bytes, 8-byte aligned (the block
 * sums, [n][ceil(T/256)] float64; 0 with the error message set for n outside 0..65535 or T < 1).  No atomics, no
 * device-side assert: two calls give identical bytes, and the result does not depend on what the outputs or the
 * workspace held.  With NaN or Inf samples the result is unspecified but every access stays in bounds.  Every refusal
 * (n < 0 or > 65535, T < 1, kcap too small, null pointer, short workspace) happens before the first launch; n = 0
 * succeeds and launches nothing.  The tables are what asw_segment_sisdr reads. */
size_t asw_voiced_segments_workspace_bytes(int n, int T);
int asw_voiced_segments(const float* y, int n, int T, double thr, double Q, int32_t* segments, int kcap,
                        int32_t* counts, double* ms, void* workspace, size_t workspace_bytes, void* stream);

/* The fine stage's per-coarse-patch clustering of N candidate outputs in G groups on the device (the thresholds and
 * the greedy SI-SDR loop of Mic_Array.py:283-383), as fine_cluster.fine_clusters_f64 states it and equal to that
 * statement bit for bit.  y [N][T] float32 (device), the mean-removed outputs, any T >= 1 (a row need not be 16-byte
 * aligned).  bounds_host int32 [G + 1] is a HOST array and is read before the call returns: group g = rows
 * bounds[g] .. bounds[g + 1], bounds[0] = 0, non-decreasing, bounds[G] = N; empty groups are allowed.  energies
 * float64 [N][2] = (power, power2), gate float64 [N], group_gate float64 [G] (device); min_trigger and ratio =
 * 10^(sim_db / 10) are the caller's doubles.
 *   Gram: for rows a, b of one group G[a][b] = sum_t double(y_a[t]) * double(y_b[t]) in one fixed order -- 256
 *   partial sums p[l] over t = l, l + 256, ... from 0.0; each 64-wide quarter reduced by p[:s] += p[s:2s], s = 32 .. 1;
 *   the four quarter sums as (w0 + w1) + (w2 + w3) -- which depends neither on the group size nor on the tile or the
 *   workgroup a pair falls in; G[a][b] and G[b][a] are the same bits.
 *   Group g is open unless it is empty or max power2 of the group < group_gate[g]; every candidate of a closed group
 *   gets label -1.  order int32 [N]: order[bounds[g] + r] = global row of the r-th candidate of group g by descending
 *   power, equal powers by ascending row (closed groups too).  Candidate k is skipped (label -1) iff power2[k] <
 *   gate[k] or power[k] < min_trigger; any other joins the first head h in creation order with
 *   sss > ratio * snn, sss = es * es / ss, snn = max(ee - sss, 0) + 1e-8 (ee = G[k][k], ss = G[h][h], es = G[k][h]) --
 *   label[k] = h, a global row -- or becomes a head, label[k] = k.  label int32 [N].
 * gram float64 [sum n_g^2] receives the block-diagonal Gram matrix, group g row-major n_g x n_g at element offset
 * sum_{h<g} n_h^2, or NULL.  workspace: asw_fine_clusters_workspace_bytes(bounds_host, G) bytes, 8-byte aligned (the
 * Gram matrix, the group / tile table of the launch and one head slot per candidate; 0 with the error message set
 * for bounds this call would refuse).  Two launches (group_gram, fine_cluster) and one small host-to-device copy of
 * the table; no atomics, no device-side assert, plain vector stores: two calls give identical bytes, every slot of
 * order and label is written, and the result does not depend on what the outputs or the workspace held.  With NaN
 * or Inf in y or energies the result is unspecified but every access stays in bounds.  Every refusal -- null pointer,
 * N < 0, T < 1, G outside 0..65535, bounds that do not start at 0, decrease or do not end at N, sum n_g^2 above 2^27
 * elements, a short or misaligned workspace -- happens on the host before the copy and the first launch; N = 0 or
 * G = 0 (with valid bounds) succeeds and launches nothing. */
size_t asw_fine_clusters_workspace_bytes(const int32_t* bounds_host, int G);
int asw_fine_clusters(const float* y, int N, int T, const int32_t* bounds_host, int G, const double* energies,
                      const double* gate, const double* group_gate, double min_trigger, double ratio, void* workspace,
                      size_t workspace_bytes, int32_t* order, int32_t* label, double* gram, void* stream);

/* The global clustering's decisions over n cluster heads on the device (the walk of Mic_Array.py:399-500), as
 * global_cluster.global_clusters_f64 states them and equal to that statement on every input: there is no arithmetic,
 * only comparisons of the float64 values below, a first-hit scan and a running maximum.  All arrays are device
 * arrays; the rows are in visiting order (descending power).  full float64 [n][n] = SI-SDR of est i against ref j
 * (asw_pair_sisdr); seg float64 [n][n][K], K >= 1 (asw_segment_sisdr); counts int32 [n], c_i = min(max(counts[i], 0),
 * K): only the slots k < c_i of row i are read, the others may hold anything; near uint8 [n][n], non-zero = the two
 * centres lie within the merge distance.
 *   win[i][j] = (any k < c_i: seg[i][j][k] > win_hi) and not (any k < c_i: seg[i][j][k] < win_lo);
 *   merge[i][j] = full[i][j] > sim_db or win[i][j] or near[i][j] != 0; a NaN compares false everywhere.
 *   Walking i = 0 .. n - 1 with the heads kept in creation order: c_i == 0 -> label[i] = -1; else some head h with
 *   merge[i][h] -> label[i] = the first such head in creation order; else, with at least one head, best[k] = the
 *   NaN-propagating maximum over ALL heads h of seg[i][h][k], k < c_i, and (any best[k] > best_hi) and not (any
 *   best[k] < best_lo) -> label[i] = -2; else label[i] = i and i joins the heads.  label int32 [n].
 * merge uint8 [n][n] receives the matrix (0 or 1), or NULL: it then lives in the workspace.  workspace:
 * asw_global_clusters_workspace_bytes(n) bytes, 8-byte aligned (one head slot per candidate and the merge matrix; 0
 * with the error message set for n outside 0..8192; 0 for n = 0 too, without an error).  Two launches (global_merge:
 * a wavefront per ordered pair; global_walk: one workgroup, serial in i); no atomics, no device-side assert, plain
 * vector stores: two calls give identical bytes, every slot of label and merge is written, and the result does not
 * depend on what the outputs or the workspace held.  Garbage in counts stays in bounds by the clamp.  Every refusal
 * -- n < 0 or n > 8192, K < 1, a null pointer other than merge, a short or misaligned workspace -- happens on the host
 * before the first launch; n = 0 succeeds and launches nothing, whatever the pointers are. */
size_t asw_global_clusters_workspace_bytes(int n);
int asw_global_clusters(const double* full, const double* seg, const int32_t* counts, const uint8_t* near, int n, int K,
                        double sim_db, double win_hi, double win_lo, double best_hi, double best_lo, void* workspace,
                        size_t workspace_bytes, int32_t* label, uint8_t* merge_or_null, void* stream);

/* The coarse stage's decision over the N cubes of a lattice on the device (binary_search_baseline,
 * local_utils_3d.py:339-388, with the survivors mask of Prone_method="DENSE_NMS"), as search.coarse_select_f64 states
 * it and equal to that statement in every output byte.  All arrays are device arrays.  energies float64 [N][2] as
 * asw_spot_shift_and_sep writes it: only column 1, power_win, is read, in place; dis1 float64 [N] = 1 + the distance
 * of the cube's centre to microphone 0; best int32 [N] from asw_lattice_nms, or NULL: cube i is alive when best[i] ==
 * i (NULL: every cube is).
 *   wd[i] = power_win[i] * dis1[i], one IEEE multiply.  max_wd = the largest wd that is not NaN (+0.0 when the largest
 *   is a zero and some wd is +0.0; the quiet NaN 0x7ff8000000000000 when there is none).  thr = thr1; with relative != 0
 *   and a max_wd that is not NaN, t = rel * max_wd and thr = t < thr1 ? t : thr1.
 *   Cube i passes when not (wd[i] < thr) and it is alive -- a NaN passes.  The cubes that pass are ordered by descending
 *   power_win, equal values (-0.0 equals 0.0) by ascending index, every NaN after every number, by index.
 * kept int32 [cap]: the first min(cap, n_pass) of that order, the other slots -1.  counts int32 [2] = (n_pass, the number
 * of cubes, alive or not, whose power_win is not finite).  thr float64 [2] = (thr, max_wd).
 * workspace: asw_coarse_select_workspace_bytes(N, cap) bytes, 8-byte aligned (0 with the error message set for N outside
 * 0..2^24 or cap outside 1..64).  The cubes are cut into slices of 1024.  Launches: coarse_max (only with relative != 0;
 * at most 256 workgroups, each writes the maximum of its share of the cubes), coarse_slices (a workgroup per slice: its counts, its
 * maximum and its ordered best cap cubes, found by counting each cube's predecessors in LDS) and coarse_merge (one
 * workgroup folds the slices' lists, 1024 entries at a time, into the best cap and sums the counts).  Workgroups hand
 * nothing to each other inside a launch; no atomics, no device-side assert, plain vector stores: two calls give
 * identical bytes, every output slot is written, every workspace slot that is read is written first, and the result does
 * not depend on what the outputs or the workspace held.  A value of best outside 0..N-1 only makes its cube not alive.
 * Every refusal -- N < 0 or N > 2^24, cap outside 1..64, a null pointer other than best, a short or misaligned
 * workspace -- happens on the host before the first launch; N = 0 succeeds, launches no kernel and fills the outputs
 * (-1, (0, 0), (thr1, NaN)) by memsets on the stream. */
size_t asw_coarse_select_workspace_bytes(int N, int cap);
int asw_coarse_select(const double* energies, const double* dis1, const int32_t* best_or_null, int N, double thr1,
                      int relative, double rel, int cap, void* workspace, size_t workspace_bytes, int32_t* kept,
                      int32_t* counts, double* thr, void* stream);

/* BSS-eval SDR of a ragged batch of K samples on the device, as evalkit.bss_eval_sdr states it (the BSS-eval v3
 * "mtifilt" decomposition of evalkit._project; a restatement of the published algorithm, so parity with mir_eval stays
 * unpinned: what is pinned is this entry point against the repository's own float64 statement).  ref float32 [N][T]
 * (device), N = sum counts, the references of item after item with no padding; est float32 [R][N][T] (device), R
 * estimate sets, est[r][n] goes with ref[n]; counts_host int32 [K] is a HOST array read before the call returns.  For
 * item k with S = counts[k] references at rows n0 .. n0 + S, sdr[r][n0 + j] is what
 * evalkit.bss_eval_sdr(ref_k, est_k[r], flen)[j] returns.  The float32 inputs are widened exactly; everything after
 * is float64.  sdr float64 [R][N], status int32 [K] (device).
 *   Correlations, directly and in a fixed order: c(i, b, p) = sum_t ref_i[t - p] b[t], p = 0 .. flen - 1, for every
 *   reference i and every row b (reference or estimate) of the item; T is cut into chunks of 1024, a workgroup sums a
 *   run of whole chunks in order (at most 8 runs), a second launch folds the runs left to right.
 *   Systems: per item the (S flen)^2 block-Toeplitz Gram matrix G[(i,a)][(j,b)] = sum_u ref_i[u-a] ref_j[u-b] (only when
 *   S > 1) and the S single-reference flen^2 Toeplitz matrices, dense, lower triangle in use; all systems of the call
 *   form one ragged list that one blocked Cholesky walks in 64-wide steps (diagonal tile in LDS, panel solve, trailing
 *   update: three launches per step over the whole list; a system that has run out of tiles exits at the top).
 *   A pivot that is not > 2^-40 times the row's original diagonal entry (NaN included) sets status[k] = 1 and is
 *   replaced by 1.0: nothing loops on data.  status[k] = 0 otherwise, also for an item with no reference.  The sdr
 *   rows of an item with status 1 are written but meaningless: the caller recomputes them (evalkit does, with the
 *   host statement, which itself leaves its LU route for lstsq on such input -- silent or duplicated references).
 *   Right-hand sides: R S for the full system, R for each single one; forward and backward substitution, a workgroup
 *   per right-hand side.  An item with S = 1 has no full system: its full projection IS the single one, so e_interf is
 *   exactly 0, as in the statement.
 *   Projections as direct flen-tap FIRs over T + flen - 1 samples, then s_true, e_spat, e_interf, e_artif and the two
 *   sums of squares exactly as the statement forms them, per chunk of 1024 samples with a fixed tree, the chunks folded
 *   left to right; sdr = 10 log10(num / den), +inf when den == 0.
 * workspace: asw_bss_eval_sdr_workspace_bytes(counts_host, K, R, T, flen) bytes, 8-byte aligned (the lists, the
 * correlations and their partial sums, the systems, the solutions, the energy partials; the systems dominate: 52 MB
 * for S = 5, flen = 512; 0 with the error message set for arguments this call would refuse).  One small
 * host-to-device copy of the lists and one memset of status on the stream.  No atomics, no cross-lane operations, no
 * device-side assert, plain vector stores; workgroups hand nothing to each other inside a launch: two calls give
 * identical bytes, every output slot is written, every workspace word that is read is written first, and the result
 * does not depend on what the outputs or the workspace held.  Every refusal -- a null pointer, K < 0, R < 1, flen
 * outside 1..1024, T < flen (or T > 2^25), a count outside 0..16, an item with S flen > 8192, a short or misaligned
 * workspace -- happens on the host before the copy and the first launch; K = 0 succeeds and touches nothing, N = 0
 * only clears status. */
size_t asw_bss_eval_sdr_workspace_bytes(const int32_t* counts_host, int K, int R, int T, int flen);
int asw_bss_eval_sdr(const float* ref, const float* est, const int32_t* counts_host, int K, int R, int T, int flen,
                     double* sdr, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Full BSS-eval of a ragged batch on the device: SDR, SIR and SAR as evalkit.bss_eval_sources / evalkit.bss_eval_matrices
 * state them (the same restatement of BSS-eval v3, so parity with mir_eval stays unpinned here too).  asw_bss_eval_sdr
 * above is this call with all_pairs = 0 and sir = sar = null; inputs, limits, the packed ragged layout, status, the
 * correlation, Gram, Cholesky and solve steps and every guarantee stated there hold here unchanged.  With u = s_true +
 * e_spat, e_i = e_interf and e_a = e_artif of the decomposition:
 *   sdr = 10 log10(sum u^2 / sum (e_i + e_a)^2), sir = 10 log10(sum u^2 / sum e_i^2),
 *   sar = 10 log10(sum (u + e_i)^2 / sum e_a^2), each +inf when its denominator is exactly 0 (an item with S = 1 has
 *   e_i exactly 0, so its sir is +inf).
 * all_pairs = 0: estimate j of a set goes against reference j; sdr, sir, sar float64 [R][N] (device), as sdr above.
 * all_pairs = 1: every estimate against every reference; the outputs are [R][Q], Q = sum_k S_k^2; item k owns columns
 *   q0_k = sum_{k' < k} S_k'^2 onward and entry [r][q0_k + e S_k + j] is estimate e of set r against reference j (a
 *   row-major [S_k][S_k] matrix per set and item, what evalkit.bss_eval_matrices(ref_k, est_k[r], flen) returns).
 *   The single-reference right-hand side of (e, j) is c(j, est_e, .), which the correlations hold already: R S_k^2
 *   single solves instead of R S_k, the R S_k full solves unchanged, R S_k^2 rows in the projection, each of which
 *   forms the full projection of its estimate again.  x grows by R S_k (S_k - 1) flen doubles per item.
 * sir and sar may both be null (only the SDR is produced: two sums per row and chunk, the kernels of asw_bss_eval_sdr),
 * but not one alone.  With both, the projection sums five squares through the same fixed tree -- u^2, (e_i + e_a)^2,
 * e_i^2, (u + e_i)^2, e_a^2 -- the first two by the same expressions in the same order, so sdr holds the same bytes
 * either way.
 * workspace: asw_bss_eval_sources_workspace_bytes(counts_host, K, R, T, flen, all_pairs) bytes, 8-byte aligned: the
 * size with sir and sar wanted (five energy partials per row and chunk); a call without them needs 24 bytes per row and
 * chunk less and accepts this size too (all_pairs = 0: exactly asw_bss_eval_sdr_workspace_bytes).  0 with the error
 * message set for arguments the call would refuse.  Refusals beyond those of asw_bss_eval_sdr, on the host before the
 * copy and the first launch: all_pairs other than 0 or 1; one of sir, sar null alone. */
size_t asw_bss_eval_sources_workspace_bytes(const int32_t* counts_host, int K, int R, int T, int flen, int all_pairs);
int asw_bss_eval_sources(const float* ref, const float* est, const int32_t* counts_host, int K, int R, int T, int flen,
                         int all_pairs, double* sdr, double* sir, double* sar, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);

/* SI-SDR of every (estimate, reference) pair of a ragged batch of K samples on the device, as hostdsp.si_sdr states it
 * in float64: for estimate e and reference r of one item, rr = sum r^2, a = sum r e / rr, te = sum (a r)^2,
 * ne = sum (e - a r)^2, value 10 log10(te / (ne + 1e-8)).  est float32 [NE][T] and ref float32 [NR][T] (device): item k
 * owns the next P_k = est_counts_host[k] rows of est and the next S_k = ref_counts_host[k] rows of ref, with no padding;
 * both count arrays are HOST arrays read before the call returns.  out float64 (device), packed with no padding: item k
 * is a row-major [P_k][S_k] block at offset sum_{j<k} P_j S_j, entry (p, s) = si_sdr(est_p, ref_s).  status int32 [K]
 * (device).  The float32 inputs are widened exactly; everything after is float64.
 *   Two passes, as the statement: pass A sums rr and sum r e (a float32 x float32 product is exact in double), pass B
 *   sums te and ne element by element from a r and e - a r with a known -- ne is NOT formed as sum e^2 - (sum r e)^2 / rr,
 *   which loses the value from about 57 dB up.  The file is compiled without floating-point contraction: a r is rounded
 *   before it is subtracted, as numpy rounds it, so only the order of the sums differs from the statement.
 *   T is cut into chunks of 512; a workgroup owns a tile of 8 estimate rows x 8 reference rows of one item and a run of
 *   whole chunks (at most 8 runs), stages every row of the tile once per chunk and pass in LDS (a row beyond the item's
 *   own and samples beyond T as zeros, never read from memory), sums its run in order -- a lane per pair, each of the
 *   four waves a fixed quarter of every chunk, the quarters folded in order -- and a second launch folds the runs left
 *   to right.
 *   status[k] = 1 when some pair of item k has rr == 0, te == 0 or a value that is not finite (a silent reference
 *   divides by zero in the statement, an all-zero estimate raises in its log10): the caller recomputes the item with
 *   the host statement (evalkit.cross_sisdr_batch does); its out block is written but meaningless.  status[k] = 0
 *   otherwise, also for an item with P_k = 0 or S_k = 0, which rides along and writes nothing else.
 * workspace: asw_cross_sisdr_workspace_bytes(est_counts_host, ref_counts_host, K, T) bytes, 8-byte aligned (the
 * lists, (a, rr) per pair, the partial sums, a flag per tile; 0 with the error message set for arguments this call
 * would refuse).  One small host-to-device copy of the lists on the stream.  No atomics, no cross-lane operations, no
 * device-side assert, plain vector stores, one writer per address; workgroups hand nothing to each other inside a
 * launch: two calls give identical bytes, every output slot is written, every workspace word that is read is written
 * first, and the result does not depend on what out, status or the workspace held.  Every refusal -- a null pointer,
 * K < 0 or K > 65535, T < 1 or T > 2^25, a negative count, P_k > 4096 or S_k > 64, a short or misaligned workspace --
 * happens on the host before the copy and the first launch; K = 0 succeeds and touches nothing. */
size_t asw_cross_sisdr_workspace_bytes(const int32_t* est_counts_host, const int32_t* ref_counts_host, int K, int T);
int asw_cross_sisdr(const float* est, const float* ref, const int32_t* est_counts_host, const int32_t* ref_counts_host,
                    int K, int T, double* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* HOST function (no GPU): breadth-first subdivision of one coarse hypercube into the fine
 * candidate hypercubes -- search_area / binary_area_divide_width
 * (sep/helpers/local_utils_3d.py:212-335) with Patch.check_out / hyperbola_sample
 * (sep/Traditional_SP/Patch_3D.py:40-47,69-87).  points [3][n_pts] float64 (the coarse patch's
 * area_points), mic [M][3]; offset/width [M-1] are IN/OUT (check_out mutates the caller's
 * patch, as the reference does); ub [M-1] physical TDoA bounds or NULL.  Results are
 * malloc'ed: child_offset/child_width [n_children][M-1], child_count [n_children] and the
 * concatenated point indices child_index; release each with asw_free. */
int asw_search_area(const double* points, int n_pts, const double* mic, int M, double* offset,
                    double* width, const double* ub, double sound_speed, double fs, int* n_children,
                    double** child_offset, double** child_width, int** child_count, int** child_index);
void asw_free(void* p);

/* HOST function (no GPU): flat indices ((y*nx + x)*nz + z), in scan order, of the points of the
 * sub-box [y0,y1) x [x0,x1) x all z of a TDoA lookup table offsets[ny][nx][nz][P] (float64)
 * whose every pair offset lies in [lo[p], hi[p]] -- hyperbola_offset / hyperbola_area_sample
 * (sep/Traditional_SP/SRP_Prunning.py:19-61). */
int asw_cube_select(const double* offsets, int ny, int nx, int nz, int P, int y0, int y1, int x0, int x1,
                    const double* lo, const double* hi, int32_t* out_idx, int64_t cap, int64_t* count);
/* The same scan over a pair-major table planes[P][ny][nx][nz] (8 bytes streamed per point instead of 8 P: the
 * first pair rejects almost every point); identical comparisons, order and result. */
int asw_cube_select_planes(const double* planes, int ny, int nx, int nz, int P, int y0, int y1, int x0, int x1,
                    const double* lo, const double* hi, int32_t* out_idx, int64_t cap, int64_t* count);

/* SRP-PHAT pruning map (sep/Traditional_SP/SRP_Prunning.py:387-434), two stages.
 *
 * asw_srp_cross_spectra: for each of n_windows analysis windows (start w*step, length
 * `window`): STFT restricted to `nbins` bins (rectangular window, hop `hop`, :404-409) as
 * a DFT-GEMM against `twiddle` [2*nb_pad][nfft] (row k: cos(2 pi (bin0+k) n / nfft),
 * row nb_pad+k: -sin(...)), PHAT normalisation X/max(|X|,tol) (:414-416), frame-averaged
 * cross-spectrum of the P = M(M-1)/2 pairs (pair_i < pair_j, :421-426).
 *   mix [M][T]; xf_scratch [M][frames][2*nb_pad]; cc [n_windows][nbins][P][2] (re,im).
 *
 * asw_srp_map: out[g] = max(0, max_w (1/(nbins*P)) sum_{k,p} Re(cc[w][k][p] *
 * exp(+j omega[k] (tau[g][pair_i[p]] - tau[g][pair_j[p]])))) (:428-430; the map starts
 * from zeros, :248-256).  tau [G][M] float64 seconds (mic z ignored by the caller,
 * :368-381); omega [nbins] float64 rad/s; part_scratch [8][8][G] float32; out [G]. */
int asw_srp_frames(int window, int nfft, int hop);
int asw_srp_cross_spectra(const float* mix, int M, int T, int window, int step, int n_windows,
                          int nfft, int hop, int nbins, int nb_pad, float tol,
                          const float* twiddle, const int32_t* pair_i, const int32_t* pair_j,
                          int P, float* xf_scratch, float* cc, void* stream);
int asw_srp_map(const float* cc, int n_windows, int nbins, int P, const double* tau, int G, int M,
                const double* omega, const int32_t* pair_i, const int32_t* pair_j,
                float* part_scratch, float* out, void* stream);

/* MUSIC / TOPS pruning maps (sep/Traditional_SP/SRP_Prunning.py:436-497, MUSIC_block.py,
 * TOPS_block.py), four stages.  All take 4 <= M <= 16 microphones (3 signal vectors).
 *
 * asw_pruner_covariance: for each of n_windows windows (start w*step, length `window`) and
 * each bin k < nbins: X = the STFT bin bin0+k (rectangular, hop `hop`) as a direct DFT in
 * double; cov[w][k] = (1/frames) sum_f X_f X_f^H as a full Hermitian [M][M] complex double
 * matrix and magsum[w][k] = sum_m sum_f |X[m][k][f]| in double.
 *   mix [M][T] float; cov [n_windows][nbins][M][M][2]; magsum [n_windows][nbins].
 *
 * asw_hermitian_eigh: n Hermitian matrices a [n][M][M][2] (complex double; the Hermitian part
 * is used), 1 <= M <= 16, by cyclic complex Jacobi in double.  evals [n][M] ascending,
 * evecs [n][M][M][2] with eigenvector j in column j (numpy.linalg.eigh's layout).
 *
 * asw_music_map: out[g] = mean_w mean_k P[w][k][g] / max_g' P[w][k][g'], with
 * P = 1 / sum_{j < M-3} |e_j^H a|^2 over the noise columns of evecs [n_windows][nbins] (as
 * asw_hermitian_eigh writes them) and a_m = exp(+j omega[k] tau[g][m]).  tau [G][M] float64
 * seconds, omega [nbins] rad/s; p_scratch [n_windows][nbins][G] double;
 * max_scratch [n_windows][nbins] double; out [G] float.
 *
 * asw_tops_map: per window, max_bin[w] = first argmax_k magsum[w][k]; f0 = bin0 + max_bin;
 * out[g] = mean_w 1/s_min(D), D = [F0^H diag(conj phi_k) W_k] for k = 0 .. nbins-2, F0 the
 * 3 signal columns of bin max_bin, W_k the M-3 noise columns of bin k,
 * phi_k[m] = exp(j coef (k - f0) delta[g][m]) (k the raw row index, as the reference has it).
 * delta [G][M] float64 path differences; q_scratch double[n_windows][nbins-1][3][M-3][M][2];
 * max_bin int32[n_windows]; out [G] float. */
int asw_pruner_covariance(const float* mix, int M, int T, int window, int step, int n_windows,
                          int nfft, int hop, int bin0, int nbins, double* cov, double* magsum,
                          void* stream);
int asw_hermitian_eigh(const double* a, int n, int M, double* evals, double* evecs, void* stream);
int asw_music_map(const double* evecs, int n_windows, int nbins, int M, const double* tau, int G,
                  const double* omega, double* p_scratch, double* max_scratch, float* out,
                  void* stream);
int asw_tops_map(const double* evecs, const double* magsum, int n_windows, int nbins, int bin0,
                 int M, const double* delta, int G, double coef, double* q_scratch,
                 int32_t* max_bin, float* out, void* stream);

/* Geometry tables of the SRP-PHAT stage built on the device (csrc/geometry_kernels.hip; reference:
 * SRP_PHAT.__init__, Map_3D_TDoA, search_cluster, sep/Traditional_SP/SRP_Prunning.py:149-180,277-344,368-381).
 * All arithmetic is float64 in the expression order of the numpy statements of srp.py, contraction off; the
 * axis arrays are the host's numpy.arange results.  mics [M][3], 2 <= M <= 32, P = M - 1.
 *
 * asw_geom_lookup_planes: planes[p][y][x][z] = (|pt - mics[p+1]| - |pt - mics[0]|) / C * FS with
 * pt = (xs[x], ys[y], zs[z]) -- the pair-major table asw_cube_select_planes reads.
 *
 * asw_geom_voxel_map: per voxel v = (ix*Ly + iy)*Lz + iz of the SRP lattice the quantised TDoA vector
 * q[v][p] = rint(off / resolution) * resolution (round half to even; resolution a whole number) and
 * valid[v] = 0 inside the keep-out rectangle border = {x_lo, y_lo, x_hi, y_hi} (HOST pointer, open interval),
 * 1 elsewhere; dis_matrix[ix][iy] = sqrt((x - centre[0])^2 + (y - centre[1])^2) + 1e-8 (centre: HOST, 3 doubles).
 *
 * asw_geom_label: labels[v] = smallest C-order index of v's component among the 26-connected valid voxels with
 * an identical q vector, -1 for invalid voxels.  Min-label propagation with pointer jumping until a device flag
 * reports no change (synchronises the stream); *sweeps (HOST, may be NULL) = sweeps run.
 * adj_scratch uint32 [n], flag_scratch int32 [1].
 *
 * asw_geom_workspace_bytes: size of asw_geom_compact's workspace for an n-voxel lattice (negative: asw_status).
 *
 * asw_geom_compact: clusters ranked by their label (the order the reference's scan meets them in).  Every output
 * is allocated for the lattice size n = Lx*Ly*Lz by the caller; counts (HOST, 2 ints) receives G clusters and
 * V valid voxels (synchronises the stream).  power_index int32 [n] (0 on invalid voxels); valid_flat / valid_cid
 * int32 [V]: valid voxels ascending and their cluster; members int32 [V] with bounds int32 [G+1]: CSR member
 * lists, ascending voxel index within a cluster; offsets int32 [G][P]; centres [G][3]: sequential sum of the
 * member positions in that order / count; tau [G][M] = sqrt((dx^2 + dy^2) + z^2) / C (mic z ignored);
 * delta [G][M] = |c - centre| - |(c - centre) - (m - centre)|.
 *
 * asw_geom_lattice_workspace_bytes: size of asw_geom_lattice's workspace for a lookup grid of n_points points and P
 * pairs (negative: asw_status).
 *
 * asw_geom_lattice: the coarse TDoA lattice of a lookup grid (dense_grid.coarse_lattice).  planes [P][ny][nx][nz] as
 * asw_geom_lookup_planes writes them, point i = (iy*nx + ix)*nz + iz.  Points inside the keep-out rectangle border
 * (HOST, 4 doubles, open interval) are left out; the cell of a kept point on pair p is rint(planes[p][i] / width)
 * (round half to even) and a cube is a distinct cell vector.  cells int32 [N][P]: the cubes in lexicographic order
 * (pair 0 most significant, signed); members int32 [K] with bounds int32 [N+1]: CSR member lists, ascending point
 * index within a cube; centres [N][3]: sequential sum of the member positions in that order / count.  Every output
 * is allocated for the grid size n = ny*nx*nz by the caller (bounds: n + 1); counts (HOST, 2 ints) receives N cubes
 * and K kept points (synchronises the stream).  N = 0 (every point inside the keep-out) is a valid result: bounds[0]
 * = 0 and nothing else is written.  No atomics, stable radix passes: two builds are bit-identical.
 *
 * asw_lattice_nms_workspace_bytes: size of asw_lattice_nms's workspace for N cubes of P pairs, 0 <= N <= 2^24
 * (negative: asw_status; 0 for N = 0).
 *
 * asw_lattice_nms: non-maximum suppression over a lattice (dense_grid.lattice_local_maxima).  cells int32 [N][P] as
 * asw_geom_lattice writes them, scores float64 [N], both on the device; 1 <= P <= 31, radius >= 1.  Cube j is near
 * cube i when |cells[i][p] - cells[j][p]| <= radius on every pair (the differences are formed without overflow: any
 * int32 cells, any radius); a cube is near itself.  degree[i] = near cubes other than i; best[i] = the near cube with
 * the largest score, the lowest index among equal scores (-0.0 equals 0.0); i is a local maximum when best[i] == i.
 * RELIES ON column 0 of cells being non-decreasing, as in a table sorted with pair 0 most significant: the cubes that
 * can be near a block of rows are found by bisection in that column.  On a table that breaks the order, or with
 * non-finite scores, the result is unspecified but every access stays in bounds.  Integer and exact float64 compares,
 * partial results per split of the j range combined in a fixed order, no atomics: two calls are bit-identical, and
 * the result does not depend on what the workspace held.  Every refusal (null pointer, N < 0 or > 2^24, P outside
 * 1..31, radius < 1, short workspace) happens before the first launch; N = 0 succeeds and launches nothing. */
int asw_geom_lookup_planes(const double* ys, int ny, const double* xs, int nx, const double* zs, int nz,
                           const double* mics, int M, double C, double FS, double* planes, void* stream);
int asw_geom_voxel_map(const double* xs, int Lx, const double* ys, int Ly, const double* zs, int Lz,
                       const double* mics, int M, const double* border, const double* centre, double C,
                       double FS, double resolution, int32_t* q, uint8_t* valid, double* dis_matrix,
                       void* stream);
int asw_geom_label(const int32_t* q, const uint8_t* valid, int Lx, int Ly, int Lz, int P,
                   uint32_t* adj_scratch, int32_t* flag_scratch, int32_t* labels, int* sweeps, void* stream);
int64_t asw_geom_workspace_bytes(int n_voxels);
int asw_geom_compact(const int32_t* labels, const int32_t* q, const double* xs, int Lx, const double* ys, int Ly,
                     const double* zs, int Lz, const double* mics, int M, const double* centre, double C,
                     void* workspace, int64_t workspace_bytes, int32_t* power_index, int32_t* valid_flat,
                     int32_t* valid_cid, int32_t* members, int32_t* bounds, int32_t* offsets, double* centres,
                     double* tau, double* delta, int* counts, void* stream);
int64_t asw_geom_lattice_workspace_bytes(int n_points, int P);
int asw_geom_lattice(const double* planes, int P, int ny, int nx, int nz, const double* xs, const double* ys,
                     const double* zs, const double* border, double width, void* workspace,
                     int64_t workspace_bytes, int32_t* cells, int32_t* bounds, int32_t* members, double* centres,
                     int* counts, void* stream);
int64_t asw_lattice_nms_workspace_bytes(int N, int P);
int asw_lattice_nms(const int32_t* cells, int N, int P, const double* scores, int radius, void* workspace,
                    int64_t workspace_bytes, int32_t* best, int32_t* degree, void* stream);

/* ---- a recording of any length as overlapping blocks (longform.py) --------------------------
 * starts and row_of are HOST tables, read before the call returns; every other pointer is device memory.  Both calls
 * launch on `stream` and synchronise nothing; every refusal (null pointer, a shape outside M <= 65535 and
 * T, Ttot <= 2^30, a table entry out of range) happens before the first launch.
 *
 * asw_frame_blocks: out[k][m][j] = mix[m][starts[k] + j] for j < T, 0 where starts[k] + j >= Ttot (longform.frame_f64).
 * mix [M][Ttot], out [K][M][T]; 0 <= starts[k] < Ttot, in any order.
 *
 * asw_stitch_blocks: the normalised overlap-add of longform.stitch_f64,
 *   out[s][t] = sum_k taper[t - starts[k]] x_k[s][t - starts[k]] / sum_k taper[t - starts[k]]
 * over the blocks k with starts[k] <= t < starts[k] + T, in ascending k, accumulated in float64 and rounded once to
 * float32.  rows [N][T] float32; x_k[s] is row row_of[k*S + s] of it, zeros when that entry is -1 (the track is absent
 * from the block: its weight still counts in the denominator).  taper float64 [T], strictly positive (longform.taper;
 * not checked: a zero denominator gives a non-finite sample, never an access out of bounds).  out [S][Ttot]; each
 * sample is written once, by one thread, without atomics.  starts: starts[0] = 0, ascending, at most T apart (no gap)
 * and starts[K-1] + T >= Ttot; row_of entries in -1 .. N-1.  The tables travel as kernel arguments; tables beyond one
 * launch's share are cut into launches that each own a range of the output (a run of blocks and of tracks), for any S
 * and K; only starts of which more than 15 blocks cover one sample are refused. */
int asw_frame_blocks(const float* mix, int M, int Ttot, const int32_t* starts, int K, int T, float* out, void* stream);
int asw_stitch_blocks(const float* rows, int N, const double* taper, const int32_t* starts, const int32_t* row_of, int K,
                      int S, int T, int Ttot, float* out, void* stream);

/* ---- STFT, inverse STFT and the oracle mask baselines (oracle_masks.py) ---------------------
 * The transform pair of scipy.signal.stft(x, nperseg=2048) / scipy.signal.istft(Z) with every other argument at its
 * default, in float64: periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / 2048), hop 1024, 1025 one-sided bins, the
 * signal extended by 1024 zeros on each side and zero-padded to a whole hop, F = ceil(N / 1024) + 1 frames, every
 * spectrum divided by sum(w); backwards the one-sided inverse transform (the imaginary parts of bins 0 and 1024 do not
 * count) times w sum(w), overlap-added, divided by the overlap-added w^2 -- a table of 1024 values, periodic in the hop,
 * as every kept sample lies in exactly two frames -- and trimmed by 1024 samples at both ends.  The statements are
 * oracle_masks.stft_f64 and istft_f64; only the order of the sums inside a transform differs from them.
 *   A workgroup owns one frame: the 2048 windowed samples as 1024 complex values, a 1024-point radix-2 Stockham
 *   transform between two LDS buffers (self-sorting), and a split pass into the 1025 bins; the inverse runs the three
 *   steps backwards.  Twiddles and windows come from a float64 table that the host builds once per device (one
 *   hipMalloc and one blocking copy of 57 KB at the first call on that device; never freed).  The overlap-add has one
 *   writer per output sample, which gathers its two frames: no atomics, two calls give identical bytes.
 * Every pointer is device memory unless it says HOST; calls launch on `stream` and synchronise nothing; every refusal
 * happens on the host before the first launch.  Lengths below 2048 are refused (scipy would shrink the window).
 *
 * asw_stft: x float32 [R][N] -> z complex128 [R][1025][F] (re, im interleaved; 16-byte aligned), F = ceil(N/1024) + 1.
 *   0 <= R <= 65535, 2048 <= N <= 2^25; R = 0 succeeds and touches nothing.
 * asw_istft: z complex128 [R][1025][F] -> out float64 [R][N], the first N samples of the inverse, 0 <= N <= 1024 (F - 1),
 *   F >= 2.  workspace: asw_istft_workspace_bytes(R, F) bytes, 16-byte aligned (the windowed time frames, 2048 doubles
 *   per row and frame, behind one small table that a host-to-device copy on the stream fills).
 *
 * asw_oracle_masks: the ideal ratio mask (kind ASW_ORACLE_IRM) or ideal binary mask (ASW_ORACLE_IBM) estimates of K
 * items in one launch sequence (oracle_masks.irm_f64 / ibm_f64 per item).  Item k is one mixture row, S_k =
 * counts_host[k] reference rows and a length N_k = lengths_host[k]; both lists are HOST arrays read before the call
 * returns.  mix float32 [K][stride], ref float32 [sum S_k][stride] with item k owning the next S_k rows, out float64
 * [sum S_k][stride] in the same row order: out row j of item k holds the N_k samples of the estimate for reference j,
 * then zeros up to the stride; samples of mix and ref beyond N_k are never read.  With X the STFT of the mixture and S_j
 * those of the references, eps = 2^-52:
 *   IRM  mask_j = |S_j|^alpha / (eps + sum_k |S_k|^alpha), the sum in reference order starting from eps;
 *   IBM  r_j = |S_j|^alpha / (eps + |X|^alpha), mask_j = 1 where r_j >= theta, else 0;
 *   the estimate is the inverse STFT of X mask_j.  alpha == 1 takes |.| as it is, any other alpha goes through pow.
 *   First launch, a workgroup per (frame, item): it transforms the mixture's frame and keeps the spectrum in LDS, for
 *   the IRM transforms every reference once to sum the denominator, then transforms reference after reference (again),
 *   forms the mask, and inverse-transforms X mask_j; the windowed time frames go to the workspace, no spectrum does.
 *   Second launch: the overlap-add, normalisation and trim, one thread per output sample.
 * workspace: asw_oracle_masks_workspace_bytes(counts_host, lengths_host, K) bytes, 16-byte aligned; a multiple of 8; 0
 * with the error message set for arguments this call would refuse.  Refused: a null pointer with work to do, K < 0 or
 * K > 65535, S_k < 0 or S_k > 64, N_k < 2048 or N_k > 2^25 or N_k > stride, a kind that is neither, alpha or theta not
 * a number, a short or misaligned workspace.  K = 0 succeeds and touches nothing; an item with S_k = 0 rides along. */
#define ASW_ORACLE_IRM 0
#define ASW_ORACLE_IBM 1
int asw_stft(const float* x, int R, int N, double* z, void* stream);
size_t asw_istft_workspace_bytes(int R, int F);
int asw_istft(const double* z, int R, int F, int N, double* out, void* workspace, size_t workspace_bytes, void* stream);
size_t asw_oracle_masks_workspace_bytes(const int32_t* counts_host, const int32_t* lengths_host, int K);
int asw_oracle_masks(const float* mix, const float* ref, const int32_t* counts_host, const int32_t* lengths_host, int K,
                     int stride, int kind, double alpha, double theta, double* out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- Room simulator: image-source impulse responses and their convolution (roomsim.py) --------
 * The shoebox simulation of the dataset generator in float64, many scenes per call.  Scene k is an axis-aligned box
 * rooms[k] = (Lx, Ly, Lz) with one corner at the origin, one energy absorption a_k on all six walls (amplitude
 * reflection r = sqrt(1 - a)), an image order N_k and S_k = counts[k] sources; the sources of all scenes are packed in
 * scene order, every scene has M microphones.  The statements are roomsim.rir_f64 and roomsim.convolve_f64.
 *
 * asw_room_rir: rir float64 [sum S_k][M][length] (device), every sample written once.  Every other array is a HOST
 *   array read before the call returns: rooms [K][3], absorption [K], max_orders [K], src [sum S_k][3], mics [K][M][3],
 *   counts [K].  The images are the integer triples n with |nx| + |ny| + |nz| <= N in the order nx, ny, nz ascending;
 *   along an axis image n lies at n L + s for even n and (n + 1) L - s for odd n.  With d = sqrt(dx dx + dy dy + dz dz)
 *   summed in that order, t = d / 343 * fs, ip = floor(t) and f = t - ip, an image adds
 *   r^(|nx|+|ny|+|nz|) / (4 pi d) * w[j] * sinc(j - 40 - f) to sample ip + j for j = 0..80, w[j] = 0.5 - 0.5 cos(2 pi j /
 *   80); taps at or beyond `length` are dropped.  ip and f are those of the statement bit for bit (the file is compiled
 *   without fused multiply-adds); sin, the r^n table of the host's pow and the order of the sum are the library's own.
 *     A workgroup owns one (source, microphone) pair and 1024 samples; it walks the (nx, ny) columns, solves each for the
 *     nz that can reach its samples, decides by the exact delay and adds the hits in image order.  No atomics.
 *   workspace: asw_room_rir_workspace_bytes(K, M, sum S_k) bytes, 8-byte aligned (the host-built tables).
 *   Refused: K outside 0..65535, M outside 1..1024, S_k outside 0..64, more than 65535 sources, length outside 1..2^25,
 *   fs outside (0, 1e9], a side outside (0, 1e6], absorption outside (0, 1], an order outside 0..150, a source or
 *   microphone not strictly inside its room, a source at a microphone's position, a null pointer with work to do, a
 *   short or misaligned workspace.  K = 0 succeeds and touches nothing.
 *
 * asw_room_convolve: premix[s][m][t] = sum_k dry[s][t - k] rir[s][m][k] for t < T, and mix[k][m] the sum of the premix
 *   rows of scene k in source order.  dry float32 [sum S_k][T], rir float64 [sum S_k][M][length], premix float64
 *   [sum S_k][M][T], mix float64 [K][M][T], all device; counts HOST.  Uniformly partitioned overlap-save with hop 1024
 *   and frame 2048 on the transform of the STFT: one launch each transforms the frames of dry and the zero-padded
 *   1024-tap partitions of rir, a third accumulates X[s][b - p] H[s][m][p] over p ascending per (scene, microphone,
 *   block), inverts and keeps the second half.  A scene with S_k = 0 gets a zero mix.
 *   workspace: asw_room_convolve_workspace_bytes(counts, K, M, length, T) bytes, 16-byte aligned (the spectra: 16400
 *   bytes per source and block of T plus per source, microphone and partition of length); 0 with the error message set
 *   for arguments the call would refuse.  Refused: K outside 0..65535, M outside 1..1024, S_k outside 0..64, length or T
 *   outside 1..2^25, more than 65535 (source, microphone) pairs, a null pointer with work to do, a short or misaligned
 *   workspace. */
size_t asw_room_rir_workspace_bytes(int K, int M, int n_src);
int asw_room_rir(const double* rooms_host, const double* absorption_host, const int32_t* max_orders_host, const double* src_host,
                 const double* mics_host, const int32_t* counts_host, int K, int M, double fs, int length, double* rir,
                 void* workspace, size_t workspace_bytes, void* stream);
size_t asw_room_convolve_workspace_bytes(const int32_t* counts_host, int K, int M, int length, int T);
int asw_room_convolve(const float* dry, const double* rir, const int32_t* counts_host, int K, int M, int length, int T,
                      double* premix, double* mix, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Training batches: noise, rolled mixtures, loss terms (train_data.py) ------------------------
 * float64 arithmetic, no atomics, every sum in a fixed order: two calls give identical bytes.  The statements are
 * train_data.colored_noise_f64, train_batch_f64 and row_losses_f64.
 *
 * asw_colored_noise: out float64 [rows][T] (device), every sample written once.  Row r is the power-law noise
 *   irfft(s, n = T) / sigma of the reference's powerlaw_psd_gaussian (fmin = 0), its two arrays of normals drawn by
 *   Philox4x32-10 under the 64-bit key row_key[r] with the counter (bin, row_id[r], 0, 0): words 0:1 and 2:3 give two
 *   uniforms (2 m + 1) / 2^53, m the top 52 bits, and Box-Muller the pair of normals.  row_key and row_id are HOST arrays
 *   read before the call returns.  Any 2 <= T <= 524288: Bluestein's chirp transform over L = 1024 R >= 2 T - 1, the
 *   L-point transform a four-step (R-point column transforms, twiddles, 1024-point row transforms); rows 2p and 2p + 1
 *   share one complex transform as its real and imaginary part.  Rows are processed in passes of at most
 *   max_rows_per_pass (0: as many as fit 256 MiB of workspace; otherwise at least 2, odd values round down); the bytes do
 *   not depend on it.
 *   workspace: asw_colored_noise_workspace_bytes(rows, T, max_rows_per_pass) bytes, 16-byte aligned; 0 with the error
 *   message set for arguments the call would refuse.  Refused: rows outside 0..2^20, T outside 2..524288, exponent outside
 *   0..8, max_rows_per_pass negative or 1, a null pointer with work to do, a short or misaligned workspace.
 *
 * asw_train_batch: out [items][S_max * M][T], float32 or (out_f64 != 0) float64, device.  Row c = s M + m of item i is
 *   x + white_level[i] w + pink_level[i] pink[i][c][t] summed in float64 in that order and rounded once, where x is
 *   mix[item_mix[i]][m][(t - shifts[i][s][m]) mod T] for s < counts[i] and |shift| <= T and zero otherwise, and w is the
 *   first normal of the Philox block (t, c, 1, 0) under white_key[i].  A level of zero leaves its term out, so that with
 *   both zero the output is the rolled mixture bit for bit.  mix float32 [K][M][T] and pink float64 [items][S_max * M][T]
 *   (may be null when every pink level is zero) are device arrays; item_mix, shifts, counts, the levels and white_key are
 *   HOST arrays read before the call returns.
 *   workspace: asw_train_batch_workspace_bytes(items, S_max, M) bytes, 8-byte aligned.
 *   Refused: items or S_max * M beyond 65535, T outside 1..2^25, a count outside 0..S_max, an item_mix outside 0..K-1 on
 *   an item with talkers, a level that is not finite, a non-zero pink level without pink, a null pointer with work to do.
 *
 * asw_train_losses: out float64 [N][4] = (mean |e - g|, -SNR, -SI-SDR, max |g|) of every row of est, gt float32 [N][T]
 *   (device).  SNR and SI-SDR are those of asteroid's SingleSrcNegSDR: both rows zero-meaned, EPS = 1e-8 added to the
 *   denominator and inside the logarithm.  One workgroup per row, three passes: the means, the centred sums, the residual
 *   against the scaled target. */
size_t asw_colored_noise_workspace_bytes(int rows, int T, int max_rows_per_pass);
int asw_colored_noise(const int64_t* row_key_host, const int32_t* row_id_host, int rows, int T, double exponent, int max_rows_per_pass,
                      double* out, void* workspace, size_t workspace_bytes, void* stream);
size_t asw_train_batch_workspace_bytes(int items, int S_max, int M);
int asw_train_batch(const float* mix, int K, int M, int T, int items, int S_max, const int32_t* item_mix_host, const int32_t* shifts_host,
                    const int32_t* counts_host, const double* pink_level_host, const double* white_level_host,
                    const int64_t* white_key_host, const double* pink, void* out, int out_f64, void* workspace, size_t workspace_bytes,
                    void* stream);
int asw_train_losses(const float* est, const float* gt, int N, int T, double* out, void* stream);

/* Corpus voices on the device (voiceprep.py): the polyphase resampler and the silence trim that
 * the dataset generator applies to voice files, as voiceprep.resample_poly_f64 and voiceprep.trim_f64 state them and
 * equal to those statements bit for bit.  Both calls take a ragged batch: x float32 [x_len] (device) holds the rows packed
 * in any order, row r = x[row_offset[r] .. + row_len[r]); a padded [n][T_max] matrix is the table row_offset[r] = r T_max.
 * row_offset, row_len, win_begin and win_len are HOST arrays, validated and read before the call returns.  No atomics,
 * one writer per address, every output element written: two calls give identical bytes.
 *
 * asw_voice_resample: one call serves one ratio up/down (reduced by their gcd here).  h float64 [h_len] (device) is the
 *   filter table voiceprep.resample_filter(up, down): 2 half + 1 taps, half = 10 max(up, down) of the reduced ratio,
 *   scaled by up; one tap 1.0 for the ratio 1/1, which makes the call a windowed copy.  With n_out = ceil(row_len up /
 *   down) and m = n down + half, y[n] = sum_j h[m % up + j up] x[m / up - j] over ascending j while the tap index stays
 *   <= 2 half, terms outside the row left out, every product and sum rounded on its own.  out [n][T_out], float32 or
 *   (out_f64 != 0) float64, device: out[r][t] = y_r[win_begin[r] + t] for t < win_len[r] while that index is below
 *   n_out, else 0; the float32 value is the float64 value rounded once.  The same entry therefore serves the whole rows
 *   (win_begin 0, win_len n_out) and the cropped, zero-padded T samples a scene keeps.
 *   Limit: max(up, down) <= ASW_VOICE_MAX_RATIO after reduction -- the table (102,408 bytes then) is staged in the LDS of
 *   one workgroup; it covers 8 / 11.025 / 16 / 22.05 / 32 / 44.1 kHz to and from 16 / 48 kHz.
 *   workspace: asw_voice_resample_workspace_bytes(n) bytes, 8-byte aligned.
 *   Refused before any launch: n outside 0..65535, up or down < 1, a ratio beyond the limit, h_len that is not the
 *   ratio's, T_out outside 1..2^30, a row that leaves x, win_begin outside 0..2^40, win_len outside 0..T_out, a null
 *   pointer, a short workspace.  n = 0 succeeds and launches nothing.
 *
 * asw_voice_trim: librosa.effects.trim over centred, zero-padded frames of 2048 at hop 512, nfr = 1 + row_len / 512
 *   frames, without logarithms.  A 512-sample block sum is 64 partial sums of 8 consecutive squares, left to right, and
 *   a six-step butterfly; a frame is its four blocks left to right, / 2048.  Frame f is non-silent iff
 *   max(1e-10, ms[f]) > thr max(1e-10, max_f ms[f]); thr = 10^(-top_db / 10) is the caller's double.  bounds int32
 *   [n][2] = (512 first, min(row_len, 512 (last + 1))) over the non-silent frames ((0, 0) when there is none);
 *   stats float64 [n][2] = (max_f ms[f], the two-pass population variance of the kept span in the order of
 *   voiceprep.span_var_f64; 0 for an empty span).  row_len[r] <= max_len.
 *   workspace: asw_voice_trim_workspace_bytes(n, max_len) bytes, 8-byte aligned (the row table and the block sums).
 *   Refused before any launch: n outside 0..65535, max_len < 0, a row longer than max_len or one that leaves x, a
 *   threshold that is not a number, a null pointer, a short workspace.  With NaN or Inf samples the result is
 *   unspecified but every access stays in bounds. */
#define ASW_VOICE_MAX_RATIO 640
size_t asw_voice_resample_workspace_bytes(int n);
int asw_voice_resample(const float* x, int64_t x_len, const int64_t* row_offset_host, const int32_t* row_len_host, int n, int up,
                       int down, const double* h, int h_len, const int64_t* win_begin_host, const int32_t* win_len_host, int T_out,
                       void* out, int out_f64, void* workspace, size_t workspace_bytes, void* stream);
size_t asw_voice_trim_workspace_bytes(int n, int max_len);
int asw_voice_trim(const float* x, int64_t x_len, const int64_t* row_offset_host, const int32_t* row_len_host, int n, int max_len,
                   double thr, int32_t* bounds, double* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASW_HIP_H */
