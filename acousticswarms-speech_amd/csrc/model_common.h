// model_common.h -- host-side pieces shared by the two device-resident networks
// (spot_model.hip: sep/training/SpeakerLocalization/network.py; sep_model.hip:
// sep/training/SpeakerSeparation/network.py): device buffers, GEMM weights in both arithmetic
// forms, the dilated-residual stack and the linear-layer launch helper.
#pragma once
#include <cstdlib>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "asw_common.h"

namespace asw_model {

struct DevBuf {
  float* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  int upload(const std::vector<float>& h) {
    if (p) { (void)hipFree(p); p = nullptr; }
    n = h.size();
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return asw::set_error(ASW_ERR_NOMEM, "hipMalloc(%zu floats)", n);
    ASW_HIP(hipMemcpy(p, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return ASW_OK;
  }
};

// A GEMM weight in both arithmetic forms: fp32 (exact f32 MFMA) and the fp16 hi/lo split
// with its power-of-two pre-scale (f16x3 MFMA), see convgemm.hip.
struct WBuf {
  DevBuf f32;
  uint16_t* hi = nullptr;
  uint16_t* lo = nullptr;
  int32_t shift = 0;
  WBuf() = default;
  WBuf(const WBuf&) = delete;
  WBuf& operator=(const WBuf&) = delete;
  WBuf(WBuf&& o) noexcept : f32(std::move(o.f32)), hi(o.hi), lo(o.lo), shift(o.shift), fhi(o.fhi), flo(o.flo) {
    o.hi = o.lo = o.fhi = o.flo = nullptr;
  }
  ~WBuf() {
    if (hi) (void)hipFree(hi);
    if (lo) (void)hipFree(lo);
    if (fhi) (void)hipFree(fhi);
    if (flo) (void)hipFree(flo);
  }
  // GEMM weight Wt[N][K] in every form the kernels take: fp32, fp16 hi / lo row-major, and -- when the
  // shape allows (N % 32 == 0, K % 16 == 0) -- hi / lo in MFMA-fragment order for the kernels that
  // pull their B operand straight from global memory (residual layers, pipelined wide tiles)
  int upload_gemm(const std::vector<float>& h, int N, int K) {
    int rc = upload(h);
    if (rc) return rc;
    if (N % 32 == 0 && K % 16 == 0 && (size_t)N * K == h.size()) return upload_frags(h, N, K);
    return ASW_OK;
  }
  int upload(const std::vector<float>& h) {
    int rc = f32.upload(h);
    if (rc) return rc;
    std::vector<uint16_t> vh(h.size()), vl(h.size());
    if ((rc = asw_split_weights_f16(h.data(), h.size(), vh.data(), vl.data(), &shift))) return rc;
    if (hi) { (void)hipFree(hi); hi = nullptr; }
    if (lo) { (void)hipFree(lo); lo = nullptr; }
    if (hipMalloc(&hi, h.size() * 2) != hipSuccess || hipMalloc(&lo, h.size() * 2) != hipSuccess)
      return asw::set_error(ASW_ERR_NOMEM, "hipMalloc(%zu halves)", h.size());
    ASW_HIP(hipMemcpy(hi, vh.data(), h.size() * 2, hipMemcpyHostToDevice));
    ASW_HIP(hipMemcpy(lo, vl.data(), h.size() * 2, hipMemcpyHostToDevice));
    return ASW_OK;
  }
  // fragment-major copy for the halo-staged residual conv (Wt is [N][K])
  uint16_t* fhi = nullptr;
  uint16_t* flo = nullptr;
  int upload_frags(const std::vector<float>& h, int N, int K) {
    std::vector<uint16_t> vh(h.size()), vl(h.size());
    int32_t sh = 0;
    int rc = asw_pack_fragments_f16(h.data(), N, K, vh.data(), vl.data(), &sh);
    if (rc) return rc;
    if (sh != shift) return asw::set_error(ASW_ERR_STATE, "fragment pack: inconsistent weight shift");
    if (fhi) { (void)hipFree(fhi); fhi = nullptr; }
    if (flo) { (void)hipFree(flo); flo = nullptr; }
    if (hipMalloc(&fhi, h.size() * 2) != hipSuccess || hipMalloc(&flo, h.size() * 2) != hipSuccess)
      return asw::set_error(ASW_ERR_NOMEM, "hipMalloc(%zu halves)", h.size());
    ASW_HIP(hipMemcpy(fhi, vh.data(), h.size() * 2, hipMemcpyHostToDevice));
    ASW_HIP(hipMemcpy(flo, vl.data(), h.size() * 2, hipMemcpyHostToDevice));
    return ASW_OK;
  }
  // the K-permuted fragment copy alone, for the UpFeed of a residual stack (asw_resstack_args.up_hi): split and
  // power-of-two pre-scale as upload_gemm's
  int upload_up_feed(const std::vector<float>& h, int N, int K) {
    std::vector<uint16_t> vh(h.size()), vl(h.size());
    int rc = asw_pack_up_feed_f16(h.data(), N, K, vh.data(), vl.data(), &shift);
    if (rc) return rc;
    if (fhi) { (void)hipFree(fhi); fhi = nullptr; }
    if (flo) { (void)hipFree(flo); flo = nullptr; }
    if (hipMalloc(&fhi, h.size() * 2) != hipSuccess || hipMalloc(&flo, h.size() * 2) != hipSuccess)
      return asw::set_error(ASW_ERR_NOMEM, "hipMalloc(%zu halves)", h.size());
    ASW_HIP(hipMemcpy(fhi, vh.data(), h.size() * 2, hipMemcpyHostToDevice));
    ASW_HIP(hipMemcpy(flo, vl.data(), h.size() * 2, hipMemcpyHostToDevice));
    return ASW_OK;
  }
  void bind(asw_convgemm_args& a, int precision) const {
    a.Wt = f32.p; a.Wt_hi = hi; a.Wt_lo = lo; a.w_shift = shift; a.precision = precision;
    a.Wf_hi = fhi; a.Wf_lo = flo;
  }
};

struct ResLayer { WBuf wt; DevBuf bias, g, b; int dil = 1; };

// conv weight [N][Cin][K] -> Wt[N][tap*Cin + c] (optionally scaled per input channel)
inline std::vector<float> pack_conv(const std::vector<float>& w, int N, int Cin, int K, const float* in_gate) {
  std::vector<float> o((size_t)N * Cin * K);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < Cin; ++c)
      for (int k = 0; k < K; ++k)
        o[((size_t)n * K + k) * Cin + c] = w[((size_t)n * Cin + c) * K + k] * (in_gate ? in_gate[c] : 1.f);
  return o;
}


// DilatedResidualSequence weights (network.py:70-82 of either network): conv weights in GEMM
// layout (+ MFMA-fragment order for the halo-staged f16x3 kernel), bias, LayerNorm affine.
inline int pack_res_layers(const std::map<std::string, std::vector<float>>& raw, const std::string& p, int ch, int K,
                           int n_layers, int dil_factor, std::vector<ResLayer>& out) {
  out.clear();
  out.resize(n_layers);
  int dil = 1;
  for (int j = 0; j < n_layers; ++j) {
    const std::string q = p + ".res.seq." + std::to_string(j);
    int rc;
    {
      const std::vector<float> packed = pack_conv(raw.at(q + ".conv.weight"), ch, ch, K, nullptr);
      if ((rc = out[j].wt.upload(packed))) return rc;
      if (ch % 32 == 0 && (ch * K) % 16 == 0 && (rc = out[j].wt.upload_frags(packed, ch, ch * K))) return rc;
    }
    if ((rc = out[j].bias.upload(raw.at(q + ".conv.bias")))) return rc;
    if ((rc = out[j].g.upload(raw.at(q + ".norm.weight")))) return rc;
    if ((rc = out[j].b.upload(raw.at(q + ".norm.bias")))) return rc;
    out[j].dil = dil;
    dil *= dil_factor;
  }
  return ASW_OK;
}

// ---- workspace arena --------------------------------------------------------
struct Arena {
  char* base;
  size_t off = 0, cap;
  bool dry;
  Arena(char* b, size_t c, bool d) : base(b), cap(c), dry(d) {}
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};


// Input of a residual stack given as the un-normalised output of the preceding (transposed) convolution:
// the first layer applies GroupNorm + GLU while it stages its rows (asw_convgemm_args.glu_raw).
struct GluSrc { const float* raw; const float* mr; const float* gamma; const float* beta; float* side_out = nullptr; };

// f16 arithmetic, 64..512 channels, first layer of dilation 1 with fragment-order weights: the layers that can do it.
// Above 64 channels the layer needs GluSrc.side_out (it reads its residual from there).  ASW_GLU_ON_LOAD_MAX_C=64
// keeps the wider blocks on the separate asw_gn_glu pass (A/B measurements).
inline bool glu_on_load_ok(const std::vector<ResLayer>& res, int prec, int ch) {
  static const int max_c = getenv("ASW_GLU_ON_LOAD_MAX_C") ? atoi(getenv("ASW_GLU_ON_LOAD_MAX_C")) : 512;
  return prec >= 1 && (ch == 64 || ch == 128 || ch == 256 || ch == 512) && ch <= max_c && !res.empty() &&
         res[0].dil == 1 && res[0].wt.fhi && res[0].wt.flo;
}

// 64-channel stacks in f16x3 arithmetic run through asw_resstack64_f16x3 (resstack.hip): consecutive layers whose
// later dilations leave most of a 256-row tile (summed halo <= 64 rows per side) share ONE launch, the rest
// (dilation 49) run as single layers of the same kernel.  ASW_NO_RESSTACK=1 keeps the per-layer kernels
// of resconv.hip (A/B measurements).
inline bool resstack_ok(const std::vector<ResLayer>& res, int prec, int ch, int K) {
  static const bool off = getenv("ASW_NO_RESSTACK") != nullptr;
  if (off || prec < 1 || ch != 64 || K % 2 == 0 || K < 3 || K > 15) return false;
  for (const ResLayer& r : res)
    if (!r.wt.fhi || !r.wt.flo) return false;
  return true;
}

// how many layers from layer j on share one resstack launch
inline size_t resstack_fuse_count(const std::vector<ResLayer>& res, size_t j, int K) {
  static const bool nofuse = getenv("ASW_RESSTACK_NOFUSE") != nullptr;
  size_t n = 1;
  int halo = 0;
  while (!nofuse && j + n < res.size() && n < 3) {
    const int pad = res[j + n].dil * (K - 1) / 2;
    if (halo + pad > 64) break;
    halo += pad;
    ++n;
  }
  return n;
}

// Input of a residual stack given as the 8-channel source of the 1x1 convolution in front of it (asw_resstack_args.src_hi):
// the two fp16 planes, the composed layer-0 weight and the 1x1 weight that rebuilds the residual.
struct SrcFeed { const void* hi; const void* lo; const WBuf* comp; const WBuf* pre; };

// Output of a residual stack taken as the raw rows of the next decoder block's transposed convolution
// (asw_resstack_args.up_hi): the permuted-K weight, the bias, the skip tensor, the raw rows and their partial sums.
// `tiles` receives the number of partial sums per item.
struct UpFeed { const WBuf* w; const float* bias; const float* skip; float* out; float* stats; int tiles; };

// the last launch of a 64-channel stack that runs through asw_resstack64_f16x3: its first layer and its layer count
inline void resstack_last_launch(const std::vector<ResLayer>& res, int K, size_t& j0, size_t& n) {
  j0 = 0;
  n = resstack_fuse_count(res, 0, K);
  while (j0 + n < res.size()) { j0 += n; n = resstack_fuse_count(res, j0, K); }
}
inline int up_feed_tiles(const std::vector<ResLayer>& res, int K, int T, bool glu) {
  size_t j0, n;
  resstack_last_launch(res, K, j0, n);
  int32_t dil[3] = {1, 1, 1};
  for (size_t i = 0; i < n; ++i) dil[i] = res[j0 + i].dil;
  return asw_resstack_tiles(T, K, (int)n, dil, glu && j0 == 0);
}

// ---- the parts of a residual-stack launch description (asw_resstack_args), one helper per part
inline void bind_layer(asw_reslayer_desc& d, const ResLayer& r) {
  d.Wf_hi = r.wt.fhi; d.Wf_lo = r.wt.flo; d.w_shift = r.wt.shift;
  d.bias = r.bias.p; d.ln_gamma = r.g.p; d.ln_beta = r.b.p; d.dil = r.dil;
}
// GroupNorm + GLU on load: the same five fields in asw_resstack_args and asw_convgemm_args
template <typename Args>
inline void bind_glu(Args& a, const GluSrc& g) {
  a.glu_raw = g.raw; a.glu_mr = g.mr; a.glu_gamma = g.gamma; a.glu_beta = g.beta; a.glu_out = g.side_out;
}
// the source-fed form: no x, the composed weight in layer 0's place
inline void bind_src_feed(asw_resstack_args& a, const SrcFeed& f) {
  a.src_hi = f.hi; a.src_lo = f.lo;
  a.layer[0].Wf_hi = f.comp->fhi; a.layer[0].Wf_lo = f.comp->flo; a.layer[0].w_shift = f.comp->shift;
  a.pre_hi = f.pre->fhi; a.pre_lo = f.pre->flo; a.pre_shift = f.pre->shift;
}
// UpFeed: the rows go to the next block's transposed convolution; the stack's output is not written
inline void bind_up_feed(asw_resstack_args& a, const UpFeed& u) {
  a.out = nullptr;
  a.up_hi = u.w->fhi; a.up_lo = u.w->flo; a.up_shift = u.w->shift; a.up_bias = u.bias; a.up_skip = u.skip;
  a.up_out = u.out; a.up_stats = u.stats;
}

inline int run_res(const std::vector<ResLayer>& res, int prec, int B, int T, int ch, int K, float* x, float* p, float* q,
            float** final_out, hipStream_t s, const GluSrc* glu = nullptr, const SrcFeed* feed = nullptr, UpFeed* up = nullptr) {
  // ping-pong: layer 0 reads x (kept intact), later layers alternate p/q
  const float* in = glu ? glu->raw : x;
  float* outb = p;
  if (feed && !(resstack_ok(res, prec, ch, K) && prec == 1 && resstack_fuse_count(res, 0, K) == 2))
    return asw::set_error(ASW_ERR_STATE, "run_res: the source-fed form needs the fused f16x3 pair");
  if (up && !(resstack_ok(res, prec, ch, K) && prec == 1))
    return asw::set_error(ASW_ERR_STATE, "run_res: UpFeed needs the f16x3 stack kernel");
  if (resstack_ok(res, prec, ch, K)) {
    size_t j = 0;
    while (j < res.size()) {
      const size_t n = resstack_fuse_count(res, j, K);
      asw_resstack_args a = {};
      a.x = ((glu || feed) && j == 0) ? nullptr : in;
      a.out = outb;
      a.B = B; a.T = T; a.C = ch; a.taps = K; a.n_layers = (int)n; a.precision = prec; a.ln_eps = 1e-5f;
      for (size_t i = 0; i < n; ++i) bind_layer(a.layer[i], res[j + i]);
      if (glu && j == 0) bind_glu(a, *glu);
      if (feed && j == 0) bind_src_feed(a, *feed);
      if (up && j + n == res.size()) {
        // the last launch hands its rows to the next block's transposed convolution
        bind_up_feed(a, *up);
        up->tiles = up_feed_tiles(res, K, T, glu != nullptr);
        if (up->tiles < 0) return up->tiles;
        outb = nullptr;
      }
      int rc = asw_resstack64_f16x3(&a, s);
      if (rc) return rc;
      in = outb;
      outb = (outb == p) ? q : p;
      j += n;
    }
    *final_out = const_cast<float*>(in);
    return ASW_OK;
  }
  for (size_t j = 0; j < res.size(); ++j) {
    asw_convgemm_args a = {};
    a.A = in; res[j].wt.bind(a, prec); a.bias = res[j].bias.p; a.resid = in;
    if (glu && j == 0) bind_glu(a, *glu);
    a.ln_gamma = res[j].g.p; a.ln_beta = res[j].b.p; a.out = outb;
    a.B = B; a.M_out = T; a.N = ch; a.Cin = ch; a.taps = K; a.stride = 1; a.dil = res[j].dil;
    a.pad = (res[j].dil * (K - 1) + 1) / 2;
    a.a_row_stride = ch; a.a_batch_stride = (int64_t)T * ch; a.a_len = (int64_t)T * ch;
    a.relu = 1; a.ln_eps = 1e-5f;
    int rc = asw_convgemm_f32(&a, s);
    if (rc) return rc;
    in = outb;
    outb = (outb == p) ? q : p;
  }
  *final_out = const_cast<float*>(in);
  return ASW_OK;
}

inline int linear(const float* A, const WBuf& W, int prec, const float* bias, int rows, int N, int K, int relu, const float* resid,
           const float* g, const float* b, float* out, hipStream_t s) {
  asw_convgemm_args a = {};
  a.A = A; W.bind(a, prec); a.bias = bias; a.resid = resid; a.ln_gamma = g; a.ln_beta = b; a.out = out;
  a.B = 1; a.M_out = rows; a.N = N; a.Cin = K; a.taps = 1; a.stride = 1; a.dil = 1; a.pad = 0;
  a.a_row_stride = K; a.a_batch_stride = (int64_t)rows * K; a.a_len = (int64_t)rows * K;
  a.relu = relu; a.ln_eps = 1e-5f;
  if (g && N >= 1024 && N % 256 == 0 && N <= 2048) {
    // a LayerNorm-fused tile must hold the whole row: at d = 1024 that leaves 32 rows per
    // workgroup and every workgroup re-reads all of W (measured 75 TFLOP/s).  Run the GEMM on
    // the wide tile instead and normalise in one extra pass over the rows (240 TFLOP/s + 30 us).
    a.resid = nullptr; a.ln_gamma = nullptr; a.ln_beta = nullptr;
    int rc = asw_convgemm_f32(&a, s);
    if (rc) return rc;
    return asw_add_layernorm(out, resid, g, b, rows, N, 1e-5f, out, s);
  }
  return asw_convgemm_f32(&a, s);
}

// ConvTranspose1d weight w [Cin][N][S] / bias b [N] with kernel == stride as a plain GEMM whose output row t_in holds the
// S output frames t_in*S .. t_in*S+S-1 back to back: Wt[r*N + n][c], bias[r*N + n] (optionally scaled per output channel)
inline void pack_conv_transpose(const std::vector<float>& w, const std::vector<float>& b, int Cin, int N, int S,
                                const float* out_gate, std::vector<float>& wt, std::vector<float>& bb) {
  wt.assign((size_t)S * N * Cin, 0.f);
  bb.assign((size_t)S * N, 0.f);
  for (int r = 0; r < S; ++r)
    for (int n = 0; n < N; ++n) {
      bb[(size_t)r * N + n] = out_gate ? b[n] * out_gate[n] : b[n];
      for (int c = 0; c < Cin; ++c) {
        const float v = w[((size_t)c * N + n) * S + r];
        wt[((size_t)r * N + n) * Cin + c] = out_gate ? v * out_gate[n] : v;
      }
    }
}

// ---- the U-Net trunk of both networks ---------------------------------------------------------------------------------
// preproc output -> encoder blocks (residual stack, stride-k conv, GroupNorm + GLU) -> the network's own bottleneck ->
// decoder blocks (ConvTranspose as a GEMM with the skip added on load, GroupNorm + GLU, residual stack) -> mask path
// (reference_bypass, mask_encoder, output_decoder, overlap-add).  asw_spot and asw_sep derive from Trunk.

#define UP(buf, vec) if ((rc = (buf).upload(vec))) return rc

// The U-Net hyper-parameters that asw_spot_config and asw_sep_config both carry, under the same names.
struct TrunkCfg {
  int n_mics, kernel_size, depth, stride_list[8], channels, growth, encoder_channels, encoder_kernel_size,
      encoder_stride, residual_layers, residual_dilation_factor, ffw_dim;
  template <class Cfg>
  static TrunkCfg of(const Cfg& c) {
    TrunkCfg t = {c.n_mics, c.kernel_size, c.depth, {}, c.channels, c.growth, c.encoder_channels,
                  c.encoder_kernel_size, c.encoder_stride, c.residual_layers, c.residual_dilation_factor, c.ffw_dim};
    for (int i = 0; i < 8; ++i) t.stride_list[i] = c.stride_list[i];
    return t;
  }
};

// The trunk checks of asw_*_create that need no device.  `who` prefixes the message; `odd` is the network's wording of
// the odd-kernel message (the separation network's also covers its bottleneck kernel).
inline int check_trunk_config(const TrunkCfg& c, const char* who, const char* odd) {
  ASW_CHECK_ARG(c.depth >= 1 && c.depth <= 8, "%s: depth %d", who, c.depth);
  ASW_CHECK_ARG(c.n_mics >= 1 && c.n_mics <= 32, "%s: n_mics %d", who, c.n_mics);
  ASW_CHECK_ARG(c.channels % 64 == 0, "%s: channels=%d must be a multiple of 64 for the MFMA tiles", who, c.channels);
  ASW_CHECK_ARG(c.growth >= 1 && c.residual_layers >= 1, "%s: bad config", who);
  ASW_CHECK_ARG(c.kernel_size % 2 == 1, "%s: %s", who, odd);
  ASW_CHECK_ARG(c.encoder_channels % 128 == 0, "%s: encoder_channels must be a multiple of 128", who);
  ASW_CHECK_ARG(c.encoder_stride % 4 == 0 && c.encoder_kernel_size / 2 == c.encoder_stride && c.encoder_kernel_size <= 64,
                "%s: encoder kernel/stride %d/%d unsupported (the reference's trim [9:-8] assumes 33/16)", who,
                c.encoder_kernel_size, c.encoder_stride);
  ASW_CHECK_ARG(c.ffw_dim % 128 == 0, "%s: ffw_dim must be a multiple of 128", who);
  return ASW_OK;
}

struct EncBlock { std::vector<ResLayer> res; DevBuf bias, gn_g, gn_b; };
struct DecBlock { std::vector<ResLayer> res; DevBuf gn_g, gn_b; };
// The convolutions a window gate folds into (embed1, spot network.py:101,186): each encoder's down conv (gate per input
// channel) and each decoder's transposed conv (gate per output channel).  The spot network packs one set per window
// embedding, the separation network one without a gate.
// up_feed[j]: up_wt[j] with the K order of a residual stack's UpFeed, where block j can be fed that way (Trunk::up_feed_shape).
struct GatedConvs { std::vector<WBuf> down_wt, up_wt, up_feed; std::vector<DevBuf> up_bias; };
struct Tap { const float* p; size_t numel; };
using ParamList = std::vector<std::pair<std::string, size_t>>;

// The trunk's part of a workspace.  X[i] is the input of encoder block i (X[0] = preproc output).
struct TrunkPlan {
  int B, T, Tp, F, RL;                     // B: sequences in this batch
  std::vector<int> Tl;                     // length at level 0..depth
  float *mean, *stdv, *refn;
  uint16_t *src_hi = nullptr, *src_lo = nullptr;   // the 8-channel network input as fp16 planes (source-fed block 0)
  std::vector<float*> X, Pb, Qb, raw_dn, raw_up, st_dn, st_up, mr_dn, mr_up;
  float *Y, *D, *ywave;
};

struct Trunk {
  TrunkCfg tc;
  std::map<std::string, std::vector<float>> raw;   // state dict as set_param received it
  std::map<std::string, Tap> taps;                 // activations of the last batch
  bool finalized = false;
  int device = 0;                          // HIP device the weights and the workspace live on
  int precision = 0;                       // 0 = exact f32 MFMA, 1 = f16x3 split MFMA, 2 = single-pass f16
  bool exact_raw = false;                  // "f16x3_safe" (ABI value 3 = precision 1 + this flag), see site()
  bool fuse_mask = true;                   // f16x3: GroupNorm + GLU on load; bypass + mask encoder + decoder taps in one launch
  bool want_src = false;                   // the network has a source-fed front end (the spot network's candidate loop)
  bool src_stack = true;                   // ... and uses it (asw_spot_set_source_stack)
  bool want_up = false;                    // the network feeds 64 -> 64 decoder blocks from the stack in front (the candidate loop)
  bool up_fusion = true;                   // ... and uses it (asw_spot_set_up_fusion)

  std::vector<int> enc_cin, enc_cout;      // per encoder block
  std::vector<int> dec_cin, dec_cout, dec_stride;   // per decoder block, in execution order
  int stride_product = 1;

  DevBuf pre_w, pre_b;
  WBuf src_wt, src_pre;                    // preproc folded into encoder block 0's first layer: composed weight, [W | b]
  std::vector<EncBlock> enc;
  std::vector<DecBlock> dec;
  WBuf byp_wt, mask_wt, dec_wt;
  WBuf byp_wt48;                           // bypass kernel padded to 48 taps, fragment order (fused mask path)
  DevBuf byp_b, mask_b;
  float out_bias = 0.f;
  int byp_k = 0;                           // padded K of the bypass GEMM

  const std::vector<float>& P(const std::string& k) const { return raw.at(k); }

  // The per-call precision of a GEMM-class site, decided by what its A operand is.  Normed: the output of a LayerNorm,
  // of GroupNorm + GLU or of the input normalisation, that output through a bounded pointwise step (Swish), or the
  // skip-add of two such tensors -- bounded by the affine parameters whatever the weights do.  Raw: anything else (the
  // attention context, a feed-forward hidden layer, the masked latent).  The residual stacks and the strided /
  // transposed convolutions of the trunk all read Normed operands and pass `precision` itself.
  //  * f32 / f16x3 / f16: every site runs in the model's precision.
  //  * f16x3_safe: a Raw site runs on the exact f32 MFMA (the fp32 weights sit beside the split ones, WBuf::bind); a
  //    Normed site runs the f16x3 kernels under per-call precision 3, which differs from 1 only in the range guard of
  //    the plain epilogue: no split GEMM reads that output, so a finite value of any size is no error.
  enum class Src { Normed, Raw };
  int site(Src a) const { return !exact_raw ? precision : a == Src::Raw ? 0 : 3; }

  // ---- create: the device, the derived shape and its checks
  int init_shape(const TrunkCfg& c, const char* who) {
    tc = c;
    ASW_HIP(hipGetDevice(&device));
    int cin = c.channels, ch = c.channels;
    for (int i = 0; i < c.depth; ++i) {
      ASW_CHECK_ARG(c.stride_list[i] >= 1, "%s: stride", who);
      enc_cin.push_back(cin);
      enc_cout.push_back(ch);
      stride_product *= c.stride_list[i];
      cin = ch;
      ch *= c.growth;
    }
    // decoder blocks in execution order (network.py:221-231 inserts at the front): the encoder's, mirrored
    dec_cin.assign(enc_cout.rbegin(), enc_cout.rend());
    dec_cout.assign(enc_cin.rbegin(), enc_cin.rend());
    dec_stride.assign(std::make_reverse_iterator(c.stride_list + c.depth), std::make_reverse_iterator(c.stride_list));
    return ASW_OK;
  }
  // the last check of create, after the network's bottleneck-width check, which a bad growth or channel count fails first
  int check_level_widths(const char* who) const {
    for (int w : enc_cin) ASW_CHECK_ARG(w <= 512 && (w & (w - 1)) == 0, "%s: level width %d must be a power of two <= 512", who, w);
    return ASW_OK;
  }

  // ---- finalize
  ParamList trunk_params() const {
    ParamList v;
    const size_t K = tc.kernel_size;
    v.push_back({"preproc.weight", (size_t)tc.channels * tc.n_mics});
    v.push_back({"preproc.bias", (size_t)tc.channels});
    auto res = [&](const std::string& p, size_t ch) {
      for (int j = 0; j < tc.residual_layers; ++j) {
        const std::string q = p + ".res.seq." + std::to_string(j);
        v.push_back({q + ".conv.weight", ch * ch * K});
        v.push_back({q + ".conv.bias", ch});
        v.push_back({q + ".norm.weight", ch});
        v.push_back({q + ".norm.bias", ch});
      }
    };
    for (int i = 0; i < tc.depth; ++i) {
      const std::string p = "encoder.module_list." + std::to_string(i);
      const size_t ci = enc_cin[i], co = enc_cout[i];
      res(p, ci);
      v.push_back({p + ".conv1.weight", 2 * co * ci * K});
      v.push_back({p + ".conv1.bias", 2 * co});
      v.push_back({p + ".norm1.weight", 2 * co});
      v.push_back({p + ".norm1.bias", 2 * co});
    }
    for (int i = 0; i < tc.depth; ++i) {
      const std::string p = "decoder.module_list." + std::to_string(i);
      const size_t ci = dec_cin[i], co = dec_cout[i], s = dec_stride[i];
      v.push_back({p + ".upsample.conv.weight", ci * 2 * co * s});
      v.push_back({p + ".upsample.conv.bias", 2 * co});
      v.push_back({p + ".norm1.weight", 2 * co});
      v.push_back({p + ".norm1.bias", 2 * co});
      res(p, co);
    }
    const size_t E = tc.encoder_channels, EK = tc.encoder_kernel_size;
    v.push_back({"reference_bypass.weight", E * EK});
    v.push_back({"reference_bypass.bias", E});
    v.push_back({"mask_encoder.weight", E * tc.channels * EK});
    v.push_back({"mask_encoder.bias", E});
    v.push_back({"output_decoder.weight", E * EK});
    v.push_back({"output_decoder.bias", 1});
    return v;
  }

  // The device check, the strict check of the state dict against `want` (the trunk's keys and the network's own), then
  // the trunk weights that no gate touches.
  int finalize_trunk(const char* who, const ParamList& want) {
    {
      int dev = -1;
      ASW_HIP(hipGetDevice(&dev));
      if (dev != device)
        return asw::set_error(ASW_ERR_STATE, "%s: model was created on HIP device %d, current device is %d", who, device, dev);
    }
    for (const auto& kv : want) {
      auto it = raw.find(kv.first);
      if (it == raw.end()) return asw::set_error(ASW_ERR_STATE, "state dict is missing key %s", kv.first.c_str());
      if (it->second.size() != kv.second)
        return asw::set_error(ASW_ERR_ARG, "%s: %zu elements, expected %zu", kv.first.c_str(), it->second.size(), kv.second);
    }
    if (raw.size() != want.size())
      return asw::set_error(ASW_ERR_ARG, "state dict has %zu unexpected keys", raw.size() - want.size());
    int rc;
    const int K = tc.kernel_size, RL = tc.residual_layers, RD = tc.residual_dilation_factor;
    UP(pre_w, P("preproc.weight"));
    UP(pre_b, P("preproc.bias"));
    enc.clear(); enc.resize(tc.depth);
    dec.clear(); dec.resize(tc.depth);
    for (int i = 0; i < tc.depth; ++i) {
      const std::string p = "encoder.module_list." + std::to_string(i);
      if ((rc = pack_res_layers(raw, p, enc_cin[i], K, RL, RD, enc[i].res))) return rc;
      UP(enc[i].bias, P(p + ".conv1.bias"));
      UP(enc[i].gn_g, P(p + ".norm1.weight"));
      UP(enc[i].gn_b, P(p + ".norm1.bias"));
    }
    if (want_src && tc.channels == 64 && tc.n_mics <= 7 && K <= 7 && enc[0].res[0].wt.fhi) {
      // No non-linearity separates preproc (1x1, n_mics -> 64) from the first residual layer's convolution:
      // conv(preproc(u)) is a convolution of u~ = (u_0 .. u_6, 1) with Wc_k [W | b], composed here in double.  The
      // last channel carries the bias, so the rows next to the zero padding come out right without a special case.
      // No window gate enters encoder block 0's residual layers: one composed weight serves every gate set.
      std::vector<float> pre16((size_t)64 * 16), comp((size_t)64 * 64);
      if ((rc = asw_compose_source_weights(P("encoder.module_list.0.res.seq.0.conv.weight").data(), P("preproc.weight").data(),
                                           P("preproc.bias").data(), tc.n_mics, K, comp.data(), pre16.data())))
        return rc;
      if ((rc = src_wt.upload_gemm(comp, 64, 64))) return rc;
      if ((rc = src_pre.upload_gemm(pre16, 64, 16))) return rc;
    }
    for (int i = 0; i < tc.depth; ++i) {
      const std::string p = "decoder.module_list." + std::to_string(i);
      if ((rc = pack_res_layers(raw, p, dec_cout[i], K, RL, RD, dec[i].res))) return rc;
      UP(dec[i].gn_g, P(p + ".norm1.weight"));
      UP(dec[i].gn_b, P(p + ".norm1.bias"));
    }
    const int E = tc.encoder_channels, EK = tc.encoder_kernel_size;
    byp_k = ((EK + 31) / 32) * 32;
    {
      const std::vector<float>& w = P("reference_bypass.weight");   // [E][1][EK]
      std::vector<float> wt((size_t)E * byp_k, 0.f);
      for (int n = 0; n < E; ++n)
        for (int k = 0; k < EK; ++k) wt[(size_t)n * byp_k + k] = w[(size_t)n * EK + k];
      UP(byp_wt, wt);
      UP(byp_b, P("reference_bypass.bias"));
      if (E % 32 == 0 && EK <= 48) {
        std::vector<float> w48((size_t)E * 48, 0.f);
        for (int n = 0; n < E; ++n)
          for (int k = 0; k < EK; ++k) w48[(size_t)n * 48 + k] = w[(size_t)n * EK + k];
        if ((rc = byp_wt48.upload_gemm(w48, E, 48))) return rc;
      }
    }
    if ((rc = mask_wt.upload_gemm(pack_conv(P("mask_encoder.weight"), E, tc.channels, EK, nullptr), E, tc.channels * EK))) return rc;
    UP(mask_b, P("mask_encoder.bias"));
    {
      const std::vector<float>& w = P("output_decoder.weight");     // [E][1][EK]
      std::vector<float> wt((size_t)64 * E, 0.f);
      for (int j = 0; j < EK; ++j)
        for (int e = 0; e < E; ++e) wt[(size_t)j * E + e] = w[(size_t)e * EK + j];
      if ((rc = dec_wt.upload_gemm(wt, 64, E))) return rc;
      out_bias = P("output_decoder.bias")[0];
    }
    return ASW_OK;
  }

  // gate(p): the gate of block p ("encoder.module_list.i" / "decoder.module_list.j"), empty for none
  template <class Gate>
  int pack_gated(GatedConvs& o, Gate gate) const {
    const int K = tc.kernel_size;
    int rc;
    o.down_wt.clear(); o.down_wt.resize(tc.depth);
    o.up_wt.clear(); o.up_wt.resize(tc.depth);
    o.up_bias.clear(); o.up_bias.resize(tc.depth);
    o.up_feed.clear(); o.up_feed.resize(tc.depth);
    for (int i = 0; i < tc.depth; ++i) {
      const std::string p = "encoder.module_list." + std::to_string(i);
      const std::vector<float> g = gate(p);
      const int n = 2 * enc_cout[i], ci = enc_cin[i];
      if ((rc = o.down_wt[i].upload_gemm(pack_conv(P(p + ".conv1.weight"), n, ci, K, g.empty() ? nullptr : g.data()), n, ci * K)))
        return rc;
    }
    for (int j = 0; j < tc.depth; ++j) {
      const std::string p = "decoder.module_list." + std::to_string(j);
      const std::vector<float> g = gate(p);
      const int ci = dec_cin[j], co2 = 2 * dec_cout[j], s = dec_stride[j];
      std::vector<float> wt, bb;
      pack_conv_transpose(P(p + ".upsample.conv.weight"), P(p + ".upsample.conv.bias"), ci, co2, s,
                          g.empty() ? nullptr : g.data(), wt, bb);
      if ((rc = o.up_wt[j].upload_gemm(wt, s * co2, ci))) return rc;
      if (want_up && up_feed_shape(j) && (rc = o.up_feed[j].upload_up_feed(wt, s * co2, ci))) return rc;
      UP(o.up_bias[j], bb);
    }
    return ASW_OK;
  }

  // ---- workspace
  // The one-launch mask path (asw_mask_path_f16x3) applies in f16x3 mode when the shapes fit its tiles.
  bool fused_mask_path() const {
    return fuse_mask && precision >= 1 && tc.encoder_channels % 256 == 0 && tc.channels % 32 == 0 &&
           tc.encoder_kernel_size <= 48 && tc.encoder_stride % 4 == 0 && byp_wt48.fhi && dec_wt.fhi && mask_wt.fhi;
  }
  // the candidate loop feeds encoder block 0 from the network input (f16x3, the fused pair as its first launch)
  bool src_path() const {
    return want_src && src_stack && precision == 1 && src_wt.fhi && src_pre.fhi && !enc.empty() &&
           resstack_ok(enc[0].res, precision, enc_cin[0], tc.kernel_size) &&
           resstack_fuse_count(enc[0].res, 0, tc.kernel_size) == 2;
  }
  // decoder block j is a 64 -> 64 channel stride-2 block behind a 64-channel block: the shape a stack's UpFeed serves
  bool up_feed_shape(int j) const {
    return j >= 1 && dec_cin[j] == 64 && dec_cout[j] == 64 && dec_stride[j] == 2 && dec_cout[j - 1] == 64;
  }
  // the candidate loop lets block j - 1's stack apply block j's transposed convolution.  f16x3 and f16x3_safe alike: the
  // operand is a LayerNorm output plus a skip tensor, a Normed site (site()), which both modes run on the split kernels,
  // and the raw rows leave through a statistics epilogue, which has no range guard in either.
  // ASW_NO_UP_FUSION=1 keeps the separate launch whatever the handle says (A/B measurements).
  bool up_path(const GatedConvs& g, int j) const {
    static const bool off = getenv("ASW_NO_UP_FUSION") != nullptr;
    return !off && want_up && up_fusion && precision == 1 && up_feed_shape(j) && g.up_feed[j].fhi &&
           resstack_ok(dec[j - 1].res, precision, 64, tc.kernel_size);
  }
  // the shape of a batch of B sequences of T samples and its level buffers: the head of the workspace
  void layout_levels(int B, int T, Arena& a, TrunkPlan& pl) const {
    const int depth = tc.depth, EK = tc.encoder_kernel_size, ES = tc.encoder_stride;
    pl.B = B; pl.T = T;
    pl.Tp = ((T - 1) / stride_product + 1) * stride_product;
    pl.F = (pl.Tp + 2 * (EK / 2) - EK) / ES + 1;
    pl.RL = ((EK / 2 + pl.Tp + byp_k + 64) + 3) & ~3;
    pl.Tl.assign(depth + 1, pl.Tp);
    for (int i = 0; i < depth; ++i) pl.Tl[i + 1] = pl.Tl[i] / tc.stride_list[i];
    pl.mean = a.take<float>(B);
    pl.stdv = a.take<float>(B);
    pl.refn = a.take<float>((size_t)B * pl.RL);
    if (want_src) {
      pl.src_hi = a.take<uint16_t>((size_t)B * pl.Tp * 8);
      pl.src_lo = a.take<uint16_t>((size_t)B * pl.Tp * 8);
    }
    pl.X.resize(depth + 1); pl.Pb.resize(depth); pl.Qb.resize(depth);
    pl.raw_dn.resize(depth); pl.raw_up.resize(depth); pl.st_dn.resize(depth); pl.st_up.resize(depth);
    pl.mr_up.resize(depth); pl.mr_dn.resize(depth);
    for (int i = 0; i <= depth; ++i) {
      const int ch = i == 0 ? tc.channels : enc_cout[i - 1];
      pl.X[i] = a.take<float>((size_t)B * pl.Tl[i] * ch);
    }
    for (int i = 0; i < depth; ++i) {
      const size_t n = (size_t)B * pl.Tl[i] * enc_cin[i];
      pl.Pb[i] = a.take<float>(n);
      pl.Qb[i] = a.take<float>(n);
      pl.raw_dn[i] = a.take<float>((size_t)B * pl.Tl[i + 1] * 2 * enc_cout[i]);
      pl.st_dn[i] = a.take<float>((size_t)B * 4 * asw_convgemm_stats_tiles(pl.Tl[i + 1], 2 * enc_cout[i]));
      pl.mr_dn[i] = a.take<float>((size_t)B * 4);
    }
    for (int j = 0; j < depth; ++j) {
      const int lvl = depth - j;             // input level of decoder block j
      const int s = dec_stride[j], co2 = 2 * dec_cout[j];
      pl.raw_up[j] = a.take<float>((size_t)B * pl.Tl[lvl] * s * co2);
      int tiles = asw_convgemm_stats_tiles(pl.Tl[lvl], s * co2);
      if (want_up && up_feed_shape(j))           // fed by block j - 1's stack: its row tiles, whichever is more
        for (int glu = 0; glu < 2; ++glu) {
          const int t = up_feed_tiles(dec[j - 1].res, tc.kernel_size, pl.Tl[lvl], glu != 0);
          tiles = t > tiles ? t : tiles;
        }
      pl.st_up[j] = a.take<float>((size_t)B * 4 * tiles);
      pl.mr_up[j] = a.take<float>((size_t)B * 4);
    }
  }
  // the mask path's buffers, after the bottleneck's
  void layout_mask(Arena& a, TrunkPlan& pl) const {
    const int E = tc.encoder_channels;
    const bool fused = fused_mask_path();
    // fused mask path: no latent, one partial tap tensor per 256-channel column tile
    pl.Y = fused ? nullptr : a.take<float>((size_t)pl.B * pl.F * E);
    pl.D = a.take<float>((size_t)(fused ? E / 256 : 1) * pl.B * pl.F * 64);
    pl.ywave = a.take<float>((size_t)pl.B * pl.T);
  }

  // ---- run; pl.X[0] (or the source planes) / pl.refn are filled
  // encoder (network.py:98-113,146-156): X[0] -> X[depth]
  // src0: pl.src_hi / pl.src_lo are filled instead of pl.X[0] (src_path()); X[0] is neither read nor written
  int encode(TrunkPlan& pl, const GatedConvs& g, hipStream_t s, bool src0 = false) {
    const int B = pl.B, K = tc.kernel_size;
    taps.clear();
    if (!src0) taps["preproc"] = {pl.X[0], (size_t)B * pl.Tl[0] * tc.channels};
    int rc;
    GluSrc src = {};
    const SrcFeed feed = {pl.src_hi, pl.src_lo, &src_wt, &src_pre};
    bool glu = false;                        // X[i] is still un-normalised in raw_dn[i-1]: block i applies GroupNorm + GLU
    for (int i = 0; i < tc.depth; ++i) {
      float* r = nullptr;
      if ((rc = run_res(enc[i].res, precision, B, pl.Tl[i], enc_cin[i], K, pl.X[i], pl.Pb[i], pl.Qb[i], &r, s,
                        glu ? &src : nullptr, (src0 && i == 0) ? &feed : nullptr)))
        return rc;
      asw_convgemm_args a = {};
      a.A = r; g.down_wt[i].bind(a, precision); a.bias = enc[i].bias.p; a.out = pl.raw_dn[i]; a.stats = pl.st_dn[i];
      a.B = B; a.M_out = pl.Tl[i + 1]; a.N = 2 * enc_cout[i]; a.Cin = enc_cin[i]; a.taps = K;
      a.stride = tc.stride_list[i]; a.dil = 1; a.pad = K / 2;
      a.a_row_stride = a.Cin; a.a_batch_stride = (int64_t)pl.Tl[i] * a.Cin; a.a_len = a.a_batch_stride;
      a.chan_mod = a.N;
      if ((rc = asw_convgemm_f32(&a, s))) return rc;
      // the next block normalises while its first layer stages rows and writes X[i+1] (the skip connection the
      // decoder reads) from the same registers: one pass over raw_dn less
      glu = fuse_mask && i + 1 < tc.depth && glu_on_load_ok(enc[i + 1].res, precision, enc_cout[i]);
      const int tiles = asw_convgemm_stats_tiles(a.M_out, a.N);
      if (glu) {
        if ((rc = asw_gn_finalize(pl.st_dn[i], tiles, B, pl.Tl[i + 1], enc_cout[i], 1e-5f, pl.mr_dn[i], s))) return rc;
        src = {pl.raw_dn[i], pl.mr_dn[i], enc[i].gn_g.p, enc[i].gn_b.p, pl.X[i + 1]};
      } else if ((rc = asw_gn_glu(pl.raw_dn[i], pl.st_dn[i], tiles, enc[i].gn_g.p, enc[i].gn_b.p, B, pl.Tl[i + 1],
                                  enc_cout[i], 1e-5f, pl.X[i + 1], s))) {
        return rc;
      }
      taps["enc" + std::to_string(i)] = {pl.X[i + 1], (size_t)B * pl.Tl[i + 1] * enc_cout[i]};
    }
    return ASW_OK;
  }

  // decoder (network.py:180-200,233-238): x, the bottleneck's output on entry, is the last block's output on return
  // up: the candidate loop; a 64 -> 64 block's transposed convolution is then applied by the stack in front of it
  // (up_path), whose own output -- and with it the block's tap -- does not exist
  int decode(TrunkPlan& pl, const GatedConvs& g, const float*& x, hipStream_t s, bool up = false) {
    const int B = pl.B, K = tc.kernel_size;
    int rc;
    int fed_tiles = 0;                       // > 0: block j - 1's stack has written raw_up[j] and that many partial sums per item
    for (int j = 0; j < tc.depth; ++j) {
      const int lvl = tc.depth - j, ci = dec_cin[j], co = dec_cout[j], st = dec_stride[j];
      int tiles = fed_tiles;
      if (!fed_tiles) {
        asw_convgemm_args a = {};
        a.A = x; a.A2 = pl.X[lvl]; g.up_wt[j].bind(a, precision); a.bias = g.up_bias[j].p; a.out = pl.raw_up[j];
        a.stats = pl.st_up[j];
        a.B = B; a.M_out = pl.Tl[lvl]; a.N = st * 2 * co; a.Cin = ci; a.taps = 1; a.stride = 1; a.dil = 1; a.pad = 0;
        a.a_row_stride = ci; a.a_batch_stride = (int64_t)pl.Tl[lvl] * ci; a.a_len = a.a_batch_stride;
        a.chan_mod = 2 * co;
        if ((rc = asw_convgemm_f32(&a, s))) return rc;
        tiles = asw_convgemm_stats_tiles(a.M_out, a.N);
      }
      const int To = pl.Tl[lvl] * st;        // == pl.Tl[lvl-1]
      float* gb = pl.Qb[lvl - 1];
      float* r = nullptr;
      const bool feed_next = up && j + 1 < tc.depth && up_path(g, j + 1);
      UpFeed uf = {};
      if (feed_next) uf = {&g.up_feed[j + 1], g.up_bias[j + 1].p, pl.X[lvl - 1], pl.raw_up[j + 1], pl.st_up[j + 1], 0};
      UpFeed* ufp = feed_next ? &uf : nullptr;
      if (fuse_mask && glu_on_load_ok(dec[j].res, precision, co)) {
        // GroupNorm + GLU happen while the first residual layer stages its rows: at 64 channels the normalised
        // tensor is neither written nor read back (P -> gb -> P are the stack's own buffers), above that it is
        // written once for the layer's residual instead of written and read twice
        if ((rc = asw_gn_finalize(pl.st_up[j], tiles, B, To, co, 1e-5f, pl.mr_up[j], s))) return rc;
        // (gb: free until the second layer writes it; the wide layers read their residual from there)
        const GluSrc src = {pl.raw_up[j], pl.mr_up[j], dec[j].gn_g.p, dec[j].gn_b.p, co > 64 ? gb : nullptr};
        if ((rc = run_res(dec[j].res, precision, B, To, co, K, gb, pl.Pb[lvl - 1], gb, &r, s, &src, nullptr, ufp))) return rc;
      } else {
        if ((rc = asw_gn_glu(pl.raw_up[j], pl.st_up[j], tiles, dec[j].gn_g.p, dec[j].gn_b.p, B, To, co, 1e-5f, gb, s)))
          return rc;
        // residual ping-pong: gb -> P -> gb -> P ...
        if ((rc = run_res(dec[j].res, precision, B, To, co, K, gb, pl.Pb[lvl - 1], gb, &r, s, nullptr, nullptr, ufp))) return rc;
      }
      x = r;
      fed_tiles = feed_next ? uf.tiles : 0;
      if (!feed_next) taps["dec" + std::to_string(j)] = {x, (size_t)B * To * co};
    }
    return ASW_OK;
  }

  // mask path (spot network.py:327-349,397-405): every sequence's mask gates the latent of its reference channel;
  // x is the last decoder block's output
  int mask_path(TrunkPlan& pl, const float* x, const float* mean, const float* stdv, float* out_wave, hipStream_t s) {
    const int B = pl.B, C = tc.channels, E = tc.encoder_channels, EK = tc.encoder_kernel_size, ES = tc.encoder_stride;
    int rc;
    asw_convgemm_args me = {};    // mask_encoder
    me.A = x; mask_wt.bind(me, site(Src::Normed)); me.bias = mask_b.p;
    me.B = B; me.M_out = pl.F; me.N = E; me.Cin = C; me.taps = EK; me.stride = ES; me.dil = 1; me.pad = EK / 2;
    me.a_row_stride = C; me.a_batch_stride = (int64_t)pl.Tp * C; me.a_len = me.a_batch_stride;
    if (fused_mask_path()) {
      asw_maskpath_args f = {};
      f.enc = me;
      f.ref = pl.refn; f.ref_batch_stride = pl.RL; f.ref_len = pl.RL; f.ref_hop = ES;
      f.byp_k = 48; f.byp_taps = EK; f.byp_shift = byp_wt48.shift; f.byp_hi = byp_wt48.fhi; f.byp_lo = byp_wt48.flo;
      f.byp_bias = byp_b.p;
      f.dec_hi = dec_wt.fhi; f.dec_lo = dec_wt.flo; f.dec_shift = dec_wt.shift; f.dec_taps = EK;
      f.taps = pl.D;
      // the gated latent is split inside the kernel: the safe mode takes the variant that scales every frame first
      f.enc.precision = precision;
      if ((rc = exact_raw ? asw_mask_path_f16x3_scaled(&f, s) : asw_mask_path_f16x3(&f, s))) return rc;
      return asw_overlap_add_parts(pl.D, E / 256, B, pl.F, 64, EK, EK / 2, pl.T, 9, 8, out_bias, mean, stdv, out_wave, s);
    }
    {
      asw_convgemm_args a = {};   // reference_bypass: rows of the padded reference channel, hop ES
      a.A = pl.refn; byp_wt.bind(a, site(Src::Normed)); a.bias = byp_b.p; a.out = pl.Y;
      a.B = B; a.M_out = pl.F; a.N = E; a.Cin = byp_k; a.taps = 1; a.stride = 1; a.dil = 1; a.pad = 0;
      a.a_row_stride = ES; a.a_batch_stride = pl.RL; a.a_len = pl.RL; a.relu = 1;
      if ((rc = asw_convgemm_f32(&a, s))) return rc;
    }
    me.mul = pl.Y; me.out = pl.Y; me.relu = 1;   // mask_encoder, ReLU, times the bypass latent (in place)
    if ((rc = asw_convgemm_f32(&me, s))) return rc;
    taps["latent"] = {pl.Y, (size_t)B * pl.F * E};
    {
      asw_convgemm_args a = {};   // output_decoder taps: D[f][j] = sum_e latent[f][e] * w[e][j]
      a.A = pl.Y; dec_wt.bind(a, site(Src::Raw)); a.out = pl.D;
      a.B = B; a.M_out = pl.F; a.N = 64; a.Cin = E; a.taps = 1; a.stride = 1; a.dil = 1; a.pad = 0;
      a.a_row_stride = E; a.a_batch_stride = (int64_t)pl.F * E; a.a_len = a.a_batch_stride;
      if ((rc = asw_convgemm_f32(&a, s))) return rc;
    }
    return asw_overlap_add_unnorm(pl.D, B, pl.F, 64, EK, EK / 2, pl.T, 9, 8, out_bias, mean, stdv, out_wave, s);
  }
};

// ---- the post-norm transformer layer of both bottlenecks (nn.TransformerEncoderLayer, norm_first = False): the spot
// network's layers along time and the separation network's layers across speakers.  The uploads stay with the networks
// and differ on purpose: the spot layer packs MFMA fragments (WBuf::upload_gemm), the separation layer does not (UP) --
// `linear` picks its kernel by what the weight carries, so uploading alike would change the kernels a network runs.
struct PostNormLayer { WBuf w_in, w_out, w1, w2; DevBuf b_in, b_out, b1, b2, n1g, n1b, n2g, n2b; };
struct PostNormBufs { float *qkv, *ctx, *x1, *ff; };      // [rows][3d], [rows][d], [rows][d], [rows][ffw] of the caller's plan

// x -> out, both [rows][d]: in-proj, attention(qkv, ctx), out-proj + residual + LayerNorm, linear1 + ReLU,
// linear2 + residual + LayerNorm.  x and x1 are normalised tensors, ctx and the hidden layer are not (Trunk::site).
template <class Attention>
int run_post_norm(const Trunk& m, const PostNormLayer& t, const PostNormBufs& b, const float* x, float* out, int rows, int d,
                  int ffw, Attention&& attention, hipStream_t s) {
  const int normed = m.site(Trunk::Src::Normed), rawp = m.site(Trunk::Src::Raw);
  int rc;
  if ((rc = linear(x, t.w_in, normed, t.b_in.p, rows, 3 * d, d, 0, nullptr, nullptr, nullptr, b.qkv, s))) return rc;
  if ((rc = attention(b.qkv, b.ctx))) return rc;
  if ((rc = linear(b.ctx, t.w_out, rawp, t.b_out.p, rows, d, d, 0, x, t.n1g.p, t.n1b.p, b.x1, s))) return rc;
  if ((rc = linear(b.x1, t.w1, normed, t.b1.p, rows, ffw, d, 1, nullptr, nullptr, nullptr, b.ff, s))) return rc;
  return linear(b.ff, t.w2, rawp, t.b2.p, rows, d, ffw, 0, b.x1, t.n2g.p, t.n2b.p, out, s);
}

// ---- the handle calls both networks share; `who` / `fin` name the entry point in the messages
inline int check_ready(const Trunk* m, const char* fin) {
  if (!m) return asw::set_error(ASW_ERR_ARG, "null model handle");
  if (!m->finalized) return asw::set_error(ASW_ERR_STATE, "%s() has not been called", fin);
  int dev = -1;
  ASW_HIP(hipGetDevice(&dev));
  if (dev != m->device)
    return asw::set_error(ASW_ERR_STATE, "model lives on HIP device %d but the current device is %d", m->device, dev);
  return ASW_OK;
}

inline int set_precision(Trunk* m, const char* who, int precision) {
  ASW_CHECK_ARG(m && (precision >= 0 && precision <= 3), "%s: 0 (f32), 1 (f16x3), 2 (single-pass f16) or 3 (f16x3_safe)", who);
  // 3 is the three-term split (every `precision == 1` choice of kernels holds) plus exact arithmetic at the Raw sites
  m->exact_raw = precision == 3;
  m->precision = m->exact_raw ? 1 : precision;
  return ASW_OK;
}

inline int set_param(Trunk* m, const char* who, const char* key, const float* host_data, size_t numel) {
  ASW_CHECK_ARG(m && key && host_data, "%s: null pointer", who);
  m->raw[key].assign(host_data, host_data + numel);
  m->finalized = false;
  return ASW_OK;
}

inline int get_tap(const Trunk* m, const char* who, const char* name, float* dst, size_t capacity, size_t* numel,
                   void* stream) {
  ASW_CHECK_ARG(m && name && numel, "%s: null pointer", who);
  auto it = m->taps.find(name);
  if (it == m->taps.end()) return asw::set_error(ASW_ERR_ARG, "%s: no activation named %s", who, name);
  *numel = it->second.numel;
  if (dst) {
    ASW_CHECK_ARG(capacity >= it->second.numel, "%s: buffer too small", who);
    ASW_HIP(hipMemcpyAsync(dst, it->second.p, it->second.numel * sizeof(float), hipMemcpyDeviceToDevice,
                           asw::as_stream(stream)));
  }
  return ASW_OK;
}

}  // namespace asw_model
