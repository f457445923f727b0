// sep_model.hip -- device-resident joint separation network ("separation by localization"):
// weight packing + the layer schedule of Network.forward / infer_sample
// (sep/training/SpeakerSeparation/network.py:418-548) as launches of the kernels in
// prep_kernels.hip / convgemm.hip / misc_kernels.hip / sep_kernels.hip on one HIP stream.
//
// One call separates the S talkers the search found: every speaker s is one "sequence" --
// the mixture aligned to that speaker (zero-filled integer shift), normalised with statistics
// shared by all S*M channels -- so the U-Net encoder / decoder and the mask path run with
// batch S on the same channels-last [S][T_l][C] layout and the same MFMA kernels as the spot
// network (kernel size 5, strides 2,2,4,4, dilations 1,2,4, latent 4096).  The bottleneck
// ([S][L][d], L = T/64, d = 512) alternates a Conformer layer along time per speaker with a
// transformer layer across the S speakers of each time step (:270-321).
//
// The Conformer follows the published speechbrain definitions (the library is absent from the
// image; oracle/sep_ref.py restates it and states what is pinned).  Weight transformations done
// once at finalize: speechbrain's per-head (q,k,v) interleave of in_proj_weight is permuted to
// Q | K | V; the macaron factor 1/2 is folded into the second feed-forward linear; the
// depthwise kernel is stored tap-major.
//
// The U-Net trunk is model_common.h's Trunk, shared with the spot network; this file holds the
// Conformer / inter-speaker bottleneck, the workspace policy and the C entry points.
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "model_common.h"

using namespace asw_model;

extern "C" int asw_joint_shift_stats_scratch_doubles(void);
namespace asw {   // sep_kernels.hip: the launcher behind asw_inter_attention / asw_inter_attention_groups
int inter_attention_launch(const char* who, const float* qkv, const int32_t* bounds, int G, int S_uniform, int L, int d,
                           int nhead, float* ctx, hipStream_t st);
}

namespace {

struct Ffn { DevBuf lng, lnb, b1, b2; WBuf w1, w2; };                       // w2 / b2 carry the macaron 1/2
struct ConfLayer {
  Ffn f1, f2;
  DevBuf n1g, n1b, n2g, n2b, fng, fnb;                                     // norm1, norm2, encoder-final norm
  WBuf w_in, w_pos, w_out;
  DevBuf b_out, bu, bv;
  DevBuf cm_lng, cm_lnb, cm_pwb, dw_wT, dw_b, ac_lng, ac_lnb, ac_b;
  WBuf cm_pw, ac_w;
};

}  // namespace

struct asw_sep : Trunk {
  asw_sep_config cfg;
  GatedConvs convs;                         // down / up convolutions (no window gate in this network)
  std::vector<ConfLayer> conf;
  std::vector<PostNormLayer> inter;           // across the speakers of a time step
  std::vector<float> inv_freq;
  DevBuf pe;                                // sinusoid table [2L-1][d] of the last sequence length
  int pe_L = 0;

  char* ws = nullptr;
  size_t ws_bytes = 0;

  ~asw_sep() { if (ws) (void)hipFree(ws); }
};

namespace {

// the trunk's keys, then the bottleneck's
ParamList expected_params(const asw_sep* m) {
  const asw_sep_config& c = m->cfg;
  ParamList v = m->trunk_params();
  const size_t d = m->enc_cout.back(), f = c.ffw_dim, BK = c.bottleneck_ksize;
  v.push_back({"bottleneck.pe_single.inv_freq", d / 2});
  for (int l = 0; l < c.bottleneck_layers; ++l) {
    const std::string cl = "bottleneck.module_list." + std::to_string(l) + ".intra.layers.0";
    v.push_back({cl + ".mha_layer.in_proj_weight", 3 * d * d});
    v.push_back({cl + ".mha_layer.pos_bias_u", d});
    v.push_back({cl + ".mha_layer.pos_bias_v", d});
    v.push_back({cl + ".mha_layer.out_proj.weight", d * d});
    v.push_back({cl + ".mha_layer.out_proj.bias", d});
    v.push_back({cl + ".mha_layer.linear_pos.weight", d * d});
    v.push_back({cl + ".convolution_module.layer_norm.weight", d});
    v.push_back({cl + ".convolution_module.layer_norm.bias", d});
    v.push_back({cl + ".convolution_module.bottleneck.0.weight", 2 * d * d});
    v.push_back({cl + ".convolution_module.bottleneck.0.bias", 2 * d});
    v.push_back({cl + ".convolution_module.conv.weight", d * BK});
    v.push_back({cl + ".convolution_module.conv.bias", d});
    v.push_back({cl + ".convolution_module.after_conv.0.weight", d});
    v.push_back({cl + ".convolution_module.after_conv.0.bias", d});
    v.push_back({cl + ".convolution_module.after_conv.2.weight", d * d});
    v.push_back({cl + ".convolution_module.after_conv.2.bias", d});
    for (const char* fm : {".ffn_module1", ".ffn_module2"}) {
      v.push_back({cl + fm + ".0.weight", d});
      v.push_back({cl + fm + ".0.bias", d});
      v.push_back({cl + fm + ".1.ffn.0.weight", f * d});
      v.push_back({cl + fm + ".1.ffn.0.bias", f});
      v.push_back({cl + fm + ".1.ffn.3.weight", d * f});
      v.push_back({cl + fm + ".1.ffn.3.bias", d});
    }
    v.push_back({cl + ".norm1.norm.weight", d});
    v.push_back({cl + ".norm1.norm.bias", d});
    v.push_back({cl + ".norm2.norm.weight", d});
    v.push_back({cl + ".norm2.norm.bias", d});
    const std::string ce = "bottleneck.module_list." + std::to_string(l) + ".intra.norm.norm";
    v.push_back({ce + ".weight", d});
    v.push_back({ce + ".bias", d});
    const std::string t = "bottleneck.module_list." + std::to_string(l) + ".inter.layers.0";
    v.push_back({t + ".self_attn.in_proj_weight", 3 * d * d});
    v.push_back({t + ".self_attn.in_proj_bias", 3 * d});
    v.push_back({t + ".self_attn.out_proj.weight", d * d});
    v.push_back({t + ".self_attn.out_proj.bias", d});
    v.push_back({t + ".linear1.weight", f * d});
    v.push_back({t + ".linear1.bias", f});
    v.push_back({t + ".linear2.weight", d * f});
    v.push_back({t + ".linear2.bias", d});
    v.push_back({t + ".norm1.weight", d});
    v.push_back({t + ".norm1.bias", d});
    v.push_back({t + ".norm2.weight", d});
    v.push_back({t + ".norm2.bias", d});
  }
  return v;
}

std::vector<float> scaled(const std::vector<float>& w, float a) {
  std::vector<float> o(w.size());
  for (size_t i = 0; i < w.size(); ++i) o[i] = w[i] * a;
  return o;
}

// ---- workspace ---------------------------------------------------------------------------
struct Plan : TrunkPlan {
  int L, d;
  // The B sequences are G groups that attend -- and, in infer / infer_batch, are normalised -- apart: all S > 0 wide
  // (forward: B = G * S), or with S == 0 the groups of the host bounds [G+1] (infer: one group; infer_batch: ragged).
  int G = 0, S = 0;
  const int32_t* bounds = nullptr;
  double* jscr;
  std::vector<float*> intra_out, inter_out;   // per bottleneck layer (kept apart so every tap stays readable)
  float *h, *g, *x1, *x2, *x3, *qkv, *ctx, *raw2, *u, *v2, *y, *f, *pos;
  const int32_t* counts = nullptr;            // forward_counts() only, host [G]: speakers present per item, the rest are zero rows
  int32_t* mix_index;                         // device [B]
};

void layout(const asw_sep* m, int B, int T, int groups, Arena& a, Plan& pl) {
  const asw_sep_config& c = m->cfg;
  m->layout_levels(B, T, a, pl);
  const size_t L = pl.Tl[c.depth], d = m->enc_cout.back(), rows = (size_t)pl.B * L;
  pl.L = (int)L; pl.d = (int)d;
  pl.intra_out.resize(c.bottleneck_layers); pl.inter_out.resize(c.bottleneck_layers);
  for (int l = 0; l < c.bottleneck_layers; ++l) { pl.intra_out[l] = a.take<float>(rows * d); pl.inter_out[l] = a.take<float>(rows * d); }
  float** dbufs[] = {&pl.h, &pl.g, &pl.x1, &pl.x2, &pl.x3, &pl.ctx, &pl.u, &pl.v2, &pl.y};
  for (float** b : dbufs) *b = a.take<float>(rows * d);
  pl.qkv = a.take<float>(rows * 3 * d);
  pl.raw2 = a.take<float>(rows * 2 * d);
  pl.f = a.take<float>(rows * c.ffw_dim);
  pl.pos = a.take<float>((2 * L - 1) * d);
  m->layout_mask(a, pl);
  pl.jscr = a.take<double>((size_t)asw_joint_shift_stats_scratch_doubles() * groups);
  pl.mix_index = a.take<int32_t>(pl.B);
}

int ensure_ws(asw_sep* m, int B, int T, Plan& pl, int groups = 1) {
  Arena dry(nullptr, 0, true);
  layout(m, B, T, groups, dry, pl);
  const size_t need = dry.off + 4096;
  if (need > m->ws_bytes) {
    // the number of talkers changes from mixture to mixture: grow by half again, not to the exact size, so that a
    // stream of mixtures re-allocates (device synchronisation + hipFree / hipMalloc of GBs) a few times, not every
    // time one more talker than ever before turns up
    size_t want = need + need / 2;
    if (m->ws) { ASW_HIP(hipDeviceSynchronize()); (void)hipFree(m->ws); m->ws = nullptr; m->ws_bytes = 0; }
    if (hipMalloc(&m->ws, want) != hipSuccess) {
      (void)hipGetLastError();
      want = need;
      if (hipMalloc(&m->ws, want) != hipSuccess)
        return asw::set_error(ASW_ERR_NOMEM, "workspace of %.1f MiB for %d sequences, T=%d", need / 1048576.0, B, T);
    }
    m->ws_bytes = want;
  }
  Arena real(m->ws, m->ws_bytes, false);
  layout(m, B, T, groups, real, pl);
  return ASW_OK;
}

// RelPosEncXL table for sequence length L: row r stands for relative position (L-1) - r; even
// columns sin(|pos| * inv_freq), odd columns cos (the published table uses the same sinusoid for
// past and future).  float32 arithmetic like the torch module.  Cached per L.
int ensure_pos_table(asw_sep* m, int L) {
  if (m->pe_L == L && m->pe.p) return ASW_OK;
  const int d = m->enc_cout.back();
  std::vector<float> pe((size_t)(2 * L - 1) * d);
  for (int r = 0; r < 2 * L - 1; ++r) {
    const float pos = (float)std::abs(r - (L - 1));
    for (int k = 0; k < d / 2; ++k) {
      const float ang = pos * m->inv_freq[k];
      pe[(size_t)r * d + 2 * k] = sinf(ang);
      pe[(size_t)r * d + 2 * k + 1] = cosf(ang);
    }
  }
  ASW_HIP(hipDeviceSynchronize());            // launches that read the previous table have finished
  int rc = m->pe.upload(pe);
  if (rc) return rc;
  m->pe_L = L;
  return ASW_OK;
}

int ffn_first(const Ffn& f, int prec, const float* hin, int rows, int d, int ffw, float* fbuf, hipStream_t s) {
  return linear(hin, f.w1, prec, f.b1.p, rows, ffw, d, /*swish*/ 2, nullptr, nullptr, nullptr, fbuf, s);
}

// one Conformer layer along time for the BS sequences: x -> out (both [BS*L][d])
int run_conformer(asw_sep* m, Plan& pl, ConfLayer& c, const float* x, float* out, hipStream_t s) {
  const asw_sep_config& cfg = m->cfg;
  const int rows = pl.B * pl.L, d = pl.d, ffw = cfg.ffw_dim;
  // prec: A is a LayerNorm output, the sinusoid table, or Swish of a LayerNorm output; rawp: the Swish'd hidden layer
  // of a feed-forward module and the attention context (Trunk::site)
  const int prec = m->site(Trunk::Src::Normed), rawp = m->site(Trunk::Src::Raw);
  int rc;
  // x1 = x + FFN1(x)/2
  if ((rc = asw_add_layernorm2(x, nullptr, 0.f, c.f1.lng.p, c.f1.lnb.p, rows, d, 1e-5f, 0, nullptr, pl.h, s))) return rc;
  if ((rc = ffn_first(c.f1, prec, pl.h, rows, d, ffw, pl.f, s))) return rc;
  if ((rc = linear(pl.f, c.f1.w2, rawp, c.f1.b2.p, rows, d, ffw, 0, nullptr, nullptr, nullptr, pl.g, s))) return rc;
  if ((rc = asw_add_layernorm2(x, pl.g, 1.f, c.n1g.p, c.n1b.p, rows, d, 1e-5f, 0, pl.x1, pl.h, s))) return rc;   // h = norm1(x1)
  // x2 = x1 + MHA(norm1(x1))
  if ((rc = linear(pl.h, c.w_in, prec, nullptr, rows, 3 * d, d, 0, nullptr, nullptr, nullptr, pl.qkv, s))) return rc;
  if ((rc = linear(m->pe.p, c.w_pos, prec, nullptr, 2 * pl.L - 1, d, d, 0, nullptr, nullptr, nullptr, pl.pos, s))) return rc;
  if ((rc = asw_relpos_attention(pl.qkv, pl.pos, c.bu.p, c.bv.p, pl.B, pl.L, d, cfg.num_head, 1.0f / sqrtf((float)d), pl.ctx, s)))
    return rc;
  if ((rc = linear(pl.ctx, c.w_out, rawp, c.b_out.p, rows, d, d, 0, nullptr, nullptr, nullptr, pl.g, s))) return rc;
  if ((rc = asw_add_layernorm2(pl.x1, pl.g, 1.f, c.cm_lng.p, c.cm_lnb.p, rows, d, 1e-5f, 0, pl.x2, pl.h, s))) return rc;
  // x3 = x2 + ConvolutionModule(x2)
  if ((rc = linear(pl.h, c.cm_pw, prec, c.cm_pwb.p, rows, 2 * d, d, 0, nullptr, nullptr, nullptr, pl.raw2, s))) return rc;
  if ((rc = asw_glu_rows(pl.raw2, rows, d, pl.u, s))) return rc;
  if ((rc = asw_dwconv_ln_swish(pl.u, c.dw_wT.p, c.dw_b.p, c.ac_lng.p, c.ac_lnb.p, pl.B, pl.L, d, cfg.bottleneck_ksize, 1e-5f,
                                pl.v2, s)))
    return rc;
  if ((rc = linear(pl.v2, c.ac_w, prec, c.ac_b.p, rows, d, d, 0, nullptr, nullptr, nullptr, pl.g, s))) return rc;
  if ((rc = asw_add_layernorm2(pl.x2, pl.g, 1.f, c.f2.lng.p, c.f2.lnb.p, rows, d, 1e-5f, 0, pl.x3, pl.h, s))) return rc;
  // y = norm2(x3 + FFN2(x3)/2); out = final norm (eps 1e-6)
  if ((rc = ffn_first(c.f2, prec, pl.h, rows, d, ffw, pl.f, s))) return rc;
  if ((rc = linear(pl.f, c.f2.w2, rawp, c.f2.b2.p, rows, d, ffw, 0, pl.x3, c.n2g.p, c.n2b.p, pl.y, s))) return rc;
  return asw_add_layernorm2(pl.y, nullptr, 0.f, c.fng.p, c.fnb.p, rows, d, 1e-6f, 0, nullptr, out, s);
}

// post-norm transformer layer across the speakers of every time step, group by group: x -> out
int run_inter(asw_sep* m, Plan& pl, PostNormLayer& t, const float* x, float* out, hipStream_t s) {
  auto attention = [&](const float* qkv, float* ctx) {
    return asw::inter_attention_launch("inter_attention", qkv, pl.bounds, pl.G, pl.S, pl.L, pl.d, m->cfg.num_head, ctx, s);
  };
  return run_post_norm(*m, t, {pl.qkv, pl.ctx, pl.x1, pl.f}, x, out, pl.B * pl.L, pl.d, m->cfg.ffw_dim, attention, s);
}

// everything after the preproc stage; pl.X[0] / pl.refn are filled
int run_network(asw_sep* m, Plan& pl, const float* mean, const float* stdv, float* out_wave, hipStream_t s) {
  const asw_sep_config& c = m->cfg;
  const int B = pl.B;
  int rc;
  if ((rc = m->encode(pl, m->convs, s))) return rc;
  // ---- bottleneck (:296-321): [BS][L][d] is already the (B*S, T, F) layout of the Conformer and,
  // row for row, the (N*T, S, F) layout of the inter-speaker layer
  if ((rc = ensure_pos_table(m, pl.L))) return rc;
  const float* x = pl.X[c.depth];
  for (int l = 0; l < c.bottleneck_layers; ++l) {
    if ((rc = run_conformer(m, pl, m->conf[l], x, pl.intra_out[l], s))) return rc;
    m->taps["intra" + std::to_string(l)] = {pl.intra_out[l], (size_t)B * pl.L * pl.d};
    if (pl.counts) {
      // items with fewer speakers: batches_to_speakers (:250-268) re-inserts the missing ones as ZERO sequences, which
      // take part in the inter-speaker attention below; whatever the Conformer made of those rows is discarded
      for (int n = 0; n < pl.G; ++n)
        if (pl.counts[n] < pl.S)
          ASW_HIP(hipMemsetAsync(pl.intra_out[l] + ((size_t)n * pl.S + pl.counts[n]) * pl.L * pl.d, 0,
                                 (size_t)(pl.S - pl.counts[n]) * pl.L * pl.d * sizeof(float), s));
    }
    if ((rc = run_inter(m, pl, m->inter[l], pl.intra_out[l], pl.inter_out[l], s))) return rc;
    m->taps["inter" + std::to_string(l)] = {pl.inter_out[l], (size_t)B * pl.L * pl.d};
    x = pl.inter_out[l];
  }
  m->taps["bottleneck"] = {x, (size_t)B * pl.L * pl.d};
  if ((rc = m->decode(pl, m->convs, x, s))) return rc;
  return m->mask_path(pl, x, mean, stdv, out_wave, s);
}

}  // namespace

extern "C" int asw_sep_create(const asw_sep_config* cfg, asw_sep** out) {
  ASW_CHECK_ARG(cfg && out, "sep_create: null pointer");
  const asw_sep_config& c = *cfg;
  const TrunkCfg tc = TrunkCfg::of(c);
  int rc = check_trunk_config(tc, "sep_create", "kernel sizes must be odd");
  if (rc) return rc;
  ASW_CHECK_ARG(c.max_speakers >= 1 && c.max_speakers <= 64, "sep_create: max_speakers %d", c.max_speakers);
  ASW_CHECK_ARG(c.bottleneck_layers >= 0, "sep_create: bad config");
  ASW_CHECK_ARG(c.bottleneck_ksize % 2 == 1, "sep_create: kernel sizes must be odd");
  std::unique_ptr<asw_sep> m(new asw_sep());
  m->cfg = c;
  if ((rc = m->init_shape(tc, "sep_create"))) return rc;
  const int d = m->enc_cout.back();
  ASW_CHECK_ARG(d <= 1024 && (d & (d - 1)) == 0 && d >= 128, "sep_create: bottleneck width %d must be a power of two in 128..1024", d);
  const int hd = c.num_head > 0 && d % c.num_head == 0 ? d / c.num_head : 0;
  ASW_CHECK_ARG(hd == 16 || hd == 32 || hd == 64, "sep_create: head_dim %d unsupported (16, 32, 64)", hd);
  if ((rc = m->check_level_widths("sep_create"))) return rc;
  *out = m.release();
  return ASW_OK;
}

extern "C" void asw_sep_destroy(asw_sep* m) { delete m; }

extern "C" int asw_sep_set_precision(asw_sep* m, int precision) { return set_precision(m, "sep_set_precision", precision); }

extern "C" int asw_sep_set_param(asw_sep* m, const char* key, const float* host_data, size_t numel) {
  return set_param(m, "sep_set_param", key, host_data, numel);
}

extern "C" int asw_sep_finalize(asw_sep* m) {
  ASW_CHECK_ARG(m, "sep_finalize: null handle");
  const asw_sep_config& c = m->cfg;
  int rc = m->finalize_trunk("sep_finalize", expected_params(m));
  if (rc) return rc;
  if ((rc = m->pack_gated(m->convs, [](const std::string&) { return std::vector<float>(); }))) return rc;
  const int d = m->enc_cout.back(), H = c.num_head, hd = d / H, BK = c.bottleneck_ksize;
  m->inv_freq = m->P("bottleneck.pe_single.inv_freq");
  m->pe_L = 0;
  m->conf.clear(); m->conf.resize(c.bottleneck_layers);
  m->inter.clear(); m->inter.resize(c.bottleneck_layers);
  for (int l = 0; l < c.bottleneck_layers; ++l) {
    const std::string cl = "bottleneck.module_list." + std::to_string(l) + ".intra.layers.0";
    ConfLayer& q = m->conf[l];
    auto ffn = [&](Ffn& f, const std::string& p) -> int {
      UP(f.lng, m->P(p + ".0.weight")); UP(f.lnb, m->P(p + ".0.bias"));
      UP(f.w1, m->P(p + ".1.ffn.0.weight")); UP(f.b1, m->P(p + ".1.ffn.0.bias"));
      UP(f.w2, scaled(m->P(p + ".1.ffn.3.weight"), 0.5f)); UP(f.b2, scaled(m->P(p + ".1.ffn.3.bias"), 0.5f));
      return ASW_OK;
    };
    if ((rc = ffn(q.f1, cl + ".ffn_module1"))) return rc;
    if ((rc = ffn(q.f2, cl + ".ffn_module2"))) return rc;
    UP(q.n1g, m->P(cl + ".norm1.norm.weight")); UP(q.n1b, m->P(cl + ".norm1.norm.bias"));
    UP(q.n2g, m->P(cl + ".norm2.norm.weight")); UP(q.n2b, m->P(cl + ".norm2.norm.bias"));
    const std::string ce = "bottleneck.module_list." + std::to_string(l) + ".intra.norm.norm";
    UP(q.fng, m->P(ce + ".weight")); UP(q.fnb, m->P(ce + ".bias"));
    {
      // RelPosMHAXL cuts the in_proj output per head into (q, k, v): source row h*3*hd + part*hd + c
      // -> row part*d + h*hd + c of the standard Q | K | V layout the attention kernel reads
      const std::vector<float>& w = m->P(cl + ".mha_layer.in_proj_weight");
      std::vector<float> o(w.size());
      for (int h = 0; h < H; ++h)
        for (int part = 0; part < 3; ++part)
          for (int cc = 0; cc < hd; ++cc)
            memcpy(&o[((size_t)part * d + h * hd + cc) * d], &w[((size_t)h * 3 * hd + part * hd + cc) * d], sizeof(float) * d);
      UP(q.w_in, o);
    }
    UP(q.w_pos, m->P(cl + ".mha_layer.linear_pos.weight"));
    UP(q.w_out, m->P(cl + ".mha_layer.out_proj.weight")); UP(q.b_out, m->P(cl + ".mha_layer.out_proj.bias"));
    // pos_bias_* are stored [hd][H] and read through .view(1,1,H,hd): the flat buffer, head-major
    UP(q.bu, m->P(cl + ".mha_layer.pos_bias_u")); UP(q.bv, m->P(cl + ".mha_layer.pos_bias_v"));
    UP(q.cm_lng, m->P(cl + ".convolution_module.layer_norm.weight"));
    UP(q.cm_lnb, m->P(cl + ".convolution_module.layer_norm.bias"));
    UP(q.cm_pw, m->P(cl + ".convolution_module.bottleneck.0.weight"));       // [2d][d][1] == [2d][d]
    UP(q.cm_pwb, m->P(cl + ".convolution_module.bottleneck.0.bias"));
    {
      const std::vector<float>& w = m->P(cl + ".convolution_module.conv.weight");   // [d][1][BK] -> [BK][d]
      std::vector<float> o((size_t)BK * d);
      for (int cc = 0; cc < d; ++cc)
        for (int k = 0; k < BK; ++k) o[(size_t)k * d + cc] = w[(size_t)cc * BK + k];
      UP(q.dw_wT, o);
    }
    UP(q.dw_b, m->P(cl + ".convolution_module.conv.bias"));
    UP(q.ac_lng, m->P(cl + ".convolution_module.after_conv.0.weight"));
    UP(q.ac_lnb, m->P(cl + ".convolution_module.after_conv.0.bias"));
    UP(q.ac_w, m->P(cl + ".convolution_module.after_conv.2.weight"));
    UP(q.ac_b, m->P(cl + ".convolution_module.after_conv.2.bias"));
    const std::string t = "bottleneck.module_list." + std::to_string(l) + ".inter.layers.0";
    PostNormLayer& il = m->inter[l];
    UP(il.w_in, m->P(t + ".self_attn.in_proj_weight")); UP(il.b_in, m->P(t + ".self_attn.in_proj_bias"));
    UP(il.w_out, m->P(t + ".self_attn.out_proj.weight")); UP(il.b_out, m->P(t + ".self_attn.out_proj.bias"));
    UP(il.w1, m->P(t + ".linear1.weight")); UP(il.b1, m->P(t + ".linear1.bias"));
    UP(il.w2, m->P(t + ".linear2.weight")); UP(il.b2, m->P(t + ".linear2.bias"));
    UP(il.n1g, m->P(t + ".norm1.weight")); UP(il.n1b, m->P(t + ".norm1.bias"));
    UP(il.n2g, m->P(t + ".norm2.weight")); UP(il.n2b, m->P(t + ".norm2.bias"));
  }
  m->finalized = true;
  return ASW_OK;
}

namespace {
// The one inference body.  The B = bounds[G] sequences are the G groups of `bounds`, group g the talkers of mixture
// item[g] of mix [K][M][T] (items ascending): joint statistics and inter-speaker attention per group, everything else
// over all B sequences at once.  The callers have checked the arguments.
int infer_groups(asw_sep* m, const float* mix, int M, int T, const int32_t* offsets, const std::vector<int32_t>& bounds,
                 const std::vector<int32_t>& item, float* out, hipStream_t s) {
  const int B = bounds.back(), G = (int)item.size();
  int rc;
  Plan pl;
  if ((rc = ensure_ws(m, B, T, pl, G))) return rc;
  const int C = m->cfg.channels, pad_l = m->cfg.encoder_kernel_size / 2;
  ASW_HIP(hipMemsetAsync(pl.refn, 0, (size_t)B * pl.RL * sizeof(float), s));
  if ((rc = asw_joint_shift_stats_groups(mix, M, T, offsets, bounds.data(), G, item.data(), pl.jscr, pl.mean, pl.stdv, s)))
    return rc;
  // sequence n reads mixture mix_index[n]; when every one reads mixture 0 no table is needed (and none is copied)
  const int32_t* mix_index = nullptr;
  if (item.back() != 0) {
    std::vector<int32_t> mi;
    for (int g = 0; g < G; ++g) mi.insert(mi.end(), bounds[g + 1] - bounds[g], item[g]);
    // pageable source: the runtime has taken the table before the call returns
    ASW_HIP(hipMemcpyAsync(pl.mix_index, mi.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    mix_index = pl.mix_index;
  }
  if ((rc = asw_shift_norm_preproc_multi(mix, M, T, pl.Tp, offsets, mix_index, B, /*circular*/ 0, pl.mean, pl.stdv, m->pre_w.p,
                                         m->pre_b.p, C, pl.X[0], pl.refn + pad_l, pl.RL, s)))
    return rc;
  pl.G = G;
  pl.bounds = bounds.data();
  return run_network(m, pl, pl.mean, pl.stdv, out, s);
}
}  // namespace

extern "C" int asw_sep_infer(asw_sep* m, const float* mix, int M, int T, const int32_t* offsets, int S, float* out,
                             void* stream) {
  int rc = check_ready(m, "asw_sep_finalize");
  if (rc) return rc;
  ASW_CHECK_ARG(S >= 0 && S <= 64, "sep_infer: S=%d speakers (at most 64 per call)", S);
  if (S == 0) return ASW_OK;
  ASW_CHECK_ARG(mix && offsets && out, "sep_infer: null pointer");
  ASW_CHECK_ARG(M == m->cfg.n_mics, "sep_infer: mixture has %d channels, model expects %d", M, m->cfg.n_mics);
  ASW_CHECK_ARG(T >= 2, "sep_infer: T=%d", T);
  return infer_groups(m, mix, M, T, offsets, {0, S}, {0}, out, asw::as_stream(stream));   // one mixture, one group
}

extern "C" int asw_sep_infer_batch(asw_sep* m, const float* mix, int K, int M, int T, const int32_t* offsets,
                                   const int32_t* counts, float* out, void* stream) {
  int rc = check_ready(m, "asw_sep_finalize");
  if (rc) return rc;
  ASW_CHECK_ARG(K >= 0, "sep_infer_batch: K=%d mixtures", K);
  if (K == 0) return ASW_OK;
  ASW_CHECK_ARG(counts, "sep_infer_batch: null pointer (counts)");
  // the groups: one per item that holds a talker, in order
  std::vector<int32_t> bounds(1, 0), item;
  long N = 0;
  for (int k = 0; k < K; ++k) {
    ASW_CHECK_ARG(counts[k] >= 0 && counts[k] <= 64, "sep_infer_batch: item %d holds %d speakers (0..64)", k, counts[k]);
    N += counts[k];
    if (counts[k] == 0) continue;
    bounds.push_back((int32_t)N);
    item.push_back(k);
  }
  ASW_CHECK_ARG(N <= 64, "sep_infer_batch: %ld sequences (at most 64 per call)", N);
  if (N == 0) return ASW_OK;
  ASW_CHECK_ARG(mix && offsets && out, "sep_infer_batch: null pointer");
  ASW_CHECK_ARG(M == m->cfg.n_mics, "sep_infer_batch: mixtures have %d channels, model expects %d", M, m->cfg.n_mics);
  ASW_CHECK_ARG(T >= 2, "sep_infer_batch: T=%d", T);
  return infer_groups(m, mix, M, T, offsets, bounds, item, out, asw::as_stream(stream));
}

extern "C" int asw_sep_forward(asw_sep* m, const float* mix_norm, int B, int S, int M, int t, float* out, void* stream) {
  return asw_sep_forward_counts(m, mix_norm, B, S, M, t, nullptr, out, stream);
}

extern "C" int asw_sep_forward_counts(asw_sep* m, const float* mix_norm, int B, int S, int M, int t, const int32_t* counts,
                                      float* out, void* stream) {
  int rc = check_ready(m, "asw_sep_finalize");
  if (rc) return rc;
  if (counts) {
    int mx = 0;
    for (int n = 0; n < B; ++n) {
      ASW_CHECK_ARG(counts[n] >= 1 && counts[n] <= S, "sep_forward: item %d holds %d speakers of a %d-wide stack", n, counts[n], S);
      mx = counts[n] > mx ? counts[n] : mx;
    }
    ASW_CHECK_ARG(B == 0 || mx == S, "sep_forward: the stack is %d speakers wide but the largest item holds %d "
                                     "(the reference pads to the largest count, :250-268)", S, mx);
  }
  ASW_CHECK_ARG(B >= 0 && S >= 1 && (long)B * S <= 64, "sep_forward: B=%d S=%d (at most 64 sequences per call)", B, S);
  if (B == 0) return ASW_OK;
  ASW_CHECK_ARG(mix_norm && out, "sep_forward: null pointer");
  ASW_CHECK_ARG(M == m->cfg.n_mics && t >= 1, "sep_forward: bad shape");
  hipStream_t s = asw::as_stream(stream);
  Plan pl;
  const int BS = B * S;
  if ((rc = ensure_ws(m, BS, t, pl))) return rc;
  const int C = m->cfg.channels, pad_l = m->cfg.encoder_kernel_size / 2;
  ASW_HIP(hipMemsetAsync(pl.refn, 0, (size_t)BS * pl.RL * sizeof(float), s));
  // [B][S*M][t] is [B*S][M][t]: every speaker block of M channels is one sequence (:436-437)
  if ((rc = asw_pad_preproc(mix_norm, BS, M, t, pl.Tp, m->pre_w.p, m->pre_b.p, C, pl.X[0], pl.refn + pad_l, pl.RL, s))) return rc;
  // the reference channel of an item is the FIRST channel of its stack (:430): give every
  // speaker of item b the padded channel 0 of sequence (b, 0)
  for (int sp = 1; sp < S; ++sp)
    ASW_HIP(hipMemcpy2DAsync(pl.refn + (size_t)sp * pl.RL, (size_t)S * pl.RL * sizeof(float), pl.refn,
                             (size_t)S * pl.RL * sizeof(float), (size_t)pl.RL * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  pl.G = B; pl.S = S;                       // every item is one group, as wide as the stack
  pl.counts = counts;
  if ((rc = run_network(m, pl, nullptr, nullptr, pl.ywave, s))) return rc;
  if (counts) {
    // a missing speaker has a zero mask, so its output is the bare output_decoder bias (:474-484)
    uint32_t bits;
    memcpy(&bits, &m->out_bias, sizeof bits);
    for (int n = 0; n < B; ++n)
      if (counts[n] < S)
        ASW_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pl.ywave + ((size_t)n * S + counts[n]) * t), (int)bits,
                                  (size_t)(S - counts[n]) * t, s));
  }
  // rows padded with zeros to max_speakers (:486-488)
  const int R = S > m->cfg.max_speakers ? S : m->cfg.max_speakers;
  ASW_HIP(hipMemsetAsync(out, 0, (size_t)B * R * t * sizeof(float), s));
  ASW_HIP(hipMemcpy2DAsync(out, (size_t)R * t * sizeof(float), pl.ywave, (size_t)S * t * sizeof(float),
                           (size_t)S * t * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  return ASW_OK;
}

extern "C" int asw_sep_get_config(const asw_sep* m, asw_sep_config* out) {
  ASW_CHECK_ARG(m && out, "sep_get_config: null pointer");
  *out = m->cfg;
  return ASW_OK;
}

extern "C" int asw_sep_get_tap(asw_sep* m, const char* name, float* dst, size_t capacity, size_t* numel, void* stream) {
  return get_tap(m, "sep_get_tap", name, dst, capacity, numel, stream);
}
