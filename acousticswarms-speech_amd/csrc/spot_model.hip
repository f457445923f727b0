// spot_model.hip -- device-resident spot network: weight packing + the layer schedule of
// Network.forward (sep/training/SpeakerLocalization/network.py:363-405) and of the
// candidate hot loop DataParallelSpotModel.shift_and_sep
// (sep/training/JointModel/network.py:37-104), expressed as launches of the kernels in
// prep_kernels.hip / convgemm.hip / misc_kernels.hip on one HIP stream.
//
// Data layout in HBM: every activation is channels-last [B][T_l][C] fp32, so a
// LayerNorm row, a GLU pair and a GEMM A-row are each contiguous.  Weights are packed
// once (finalize) as Wt[N][tap*Cin + c]; the window gate of an encoder/decoder block
// (embed1, network.py:101,186) is folded into the adjacent convolution's weights per
// window embedding, so it costs nothing at run time.
//
// The U-Net trunk around the transformer is model_common.h's Trunk; this file holds the
// transformer bottleneck, the window gates, the workspace policy and the C entry points.
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "model_common.h"

using namespace asw_model;

namespace {

// the gated convolutions of one window embedding
struct GateSet : GatedConvs { uint64_t stamp = 0; };   // stamp: last use (LRU eviction)

}  // namespace

struct asw_spot : Trunk {
  asw_spot_config cfg;
  int batch = 32;
  uint64_t clock = 0;
  std::vector<PostNormLayer> tf;
  std::map<std::pair<float, float>, std::unique_ptr<GateSet>> gates;

  // workspace: one arena per lane.  With two lanes consecutive internal batches run on two HIP
  // streams (the caller's and a side stream), so the memory-bound passes and the launch tails of
  // one batch overlap the MFMA kernels of the other.
  char* ws[2] = {nullptr, nullptr};
  size_t ws_bytes[2] = {0, 0};
  int lanes = 1;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  asw_spot() { want_src = true; want_up = true; }
  ~asw_spot() {
    for (char* w : ws) if (w) (void)hipFree(w);
    if (side) (void)hipStreamDestroy(side);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
  }
};

namespace {

// the trunk's keys, then the window gates (embed1) and the transformer
ParamList expected_params(const asw_spot* m) {
  const asw_spot_config& c = m->cfg;
  ParamList v = m->trunk_params();
  for (int i = 0; i < c.depth; ++i) {
    const std::string p = "encoder.module_list." + std::to_string(i);
    v.push_back({p + ".embed1.weight", (size_t)m->enc_cin[i] * 2});
    v.push_back({p + ".embed1.bias", (size_t)m->enc_cin[i]});
  }
  for (int i = 0; i < c.depth; ++i) {
    const std::string p = "decoder.module_list." + std::to_string(i);
    v.push_back({p + ".embed1.weight", (size_t)2 * m->dec_cout[i] * 2});
    v.push_back({p + ".embed1.bias", (size_t)2 * m->dec_cout[i]});
  }
  const size_t d = m->enc_cout.back(), f = c.ffw_dim;
  for (int l = 0; l < c.num_transformer_layers; ++l) {
    const std::string p = "bottleneck.transf.layers." + std::to_string(l);
    v.push_back({p + ".self_attn.in_proj_weight", 3 * d * d});
    v.push_back({p + ".self_attn.in_proj_bias", 3 * d});
    v.push_back({p + ".self_attn.out_proj.weight", d * d});
    v.push_back({p + ".self_attn.out_proj.bias", d});
    v.push_back({p + ".linear1.weight", f * d});
    v.push_back({p + ".linear1.bias", f});
    v.push_back({p + ".linear2.weight", d * f});
    v.push_back({p + ".linear2.bias", d});
    v.push_back({p + ".norm1.weight", d});
    v.push_back({p + ".norm1.bias", d});
    v.push_back({p + ".norm2.weight", d});
    v.push_back({p + ".norm2.bias", d});
  }
  return v;
}

// gate[c] = W[c][0]*w0 + W[c][1]*w1 + b[c]   (embed1 is Conv1d(2->C, k=1))
std::vector<float> gate_of(const std::vector<float>& w, const std::vector<float>& b, float w0, float w1) {
  std::vector<float> g(b.size());
  for (size_t c = 0; c < b.size(); ++c) g[c] = w[2 * c] * w0 + w[2 * c + 1] * w1 + b[c];
  return g;
}

int get_gates(asw_spot* m, float w0, float w1, GateSet** out) {
  auto key = std::make_pair(w0, w1);
  auto it = m->gates.find(key);
  if (it != m->gates.end()) { it->second->stamp = ++m->clock; *out = it->second.get(); return ASW_OK; }
  if (m->gates.size() >= 8) {
    // bounded cache: drop the least recently used set.  Launches that read it may still be queued;
    // its buffers are released with hipFree, which waits for the device, so they finish first.
    auto lru = m->gates.begin();
    for (auto g = m->gates.begin(); g != m->gates.end(); ++g)
      if (g->second->stamp < lru->second->stamp) lru = g;
    m->gates.erase(lru);
  }
  std::unique_ptr<GateSet> gs(new GateSet());
  gs->stamp = ++m->clock;
  int rc = m->pack_gated(*gs, [&](const std::string& p) {
    return gate_of(m->P(p + ".embed1.weight"), m->P(p + ".embed1.bias"), w0, w1);
  });
  if (rc) return rc;
  *out = gs.get();
  m->gates[key] = std::move(gs);
  return ASW_OK;
}

struct Plan : TrunkPlan {
  float *qkv, *ctx, *x1, *ff, *ha, *hb;
};

void layout(const asw_spot* m, int B, int T, Arena& a, Plan& pl) {
  m->layout_levels(B, T, a, pl);
  const size_t L = pl.Tl[m->cfg.depth], d = m->enc_cout.back(), rows = (size_t)B * L;
  pl.qkv = a.take<float>(rows * 3 * d);
  pl.ctx = a.take<float>(rows * d);
  pl.x1 = a.take<float>(rows * d);
  pl.ff = a.take<float>(rows * m->cfg.ffw_dim);
  pl.ha = a.take<float>(rows * d);
  pl.hb = a.take<float>(rows * d);
  m->layout_mask(a, pl);
}

int ensure_ws(asw_spot* m, int B, int T, Plan& pl, int lane = 0) {
  Arena dry(nullptr, 0, true);
  layout(m, B, T, dry, pl);
  const size_t need = dry.off + 4096;
  if (need > m->ws_bytes[lane]) {
    // A workspace that has to grow grows to the model's full internal batch at once: a search issues calls of 30,
    // then 50 ... 256 candidates, and every growth is a device synchronisation plus a hipFree / hipMalloc of tens of
    // GB (about 0.2 GB per candidate at T = 48 000) -- 2-3 s each in the kernel trace of the 64-mixture run.
    size_t want = need;
    if (B < m->batch) {
      Plan full;
      Arena dry_full(nullptr, 0, true);
      layout(m, m->batch, T, dry_full, full);
      want = dry_full.off + 4096;
    }
    if (m->ws[lane]) { ASW_HIP(hipDeviceSynchronize()); (void)hipFree(m->ws[lane]); m->ws[lane] = nullptr; m->ws_bytes[lane] = 0; }
    if (hipMalloc(&m->ws[lane], want) != hipSuccess) {
      (void)hipGetLastError();
      want = need;                                         // not enough memory for the full batch: what this call needs
      if (hipMalloc(&m->ws[lane], want) != hipSuccess)
        return asw::set_error(ASW_ERR_NOMEM, "workspace of %.1f MiB for batch %d, T=%d", need / 1048576.0, B, T);
    }
    m->ws_bytes[lane] = want;
  }
  Arena real(m->ws[lane], m->ws_bytes[lane], false);
  layout(m, B, T, real, pl);
  return ASW_OK;
}

// everything after the preproc stage; pl.X[0] (src0: the source planes instead) / pl.refn are filled
// cand: the candidate loop (the decoder may feed its 64 -> 64 block from the stack in front, Trunk::decode)
int run_network(asw_spot* m, Plan& pl, GateSet* gs, const float* mean, const float* stdv, float* out_wave,
                hipStream_t s, bool src0 = false, bool cand = false) {
  const asw_spot_config& c = m->cfg;
  int rc;
  if ((rc = m->encode(pl, *gs, s, src0))) return rc;
  // ---- bottleneck (network.py:240-265): post-norm transformer layers, batch-first rows
  const int L = pl.Tl[c.depth], d = m->enc_cout.back(), rows = pl.B * L;
  const float* h = pl.X[c.depth];
  // h is a GroupNorm + GLU / LayerNorm output; the attention reads qkv, a Raw operand (Trunk::site)
  const int rawp = m->site(Trunk::Src::Raw);
  auto attention = [&](const float* qkv, float* ctx) { return asw_attention_prec(qkv, pl.B, L, d, c.num_head, rawp, ctx, s); };
  for (int l = 0; l < c.num_transformer_layers; ++l) {
    float* hout = (l % 2 == 0) ? pl.ha : pl.hb;
    if ((rc = run_post_norm(*m, m->tf[l], {pl.qkv, pl.ctx, pl.x1, pl.ff}, h, hout, rows, d, c.ffw_dim, attention, s))) return rc;
    h = hout;
  }
  m->taps["bottleneck"] = {h, (size_t)rows * d};
  if ((rc = m->decode(pl, *gs, h, s, cand))) return rc;
  return m->mask_path(pl, h, mean, stdv, out_wave, s);
}

}  // namespace

extern "C" int asw_spot_create(const asw_spot_config* cfg, asw_spot** out) {
  ASW_CHECK_ARG(cfg && out, "spot_create: null pointer");
  const asw_spot_config& c = *cfg;
  const TrunkCfg tc = TrunkCfg::of(c);
  int rc = check_trunk_config(tc, "spot_create", "kernel_size must be odd");
  if (rc) return rc;
  ASW_CHECK_ARG(c.num_transformer_layers >= 0, "spot_create: bad config");
  std::unique_ptr<asw_spot> m(new asw_spot());
  m->cfg = c;
  if ((rc = m->init_shape(tc, "spot_create"))) return rc;
  const int d = m->enc_cout.back();
  ASW_CHECK_ARG(d <= 1024 && (d & (d - 1)) == 0, "spot_create: bottleneck width %d must be a power of two <= 1024", d);
  ASW_CHECK_ARG(d % c.num_head == 0 && (d / c.num_head) % 16 == 0 && d / c.num_head <= 128,
                "spot_create: head_dim %d unsupported", d / (c.num_head ? c.num_head : 1));
  if ((rc = m->check_level_widths("spot_create"))) return rc;
  *out = m.release();
  return ASW_OK;
}

extern "C" void asw_spot_destroy(asw_spot* m) { delete m; }

extern "C" int asw_spot_set_precision(asw_spot* m, int precision) { return set_precision(m, "set_precision", precision); }

extern "C" int asw_spot_set_batch(asw_spot* m, int batch) {
  ASW_CHECK_ARG(m && batch >= 1 && batch <= 4096, "set_batch: bad argument");
  m->batch = batch;
  return ASW_OK;
}

extern "C" int asw_spot_set_param(asw_spot* m, const char* key, const float* host_data, size_t numel) {
  return set_param(m, "set_param", key, host_data, numel);
}

extern "C" int asw_spot_finalize(asw_spot* m) {
  ASW_CHECK_ARG(m, "finalize: null handle");
  const asw_spot_config& c = m->cfg;
  int rc = m->finalize_trunk("finalize", expected_params(m));
  if (rc) return rc;
  m->tf.clear(); m->tf.resize(c.num_transformer_layers);
  for (int l = 0; l < c.num_transformer_layers; ++l) {
    const std::string p = "bottleneck.transf.layers." + std::to_string(l);
    PostNormLayer& t = m->tf[l];
    {
      const int dm = m->enc_cout.back(), ff = c.ffw_dim;
      if ((rc = t.w_in.upload_gemm(m->P(p + ".self_attn.in_proj_weight"), 3 * dm, dm))) return rc;
      if ((rc = t.w_out.upload_gemm(m->P(p + ".self_attn.out_proj.weight"), dm, dm))) return rc;
      if ((rc = t.w1.upload_gemm(m->P(p + ".linear1.weight"), ff, dm))) return rc;
      if ((rc = t.w2.upload_gemm(m->P(p + ".linear2.weight"), dm, ff))) return rc;
    }
    UP(t.b_in, m->P(p + ".self_attn.in_proj_bias"));
    UP(t.b_out, m->P(p + ".self_attn.out_proj.bias"));
    UP(t.b1, m->P(p + ".linear1.bias"));
    UP(t.b2, m->P(p + ".linear2.bias"));
    UP(t.n1g, m->P(p + ".norm1.weight")); UP(t.n1b, m->P(p + ".norm1.bias"));
    UP(t.n2g, m->P(p + ".norm2.weight")); UP(t.n2b, m->P(p + ".norm2.bias"));
  }
  m->gates.clear();
  m->finalized = true;
  return ASW_OK;
}

extern "C" int asw_spot_shift_and_sep(asw_spot* m, const float* mix, int M, int T, const int32_t* offsets, int N,
                                      int strict, int circular, float* out_wave, double* out_energy,
                                      int energy_window, void* stream) {
  return asw_spot_shift_and_sep_multi(m, mix, 1, M, T, offsets, nullptr, N, strict, circular, out_wave, out_energy,
                                      energy_window, stream);
}

extern "C" int asw_spot_shift_and_sep_multi(asw_spot* m, const float* mix, int K, int M, int T, const int32_t* offsets,
                                            const int32_t* mix_index, int N, int strict, int circular, float* out_wave,
                                            double* out_energy, int energy_window, void* stream) {
  int rc = check_ready(m, "asw_spot_finalize");
  ASW_CHECK_ARG(K >= 1 && (K == 1 || mix_index != nullptr), "shift_and_sep: K=%d mixtures need a mix_index array", K);
  if (rc) return rc;
  ASW_CHECK_ARG(N >= 0, "shift_and_sep: N=%d", N);
  if (N == 0) return ASW_OK;
  ASW_CHECK_ARG(mix && offsets, "shift_and_sep: null pointer");
  ASW_CHECK_ARG(M == m->cfg.n_mics, "shift_and_sep: mixture has %d channels, model expects %d", M, m->cfg.n_mics);
  ASW_CHECK_ARG(T >= 2, "shift_and_sep: T=%d", T);
  ASW_CHECK_ARG(out_energy == nullptr || energy_window > 0, "shift_and_sep: energy_window");
  hipStream_t s = asw::as_stream(stream);
  GateSet* gs = nullptr;
  if ((rc = get_gates(m, strict == 1 ? 1.f : 0.f, strict == 1 ? 0.f : 1.f, &gs))) return rc;
  const int Bmax = N < m->batch ? N : m->batch;
  const int n_batches = (N + Bmax - 1) / Bmax;
  const int lanes = (m->lanes == 2 && n_batches >= 2) ? 2 : 1;
  Plan pl[2];
  for (int l = 0; l < lanes; ++l)
    if ((rc = ensure_ws(m, Bmax, T, pl[l], l))) return rc;
  hipStream_t st[2] = {s, s};
  if (lanes == 2) {
    if (!m->side) {
      ASW_HIP(hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
      ASW_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
      ASW_HIP(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
    }
    st[1] = m->side;
    ASW_HIP(hipEventRecord(m->ev_fork, s));                // the side lane starts after everything queued before this call
    ASW_HIP(hipStreamWaitEvent(m->side, m->ev_fork, 0));
  }
  const int C = m->cfg.channels, pad_l = m->cfg.encoder_kernel_size / 2;
  const bool src0 = m->src_path();
  // The caller's stream continues after BOTH lanes on every exit path: when a launch fails half way the side
  // lane may still be writing out_wave / out_energy (the caller's buffers), so the join is not skipped -- and if
  // the join itself cannot be queued the side lane is drained before the status is returned.
  auto batches = [&]() -> int {
    int k = 0;
    for (int i0 = 0; i0 < N; i0 += Bmax, ++k) {
      const int B = N - i0 < Bmax ? N - i0 : Bmax;
      Plan& p = pl[k % lanes];
      hipStream_t q = st[k % lanes];
      p.B = B;
      const int32_t* off = offsets + (size_t)i0 * (M - 1);
      const int32_t* mi = mix_index ? mix_index + i0 : nullptr;
      ASW_HIP(hipMemsetAsync(p.refn, 0, (size_t)B * p.RL * sizeof(float), q));
      int r;
      if ((r = asw_shift_stats_multi(mix, M, T, off, mi, B, circular, p.mean, p.stdv, q))) return r;
      if (src0) {
        // preproc folded into encoder block 0's first layer: the 8-channel input goes out, X[0] is never written
        if ((r = asw_shift_norm_src_multi(mix, M, T, p.Tp, off, mi, B, circular, p.mean, p.stdv, p.src_hi, p.src_lo,
                                          p.refn + pad_l, p.RL, q)))
          return r;
      } else if ((r = asw_shift_norm_preproc_multi(mix, M, T, p.Tp, off, mi, B, circular, p.mean, p.stdv, m->pre_w.p,
                                                   m->pre_b.p, C, p.X[0], p.refn + pad_l, p.RL, q))) {
        return r;
      }
      float* y = out_wave ? out_wave + (size_t)i0 * T : p.ywave;
      if ((r = run_network(m, p, gs, p.mean, p.stdv, y, q, src0, true))) return r;
      if (out_energy && (r = asw_energies(y, B, T, energy_window, nullptr, out_energy + (size_t)i0 * 2, q))) return r;
    }
    return ASW_OK;
  };
  rc = batches();
  if (lanes == 2) {
    if (hipEventRecord(m->ev_join, m->side) != hipSuccess || hipStreamWaitEvent(s, m->ev_join, 0) != hipSuccess) {
      (void)hipStreamSynchronize(m->side);
      if (!rc) rc = asw::set_error(ASW_ERR_HIP, "shift_and_sep: joining the side lane failed");
    }
  }
  return rc;
}

extern "C" int asw_spot_set_lanes(asw_spot* m, int lanes) {
  ASW_CHECK_ARG(m && (lanes == 1 || lanes == 2), "set_lanes: 1 or 2");
  m->lanes = lanes;
  return ASW_OK;
}

extern "C" int asw_spot_forward(asw_spot* m, const float* mix_norm, int B, int M, int t,
                                const float* window_embedding_host, float* out, void* stream) {
  int rc = check_ready(m, "asw_spot_finalize");
  if (rc) return rc;
  ASW_CHECK_ARG(B >= 0, "forward: B=%d", B);
  if (B == 0) return ASW_OK;
  ASW_CHECK_ARG(mix_norm && window_embedding_host && out, "forward: null pointer");
  ASW_CHECK_ARG(M == m->cfg.n_mics && t >= 1, "forward: bad shape");
  hipStream_t s = asw::as_stream(stream);
  GateSet* gs = nullptr;
  if ((rc = get_gates(m, window_embedding_host[0], window_embedding_host[1], &gs))) return rc;
  const int Bmax = B < m->batch ? B : m->batch;
  Plan pl;
  if ((rc = ensure_ws(m, Bmax, t, pl))) return rc;
  const int C = m->cfg.channels, pad_l = m->cfg.encoder_kernel_size / 2;
  for (int i0 = 0; i0 < B; i0 += Bmax) {
    const int b = B - i0 < Bmax ? B - i0 : Bmax;
    pl.B = b;
    ASW_HIP(hipMemsetAsync(pl.refn, 0, (size_t)b * pl.RL * sizeof(float), s));
    if ((rc = asw_pad_preproc(mix_norm + (size_t)i0 * M * t, b, M, t, pl.Tp, m->pre_w.p, m->pre_b.p, C, pl.X[0],
                              pl.refn + pad_l, pl.RL, s)))
      return rc;
    if ((rc = run_network(m, pl, gs, nullptr, nullptr, out + (size_t)i0 * t, s))) return rc;
  }
  return ASW_OK;
}

extern "C" int asw_spot_set_fused_mask(asw_spot* m, int on) {
  ASW_CHECK_ARG(m, "set_fused_mask: null model handle");
  m->fuse_mask = on != 0;
  return ASW_OK;
}

extern "C" int asw_spot_set_source_stack(asw_spot* m, int on) {
  ASW_CHECK_ARG(m, "set_source_stack: null model handle");
  m->src_stack = on != 0;
  return ASW_OK;
}

extern "C" int asw_spot_set_up_fusion(asw_spot* m, int on) {
  ASW_CHECK_ARG(m, "set_up_fusion: null model handle");
  m->up_fusion = on != 0;
  return ASW_OK;
}

extern "C" int asw_spot_get_tap(asw_spot* m, const char* name, float* dst, size_t capacity, size_t* numel,
                                void* stream) {
  return get_tap(m, "get_tap", name, dst, capacity, numel, stream);
}
