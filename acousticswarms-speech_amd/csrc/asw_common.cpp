#include "asw_common.h"

#include <cmath>
#include <cstdlib>

namespace asw {
char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}
int SmemAttr::ensure(const void* kern, size_t want) {
  int dev = 0;
  ASW_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDev) return set_error(ASW_ERR_ARG, "device ordinal %d out of range", dev);
  if (bytes[dev] >= want) return ASW_OK;
  ASW_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
  bytes[dev] = want;
  return ASW_OK;
}
}  // namespace asw

extern "C" const char* asw_last_error(void) { return asw::err_buf(); }
extern "C" int asw_abi_version(void) { return 3; }   // 2: + joint separation network (asw_sep_*); 3: + asw_resstack64_f16x3
                                                     // (asw_residue_schedule is an addition: no bump)

// ---- host-side weight preparation of the f16x3 kernels (layout: f16x3_tile.h) ------------
extern "C" int asw_split_weights_f16(const float* w, size_t n, uint16_t* hi, uint16_t* lo, int32_t* w_shift) {
  ASW_CHECK_ARG(w && hi && lo && w_shift, "split_weights: null pointer");
  float mx = 0.f;
  // (a NaN compares false with everything: it has to be carried into mx by hand to reach the check below)
  for (size_t i = 0; i < n; ++i) { const float a = w[i] < 0 ? -w[i] : w[i]; if (a > mx || a != a) mx = a; }
  ASW_CHECK_ARG(mx == mx && mx < 3.0e38f, "split_weights: non-finite weight");
  // largest power of two with max|w| * 2^shift < 2048 (fp16 keeps 11 significant bits there and
  // typical weights, 10-100x below the maximum, still have normal lo parts); bounded to +-24.
  int shift = 0;
  if (mx > 0.f) {
    int e;
    (void)frexpf(mx, &e);                  // mx = f * 2^e, f in [0.5,1)
    shift = 11 - e;
    if (shift > 24) shift = 24;
    if (shift < -24) shift = -24;
  }
  const float sc = ldexpf(1.0f, shift);
  for (size_t i = 0; i < n; ++i) {
    float c = w[i] * sc;
    if (c > 65504.f) c = 65504.f;
    if (c < -65504.f) c = -65504.f;
    const _Float16 h = (_Float16)c;
    const _Float16 l = (_Float16)(c - (float)h);
    memcpy(hi + i, &h, 2);
    memcpy(lo + i, &l, 2);
  }
  *w_shift = shift;
  return ASW_OK;
}

extern "C" int asw_pack_fragments_f16(const float* Wt, int N, int K, uint16_t* hi, uint16_t* lo, int32_t* w_shift) {
  ASW_CHECK_ARG(Wt && hi && lo && w_shift, "pack_fragments: null pointer");
  ASW_CHECK_ARG(N > 0 && K > 0 && N % 32 == 0 && K % 16 == 0, "pack_fragments: N %% 32, K %% 16 required (N=%d K=%d)", N, K);
  const size_t n = (size_t)N * K;
  uint16_t* th = new uint16_t[2 * n];
  uint16_t* tl = th + n;
  int rc = asw_split_weights_f16(Wt, n, th, tl, w_shift);
  if (rc == ASW_OK) {
    const int NT = N / 32;
    for (int ks = 0; ks < K / 16; ++ks)
      for (int nt = 0; nt < NT; ++nt)
        for (int l = 0; l < 64; ++l) {
          const size_t src = (size_t)(nt * 32 + (l & 31)) * K + ks * 16 + 8 * (l >> 5);
          const size_t dst = (((size_t)ks * NT + nt) * 64 + l) * 8;
          memcpy(hi + dst, th + src, 16);
          memcpy(lo + dst, tl + src, 16);
        }
  }
  delete[] th;
  return rc;
}

// UpFeed (resstack.hip): register 8 s + j of a 32 x 32 accumulator block, lane half h, is its row 16 s + 8 (j >> 2) + 4 h +
// (j & 3), and as an MFMA operand that register is k = 8 h + j of k-step s
extern "C" int asw_up_feed_kperm(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }

extern "C" int asw_pack_up_feed_f16(const float* Wt, int N, int K, uint16_t* hi, uint16_t* lo, int32_t* w_shift) {
  ASW_CHECK_ARG(Wt && N > 0 && K > 0 && K % 16 == 0, "pack_up_feed: K %% 16 required (N=%d K=%d)", N, K);
  float* wp = new float[(size_t)N * K];
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) wp[(size_t)n * K + k] = Wt[(size_t)n * K + (k & ~15) + asw_up_feed_kperm(k & 15)];
  const int rc = asw_pack_fragments_f16(wp, N, K, hi, lo, w_shift);
  delete[] wp;
  return rc;
}

// ---- residue-image A feed: the residue walk of pipe_mainloop, enumerated on the host ----
namespace asw {
bool residue_feed_on() {                  // like ASW_NO_RESSTACK: set to anything, "0" included, means off
  static const bool off = getenv("ASW_NO_RESIDUE_FEED") != nullptr;
  return !off;
}
}  // namespace asw

extern "C" int asw_residue_schedule(int taps, int stride, int dil, int pad, int Cin, int BK, int BM, int m0, int has_skip,
                                    asw_residue_stage* out, int cap, int* n_stages, int* max_shift) {
  ASW_CHECK_ARG(n_stages != nullptr && cap >= 0 && (out != nullptr || cap == 0), "residue_schedule: null pointer");
  ASW_CHECK_ARG(taps > 0 && stride > 0 && dil > 0 && Cin > 0 && BK > 0 && BM > 0, "residue_schedule: bad dims");
  *n_stages = 0;
  if (max_shift) *max_shift = 0;
  if (!asw::residue_feed_applies(taps, stride, dil, Cin, BK, has_skip != 0)) return ASW_OK;
  const asw::ResidueFeed rf{taps, stride, Cin / BK};
  ASW_CHECK_ARG(rf.ntaps(0) <= ASW_RESIDUE_MAX_TAPS, "residue_schedule: %d taps on one image, at most %d", rf.ntaps(0),
                ASW_RESIDUE_MAX_TAPS);
  *n_stages = rf.stages();
  if (max_shift) *max_shift = rf.shifts(0);
  for (int s = 0; s < rf.stages() && s < cap; ++s) {
    asw_residue_stage& d = out[s];
    memset(&d, 0, sizeof d);
    d.residue = s / rf.cpb;
    d.chunk = s - d.residue * rf.cpb;
    d.rows = BM + rf.shifts(d.residue);
    d.first_row = m0 * stride - pad + d.residue;
    d.ntaps = rf.ntaps(d.residue);
    for (int q = 0; q < d.ntaps; ++q) {
      d.tap[q] = rf.tap(d.residue, q);
      d.shift[q] = q;
      d.kstep[q] = rf.kstep(d.tap[q], d.chunk, BK / 16);
    }
  }
  return ASW_OK;
}

// ---- launch profiler -----------------------------------------------------------------
#include <map>
#include <mutex>
#include <vector>
namespace asw {
namespace {
struct Rec { std::string name; double work, bytes; hipEvent_t e0, e1; };
std::mutex g_mu;
bool g_on = false;
bool g_detail = false;
bool g_form = true;
std::vector<Rec> g_recs;
std::vector<hipEvent_t> g_pool;
hipEvent_t take_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace

std::string prof_name(const char* base, int bm, int bn, int bk, bool ln, bool stats) {
  char b[96];
  snprintf(b, sizeof b, "%s<%d,%d,%d,%s>", base, bm, bn, bk, ln ? "ln" : stats ? "stats" : "plain");
  return b;
}
bool prof_detail() { return g_detail; }
bool prof_form() { return g_form; }
ProfScope::ProfScope(hipStream_t s, const std::string& name, double work, double bytes) : slot(-1), stream(s) {
  if (!g_on) return;
  std::lock_guard<std::mutex> lk(g_mu);
  Rec r{name, work, bytes, take_event(), take_event()};
  (void)hipEventRecord(r.e0, s);
  g_recs.push_back(r);
  slot = (int)g_recs.size() - 1;
}
ProfScope::~ProfScope() {
  if (slot < 0) return;
  std::lock_guard<std::mutex> lk(g_mu);
  if (slot < (int)g_recs.size()) (void)hipEventRecord(g_recs[slot].e1, stream);
}
}  // namespace asw

extern "C" int asw_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(asw::g_mu);
  for (auto& r : asw::g_recs) { asw::g_pool.push_back(r.e0); asw::g_pool.push_back(r.e1); }
  asw::g_recs.clear();
  asw::g_on = on != 0;
  asw::g_detail = on == 2 || on == 3;      // 2, 3: GEMM launch names carry their shape
  asw::g_form = on != 2;                   // 2 alone leaves out the tiling form (prof_form)
  return ASW_OK;
}

extern "C" int asw_profile_report(char* buf, size_t cap) {
  if (!buf || cap < 64) return asw::set_error(ASW_ERR_ARG, "profile_report: buffer too small");
  std::lock_guard<std::mutex> lk(asw::g_mu);
  struct Agg { long n = 0; double ms = 0, work = 0, bytes = 0; };
  std::map<std::string, Agg> agg;
  for (auto& r : asw::g_recs) {
    if (hipEventSynchronize(r.e1) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    Agg& a = agg[r.name];
    a.n += 1; a.ms += ms; a.work += r.work; a.bytes += r.bytes;
  }
  size_t off = 0;
  off += snprintf(buf + off, cap - off, "{");
  bool first = true;
  for (auto& kv : agg) {
    if (off + 256 >= cap) break;
    off += snprintf(buf + off, cap - off, "%s\"%s\":{\"launches\":%ld,\"ms\":%.6f,\"work\":%.6e,\"bytes\":%.6e}", first ? "" : ",",
                    kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.work, kv.second.bytes);
    first = false;
  }
  snprintf(buf + off, cap - off, "}");
  return ASW_OK;
}
