// Shared host-side helpers for libasw_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/asw_hip.h"

namespace asw {

// thread-local error message returned by asw_last_error()
char* err_buf();
int set_error(int code, const char* fmt, ...);

#define ASW_CHECK_ARG(cond, ...)                                   \
  do {                                                             \
    if (!(cond)) return ::asw::set_error(ASW_ERR_ARG, __VA_ARGS__); \
  } while (0)

#define ASW_HIP(call)                                                                 \
  do {                                                                                \
    hipError_t _e = (call);                                                           \
    if (_e != hipSuccess)                                                             \
      return ::asw::set_error(ASW_ERR_HIP, "%s failed: %s (%s:%d)", #call,            \
                              hipGetErrorString(_e), __FILE__, __LINE__);             \
  } while (0)

#define ASW_LAUNCH_CHECK()                                                            \
  do {                                                                                \
    hipError_t _e = hipGetLastError();                                                \
    if (_e != hipSuccess)                                                             \
      return ::asw::set_error(ASW_ERR_HIP, "kernel launch failed: %s (%s:%d)",        \
                              hipGetErrorString(_e), __FILE__, __LINE__);             \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel.  One
// SmemAttr per launch site remembers the largest size already set on each device, so a process
// that serves several GPUs (SpotModel.to("cuda:1"), one stream per device) sets it on each.
struct SmemAttr {
  static constexpr int kMaxDev = 64;
  size_t bytes[kMaxDev] = {};
  int ensure(const void* kern, size_t want);     // 0 or a negative asw_status
};
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- residue-image A feed (include/asw_hip.h: asw_residue_schedule).  The formulae of the schedule, written once:
// the host enumeration (asw_common.cpp) and the device loop (pipe_mainloop, pipegemm.hip) both go through them.
#ifdef __HIPCC__
#define ASW_HOST_DEVICE __host__ __device__
#else
#define ASW_HOST_DEVICE
#endif
struct ResidueFeed {
  int taps, stride, cpb;                                   // cpb = Cin / BK chunks per tap
  ASW_HOST_DEVICE int stages() const { return stride * cpb; }                           // stage = r * cpb + c
  ASW_HOST_DEVICE int shifts(int r) const { return (taps - 1 - r) / stride; }           // rows of image r beyond BM
  ASW_HOST_DEVICE int ntaps(int r) const { return shifts(r) + 1; }                      // taps r, r + stride, ...
  ASW_HOST_DEVICE int tap(int r, int q) const { return r + q * stride; }
  // first k-step (16 K each, KS = BK / 16 per chunk) of (tap, chunk c) in the packed fragment-order weights
  ASW_HOST_DEVICE int kstep(int tap, int c, int KS) const { return (tap * cpb + c) * KS; }
};
inline bool residue_feed_applies(int taps, int stride, int dil, int Cin, int BK, bool skip) {
  return dil == 1 && stride >= 2 && taps > stride && BK > 0 && BK % 16 == 0 && Cin > 0 && Cin % BK == 0 && !skip;
}
bool residue_feed_on();                                    // false when ASW_NO_RESIDUE_FEED is set, to any value (read once)
// What every launch of a pipelined tile (pipegemm.hip) asks beside a_len < 2^29: the element offsets of its A operand
// (ResidueA, f16x3_tile.h) are 32-bit.  Past a_len a tile forms offsets of up to BM + ASW_RESIDUE_MAX_SHIFT + NT / KV
// (= 64) frames of `stride` rows, and the chunk walk adds up to taps * dil rows for the tap: with each product below
// 2^20 the sum stays below 2^30.  A convolution beyond these goes to the two-barrier 256 x 256 tile (64-bit offsets);
// the mask path, which has no other kernel, refuses it.  No model comes near them.
inline bool pipe_offsets_ok(const asw_convgemm_args& a) {
  return (int64_t)a.stride * a.a_row_stride < (1 << 20) && (int64_t)a.pad * a.a_row_stride < (1 << 20) &&
         (int64_t)a.taps * a.dil * a.a_row_stride < (1 << 20);
}
// what the pipelined tiles ask before they take the residue walk: their ring has ASW_RESIDUE_MAX_SHIFT rows beyond BM
// per image (every other shape, or every shape under ASW_NO_RESIDUE_FEED, takes the chunk walk)
inline bool residue_feed_ok(const asw_convgemm_args& a, int BK) {
  return residue_feed_on() && residue_feed_applies(a.taps, a.stride, a.dil, a.Cin, BK, a.A2 != nullptr) &&
         (a.taps - 1) / a.stride <= ASW_RESIDUE_MAX_SHIFT;
}

#ifdef __HIPCC__
// GroupNorm(2) + GLU of one (value, gate) pair: (a - m0) r0 ga + ba, gated by the sigmoid of the normalised
// gate.  One definition with every rounding spelled out, because two kernels apply it (gn_glu_kernel and the
// residual layer that normalises while it loads) and must agree to the bit whatever the compiler would
// contract around them.
__device__ __forceinline__ float gn_glu_value(float a, float g, float m0, float r0, float m1, float r1, float ga, float ba,
                                              float gg, float bg) {
  const float av = __fmaf_rn(__fmul_rn(__fsub_rn(a, m0), r0), ga, ba);
  const float gv = __fmaf_rn(__fmul_rn(__fsub_rn(g, m1), r1), gg, bg);
  // sigmoid on the hardware transcendentals (v_exp_f32, v_rcp_f32: 1 ulp each, about 3e-7 overall): the IEEE expf +
  // division sequence is some 35 VALU instructions per element, and in the layers that normalise while they stage
  // their rows (resstack.hip, resconv16) that was 10 k of a workgroup's 70 k cycles with the matrix pipe idle
  const float e = __builtin_amdgcn_exp2f(__fmul_rn(gv, -1.4426950408889634f));
  return __fmul_rn(av, __builtin_amdgcn_rcpf(__fadd_rn(1.0f, e)));
}
#endif

}  // namespace asw

// ---- optional in-library launch profiler (HIP events on the launch stream) -----------
// bench.py enables it for the timed region so per-kernel durations are measured live on
// the stream the kernels run on; disabled (the default) it costs one branch per launch.
#include <string>
namespace asw {
std::string prof_name(const char* base, int bm, int bn, int bk, bool ln, bool stats);
bool prof_detail();
// Does a launch name say which of several bit-identical tilings ran (resstack64's ",carry")?  Not under
// asw_profile_enable(2), whose names identify the arithmetic of a launch and nothing else.
bool prof_form();
// `work` = algorithmic FLOPs of the launch (GEMM-class kernels), `bytes` = algorithmic HBM bytes (the
// memory-bound passes); either may be 0.
struct ProfScope {
  ProfScope(hipStream_t s, const std::string& name, double work, double bytes = 0.0);
  ~ProfScope();
  int slot;
  hipStream_t stream;
};

// "[B.. M.. N.. K.. <key><val>]": the shape suffix of a GEMM launch name in the detailed profile (empty otherwise);
// `feed` (" res": the residue-image A feed) goes in front of the closing bracket
struct ShapeTag {
  char s[64] = "";
  ShapeTag(const asw_convgemm_args& a, char key, int val, const char* feed = "") {
    if (prof_detail())
      snprintf(s, sizeof s, "[B%d M%d N%d K%d %c%d%s]", a.B, a.M_out, a.N, a.taps * a.Cin, key, val, feed);
  }
};

#ifdef __HIPCC__
// The launch protocol of the kernels that come as a (one-term, three-term) pair of instantiations, K1 for the
// single-pass f16 mode (precision 2) and K3 for everything else: pick the instantiation, raise its per-device
// dynamic-LDS limit to lds_limit (one SmemAttr per device and instantiation), open the profiler scope under
// `name` + `detail`, launch, check.  `detail` is the shape suffix of the detailed profile (asw_profile_enable(2)).
template <auto K1, auto K3, typename... Args>
int launch_pair(int precision, dim3 grid, dim3 block, size_t lds, size_t lds_limit, std::string name, const char* detail,
                double flops, double bytes, hipStream_t s, const Args&... args) {
  const bool x1 = precision == 2;
  auto kern = x1 ? K1 : K3;
  static SmemAttr attr[2];
  if (int rc = attr[x1].ensure(reinterpret_cast<const void*>(kern), lds_limit)) return rc;
  if (prof_detail()) name += detail;
  ProfScope prof(s, name, flops, bytes);
  hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
#endif
}  // namespace asw
