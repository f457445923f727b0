// mfma_util.h -- device helpers shared by the MFMA kernels (convgemm.hip, pipegemm.hip, resconv.hip, resstack.hip, downconv.hip,
// attention.hip): vector types, the accumulator row mapping, the buffer-descriptor activation load, the f32 row product of
// the attention kernels and the fp32 -> fp16 hi / lo operand split of the f16x3 mode.
#pragma once
#include "asw_common.h"
#include "wave_util.h"

namespace asw_mfma {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

using asw::wave_sum;

// row, within a 32 x 32 MFMA accumulator block, that register r of a lane in half lh = lane >> 5 holds (its column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// acc += A B^T of two row-major fp32 operands on v_mfma_f32_32x32x2_f32 (an fmaf chain: exact fp32): a_row / b_row
// already include this lane's (row, 4 * (lane >> 5)) offset; 8 k per step, KSTEPS = K / 8
template <int KSTEPS>
__device__ __forceinline__ floatx16 mma_row(const float* a_row, const float* b_row, floatx16 acc) {
#pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) {
    const float4 a = *reinterpret_cast<const float4*>(a_row + kk * 8);
    const float4 b = *reinterpret_cast<const float4*>(b_row + kk * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

// Activation loads go through a raw buffer descriptor: an offset outside [0, bytes) -- the
// zero padding of the convolution, rows past the end of the sequence, or a disabled lane --
// makes the hardware return zeros, so the staging loads carry no branch and no
// select.  (With plain pointers hipcc turns "load, then select zero" back into a branch around
// the load and waits vmcnt(0) between loads: a full memory latency per K chunk, exposed.)
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef float floatx4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t act_rsrc(const float* base, long elems) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)(elems * 4), 0x00020000);
}
__device__ __forceinline__ float4 act_load4(__amdgpu_buffer_rsrc_t r, long elem, bool ok) {
  // disabled / negative -> 0x80000000: beyond any descriptor (bytes < 2^31) without wrapping
  const intx4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (ok && elem >= 0) ? (int)(elem * 4) : (int)0x80000000, 0, 0);
  const floatx4v f = __builtin_bit_cast(floatx4v, v);
  return make_float4(f[0], f[1], f[2], f[3]);
}

// x -> hi + lo with two packed round-toward-zero conversions per pair (v_cvt_pkrtz_f16_f32:
// finite overflow saturates at +-65504 instead of becoming inf).  hi carries 11 bits, the
// remainder x - hi is exact in fp32, lo carries its next 11 bits truncated: |x - hi - lo| < 2^-20 |x|.
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split4(const float4 x, half4& hi, half4& lo) {
  const fp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(x.x, x.y);
  const fp16x2 h23 = __builtin_amdgcn_cvt_pkrtz(x.z, x.w);
  const fp16x2 l01 = __builtin_amdgcn_cvt_pkrtz(x.x - (float)h01[0], x.y - (float)h01[1]);
  const fp16x2 l23 = __builtin_amdgcn_cvt_pkrtz(x.z - (float)h23[0], x.w - (float)h23[1]);
  union { fp16x2 v[2]; half4 h; } uh, ul;
  uh.v[0] = h01; uh.v[1] = h23;
  ul.v[0] = l01; ul.v[1] = l23;
  hi = uh.h;
  lo = ul.h;
}

// Single-pass f16 mode (precision 2: one MFMA per product, the hi halves only): the hi half is rounded to
// nearest instead of truncated -- with no lo half to catch the remainder, truncation would bias every
// product low by ~2^-12.  lo is still produced (the C = 64 residual layer reads its residual from the image).
// The plain conversion turns |x| >= 65520 into inf (and the remainder x - inf into NaN), so x is clamped to the fp16
// range first (one v_med3_f32 per element): finite overflow saturates at +-65504 here as it does in split4.
__device__ __forceinline__ _Float16 rn_sat(float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.f, 65504.f); }
__device__ __forceinline__ void split4_rn(const float4 x, half4& hi, half4& lo) {
  const _Float16 h0 = rn_sat(x.x), h1 = rn_sat(x.y), h2 = rn_sat(x.z), h3 = rn_sat(x.w);
  const fp16x2 l01 = __builtin_amdgcn_cvt_pkrtz(x.x - (float)h0, x.y - (float)h1);
  const fp16x2 l23 = __builtin_amdgcn_cvt_pkrtz(x.z - (float)h2, x.w - (float)h3);
  hi = half4{h0, h1, h2, h3};
  union { fp16x2 v[2]; half4 h; } ul;
  ul.v[0] = l01; ul.v[1] = l23;
  lo = ul.h;
}
template <int NTERM>
__device__ __forceinline__ void split4t(const float4 x, half4& hi, half4& lo) {
  if constexpr (NTERM == 1) split4_rn(x, hi, lo);
  else split4(x, hi, lo);
}

}  // namespace asw_mfma
