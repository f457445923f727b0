// wave_util.h -- the device helpers every small kernel shares: full-wave (64-lane) reductions, the workgroup sum
// built on them, and the int16 quantiser of the input normalisation.  One definition each, because kernels that must
// agree to the bit (the single-shape entry points and their general forms, the spot and the joint statistics) go
// through the same order of additions: xor butterfly 32, 16, ... 1, every lane ends with the result.
// The partial-width reductions (4 or 16 lanes per row in the attention softmaxes, the GEMM epilogue, the residual
// stacks, the clustering kernels) are different operations and stay where they are.
#pragma once
#include <hip/hip_runtime.h>

namespace asw {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {                  // float or double
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over the workgroup (blockDim.x a multiple of 64, red[] one double per wave); every thread gets the result, the
// waves' sums are added in wave order.  red[] may be reused by the next call: the first barrier covers its readers.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

// (x * 2**15).round() / 2**15, round-half-even like torch.round (SpeakerLocalization/network.py:34)
__device__ __forceinline__ float quant16(float x) { return rintf(x * 32768.0f) * (1.0f / 32768.0f); }

}  // namespace asw
