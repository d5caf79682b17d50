// Shared device/host helpers of the gfx950 neural-process kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "npf_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace npf {

constexpr int kTilePts = 32;  // points per PT32 tile

// Offset (floats) of the float4 holding features [4*f4, 4*f4+4) of point p inside a PT32 tile.
__host__ __device__ inline int pt_off(int f4, int p) { return (f4 * 32 + p) * 4; }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Entry i of a device tensor of per-task counts, clamped to [0, hi], the rows the task's tensors hold (the host never reads a count)
__device__ __forceinline__ int clamp_count(const int32_t* __restrict__ n, size_t i, int hi) {
  const int v = n[i];
  return v < 0 ? 0 : (v > hi ? hi : v);
}

#define NPF_CHECK_LAUNCH()                     \
  do {                                         \
    hipError_t e__ = hipGetLastError();        \
    if (e__ != hipSuccess) return NPF_ELAUNCH; \
  } while (0)

// Sum over the threads of a workgroup (whole wavefronts, <= 8 of them); ``red``: 8 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read by a previous call
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

// softplus of the Gaussian head's scale: scale = 0.01 + 0.99 softplus(raw) (npf/neuralproc/base.py:116)
__device__ __forceinline__ float softplus_t(float x) { return x > 20.f ? x : log1pf(expf(x)); }

}  // namespace npf
