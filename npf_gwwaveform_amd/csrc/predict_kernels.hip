// Predictive summary of the decoder's raw output: per target point and output dimension the mean, the standard deviation and
// quantiles of the equal-weight mixture of the n_z Gaussians N(mu_k, sg_k^2) the latent samples give (npf_mixture_summary).
// Nothing of size [n_z, B, T, dy] is written: the 2 n_z component parameters of an element are read once from suff, kept by
// the element's thread (registers for n_z <= 32, a private LDS column beyond) and every pass over them -- the mean, the centred
// second moment, each Newton / bisection step of each quantile -- runs on that copy.
//
// One thread per (t, d) element of a task, grid = (point tiles, task).  Without quantiles the launch is a stream of suff (HBM-
// bound); with them it is erfcf / expf-bound (one of each per component and solver step).  Homoskedastic heads pool the scale
// of every (z-sample, task) row over the task's points first: a first phase of the same workgroup (one wavefront per row and
// output dimension, no barrier inside), so such a launch uses fewer workgroups per task than tiles to bound the repeated reads.
#include "npf_common.hpp"

namespace npf {

constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;
constexpr int kMixMaxIter = 64;          // solver steps per quantile at most (each at least halves the bracket every other step)
constexpr float kMixResidual = 2.4e-7f;  // 4 * 2^-24: |F(x) - p| below the rounding of the fp32 sum F itself
constexpr int kMixMaxNz = 128;
constexpr int kMixMaxDy = 16;

#ifdef NPF_MIXTURE_COUNT_ITERS
// debug build only (tools/microbench measurements): [0] evaluations of the mixture CDF, [1] quantiles solved iteratively
__device__ unsigned long long g_mix_iters[2];
#endif

// NZ: component capacity; IN_LDS: components in a private LDS column (comp[2 k][thread], comp[2 k + 1][thread]) instead of registers
template <int NZ, bool IN_LDS, int THREADS>
__global__ __launch_bounds__(THREADS) void mixture_summary_kernel(const float* __restrict__ suff, const int32_t* __restrict__ n_valid,
                                                                   int n_z, int n_tasks, int pts, int dy, int homosk,
                                                                   const float* __restrict__ z_p, int n_probs,
                                                                   const float* __restrict__ probs, float* __restrict__ mean_out,
                                                                   float* __restrict__ std_out, float* __restrict__ quant) {
  __shared__ float pooled[kMixMaxNz * kMixMaxDy];     // [k][d] pooled scale of row (k, task)
  __shared__ double pooled_d[kMixMaxNz * kMixMaxDy];  // ... before its rounding to fp32 (the collapsed bracket below)
  __shared__ float comp[IN_LDS ? 2 * NZ * THREADS : 1];
  const int b = blockIdx.y;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const size_t row_stride = (size_t)pts * (size_t)(2 * dy);  // floats of one (z-sample, task) row of suff
  const float* s_task = suff + (size_t)b * row_stride;         // row k of this task: + k * n_tasks * row_stride
  const size_t k_stride = (size_t)n_tasks * row_stride;

  if (homosk && nv > 0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = THREADS >> 6;
    for (int i = wave; i < n_z * dy; i += n_waves) {
      const int k = i / dy, d = i - k * dy;
      const float* s = s_task + (size_t)k * k_stride;
      double part = 0.0;  // (fp32 terms, the head's formula; summed in double: the mean carries no summation error)
      for (int t = lane; t < nv; t += 64) part += (double)(0.01f + 0.99f * softplus_t(s[t * 2 * dy + dy + d]));
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
      if (lane == 0) {
        pooled_d[i] = part / (double)nv;
        pooled[i] = (float)pooled_d[i];
      }
    }
    __syncthreads();
  }

  const int n_elem = pts * dy, n_live = nv * dy;
  const size_t out_base = (size_t)b * (size_t)n_elem;
  const size_t q_stride = (size_t)n_tasks * (size_t)n_elem;
  const float inv_nz = 1.f / (float)n_z;
  [[maybe_unused]] float mu_r[IN_LDS ? 1 : NZ], sg_r[IN_LDS ? 1 : NZ];
  [[maybe_unused]] float* col = comp + threadIdx.x;

  // f(mu_k, sg_k) over the components of this thread's element
  auto each = [&](auto&& f) {
    if constexpr (IN_LDS) {
      for (int k = 0; k < n_z; ++k) f(col[(2 * k) * THREADS], col[(2 * k + 1) * THREADS]);
    } else {
#pragma unroll
      for (int k = 0; k < NZ; ++k)
        if (k < n_z) f(mu_r[k], sg_r[k]);
    }
  };

  for (int e = blockIdx.x * THREADS + threadIdx.x; e < n_elem; e += gridDim.x * THREADS) {
    if (e >= n_live) {  // a row beyond the count: loc = 0, scale = 1 (the masked head's convention); suff there is never read
      mean_out[out_base + e] = 0.f;
      std_out[out_base + e] = 1.f;
      for (int j = 0; j < n_probs; ++j) quant[(size_t)j * q_stride + out_base + e] = z_p[j];
      continue;
    }
    const int t = e / dy, d = e - t * dy;
    const float* s = s_task + (size_t)t * (size_t)(2 * dy) + d;
    if constexpr (IN_LDS) {
      for (int k = 0; k < n_z; ++k) {
        const float* sk = s + (size_t)k * k_stride;
        col[(2 * k) * THREADS] = sk[0];
        col[(2 * k + 1) * THREADS] = homosk ? pooled[k * dy + d] : 0.01f + 0.99f * softplus_t(sk[dy]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NZ; ++k) {
        if (k < n_z) {
          const float* sk = s + (size_t)k * k_stride;
          mu_r[k] = sk[0];
          sg_r[k] = homosk ? pooled[k * dy + d] : 0.01f + 0.99f * softplus_t(sk[dy]);
        }
      }
    }
    float mean = 0.f;
    each([&](float m, float) { mean += m; });
    mean *= inv_nz;
    float var = 0.f;
    each([&](float m, float sg) { var += sg * sg + (m - mean) * (m - mean); });  // (centred: no E[x^2] - mean^2 cancellation)
    const float sd = sqrtf(var * inv_nz);
    mean_out[out_base + e] = mean;
    std_out[out_base + e] = sd;

    for (int j = 0; j < n_probs; ++j) {
      const float z = z_p[j], p = probs[j];
      // a_k = mu_k + sg_k z is the p-quantile of component k: F(min_k a_k) <= p <= F(max_k a_k)
      float lo = INFINITY, hi = -INFINITY;
      each([&](float m, float sg) {
        const float a = fmaf(sg, z, m);
        lo = fminf(lo, a);
        hi = fmaxf(hi, a);
      });
      float x;
      if (!(hi > lo)) {
        // one component, or identical ones: a_k itself.  It is the returned value here, not a bracket end, so it is evaluated
        // once more in double from the raw scale (this branch only: the fp32 softplus above is good to a few ulp, not to one)
        const double raw = (double)s[dy];
        const double sg = homosk ? pooled_d[d] : 0.01 + 0.99 * (raw > 30.0 ? raw : log1p(exp(raw)));
        x = (float)((double)s[0] + sg * (double)z);
      } else {
        float g, dens;  // F(x) - p and the mixture density F'(x), one pass over the components
        auto eval = [&](float at) {
          float F = 0.f, f = 0.f;
          each([&](float m, float sg) {
            const float inv = __builtin_amdgcn_rcpf(sg);
            const float u = (at - m) * inv;
            F += 0.5f * erfcf(-u * kInvSqrt2);
            f += kInvSqrt2Pi * inv * __expf(-0.5f * u * u);
          });
          g = F * inv_nz - p;
          dens = f * inv_nz;
        };
        x = fminf(fmaxf(fmaf(sd, z, mean), lo), hi);  // start: the quantile of the moment-matched Gaussian
        float dx_old = hi - lo;
        [[maybe_unused]] int n_eval = 1;
        eval(x);
        for (int it = 0; it < kMixMaxIter; ++it) {
          if (fabsf(g) <= kMixResidual) break;
          if (g > 0.f) hi = x; else lo = x;
          // Newton inside the bracket while it at least halves the step, bisection otherwise (dens == 0 on a plateau: NaN / inf
          // fail the comparisons)
          float xn = x - g / dens;
          if (!(xn > lo && xn < hi && fabsf(2.f * g) <= fabsf(dx_old * dens))) xn = 0.5f * lo + 0.5f * hi;
          if (!(xn > lo && xn < hi) || xn == x) break;  // the bracket no longer shrinks in fp32
          dx_old = fabsf(xn - x);
          x = xn;
          eval(x);
#ifdef NPF_MIXTURE_COUNT_ITERS
          ++n_eval;
#endif
        }
#ifdef NPF_MIXTURE_COUNT_ITERS
        atomicAdd(&g_mix_iters[0], (unsigned long long)n_eval);
        atomicAdd(&g_mix_iters[1], 1ull);
#endif
      }
      quant[(size_t)j * q_stride + out_base + e] = x;
    }
  }
}

}  // namespace npf

#ifdef NPF_MIXTURE_COUNT_ITERS
extern "C" int npf_debug_mixture_iters(unsigned long long* out2, int reset) {
  if (out2 && hipMemcpyFromSymbol(out2, HIP_SYMBOL(npf::g_mix_iters), sizeof(npf::g_mix_iters)) != hipSuccess) return NPF_ELAUNCH;
  if (reset) {
    const unsigned long long zero[2] = {0ull, 0ull};
    if (hipMemcpyToSymbol(HIP_SYMBOL(npf::g_mix_iters), zero, sizeof(zero)) != hipSuccess) return NPF_ELAUNCH;
  }
  return NPF_OK;
}
#endif

extern "C" int npf_mixture_summary(const float* suff, const int32_t* n_valid, int32_t n_z, int32_t n_tasks, int32_t pts, int32_t dy,
                                   int32_t homoskedastic, const float* z_p, int32_t n_probs, const float* probs, float* mean,
                                   float* std, float* quant, void* stream) {
  using namespace npf;
  if (!suff || !mean || !std || n_z <= 0 || n_z > kMixMaxNz || n_tasks <= 0 || n_tasks > 65535 || pts <= 0 || dy <= 0 || dy > kMixMaxDy)
    return NPF_EINVAL;
  if (n_probs < 0 || (n_probs > 0 && (!z_p || !probs || !quant))) return NPF_EINVAL;
  if ((int64_t)pts * dy > (int64_t)1 << 30) return NPF_EINVAL;  // (element indices are ints)
  const int n_elem = pts * dy;
  auto launch = [&](auto kernel, int threads) {
    int tiles = (n_elem + threads - 1) / threads;
    if (homoskedastic) {  // every workgroup pools the task's rows first: fewer, longer workgroups per task
      const int cap = n_tasks >= 256 ? 1 : 256 / n_tasks;
      tiles = tiles < cap ? tiles : cap;
    }
    hipLaunchKernelGGL(kernel, dim3(tiles, n_tasks), dim3(threads), 0, (hipStream_t)stream, suff, n_valid, n_z, n_tasks, pts, dy,
                       homoskedastic, z_p, n_probs, probs, mean, std, quant);
  };
  if (n_z <= 8)
    launch(mixture_summary_kernel<8, false, 256>, 256);
  else if (n_z <= 32)
    launch(mixture_summary_kernel<32, false, 256>, 256);
  else if (n_z <= 64)
    launch(mixture_summary_kernel<64, true, 64>, 64);
  else
    launch(mixture_summary_kernel<128, true, 64>, 64);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}
