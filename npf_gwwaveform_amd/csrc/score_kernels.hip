// Scores of an observation y under the predictive mixture (npf_mixture_score), the counterpart of npf_mixture_summary evaluated at
// y: per target point and output dimension the log density, the probability integral transform (PIT) and the continuous ranked
// probability score (CRPS) of the equal-weight mixture of the n_z Gaussians N(mu_k, sg_k^2) the latent samples give.  As in
// predict_kernels.hip nothing of size [n_z, B, T, dy] is written: one thread per (t, d) element of a task, grid = (point tiles,
// task); the 2 n_z component parameters of the element are read once from suff and kept by the thread (registers for n_z <= 32, a
// private LDS column beyond: thread on the fast axis, so a wavefront's reads of one component fall on consecutive banks).
//
// Log density and PIT are one pass over the components (an erfcf, a logf and an expf each).  The CRPS is
//   1/K sum_k A(y - mu_k, sg_k) - 1/(2 K^2) sum_{i,j} A(mu_i - mu_j, sqrt(sg_i^2 + sg_j^2)),  A(m, s) = 2 s phi(m / s) + m erf(m / (s sqrt 2))
// whose pair sum is symmetric with the diagonal 2 sg_i / sqrt(pi): K (K - 1) / 2 evaluations of A (an rsq, an erff and an exp each:
// the hot path, 8128 of them per element at K = 128) plus K terms.  For the pair loop the thread's copy holds the variances sg_k^2.
// Registers cannot be indexed by a loop counter, so only the 8-component instance runs the pair loop on them (28 pairs, unrolled);
// unrolled for 32 components it is 233 KB of code and 276 VGPRs.  The 32-component instance therefore keeps its components in
// registers for the passes over k and hands (mu_k, sg_k^2) to a private LDS column for the pair loop, which the LDS instances
// run on the column they already hold: row i in registers, row j < i read from the column, four j in flight.
// Every A is an fp32 value; they are summed in double (two instructions of ~70 per pair), so the difference of the two sums
// carries the rounding of its terms only, not that of 8128 additions.
//
// Homoskedastic heads pool the scale of every (z-sample, task) row over the task's valid points first, exactly as the summary kernel
// does (its first phase, restated here).
#include "npf_common.hpp"

namespace npf {

constexpr float kScInvSqrt2 = 0.70710678118654752440f;
constexpr float kScInvSqrt2Pi = 0.39894228040143267794f;
constexpr float kScInvSqrtPi = 0.56418958354775628695f;
constexpr float kScLogSqrt2Pi = 0.91893853320467274178f;
constexpr int kScMaxNz = 128;
constexpr int kScMaxDy = 16;

// A(m, sqrt(v)) of the pair sum, m = mu_i - mu_j, v = sg_i^2 + sg_j^2 > 0: |m| erf(|m| / sqrt(2 v)) + 2 sqrt(v) phi(m / sqrt(v)).
// |m| multiplies the erf directly (2 Phi - 1 is never formed as a difference); the rsq only reaches the phi term and the arguments.
__device__ __forceinline__ float pair_term(float m, float v) {
  const float r = __builtin_amdgcn_rsqf(v);
  const float a = fabsf(m), z = a * r;
  return fmaf(a, erff(z * kScInvSqrt2), (2.f * kScInvSqrt2Pi) * (v * r) * __expf(-0.5f * z * z));
}

// NZ: component capacity; IN_LDS: components in a private LDS column (comp[2 k][thread], comp[2 k + 1][thread]) instead of registers;
// PAIR_LDS: the pair loop runs on such a column (always with IN_LDS)
template <int NZ, bool IN_LDS, bool PAIR_LDS, int THREADS>
__global__ __launch_bounds__(THREADS) void mixture_score_kernel(const float* __restrict__ suff, const float* __restrict__ Y,
                                                                 const int32_t* __restrict__ n_valid, int n_z, int n_tasks, int pts,
                                                                 int dy, int homosk, float* __restrict__ ld_out,
                                                                 float* __restrict__ pit_out, float* __restrict__ crps_out) {
  __shared__ float pooled[NZ * kScMaxDy];  // [k][d] pooled scale of row (k, task)
  __shared__ float comp[PAIR_LDS ? 2 * NZ * THREADS : 1];
  const int b = blockIdx.y;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const size_t row_stride = (size_t)pts * (size_t)(2 * dy);  // floats of one (z-sample, task) row of suff
  const float* s_task = suff + (size_t)b * row_stride;         // row k of this task: + k * n_tasks * row_stride
  const size_t k_stride = (size_t)n_tasks * row_stride;

  if (homosk && nv > 0) {  // (the pooling phase of mixture_summary_kernel: one wavefront per row and output dimension)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = THREADS >> 6;
    for (int i = wave; i < n_z * dy; i += n_waves) {
      const int k = i / dy, d = i - k * dy;
      const float* s = s_task + (size_t)k * k_stride;
      double part = 0.0;  // (fp32 terms, the head's formula; summed in double: the mean carries no summation error)
      for (int t = lane; t < nv; t += 64) part += (double)(0.01f + 0.99f * softplus_t(s[t * 2 * dy + dy + d]));
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
      if (lane == 0) pooled[i] = (float)(part / (double)nv);
    }
    __syncthreads();
  }

  const int n_elem = pts * dy, n_live = nv * dy;
  const size_t out_base = (size_t)b * (size_t)n_elem;
  [[maybe_unused]] float mu_r[IN_LDS ? 1 : NZ], sg_r[IN_LDS ? 1 : NZ];
  [[maybe_unused]] float* col = comp + threadIdx.x;

  // f(mu_k, sg_k) over the components of this thread's element (references: the pair loop's pass turns sg_k into sg_k^2)
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
    if (e >= n_live) {  // a row beyond the count: zeros that leave a sum over the points right, PIT 0.5; suff and Y there are never read
      if (ld_out) ld_out[out_base + e] = 0.f;
      if (pit_out) pit_out[out_base + e] = 0.5f;
      if (crps_out) crps_out[out_base + e] = 0.f;
      continue;
    }
    const int t = e / dy, d = e - t * dy;
    const float* s = s_task + (size_t)t * (size_t)(2 * dy) + d;
    const float y = Y[out_base + e];
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

    if (ld_out) {  // logsumexp_k(-u_k^2 / 2 - log sg_k - log sqrt(2 pi)) - log K, the maximum subtracted
      auto logp = [&](float m, float sg) {
        const float u = (y - m) / sg;
        return -0.5f * u * u - logf(sg) - kScLogSqrt2Pi;
      };
      float mx = -INFINITY;
      each([&](float& m, float& sg) { mx = fmaxf(mx, logp(m, sg)); });
      float ld;
      if (mx > -INFINITY) {
        float sum = 0.f;
        each([&](float& m, float& sg) { sum += __expf(logp(m, sg) - mx); });  // (a component at -inf: weight 0)
        ld = mx + logf(sum) - logf((float)n_z);
      } else {
        ld = y != y ? y : -INFINITY;  // every component at -inf (y = +-inf), or y NaN
      }
      ld_out[out_base + e] = ld;
    }
    if (pit_out) {  // 1/K sum_k Phi(u_k); erfc of the negated argument: small Phi comes out of erfc's tail, nothing near 1 is subtracted
      float F = 0.f;
      each([&](float& m, float& sg) { F += 0.5f * erfcf((m - y) / sg * kScInvSqrt2); });
      pit_out[out_base + e] = F / (float)n_z;  // (a division: every term <= 1, so the sum <= K and the quotient <= 1)
    }
    if (crps_out) {
      double t1 = 0.0, t2 = 0.0;  // sum_k A(y - mu_k, sg_k); sum_{i<j} A_ij + sum_i sg_i / sqrt(pi)
      each([&](float& m, float& sg) {
        const float a = fabsf(y - m), u = a / sg;
        t1 += (double)fmaf(a, erff(u * kScInvSqrt2), (2.f * kScInvSqrt2Pi) * sg * __expf(-0.5f * u * u));
        t2 += (double)(sg * kScInvSqrtPi);
        sg = sg * sg;
      });
      if constexpr (PAIR_LDS && !IN_LDS) {
#pragma unroll
        for (int k = 0; k < NZ; ++k) {
          if (k < n_z) {
            col[(2 * k) * THREADS] = mu_r[k];
            col[(2 * k + 1) * THREADS] = sg_r[k];
          }
        }
      }
      if constexpr (PAIR_LDS) {
        for (int i = 1; i < n_z; ++i) {
          const float mi = col[(2 * i) * THREADS], vi = col[(2 * i + 1) * THREADS];
#pragma unroll 4
          for (int j = 0; j < i; ++j) t2 += (double)pair_term(mi - col[(2 * j) * THREADS], vi + col[(2 * j + 1) * THREADS]);
        }
      } else {
#pragma unroll
        for (int i = 1; i < NZ; ++i) {
          if (i < n_z) {
#pragma unroll
            for (int j = 0; j < i; ++j) t2 += (double)pair_term(mu_r[i] - mu_r[j], sg_r[i] + sg_r[j]);
          }
        }
      }
      const double K = (double)n_z;
      crps_out[out_base + e] = (float)(t1 / K - t2 / (K * K));
    }
  }
}

}  // namespace npf

extern "C" int npf_mixture_score(const float* suff, const float* Y, const int32_t* n_valid, int32_t n_z, int32_t n_tasks, int32_t pts,
                                 int32_t dy, int32_t homoskedastic, float* log_density, float* pit, float* crps, void* stream) {
  using namespace npf;
  if (!suff || !Y || n_z <= 0 || n_z > kScMaxNz || n_tasks <= 0 || n_tasks > 65535 || pts <= 0 || dy <= 0 || dy > kScMaxDy)
    return NPF_EINVAL;
  if (!log_density && !pit && !crps) return NPF_EINVAL;
  if ((int64_t)pts * dy > (int64_t)1 << 30) return NPF_EINVAL;  // (element indices are ints)
  const int n_elem = pts * dy;
  auto launch = [&](auto kernel, int threads) {
    int tiles = (n_elem + threads - 1) / threads;
    if (homoskedastic) {  // every workgroup pools the task's rows first: fewer, longer workgroups per task
      const int cap = n_tasks >= 256 ? 1 : 256 / n_tasks;
      tiles = tiles < cap ? tiles : cap;
    }
    hipLaunchKernelGGL(kernel, dim3(tiles, n_tasks), dim3(threads), 0, (hipStream_t)stream, suff, Y, n_valid, n_z, n_tasks, pts, dy,
                       homoskedastic, log_density, pit, crps);
  };
  if (n_z <= 8)
    launch(mixture_score_kernel<8, false, false, 256>, 256);
  else if (n_z <= 32)
    launch(mixture_score_kernel<32, false, true, 256>, 256);
  else if (n_z <= 64)
    launch(mixture_score_kernel<64, true, true, 64>, 64);
  else
    launch(mixture_score_kernel<128, true, true, 64>, 64);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}
