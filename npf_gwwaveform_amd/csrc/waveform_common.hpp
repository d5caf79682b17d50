// What waveform_kernels.hip, waveform_net_kernels.hip, waveform_dist_kernels.hip and waveform_grad_kernels.hip share: the launch
// geometry and the workspace rows of the correlation launches, the launch helpers of the two likelihoods, the fixed-order
// workgroup sum, ln I0 and I1 / I0 in double.
#pragma once
#include "npf_common.hpp"

namespace npf {

constexpr int kWfJC = NPF_WAVEFORM_JC;  // time shifts per workgroup of launch 1
constexpr int kWfThreads = 128;
constexpr int kWfBwdThreads = 256;  // points per workgroup pass of the backward launches
constexpr int kWfBwdMaxGridY = 1024;
constexpr int kWfMaxTau = 65536;
constexpr double kWfTwoPi = 6.283185307179586476925286766559;

inline int wf_chunks(int n_tau) { return n_tau > 0 ? (n_tau + kWfJC - 1) / kWfJC : 1; }

// doubles per workspace row of the single-stream launches (waveform_kernels.hip) and of the network ones (waveform_net_kernels.hip)
inline int64_t wf_row_doubles(int n_tau) { return 4 + 2 * (int64_t)kWfJC * wf_chunks(n_tau); }
inline int64_t wf_net_row_doubles(int n_det, int n_tau) { return 2 + 2 * (int64_t)n_det + 2 * (int64_t)kWfJC * wf_chunks(n_tau); }

// The launches of npf_waveform_loglike / npf_waveform_loglike_net on arguments their entries have checked (wf_loglike_args_bad /
// wf_loglike_net_args_bad: everything but "no output requested"), over workspace rows of row_doubles doubles -- the layout's own
// count or more (waveform_dist_kernels.hip keeps a tail behind it).  finish == false: launch 1 only.  -> NPF_OK or NPF_ELAUNCH.
bool wf_loglike_args_bad(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                         int n_rows, int n_tasks, int pts, int n_tau, const void* workspace);
int wf_loglike_launch(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                      const int32_t* n_valid, int n_rows, int n_tasks, int pts, double tau0, double dtau, int n_tau, double* hh, double* dd,
                      double* snr, double* lnl_max, double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                      double* lnl_max_mix, double* ws, int64_t row_doubles, bool finish, hipStream_t stream);
bool wf_loglike_net_args_bad(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                             const double* delay, const double* resp, int n_rows, int n_tasks, int n_det, int pts, int n_tau,
                             const void* workspace);
int wf_loglike_net_launch(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                          const int32_t* n_valid, const double* delay, const double* resp, int n_rows, int n_tasks, int n_det, int pts,
                          double tau0, double dtau, int n_tau, double* hh, double* dd, double* snr, double* lnl_max, double* lnl_marg,
                          int32_t* tau_index, double* phase, double* series, double* lnl_mix, double* lnl_max_mix, double* hh_det,
                          double* snr_det, double* dd_det, double* ws, int64_t row_doubles, bool finish, hipStream_t stream);

// dst[i] = sum over the workgroup of v[i], i < N (N <= THREADS): lanes by xor shuffles, then the waves in order.  red: N * waves doubles.
template <int N, int THREADS>
__device__ __forceinline__ void block_sum_store(double (&v)[N], double* red, double* __restrict__ dst) {
  constexpr int WAVES = THREADS / 64;
  static_assert(N <= THREADS, "one thread per sum");
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read by a previous call
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[i * WAVES + wave] = v[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < N) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[threadIdx.x * WAVES + w];
    dst[threadIdx.x] = s;
  }
}

constexpr int kWfLlThreads = 256;  // threads of a finishing workgroup
constexpr double kWfI0Switch = NPF_LOGLIKE_I0_SWITCH;
constexpr int kWfI0AsymTerms = 16;   // terms of the 1 / (8 x) series above the switch: truncation 2.7e-16 of I0 at x = 24, less beyond
constexpr int kWfI0PowerTerms = 48;  // cap of the power series below it (40 terms reach 2^-60 of the sum at x = 24)

// ln I0(x), x >= 0, without overflow.  Below the switch point x_s = 24: log1p of the power series I0 - 1 = sum_{k >= 1} (x^2 / 4)^k /
// (k!)^2 (positive terms: no cancellation, and log1p keeps the relative accuracy as x -> 0).  From x_s on:
// x - ln(2 pi x) / 2 + log1p(S) with S = sum_{k = 1 .. 16} prod_{m <= k} (2 m - 1)^2 / (8 x m), summed by Horner's rule.
__device__ __forceinline__ double wf_log_i0(double x) {
  if (x < kWfI0Switch) {
    const double q = 0.25 * x * x;
    double t = q, s = q;
#pragma unroll
    for (int k = 2; k <= kWfI0PowerTerms; ++k) {
      t *= q * (1.0 / (double)(k * k));  // (unrolled: the reciprocal is a constant, no division in the chain)
      s += t;
      if (t <= s * 0x1p-60) break;
    }
    return log1p(s);
  }
  const double u = 0.125 / x;
  double acc = 0.0;
#pragma unroll
  for (int k = kWfI0AsymTerms; k >= 1; --k) acc = u * ((double)((2 * k - 1) * (2 * k - 1)) / (double)k) * (1.0 + acc);
  return x - 0.5 * log(kWfTwoPi * x) + log1p(acc);
}

// rho(x) = I1(x) / I0(x), x >= 0: d ln I0 / dx, in [0, 1), rho(0) = 0 exactly, no overflow for any finite x.  Below the switch point:
// (x / 2) S1 / S0 with S0 = sum_{k >= 0} q^k / (k!)^2, S1 = sum_{k >= 0} q^k / (k! (k + 1)!), q = x^2 / 4 (positive terms; the stopping
// rule and the cap of wf_log_i0).  From the switch point on: the ratio of the two 16-term series in 1 / (8 x), I0 with the factors
// (2 m - 1)^2 / (8 x m), I1 with ((2 m - 1)^2 - 4) / (8 x m) (the first one is -3 / (8 x)); e^x / sqrt(2 pi x) cancels.
__device__ __forceinline__ double wf_i1_over_i0(double x) {
  if (x < kWfI0Switch) {
    const double q = 0.25 * x * x;
    double t0 = 1.0, t1 = 1.0, s0 = 1.0, s1 = 1.0;
#pragma unroll
    for (int k = 1; k <= kWfI0PowerTerms; ++k) {
      t0 *= q * (1.0 / (double)(k * k));  // (unrolled: the reciprocals are constants)
      t1 *= q * (1.0 / (double)(k * (k + 1)));
      s0 += t0;
      s1 += t1;
      if (t0 <= s0 * 0x1p-60) break;
    }
    return (0.5 * x) * (s1 / s0);
  }
  const double u = 0.125 / x;
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = kWfI0AsymTerms; k >= 1; --k) {
    a0 = u * ((double)((2 * k - 1) * (2 * k - 1)) / (double)k) * (1.0 + a0);
    a1 = u * ((double)((2 * k - 1) * (2 * k - 1) - 4) / (double)k) * (1.0 + a1);
  }
  return (1.0 + a1) / (1.0 + a0);
}

}  // namespace npf
