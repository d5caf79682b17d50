// Distance-marginalised matched-filter likelihood (npf_waveform_loglike_dist / npf_waveform_loglike_net_dist): the predicted waveform
// is a template at a reference distance; at amplitude scale a (= d_ref / d) it is a h, and with x_j = |kappa_j| (|K_j| for the
// network), HH and n = max(n_tau, 1) of the parent likelihood the evidence of the grid scale a_i with log prior mass ln pi_i is
//   u_i = ln pi_i + (ln I0(a_i x*) - a_i^2 HH / 2) + (ln sum_j exp(ln I0(a_i x_j) - ln I0(a_i x*)) - ln n),   x* = max_j x_j,
// marginal over phase and grid time (every term of the sum is <= 1: ln I0 increases), -inf for a dead scale (a_i not in (0, inf) or
// ln pi_i not finite; nothing else of it is used).  A row with HH == 0 has x_j = 0: u_i = ln pi_i.  Everything in double.
//
// The two launches run after launch 1 of the parent (waveform_filter_kernel / waveform_filter_net_kernel) and read its workspace rows:
// HH at row[0], the candidates (Re, Im) at the parent layout's offset.  Behind the parent's doubles every row keeps a tail
// [x*, u_i (i < n_a)].
// Launch A (waveform_scale_marg_kernel): one workgroup per (row, chunk of SC scales).  It finds x* over the row's candidates (the
// smallest-index, fixed-order reduction of the finishing kernels) and keeps x_j in LDS while n <= 4096 (32 KiB of dynamic LDS, sized
// to the grid); a longer grid re-reads the candidates, which stay in L2.  Thread i < SC computes ln I0(a_i x*) once; then per scale
// the threads stride over j, the lanes add by xor shuffles, and after one barrier thread i adds the waves in order and writes u_i.
// Launch B (waveform_scale_finish_kernel): one workgroup per task walks its n_z rows in order: max_i u_i with the smallest index, the
// shifted sum, the row's outputs, post; thread 0 keeps the running (max, sum) of the mixture; post_mix is a second pass over the u_i.
// Differences are taken before logs are added ((u_i - max) - ln sum): sum_i exp(post_i) = 1 holds to rounding where u ~ 1e6.
// No atomics: a second call on the same inputs gives the same bits.
#include <climits>

#include "waveform_common.hpp"

namespace npf {

constexpr int kWfDistSC = NPF_DIST_SC;  // scales per workgroup of launch A
constexpr int kWfDistMaxScales = NPF_DIST_MAX_SCALES;
constexpr int kWfDistLdsTau = 4096;  // grid times whose x_j a workgroup of launch A keeps in LDS (32 KiB)

template <int SC>
__global__ __launch_bounds__(kWfLlThreads) void waveform_scale_marg_kernel(double* ws, int64_t row_doubles, int cand_off, int64_t tail_off,
                                                                            int n_tasks, int n_tau, const double* __restrict__ scales,
                                                                            int scale_per_task, const double* __restrict__ log_prior,
                                                                            int prior_per_task, int n_a) {
  constexpr int WAVES = kWfLlThreads / 64;
  extern __shared__ double xs[];  // x_j, j < n (n <= kWfDistLdsTau; else unused)
  __shared__ double red_v[WAVES];
  __shared__ int red_j[WAVES];
  __shared__ double sc_a[SC], sc_lp[SC], sc_l0[SC];  // a_i (0: dead), ln pi_i, ln I0(a_i x*)
  __shared__ double red_s[SC * WAVES];
  const int r = blockIdx.x, chunk = blockIdx.y, b = r % n_tasks, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = n_tau > 0 ? n_tau : 1;
  double* row = ws + (size_t)r * (size_t)row_doubles;
  const double vhh = row[0];
  const bool degenerate = vhh == 0.0;  // (Lambda = 1 at every scale: x_j = 0)
  const double* c = row + cand_off;
  const bool in_lds = n <= kWfDistLdsTau;

  double best = -1.0;
  int best_j = 0;
  for (int j = tid; j < n; j += kWfLlThreads) {
    const double re = c[2 * j], im = c[2 * j + 1], m2 = degenerate ? 0.0 : re * re + im * im;
    if (m2 > best) {  // (j ascends: the smallest index of the thread stays)
      best = m2;
      best_j = j;
    }
    if (in_lds) xs[j] = sqrt(m2);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oj = __shfl_xor(best_j, off);
    if (ob > best || (ob == best && oj < best_j)) {
      best = ob;
      best_j = oj;
    }
  }
  if (lane == 0) {
    red_v[wave] = best;
    red_j[wave] = best_j;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const double ob = red_v[w];
    const int oj = red_j[w];
    if (w == 0 || ob > best || (ob == best && oj < best_j)) {
      best = ob;
      best_j = oj;
    }
  }
  const double x_best = sqrt(best);  // (every thread: the same bits)
  if (chunk == 0 && tid == 0) row[tail_off] = x_best;

  const int i_mine = chunk * SC + tid;  // (tid < SC: the scale this thread prepares and finishes)
  if (tid < SC) {
    double a = 0.0, lp = 0.0;
    if (i_mine < n_a) {
      a = scales[(scale_per_task ? (size_t)b * (size_t)n_a : 0) + (size_t)i_mine];
      lp = log_prior[(prior_per_task ? (size_t)b * (size_t)n_a : 0) + (size_t)i_mine];
    }
    const bool live = i_mine < n_a && a > 0.0 && a < INFINITY && lp > -INFINITY && lp < INFINITY;  // (a NaN fails every test)
    sc_a[tid] = live ? a : 0.0;
    sc_lp[tid] = live ? lp : 0.0;
    sc_l0[tid] = live ? wf_log_i0(a * x_best) : 0.0;
  }
  __syncthreads();  // (xs and sc_* are complete)

#pragma unroll 1
  for (int k = 0; k < SC; ++k) {
    const double a = sc_a[k];
    if (a == 0.0) continue;  // a dead scale, or beyond n_a (the same for every thread)
    const double l0 = sc_l0[k];
    double sum = 0.0;
    for (int j = tid; j < n; j += kWfLlThreads) {
      double x;
      if (in_lds) {
        x = xs[j];
      } else {
        const double re = c[2 * j], im = c[2 * j + 1];
        x = degenerate ? 0.0 : sqrt(re * re + im * im);
      }
      sum += exp(wf_log_i0(a * x) - l0);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) red_s[k * WAVES + wave] = sum;
  }
  __syncthreads();
  if (tid < SC && i_mine < n_a) {
    const double a = sc_a[tid];
    double u = -INFINITY;
    if (a != 0.0) {
      double total = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) total += red_s[tid * WAVES + w];
      u = (sc_lp[tid] + (sc_l0[tid] - (a * a) * (0.5 * vhh))) + (log(total) - log((double)n));
    }
    row[tail_off + 1 + i_mine] = u;
  }
}

// One workgroup per task: its n_z = n_rows / n_tasks rows in order, then the mixture over them.
__global__ __launch_bounds__(kWfLlThreads) void waveform_scale_finish_kernel(
    const double* __restrict__ ws, int64_t row_doubles, int64_t tail_off, int n_rows, int n_tasks, int n_a, double* __restrict__ lnl_dist,
    int32_t* __restrict__ scale_index, double* __restrict__ scale_hat, double* __restrict__ lnl_amp_max, double* __restrict__ lnl_dist_mix,
    double* __restrict__ post, double* __restrict__ post_mix) {
  constexpr int WAVES = kWfLlThreads / 64;
  __shared__ double red_v[WAVES];
  __shared__ int red_i[WAVES];
  __shared__ double mix_sh[2];  // the mixture's shift and the log of its shifted sum
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_z = n_rows / n_tasks;
  // running log-sum-exp over the rows (thread 0): the largest max_i u_i so far and the sum of exp(u_i - it) over the rows' scales
  double mix_m = -INFINITY, mix_s = 0.0;

  for (int s = 0; s < n_z; ++s) {
    const int r = s * n_tasks + b;
    const double* row = ws + (size_t)r * (size_t)row_doubles;
    const double* u = row + tail_off + 1;

    double best = -INFINITY;
    int best_i = INT_MAX;
    for (int i = tid; i < n_a; i += kWfLlThreads) {
      const double v = u[i];
      if (v > best) {  // (i ascends: the smallest index of the thread stays)
        best = v;
        best_i = i;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(best_i, off);
      if (ob > best || (ob == best && oi < best_i)) {
        best = ob;
        best_i = oi;
      }
    }
    __syncthreads();  // (red_* may still be read for the previous row)
    if (lane == 0) {
      red_v[wave] = best;
      red_i[wave] = best_i;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const double ob = red_v[w];
      const int oi = red_i[w];
      if (w == 0 || ob > best || (ob == best && oi < best_i)) {
        best = ob;
        best_i = oi;
      }
    }
    const bool none = !(best > -INFINITY);  // no live scale (every thread: the same bits)

    double sum = 0.0;
    if (!none) {
      for (int i = tid; i < n_a; i += kWfLlThreads) sum += exp(u[i] - best);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();  // (the maximum has been read by every thread)
    if (lane == 0) red_v[wave] = sum;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += red_v[w];
    const double log_total = none ? 0.0 : log(total);
    if (post) {
      double* o = post + (size_t)r * (size_t)n_a;
      for (int i = tid; i < n_a; i += kWfLlThreads) o[i] = none ? -INFINITY : (u[i] - best) - log_total;
    }
    if (tid == 0) {
      const double vhh = row[0], x_best = row[tail_off];
      if (lnl_dist) lnl_dist[r] = none ? -INFINITY : best + log_total;
      if (scale_index) scale_index[r] = none ? 0 : best_i;
      if (scale_hat) scale_hat[r] = vhh == 0.0 ? 0.0 : x_best / vhh;
      if (lnl_amp_max) lnl_amp_max[r] = vhh == 0.0 ? 0.0 : (x_best * x_best) / (2.0 * vhh);
      if (!none) {
        if (best > mix_m) {
          mix_s = mix_s * exp(mix_m - best) + total;
          mix_m = best;
        } else {
          mix_s += exp(best - mix_m) * total;
        }
      }
    }
  }
  if (tid == 0) {
    const bool none = !(mix_m > -INFINITY);
    const double log_s = none ? 0.0 : log(mix_s);
    if (lnl_dist_mix) lnl_dist_mix[b] = none ? -INFINITY : mix_m + (log_s - log((double)n_z));
    mix_sh[0] = mix_m;
    mix_sh[1] = log_s;
  }
  __syncthreads();
  if (post_mix) {  // ln (sum_s exp u_i[s]) - ln (sum_s sum_i exp u_i[s]): ln n_z cancels
    const double m_all = mix_sh[0], log_s = mix_sh[1];
    const double* u0 = ws + (size_t)b * (size_t)row_doubles + tail_off + 1;
    const size_t step = (size_t)n_tasks * (size_t)row_doubles;
    for (int i = tid; i < n_a; i += kWfLlThreads) {
      double m = -INFINITY;
      for (int s = 0; s < n_z; ++s) {
        const double v = u0[(size_t)s * step + i];
        if (v > m) m = v;
      }
      double out = -INFINITY;
      if (m > -INFINITY) {
        double acc = 0.0;
        for (int s = 0; s < n_z; ++s) acc += exp(u0[(size_t)s * step + i] - m);
        out = (m - m_all) + (log(acc) - log_s);
      }
      post_mix[(size_t)b * (size_t)n_a + i] = out;
    }
  }
}

static bool wf_dist_args_bad(const double* scales, int scale_rows, const double* log_prior, int prior_rows, int n_a, int n_tasks) {
  if (n_a < 1 || n_a > kWfDistMaxScales || !scales || !log_prior) return true;
  if (scale_rows != 1 && scale_rows != n_tasks) return true;
  if (prior_rows != 1 && prior_rows != n_tasks) return true;
  return false;
}

// Launches A and B over rows of row_doubles doubles whose tail starts at tail_off; cand_off: where the parent keeps (Re, Im).
static int wf_dist_launch(double* ws, int64_t row_doubles, int cand_off, int64_t tail_off, int n_rows, int n_tasks, int n_tau,
                          const double* scales, int scale_rows, const double* log_prior, int prior_rows, int n_a, double* lnl_dist,
                          int32_t* scale_index, double* scale_hat, double* lnl_amp_max, double* lnl_dist_mix, double* post,
                          double* post_mix, hipStream_t stream) {
  const int n = n_tau > 0 ? n_tau : 1;
  const size_t lds = n <= kWfDistLdsTau ? (size_t)n * sizeof(double) : 0;
  hipLaunchKernelGGL(waveform_scale_marg_kernel<kWfDistSC>, dim3(n_rows, (n_a + kWfDistSC - 1) / kWfDistSC), dim3(kWfLlThreads), lds, stream,
                     ws, row_doubles, cand_off, tail_off, n_tasks, n_tau, scales, (int)(scale_rows != 1), log_prior, (int)(prior_rows != 1),
                     n_a);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(waveform_scale_finish_kernel, dim3(n_tasks), dim3(kWfLlThreads), 0, stream, ws, row_doubles, tail_off, n_rows, n_tasks,
                     n_a, lnl_dist, scale_index, scale_hat, lnl_amp_max, lnl_dist_mix, post, post_mix);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_dist_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t n_tau, int32_t n_a) {
  using namespace npf;
  if (n_rows <= 0 || n_det < 0 || n_det > NPF_NET_MAX_DET || n_tau < 0 || n_tau > kWfMaxTau || n_a < 1 || n_a > kWfDistMaxScales)
    return NPF_EINVAL;
  const int64_t parent = n_det == 0 ? wf_row_doubles(n_tau) : wf_net_row_doubles(n_det, n_tau);
  return (int64_t)n_rows * (parent + 1 + (int64_t)n_a) * (int64_t)sizeof(double);
}

extern "C" int npf_waveform_loglike_dist(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows, const float* freq,
                                         int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts,
                                         double tau0, double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max,
                                         double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                                         double* lnl_max_mix, const double* scales, int32_t scale_rows, const double* log_prior,
                                         int32_t prior_rows, int32_t n_a, double* lnl_dist, int32_t* scale_index, double* scale_hat,
                                         double* lnl_amp_max, double* lnl_dist_mix, double* post, double* post_mix, void* workspace,
                                         void* stream) {
  using namespace npf;
  if (wf_loglike_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_rows, n_tasks, pts, n_tau, workspace)) return NPF_EINVAL;
  if (wf_dist_args_bad(scales, scale_rows, log_prior, prior_rows, n_a, n_tasks)) return NPF_EINVAL;
  const bool parent = hh || dd || snr || lnl_max || lnl_marg || tau_index || phase || series || lnl_mix || lnl_max_mix;
  const bool mine = lnl_dist || scale_index || scale_hat || lnl_amp_max || lnl_dist_mix || post || post_mix;
  if (!parent && !mine) return NPF_EINVAL;
  const int64_t tail_off = wf_row_doubles(n_tau), row_doubles = tail_off + 1 + n_a;
  double* ws = (double*)workspace;
  const int rc = wf_loglike_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, hh, dd, snr,
                                   lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, ws, row_doubles, parent,
                                   (hipStream_t)stream);
  if (rc != NPF_OK || !mine) return rc;
  return wf_dist_launch(ws, row_doubles, n_tau > 0 ? 4 : 2, tail_off, n_rows, n_tasks, n_tau, scales, scale_rows, log_prior, prior_rows, n_a,
                        lnl_dist, scale_index, scale_hat, lnl_amp_max, lnl_dist_mix, post, post_mix, (hipStream_t)stream);
}

extern "C" int npf_waveform_loglike_net_dist(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                             const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* delay,
                                             const double* resp, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, double tau0,
                                             double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max,
                                             double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                                             double* lnl_max_mix, double* hh_det, double* snr_det, double* dd_det, const double* scales,
                                             int32_t scale_rows, const double* log_prior, int32_t prior_rows, int32_t n_a, double* lnl_dist,
                                             int32_t* scale_index, double* scale_hat, double* lnl_amp_max, double* lnl_dist_mix,
                                             double* post, double* post_mix, void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_net_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, delay, resp, n_rows, n_tasks, n_det, pts, n_tau, workspace))
    return NPF_EINVAL;
  if (wf_dist_args_bad(scales, scale_rows, log_prior, prior_rows, n_a, n_tasks)) return NPF_EINVAL;
  const bool parent = hh || dd || snr || lnl_max || lnl_marg || tau_index || phase || series || lnl_mix || lnl_max_mix || hh_det ||
                      snr_det || dd_det;
  const bool mine = lnl_dist || scale_index || scale_hat || lnl_amp_max || lnl_dist_mix || post || post_mix;
  if (!parent && !mine) return NPF_EINVAL;
  const int64_t tail_off = wf_net_row_doubles(n_det, n_tau), row_doubles = tail_off + 1 + n_a;
  double* ws = (double*)workspace;
  const int rc = wf_loglike_net_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, delay, resp, n_rows, n_tasks, n_det, pts, tau0,
                                       dtau, n_tau, hh, dd, snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, hh_det,
                                       snr_det, dd_det, ws, row_doubles, parent, (hipStream_t)stream);
  if (rc != NPF_OK || !mine) return rc;
  return wf_dist_launch(ws, row_doubles, 2 + 2 * n_det, tail_off, n_rows, n_tasks, n_tau, scales, scale_rows, log_prior, prior_rows, n_a,
                        lnl_dist, scale_index, scale_hat, lnl_amp_max, lnl_dist_mix, post, post_mix, (hipStream_t)stream);
}
