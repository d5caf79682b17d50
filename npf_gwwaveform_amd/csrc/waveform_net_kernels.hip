// Coherent matched-filter log likelihood of a detector network (npf_waveform_loglike_net): detector k < D sees the predicted waveform
// h_t = A_t e^{i phi_t} with its own noise weights w_{k,t}, its own arrival delay and its own complex response C_k,
//   kappa_{k,j} = sum_t w_{k,t} A_t e^{i (phi_t + 2 pi f_t (tau_j + delay_k))} conj(d_{k,t}),   hh_k = sum_t w_{k,t} A_t^2,
//   K_j = sum_k C_k kappa_{k,j},   HH = sum_k |C_k|^2 hh_k,   DD = sum_k dd_k,
// and the outputs of npf_waveform_loglike are formed from (K_j, HH, DD): the complex sums are added BEFORE the modulus is taken, one
// phase and one grid time are shared by the detectors.  The delays are device doubles that enter the sincos argument, so they are
// carried exactly and need not lie on the grid.  Everything in double from fp32 inputs widened exactly.
//
// Launch 1 (waveform_filter_net_kernel): geometry, recurrence and reduction order of waveform_filter_kernel -- one workgroup per
// (row, chunk of JC shifts) -- with the detector loop INSIDE the workgroup: per detector the 2 JC register sums are zeroed, the
// points strided with c = w_k A conj(d_k) (one sincos at the chunk's first shift plus the delay, one of the step, four FMAs per
// further shift), reduced (xor shuffles, then the waves through LDS), and reducing thread i adds its component of C_k kappa_{k,j}
// to a network sum it keeps in one register.  The sums per thread do not grow with D; detectors are added in ascending k.  The
// chunk-0 workgroup also reduces hh_k and dd_k and thread 0 adds |C_k|^2 hh_k and dd_k.
// Launch 2 (waveform_loglike_net_finish_kernel): waveform_loglike_finish_kernel over the network sums; for snr_det it forms the D
// sums kappa_{k,j*} again at the one shift j* (a direct sincos per live point), so no per-detector series is kept.
// No atomics anywhere: a second call on the same inputs gives the same bits.
//
// Workspace, doubles, per row: [HH, DD, hh_k (k < D), dd_k (k < D), (Re K_j, Im K_j) for j < JC * chunks].
#include "waveform_common.hpp"

namespace npf {

constexpr int kWfNetMaxDet = NPF_NET_MAX_DET;

template <int JC, int THREADS>
__global__ __launch_bounds__(THREADS) void waveform_filter_net_kernel(
    const float* __restrict__ h, int h_ld, const float* __restrict__ d, const float* __restrict__ wgt, int wgt_per_task,
    const float* __restrict__ freq, int freq_per_task, const int32_t* __restrict__ n_valid, const double* __restrict__ delay,
    const double* __restrict__ resp, int n_tasks, int n_det, int pts, double tau0, double dtau, int n_tau, double* __restrict__ ws,
    int64_t row_doubles) {
  __shared__ double red[2 * JC * (THREADS / 64)];
  __shared__ double kap[2 * JC];  // (Re, Im) of the detector's kappa_j
  __shared__ double bas[2];       // hh_k, dd_k
  const int r = blockIdx.x, chunk = blockIdx.y, b = r % n_tasks, tid = threadIdx.x;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
  const float* fr = freq ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;  // (NULL: no grid and no delays)
  const double tau_c = tau0 + (double)(chunk * JC) * dtau;  // the chunk's first shift (no grid: tau0 = dtau = 0, one chunk)
  const bool first = chunk == 0;
  double* row = ws + (size_t)r * (size_t)row_doubles;

  double net = 0.0;                // thread i < 2 JC: component i of K_j, j = chunk * JC + i / 2
  double sum_hh = 0.0, sum_dd = 0.0;  // thread 0 of chunk 0: HH, DD

  for (int k = 0; k < n_det; ++k) {
    const size_t bk = (size_t)b * (size_t)n_det + (size_t)k;
    const float* dr = d + bk * (size_t)pts * 2;
    const float* wr = wgt ? wgt + (wgt_per_task ? bk : (size_t)k) * (size_t)pts : nullptr;
    const double tau_k = tau_c + (delay ? delay[bk] : 0.0);

    double acc[2 * JC];  // (Re, Im) of kappa_{k,j}, j = chunk * JC + 0 .. JC - 1
#pragma unroll
    for (int i = 0; i < 2 * JC; ++i) acc[i] = 0.0;
    double base[2] = {0.0, 0.0};  // hh_k, dd_k (chunk 0 only)

    for (int t = tid; t < nv; t += THREADS) {
      const float wf = wr ? wr[t] : 1.f;
      if (!(wf > 0.f && wf < INFINITY)) continue;  // not live for this detector: nothing else of it is read
      const double w = (double)wf;
      const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
      const double dre = (double)dr[2 * (size_t)t], dim = (double)dr[2 * (size_t)t + 1];
      const double wa = w * A, cr = wa * dre, ci = -(wa * dim);  // c = w A conj(d)
      if (first) {
        base[0] += wa * A;
        base[1] += w * (dre * dre + dim * dim);
      }
      const double om = fr ? kWfTwoPi * (double)fr[t] : 0.0;
      double sn, cs, ssn, scs;
      sincos(ph + om * tau_k, &sn, &cs);
      sincos(om * dtau, &ssn, &scs);
      double zr = cs * cr - sn * ci, zi = cs * ci + sn * cr;
#pragma unroll
      for (int j = 0; j < JC; ++j) {
        acc[2 * j] += zr;
        acc[2 * j + 1] += zi;
        const double nr = zr * scs - zi * ssn;
        zi = zr * ssn + zi * scs;
        zr = nr;
      }
    }

    block_sum_store<2 * JC, THREADS>(acc, red, kap);
    __syncthreads();
    const double c_re = resp[2 * bk], c_im = resp[2 * bk + 1];  // (read here: not live across the point loop)
    if (tid < 2 * JC) {  // C_k kappa_{k,j}: Re = C_re Re - C_im Im, Im = C_re Im + C_im Re
      const double re = kap[tid & ~1], im = kap[tid | 1];
      net += (tid & 1) ? c_re * im + c_im * re : c_re * re - c_im * im;
    }
    if (first) {
      block_sum_store<2, THREADS>(base, red, bas);
      __syncthreads();
      if (tid == 0) {
        row[2 + k] = bas[0];
        row[2 + n_det + k] = bas[1];
        sum_hh += (c_re * c_re + c_im * c_im) * bas[0];
        sum_dd += bas[1];
      }
    }
  }

  if (tid < 2 * JC) row[2 + 2 * n_det + 2 * JC * chunk + tid] = net;
  if (first && tid == 0) {
    row[0] = sum_hh;
    row[1] = sum_dd;
  }
}

// One workgroup per task: its n_z = n_rows / n_tasks rows in order, then the two log-mean-exps over them.
__global__ __launch_bounds__(kWfLlThreads) void waveform_loglike_net_finish_kernel(
    const double* __restrict__ ws, int64_t row_doubles, const float* __restrict__ h, int h_ld, const float* __restrict__ d,
    const float* __restrict__ wgt, int wgt_per_task, const float* __restrict__ freq, int freq_per_task,
    const int32_t* __restrict__ n_valid, const double* __restrict__ delay, int n_rows, int n_tasks, int n_det, int pts, double tau0,
    double dtau, int n_tau, double* __restrict__ hh, double* __restrict__ dd, double* __restrict__ snr, double* __restrict__ lnl_max,
    double* __restrict__ lnl_marg, int32_t* __restrict__ tau_index, double* __restrict__ phase, double* __restrict__ series,
    double* __restrict__ lnl_mix, double* __restrict__ lnl_max_mix, double* __restrict__ hh_det, double* __restrict__ snr_det,
    double* __restrict__ dd_det) {
  constexpr int WAVES = kWfLlThreads / 64;
  __shared__ double red_v[2 * WAVES];
  __shared__ int red_j[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = n_tau > 0 ? n_tau : 1, n_z = n_rows / n_tasks;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const float* fr = freq ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;  // (NULL: no grid and no delays)
  const double log_n = log((double)n);
  // running log-sum-exp over the rows (thread 0): maximum so far and the sum of exp(value - maximum)
  double mix_m = 0.0, mix_s = 0.0, mxm_m = 0.0, mxm_s = 0.0;

  for (int s = 0; s < n_z; ++s) {
    const int r = s * n_tasks + b;
    const double* row = ws + (size_t)r * (size_t)row_doubles;
    const double vhh = row[0];
    const bool degenerate = vhh == 0.0;  // (no live point, a zero template or no response: Lambda = 1)
    const double half_hh = 0.5 * vhh, rt_hh = sqrt(vhh);
    const double* c = row + 2 + 2 * n_det;

    double best = -1.0;
    int best_j = 0;
    for (int j = tid; j < n; j += kWfLlThreads) {
      const double re = c[2 * j], im = c[2 * j + 1], m2 = re * re + im * im;
      if (m2 > best) {  // (j ascends: the smallest index of the thread stays)
        best = m2;
        best_j = j;
      }
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
    __syncthreads();  // (red_* may still be read for the previous row)
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
    if (degenerate) best_j = 0;
    const double x_best = sqrt(best), li0_best = wf_log_i0(x_best);  // (every thread: the same bits)

    double sum = 0.0;
    for (int j = tid; j < n; j += kWfLlThreads) {
      const double re = c[2 * j], im = c[2 * j + 1], x = sqrt(re * re + im * im), li0 = wf_log_i0(x);
      sum += exp(li0 - li0_best);
      if (series) {
        double* o = series + ((size_t)r * (size_t)n + (size_t)j) * 2;
        o[0] = degenerate ? 0.0 : li0 - half_hh;
        o[1] = degenerate ? 0.0 : x / rt_hh;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();  // (the maximum has been read by every thread)
    if (lane == 0) red_v[wave] = sum;
    __syncthreads();
    if (tid == 0) {
      double total = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) total += red_v[w];
      const double v_max = degenerate ? 0.0 : x_best - half_hh;
      const double v_marg = degenerate ? 0.0 : (li0_best - half_hh) + (log(total) - log_n);
      if (hh) hh[r] = vhh;
      if (dd && s == 0) dd[b] = row[1];
      if (snr) snr[r] = degenerate ? 0.0 : x_best / rt_hh;
      if (lnl_max) lnl_max[r] = v_max;
      if (lnl_marg) lnl_marg[r] = v_marg;
      if (tau_index) tau_index[r] = best_j;
      if (phase) phase[r] = degenerate ? 0.0 : atan2(c[2 * best_j + 1], c[2 * best_j]);
      if (s == 0) {
        mix_m = v_marg, mix_s = 1.0, mxm_m = v_max, mxm_s = 1.0;
      } else {
        if (v_marg > mix_m) {
          mix_s = mix_s * exp(mix_m - v_marg) + 1.0;
          mix_m = v_marg;
        } else {
          mix_s += exp(v_marg - mix_m);
        }
        if (v_max > mxm_m) {
          mxm_s = mxm_s * exp(mxm_m - v_max) + 1.0;
          mxm_m = v_max;
        } else {
          mxm_s += exp(v_max - mxm_m);
        }
      }
    }
    if (tid < n_det) {
      if (hh_det) hh_det[(size_t)r * (size_t)n_det + tid] = row[2 + tid];
      if (dd_det && s == 0) dd_det[(size_t)b * (size_t)n_det + tid] = row[2 + n_det + tid];
    }

    if (snr_det) {  // |kappa_{k,j*}| / sqrt(hh_k): the detector's sum once more, at the one shift j* (a degenerate row: j* = 0)
      const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
      const double tau_best = tau0 + (double)best_j * dtau;  // (no grid: tau0 = dtau = 0)
      for (int k = 0; k < n_det; ++k) {
        const double hh_k = row[2 + k];
        if (hh_k == 0.0) {  // (the same for every thread)
          if (tid == 0) snr_det[(size_t)r * (size_t)n_det + k] = 0.0;
          continue;
        }
        const size_t bk = (size_t)b * (size_t)n_det + (size_t)k;
        const float* dr = d + bk * (size_t)pts * 2;
        const float* wr = wgt ? wgt + (wgt_per_task ? bk : (size_t)k) * (size_t)pts : nullptr;
        const double tau_k = tau_best + (delay ? delay[bk] : 0.0);
        double kr = 0.0, ki = 0.0;
        for (int t = tid; t < nv; t += kWfLlThreads) {
          const float wf = wr ? wr[t] : 1.f;
          if (!(wf > 0.f && wf < INFINITY)) continue;
          const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
          const double dre = (double)dr[2 * (size_t)t], dim = (double)dr[2 * (size_t)t + 1];
          const double wa = (double)wf * A, cr = wa * dre, ci = -(wa * dim);
          const double om = fr ? kWfTwoPi * (double)fr[t] : 0.0;
          double sn, cs;
          sincos(ph + om * tau_k, &sn, &cs);
          kr += cs * cr - sn * ci;
          ki += cs * ci + sn * cr;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          kr += __shfl_xor(kr, off);
          ki += __shfl_xor(ki, off);
        }
        __syncthreads();  // (red_v may still be read for the previous detector or the row's sum)
        if (lane == 0) {
          red_v[2 * wave] = kr;
          red_v[2 * wave + 1] = ki;
        }
        __syncthreads();
        if (tid == 0) {
          double tr = 0.0, ti = 0.0;
#pragma unroll
          for (int w = 0; w < WAVES; ++w) {
            tr += red_v[2 * w];
            ti += red_v[2 * w + 1];
          }
          snr_det[(size_t)r * (size_t)n_det + k] = sqrt(tr * tr + ti * ti) / sqrt(hh_k);
        }
      }
    }
  }
  if (tid == 0) {
    const double log_nz = log((double)n_z);
    if (lnl_mix) lnl_mix[b] = mix_m + (log(mix_s) - log_nz);
    if (lnl_max_mix) lnl_max_mix[b] = mxm_m + (log(mxm_s) - log_nz);
  }
}

bool wf_loglike_net_args_bad(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                             const double* delay, const double* resp, int n_rows, int n_tasks, int n_det, int pts, int n_tau,
                             const void* workspace) {
  if (!h || !d || !workspace || h_ld < 2 || n_tasks <= 0 || n_rows <= 0 || n_rows > (1 << 24) || n_rows % n_tasks != 0 || pts <= 0)
    return true;
  if (n_tau < 0 || n_tau > kWfMaxTau || (n_tau > 0 && !freq)) return true;
  if (n_det < 1 || n_det > kWfNetMaxDet || !resp || (delay && !freq)) return true;
  if (wgt && wgt_rows != 1 && wgt_rows != n_tasks) return true;
  if (freq && freq_rows != 1 && freq_rows != n_tasks) return true;
  return false;
}

int wf_loglike_net_launch(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                          const int32_t* n_valid, const double* delay, const double* resp, int n_rows, int n_tasks, int n_det, int pts,
                          double tau0, double dtau, int n_tau, double* hh, double* dd, double* snr, double* lnl_max, double* lnl_marg,
                          int32_t* tau_index, double* phase, double* series, double* lnl_mix, double* lnl_max_mix, double* hh_det,
                          double* snr_det, double* dd_det, double* ws, int64_t row_doubles, bool finish, hipStream_t stream) {
  if (n_tau == 0) {  // the one candidate is tau = 0; without delays either, freq is not read
    tau0 = dtau = 0.0;
    if (!delay) freq = nullptr;
  }
  hipLaunchKernelGGL((waveform_filter_net_kernel<kWfJC, kWfThreads>), dim3(n_rows, wf_chunks(n_tau)), dim3(kWfThreads), 0, stream, h, h_ld,
                     d, wgt, (int)(wgt_rows != 1), freq, (int)(freq_rows != 1), n_valid, delay, resp, n_tasks, n_det, pts, tau0, dtau,
                     n_tau, ws, row_doubles);
  NPF_CHECK_LAUNCH();
  if (!finish) return NPF_OK;
  hipLaunchKernelGGL(waveform_loglike_net_finish_kernel, dim3(n_tasks), dim3(kWfLlThreads), 0, stream, ws, row_doubles, h, h_ld, d, wgt,
                     (int)(wgt_rows != 1), freq, (int)(freq_rows != 1), n_valid, delay, n_rows, n_tasks, n_det, pts, tau0, dtau, n_tau, hh,
                     dd, snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, hh_det, snr_det, dd_det);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_net_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t n_tau) {
  using namespace npf;
  if (n_rows <= 0 || n_det < 1 || n_det > kWfNetMaxDet || n_tau < 0 || n_tau > kWfMaxTau) return NPF_EINVAL;
  return (int64_t)n_rows * wf_net_row_doubles(n_det, n_tau) * (int64_t)sizeof(double);
}

extern "C" int npf_waveform_loglike_net(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                        const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* delay,
                                        const double* resp, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, double tau0,
                                        double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max,
                                        double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                                        double* lnl_max_mix, double* hh_det, double* snr_det, double* dd_det, void* workspace,
                                        void* stream) {
  using namespace npf;
  if (wf_loglike_net_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, delay, resp, n_rows, n_tasks, n_det, pts, n_tau, workspace))
    return NPF_EINVAL;
  if (!hh && !dd && !snr && !lnl_max && !lnl_marg && !tau_index && !phase && !series && !lnl_mix && !lnl_max_mix && !hh_det &&
      !snr_det && !dd_det)
    return NPF_EINVAL;
  return wf_loglike_net_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, delay, resp, n_rows, n_tasks, n_det, pts, tau0, dtau,
                               n_tau, hh, dd, snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, hh_det, snr_det,
                               dd_det, (double*)workspace, wf_net_row_doubles(n_det, n_tau), true, (hipStream_t)stream);
}
