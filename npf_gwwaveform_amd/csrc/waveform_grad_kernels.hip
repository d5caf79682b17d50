// Gradient of the matched-filter log likelihoods (npf_waveform_loglike, npf_waveform_loglike_net) with respect to the predicted
// waveform h_t = A_t e^{i phi_t}: the adjoint of their first launch.  With x_j = |kappa_j|, u_j = kappa_j / x_j (0 where x_j == 0),
// L_j = ln I0(x_j) - hh / 2, p_j = exp(L_j - logsumexp_j L_j), rho = I1 / I0 and the upstream gradients g_marg, g_max of a row's
// lnl_marg and lnl_max (the share of the two mixtures over the latent samples included):
//   q_j = p_j rho(x_j) conj(u_j)                                                     (|sum_j q_j| <= 1)
//   G_t = g_marg sum_j q_j e^{i 2 pi f_t tau_j} + g_max conj(u_{j*}) e^{i 2 pi f_t tau_{j*}}      (no grid: no time factor)
//   E_t = conj(d_t) e^{i phi_t}
//   dF/dA_t = w_t (Re(E_t G_t) - (g_marg + g_max) A_t),   dF/dphi_t = -w_t A_t Im(E_t G_t).
// The network: q_j from (K_j, HH), one G_t shared by the detectors, and per live detector in ascending k
//   E_{k,t} = C_k conj(d_{k,t}) e^{i (phi_t + 2 pi f_t delay_k)},  dA += w_{k,t} (Re(E_{k,t} G_t) - (g_marg + g_max) |C_k|^2 A_t),
//   dphi -= w_{k,t} A_t Im(E_{k,t} G_t).
//
// waveform_loglike_coef_kernel: one workgroup per row reads the workspace row launch 1 left, finds the maximum and the shifted sum in
// the order of waveform_loglike_finish_kernel -- so p_j is consistent with the lnl_marg the forward returned -- and writes the row of
// `saved`: [hh, Re conj(u_{j*}), Im conj(u_{j*}), 0, (Re q_j, Im q_j) j < n].  The workspace pool is shared and may be overwritten
// before the backward runs; `saved` is the caller's.
// waveform_loglike_bwd_kernel: grid (rows, point blocks), one thread per point with a grid-stride loop.  The workgroup stages
// kWfBwdTile shifts of g_marg q_j (+ g_max conj(u_{j*}) at j = j*) into LDS; every lane reads the same entry per step (a broadcast
// read).  Per point and chunk of kWfJC shifts one direct double sincos of 2 pi f_t tau_{j0}, one of 2 pi f_t dtau per point, then
// G += q_j z, z <- z s: 8 FMAs per (t, j), and the recurrence never runs longer than kWfJC steps -- the bound launch 1 has.  The
// sums stay in registers: no cross-thread reduction, no atomics, the same bits on a second call.
#include "waveform_common.hpp"

namespace npf {

constexpr int kWfBwdTile = 256;  // shifts per LDS tile of the backward launch: 4 KiB, one (Re, Im) pair per thread to stage
constexpr int kWfNetMaxDetGrad = NPF_NET_MAX_DET;
static_assert(kWfBwdTile % kWfJC == 0 && kWfBwdTile == kWfBwdThreads, "a tile is whole chunks, staged one shift per thread");

inline int64_t wf_saved_doubles(int n_tau) { return 4 + 2 * (int64_t)(n_tau > 0 ? n_tau : 1); }

// c_off: where the candidates start in a workspace row ([hh, dd, kappa_0/, kappa_j ..]: 4, or 2 without a grid; the network's
// [HH, DD, hh_k, dd_k, K_j ..]: 2 + 2 D).  n = max(n_tau, 1).
__global__ __launch_bounds__(kWfLlThreads) void waveform_loglike_coef_kernel(const double* __restrict__ ws, int64_t row_doubles, int c_off,
                                                                             int n, double* __restrict__ saved) {
  constexpr int WAVES = kWfLlThreads / 64;
  __shared__ double red_v[WAVES];
  __shared__ int red_j[WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* row = ws + (size_t)r * (size_t)row_doubles;
  const double* c = row + c_off;
  double* sv = saved + (size_t)r * (size_t)(4 + 2 * (int64_t)n);
  const double vhh = row[0];
  if (vhh == 0.0) {  // (the same for every thread) no live point, a zero template or no response: Lambda = 1, no gradient
    for (int i = tid; i < 4 + 2 * n; i += kWfLlThreads) sv[i] = 0.0;
    return;
  }

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
  const double x_best = sqrt(best), li0_best = wf_log_i0(x_best);  // (every thread: the same bits)

  double sum = 0.0;
  for (int j = tid; j < n; j += kWfLlThreads) {
    const double re = c[2 * j], im = c[2 * j + 1], x = sqrt(re * re + im * im);
    sum += exp(wf_log_i0(x) - li0_best);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  __syncthreads();  // (the maximum has been read by every thread)
  if (lane == 0) red_v[wave] = sum;
  __syncthreads();
  double total = 0.0;  // (every thread: the waves in order, the bits the finishing kernel's thread 0 forms)
#pragma unroll
  for (int w = 0; w < WAVES; ++w) total += red_v[w];

  for (int j = tid; j < n; j += kWfLlThreads) {
    const double re = c[2 * j], im = c[2 * j + 1], x = sqrt(re * re + im * im);
    const double pr = (exp(wf_log_i0(x) - li0_best) / total) * wf_i1_over_i0(x);  // p_j rho(x_j)
    const bool dir = x > 0.0;                                                       // (x == 0: rho = 0, and no direction)
    sv[4 + 2 * j] = dir ? pr * (re / x) : 0.0;
    sv[5 + 2 * j] = dir ? -(pr * (im / x)) : 0.0;
  }
  if (tid == 0) {
    const double re = c[2 * best_j], im = c[2 * best_j + 1];
    const bool dir = x_best > 0.0;
    sv[0] = vhh;
    sv[1] = dir ? re / x_best : 0.0;
    sv[2] = dir ? -(im / x_best) : 0.0;
    sv[3] = 0.0;
  }
}

// LD: dh_ld when it is 2 or 4 and d_h is aligned to a whole point (one 8- / 16-byte store per point), 0 for any other leading
// dimension.  NET: d [n_tasks][n_det][pts][2], wgt per detector, delay and resp as in waveform_filter_net_kernel; else n_det is 1 and
// delay / resp are not read.  freq may be NULL where there is neither a grid nor (NET) a delay.  Every element of the n_bcast row
// blocks of d_h is written; a point that is not live (for any detector) and every point of a row with hh == 0 are SELECTED to zero:
// nothing of them, and of such a row's upstream gradients, is read.
template <int LD, bool NET>
__global__ __launch_bounds__(kWfBwdThreads) void waveform_loglike_bwd_kernel(
    const float* __restrict__ h, int h_ld, const float* __restrict__ d, const float* __restrict__ wgt, int wgt_per_task,
    const float* __restrict__ freq, int freq_per_task, const int32_t* __restrict__ n_valid, const double* __restrict__ delay,
    const double* __restrict__ resp, int n_rows, int n_tasks, int n_det, int pts, double tau0, double dtau, int n_tau,
    const int32_t* __restrict__ tau_index, const double* __restrict__ saved, const double* __restrict__ lnl_marg,
    const double* __restrict__ lnl_max, const double* __restrict__ lnl_mix, const double* __restrict__ lnl_max_mix,
    const double* __restrict__ d_marg, const double* __restrict__ d_max, const double* __restrict__ d_mix,
    const double* __restrict__ d_max_mix, int n_bcast, float* __restrict__ d_h, int dh_ld) {
  __shared__ double2 q_s[kWfBwdTile];
  const int r = blockIdx.x, b = r % n_tasks, tid = threadIdx.x;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const bool grid = n_tau > 0;
  const int n = grid ? n_tau : 1;
  const double* sv = saved + (size_t)r * (size_t)(4 + 2 * (int64_t)n);
  const bool live_row = sv[0] != 0.0;  // (hh == 0: the coefficient kernel wrote zeros)
  // the total upstream gradients of the row's lnl_marg and lnl_max (workgroup-uniform), already divided by n_bcast
  double g_marg = 0.0, g_max = 0.0;
  if (live_row) {
    const double inv_nz = 1.0 / (double)(n_rows / n_tasks);
    if (d_marg) g_marg += d_marg[r];
    if (d_mix) g_marg += d_mix[b] * exp(lnl_marg[r] - lnl_mix[b]) * inv_nz;
    if (d_max) g_max += d_max[r];
    if (d_max_mix) g_max += d_max_mix[b] * exp(lnl_max[r] - lnl_max_mix[b]) * inv_nz;
    g_marg /= (double)n_bcast;
    g_max /= (double)n_bcast;
  }
  const double g_sum = g_marg + g_max;
  const double ur = live_row ? g_max * sv[1] : 0.0, ui = live_row ? g_max * sv[2] : 0.0;  // g_max conj(u_{j*})
  const int j_star = grid && live_row ? tau_index[r] : 0;
  const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
  const float* fr = freq ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;
  const size_t bk0 = (size_t)b * (size_t)n_det;  // (single stream: n_det == 1, so task b)
  const size_t block_stride = (size_t)n_rows * (size_t)pts * (size_t)dh_ld;

  // (the loop bounds are the same for every thread of the workgroup: the barriers inside are reached by all of them)
  for (int64_t base = (int64_t)blockIdx.y * kWfBwdThreads; base < pts; base += (int64_t)gridDim.y * kWfBwdThreads) {
    const int64_t t = base + tid;
    bool live = live_row && t < nv;
    float w1 = 1.f;
    if (live) {
      if (NET) {  // live for at least one detector
        bool any = wgt == nullptr;
        for (int k = 0; k < n_det && !any; ++k) {
          const float wf = wgt[(wgt_per_task ? bk0 + k : (size_t)k) * (size_t)pts + (size_t)t];
          any = wf > 0.f && wf < INFINITY;
        }
        live = any;
      } else {
        w1 = wgt ? wgt[(wgt_per_task ? (size_t)b * (size_t)pts : 0) + (size_t)t] : 1.f;
        live = w1 > 0.f && w1 < INFINITY;  // (else a removed point: nothing else of it is read)
      }
    }
    double om = 0.0, ssn = 0.0, scs = 1.0, Gr = 0.0, Gi = 0.0;
    if (live && fr) {
      om = kWfTwoPi * (double)fr[t];
      if (grid) sincos(om * dtau, &ssn, &scs);
    }
    if (live_row) {
      for (int j0 = 0; j0 < n; j0 += kWfBwdTile) {
        __syncthreads();  // (the previous tile may still be read)
        {
          const int j = j0 + tid;
          double2 v = make_double2(0.0, 0.0);  // (beyond the grid: zeros, so that the last chunk runs whole)
          if (j < n) {
            v.x = g_marg * sv[4 + 2 * (size_t)j];
            v.y = g_marg * sv[5 + 2 * (size_t)j];
            if (j == j_star) {
              v.x += ur;
              v.y += ui;
            }
          }
          q_s[tid] = v;
        }
        __syncthreads();
        if (live) {
          const int lim = n - j0 < kWfBwdTile ? n - j0 : kWfBwdTile;
          for (int c0 = 0; c0 < lim; c0 += kWfJC) {
            double zr = 1.0, zi = 0.0;
            if (grid) sincos(om * (tau0 + (double)(j0 + c0) * dtau), &zi, &zr);  // the chunk's first shift, directly
#pragma unroll
            for (int j = 0; j < kWfJC; ++j) {
              const double2 q = q_s[c0 + j];
              Gr += q.x * zr - q.y * zi;
              Gi += q.x * zi + q.y * zr;
              const double nr = zr * scs - zi * ssn;
              zi = zr * ssn + zi * scs;
              zr = nr;
            }
          }
        }
      }
    }
    if (t >= pts) continue;  // (after the barriers)

    float dA = 0.f, dphi = 0.f;
    if (live) {
      const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
      if (NET) {
        double a = 0.0, p = 0.0, sn = 0.0, cs = 1.0;
        if (!delay) sincos(ph, &sn, &cs);
        for (int k = 0; k < n_det; ++k) {  // ascending k
          const size_t bk = bk0 + (size_t)k;
          const float wf = wgt ? wgt[(wgt_per_task ? bk : (size_t)k) * (size_t)pts + (size_t)t] : 1.f;
          if (!(wf > 0.f && wf < INFINITY)) continue;  // not live for this detector: nothing else of it is read
          const double w = (double)wf, c_re = resp[2 * bk], c_im = resp[2 * bk + 1];
          const float* dr = d + (bk * (size_t)pts + (size_t)t) * 2;
          const double dre = (double)dr[0], dim = (double)dr[1];
          if (delay) sincos(ph + om * delay[bk], &sn, &cs);
          const double er = dre * cs + dim * sn, ei = dre * sn - dim * cs;      // conj(d) e^{i (phi + 2 pi f delay)}
          const double Er = c_re * er - c_im * ei, Ei = c_re * ei + c_im * er;  // times C_k
          const double re = Er * Gr - Ei * Gi, im = Er * Gi + Ei * Gr;
          a += w * (re - g_sum * (c_re * c_re + c_im * c_im) * A);
          p -= (w * A) * im;
        }
        dA = (float)a;
        dphi = (float)p;
      } else {
        const float* dr = d + ((size_t)b * (size_t)pts + (size_t)t) * 2;
        const double w = (double)w1, dre = (double)dr[0], dim = (double)dr[1];
        double sn, cs;
        sincos(ph, &sn, &cs);
        const double Er = dre * cs + dim * sn, Ei = dre * sn - dim * cs;  // conj(d) e^{i phi}
        const double re = Er * Gr - Ei * Gi, im = Er * Gi + Ei * Gr;
        dA = (float)(w * (re - g_sum * A));
        dphi = (float)(-((w * A) * im));
      }
    }
    float* o = d_h + ((size_t)r * (size_t)pts + (size_t)t) * (size_t)dh_ld;
    for (int q = 0; q < n_bcast; ++q, o += block_stride) {
      if (LD == 2) {
        *reinterpret_cast<float2*>(o) = make_float2(dA, dphi);
      } else if (LD == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(dA, dphi, 0.f, 0.f);
      } else {
        o[0] = dA;
        o[1] = dphi;
        for (int e = 2; e < dh_ld; ++e) o[e] = 0.f;
      }
    }
  }
}

static int wf_coef_launch(const double* ws, int64_t row_doubles, int c_off, int n_rows, int n_tau, double* saved, hipStream_t stream) {
  hipLaunchKernelGGL(waveform_loglike_coef_kernel, dim3(n_rows), dim3(kWfLlThreads), 0, stream, ws, row_doubles, c_off,
                     n_tau > 0 ? n_tau : 1, saved);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

// What both backward entries refuse beyond the forward's rules (workspace aside: the backward has none).
static bool wf_bwd_args_bad(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                            int n_rows, int n_tasks, int pts, int n_tau, const int32_t* tau_index, const double* saved,
                            const double* lnl_marg, const double* lnl_max, const double* lnl_mix, const double* lnl_max_mix,
                            const double* d_marg, const double* d_max, const double* d_mix, const double* d_max_mix, int n_bcast,
                            const float* d_h, int dh_ld) {
  if (!h || !d || !saved || !d_h || h_ld < 2 || dh_ld < 2 || n_bcast < 1 || n_tasks <= 0 || n_rows <= 0 || n_rows > (1 << 24) ||
      n_rows % n_tasks != 0 || pts <= 0)
    return true;
  if (n_tau < 0 || n_tau > kWfMaxTau || (n_tau > 0 && (!freq || !tau_index))) return true;
  if (wgt && wgt_rows != 1 && wgt_rows != n_tasks) return true;
  if (freq && freq_rows != 1 && freq_rows != n_tasks) return true;
  if (!d_marg && !d_max && !d_mix && !d_max_mix) return true;  // no upstream gradient at all
  if (d_mix && (!lnl_marg || !lnl_mix)) return true;           // a mixture's gradient needs the forward's values
  if (d_max_mix && (!lnl_max || !lnl_max_mix)) return true;
  return false;
}

template <bool NET>
static int wf_bwd_launch(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                         const int32_t* n_valid, const double* delay, const double* resp, int n_rows, int n_tasks, int n_det, int pts,
                         double tau0, double dtau, int n_tau, const int32_t* tau_index, const double* saved, const double* lnl_marg,
                         const double* lnl_max, const double* lnl_mix, const double* lnl_max_mix, const double* d_marg,
                         const double* d_max, const double* d_mix, const double* d_max_mix, int n_bcast, float* d_h, int dh_ld,
                         hipStream_t stream) {
  if (n_tau == 0) {  // the one candidate is tau = 0; without delays either, freq is not read
    tau0 = dtau = 0.0;
    if (!delay) freq = nullptr;
  }
  const int64_t blocks = ((int64_t)pts + kWfBwdThreads - 1) / kWfBwdThreads;
  const dim3 grid(n_rows, (unsigned)(blocks < kWfBwdMaxGridY ? blocks : kWfBwdMaxGridY)), block(kWfBwdThreads);
  const bool whole = (uintptr_t)d_h % ((size_t)dh_ld * sizeof(float)) == 0;  // one store per point needs the point aligned
#define NPF_WF_LL_BWD(LD)                                                                                                              \
  hipLaunchKernelGGL((waveform_loglike_bwd_kernel<LD, NET>), grid, block, 0, stream, h, h_ld, d, wgt, (int)(wgt_rows != 1), freq,      \
                     (int)(freq_rows != 1), n_valid, delay, resp, n_rows, n_tasks, n_det, pts, tau0, dtau, n_tau, tau_index, saved,    \
                     lnl_marg, lnl_max, lnl_mix, lnl_max_mix, d_marg, d_max, d_mix, d_max_mix, n_bcast, d_h, dh_ld)
  if (dh_ld == 2 && whole) {
    NPF_WF_LL_BWD(2);
  } else if (dh_ld == 4 && whole) {
    NPF_WF_LL_BWD(4);
  } else {
    NPF_WF_LL_BWD(0);
  }
#undef NPF_WF_LL_BWD
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_saved_doubles(int32_t n_tau) {
  using namespace npf;
  if (n_tau < 0 || n_tau > kWfMaxTau) return NPF_EINVAL;
  return wf_saved_doubles(n_tau);
}

extern "C" int npf_waveform_loglike_ex(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows, const float* freq,
                                       int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts,
                                       double tau0, double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max,
                                       double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                                       double* lnl_max_mix, double* saved, void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_rows, n_tasks, pts, n_tau, workspace) || !saved) return NPF_EINVAL;
  const int64_t row_doubles = wf_row_doubles(n_tau);
  const int rc = wf_loglike_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, hh, dd,
                                   snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, (double*)workspace,
                                   row_doubles, true, (hipStream_t)stream);
  if (rc != NPF_OK) return rc;
  return wf_coef_launch((const double*)workspace, row_doubles, n_tau > 0 ? 4 : 2, n_rows, n_tau, saved, (hipStream_t)stream);
}

extern "C" int npf_waveform_loglike_net_ex(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                           const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* delay,
                                           const double* resp, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, double tau0,
                                           double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max,
                                           double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                                           double* lnl_max_mix, double* hh_det, double* snr_det, double* dd_det, double* saved,
                                           void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_net_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, delay, resp, n_rows, n_tasks, n_det, pts, n_tau, workspace) ||
      !saved)
    return NPF_EINVAL;
  const int64_t row_doubles = wf_net_row_doubles(n_det, n_tau);
  const int rc = wf_loglike_net_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, delay, resp, n_rows, n_tasks, n_det, pts,
                                       tau0, dtau, n_tau, hh, dd, snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix,
                                       lnl_max_mix, hh_det, snr_det, dd_det, (double*)workspace, row_doubles, true, (hipStream_t)stream);
  if (rc != NPF_OK) return rc;
  return wf_coef_launch((const double*)workspace, row_doubles, 2 + 2 * n_det, n_rows, n_tau, saved, (hipStream_t)stream);
}

extern "C" int npf_waveform_loglike_bwd(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                        const float* freq, int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks,
                                        int32_t pts, double tau0, double dtau, int32_t n_tau, const int32_t* tau_index,
                                        const double* saved, const double* lnl_marg, const double* lnl_max, const double* lnl_mix,
                                        const double* lnl_max_mix, const double* d_marg, const double* d_max, const double* d_mix,
                                        const double* d_max_mix, int32_t n_bcast, float* d_h, int32_t dh_ld, void* stream) {
  using namespace npf;
  if (wf_bwd_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_rows, n_tasks, pts, n_tau, tau_index, saved, lnl_marg, lnl_max,
                      lnl_mix, lnl_max_mix, d_marg, d_max, d_mix, d_max_mix, n_bcast, d_h, dh_ld))
    return NPF_EINVAL;
  return wf_bwd_launch<false>(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, nullptr, nullptr, n_rows, n_tasks, 1, pts, tau0, dtau,
                              n_tau, tau_index, saved, lnl_marg, lnl_max, lnl_mix, lnl_max_mix, d_marg, d_max, d_mix, d_max_mix, n_bcast,
                              d_h, dh_ld, (hipStream_t)stream);
}

extern "C" int npf_waveform_loglike_net_bwd(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                            const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* delay,
                                            const double* resp, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, double tau0,
                                            double dtau, int32_t n_tau, const int32_t* tau_index, const double* saved,
                                            const double* lnl_marg, const double* lnl_max, const double* lnl_mix,
                                            const double* lnl_max_mix, const double* d_marg, const double* d_max, const double* d_mix,
                                            const double* d_max_mix, int32_t n_bcast, float* d_h, int32_t dh_ld, void* stream) {
  using namespace npf;
  if (wf_bwd_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_rows, n_tasks, pts, n_tau, tau_index, saved, lnl_marg, lnl_max,
                      lnl_mix, lnl_max_mix, d_marg, d_max, d_mix, d_max_mix, n_bcast, d_h, dh_ld))
    return NPF_EINVAL;
  if (n_det < 1 || n_det > kWfNetMaxDetGrad || !resp || (delay && !freq)) return NPF_EINVAL;
  return wf_bwd_launch<true>(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, delay, resp, n_rows, n_tasks, n_det, pts, tau0, dtau,
                             n_tau, tau_index, saved, lnl_marg, lnl_max, lnl_mix, lnl_max_mix, d_marg, d_max, d_mix, d_max_mix, n_bcast,
                             d_h, dh_ld, (hipStream_t)stream);
}
