// Match of predicted waveforms h_t = A_t e^{i phi_t} against reference waveforms g_t = A'_t e^{i phi'_t} over a uniform grid of time
// shifts tau_j = tau0 + j dtau (npf_waveform_match): the noise-weighted complex correlation
//   c_j = sum_t w_t A_t A'_t exp(i (phi_t - phi'_t + 2 pi f_t tau_j)),   hh = sum_t w_t A_t^2,   gg = sum_t w_t A'_t^2,
// c_0/ the same sum without the time-shift term, and per row overlap = Re c_0/ / sqrt(hh gg), match = max_j |c_j| / sqrt(hh gg) with
// the first index that attains it, phase = arg c there and mismatch = 1 - match.  A pure reduction, in DOUBLE throughout: useful
// mismatches are 1e-4 .. 1e-8 and the phases reach thousands of radians, where fp32 sines and sums are worth 1e-8 of the match.
// The inputs are fp32 values widened exactly; every output is rounded to fp32 once.
//
// Launch 1 (waveform_corr_kernel): one workgroup per (row, chunk of JC time shifts).  A thread strides over the points; per point it
// forms z = a_t e^{i (theta_t + 2 pi f_t tau_j0)} at the chunk's first shift and the step s = e^{i 2 pi f_t dtau} with one double
// sincos each and advances z <- z s through the chunk: four FMAs per (t, j), no sine in the inner loop, and the recurrence restarts
// from a direct sincos at every chunk, so it never runs longer than JC steps.  The 2 JC sums live in registers and are reduced in a
// fixed order (wave shuffles, then LDS across the waves) into the double workspace; the chunk-0 workgroup adds hh, gg and c_0/.
// Launch 2 (waveform_finish_kernel): one wavefront per row normalises, takes the maximum with the smallest index and writes the
// outputs.  No atomics anywhere: a second call on the same inputs gives the same bits.
//
// Workspace, doubles, per row: [hh, gg, Re c_0/, Im c_0/, (Re c_j, Im c_j) for j < JC * chunks].
#include "waveform_common.hpp"  // kWfJC, kWfThreads, kWfBwdThreads, kWfBwdMaxGridY, kWfMaxTau, kWfTwoPi, wf_chunks, block_sum_store; kWfLlThreads, wf_log_i0

namespace npf {

template <int JC, int THREADS>
__global__ __launch_bounds__(THREADS) void waveform_corr_kernel(const float* __restrict__ h, int h_ld, const float* __restrict__ g,
                                                                 const float* __restrict__ wgt, int wgt_per_task,
                                                                 const float* __restrict__ freq, int freq_per_task,
                                                                 const int32_t* __restrict__ n_valid, int n_tasks, int pts, double tau0,
                                                                 double dtau, int n_tau, double* __restrict__ ws, int64_t row_doubles) {
  __shared__ double red[2 * JC * (THREADS / 64)];
  const int r = blockIdx.x, chunk = blockIdx.y, b = r % n_tasks;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
  const float* gr = g + (size_t)b * (size_t)pts * 2;
  const float* wr = wgt ? wgt + (wgt_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;
  const float* fr = n_tau > 0 ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;  // (n_tau == 0: freq is not read)
  const double tau_c = tau0 + (double)(chunk * JC) * dtau;  // the chunk's first shift
  const bool first = chunk == 0;

  double acc[2 * JC];  // (Re, Im) of c_j, j = chunk * JC + 0 .. JC - 1
#pragma unroll
  for (int i = 0; i < 2 * JC; ++i) acc[i] = 0.0;
  double base[4] = {0.0, 0.0, 0.0, 0.0};  // hh, gg, Re c_0/, Im c_0/ (chunk 0 only)

  for (int t = threadIdx.x; t < nv; t += THREADS) {
    const float wf = wr ? wr[t] : 1.f;
    if (!(wf > 0.f && wf < INFINITY)) continue;  // a removed point: nothing else of it is read
    const double w = (double)wf;
    const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
    const double Ag = (double)gr[2 * (size_t)t], phg = (double)gr[2 * (size_t)t + 1];
    const double wa = w * A, a = wa * Ag, theta = ph - phg;
    if (first) {
      double sn, cs;
      sincos(theta, &sn, &cs);
      base[0] += wa * A;
      base[1] += (w * Ag) * Ag;
      base[2] += a * cs;
      base[3] += a * sn;
    }
    if (n_tau > 0) {
      const double om = kWfTwoPi * (double)fr[t];
      double sn, cs, ssn, scs;
      sincos(theta + om * tau_c, &sn, &cs);
      sincos(om * dtau, &ssn, &scs);
      double zr = a * cs, zi = a * sn;
#pragma unroll
      for (int j = 0; j < JC; ++j) {
        acc[2 * j] += zr;
        acc[2 * j + 1] += zi;
        const double nr = zr * scs - zi * ssn;
        zi = zr * ssn + zi * scs;
        zr = nr;
      }
    }
  }

  double* row = ws + (size_t)r * (size_t)row_doubles;
  if (n_tau > 0) block_sum_store<2 * JC, THREADS>(acc, red, row + 4 + 2 * JC * chunk);
  if (first) block_sum_store<4, THREADS>(base, red, row);
}

// One wavefront per row: the maximum of |c_j|^2 with the smallest index that attains it, then the outputs.
__global__ __launch_bounds__(64) void waveform_finish_kernel(const double* __restrict__ ws, int64_t row_doubles, int n_tasks, int n_tau,
                                                              float* __restrict__ hh, float* __restrict__ gg, float* __restrict__ overlap,
                                                              float* __restrict__ match, float* __restrict__ mismatch,
                                                              int32_t* __restrict__ tau_index, float* __restrict__ phase,
                                                              float* __restrict__ corr, double* __restrict__ saved) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const double* row = ws + (size_t)r * (size_t)row_doubles;
  const double vhh = row[0], vgg = row[1], prod = vhh * vgg;
  const bool degenerate = prod == 0.0;  // (no point left: both sums are empty)
  const double nrm = sqrt(prod);
  const int n = n_tau > 0 ? n_tau : 1;
  const double* c = n_tau > 0 ? row + 4 : row + 2;  // (no time maximisation: the one candidate is c_0/)

  double best = -1.0;
  int best_j = 0;
  for (int j = lane; j < n; j += 64) {
    const double re = c[2 * j], im = c[2 * j + 1], m2 = re * re + im * im;
    if (m2 > best) {  // (j ascends: the smallest index of the lane stays)
      best = m2;
      best_j = j;
    }
    if (corr) {
      float* o = corr + ((size_t)r * (size_t)n + (size_t)j) * 2;
      o[0] = degenerate ? 0.f : (float)(re / nrm);
      o[1] = degenerate ? 0.f : (float)(im / nrm);
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
  if (lane != 0) return;
  if (hh) hh[r] = (float)vhh;
  if (gg && r < n_tasks) gg[r] = (float)vgg;  // (row r < n_tasks is latent sample 0 of task r)
  const double re = c[2 * best_j], im = c[2 * best_j + 1];
  const double m = degenerate ? 0.0 : sqrt(re * re + im * im) / nrm;
  if (overlap) overlap[r] = degenerate ? 0.f : (float)(row[2] / nrm);
  if (match) match[r] = (float)m;
  if (mismatch) mismatch[r] = (float)(1.0 - m);
  if (tau_index) tau_index[r] = degenerate ? 0 : best_j;
  if (phase) phase[r] = degenerate ? 0.f : (float)atan2(im, re);
  if (saved) {  // what the backward launch starts from, unrounded
    double* sv = saved + 4 * (size_t)r;
    sv[0] = degenerate ? 0.0 : vhh;
    sv[1] = degenerate ? 0.0 : vgg;
    sv[2] = degenerate ? 0.0 : re;
    sv[3] = degenerate ? 0.0 : im;
  }
}

// Backward of the match with respect to (A, phi) at the maximiser the forward found: one thread per point, no reduction.  With
// c = c_{j*} = |c| e^{i psi}, N = sqrt(hh gg), M = |c| / N and theta_t = phi_t - phi'_t + 2 pi f_t tau*:
//   dM/dA_t = w_t (A'_t cos(theta_t - psi) / N - M A_t / hh),   dM/dphi_t = -w_t A_t A'_t sin(theta_t - psi) / N,
// where cos(theta - psi) = (cos theta Re c + sin theta Im c) / |c| and sin(theta - psi) = (sin theta Re c - cos theta Im c) / |c|:
// one sincos per point and no atan2.  Every element of the n_bcast row blocks of d_h is written; a removed or padded point and a
// degenerate row are SELECTED to zero (nothing of them is read or multiplied in).  LD: dh_ld when it is 2 or 4 and d_h is aligned
// to a whole point (one 8- / 16-byte store per point), 0 for any other leading dimension.
template <int LD>
__global__ __launch_bounds__(kWfBwdThreads) void waveform_match_bwd_kernel(
    const float* __restrict__ h, int h_ld, const float* __restrict__ g, const float* __restrict__ wgt, int wgt_per_task,
    const float* __restrict__ freq, int freq_per_task, const int32_t* __restrict__ n_valid, int n_rows, int n_tasks, int pts, double tau0,
    double dtau, int n_tau, const int32_t* __restrict__ tau_index, const double* __restrict__ saved, const float* __restrict__ d_match,
    int n_bcast, float* __restrict__ d_h, int dh_ld) {
  const int r = blockIdx.x, b = r % n_tasks;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const double* sv = saved + 4 * (size_t)r;
  const double vhh = sv[0], vgg = sv[1], re = sv[2], im = sv[3];
  const double prod = vhh * vgg, mag = sqrt(re * re + im * im);
  const bool live_row = prod > 0.0 && mag > 0.0;  // (a degenerate row; c = 0: no direction to move the phase in, M A / hh = 0)
  const double nrm = sqrt(prod);
  const double inv_n = live_row ? 1.0 / nrm : 0.0, m_hh = live_row ? (mag / nrm) / vhh : 0.0;
  const double ur = live_row ? re / mag : 0.0, ui = live_row ? im / mag : 0.0;  // e^{i psi}
  const double scale = live_row ? (double)d_match[r] / (double)n_bcast : 0.0;
  const double tau = n_tau > 0 ? tau0 + (double)tau_index[r] * dtau : 0.0;
  const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
  const float* gr = g + (size_t)b * (size_t)pts * 2;
  const float* wr = wgt ? wgt + (wgt_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;
  const float* fr = n_tau > 0 ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;
  const size_t block_stride = (size_t)n_rows * (size_t)pts * (size_t)dh_ld;

  for (int64_t t = (int64_t)blockIdx.y * kWfBwdThreads + threadIdx.x; t < pts; t += (int64_t)gridDim.y * kWfBwdThreads) {
    float dA = 0.f, dphi = 0.f;
    if (live_row && t < nv) {
      const float wf = wr ? wr[t] : 1.f;
      if (wf > 0.f && wf < INFINITY) {  // (else a removed point: nothing else of it is read)
        const double w = (double)wf;
        const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
        const double Ag = (double)gr[2 * (size_t)t], phg = (double)gr[2 * (size_t)t + 1];
        double theta = ph - phg;
        if (n_tau > 0) theta += (kWfTwoPi * (double)fr[t]) * tau;
        double sn, cs;
        sincos(theta, &sn, &cs);
        const double cd = cs * ur + sn * ui, sd = sn * ur - cs * ui;  // cos / sin of theta - psi
        dA = (float)(scale * (w * (Ag * cd * inv_n - m_hh * A)));
        dphi = (float)(scale * (-(w * A * Ag) * sd * inv_n));
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

}  // namespace npf

extern "C" int64_t npf_waveform_match_workspace_bytes(int32_t n_rows, int32_t n_tau) {
  using namespace npf;
  if (n_rows <= 0 || n_tau < 0 || n_tau > kWfMaxTau) return NPF_EINVAL;
  return (int64_t)n_rows * wf_row_doubles(n_tau) * (int64_t)sizeof(double);
}

extern "C" int npf_waveform_match_ex(const float* h, int32_t h_ld, const float* g, const float* wgt, int32_t wgt_rows, const float* freq,
                                     int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                                     double dtau, int32_t n_tau, float* hh, float* gg, float* overlap, float* match, float* mismatch,
                                     int32_t* tau_index, float* phase, float* corr, void* workspace, double* saved, void* stream) {
  using namespace npf;
  if (!h || !g || !workspace || h_ld < 2 || n_tasks <= 0 || n_rows <= 0 || n_rows > (1 << 24) || n_rows % n_tasks != 0 || pts <= 0)
    return NPF_EINVAL;
  if (n_tau < 0 || n_tau > kWfMaxTau || (n_tau > 0 && !freq)) return NPF_EINVAL;
  if (wgt && wgt_rows != 1 && wgt_rows != n_tasks) return NPF_EINVAL;
  if (freq && freq_rows != 1 && freq_rows != n_tasks) return NPF_EINVAL;
  if (!hh && !gg && !overlap && !match && !mismatch && !tau_index && !phase && !corr && !saved) return NPF_EINVAL;
  const int64_t row_doubles = wf_row_doubles(n_tau);
  double* ws = (double*)workspace;
  hipLaunchKernelGGL((waveform_corr_kernel<kWfJC, kWfThreads>), dim3(n_rows, wf_chunks(n_tau)), dim3(kWfThreads), 0, (hipStream_t)stream,
                     h, h_ld, g, wgt, (int)(wgt_rows != 1), freq, (int)(freq_rows != 1), n_valid, n_tasks, pts, tau0, dtau, n_tau, ws,
                     row_doubles);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(waveform_finish_kernel, dim3(n_rows), dim3(64), 0, (hipStream_t)stream, ws, row_doubles, n_tasks, n_tau, hh, gg,
                     overlap, match, mismatch, tau_index, phase, corr, saved);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

extern "C" int npf_waveform_match(const float* h, int32_t h_ld, const float* g, const float* wgt, int32_t wgt_rows, const float* freq,
                                  int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                                  double dtau, int32_t n_tau, float* hh, float* gg, float* overlap, float* match, float* mismatch,
                                  int32_t* tau_index, float* phase, float* corr, void* workspace, void* stream) {
  return npf_waveform_match_ex(h, h_ld, g, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, hh, gg, overlap,
                               match, mismatch, tau_index, phase, corr, workspace, nullptr, stream);
}

extern "C" int npf_waveform_match_bwd(const float* h, int32_t h_ld, const float* g, const float* wgt, int32_t wgt_rows, const float* freq,
                                      int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                                      double dtau, int32_t n_tau, const int32_t* tau_index, const double* saved, const float* d_match,
                                      int32_t n_bcast, float* d_h, int32_t dh_ld, void* stream) {
  using namespace npf;
  if (!h || !g || !saved || !d_match || !d_h || h_ld < 2 || dh_ld < 2 || n_bcast < 1 || n_tasks <= 0 || n_rows <= 0 ||
      n_rows > (1 << 24) || n_rows % n_tasks != 0 || pts <= 0)
    return NPF_EINVAL;
  if (n_tau < 0 || n_tau > kWfMaxTau || (n_tau > 0 && (!freq || !tau_index))) return NPF_EINVAL;
  if (wgt && wgt_rows != 1 && wgt_rows != n_tasks) return NPF_EINVAL;
  if (freq && freq_rows != 1 && freq_rows != n_tasks) return NPF_EINVAL;
  const int blocks_y = (int)((((int64_t)pts + kWfBwdThreads - 1) / kWfBwdThreads < kWfBwdMaxGridY)
                                 ? ((int64_t)pts + kWfBwdThreads - 1) / kWfBwdThreads
                                 : kWfBwdMaxGridY);
  const dim3 grid(n_rows, blocks_y), block(kWfBwdThreads);
  const bool whole = (uintptr_t)d_h % ((size_t)dh_ld * sizeof(float)) == 0;  // one store per point needs the point aligned
#define NPF_WF_BWD(LD)                                                                                                                   \
  hipLaunchKernelGGL(waveform_match_bwd_kernel<LD>, grid, block, 0, (hipStream_t)stream, h, h_ld, g, wgt, (int)(wgt_rows != 1), freq,    \
                     (int)(freq_rows != 1), n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, tau_index, saved, d_match, n_bcast, d_h,   \
                     dh_ld)
  if (dh_ld == 2 && whole) {
    NPF_WF_BWD(2);
  } else if (dh_ld == 4 && whole) {
    NPF_WF_BWD(4);
  } else {
    NPF_WF_BWD(0);
  }
#undef NPF_WF_BWD
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

// ---- matched-filter log likelihood of complex data under the predicted waveforms (npf_waveform_loglike) ------------------------------
// The data d_t = (Re, Im) are Cartesian, so no atan2 and no fp32 phase of the data enters: with c_t = w_t A_t conj(d_t),
//   kappa_j = sum_t c_t e^{i (phi_t + 2 pi f_t tau_j)},   hh = sum_t w_t A_t^2,   dd = sum_t w_t |d_t|^2,
// kappa_0/ the same sum without the time term.  Launch 1 (waveform_filter_kernel) has the geometry, the recurrence, the reduction
// order and the workspace layout of waveform_corr_kernel: per row [hh, dd, Re kappa_0/, Im kappa_0/, (Re, Im) kappa_j ...].
// Launch 2 (waveform_loglike_finish_kernel): one workgroup per task walks the task's latent samples in order; per row the maximum of
// x_j = |kappa_j| with the smallest index, then sum_j exp(L_j - L_max) with L_j = ln I0(x_j) - hh / 2 (lanes, then waves, in a fixed
// order), the row's outputs, and after the last row the two log-mean-exps over the latent samples (a running maximum: rows whose
// likelihoods lie further apart than the range of exp cost nothing).  No atomics; every output is a double.
namespace npf {

template <int JC, int THREADS>
__global__ __launch_bounds__(THREADS) void waveform_filter_kernel(const float* __restrict__ h, int h_ld, const float* __restrict__ d,
                                                                   const float* __restrict__ wgt, int wgt_per_task,
                                                                   const float* __restrict__ freq, int freq_per_task,
                                                                   const int32_t* __restrict__ n_valid, int n_tasks, int pts, double tau0,
                                                                   double dtau, int n_tau, double* __restrict__ ws, int64_t row_doubles) {
  __shared__ double red[2 * JC * (THREADS / 64)];
  const int r = blockIdx.x, chunk = blockIdx.y, b = r % n_tasks;
  const int nv = n_valid ? clamp_count(n_valid, b, pts) : pts;
  const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
  const float* dr = d + (size_t)b * (size_t)pts * 2;
  const float* wr = wgt ? wgt + (wgt_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;
  const float* fr = n_tau > 0 ? freq + (freq_per_task ? (size_t)b * (size_t)pts : 0) : nullptr;  // (n_tau == 0: freq is not read)
  const double tau_c = tau0 + (double)(chunk * JC) * dtau;  // the chunk's first shift
  const bool first = chunk == 0;

  double acc[2 * JC];  // (Re, Im) of kappa_j, j = chunk * JC + 0 .. JC - 1
#pragma unroll
  for (int i = 0; i < 2 * JC; ++i) acc[i] = 0.0;
  double base[4] = {0.0, 0.0, 0.0, 0.0};  // hh, dd, Re kappa_0/, Im kappa_0/ (chunk 0 only)

  for (int t = threadIdx.x; t < nv; t += THREADS) {
    const float wf = wr ? wr[t] : 1.f;
    if (!(wf > 0.f && wf < INFINITY)) continue;  // a removed point: nothing else of it is read
    const double w = (double)wf;
    const double A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
    const double dre = (double)dr[2 * (size_t)t], dim = (double)dr[2 * (size_t)t + 1];
    const double wa = w * A, cr = wa * dre, ci = -(wa * dim);  // c = w A conj(d)
    if (first) {
      double sn, cs;
      sincos(ph, &sn, &cs);
      base[0] += wa * A;
      base[1] += w * (dre * dre + dim * dim);
      base[2] += cs * cr - sn * ci;
      base[3] += cs * ci + sn * cr;
    }
    if (n_tau > 0) {
      const double om = kWfTwoPi * (double)fr[t];
      double sn, cs, ssn, scs;
      sincos(ph + om * tau_c, &sn, &cs);
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
  }

  double* row = ws + (size_t)r * (size_t)row_doubles;
  if (n_tau > 0) block_sum_store<2 * JC, THREADS>(acc, red, row + 4 + 2 * JC * chunk);
  if (first) block_sum_store<4, THREADS>(base, red, row);
}

// One workgroup per task: its n_z = n_rows / n_tasks rows in order, then the two log-mean-exps over them.
__global__ __launch_bounds__(kWfLlThreads) void waveform_loglike_finish_kernel(
    const double* __restrict__ ws, int64_t row_doubles, int n_rows, int n_tasks, int n_tau, double* __restrict__ hh,
    double* __restrict__ dd, double* __restrict__ snr, double* __restrict__ lnl_max, double* __restrict__ lnl_marg,
    int32_t* __restrict__ tau_index, double* __restrict__ phase, double* __restrict__ series, double* __restrict__ lnl_mix,
    double* __restrict__ lnl_max_mix) {
  constexpr int WAVES = kWfLlThreads / 64;
  __shared__ double red_v[WAVES];
  __shared__ int red_j[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = n_tau > 0 ? n_tau : 1, n_z = n_rows / n_tasks;
  const double log_n = log((double)n);
  // running log-sum-exp over the rows (thread 0): maximum so far and the sum of exp(value - maximum)
  double mix_m = 0.0, mix_s = 0.0, mxm_m = 0.0, mxm_s = 0.0;

  for (int s = 0; s < n_z; ++s) {
    const int r = s * n_tasks + b;
    const double* row = ws + (size_t)r * (size_t)row_doubles;
    const double vhh = row[0];
    const bool degenerate = vhh == 0.0;  // (no live point, or a zero template: Lambda = 1)
    const double half_hh = 0.5 * vhh, rt_hh = sqrt(vhh);
    const double* c = n_tau > 0 ? row + 4 : row + 2;  // (no grid: the one candidate is kappa_0/)

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
      if (tau_index) tau_index[r] = degenerate ? 0 : best_j;
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
  }
  if (tid == 0) {
    const double log_nz = log((double)n_z);
    if (lnl_mix) lnl_mix[b] = mix_m + (log(mix_s) - log_nz);
    if (lnl_max_mix) lnl_max_mix[b] = mxm_m + (log(mxm_s) - log_nz);
  }
}

bool wf_loglike_args_bad(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                         int n_rows, int n_tasks, int pts, int n_tau, const void* workspace) {
  if (!h || !d || !workspace || h_ld < 2 || n_tasks <= 0 || n_rows <= 0 || n_rows > (1 << 24) || n_rows % n_tasks != 0 || pts <= 0)
    return true;
  if (n_tau < 0 || n_tau > kWfMaxTau || (n_tau > 0 && !freq)) return true;
  if (wgt && wgt_rows != 1 && wgt_rows != n_tasks) return true;
  if (freq && freq_rows != 1 && freq_rows != n_tasks) return true;
  return false;
}

int wf_loglike_launch(const float* h, int h_ld, const float* d, const float* wgt, int wgt_rows, const float* freq, int freq_rows,
                      const int32_t* n_valid, int n_rows, int n_tasks, int pts, double tau0, double dtau, int n_tau, double* hh, double* dd,
                      double* snr, double* lnl_max, double* lnl_marg, int32_t* tau_index, double* phase, double* series, double* lnl_mix,
                      double* lnl_max_mix, double* ws, int64_t row_doubles, bool finish, hipStream_t stream) {
  hipLaunchKernelGGL((waveform_filter_kernel<kWfJC, kWfThreads>), dim3(n_rows, wf_chunks(n_tau)), dim3(kWfThreads), 0, stream, h, h_ld, d,
                     wgt, (int)(wgt_rows != 1), freq, (int)(freq_rows != 1), n_valid, n_tasks, pts, tau0, dtau, n_tau, ws, row_doubles);
  NPF_CHECK_LAUNCH();
  if (!finish) return NPF_OK;
  hipLaunchKernelGGL(waveform_loglike_finish_kernel, dim3(n_tasks), dim3(kWfLlThreads), 0, stream, ws, row_doubles, n_rows, n_tasks, n_tau,
                     hh, dd, snr, lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_workspace_bytes(int32_t n_rows, int32_t n_tau) {
  return npf_waveform_match_workspace_bytes(n_rows, n_tau);  // (the same layout)
}

extern "C" int npf_waveform_loglike(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows, const float* freq,
                                    int32_t freq_rows, const int32_t* n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                                    double dtau, int32_t n_tau, double* hh, double* dd, double* snr, double* lnl_max, double* lnl_marg,
                                    int32_t* tau_index, double* phase, double* series, double* lnl_mix, double* lnl_max_mix,
                                    void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_rows, n_tasks, pts, n_tau, workspace)) return NPF_EINVAL;
  if (!hh && !dd && !snr && !lnl_max && !lnl_marg && !tau_index && !phase && !series && !lnl_mix && !lnl_max_mix) return NPF_EINVAL;
  return wf_loglike_launch(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, hh, dd, snr,
                           lnl_max, lnl_marg, tau_index, phase, series, lnl_mix, lnl_max_mix, (double*)workspace, wf_row_doubles(n_tau),
                           true, (hipStream_t)stream);
}
