// Sky-grid network likelihood (npf_waveform_loglike_sky): the coherent likelihood of npf_waveform_loglike_net at every pixel of ONE
// sky grid shared by the tasks, marginalised over the pixels.  For row r, grid time j and pixel p
//   K_{j,p}[r] = sum_k sum_t [ w_{k,t} A_t e^{i phi_t} conj(d_{k,t}) e^{i 2 pi f_t tau_j} ] [ C_{p,k} e^{i 2 pi f_t Delta_{p,k}} ]:
// the first factor depends on (row, j) only, the second on the pixel only, so this is one complex GEMM with M = rows x n_tau, N = P
// and K = D x T on v_mfma_f64_16x16x4_f64.  The detectors fold into the contraction axis: the sum over k stays inside the modulus.
// DOUBLE throughout, from fp32 inputs widened exactly.
//
// Launch 1 (sky_prep_kernel): one workgroup per row, per pixel and per auxiliary row.  U holds a_{r,k,t} = w A e^{i phi} conj(d) (an
// exact zero, by a select, at a point that is not live for detector k), V holds C_{p,k} e^{i 2 pi f_t Delta_{p,k}} (one double sincos per
// (p, k, t); zeros for a dead pixel), both in the MFMA fragment order of the bank match, the K axis detector-major with every
// detector's points padded to tp = pts rounded up to 4 and rows / pixels padded to whole tiles of 16 with zeros.  The step
// e^{i 2 pi f dtau} and the start e^{i 2 pi f tau_c} of every chunk of JC shifts are stored once over t.  hh_k per (row, detector):
// thread i owns points i, i + THREADS, ..., then lanes and waves in a fixed order.
// Launch 2 (sky_corr_kernel): one wavefront per (16 rows, 16 pixels), four pixel tiles per workgroup.  Per chunk the 2 JC accumulator
// tiles live in registers; per k-step the lane rotates its own point, z = a start, then per shift four MFMAs -- Re K += Re z Re v +
// Im z (-Im v), Im K += Re z Im v + Im z Re v, the plain product -- and z <- z step.  After a chunk x = |K| and ln I0(x) are formed
// on the accumulators (a rolled loop over the shifts that rotates the accumulator tiles through slot 0, so ln I0 is instantiated
// four times, not 4 JC times) and the running (m, s) of the log-sum-exp over j and the running max x with its first j are updated
// in registers: nothing of size [R][P][n_tau] is written.  At the end u, max x, j and HH per (row, pixel) go to the workspace.
// C/D fragment of the f64 instruction: column = lane & 15, row = (lane >> 4) + 4 * reg.
// Launch 3 (sky_finish_kernel): one workgroup per task over its n_z rows in order: the log-sum-exp over the pixels, the indices,
// post, snr, snr_map, then the mixtures.  The sum over the pixels of exp(u_p - max) is taken in 2^-62 fixed point on two integer
// accumulators, so it does not depend on the order of the pixels (error <= P 2^-62 of the largest term).
// No atomics, a fixed K order (detector ascending, then point ascending): a second call on the same inputs gives the same bits.
//
// Workspace (after alignment to 16 bytes), doubles: [hh_k: rows_pad x D][step: tp x 2][start: chunks x tp x 2][U: rows_pad x D tp x 2]
// [V: pix_pad x D tp x 2][u: R x P][max x: R x P][HH: R x P][j: R x P int32].
#include "waveform_common.hpp"  // kWfMaxTau, kWfTwoPi, block_sum_store, wf_log_i0, wf_loglike_net_args_bad

namespace npf {

constexpr int kSkyJC = NPF_SKY_JC;  // time shifts per chunk of launch 2
constexpr int kSkyPrepThreads = 256;
constexpr int kSkyCorrWaves = 4;  // pixel tiles per workgroup of launch 2
constexpr int kSkyFinishThreads = 256;
constexpr int kSkyMaxPix = NPF_SKY_MAX_PIX;

typedef double sky_f64x4 __attribute__((ext_vector_type(4)));

inline int sky_chunks(int n_tau) { return n_tau > 0 ? (n_tau + kSkyJC - 1) / kSkyJC : 1; }

struct SkyLayout {
  int64_t rows_pad, pix_pad, tp, chunks;
  int64_t hhk, step, start, u, v, lu, xm, hh, jx, total;  // offsets in doubles
};

inline SkyLayout sky_layout(int n_rows, int n_det, int pts, int n_pix, int n_tau) {
  SkyLayout L;
  L.rows_pad = ((int64_t)n_rows + 15) / 16 * 16;
  L.pix_pad = ((int64_t)n_pix + 15) / 16 * 16;
  L.tp = ((int64_t)pts + 3) / 4 * 4;
  L.chunks = sky_chunks(n_tau);
  const int64_t kp = L.tp * n_det, rp = (int64_t)n_rows * n_pix;
  L.hhk = 0;
  L.step = L.hhk + L.rows_pad * n_det;
  L.start = L.step + 2 * L.tp;
  L.u = L.start + 2 * L.tp * L.chunks;
  L.v = L.u + 2 * kp * L.rows_pad;
  L.lu = L.v + 2 * kp * L.pix_pad;
  L.xm = L.lu + rp;
  L.hh = L.xm + rp;
  L.jx = L.hh + rp;
  L.total = L.jx + (rp + 1) / 2;
  return L;
}

// position of (row, point kk of the K axis) in a fragment-ordered panel of ks_max k-steps per tile, in (Re, Im) pairs
__device__ __forceinline__ size_t sky_frag_index(int row, size_t kk, size_t ks_max) {
  return ((size_t)(row >> 4) * ks_max + (kk >> 2)) * 64 + (size_t)(((kk & 3) << 4) | (size_t)(row & 15));
}

__device__ __forceinline__ bool sky_pixel_live(const double* __restrict__ log_prior, int p) {
  if (!log_prior) return true;
  const double lp = log_prior[p];
  return lp - lp == 0.0;  // finite
}

template <int JC, int THREADS>
__global__ __launch_bounds__(THREADS) void sky_prep_kernel(const float* __restrict__ h, int h_ld, const float* __restrict__ d,
                                                            const float* __restrict__ wgt, int wgt_per_task,
                                                            const float* __restrict__ freq, const int32_t* __restrict__ n_valid,
                                                            const double* __restrict__ resp, const double* __restrict__ delay,
                                                            const double* __restrict__ log_prior, int n_rows, int n_tasks, int n_det,
                                                            int pts, int n_pix, double tau0, double dtau, int n_tau, int rows_pad,
                                                            int pix_pad, int tp, double* __restrict__ hhk, double2* __restrict__ step,
                                                            double2* __restrict__ start, double2* __restrict__ U,
                                                            double2* __restrict__ V) {
  __shared__ double red[THREADS / 64];
  const int blk = blockIdx.x, tid = threadIdx.x;
  const size_t ks_max = (size_t)n_det * (size_t)(tp >> 2);

  if (blk < rows_pad) {  // a row of U and its hh_k
    const int r = blk;
    const bool pad_row = r >= n_rows;  // a row of zeros that fills the last tile
    const int b = pad_row ? 0 : r % n_tasks;
    const int nv = pad_row ? 0 : (n_valid ? clamp_count(n_valid, b, pts) : pts);
    const float* hr = h + (size_t)r * (size_t)pts * (size_t)h_ld;
    for (int k = 0; k < n_det; ++k) {
      const size_t bk = (size_t)b * (size_t)n_det + (size_t)k;
      const float* dr = d + bk * (size_t)pts * 2;
      const float* wr = wgt ? wgt + (wgt_per_task ? bk : (size_t)k) * (size_t)pts : nullptr;
      double sum[1] = {0.0};
      for (int t = tid; t < tp; t += THREADS) {
        double ar = 0.0, ai = 0.0;
        if (t < nv) {
          const float wf = wr ? wr[t] : 1.f;
          if (wf > 0.f && wf < INFINITY) {  // live for this detector; else nothing more of the point is read
            const double w = (double)wf, A = (double)hr[(size_t)t * h_ld], ph = (double)hr[(size_t)t * h_ld + 1];
            const double dre = (double)dr[2 * (size_t)t], dim = (double)dr[2 * (size_t)t + 1];
            const double wa = w * A, cr = wa * dre, ci = -(wa * dim);  // c = w A conj(d)
            double sn, cs;
            sincos(ph, &sn, &cs);
            ar = cs * cr - sn * ci;
            ai = cs * ci + sn * cr;
            sum[0] += wa * A;
          }
        }
        U[sky_frag_index(r, (size_t)k * (size_t)tp + (size_t)t, ks_max)] = make_double2(ar, ai);
      }
      block_sum_store<1, THREADS>(sum, red, hhk + (size_t)r * (size_t)n_det + (size_t)k);
    }
    return;
  }
  if (blk < rows_pad + pix_pad) {  // a pixel of V
    const int p = blk - rows_pad;
    const bool live = p < n_pix && sky_pixel_live(log_prior, p);  // (a dead or padding pixel: zeros; its resp / delay are not read)
    for (int k = 0; k < n_det; ++k) {
      const size_t pk = (size_t)p * (size_t)n_det + (size_t)k;
      double c_re = 0.0, c_im = 0.0, dl = 0.0;
      if (live) {
        c_re = resp[2 * pk], c_im = resp[2 * pk + 1];
        dl = delay ? delay[pk] : 0.0;
      }
      for (int t = tid; t < tp; t += THREADS) {
        double vr = 0.0, vi = 0.0;
        if (live && t < pts) {
          double sn, cs;
          sincos((kWfTwoPi * (double)freq[t]) * dl, &sn, &cs);
          vr = c_re * cs - c_im * sn;
          vi = c_re * sn + c_im * cs;
        }
        V[sky_frag_index(p, (size_t)k * (size_t)tp + (size_t)t, ks_max)] = make_double2(vr, vi);
      }
    }
    return;
  }
  // the step (chunk == -1) or the start of a chunk, over t; ones behind the points
  const int chunk = blk - rows_pad - pix_pad - 1;
  const double arg = chunk < 0 ? dtau : tau0 + (double)(chunk * JC) * dtau;
  double2* dst = chunk < 0 ? step : start + (size_t)chunk * (size_t)tp;
  for (int t = tid; t < tp; t += THREADS) {
    double sn = 0.0, cs = 1.0;
    if (t < pts && n_tau > 0) sincos((kWfTwoPi * (double)freq[t]) * arg, &sn, &cs);
    dst[t] = make_double2(cs, sn);
  }
}

// The k loop of one chunk: nj shifts (FULL: nj == JC, no guards) accumulated over the D * tq k-steps.
template <int JC, bool FULL>
__device__ __forceinline__ void sky_chunk(const double2* __restrict__ up, const double2* __restrict__ vp,
                                          const double2* __restrict__ step, const double2* __restrict__ start, int n_det, int tq, int kq,
                                          int nj, sky_f64x4 (&acc_re)[JC], sky_f64x4 (&acc_im)[JC]) {
  const int64_t ks_n = (int64_t)n_det * (int64_t)tq;
  double2 u = up[0], v = vp[0], s = step[kq], st = start[kq];
  int t4 = 0;  // the k-step within its detector
  for (int64_t ks = 0; ks < ks_n; ++ks) {
    const int64_t nx = ks + 1 < ks_n ? ks + 1 : ks;  // the next k-step's operands, in flight behind this one's matrix instructions
    const int t4n = ks + 1 < ks_n ? (t4 + 1 == tq ? 0 : t4 + 1) : t4;
    const double2 u_n = up[(size_t)nx * 64], v_n = vp[(size_t)nx * 64], s_n = step[t4n * 4 + kq], st_n = start[t4n * 4 + kq];
    double zr = u.x * st.x - u.y * st.y, zi = u.x * st.y + u.y * st.x;
    const double vr = v.x, vi = v.y, nvi = -v.y;
#pragma unroll
    for (int i = 0; i < JC; ++i) {
      if (FULL || i < nj) {
        acc_re[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr, vr, acc_re[i], 0, 0, 0);
        acc_im[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr, vi, acc_im[i], 0, 0, 0);
        acc_re[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi, nvi, acc_re[i], 0, 0, 0);
        acc_im[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi, vr, acc_im[i], 0, 0, 0);
        if (i + 1 < JC) {
          const double nr = zr * s.x - zi * s.y;
          zi = zr * s.y + zi * s.x;
          zr = nr;
        }
      }
    }
    u = u_n, v = v_n, s = s_n, st = st_n, t4 = t4n;
  }
}

template <int JC>
__global__ __launch_bounds__(64 * kSkyCorrWaves) void sky_corr_kernel(
    const double* __restrict__ hhk, const double2* __restrict__ step, const double2* __restrict__ start, const double2* __restrict__ U,
    const double2* __restrict__ V, const double* __restrict__ resp, const double* __restrict__ log_prior, int n_rows, int n_det,
    int n_pix, int tp, int n_tau, int chunks, double* __restrict__ u_out, double* __restrict__ xm_out, double* __restrict__ hh_out,
    int32_t* __restrict__ j_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x, pt = blockIdx.y * kSkyCorrWaves + wave;
  if (pt * 16 >= n_pix) return;  // (no barrier below: a wavefront without a tile leaves)
  const int tq = tp >> 2, kq = lane >> 4;
  const size_t ks_max = (size_t)n_det * (size_t)tq;
  const double2* up = U + (size_t)rt * ks_max * 64 + lane;
  const double2* vp = V + (size_t)pt * ks_max * 64 + lane;

  // per (row, pixel) of the lane's four C/D registers: the running log-sum-exp of ln I0(x_j) and the running maximum of x_j
  double lse_m[4], lse_s[4], best[4];
  int best_j[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) lse_m[q] = 0.0, lse_s[q] = 0.0, best[q] = 0.0, best_j[q] = 0;

  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int j0 = chunk * JC, nj = n_tau > 0 ? (n_tau - j0 < JC ? n_tau - j0 : JC) : 1;
    sky_f64x4 acc_re[JC], acc_im[JC];
#pragma unroll
    for (int i = 0; i < JC; ++i) acc_re[i] = sky_f64x4{0.0, 0.0, 0.0, 0.0}, acc_im[i] = sky_f64x4{0.0, 0.0, 0.0, 0.0};
    const double2* st = start + (size_t)chunk * (size_t)tp;
    if (nj == JC) {
      sky_chunk<JC, true>(up, vp, step, st, n_det, tq, kq, nj, acc_re, acc_im);
    } else {
      sky_chunk<JC, false>(up, vp, step, st, n_det, tq, kq, nj, acc_re, acc_im);
    }
    // shift i of the chunk sits in slot 0 when its turn comes: the tiles move down one slot per turn
#pragma unroll 1
    for (int i = 0; i < nj; ++i) {
      const int j = j0 + i;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double re = acc_re[0][q], im = acc_im[0][q], x = sqrt(re * re + im * im), li0 = wf_log_i0(x);
        if (j == 0) {  // (j = 0 always enters, so a NaN there stays)
          lse_m[q] = li0, lse_s[q] = 1.0, best[q] = x, best_j[q] = 0;
        } else {
          if (li0 > lse_m[q]) {
            lse_s[q] = lse_s[q] * exp(lse_m[q] - li0) + 1.0;
            lse_m[q] = li0;
          } else {
            lse_s[q] += exp(li0 - lse_m[q]);
          }
          if (x > best[q]) {  // (j ascends: the smallest index stays)
            best[q] = x;
            best_j[q] = j;
          }
        }
      }
#pragma unroll
      for (int k = 0; k + 1 < JC; ++k) acc_re[k] = acc_re[k + 1], acc_im[k] = acc_im[k + 1];
    }
  }

  const double log_n = log((double)(n_tau > 0 ? n_tau : 1));
  const int p = pt * 16 + (lane & 15);
  if (p >= n_pix) return;
  const bool live = sky_pixel_live(log_prior, p);
  const double lp = log_prior ? log_prior[p] : -log((double)n_pix);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rt * 16 + (lane >> 4) + 4 * q;  // the f64 C/D fragment: row = (lane >> 4) + 4 * reg
    if (r >= n_rows) continue;
    const size_t o = (size_t)r * (size_t)n_pix + (size_t)p;
    if (!live) {  // no mass; nothing of its resp is read
      u_out[o] = -INFINITY, xm_out[o] = 0.0, hh_out[o] = 0.0, j_out[o] = 0;
      continue;
    }
    double hh = 0.0;
    for (int k = 0; k < n_det; ++k) {  // HH_p = sum_k |C_{p,k}|^2 hh_k, k ascending
      const double c_re = resp[2 * ((size_t)p * n_det + k)], c_im = resp[2 * ((size_t)p * n_det + k) + 1];
      hh += (c_re * c_re + c_im * c_im) * hhk[(size_t)r * (size_t)n_det + (size_t)k];
    }
    u_out[o] = lp + (((lse_m[q] + log(lse_s[q])) - log_n) - 0.5 * hh);
    xm_out[o] = best[q];
    hh_out[o] = hh;
    j_out[o] = best_j[q];
  }
}

// value v enters the running log-sum-exp (m, s); s == 0: nothing has entered; -inf adds no mass
__device__ __forceinline__ void sky_lse_add(double& m, double& s, double v) {
  if (v == -INFINITY) return;
  if (s == 0.0) {
    m = v, s = 1.0;
  } else if (v > m) {
    s = s * exp(m - v) + 1.0;
    m = v;
  } else {
    s += exp(v - m);
  }
}

// One workgroup per task: its n_z = n_rows / n_tasks rows in order, then the mixtures over them.
__global__ __launch_bounds__(kSkyFinishThreads) void sky_finish_kernel(
    const double* __restrict__ u_ws, const double* __restrict__ xm_ws, const double* __restrict__ hh_ws, const int32_t* __restrict__ j_ws,
    int n_rows, int n_tasks, int n_pix, double* __restrict__ lnl_sky, int32_t* __restrict__ pix_index, int32_t* __restrict__ tau_index,
    double* __restrict__ snr, double* __restrict__ lnl_sky_mix, double* __restrict__ post, double* __restrict__ snr_map,
    double* __restrict__ post_mix) {
  constexpr int WAVES = kSkyFinishThreads / 64;
  __shared__ double red_v[WAVES];
  __shared__ int red_p[WAVES];
  __shared__ long long red_hi[WAVES], red_lo[WAVES];
  __shared__ int red_nan[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_z = n_rows / n_tasks;
  double mix_m = 0.0, mix_s = 0.0;  // (every thread carries the same running log-sum-exp over the rows)

  for (int s = 0; s < n_z; ++s) {
    const int r = s * n_tasks + b;
    const double* u = u_ws + (size_t)r * (size_t)n_pix;
    // max_p u_p with the smallest p (n_pix: no pixel with u > -inf)
    double best = -INFINITY;
    int best_p = n_pix;
    for (int p = tid; p < n_pix; p += kSkyFinishThreads) {
      const double v = u[p];
      if (v > best) {  // (p ascends: the smallest index of the thread stays; a NaN never enters)
        best = v;
        best_p = p;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ob = __shfl_xor(best, off);
      const int op = __shfl_xor(best_p, off);
      if (ob > best || (ob == best && op < best_p)) {
        best = ob;
        best_p = op;
      }
    }
    __syncthreads();  // (red_* may still be read for the previous row)
    if (lane == 0) {
      red_v[wave] = best;
      red_p[wave] = best_p;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const double ob = red_v[w];
      const int op = red_p[w];
      if (w == 0 || ob > best || (ob == best && op < best_p)) {
        best = ob;
        best_p = op;
      }
    }
    // sum_p exp(u_p - best) in 2^-62 fixed point: integer sums do not depend on the order of the pixels
    long long hi = 0, lo = 0;
    int any_nan = 0;
    for (int p = tid; p < n_pix; p += kSkyFinishThreads) {
      const double v = u[p];
      if (v == -INFINITY) continue;
      const double e = exp(v - best);  // in [0, 1]; NaN where u_p is NaN (or nothing but NaN is above -inf)
      if (!(e >= 0.0)) {
        any_nan = 1;
        continue;
      }
      const double scaled = e * 0x1p30, fl = floor(scaled);
      hi += (long long)fl;
      lo += (long long)floor((scaled - fl) * 0x1p32);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      hi += __shfl_xor(hi, off);
      lo += __shfl_xor(lo, off);
      any_nan |= __shfl_xor(any_nan, off);
    }
    __syncthreads();  // (the maximum has been read by every thread)
    if (lane == 0) red_hi[wave] = hi, red_lo[wave] = lo, red_nan[wave] = any_nan;
    __syncthreads();
    hi = 0, lo = 0, any_nan = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) hi += red_hi[w], lo += red_lo[w], any_nan |= red_nan[w];
    const double total = (double)hi * 0x1p-30 + (double)lo * 0x1p-62;
    const double v_sky = any_nan ? NAN : (best_p < n_pix ? best + log(total) : -INFINITY);  // (every thread: the same bits)
    const int p_star = best_p < n_pix ? best_p : 0;

    if (tid == 0) {
      const size_t o = (size_t)r * (size_t)n_pix + (size_t)p_star;
      const double hh = hh_ws[o];  // (a dead pixel holds 0 here)
      if (lnl_sky) lnl_sky[r] = v_sky;
      if (pix_index) pix_index[r] = p_star;
      if (tau_index) tau_index[r] = j_ws[o];
      if (snr) snr[r] = hh == 0.0 ? 0.0 : xm_ws[o] / sqrt(hh);
    }
    if (post || snr_map) {
      for (int p = tid; p < n_pix; p += kSkyFinishThreads) {
        const size_t o = (size_t)r * (size_t)n_pix + (size_t)p;
        if (post) post[o] = u[p] == -INFINITY ? -INFINITY : u[p] - v_sky;
        if (snr_map) {
          const double hh = hh_ws[o];
          snr_map[o] = hh == 0.0 ? 0.0 : xm_ws[o] / sqrt(hh);
        }
      }
    }
    sky_lse_add(mix_m, mix_s, v_sky);
  }

  const double log_nz = log((double)n_z);
  const double v_mix = mix_s == 0.0 ? -INFINITY : mix_m + (log(mix_s) - log_nz);
  if (tid == 0 && lnl_sky_mix) lnl_sky_mix[b] = v_mix;
  if (post_mix) {
    for (int p = tid; p < n_pix; p += kSkyFinishThreads) {
      double m = 0.0, sm = 0.0;
      for (int s = 0; s < n_z; ++s) sky_lse_add(m, sm, u_ws[(size_t)(s * n_tasks + b) * (size_t)n_pix + (size_t)p]);
      post_mix[(size_t)b * (size_t)n_pix + (size_t)p] = sm == 0.0 ? -INFINITY : (m + (log(sm) - log_nz)) - v_mix;
    }
  }
}

inline bool sky_sizes_bad(int n_rows, int n_det, int pts, int n_pix, int n_tau) {
  return n_rows <= 0 || n_rows > (1 << 24) || n_det < 1 || n_det > NPF_NET_MAX_DET || pts <= 0 || n_pix < 1 || n_pix > kSkyMaxPix ||
         n_tau < 0 || n_tau > kWfMaxTau;
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_sky_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t pts, int32_t n_pix, int32_t n_tau) {
  using namespace npf;
  if (sky_sizes_bad(n_rows, n_det, pts, n_pix, n_tau)) return NPF_EINVAL;
  // the largest term, the U panel, is 2^24 rows x 8 detectors x 2^31 points x 16 bytes = 2^62: the sum stays in int64
  return sky_layout(n_rows, n_det, pts, n_pix, n_tau).total * (int64_t)sizeof(double) + 16;  // (+ 16: the panels are aligned to 16 bytes)
}

extern "C" int npf_waveform_loglike_sky(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                        const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* resp,
                                        const double* delay, const double* log_prior, int32_t n_rows, int32_t n_tasks, int32_t n_det,
                                        int32_t pts, int32_t n_pix, double tau0, double dtau, int32_t n_tau, double* lnl_sky,
                                        int32_t* pix_index, int32_t* tau_index, double* snr, double* lnl_sky_mix, double* post,
                                        double* snr_map, double* post_mix, void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_net_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, delay, resp, n_rows, n_tasks, n_det, pts, n_tau, workspace))
    return NPF_EINVAL;
  if (!freq || freq_rows != 1 || sky_sizes_bad(n_rows, n_det, pts, n_pix, n_tau)) return NPF_EINVAL;
  if (!lnl_sky && !pix_index && !tau_index && !snr && !lnl_sky_mix && !post && !snr_map && !post_mix) return NPF_EINVAL;
  if (n_tau == 0) tau0 = dtau = 0.0;  // the one candidate is tau = 0
  const SkyLayout L = sky_layout(n_rows, n_det, pts, n_pix, n_tau);
  double* ws = reinterpret_cast<double*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  double2 *step = (double2*)(ws + L.step), *start = (double2*)(ws + L.start), *U = (double2*)(ws + L.u), *V = (double2*)(ws + L.v);
  int32_t* jx = reinterpret_cast<int32_t*>(ws + L.jx);
  hipStream_t st = (hipStream_t)stream;

  const int64_t prep_blocks = L.rows_pad + L.pix_pad + 1 + L.chunks;
  hipLaunchKernelGGL((sky_prep_kernel<kSkyJC, kSkyPrepThreads>), dim3((unsigned)prep_blocks), dim3(kSkyPrepThreads), 0, st, h, h_ld, d, wgt,
                     (int)(wgt_rows != 1), freq, n_valid, resp, delay, log_prior, n_rows, n_tasks, n_det, pts, n_pix, tau0, dtau, n_tau,
                     (int)L.rows_pad, (int)L.pix_pad, (int)L.tp, ws + L.hhk, step, start, U, V);
  NPF_CHECK_LAUNCH();
  const int64_t pts_tiles = L.pix_pad / 16;
  hipLaunchKernelGGL(sky_corr_kernel<kSkyJC>, dim3((unsigned)(L.rows_pad / 16), (unsigned)((pts_tiles + kSkyCorrWaves - 1) / kSkyCorrWaves)),
                     dim3(64 * kSkyCorrWaves), 0, st, ws + L.hhk, step, start, U, V, resp, log_prior, n_rows, n_det, n_pix, (int)L.tp,
                     n_tau, (int)L.chunks, ws + L.lu, ws + L.xm, ws + L.hh, jx);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(sky_finish_kernel, dim3(n_tasks), dim3(kSkyFinishThreads), 0, st, ws + L.lu, ws + L.xm, ws + L.hh, jx, n_rows, n_tasks,
                     n_pix, lnl_sky, pix_index, tau_index, snr, lnl_sky_mix, post, snr_map, post_mix);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}

// ---- sky and distance marginalised jointly ----------------------------------------------------------------------------------------
// Sky and distance marginalised jointly (npf_waveform_loglike_sky_dist): the coherent likelihood of npf_waveform_loglike_sky at every
// pixel p of the shared sky grid AND every amplitude scale a_i of a shared scale grid.  With x_{p,j} = |K_{j,p}|,
// HH_p, n = max(n_tau, 1) and the pixel prior lp_p of the sky call, a_i and ln pi_i of the distance call:
//   w_{p,i} = lp_p + ln pi_i + (logsumexp_j ln I0(a_i x_{p,j}) - ln n) - a_i^2 HH_p / 2        (-inf for a dead pixel or a dead scale)
// and everything else is sums of exp(w) over p, over i or over both.  DOUBLE throughout.
//
// Launch 1: sky_prep_kernel of the sky call, as it is.
// Launch 2 (skyd_corr_kernel): the f64 MFMA correlation of sky_corr_kernel, the same sky_chunk k loop and the same wavefront per (16
// rows, 16 pixels).  Its epilogue takes no logarithm: x = |K| of every accumulator goes to the x panel, and the running max of x_j with
// its first j stays in registers; at the end max x, j and HH_p go to the workspace with sky_corr_kernel's own arithmetic.
//   x panel: X[r][j][pix_pad], the pixel fastest.  The C/D fragment has 16 pixels across lane & 15, so the 16 lanes of one fragment
//   row store 16 consecutive doubles: one whole 128-byte line (pix_pad is a multiple of 16 and the panel starts on a 128-byte
//   boundary).  Launch 3 reads 64 consecutive pixels of one (r, j) per wavefront: four whole lines.
// Launch 3 (skyd_scale_kernel): one wavefront per (row, 64 pixels, chunk of SC scales), the lane owns a pixel.  x* = max_j x_j is known
// from launch 2, so the x*-shifted sum of 3.18 needs one pass: per j one load of x and per live scale of the chunk one
// exp(ln I0(a_i x) - ln I0(a_i x*)) <= 1.  ln I0(a_i x*) and the running sums of the SC scales sit in LDS ([scale][lane]: the lane
// touches its own column only, so there is no barrier in the loop), the scale loop stays rolled and wf_log_i0 is instantiated twice.
// It writes w_{p,i} to the w panel W[r][i][pix_pad], the pixel fastest again.
// Launch 4 (skyd_finish_kernel): one workgroup per task over its n_z rows in order.  Per pixel (a thread, i ascending): mm_p = max_i
// w, s_p = sum_i exp(w - mm_p), the moments; per scale (a wavefront, lanes over the pixels): m_i = max_p w, S_i = sum_p exp(w - m_i) in
// the 2^-62 fixed point of sky_finish_kernel; over the pixels, in the same fixed point, total = sum_p exp(mm_p - M) s_p with M = max
// w.  Every posterior is a difference first: post_sky = (mm_p - M) + (ln s_p - ln total), post_dist = (m_i - M) + (ln S_i - ln total),
// post_joint = (w - M) - ln total, so the three sum to one to rounding where w ~ 1e6.  Integer sums over the pixels: their order does
// not matter.  No atomics: a second call on the same inputs gives the same bits.
//
// Workspace (after alignment to 128 bytes), doubles: the sky call's layout (its u panel holds mm_p here), then [s_p: R x P][m_i: R x
// n_a][S_i: R x n_a][X: R x n x pix_pad][W: R x n_a x pix_pad], the two panels on 128-byte boundaries.
namespace npf {

constexpr int kSkydSC = NPF_SKYD_SC;  // scales per wavefront of launch 3
constexpr int kSkydFinishThreads = 256;
constexpr int kSkydMaxScales = NPF_DIST_MAX_SCALES;

struct SkydLayout {
  SkyLayout sky;
  int64_t ss, dm, ds, x, w, total;  // offsets in doubles; total < 0: the count does not fit int64
};

inline SkydLayout skyd_layout(int n_rows, int n_det, int pts, int n_pix, int n_tau, int n_a) {
  SkydLayout L;
  L.sky = sky_layout(n_rows, n_det, pts, n_pix, n_tau);
  const int64_t n = n_tau > 0 ? n_tau : 1, rp = (int64_t)n_rows * n_pix, ra = (int64_t)n_rows * n_a;
  L.ss = L.sky.total;
  L.dm = L.ss + rp;
  L.ds = L.dm + ra;
  L.x = (L.ds + ra + 15) / 16 * 16;
  // the panels: up to 2^24 rows x 2^16 grid times x 2^16 pixels
  const unsigned __int128 rows_pp = (unsigned __int128)n_rows * (unsigned __int128)L.sky.pix_pad;
  const unsigned __int128 xs = rows_pp * (unsigned __int128)n, wsz = rows_pp * (unsigned __int128)n_a;
  const unsigned __int128 total = (unsigned __int128)L.x + xs + wsz;
  if (total > (unsigned __int128)(INT64_MAX / 16)) {
    L.w = L.total = -1;
    return L;
  }
  L.w = L.x + (int64_t)xs;
  L.total = (int64_t)total;
  return L;
}

__device__ __forceinline__ bool skyd_scale_live(double a, double lp) {
  return a > 0.0 && a < INFINITY && lp > -INFINITY && lp < INFINITY;  // (a NaN fails every test)
}

template <int JC>
__global__ __launch_bounds__(64 * kSkyCorrWaves) void skyd_corr_kernel(
    const double* __restrict__ hhk, const double2* __restrict__ step, const double2* __restrict__ start, const double2* __restrict__ U,
    const double2* __restrict__ V, const double* __restrict__ resp, const double* __restrict__ log_prior, int n_rows, int n_det,
    int n_pix, int pix_pad, int tp, int n_tau, int chunks, double* __restrict__ x_out, double* __restrict__ xm_out,
    double* __restrict__ hh_out, int32_t* __restrict__ j_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x, pt = blockIdx.y * kSkyCorrWaves + wave;
  if (pt * 16 >= n_pix) return;  // (no barrier below: a wavefront without a tile leaves)
  const int tq = tp >> 2, kq = lane >> 4;
  const size_t ks_max = (size_t)n_det * (size_t)tq;
  const double2* up = U + (size_t)rt * ks_max * 64 + lane;
  const double2* vp = V + (size_t)pt * ks_max * 64 + lane;
  const int n = n_tau > 0 ? n_tau : 1;
  const int p = pt * 16 + (lane & 15);  // (< pix_pad: the tile lies inside the padded panel)

  // per (row, pixel) of the lane's four C/D registers: the running maximum of x_j and its first j
  double best[4];
  int best_j[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) best[q] = 0.0, best_j[q] = 0;

  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int j0 = chunk * JC, nj = n_tau > 0 ? (n_tau - j0 < JC ? n_tau - j0 : JC) : 1;
    sky_f64x4 acc_re[JC], acc_im[JC];
#pragma unroll
    for (int i = 0; i < JC; ++i) acc_re[i] = sky_f64x4{0.0, 0.0, 0.0, 0.0}, acc_im[i] = sky_f64x4{0.0, 0.0, 0.0, 0.0};
    const double2* st = start + (size_t)chunk * (size_t)tp;
    if (nj == JC) {
      sky_chunk<JC, true>(up, vp, step, st, n_det, tq, kq, nj, acc_re, acc_im);
    } else {
      sky_chunk<JC, false>(up, vp, step, st, n_det, tq, kq, nj, acc_re, acc_im);
    }
#pragma unroll
    for (int i = 0; i < JC; ++i) {
      if (i < nj) {
        const int j = j0 + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = rt * 16 + (lane >> 4) + 4 * q;  // the f64 C/D fragment: row = (lane >> 4) + 4 * reg
          const double re = acc_re[i][q], im = acc_im[i][q], x = sqrt(re * re + im * im);
          if (j == 0) {  // (j = 0 always enters, so a NaN there stays)
            best[q] = x, best_j[q] = 0;
          } else if (x > best[q]) {  // (j ascends: the smallest index stays)
            best[q] = x;
            best_j[q] = j;
          }
          if (r < n_rows) x_out[((size_t)r * (size_t)n + (size_t)j) * (size_t)pix_pad + (size_t)p] = x;  // 16 lanes: one 128-byte line
        }
      }
    }
  }

  if (p >= n_pix) return;
  const bool live = sky_pixel_live(log_prior, p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rt * 16 + (lane >> 4) + 4 * q;
    if (r >= n_rows) continue;
    const size_t o = (size_t)r * (size_t)n_pix + (size_t)p;
    if (!live) {  // no mass; nothing of its resp is read
      xm_out[o] = 0.0, hh_out[o] = 0.0, j_out[o] = 0;
      continue;
    }
    double hh = 0.0;
    for (int k = 0; k < n_det; ++k) {  // HH_p = sum_k |C_{p,k}|^2 hh_k, k ascending
      const double c_re = resp[2 * ((size_t)p * n_det + k)], c_im = resp[2 * ((size_t)p * n_det + k) + 1];
      hh += (c_re * c_re + c_im * c_im) * hhk[(size_t)r * (size_t)n_det + (size_t)k];
    }
    xm_out[o] = best[q];
    hh_out[o] = hh;
    j_out[o] = best_j[q];
  }
}

template <int SC>
__global__ __launch_bounds__(64) void skyd_scale_kernel(const double* __restrict__ x_ws, const double* __restrict__ xm_ws,
                                                         const double* __restrict__ hh_ws, const double* __restrict__ log_prior,
                                                         const double* __restrict__ scales, const double* __restrict__ log_prior_scale,
                                                         int n_pix, int pix_pad, int n_tau, int n_a, double* __restrict__ w_ws) {
  __shared__ double sc_a[SC], sc_lp[SC];             // a_i (0: dead or beyond n_a), ln pi_i
  __shared__ double l0_s[SC][64], sum_s[SC][64];     // ln I0(a_i x*), the shifted sum over j: [scale][lane]
  const int lane = threadIdx.x, r = blockIdx.x, p = blockIdx.y * 64 + lane, i0 = blockIdx.z * SC;
  const int n = n_tau > 0 ? n_tau : 1;
  if (lane < SC) {
    const int i = i0 + lane;
    double a = 0.0, lp = 0.0;
    if (i < n_a) a = scales[i], lp = log_prior_scale[i];
    const bool ok = i < n_a && skyd_scale_live(a, lp);
    sc_a[lane] = ok ? a : 0.0;
    sc_lp[lane] = ok ? lp : 0.0;
  }
  __syncthreads();
  const bool in = p < n_pix;
  const bool live = in && sky_pixel_live(log_prior, p);
  const size_t o = (size_t)r * (size_t)n_pix + (size_t)(in ? p : 0);
  const double hh = live ? hh_ws[o] : 0.0;
  const bool degenerate = hh == 0.0;  // Lambda = 1 at every scale: x_j = 0 (a dead or padding lane as well; its w is -inf below)
  const double xb = degenerate ? 0.0 : xm_ws[o];
#pragma unroll 1
  for (int k = 0; k < SC; ++k) {
    const double a = sc_a[k];
    if (a == 0.0) continue;  // (the same for every lane)
    l0_s[k][lane] = wf_log_i0(a * xb);
    sum_s[k][lane] = 0.0;
  }
  const double* xc = x_ws + (size_t)r * (size_t)n * (size_t)pix_pad + (size_t)(in ? p : 0);
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    const double x = degenerate ? 0.0 : xc[(size_t)j * (size_t)pix_pad];
#pragma unroll 1
    for (int k = 0; k < SC; ++k) {
      const double a = sc_a[k];
      if (a == 0.0) continue;
      sum_s[k][lane] += exp(wf_log_i0(a * x) - l0_s[k][lane]);
    }
  }
  if (!in) return;
  const double lp = log_prior ? log_prior[p] : -log((double)n_pix);
  const double log_n = log((double)n);
#pragma unroll 1
  for (int k = 0; k < SC; ++k) {
    const int i = i0 + k;
    if (i >= n_a) break;
    const double a = sc_a[k];
    double w = -INFINITY;
    if (live && a != 0.0) w = lp + ((sc_lp[k] + (l0_s[k][lane] - (a * a) * (0.5 * hh))) + (log(sum_s[k][lane]) - log_n));
    w_ws[((size_t)r * (size_t)n_a + (size_t)i) * (size_t)pix_pad + (size_t)p] = w;
  }
}

// max with the smallest index over the workgroup (a NaN never enters); every thread gets the same bits
template <int THREADS>
__device__ __forceinline__ void skyd_block_argmax(double& best, int& idx, double* red_v, int* red_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(idx, off);
    if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
  }
  __syncthreads();  // (red_* may still be read for the previous reduction)
  if (lane == 0) red_v[wave] = best, red_i[wave] = idx;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const double ob = red_v[w];
    const int oi = red_i[w];
    if (w == 0 || ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
  }
}

// e in [0, 2^31) enters the 2^-62 fixed-point sum (hi: units of 2^-30, lo: units of 2^-62)
__device__ __forceinline__ void skyd_fixed_add(long long& hi, long long& lo, double e) {
  const double scaled = e * 0x1p30, fl = floor(scaled);
  hi += (long long)fl;
  lo += (long long)floor((scaled - fl) * 0x1p32);
}

// One workgroup per task: its n_z = n_rows / n_tasks rows in order, then the mixtures over them.
__global__ __launch_bounds__(kSkydFinishThreads) void skyd_finish_kernel(
    const double* __restrict__ w_ws, const double* __restrict__ xm_ws, const double* __restrict__ hh_ws, const int32_t* __restrict__ j_ws,
    const double* __restrict__ scales, double* mm_ws, double* ss_ws, double* dm_ws, double* ds_ws, int n_rows, int n_tasks, int n_pix,
    int pix_pad, int n_a, double* __restrict__ lnl_vol, int32_t* __restrict__ pix_index, int32_t* __restrict__ scale_index,
    int32_t* __restrict__ tau_index, double* __restrict__ snr, double* __restrict__ scale_hat, double* __restrict__ lnl,
    double* __restrict__ post_sky, double* __restrict__ post_dist, double* __restrict__ post_joint, double* __restrict__ dist_mean,
    double* __restrict__ dist_std, double* __restrict__ post_sky_mix, double* __restrict__ post_dist_mix) {
  constexpr int THREADS = kSkydFinishThreads, WAVES = THREADS / 64;
  __shared__ double red_v[WAVES];
  __shared__ int red_i[WAVES];
  __shared__ long long red_hi[WAVES], red_lo[WAVES];
  __shared__ int red_nan[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_z = n_rows / n_tasks;
  const size_t pp = (size_t)pix_pad;
  double mix_m = 0.0, mix_s = 0.0;  // (every thread carries the same running log-sum-exp over the rows)

  for (int s = 0; s < n_z; ++s) {
    const int r = s * n_tasks + b;
    const double* W = w_ws + (size_t)r * (size_t)n_a * pp;
    double* mm = mm_ws + (size_t)r * (size_t)n_pix;
    double* ss = ss_ws + (size_t)r * (size_t)n_pix;
    double* dm = dm_ws + (size_t)r * (size_t)n_a;
    double* ds = ds_ws + (size_t)r * (size_t)n_a;

    // per pixel, i ascending: mm_p, s_p, u_sky = mm_p + ln s_p and the moments of 1 / a about the pixel's own weights
    double best_u = -INFINITY, w_max = -INFINITY;
    int best_p = n_pix, dummy = 0;
    for (int p = tid; p < n_pix; p += THREADS) {
      double m = -INFINITY;
      for (int i = 0; i < n_a; ++i) {
        const double v = W[(size_t)i * pp + p];
        if (v > m) m = v;  // (a NaN never enters)
      }
      double sum = 0.0, acc = 0.0;
      for (int i = 0; i < n_a; ++i) {
        const double v = W[(size_t)i * pp + p];
        if (v == -INFINITY) continue;  // a dead scale or a dead pixel: no mass, and its a_i is not used
        const double e = exp(v - m);
        sum += e;
        acc += (1.0 / scales[i]) * e;
      }
      mm[p] = m;
      ss[p] = sum;
      const double u = sum == 0.0 ? -INFINITY : m + log(sum);
      if (u > best_u) best_u = u, best_p = p;  // (p ascends: the smallest index of the thread stays)
      if (m > w_max) w_max = m;
      if (dist_mean || dist_std) {
        const size_t o = (size_t)r * (size_t)n_pix + (size_t)p;
        const double mean = sum == 0.0 ? 0.0 : acc / sum;
        if (dist_mean) dist_mean[o] = mean;
        if (dist_std) {
          double var = 0.0;  // the second pass about the mean
          for (int i = 0; i < n_a; ++i) {
            const double v = W[(size_t)i * pp + p];
            if (v == -INFINITY) continue;
            const double dv = 1.0 / scales[i] - mean;
            var += (dv * dv) * exp(v - m);
          }
          dist_std[o] = sum == 0.0 ? 0.0 : sqrt(var / sum);
        }
      }
    }
    skyd_block_argmax<THREADS>(best_u, best_p, red_v, red_i);
    skyd_block_argmax<THREADS>(w_max, dummy, red_v, red_i);

    // total = sum_p exp(mm_p - M) s_p in 2^-62 fixed point: integer sums do not depend on the order of the pixels
    long long hi = 0, lo = 0;
    int any_nan = 0;
    for (int p = tid; p < n_pix; p += THREADS) {
      const double sum = ss[p];
      if (sum == 0.0) continue;                   // no mass
      const double e = exp(mm[p] - w_max) * sum;  // in [0, n_a]; NaN where w is NaN at the pixel
      if (!(e >= 0.0)) {
        any_nan = 1;
        continue;
      }
      skyd_fixed_add(hi, lo, e);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      hi += __shfl_xor(hi, off);
      lo += __shfl_xor(lo, off);
      any_nan |= __shfl_xor(any_nan, off);
    }
    __syncthreads();
    if (lane == 0) red_hi[wave] = hi, red_lo[wave] = lo, red_nan[wave] = any_nan;
    __syncthreads();
    hi = 0, lo = 0, any_nan = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) hi += red_hi[w], lo += red_lo[w], any_nan |= red_nan[w];
    const bool none = best_p == n_pix;  // no pixel with mass (every thread: the same bits)
    const double log_total = any_nan ? NAN : log((double)hi * 0x1p-30 + (double)lo * 0x1p-62);
    const double v_vol = any_nan ? NAN : (none ? -INFINITY : w_max + log_total);
    const int p_star = none ? 0 : best_p;

    // per scale, a wavefront each, the lanes over the pixels: m_i and S_i in the same fixed point
    for (int i = wave; i < n_a; i += WAVES) {
      const double* Wi = W + (size_t)i * pp;
      double m = -INFINITY;
      for (int p = lane; p < n_pix; p += 64) {
        const double v = Wi[p];
        if (v > m) m = v;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double om = __shfl_xor(m, off);
        if (om > m) m = om;
      }
      long long h2 = 0, l2 = 0;
      int nan2 = 0;
      for (int p = lane; p < n_pix; p += 64) {
        const double v = Wi[p];
        if (v == -INFINITY) continue;
        const double e = exp(v - m);  // in [0, 1]
        if (!(e >= 0.0)) {
          nan2 = 1;
          continue;
        }
        skyd_fixed_add(h2, l2, e);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        h2 += __shfl_xor(h2, off);
        l2 += __shfl_xor(l2, off);
        nan2 |= __shfl_xor(nan2, off);
      }
      if (lane == 0) {
        dm[i] = m;
        ds[i] = nan2 ? NAN : (double)h2 * 0x1p-30 + (double)l2 * 0x1p-62;
      }
    }
    __syncthreads();  // (dm, ds of every scale are written)

    double best_d = -INFINITY;
    int best_i = n_a;
    for (int i = tid; i < n_a; i += THREADS) {
      const double sum = ds[i], u = sum == 0.0 ? -INFINITY : dm[i] + log(sum);
      if (u > best_d) best_d = u, best_i = i;
    }
    skyd_block_argmax<THREADS>(best_d, best_i, red_v, red_i);

    if (tid == 0) {
      const size_t o = (size_t)r * (size_t)n_pix + (size_t)p_star;
      const double hh = none ? 0.0 : hh_ws[o];  // (a dead pixel holds 0 here)
      if (lnl_vol) lnl_vol[r] = v_vol;
      if (pix_index) pix_index[r] = p_star;
      if (scale_index) scale_index[r] = best_i == n_a ? 0 : best_i;
      if (tau_index) tau_index[r] = none ? 0 : j_ws[o];
      if (snr) snr[r] = hh == 0.0 ? 0.0 : xm_ws[o] / sqrt(hh);
      if (scale_hat) scale_hat[r] = hh == 0.0 ? 0.0 : xm_ws[o] / hh;
    }
    if (post_sky) {
      for (int p = tid; p < n_pix; p += THREADS) {
        const double sum = ss[p];
        post_sky[(size_t)r * (size_t)n_pix + (size_t)p] = sum == 0.0 ? -INFINITY : (mm[p] - w_max) + (log(sum) - log_total);
      }
    }
    if (post_dist) {
      for (int i = tid; i < n_a; i += THREADS) {
        const double sum = ds[i];
        post_dist[(size_t)r * (size_t)n_a + (size_t)i] = sum == 0.0 ? -INFINITY : (dm[i] - w_max) + (log(sum) - log_total);
      }
    }
    if (post_joint) {
      double* dst = post_joint + (size_t)r * (size_t)n_pix * (size_t)n_a;
      const size_t cells = (size_t)n_pix * (size_t)n_a;
      for (size_t c = tid; c < cells; c += THREADS) {  // [p][i], the scale fastest
        const size_t p = c / (size_t)n_a, i = c - p * (size_t)n_a;
        const double v = W[i * pp + p];
        dst[c] = v == -INFINITY ? -INFINITY : (v - w_max) - log_total;
      }
    }
    sky_lse_add(mix_m, mix_s, v_vol);
  }

  const double log_nz = log((double)n_z);
  const double v_mix = mix_s == 0.0 ? -INFINITY : mix_m + (log(mix_s) - log_nz);
  if (tid == 0 && lnl) lnl[b] = v_mix;
  if (post_sky_mix) {
    for (int p = tid; p < n_pix; p += THREADS) {
      double m = 0.0, sm = 0.0;
      for (int s = 0; s < n_z; ++s) {
        const size_t o = (size_t)(s * n_tasks + b) * (size_t)n_pix + (size_t)p;
        const double sum = ss_ws[o];
        sky_lse_add(m, sm, sum == 0.0 ? -INFINITY : mm_ws[o] + log(sum));
      }
      post_sky_mix[(size_t)b * (size_t)n_pix + (size_t)p] = sm == 0.0 ? -INFINITY : (m + (log(sm) - log_nz)) - v_mix;
    }
  }
  if (post_dist_mix) {
    for (int i = tid; i < n_a; i += THREADS) {
      double m = 0.0, sm = 0.0;
      for (int s = 0; s < n_z; ++s) {
        const size_t o = (size_t)(s * n_tasks + b) * (size_t)n_a + (size_t)i;
        const double sum = ds_ws[o];
        sky_lse_add(m, sm, sum == 0.0 ? -INFINITY : dm_ws[o] + log(sum));
      }
      post_dist_mix[(size_t)b * (size_t)n_a + (size_t)i] = sm == 0.0 ? -INFINITY : (m + (log(sm) - log_nz)) - v_mix;
    }
  }
}

}  // namespace npf

extern "C" int64_t npf_waveform_loglike_sky_dist_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t pts, int32_t n_pix, int32_t n_tau,
                                                                 int32_t n_a) {
  using namespace npf;
  if (sky_sizes_bad(n_rows, n_det, pts, n_pix, n_tau) || n_a < 1 || n_a > kSkydMaxScales) return NPF_EINVAL;
  const SkydLayout L = skyd_layout(n_rows, n_det, pts, n_pix, n_tau, n_a);
  if (L.total < 0) return NPF_EINVAL;  // the panels' count does not fit int64
  return L.total * (int64_t)sizeof(double) + 128;  // (+ 128: the panels are aligned to 128 bytes)
}

extern "C" int npf_waveform_loglike_sky_dist(const float* h, int32_t h_ld, const float* d, const float* wgt, int32_t wgt_rows,
                                             const float* freq, int32_t freq_rows, const int32_t* n_valid, const double* resp,
                                             const double* delay, const double* log_prior, int32_t n_rows, int32_t n_tasks,
                                             int32_t n_det, int32_t pts, int32_t n_pix, double tau0, double dtau, int32_t n_tau,
                                             const double* scales, const double* log_prior_scale, int32_t n_a, double* lnl_vol,
                                             int32_t* pix_index, int32_t* scale_index, int32_t* tau_index, double* snr, double* scale_hat,
                                             double* lnl, double* post_sky, double* post_dist, double* post_joint, double* dist_mean,
                                             double* dist_std, double* post_sky_mix, double* post_dist_mix, void* workspace, void* stream) {
  using namespace npf;
  if (wf_loglike_net_args_bad(h, h_ld, d, wgt, wgt_rows, freq, freq_rows, delay, resp, n_rows, n_tasks, n_det, pts, n_tau, workspace))
    return NPF_EINVAL;
  if (!freq || freq_rows != 1 || sky_sizes_bad(n_rows, n_det, pts, n_pix, n_tau)) return NPF_EINVAL;
  if (!scales || !log_prior_scale || n_a < 1 || n_a > kSkydMaxScales) return NPF_EINVAL;
  if (!lnl_vol && !pix_index && !scale_index && !tau_index && !snr && !scale_hat && !lnl && !post_sky && !post_dist && !post_joint &&
      !dist_mean && !dist_std && !post_sky_mix && !post_dist_mix)
    return NPF_EINVAL;
  const SkydLayout D = skyd_layout(n_rows, n_det, pts, n_pix, n_tau, n_a);
  if (D.total < 0) return NPF_EINVAL;
  if (n_tau == 0) tau0 = dtau = 0.0;  // the one candidate is tau = 0
  const SkyLayout& L = D.sky;
  double* ws = reinterpret_cast<double*>(((uintptr_t)workspace + 127) & ~(uintptr_t)127);
  double2 *step = (double2*)(ws + L.step), *start = (double2*)(ws + L.start), *U = (double2*)(ws + L.u), *V = (double2*)(ws + L.v);
  int32_t* jx = reinterpret_cast<int32_t*>(ws + L.jx);
  hipStream_t st = (hipStream_t)stream;

  const int64_t prep_blocks = L.rows_pad + L.pix_pad + 1 + L.chunks;
  hipLaunchKernelGGL((sky_prep_kernel<kSkyJC, kSkyPrepThreads>), dim3((unsigned)prep_blocks), dim3(kSkyPrepThreads), 0, st, h, h_ld, d, wgt,
                     (int)(wgt_rows != 1), freq, n_valid, resp, delay, log_prior, n_rows, n_tasks, n_det, pts, n_pix, tau0, dtau, n_tau,
                     (int)L.rows_pad, (int)L.pix_pad, (int)L.tp, ws + L.hhk, step, start, U, V);
  NPF_CHECK_LAUNCH();
  const int64_t pix_tiles = L.pix_pad / 16;
  hipLaunchKernelGGL(skyd_corr_kernel<kSkyJC>, dim3((unsigned)(L.rows_pad / 16), (unsigned)((pix_tiles + kSkyCorrWaves - 1) / kSkyCorrWaves)),
                     dim3(64 * kSkyCorrWaves), 0, st, ws + L.hhk, step, start, U, V, resp, log_prior, n_rows, n_det, n_pix, (int)L.pix_pad,
                     (int)L.tp, n_tau, (int)L.chunks, ws + D.x, ws + L.xm, ws + L.hh, jx);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(skyd_scale_kernel<kSkydSC>, dim3((unsigned)n_rows, (unsigned)((n_pix + 63) / 64), (unsigned)((n_a + kSkydSC - 1) / kSkydSC)),
                     dim3(64), 0, st, ws + D.x, ws + L.xm, ws + L.hh, log_prior, scales, log_prior_scale, n_pix, (int)L.pix_pad, n_tau, n_a,
                     ws + D.w);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(skyd_finish_kernel, dim3(n_tasks), dim3(kSkydFinishThreads), 0, st, ws + D.w, ws + L.xm, ws + L.hh, jx, scales, ws + L.lu,
                     ws + D.ss, ws + D.dm, ws + D.ds, n_rows, n_tasks, n_pix, (int)L.pix_pad, n_a, lnl_vol, pix_index, scale_index, tau_index,
                     snr, scale_hat, lnl, post_sky, post_dist, post_joint, dist_mean, dist_std, post_sky_mix, post_dist_mix);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}
