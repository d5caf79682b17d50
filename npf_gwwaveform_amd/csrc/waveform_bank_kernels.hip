// Bank match (npf_waveform_match_bank): every predicted waveform h_r = A e^{i phi} against every template v_g = A' e^{i phi'} of ONE
// bank shared by the rows, maximised over the constant phase and the time-shift grid tau_j = tau0 + j dtau:
//   c_j[r, g] = sum_t u_{r,t} e^{i 2 pi f_t tau_j} conj(v_{g,t}),   u = w A e^{i phi},   hh_r = sum_t w A^2,   gg_g = sum_t w A'^2.
// The rotation by the shift depends on the row only, so it is done once per (row, point, shift) and shared by every template, and the
// complex product is a real GEMM with K = 2 pts on v_mfma_f64_16x16x4_f64.  DOUBLE throughout, from fp32 inputs widened exactly.
//
// Launch 1 (bank_prep_kernel): one workgroup per row, per template, and per auxiliary row (the step e^{i 2 pi f dtau} and the start
// e^{i 2 pi f tau_c} of every chunk of JC shifts).  Weights and frequencies are ONE row shared by everything, so the live points
// (0 < w < inf) are the same for every pair: every workgroup scans the weights and COMPACTS, live point number p goes to position p
// of its panel, and nothing of a removed point is read.  A call with removed points therefore builds the panels of the same call
// with those points cut out, bit for bit.  Panels are padded with exact zeros (u, v) and ones (step, start) to a multiple of four
// points and to whole tiles of 16 rows / templates.  hh / gg are summed over the compacted positions in a fixed order.
// Panel layout: the MFMA fragment order, [tile of 16][k-step of 4 points][lane = (point & 3) * 16 + (row & 15)][Re, Im], so a
// wavefront loads the (Re, Im) pairs of a k-step with one contiguous 1 KiB access.
//
// Launch 2 (bank_corr_kernel): one wavefront per (16 rows, 16 templates), four template tiles per workgroup.  Per chunk of JC shifts
// the 2 JC accumulator tiles (Re c_j, Im c_j) live in registers; per k-step of four points the lane rotates its own point,
// z = u start, then per shift four MFMAs -- Re c += Re z Re v + Im z Im v, Im c += Im z Re v + Re z (-Im v) -- and z <- z step: the
// recurrence of npf_waveform_match, restarted at every chunk.  One operand pair per lane feeds 4 JC matrix instructions, so the
// kernel needs no LDS.  After a chunk the running maximum of |c_j|^2, its first index and c there are updated in registers; nothing
// of size [n_rows][n_bank][n_tau] is written.  C/D fragment of the f64 instruction: column = lane & 15, row = (lane >> 4) + 4 * reg.
// Launch 3 (bank_best_kernel, when best_index / best_match are asked for): one wavefront per row over the rounded matches.
// No atomics, a fixed K order and tile order: a second call on the same inputs gives the same bits.
//
// Workspace (after alignment to 16 bytes): [n_live (int32), pad][hh: rows_pad][gg: bank_pad][step: tp x 2][start: chunks x tp x 2]
// [U: rows_pad x tp x 2][V: bank_pad x tp x 2][sq: (rows_pad + bank_pad) x tp][match: n_rows x n_bank floats], tp = pts rounded up to 4.
#include "waveform_common.hpp"  // kWfJC, kWfMaxTau, kWfTwoPi, wf_chunks, block_sum_store

namespace npf {

constexpr int kBankPrepThreads = 256;
constexpr int kBankCorrWaves = 4;  // template tiles per workgroup of launch 2
constexpr int kBankMaxRows = 1 << 24, kBankMaxBank = 1 << 20;

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct BankLayout {
  int64_t rows_pad, bank_pad, tp, chunks;
  int64_t hh, gg, step, start, u, v, sq, match, total;  // offsets in doubles (total: doubles, the float matches included)
};

inline BankLayout bank_layout(int n_rows, int n_bank, int pts, int n_tau) {
  BankLayout L;
  L.rows_pad = ((int64_t)n_rows + 15) / 16 * 16;
  L.bank_pad = ((int64_t)n_bank + 15) / 16 * 16;
  L.tp = ((int64_t)pts + 3) / 4 * 4;
  L.chunks = wf_chunks(n_tau);
  L.hh = 2;
  L.gg = L.hh + L.rows_pad;
  L.step = L.gg + L.bank_pad;
  L.start = L.step + 2 * L.tp;
  L.u = L.start + 2 * L.tp * L.chunks;
  L.v = L.u + 2 * L.tp * L.rows_pad;
  L.sq = L.v + 2 * L.tp * L.bank_pad;
  L.match = L.sq + L.tp * (L.rows_pad + L.bank_pad);
  L.total = L.match + ((int64_t)n_rows * n_bank + 1) / 2;
  return L;
}

// position of (row, compacted point p) in a fragment-ordered panel of ks_max k-steps per tile, in (Re, Im) pairs
__device__ __forceinline__ size_t bank_frag_index(int row, int p, int ks_max) {
  return ((size_t)(row >> 4) * (size_t)ks_max + (size_t)(p >> 2)) * 64 + (size_t)(((p & 3) << 4) | (row & 15));
}

template <int JC, int THREADS>
__global__ __launch_bounds__(THREADS) void bank_prep_kernel(const float* __restrict__ h, int h_ld, const float* __restrict__ bank,
                                                             const float* __restrict__ wgt, const float* __restrict__ freq, int n_rows,
                                                             int n_bank, int pts, double tau0, double dtau, int n_tau, int rows_pad,
                                                             int bank_pad, int tp, int* n_live_out, double* hh_d, double* gg_d,
                                                             double2* step, double2* start, double2* U, double2* V, double* sq,
                                                             float* __restrict__ hh_out, float* __restrict__ gg_out) {
  constexpr int WAVES = THREADS / 64;
  __shared__ int wave_cnt[WAVES];
  __shared__ double red[WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ks_max = tp >> 2;
  // what this workgroup writes: 0 a row of h, 1 a template, 2 the step, 3 the start of chunk `idx`
  int kind, idx;
  if (b < rows_pad) {
    kind = 0, idx = b;
  } else if (b < rows_pad + bank_pad) {
    kind = 1, idx = b - rows_pad;
  } else if (b == rows_pad + bank_pad) {
    kind = 2, idx = 0;
  } else {
    kind = 3, idx = b - rows_pad - bank_pad - 1;
  }
  const bool pad_row = (kind == 0 && idx >= n_rows) || (kind == 1 && idx >= n_bank);  // a row of zeros that fills the last tile
  const float* src = kind == 0 ? h + (size_t)idx * (size_t)pts * (size_t)h_ld : bank + (size_t)idx * (size_t)pts * 2;
  const int ld = kind == 0 ? h_ld : 2;
  double2* panel = kind == 0 ? U : V;
  double* sq_row = sq + (size_t)b * (size_t)tp;  // (kinds 0 and 1 only)
  const double tau_c = tau0 + (double)(idx * JC) * dtau;  // (kind 3: the chunk's first shift)

  int n_live = 0;
  if (!pad_row) {
    for (int base = 0; base < pts; base += THREADS) {
      const int t = base + tid;
      float wf = 0.f;
      if (t < pts) wf = wgt ? wgt[t] : 1.f;
      const bool live = wf > 0.f && wf < INFINITY;  // else a removed point: nothing else of it is read
      const unsigned long long mask = __ballot(live);
      if (lane == 0) wave_cnt[wave] = __popcll(mask);
      __syncthreads();
      int p = n_live + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w < wave) p += wave_cnt[w];
        n_live += wave_cnt[w];
      }
      if (live) {
        if (kind <= 1) {
          const double w = (double)wf, A = (double)src[(size_t)t * ld], ph = (double)src[(size_t)t * ld + 1];
          double sn, cs;
          sincos(ph, &sn, &cs);
          const double a = kind == 0 ? w * A : A;
          panel[bank_frag_index(idx, p, ks_max)] = make_double2(a * cs, a * sn);
          sq_row[p] = (w * A) * A;
        } else {
          double sn = 0.0, cs = 1.0;
          if (n_tau > 0) sincos((kWfTwoPi * (double)freq[t]) * (kind == 2 ? dtau : tau_c), &sn, &cs);
          (kind == 2 ? step : start + (size_t)idx * (size_t)tp)[p] = make_double2(cs, sn);
        }
      }
      __syncthreads();  // (wave_cnt is rewritten by the next pass)
    }
  }
  // behind the live points: zeros in the panels, ones in the rotations
  for (int p = n_live + tid; p < tp; p += THREADS) {
    if (kind <= 1) {
      panel[bank_frag_index(idx, p, ks_max)] = make_double2(0.0, 0.0);
    } else {
      (kind == 2 ? step : start + (size_t)idx * (size_t)tp)[p] = make_double2(1.0, 0.0);
    }
  }
  if (kind == 2 && tid == 0) *n_live_out = n_live;
  if (kind > 1) return;

  // hh / gg over the compacted positions: thread i owns positions i, i + THREADS, ..., then lanes and waves in a fixed order
  __syncthreads();  // (sq_row as the workgroup wrote it)
  double s = 0.0;
  for (int p = tid; p < n_live; p += THREADS) s += sq_row[p];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += red[w];
    (kind == 0 ? hh_d : gg_d)[idx] = total;
    float* out = kind == 0 ? hh_out : gg_out;
    if (out && !pad_row) out[idx] = (float)total;
  }
}

// The k loop of one chunk: nj shifts (FULL: nj == JC, no guards) accumulated over the ks_n k-steps of the live points.
template <int JC, bool FULL>
__device__ __forceinline__ void bank_chunk(const double2* __restrict__ up, const double2* __restrict__ vp,
                                           const double2* __restrict__ step, const double2* __restrict__ start, int ks_n, int kq, int nj,
                                           f64x4 (&acc_re)[JC], f64x4 (&acc_im)[JC]) {
  if (ks_n <= 0) return;
  double2 u = up[0], v = vp[0], s = step[kq], st = start[kq];
  for (int ks = 0; ks < ks_n; ++ks) {
    const int nx = ks + 1 < ks_n ? ks + 1 : ks;  // the next k-step's operands, in flight behind this one's matrix instructions
    const double2 u_n = up[(size_t)nx * 64], v_n = vp[(size_t)nx * 64], s_n = step[nx * 4 + kq], st_n = start[nx * 4 + kq];
    double zr = u.x * st.x - u.y * st.y, zi = u.x * st.y + u.y * st.x;
    const double vr = v.x, vi = v.y, nvi = -v.y;
#pragma unroll
    for (int i = 0; i < JC; ++i) {
      if (FULL || i < nj) {
        acc_re[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr, vr, acc_re[i], 0, 0, 0);
        acc_im[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi, vr, acc_im[i], 0, 0, 0);
        acc_re[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi, vi, acc_re[i], 0, 0, 0);
        acc_im[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr, nvi, acc_im[i], 0, 0, 0);
        if (i + 1 < JC) {
          const double nr = zr * s.x - zi * s.y;
          zi = zr * s.y + zi * s.x;
          zr = nr;
        }
      }
    }
    u = u_n, v = v_n, s = s_n, st = st_n;
  }
}

template <int JC>
__global__ __launch_bounds__(64 * kBankCorrWaves) void bank_corr_kernel(
    const int* __restrict__ n_live_p, const double* __restrict__ hh_d, const double* __restrict__ gg_d, const double2* __restrict__ step,
    const double2* __restrict__ start, const double2* __restrict__ U, const double2* __restrict__ V, int n_rows, int n_bank, int tp,
    int n_tau, int chunks, float* __restrict__ match, float* __restrict__ mismatch, int32_t* __restrict__ tau_index,
    float* __restrict__ phase, double* __restrict__ dot, float* __restrict__ match_ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x, gt = blockIdx.y * kBankCorrWaves + wave;
  if (gt * 16 >= n_bank) return;  // (no barrier below: a wavefront without a tile leaves)
  const int ks_max = tp >> 2, ks_n = (*n_live_p + 3) >> 2, kq = lane >> 4;
  const double2* up = U + (size_t)rt * (size_t)ks_max * 64 + lane;
  const double2* vp = V + (size_t)gt * (size_t)ks_max * 64 + lane;

  double best[4], c_re[4], c_im[4];
  int best_j[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) best[q] = -1.0, c_re[q] = 0.0, c_im[q] = 0.0, best_j[q] = 0;

  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int j0 = chunk * JC, nj = n_tau > 0 ? (n_tau - j0 < JC ? n_tau - j0 : JC) : 1;
    f64x4 acc_re[JC], acc_im[JC];
#pragma unroll
    for (int i = 0; i < JC; ++i) acc_re[i] = f64x4{0.0, 0.0, 0.0, 0.0}, acc_im[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double2* st = start + (size_t)chunk * (size_t)tp;
    if (nj == JC) {
      bank_chunk<JC, true>(up, vp, step, st, ks_n, kq, nj, acc_re, acc_im);
    } else {
      bank_chunk<JC, false>(up, vp, step, st, ks_n, kq, nj, acc_re, acc_im);
    }
#pragma unroll
    for (int i = 0; i < JC; ++i) {
      if (i < nj) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double re = acc_re[i][q], im = acc_im[i][q], m2 = re * re + im * im;
          if (m2 > best[q] || j0 + i == 0) {  // (j ascends: the smallest index stays; j = 0 always enters, so a NaN there stays)
            best[q] = m2;
            best_j[q] = j0 + i;
            c_re[q] = re;
            c_im[q] = im;
          }
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rt * 16 + (lane >> 4) + 4 * q, g = gt * 16 + (lane & 15);  // the f64 C/D fragment: row = (lane >> 4) + 4 * reg
    if (r >= n_rows || g >= n_bank) continue;
    const double prod = hh_d[r] * gg_d[g];
    const bool degenerate = prod == 0.0;
    const double re = degenerate ? 0.0 : c_re[q], im = degenerate ? 0.0 : c_im[q];
    const double m = degenerate ? 0.0 : sqrt(re * re + im * im) / sqrt(prod);
    const size_t o = (size_t)r * (size_t)n_bank + (size_t)g;
    if (match) match[o] = (float)m;
    if (match_ws) match_ws[o] = (float)m;
    if (mismatch) mismatch[o] = (float)(1.0 - m);
    if (tau_index) tau_index[o] = degenerate ? 0 : best_j[q];
    if (phase) phase[o] = degenerate ? 0.f : (float)atan2(im, re);
    if (dot) dot[2 * o] = re, dot[2 * o + 1] = im;
  }
}

// One wavefront per row: the largest match that is not NaN with the smallest template index, 0 if there is none.
__global__ __launch_bounds__(64) void bank_best_kernel(const float* __restrict__ m, int n_bank, int32_t* __restrict__ best_index,
                                                        float* __restrict__ best_match) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* row = m + (size_t)r * (size_t)n_bank;
  float best = -1.f;  // (a match is >= 0)
  int best_g = n_bank;
  for (int g = lane; g < n_bank; g += 64) {
    const float v = row[g];
    if (v > best) {  // (g ascends: the smallest index of the lane stays; a NaN never enters)
      best = v;
      best_g = g;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int og = __shfl_xor(best_g, off);
    if (ob > best || (ob == best && og < best_g)) {
      best = ob;
      best_g = og;
    }
  }
  if (lane != 0) return;
  if (best_g >= n_bank) best_g = 0;  // (every match of the row is NaN)
  if (best_index) best_index[r] = best_g;
  if (best_match) best_match[r] = row[best_g];
}

inline bool bank_sizes_bad(int n_rows, int n_bank, int pts, int n_tau) {
  return n_rows <= 0 || n_bank <= 0 || pts <= 0 || n_rows > kBankMaxRows || n_bank > kBankMaxBank || n_tau < 0 || n_tau > kWfMaxTau;
}

}  // namespace npf

extern "C" int64_t npf_waveform_match_bank_workspace_bytes(int32_t n_rows, int32_t n_bank, int32_t pts, int32_t n_tau) {
  using namespace npf;
  if (bank_sizes_bad(n_rows, n_bank, pts, n_tau)) return NPF_EINVAL;
  return bank_layout(n_rows, n_bank, pts, n_tau).total * (int64_t)sizeof(double) + 16;  // (+ 16: the panels are aligned to 16 bytes)
}

extern "C" int npf_waveform_match_bank(const float* h, int32_t h_ld, const float* bank, const float* wgt, const float* freq,
                                       int32_t n_rows, int32_t n_bank, int32_t pts, double tau0, double dtau, int32_t n_tau, float* hh,
                                       float* gg, float* match, float* mismatch, int32_t* tau_index, float* phase, double* dot,
                                       int32_t* best_index, float* best_match, void* workspace, void* stream) {
  using namespace npf;
  if (bank_sizes_bad(n_rows, n_bank, pts, n_tau) || !h || !bank || !workspace || h_ld < 2 || (n_tau > 0 && !freq)) return NPF_EINVAL;
  if (!hh && !gg && !match && !mismatch && !tau_index && !phase && !dot && !best_index && !best_match) return NPF_EINVAL;
  const BankLayout L = bank_layout(n_rows, n_bank, pts, n_tau);
  double* ws = reinterpret_cast<double*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  int* n_live = reinterpret_cast<int*>(ws);
  double2 *step = (double2*)(ws + L.step), *start = (double2*)(ws + L.start), *U = (double2*)(ws + L.u), *V = (double2*)(ws + L.v);
  float* match_ws = reinterpret_cast<float*>(ws + L.match);
  const bool want_best = best_index || best_match, want_pairs = match || mismatch || tau_index || phase || dot || want_best;
  hipStream_t st = (hipStream_t)stream;

  const int64_t prep_blocks = L.rows_pad + L.bank_pad + 1 + L.chunks;
  hipLaunchKernelGGL((bank_prep_kernel<kWfJC, kBankPrepThreads>), dim3((unsigned)prep_blocks), dim3(kBankPrepThreads), 0, st, h, h_ld, bank,
                     wgt, freq, n_rows, n_bank, pts, tau0, dtau, n_tau, (int)L.rows_pad, (int)L.bank_pad, (int)L.tp, n_live, ws + L.hh,
                     ws + L.gg, step, start, U, V, ws + L.sq, hh, gg);
  NPF_CHECK_LAUNCH();
  if (!want_pairs) return NPF_OK;
  const int64_t gts = L.bank_pad / 16;
  hipLaunchKernelGGL(bank_corr_kernel<kWfJC>, dim3((unsigned)(L.rows_pad / 16), (unsigned)((gts + kBankCorrWaves - 1) / kBankCorrWaves)),
                     dim3(64 * kBankCorrWaves), 0, st, n_live, ws + L.hh, ws + L.gg, step, start, U, V, n_rows, n_bank, (int)L.tp, n_tau,
                     (int)L.chunks, match, mismatch, tau_index, phase, dot, want_best && !match ? match_ws : nullptr);
  NPF_CHECK_LAUNCH();
  if (want_best) {
    hipLaunchKernelGGL(bank_best_kernel, dim3(n_rows), dim3(64), 0, st, match ? match : match_ws, n_bank, best_index, best_match);
    NPF_CHECK_LAUNCH();
  }
  return NPF_OK;
}
