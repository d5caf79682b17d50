// Attention over PADDED contexts whose real sizes are data on the device (npf_masked_attn_*): every task b has n_valid[b] real
// context points out of the n_keys rows its tensors hold, and n_valid is an int32 tensor the kernels read -- the host never does,
// so a launch can sit in a captured graph and see new counts at every replay.  (The mean over such a context,
// npf_masked_mean_fwd / _bwd, is the MASKED instance of the mean kernels in layout_kernels.hip.)
//
// What they compute, in the reference's terms: DotAttender.forward (npf/architectures/attention.py:129-164, 204-220) of the batch
// whose task b was cut to its first n_valid[b] context points.
//
// Three kernels: masked_attn_fwd_kernel, masked_attn_dq_kernel and masked_attn_dkv_kernel.  Scaled-dot attention, one head, feature
// widths d = 4 ... 256 (heads of a multihead attention come as extra tasks, npf_split_heads), fp32 throughout on
// v_mfma_f32_16x16x4_f32 with the operand roles of mha_kernel.hip (the first contraction TRANSPOSED, so the probabilities are
// directly the B operand of the second).  Keys are walked in blocks of KB = 32 (16 at the 256-wide instance) through LDS with an
// online softmax: running maximum m and sum l per query, the accumulator rescaled by exp(m_old - m_new) -- no limit on n_keys.
// The walk ends at n_valid[b]: blocks wholly beyond it are never staged or multiplied, and inside the last block the rows beyond
// it are staged as zeros and their scores set to -inf, so whatever the padding rows hold (NaN included) never meets a multiply.
// The backward pass recomputes the probabilities from the saved log-sum-exp in two kernels: d_q like the forward pass (a
// workgroup = 64 queries, walking the key blocks), d_k / d_v with a workgroup per 16 keys whose four waves walk the queries and
// meet in LDS -- no atomics, so the result does not depend on the launch.  Rows >= n_valid[b] of d_k / d_v are stored as zeros.
//
// Query counts (n_q_valid; the NQ instances): task b has n_q_valid[b] real queries out of n_queries (padded targets).  A workgroup
// whose 64 queries all lie beyond the count stores its zeros (O, d_q; lse = 0) and returns before it stages a key block; inside the
// boundary block the queries beyond the count are not live; the d_k / d_v walk over the queries ends at the count, so Q / O / dO /
// lse rows beyond it are never read.  Block order and summation order do not depend on the query count: the rows below the counts
// come out bit-identical with and without it.
//
// WHICH keys a query attends over is the forward kernel's KEY RULE, a traits struct (MkPlain, MkPrefix, MkLoo, MkWeighted below):
// compile-time flags plus the few members the rule needs, so every rule is an instance of the one forward body and pays only for
// what it uses.  The backward kernels know the plain and the weighted rule (their WGT flag).
//  * MkPlain (npf_masked_attn_fwd / _nq, _bwd / _bwd_nq): the keys below the count.
//  * MkPrefix (npf_masked_attn_fwd_prefix, inference only), a shared prefix and an own tail: task j walks the key blocks of PREFIX
//    task j % n_pre_tasks up to its count and then those of its own tail up to n_tail[j] -- S function samples of one conditioned
//    context read the context's keys / values from one copy and keep only the rows they drew themselves.  Each segment ends as the
//    single one does; the running maximum, sum and accumulator carry over the switch.  With every tail count 0 the block sequence
//    is that of MkPlain.
//  * MkLoo (npf_masked_attn_fwd_loo, inference only), leave-one-out: query row t of a task attends over the task's keys without key
//    row t (row numbers inside the task; Q and K / V stay separate tensors) -- the predictive of every context point from the
//    others, out of one encode of the context.
//  * MkWeighted (npf_masked_attn_fwd_weighted / _ex, _bwd_weighted), per-replicate key weights: task j = s * n_ctx_tasks + b is
//    replicate s of context task b = j % n_ctx_tasks.  It reads the queries, keys, values and counts of task b -- ONE stored copy of
//    the context serves every replicate -- and row j of W, a non-negative weight per key: p_k ~ w_k exp(s_k) (bootstrap
//    multiplicities, fold masks, down-weighted points).  A key is admissible iff it lies below the count and 0 < w < +inf.
//
// What the LOO and the weighted rule add to the walk (R::MAY_BE_EMPTY):
//  * a query can be without an admissible key in a block (or in the whole walk) although the block was staged: the running maximum
//    may stay -inf, so the exponentials are taken against 0 then (exp(-inf - 0) = 0, never exp(-inf + inf)); a block that holds
//    nothing for a query leaves its m, l and accumulator as they were, and a query without any key ends at l = 0 -> exact zeros,
//    stored as zeros and not as accumulator * 0.
//  * LOO: p = 0 is not enough to keep v[t] out of row t (0 * Inf = NaN on the matrix unit).  The 16 queries of a wave are rows
//    own0 .. own0 + 15, and the key sub-blocks are 16 rows at multiples of 16, so the own rows of a wave are exactly one sub-block:
//    its P V product runs on the vector unit, key by key, with the value row replaced by zeros in the lanes of the query it belongs
//    to (mk_pv_own_rows).  Every other sub-block is the MFMA product.
//  * (every rule, MK_SEG below: the score contraction is added in segments of 64 features, each a chain of its own from 0, the
//    segments added afterwards: an fp32 chain rounds at the size of its running sum, and scores that share a large component
//    (|q . k| of 1600 at 256 features) are told apart only by what those roundings leave.  The forward and both backward kernels
//    segment alike, under every rule, so the rows of a LOO call that have no own key are those of MkPlain.)
//  * weighted: the weight is per key and task, not per query, so an inadmissible key is staged as zeros in its K AND its V row
//    (mk_stage_weighted) and its score set to -inf: whatever those rows or the weight hold (NaN / Inf included) never meets a
//    multiply -- no vector-unit side path.  The score is scale <q, k> + log w, exp(s + log w - m) rather than w exp(s - m): the
//    running maximum is taken over THAT, over the admissible keys of the replicate alone, so a replicate whose highest-scoring key
//    has weight 0 never sees that key's score, and a tiny weight on a high score cannot underflow what a large one overflows.
//    log 1 = 0 and s + 0 = s exactly, so with every weight 1.0 and one replicate the walk, the summation order and the bits are
//    those of MkPlain with a query count.
//
// Training through key weights (npf_masked_attn_fwd_weighted_ex = MkWeighted<true>, which also stores the log-sum-exp -- stores only,
// O has the bits of MkWeighted<false>; npf_masked_attn_bwd_weighted = the WGT instances of the backward kernels at one replicate,
// task j reads row j of W).  With a_qk = scale <q, k> + log w_k, p_qk = exp(a_qk - lse_q), D_q = <dO_q, O_q> and
// dA_qk = p_qk (<dO_q, v_k> - D_q):  dq_q = scale sum_k dA_qk k_k,  dk_k = scale sum_q dA_qk q_q,  dv_k = sum_q p_qk dO_q  and
// dw_k = (sum_q dA_qk) / w_k  (d a_qk / d w_k = 1 / w_k), reduced in the d_k / d_v workgroup -- no atomics.  An inadmissible key
// has probability 0, and its d_k / d_v rows and its d_w are exact zeros -- a removed point is removed: there is no one-sided
// derivative at w = 0.  A query without an admissible key has lse = 0 and meets no admissible key.
#include <type_traits>

#include "npf_common.hpp"

namespace npf {

// feature f of point p of a task's PT32 tensor with Fp (padded) features
__device__ __forceinline__ size_t mk_pt(int task, int tiles, int Fp, int p, int f) {
  return ((((size_t)task * tiles + (p >> 5)) * (Fp >> 2) + (f >> 2)) * 32 + (p & 31)) * 4 + (f & 3);
}

__device__ __forceinline__ f32x4 mk_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float mk_sum4(float v) {  // over the four lanes (g = 0..3) that share a column
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ float mk_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

// rows key0 .. key0 + KB - 1 of a task's PT32 tensor into LDS, LD floats apart (LD even); rows >= nv and features >= d as zeros
template <int DP, int KB, int LD>
__device__ __forceinline__ void mk_stage(const float* __restrict__ X, int b, int tiles, int Fp, int d, int key0, int nv, float* S,
                                         int tid) {
  for (int i = tid; i < KB * (DP / 4); i += 256) {
    const int p = i % KB, f4 = i / KB, key = key0 + p;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (key < nv && 4 * f4 < d) x = *(const f32x4*)(X + mk_pt(b, tiles, Fp, key, 4 * f4));
    *(float2*)(S + p * LD + 4 * f4) = float2{x[0], x[1]};
    *(float2*)(S + p * LD + 4 * f4 + 2) = float2{x[2], x[3]};
  }
}

// mk_stage for K and V at once under key weights (wrow: the task's weight per key): the rows of inadmissible keys as zeros too.
// The weight is read below the count only.
template <int DP, int KB, int LDK, int LDV>
__device__ __forceinline__ void mk_stage_weighted(const float* __restrict__ K, const float* __restrict__ V,
                                                  const float* __restrict__ wrow, int b, int tiles, int Fp, int d, int key0, int nv,
                                                  float* Ks, float* Vs, int tid) {
  for (int i = tid; i < KB * (DP / 4); i += 256) {
    const int p = i % KB, f4 = i / KB, key = key0 + p;
    f32x4 x = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
    if (key < nv && 4 * f4 < d) {
      const float wk = wrow[key];
      if (wk > 0.f && wk < INFINITY) {
        x = *(const f32x4*)(K + mk_pt(b, tiles, Fp, key, 4 * f4));
        y = *(const f32x4*)(V + mk_pt(b, tiles, Fp, key, 4 * f4));
      }
    }
    *(float2*)(Ks + p * LDK + 4 * f4) = float2{x[0], x[1]};
    *(float2*)(Ks + p * LDK + 4 * f4 + 2) = float2{x[2], x[3]};
    *(float2*)(Vs + p * LDV + 4 * f4) = float2{y[0], y[1]};
    *(float2*)(Vs + p * LDV + 4 * f4 + 2) = float2{y[2], y[3]};
  }
}

// log w of the block's keys into LDS, -inf where the key is not admissible
template <int KB>
__device__ __forceinline__ void mk_stage_logw(const float* __restrict__ wrow, int key0, int nv, float* Lw, int tid) {
  if (tid < KB) {
    const int key = key0 + tid;
    const float wk = key < nv ? wrow[key] : 0.f;
    Lw[tid] = (wk > 0.f && wk < INFINITY) ? logf(wk) : -INFINITY;  // (NaN fails both comparisons)
  }
}

// Row q of a task's [T] PT32 tensor as an MFMA operand, X[q][4 kc + g]; zeros for a row that is not live and for features >= d
template <int NKC>
__device__ __forceinline__ void mk_load_row(const float* __restrict__ X, int b, int tilesT, int Fp, int d, int q, int g, bool live,
                                            float (&x)[NKC]) {
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) x[kc] = (live && 4 * kc < d) ? X[mk_pt(b, tilesT, Fp, q, 4 * kc) + g] : 0.f;
}

// Row q of a task's [T] PT32 tensor (O or d_q) from the lane's part x^T[f = 16 dt + 4 g + i][q]: x * factor, or zeros unless `keep`;
// every feature of the padded width, and the rows of the last tile beyond T as well
template <int NDT>
__device__ __forceinline__ void mk_store_row(float* __restrict__ X, int b, int tilesT, int Fp, int q, int g, const f32x4* x,
                                             float factor, bool keep) {
  if (q < tilesT * 32) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      if (16 * dt + 4 * g < Fp)
        *(f32x4*)(X + mk_pt(b, tilesT, Fp, q, 16 * dt + 4 * g)) = keep ? x[dt] * factor : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// LOO: P V of the key sub-block that holds the wave's own rows (Vsb: its 16 value rows in LDS; P: its probabilities,
// P^T[key = 4 g + i][q = c]) on the vector unit, key by key, the value row as zeros in the lanes of the query it belongs to
template <int NDT, int LDV>
__device__ __forceinline__ void mk_pv_own_rows(const float* Vsb, const f32x4 P, int c, int g, f32x4 (&o)[NDT]) {
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const float p = __shfl(P[kk & 3], c + 16 * (kk >> 2));  // P[key own0 + kk][q = c]
    const bool own = kk == c;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const f32x4 v = *(const f32x4*)(Vsb + kk * LDV + 16 * dt + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[dt][i] = fmaf(own ? 0.f : v[i], p, o[dt][i]);
    }
  }
}

// MFMA steps (of 4 features) per segment of the score contraction <q, k>: one chain up to 64 features, chains of 64 features added
// in order beyond (the 128- and 256-wide instances).  One chain of 64 steps left a score of 100 at 256 features with an error of
// 2e-5 (its running sum reaches 16 |s|, and each step rounds at that size), and the output with 3e-5 of its size.
template <int NKC>
inline constexpr int MK_SEG = NKC > 16 ? 16 : NKC;

template <int DP>
struct MkGeom {
  static constexpr int KB = DP == 256 ? 16 : 32;  // keys per block: 33 KB of LDS for keys + values at every width
  static constexpr int NSB = KB / 16, NKC = DP / 4, NDT = DP / 16;
  // row strides: an A operand read [row = lane % 16][k = lane / 16] is conflict-free at LD = 2 mod 32, a read
  // [row = 4 (lane / 16) + j][lane % 16] at LD = 4 mod 32 (ds_read_b32: 32 banks, the two halves of the wave apart)
  static constexpr int LDA = DP + 2, LDB = DP + 4;
};

// The key rules of the forward kernel (the file's header says what each computes).
//  PFX: a second key segment (K2, V2, tail_count) follows the first.   LOO: a query never meets the key of its own row number.
//  WGT: a weight per key, row b of W.   LSE: the log-sum-exp is stored (MkPlain: unless lse is null).
//  NQ_NULLABLE: whether there is a query count is the null check of n_q_valid at run time, not the kernel's NQ flag.
//  MAY_BE_EMPTY: a staged block can hold nothing for a query.
//  key_task / query_task: the task whose K / V / n_valid, and whose Q / n_q_valid, task b reads.
struct MkPlain {
  static constexpr bool PFX = false, LOO = false, WGT = false, LSE = true, NQ_NULLABLE = false, MAY_BE_EMPTY = false;
  static constexpr const float* K2 = nullptr;
  static constexpr const float* V2 = nullptr;
  static constexpr int n_keys2 = 0;
  __device__ __forceinline__ int key_task(int b) const { return b; }
  __device__ __forceinline__ int query_task(int b) const { return b; }
  __device__ __forceinline__ int tail_count(int) const { return 0; }
};
struct MkPrefix : MkPlain {
  static constexpr bool PFX = true, LSE = false;
  const float* K2;
  const float* V2;
  const int32_t* n_valid2;
  int n_keys2, n_pre_tasks;
  __device__ __forceinline__ int key_task(int b) const { return b % n_pre_tasks; }
  __device__ __forceinline__ int tail_count(int b) const { return clamp_count(n_valid2, b, n_keys2); }
};
struct MkLoo : MkPlain {
  static constexpr bool LOO = true, LSE = false, NQ_NULLABLE = true, MAY_BE_EMPTY = true;
};
template <bool LSE_>
struct MkWeighted : MkPlain {
  static constexpr bool WGT = true, LSE = LSE_, NQ_NULLABLE = true, MAY_BE_EMPTY = true;
  const float* W;
  int n_ctx_tasks;
  __device__ __forceinline__ int key_task(int b) const { return b % n_ctx_tasks; }
  __device__ __forceinline__ int query_task(int b) const { return b % n_ctx_tasks; }
};

// One workgroup = one task and 64 queries (16 per wave); DP = the tile width the instance computes on (d <= DP).
// NQ: the task's queries beyond n_q_valid[b] are padding (zeros out, never read); without it (and without R::NQ_NULLABLE) n_q_valid
// is not looked at.  R: the key rule.  lse is looked at iff R::LSE.
template <int DP, bool NQ, class R>
__global__ __launch_bounds__(256) void masked_attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ V, const int32_t* __restrict__ n_valid,
                                                             const int32_t* __restrict__ n_q_valid, float* __restrict__ O,
                                                             float* __restrict__ lse, int n_keys, int T, int Fp, int d, float scale,
                                                             const R r) {
  using G = MkGeom<DP>;
  constexpr int KB = G::KB, NSB = G::NSB, NKC = G::NKC, NDT = G::NDT, LDK = G::LDA, LDV = G::LDB;
  constexpr int SEG = MK_SEG<NKC>;
  __shared__ __attribute__((aligned(16))) float Ks[KB * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KB * LDV];
  [[maybe_unused]] float* Lw = nullptr;  // log w of the block's keys
  [[maybe_unused]] const float* wrow = nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int qblocks = (T + 63) >> 6;
  const int qb = blockIdx.x % qblocks, b = blockIdx.x / qblocks;
  const int tilesC0 = (n_keys + 31) >> 5, tilesT = (T + 31) >> 5;
  const int bp = r.key_task(b), bq = r.query_task(b);
  const int nv0 = clamp_count(n_valid, bp, n_keys);
  const int nv1 = r.tail_count(b);  // (both uniform over the workgroup)
  const bool counted = R::NQ_NULLABLE ? n_q_valid != nullptr : NQ;
  const int nq = counted ? clamp_count(n_q_valid, bq, T) : T;
  const bool has_lse = R::LSE && (R::WGT || lse != nullptr);
  if constexpr (R::WGT) {
    __shared__ __attribute__((aligned(16))) float Lw_[KB];
    Lw = Lw_;
    wrow = r.W + (size_t)b * n_keys;
  }
  const int own0 = qb * 64 + wave * 16;  // the wave's queries, and (LOO) the key sub-block that holds their own rows
  const int q = own0 + c;
  if ((NQ || R::NQ_NULLABLE) && qb * 64 >= nq) {  // (uniform over the workgroup, ahead of every barrier) all 64 queries are padding:
    mk_store_row<NDT>(O, b, tilesT, Fp, q, g, nullptr, 0.f, false);  // zeros, no key staged
    if (q < T && g == 0 && has_lse) lse[(size_t)b * T + q] = 0.f;
    return;
  }
  const bool live = q < nq;
  float Qq[NKC];  // the lane's query as an operand: Q[q][4 kc + g]
  mk_load_row<NKC>(Q, bq, tilesT, Fp, d, q, g, live, Qq);
  f32x4 o[NDT];  // O^T[dv = 16 dt + 4 g + i][q = c], not yet divided by l
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
#pragma unroll 1
  for (int seg = 0; seg < (R::PFX ? 2 : 1); ++seg) {  // (one segment without PFX: the loop is gone)
    const bool tail = R::PFX && seg == 1;
    const float* __restrict__ Kg = tail ? r.K2 : K;
    const float* __restrict__ Vg = tail ? r.V2 : V;
    const int tilesC = tail ? (r.n_keys2 + 31) >> 5 : tilesC0;
    const int bk = tail ? b : bp;  // the task whose rows the segment reads
    const int nv = tail ? nv1 : nv0;
    for (int key0 = 0; key0 < nv; key0 += KB) {
      __syncthreads();
      if constexpr (R::WGT) {
        mk_stage_weighted<DP, KB, LDK, LDV>(Kg, Vg, wrow, bk, tilesC, Fp, d, key0, nv, Ks, Vs, tid);
        mk_stage_logw<KB>(wrow, key0, nv, Lw, tid);
      } else {
        mk_stage<DP, KB, LDK>(Kg, bk, tilesC, Fp, d, key0, nv, Ks, tid);
        mk_stage<DP, KB, LDV>(Vg, bk, tilesC, Fp, d, key0, nv, Vs, tid);
      }
      __syncthreads();
      f32x4 S[NSB];  // S^T[key = key0 + 16 sb + 4 g + i][q = c]
      float bm = -INFINITY;
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};  // (one segment, SEG = NKC: one chain)
#pragma unroll
        for (int k0 = 0; k0 < NKC; k0 += SEG) {
          f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kc = k0; kc < k0 + SEG; ++kc) part = mk_mfma(Ks[(16 * sb + c) * LDK + 4 * kc + g], Qq[kc], part);
          acc = k0 == 0 ? part : acc + part;
        }
        [[maybe_unused]] f32x4 lw;
        if constexpr (R::WGT) lw = *(const f32x4*)(Lw + 16 * sb + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = key0 + 16 * sb + 4 * g + i;
          if constexpr (R::WGT)
            acc[i] = lw[i] > -INFINITY ? acc[i] * scale + lw[i] : -INFINITY;  // (beyond the count, and the keys without weight)
          else
            acc[i] = (key < nv && !(R::LOO && key == q)) ? acc[i] * scale : -INFINITY;  // (beyond the count; LOO: the own row)
          bm = fmaxf(bm, acc[i]);
        }
        S[sb] = acc;
      }
      // (key0 < nv: the block has a real key, so its maximum is finite -- unless R::MAY_BE_EMPTY: then it, and the running one, can
      // be -inf here, and the exponentials are taken against 0)
      const float m_new = fmaxf(m, mk_max4(bm));
      const float m_ref = (R::MAY_BE_EMPTY && m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = expf(m - m_ref);  // (0 while m = -inf; 1 where the block holds nothing for the query)
      float ps = 0.f;
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          S[sb][i] = expf(S[sb][i] - m_ref);  // (exp(-inf) = 0 for a key the query does not attend over)
          ps += S[sb][i];
        }
      l = l * alpha + mk_sum4(ps);
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        if (R::LOO && key0 + 16 * sb == own0) {  // (uniform over the wave)
          mk_pv_own_rows<NDT, LDV>(Vs + 16 * sb * LDV, S[sb], c, g, o);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[dt] = mk_mfma(Vs[(16 * sb + 4 * g + j) * LDV + 16 * dt + c], S[sb][j], o[dt]);
        }
      }
    }
  }
  const bool filled = live && l > 0.f;  // (no key to attend over, a query beyond the count, the tile's rows beyond T: zeros)
  const float inv = filled ? 1.f / l : 0.f;
  // (MAY_BE_EMPTY: a row that is not filled as zeros; else as accumulator * 0 -- each rule's form is its behaviour where a dead
  // row's accumulator is not finite)
  mk_store_row<NDT>(O, b, tilesT, Fp, q, g, o, inv, !R::MAY_BE_EMPTY || filled);
  if (q < T && g == 0 && has_lse)
    lse[(size_t)b * T + q] = (R::MAY_BE_EMPTY ? filled : live && nv0 + nv1 > 0) ? m + logf(l) : 0.f;
}

// d_q: the forward pass's geometry.  dS^T = scale P^T (dP^T - D), P from the log-sum-exp, D[q] = <dO[q], O[q]>.
// WGT: the weighted rule at one replicate (W, else not looked at); whether there is a query count is the null check of n_q_valid then.
template <int DP, bool NQ, bool WGT>
__global__ __launch_bounds__(256) void masked_attn_dq_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                            const float* __restrict__ V, const float* __restrict__ W,
                                                            const int32_t* __restrict__ n_valid,
                                                            const int32_t* __restrict__ n_q_valid, const float* __restrict__ O,
                                                            const float* __restrict__ dO, const float* __restrict__ lse,
                                                            float* __restrict__ dQ, int n_keys, int T, int Fp, int d, float scale) {
  using G = MkGeom<DP>;
  constexpr int KB = G::KB, NSB = G::NSB, NKC = G::NKC, NDT = G::NDT, LDK = G::LDA, LDV = G::LDA, SEG = MK_SEG<NKC>;
  __shared__ __attribute__((aligned(16))) float Ks[KB * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KB * LDV];
  [[maybe_unused]] float* Lw = nullptr;  // log w of the block's keys
  [[maybe_unused]] const float* wrow = nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int qblocks = (T + 63) >> 6;
  const int qb = blockIdx.x % qblocks, b = blockIdx.x / qblocks;
  const int tilesC = (n_keys + 31) >> 5, tilesT = (T + 31) >> 5;
  const int nv = clamp_count(n_valid, b, n_keys);
  const bool counted = WGT ? n_q_valid != nullptr : NQ;
  const int nq = counted ? clamp_count(n_q_valid, b, T) : T;
  if constexpr (WGT) {
    __shared__ __attribute__((aligned(16))) float Lw_[KB];
    Lw = Lw_;
    wrow = W + (size_t)b * n_keys;
  }
  const int q = qb * 64 + wave * 16 + c;
  if ((NQ || WGT) && qb * 64 >= nq) {  // (uniform over the workgroup, ahead of every barrier) all 64 queries are padding: zero d_q rows
    mk_store_row<NDT>(dQ, b, tilesT, Fp, q, g, nullptr, 0.f, false);
    return;
  }
  const bool live = q < nq;
  float Qq[NKC], Gq[NKC];
  // D as the diagonal of O dO^T on the matrix unit, i.e. summed in the order dP^T = V dO^T is: where one key takes all the weight
  // (O = that key's V) the difference dP - D then cancels exactly instead of to the rounding of two differently ordered sums
  f32x4 dd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) {
    const bool ok = live && 4 * kc < d;
    const size_t at = mk_pt(b, tilesT, Fp, ok ? q : 0, ok ? 4 * kc : 0) + g;
    Qq[kc] = ok ? Q[at] : 0.f;
    Gq[kc] = ok ? dO[at] : 0.f;
    dd = mk_mfma(ok ? O[at] : 0.f, Gq[kc], dd);  // [row = query 4 g + i][column = query c]
  }
  // (row c of column c sits in the lane of group c / 4, element c % 4)
  const int e = c & 3;
  const float Dc = __shfl(e == 0 ? dd[0] : e == 1 ? dd[1] : e == 2 ? dd[2] : dd[3], c + 16 * (c >> 2));
  const float Lc = live ? lse[(size_t)b * T + q] : 0.f;
  f32x4 dq[NDT];  // dQ^T[f = 16 dt + 4 g + i][q = c]
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int key0 = 0; key0 < nv; key0 += KB) {
    __syncthreads();
    if constexpr (WGT) {
      mk_stage_weighted<DP, KB, LDK, LDV>(K, V, wrow, b, tilesC, Fp, d, key0, nv, Ks, Vs, tid);
      mk_stage_logw<KB>(wrow, key0, nv, Lw, tid);
    } else {
      mk_stage<DP, KB, LDK>(K, b, tilesC, Fp, d, key0, nv, Ks, tid);
      mk_stage<DP, KB, LDV>(V, b, tilesC, Fp, d, key0, nv, Vs, tid);
    }
    __syncthreads();
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < NKC; k0 += SEG) {  // (the score in the forward kernel's segments)
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = k0; kc < k0 + SEG; ++kc) {
          part = mk_mfma(Ks[(16 * sb + c) * LDK + 4 * kc + g], Qq[kc], part);
          dpt = mk_mfma(Vs[(16 * sb + c) * LDV + 4 * kc + g], Gq[kc], dpt);
        }
        st = k0 == 0 ? part : st + part;
      }
      [[maybe_unused]] f32x4 lw;
      if constexpr (WGT) lw = *(const f32x4*)(Lw + 16 * sb + 4 * g);
      f32x4 dst;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float p;  // (each rule its own expression: floating-point contraction fuses what is spelled as one)
        if constexpr (WGT)
          p = (live && lw[i] > -INFINITY) ? expf(st[i] * scale + lw[i] - Lc) : 0.f;
        else
          p = (live && key0 + 16 * sb + 4 * g + i < nv) ? expf(st[i] * scale - Lc) : 0.f;
        dst[i] = scale * p * (dpt[i] - Dc);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) dq[dt] = mk_mfma(Ks[(16 * sb + 4 * g + j) * LDK + 16 * dt + c], dst[j], dq[dt]);
    }
  }
  // (zeros where the task has no key to attend over, and in the tile's rows beyond T)
  mk_store_row<NDT>(dQ, b, tilesT, Fp, q, g, dq, 1.f, true);
}

// d_k / d_v: one workgroup = one task and 16 keys; its four waves take the 16-query blocks in turn, keep dK^T / dV^T of the 16 keys in
// registers and add them up through LDS.  Blocks beyond the count only store their zeros.  NQ: the walk over the queries ends at the
// task's query count (the kernel's cost is linear in the queries walked).
// WGT: the weighted rule at one replicate (W and dW, else not looked at; the query count as in the d_q kernel), which also adds up
// sum_q dA_qk of its 16 keys for d_w: per lane over the queries it walks, over the four lanes that share the key, then over the four
// waves in LDS in wave order -- a fixed order, no atomics.  Every row of d_k / d_v and every d_w[task][key < n_keys] is written.
template <int DP, bool NQ, bool WGT>
__global__ __launch_bounds__(256) void masked_attn_dkv_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ V, const float* __restrict__ W,
                                                             const int32_t* __restrict__ n_valid,
                                                             const int32_t* __restrict__ n_q_valid, const float* __restrict__ O,
                                                             const float* __restrict__ dO, const float* __restrict__ lse,
                                                             float* __restrict__ dK, float* __restrict__ dV, float* __restrict__ dW,
                                                             int n_keys, int T, int Fp, int d, float scale) {
  using G = MkGeom<DP>;
  constexpr int NKC = G::NKC, NDT = G::NDT, LD = G::LDA, SEG = MK_SEG<NKC>;
  __shared__ __attribute__((aligned(16))) float Ks[16 * LD];
  __shared__ __attribute__((aligned(16))) float Vs[16 * LD];
  __shared__ f32x4 red[3 * 64];
  [[maybe_unused]] float* redw = nullptr;  // sum_q dA of the 16 keys per wave
  [[maybe_unused]] const float* wrow = nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int tilesC = (n_keys + 31) >> 5, tilesT = (T + 31) >> 5;
  const int kblocks = 2 * tilesC;  // (whole tiles: every row of d_k / d_v is written)
  const int kb = blockIdx.x % kblocks, b = blockIdx.x / kblocks;
  const int nv = clamp_count(n_valid, b, n_keys);
  const bool counted = WGT ? n_q_valid != nullptr : NQ;
  const int nq = counted ? clamp_count(n_q_valid, b, T) : T;  // (uniform over the workgroup)
  const int key0 = 16 * kb;
  if constexpr (WGT) {
    __shared__ float redw_[4 * 16];
    redw = redw_;
    wrow = W + (size_t)b * n_keys;
  }
  if (key0 >= nv) {  // (uniform over the workgroup)
    for (int i = tid; i < 16 * (Fp >> 2); i += 256) {
      const size_t at = mk_pt(b, tilesC, Fp, key0 + (i & 15), 4 * (i >> 4));
      *(f32x4*)(dK + at) = f32x4{0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(dV + at) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (WGT)
      if (tid < 16 && key0 + tid < n_keys) dW[(size_t)b * n_keys + key0 + tid] = 0.f;
    return;
  }
  if constexpr (WGT) {
    mk_stage_weighted<DP, 16, LD, LD>(K, V, wrow, b, tilesC, Fp, d, key0, nv, Ks, Vs, tid);
  } else {
    mk_stage<DP, 16, LD>(K, b, tilesC, Fp, d, key0, nv, Ks, tid);
    mk_stage<DP, 16, LD>(V, b, tilesC, Fp, d, key0, nv, Vs, tid);
  }
  __syncthreads();
  f32x4 aK[NDT], aV[NDT];  // dK^T / dV^T [f = 16 dt + 4 g + i][key = key0 + c]
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) aK[dt] = aV[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool key_ok = key0 + c < nv;
  [[maybe_unused]] float wc = 0.f, lwc = 0.f;  // the weight of the lane's key and its log
  [[maybe_unused]] float aW = 0.f;  // sum_q dA[q][key = key0 + c] over the queries 4 g + i of the blocks the wave walks
  if constexpr (WGT) {
    wc = key_ok ? wrow[key0 + c] : 0.f;
    key_ok = wc > 0.f && wc < INFINITY;  // (NaN fails both comparisons)
    lwc = key_ok ? logf(wc) : 0.f;
  }
  for (int q0 = wave * 16; q0 < nq; q0 += 64) {
    const int q = q0 + c;
    const bool live = q < nq;
    // S[q = q0 + 4 g + i][key = c] and dP alike; D and the log-sum-exp of the lane's query c on the way
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
    f32x4 dd = {0.f, 0.f, 0.f, 0.f};  // dO O^T [row = query 4 g + i][column = query c]: D on its diagonal, summed as dP is
#pragma unroll
    for (int k0 = 0; k0 < NKC; k0 += SEG) {  // (the score in the forward kernel's segments)
      f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = k0; kc < k0 + SEG; ++kc) {
        const bool ok = live && 4 * kc < d;
        const size_t at = mk_pt(b, tilesT, Fp, ok ? q : 0, ok ? 4 * kc : 0) + g;
        const float qv = ok ? Q[at] : 0.f, gv = ok ? dO[at] : 0.f;
        dd = mk_mfma(gv, ok ? O[at] : 0.f, dd);
        part = mk_mfma(qv, Ks[c * LD + 4 * kc + g], part);
        dp = mk_mfma(gv, Vs[c * LD + 4 * kc + g], dp);
      }
      s = k0 == 0 ? part : s + part;
    }
    const float Lc = live ? lse[(size_t)b * T + q] : 0.f;
    f32x4 pr, ds;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (row 4 g + i of column 4 g + i: element i of the lane of this group whose column is 4 g + i; lane 4 g + i holds query
      // q0 + 4 g + i as its column)
      const float Di = __shfl(dd[i], 20 * g + i), Li = __shfl(Lc, 4 * g + i);
      const bool on = key_ok && q0 + 4 * g + i < nq;
      // (each rule its own expressions: floating-point contraction fuses what is spelled as one)
      if constexpr (WGT) {
        pr[i] = on ? expf(s[i] * scale + lwc - Li) : 0.f;
        const float da = pr[i] * (dp[i] - Di);
        aW += da;
        ds[i] = scale * da;
      } else {
        pr[i] = on ? expf(s[i] * scale - Li) : 0.f;
        ds[i] = scale * pr[i] * (dp[i] - Di);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qj = q0 + 4 * g + j;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int f = 16 * dt + c;
        const bool ok = qj < nq && f < d;
        const size_t at = mk_pt(b, tilesT, Fp, ok ? qj : 0, ok ? (f & ~3) : 0) + (f & 3);
        aV[dt] = mk_mfma(ok ? dO[at] : 0.f, pr[j], aV[dt]);  // A[row = f][k = query 4 g + j]
        aK[dt] = mk_mfma(ok ? Q[at] : 0.f, ds[j], aK[dt]);
      }
    }
  }
  if constexpr (WGT) {
    aW = mk_sum4(aW);  // (every lane of key c holds the wave's sum)
    if (g == 0) redw[wave * 16 + c] = aW;
  }
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const f32x4 mine = pass == 0 ? aK[dt] : aV[dt];
      __syncthreads();
      if (wave > 0) red[(wave - 1) * 64 + lane] = mine;
      __syncthreads();
      if (wave == 0 && 16 * dt + 4 * g < Fp) {
        f32x4 t = mine;
#pragma unroll
        for (int w = 0; w < 3; ++w) t += red[w * 64 + lane];
        if (!key_ok) t = f32x4{0.f, 0.f, 0.f, 0.f};
        *(f32x4*)((pass == 0 ? dK : dV) + mk_pt(b, tilesC, Fp, key0 + c, 16 * dt + 4 * g)) = t;
      }
    }
  }
  if constexpr (WGT) {  // (redw was written ahead of the barriers above)
    if (tid < 16 && key0 + tid < n_keys) {
      const float t = ((redw[tid] + redw[16 + tid]) + redw[32 + tid]) + redw[48 + tid];
      dW[(size_t)b * n_keys + key0 + tid] = key_ok ? t / wc : 0.f;  // (tid < 16: the lane's key c is key0 + tid)
    }
  }
}

}  // namespace npf

static bool mk_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) != 0;
}

static int masked_attn_check(const void* q, const void* k, const void* v, const void* n_valid, int32_t n_tasks, int32_t n_keys,
                             int32_t n_queries, int32_t d) {
  if (n_tasks < 0 || n_keys < 0 || n_queries < 0 || d <= 0 || (d & 3) || d > 256) return NPF_EINVAL;
  if (!q || !n_valid || (n_keys > 0 && (!k || !v)) || mk_misaligned(q, k, v)) return NPF_EINVAL;
  return NPF_OK;
}

// One launch of `blocks` workgroups on the stream: launch(width, flag, grid, block, stream, Fp) gets the tile width of d (32, 64,
// 128 or 256) and the flag as std::integral_constant values, to name the kernel instance with.
template <class F>
static int mk_launch(int32_t d, bool flag, unsigned blocks, void* stream, F&& launch) {
  const int Fp = npf::round_up(d, 32);
  const dim3 grid(blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  auto at_width = [&](auto fl) {
    if (d <= 32)
      launch(std::integral_constant<int, 32>{}, fl, grid, block, st, Fp);
    else if (d <= 64)
      launch(std::integral_constant<int, 64>{}, fl, grid, block, st, Fp);
    else if (d <= 128)
      launch(std::integral_constant<int, 128>{}, fl, grid, block, st, Fp);
    else
      launch(std::integral_constant<int, 256>{}, fl, grid, block, st, Fp);
  };
  if (flag)
    at_width(std::true_type{});
  else
    at_width(std::false_type{});
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}
static unsigned mk_query_blocks(int32_t n_tasks, int32_t n_queries) { return (unsigned)n_tasks * ((n_queries + 63) / 64); }
static unsigned mk_key_blocks(int32_t n_tasks, int32_t n_keys) { return (unsigned)n_tasks * (2 * ((n_keys + 31) / 32)); }


// The forward kernel under key rule r.  nq: n_q_valid is given, for the rules that take it as the kernel's NQ flag
template <class R>
static int masked_attn_fwd_launch(const float* q, const float* k, const float* v, const int32_t* n_valid, const int32_t* n_q_valid,
                                  int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* out, float* lse,
                                  void* stream, const R r) {
  if (n_tasks == 0 || n_queries == 0) return NPF_OK;
  return mk_launch(d, n_q_valid != nullptr && !R::NQ_NULLABLE, mk_query_blocks(n_tasks, n_queries), stream,
                   [&](auto dp, auto nq, dim3 grid, dim3 block, hipStream_t st, int Fp) {
                     constexpr bool NQ = decltype(nq)::value && !R::NQ_NULLABLE;  // (one instance per width for such a rule)
                     hipLaunchKernelGGL((npf::masked_attn_fwd_kernel<decltype(dp)::value, NQ, R>), grid, block, 0, st, q, k, v, n_valid,
                                        n_q_valid, out, lse, n_keys, n_queries, Fp, d, scale, r);
                   });
}

// The two backward kernels under the plain (w, d_w null) or the weighted rule
template <bool WGT>
static int masked_attn_bwd_launch(const float* q, const float* k, const float* v, const float* w, const int32_t* n_valid,
                                  const int32_t* n_q_valid, const float* out, const float* d_out, const float* lse, int32_t n_tasks,
                                  int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* d_q, float* d_k, float* d_v,
                                  float* d_w, void* stream) {
  if (n_tasks == 0) return NPF_OK;
  const bool nq_flag = n_q_valid != nullptr && !WGT;
  if (n_queries > 0) {
    const int rc = mk_launch(d, nq_flag, mk_query_blocks(n_tasks, n_queries), stream,
                             [&](auto dp, auto nq, dim3 grid, dim3 block, hipStream_t st, int Fp) {
                               constexpr bool NQ = decltype(nq)::value && !WGT;  // (one instance per width under WGT)
                               hipLaunchKernelGGL((npf::masked_attn_dq_kernel<decltype(dp)::value, NQ, WGT>), grid, block, 0, st, q, k,
                                                  v, w, n_valid, n_q_valid, out, d_out, lse, d_q, n_keys, n_queries, Fp, d, scale);
                             });
    if (rc != NPF_OK) return rc;
  }
  if (n_keys == 0) return NPF_OK;  // (no queries: the walk over them is empty and the kernel stores the zeros)
  return mk_launch(d, nq_flag, mk_key_blocks(n_tasks, n_keys), stream,
                   [&](auto dp, auto nq, dim3 grid, dim3 block, hipStream_t st, int Fp) {
                     constexpr bool NQ = decltype(nq)::value && !WGT;
                     hipLaunchKernelGGL((npf::masked_attn_dkv_kernel<decltype(dp)::value, NQ, WGT>), grid, block, 0, st, q, k, v, w,
                                        n_valid, n_q_valid, out, d_out, lse, d_k, d_v, d_w, n_keys, n_queries, Fp, d, scale);
                   });
}

static int masked_attn_fwd(const float* q, const float* k, const float* v, const int32_t* n_valid, const int32_t* n_q_valid,
                           int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* out, float* lse,
                           void* stream) {
  const int rc = masked_attn_check(q, k, v, n_valid, n_tasks, n_keys, n_queries, d);
  if (rc != NPF_OK) return rc;
  if (!out || mk_misaligned(out)) return NPF_EINVAL;
  return masked_attn_fwd_launch(q, k, v, n_valid, n_q_valid, n_tasks, n_keys, n_queries, d, scale, out, lse, stream, npf::MkPlain{});
}

static int masked_attn_bwd(const float* q, const float* k, const float* v, const int32_t* n_valid, const int32_t* n_q_valid,
                           const float* out, const float* d_out, const float* lse, int32_t n_tasks, int32_t n_keys,
                           int32_t n_queries, int32_t d, float scale, float* d_q, float* d_k, float* d_v, void* stream) {
  const int rc = masked_attn_check(q, k, v, n_valid, n_tasks, n_keys, n_queries, d);
  if (rc != NPF_OK) return rc;
  if (!out || !d_out || !lse || !d_q || (n_keys > 0 && (!d_k || !d_v))) return NPF_EINVAL;
  if (mk_misaligned(out, d_out, d_q) || mk_misaligned(d_k, d_v)) return NPF_EINVAL;
  return masked_attn_bwd_launch<false>(q, k, v, nullptr, n_valid, n_q_valid, out, d_out, lse, n_tasks, n_keys, n_queries, d, scale, d_q,
                                       d_k, d_v, nullptr, stream);
}

extern "C" int npf_masked_attn_fwd(const float* q, const float* k, const float* v, const int32_t* n_valid, int32_t n_tasks,
                                   int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* out, float* lse, void* stream) {
  return masked_attn_fwd(q, k, v, n_valid, nullptr, n_tasks, n_keys, n_queries, d, scale, out, lse, stream);
}

extern "C" int npf_masked_attn_bwd(const float* q, const float* k, const float* v, const int32_t* n_valid, const float* out,
                                   const float* d_out, const float* lse, int32_t n_tasks, int32_t n_keys, int32_t n_queries,
                                   int32_t d, float scale, float* d_q, float* d_k, float* d_v, void* stream) {
  return masked_attn_bwd(q, k, v, n_valid, nullptr, out, d_out, lse, n_tasks, n_keys, n_queries, d, scale, d_q, d_k, d_v, stream);
}

extern "C" int npf_masked_attn_fwd_nq(const float* q, const float* k, const float* v, const int32_t* n_valid,
                                      const int32_t* n_q_valid, int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d,
                                      float scale, float* out, float* lse, void* stream) {
  if (!n_q_valid) return NPF_EINVAL;
  return masked_attn_fwd(q, k, v, n_valid, n_q_valid, n_tasks, n_keys, n_queries, d, scale, out, lse, stream);
}

extern "C" int npf_masked_attn_bwd_nq(const float* q, const float* k, const float* v, const int32_t* n_valid,
                                      const int32_t* n_q_valid, const float* out, const float* d_out, const float* lse,
                                      int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* d_q,
                                      float* d_k, float* d_v, void* stream) {
  if (!n_q_valid) return NPF_EINVAL;
  return masked_attn_bwd(q, k, v, n_valid, n_q_valid, out, d_out, lse, n_tasks, n_keys, n_queries, d, scale, d_q, d_k, d_v, stream);
}

extern "C" int npf_masked_attn_fwd_prefix(const float* q, const float* k_pre, const float* v_pre, const int32_t* n_prefix,
                                          const float* k_tail, const float* v_tail, const int32_t* n_tail, const int32_t* n_q_valid,
                                          int32_t n_tasks, int32_t n_prefix_tasks, int32_t c_pad, int32_t m_tail, int32_t n_queries,
                                          int32_t d, float scale, float* out, void* stream) {
  if (n_tasks < 0 || n_prefix_tasks <= 0 || n_tasks % n_prefix_tasks != 0 || c_pad < 0 || m_tail < 0 || n_queries < 0) return NPF_EINVAL;
  if (d <= 0 || (d & 3) || d > 256) return NPF_EINVAL;
  if (!q || !out || !n_prefix || !n_tail || (c_pad > 0 && (!k_pre || !v_pre)) || (m_tail > 0 && (!k_tail || !v_tail))) return NPF_EINVAL;
  if (mk_misaligned(q, k_pre, v_pre, out) || mk_misaligned(k_tail, v_tail)) return NPF_EINVAL;
  return masked_attn_fwd_launch(q, k_pre, v_pre, n_prefix, n_q_valid, n_tasks, c_pad, n_queries, d, scale, out, nullptr, stream,
                                npf::MkPrefix{{}, k_tail, v_tail, n_tail, m_tail, n_prefix_tasks});
}

extern "C" int npf_masked_attn_fwd_loo(const float* q, const float* k, const float* v, const int32_t* n_valid,
                                       const int32_t* n_q_valid, int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d,
                                       float scale, float* out, void* stream) {
  const int rc = masked_attn_check(q, k, v, n_valid, n_tasks, n_keys, n_queries, d);
  if (rc != NPF_OK) return rc;
  if (!out || mk_misaligned(out)) return NPF_EINVAL;
  return masked_attn_fwd_launch(q, k, v, n_valid, n_q_valid, n_tasks, n_keys, n_queries, d, scale, out, nullptr, stream, npf::MkLoo{});
}

static int masked_attn_fwd_weighted(const float* q, const float* k, const float* v, const float* w, const int32_t* n_valid,
                                    const int32_t* n_q_valid, int32_t n_tasks, int32_t n_ctx_tasks, int32_t n_keys,
                                    int32_t n_queries, int32_t d, float scale, float* out, float* lse, void* stream) {
  if (n_ctx_tasks <= 0 || n_tasks < 0 || n_tasks % n_ctx_tasks != 0) return NPF_EINVAL;
  const int rc = masked_attn_check(q, k, v, n_valid, n_tasks, n_keys, n_queries, d);
  if (rc != NPF_OK) return rc;
  if (!out || mk_misaligned(out) || (n_keys > 0 && !w) || (((uintptr_t)w) & 3) || (((uintptr_t)lse) & 3)) return NPF_EINVAL;
  if (lse)
    return masked_attn_fwd_launch(q, k, v, n_valid, n_q_valid, n_tasks, n_keys, n_queries, d, scale, out, lse, stream,
                                  npf::MkWeighted<true>{{}, w, n_ctx_tasks});
  return masked_attn_fwd_launch(q, k, v, n_valid, n_q_valid, n_tasks, n_keys, n_queries, d, scale, out, lse, stream,
                                npf::MkWeighted<false>{{}, w, n_ctx_tasks});
}

extern "C" int npf_masked_attn_fwd_weighted(const float* q, const float* k, const float* v, const float* w, const int32_t* n_valid,
                                            const int32_t* n_q_valid, int32_t n_tasks, int32_t n_ctx_tasks, int32_t n_keys,
                                            int32_t n_queries, int32_t d, float scale, float* out, void* stream) {
  return masked_attn_fwd_weighted(q, k, v, w, n_valid, n_q_valid, n_tasks, n_ctx_tasks, n_keys, n_queries, d, scale, out, nullptr, stream);
}

extern "C" int npf_masked_attn_fwd_weighted_ex(const float* q, const float* k, const float* v, const float* w, const int32_t* n_valid,
                                               const int32_t* n_q_valid, int32_t n_tasks, int32_t n_ctx_tasks, int32_t n_keys,
                                               int32_t n_queries, int32_t d, float scale, float* out, float* lse, void* stream) {
  if (!lse) return NPF_EINVAL;
  return masked_attn_fwd_weighted(q, k, v, w, n_valid, n_q_valid, n_tasks, n_ctx_tasks, n_keys, n_queries, d, scale, out, lse, stream);
}

extern "C" int npf_masked_attn_bwd_weighted(const float* q, const float* k, const float* v, const float* w, const int32_t* n_valid,
                                            const int32_t* n_q_valid, const float* out, const float* d_out, const float* lse,
                                            int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float* d_q,
                                            float* d_k, float* d_v, float* d_w, void* stream) {
  const int rc = masked_attn_check(q, k, v, n_valid, n_tasks, n_keys, n_queries, d);
  if (rc != NPF_OK) return rc;
  if (!out || !d_out || !lse || !d_q || (n_keys > 0 && (!w || !d_k || !d_v || !d_w))) return NPF_EINVAL;
  if (mk_misaligned(out, d_out, d_q) || mk_misaligned(d_k, d_v)) return NPF_EINVAL;
  if ((((uintptr_t)w) | ((uintptr_t)d_w) | ((uintptr_t)lse)) & 3) return NPF_EINVAL;
  return masked_attn_bwd_launch<true>(q, k, v, w, n_valid, n_q_valid, out, d_out, lse, n_tasks, n_keys, n_queries, d, scale, d_q, d_k,
                                      d_v, d_w, stream);
}
