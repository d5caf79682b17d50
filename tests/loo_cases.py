"""Inputs and references of the leave-one-out edge tests (tests/test_hip_loo_edges.py, checked on the CPU by
tests/test_loo_cases_host.py): ``npf_masked_attn_fwd_loo`` (csrc/masked_kernels.hip) and ``npf_loo_mean`` (csrc/layout_kernels.hip).
Pure torch on the CPU, seeded; nothing here imports the package.

Attention.  The eight regimes of tests/masked_cases.py with T = C_pad (query row i and key row i are rows i of the same task), V
with the per-task factors of ``masked_cases.scale_per_task``, the padding rows scoring 30 above the task's maximum.  Under the
exclusion they mean something new: the ``one_key@...`` tasks have ONE query that loses the dominant key and sees the flat rest,
the last valid query of ``ascending`` and the argmax query of ``huge_pos`` exclude their row's maximum.  One more regime,
``own_dominant``: Q = 3 g d^0.25 x / |x| with x random rows and K = Q + 0.3 noise, so a row's own score is g^2 * 9 and every other
score is a random projection of it.  The host test asserts own - max(other) >= OWN_GAP = 110 on every valid row: a kernel that let
the own score into its running maximum would give every other key the weight exp(-gap), and fp32's exp is an exact zero past 104.
Gains per width and what they reach on the inputs of the test (8 tasks of up to 200 rows; smallest gap / largest own score):

    d = 32: g = 6.5 (134.9 / 389)    d = 64: g = 5.5 (145.0 / 277)    d = 128: g = 4.8 (132.0 / 211)    d = 256: g = 4.4 (125.5 / 177)

(with g = 4 at every width the smallest gaps were 47, 64, 83 and 105).  On these inputs the float64 formula evaluated in fp32 errs by
2e-6 ... 9e-6 of a task's max|ref|: scores of a few hundred carry an absolute rounding of a few 1e-5, which exp turns into a relative one.

Random directions in 4, 16 or 20 dimensions come too close to each other for 200 rows: the builder refuses d < 32.

Mean.  ``random``; ``outlier@1e3 / @1e5 / @1e7``: one valid row per task times that factor, at row 0, n - 1, 31 or 32 (whichever the
count allows, rotating over the tasks); ``offset``: every entry + 1000; ``mixed_sign_cancel``: the last valid row is minus the sum of
the others, so the per-task sum is a rounding residue.  Three evaluations: float64, the direct fp32 one (sum over the others, one
division) and ``(s - r_i) / (n - 1)`` with ``s`` the fp32 sum of all rows -- the formula ``loo_mean_kernel`` had, whose result for an
outlying row is what an fp32 sum has left of the others."""
import math

import torch

import masked_cases as MC

# ---- attention -----------------------------------------------------------------------------------------------------------------
ATTN_REGIMES = MC.REGIMES + ("own_dominant",)
C_PAD = 200  # four query workgroups; seven 32-key blocks, thirteen 16-key blocks
COUNTS = (200, 129, 128, 65, 64, 33, 17, 2)
WIDTHS = (16, 20, 64, 128, 256)
OWN_MIN_WIDTH, OWN_GAP = 32, 110.0
OWN_GAIN = {32: 6.5, 64: 5.5, 128: 4.8, 256: 4.4}
OWN_NOISE = 0.3
# query counts: None, the key counts, and "crossed" -- below the key count (0, 16 and 64 among them) and above it (up to C_pad)
Q_COUNTS = {"none": None, "same": COUNTS, "crossed": (64, 200, 0, 16, 130, 32, 81, 1)}


def regime_runs(regime, d):
    return regime != "own_dominant" or d >= OWN_MIN_WIDTH


def own_gain(d):
    """The gain of the largest listed width up to ``d`` (at a fixed gain the gap grows with the width)."""
    if d < OWN_MIN_WIDTH:
        raise ValueError(f"own_dominant needs d >= {OWN_MIN_WIDTH}: random directions in {d} dimensions do not reach a gap of {OWN_GAP}")
    return OWN_GAIN[max(w for w in OWN_GAIN if w <= d)]


def attn_seed(regime, d):
    return 1000 * ATTN_REGIMES.index(regime) + d


def attn_case(regime, d, counts=COUNTS, C_pad=C_PAD):
    """fp32 (Q, K, V), each [B, C_pad, d]."""
    gen = torch.Generator().manual_seed(attn_seed(regime, d))
    if regime == "own_dominant":
        g = own_gain(d)
        B = len(counts)
        x, noise, V = (torch.randn(B, C_pad, d, generator=gen, dtype=torch.float64) for _ in range(3))
        Q = 3.0 * g * d ** 0.25 * x / x.norm(dim=-1, keepdim=True)
        Q, K, V = Q.float(), (Q + OWN_NOISE * noise).float(), V.float()
    else:
        Q, K, V = MC.build(regime, counts, C_pad, C_pad, d, MC.key_block(d), gen)
    (V,) = MC.scale_per_task(V)
    return Q, K, V


def loo_scores64(Q, K, b, n, d):
    """float64 (S [C_pad, n], own [min(C_pad, n)]): the scaled scores of every query row of task ``b`` over its valid keys."""
    S = MC.scores64(Q, K, b, n, d)
    return S, S[:n].diagonal().clone()


def special_row(regime, S, n, KB):
    """The query of a task (``n`` >= 2 valid keys, float64 scores ``S``) whose own key is the one its row would be dominated by:
    the dominant key of ``one_key@...``, the last valid row of ``ascending``, the key built at 100.0 of ``huge_pos``; else None."""
    if regime.startswith("one_key@"):
        return MC.one_key_index(regime, n, KB)
    if regime == "ascending":
        return n - 1
    if regime == "huge_pos":
        return int(S[:n].mean(0).argmax())
    return None


def special_rows(regime, Q, K, counts, d):
    """[(task, query row)] over the tasks with at least two valid keys."""
    KB, rows = MC.key_block(d), []
    for b, n in enumerate(counts):
        if n >= 2:
            j = special_row(regime, MC.scores64(Q, K, b, n, d), n, KB)
            if j is not None:
                rows.append((b, j))
    return rows


def loo_attention(Q, K, V, counts, q_counts, scale, dtype):
    """[B, C_pad, d] in ``dtype``: row q < min(n_q, n) of a task is the softmax over the task's n valid keys WITHOUT key q; a row
    n <= q < n_q has no own key among the valid ones and attends over all n; exact zeros beyond n_q and where a row is left no key
    (n = 0; n = 1 and q = 0).  ``q_counts`` None: every row is a query."""
    out = torch.zeros_like(Q, dtype=dtype)
    C = Q.shape[1]
    for b, n in enumerate(counts):
        nq = C if q_counts is None else q_counts[b]
        if n == 0 or nq == 0:
            continue
        q, k, v = Q[b, :nq].to(dtype), K[b, :n].to(dtype), V[b, :n].to(dtype)
        S = q @ k.T * scale
        m = min(nq, n)
        S[:m].diagonal().fill_(-math.inf)
        if n == 1:  # (row 0 is left no key: zeros, not the NaN of a softmax over nothing)
            S[0, 0] = 0.0
        P = torch.softmax(S, dim=-1)
        if n == 1:
            P[0] = 0.0
        out[b, :nq] = P @ v
    return out


def plain_attention(Q, K, V, counts, scale, dtype):
    """[B, C_pad, d]: every row of a task attends over all of its valid keys (``functional.masked_attention``); zeros for n = 0."""
    out = torch.zeros_like(Q, dtype=dtype)
    for b, n in enumerate(counts):
        if n:
            out[b] = torch.softmax(Q[b].to(dtype) @ K[b, :n].to(dtype).T * scale, dim=-1) @ V[b, :n].to(dtype)
    return out


def emulate_loo_kernel(Q, K, V, counts, q_counts, d, slip=None):
    """The walk of ``masked_attn_fwd_kernel`` under the ``MkLoo`` rule in fp32 torch: key blocks of ``key_block(d)``, running maximum m and sum l per
    query, the exponentials against ``m_ref`` (0 while m is -inf), the accumulator rescaled by exp(m_old - m_ref), zeros where
    l = 0.  ``slip`` puts one mistake into the walk (never into a kernel):
      ``own_in_max``     the own score is taken out of the probabilities but still enters the running maximum;
      ``own_kept``       the own key is not excluded at all;
      ``pad_excluded``   rows at and beyond the key count are treated as having no key (zeros) instead of attending over all n;
      ``wrong_subblock`` the own row is looked for one 16-row sub-block further on (key q + 16 is excluded in place of key q)."""
    KB, scale = MC.key_block(d), 1.0 / math.sqrt(d)
    out = torch.zeros_like(Q)
    C = Q.shape[1]
    rows = torch.arange(C).view(-1, 1)
    for b, n in enumerate(counts):
        nq = C if q_counts is None else q_counts[b]
        q = Q[b]
        m, l, o = torch.full((C,), -math.inf), torch.zeros(C), torch.zeros(C, Q.shape[2])
        for key0 in range(0, n, KB):
            keys = torch.arange(key0, min(key0 + KB, n)).view(1, -1)
            S = q @ K[b, key0:key0 + keys.shape[1]].T * scale
            own = keys == (rows + 16 if slip == "wrong_subblock" else rows)
            if slip == "own_kept":
                own = torch.zeros_like(own)
            Sx = S.masked_fill(own, -math.inf)
            m_new = torch.maximum(m, (S if slip == "own_in_max" else Sx).max(-1).values)
            m_ref = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
            alpha = torch.exp(m - m_ref)
            P = torch.exp(Sx - m_ref.unsqueeze(-1))
            l = l * alpha + P.sum(-1)
            o = o * alpha.unsqueeze(-1) + P @ V[b, key0:key0 + keys.shape[1]]
            m = m_new
        live = (rows.view(-1) < nq) & (l > 0)
        if slip == "pad_excluded":
            live = live & (rows.view(-1) < n)
        out[b] = torch.where(live.unsqueeze(-1), o / l.clamp(min=1e-38).unsqueeze(-1), torch.zeros_like(o))
    return out


def task_gate(ref64, ref32, b, tol):
    """The gate of ``assert_gated_per_task`` (tests/test_hip_masked_edges.py) for task ``b``."""
    ref, r32 = ref64.double(), ref32.double()
    return max(tol * max(float(ref[b].abs().max()), 1e-3 * float(ref.abs().max())), 4 * float((r32[b] - ref[b]).abs().max()))


def tasks_missing(got, ref64, ref32, tol):
    """The tasks of ``got`` beyond their gate; every task if ``got`` holds a non-finite value."""
    got = got.double()
    if not torch.isfinite(got).all():
        return list(range(got.shape[0]))
    return [b for b in range(got.shape[0]) if float((got[b] - ref64[b].double()).abs().max()) > task_gate(ref64, ref32, b, tol)]


def row_gate(ref64_row, ref32_row, tol):
    """The gate of ``assert_gated`` (tests/test_hip_mha.py) on one row."""
    return max(tol * float(ref64_row.abs().max()), 4 * float((ref32_row.double() - ref64_row).abs().max()))


# ---- the diagonal test: one-hot values -------------------------------------------------------------------------------------------
def one_hot_case(d, n, C_pad, seed):
    """Two tasks, counts (n, 5): random Q, K at scale 1.5 and V[j] = e_j (n <= d), so output row i IS probability row i."""
    assert n <= d and n <= C_pad
    gen = torch.Generator().manual_seed(seed)
    Q, K = (1.5 * torch.randn(2, C_pad, d, generator=gen) for _ in range(2))
    V = torch.zeros(2, C_pad, d)
    V[:, torch.arange(n), torch.arange(n)] = 1.0
    return Q, K, V, (n, 5)


# ---- loo_mean --------------------------------------------------------------------------------------------------------------------
MEAN_PTS, MEAN_COUNTS, MEAN_F = 70, (70, 65, 64, 33, 32, 17, 2, 1, 0), (36, 128, 256)
OUTLIER_FACTORS = (1e3, 1e5, 1e7)
MEAN_REGIMES = ("random",) + tuple(f"outlier@{f:.0e}" for f in OUTLIER_FACTORS) + ("offset", "mixed_sign_cancel")
OUTLIER_AT = ("first", "last", 31, 32)
MEAN_TOL = 1e-6


def outlier_row(b, n, shift):
    """The outlying row of task ``b`` (n >= 1 valid rows): OUTLIER_AT rotating over the tasks, the next one where the count is too small."""
    for k in range(len(OUTLIER_AT)):
        at = OUTLIER_AT[(b + shift + k) % len(OUTLIER_AT)]
        at = {"first": 0, "last": n - 1}.get(at, at)
        if at < n:
            return at
    raise AssertionError


def mean_seed(regime, F):
    return 1000 * MEAN_REGIMES.index(regime) + F


def mean_case(regime, F, counts=MEAN_COUNTS, pts=MEAN_PTS):
    """fp32 R [B, pts, F]; the rows beyond a count hold random numbers like the rest."""
    gen = torch.Generator().manual_seed(mean_seed(regime, F))
    R = torch.randn(len(counts), pts, F, generator=gen)
    if regime.startswith("outlier@"):
        f = float(regime.split("@")[1])
        for b, n in enumerate(counts):
            if n:
                R[b, outlier_row(b, n, OUTLIER_FACTORS.index(f))] *= f
    elif regime == "offset":
        R = R + 1000.0
    elif regime == "mixed_sign_cancel":
        for b, n in enumerate(counts):
            if n >= 2:
                R[b, n - 1] = -R[b, :n - 1].sum(0)
    elif regime != "random":
        raise ValueError(regime)
    return R


def loo_mean_ref(R, counts, how):
    """[B, pts, F] (zeros beyond a count and for n <= 1).  ``how``: ``float64``; ``direct32`` -- the fp32 sum over the others and one
    division; ``formula32`` -- (s - r_i) / (n - 1) with s the fp32 sum of all n rows; ``formula64`` -- the same with s, the
    subtraction and the division in float64 and ONE rounding to fp32 (what the kernel computes now)."""
    dtype = torch.float32 if how in ("direct32", "formula32") else torch.float64
    out = torch.zeros_like(R, dtype=torch.float32 if how == "formula64" else dtype)
    for b, n in enumerate(counts):
        if n < 2:
            continue
        v = R[b, :n].to(dtype)
        if how in ("float64", "direct32"):
            keep = ~torch.eye(n, dtype=torch.bool)
            res = torch.stack([v[keep[i]].sum(0) for i in range(n)]) / (n - 1)
        else:
            res = (v.sum(0, keepdim=True) - v) / (n - 1)
        out[b, :n] = res.to(out.dtype)
    return out


def mean_row_gates(ref64, direct32, tol=MEAN_TOL):
    """[B, pts]: max(tol * max_f |ref_row|, 4 * max_f |direct fp32 - ref| of that row)."""
    return torch.maximum(tol * ref64.abs().amax(-1), 4 * (direct32.double() - ref64).abs().amax(-1))


def mean_row_ratio(got, ref64, direct32, tol=MEAN_TOL):
    """[B, pts]: error / gate per row; 0 where both are 0 (the rows that are exact zeros), inf where ``got`` is not finite."""
    err = (got.double() - ref64).abs().amax(-1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    gate = mean_row_gates(ref64, direct32, tol)
    return torch.where((err == 0) & (gate == 0), torch.zeros_like(err), err / gate)


def pair_case(F, seed):
    """fp32 R [4, 2, F] for tasks of count 2: both signs, magnitudes 10^U(-3, 3) x (0.5 ... 1.5) -- every two entries within a factor
    1e7 of each other, all normal numbers."""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (6.0 * torch.rand(4, 2, F, generator=gen, dtype=torch.float64) - 3.0) * (0.5 + torch.rand(4, 2, F, generator=gen, dtype=torch.float64))
    sign = torch.randint(0, 2, (4, 2, F), generator=gen).double() * 2.0 - 1.0
    return (sign * mag).float()
