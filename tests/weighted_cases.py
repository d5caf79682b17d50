"""Inputs of the key-weighted edge tests (tests/test_weighted_cases_host.py on the CPU, tests/test_hip_weighted_edges.py on the GPU):
the score regimes of tests/masked_cases.py under weight patterns placed where the weighted rule of csrc/masked_kernels.hip differs
from the plain one -- the score ``scale <q, k> + log w``, the running maximum over the admissible keys alone, staged blocks that hold
nothing for a query, K / V rows zeroed by weight, ``key_ok`` by weight in the d_k / d_v kernel and ``d_w = (sum_q dA) / w``.

Keys and queries are built as in ``masked_cases.build`` (``a_k u + noise`` / ``c u + noise``, the rows beyond the count 30 above the
task's maximum), here from an explicit target-score vector per task (``build_from_scores``), which adds the regime
``ascending_wide``: scores from -56 to +56 over the valid keys (WIDE_SCORE; at +-60 the float64 d_w of ``counter`` reached 1.4e30,
above the 1e30 that tests/test_weighted_cases_host.py allows a reference tensor, so the range was narrowed there).
``random`` is the unit-normal draw of the plain suite's ``_random_case``.  V and dO carry ``masked_cases.scale_per_task``; the eight key counts are ``masked_cases.key_counts``.

A key is admissible iff it lies below the count and ``0 < w < inf`` (tests/keyweight_reference.py).  Patterns, each a function of
the task's target scores, its count and the key block KB (32 keys, 16 at the 256-wide instance; the d_k / d_v kernel walks 16):

* ``drop_top``  the key with the highest target score of every task is inadmissible, every other weight is 1.  A task of count 1
  becomes empty.
* ``counter``   ``w_k = fp32(exp(-a_k))``: the weights cancel the scores, every effective logit of a task is about 0 while the raw
  scores and the weights span e^+-40 (e^+-56 under ``ascending_wide``: 2.1e24 and 4.8e-25, normal fp32 numbers).
* ``wide``      log2 w uniform in [-100, 100] independent of the scores; task 1 in [-60, -40] and task 2 in [40, 60], so that a
  whole task sits far from 1.
* ``holes``     weights 0 / 1 in seven variants: (a) the first staged block inadmissible, (b) a middle block (block ``blocks // 2``
  of the task's ``blocks`` staged blocks: the only one of a one-block task, the last of a two-block task), (c) only the last valid
  key admissible, (d) only key 0, (e) nothing admissible, (f) one aligned run of 16 keys inadmissible between live neighbours (the
  run ``[16 r, 16 r + 16)`` with ``r = max(1, count // 32)``; a task of fewer than 33 keys has no room for it and keeps every
  weight 1), (g) every key of even index inadmissible.

The weight of an inadmissible key below the count rotates over ``DEAD_WEIGHTS`` = 0.0, -0.0, -1.0, NaN, +Inf, -Inf (by task, key
and case, so that every value meets every count over the cases); ``Case.poisoned()`` gives K and V with NaN in those keys' rows.
Under every pattern the weights at and beyond the count are NaN.

Out of scope: denormal weights and weights outside [2^-100, 2^100]."""
import math
from types import SimpleNamespace

import torch

import masked_cases as MC

SHAPES = ((32, 100), (128, 100), (256, 70))  # (d, C_pad) of the plain suite: both key-block sizes, at least 3 blocks each
T = 70
Q_COUNTS = [70, 0, 65, 1, 64, 17, 33, 69]
DEAD_WEIGHTS = (0.0, -0.0, -1.0, math.nan, math.inf, -math.inf)
WIDE_SCORE = 56.0
WIDE_LOG2 = 100.0
WIDE_SHIFTED = {1: (-60.0, -40.0), 2: (40.0, 60.0)}  # task -> range of log2 w
HOLE_VARIANTS = "abcdefg"
PATTERN_REGIMES = {
    "drop_top": ("huge_pos", "one_key@first", "one_key@last", "one_key@edge", "ascending", "descending"),
    "counter": ("ascending", "descending", "ascending_wide"),
    "wide": ("equal", "huge_neg", "random"),
    "holes": ("ascending", "random"),
}
CASES = tuple((p, r, v) for p, rs in PATTERN_REGIMES.items() for r in rs for v in (HOLE_VARIANTS if p == "holes" else ("",)))


def case_id(case):
    pattern, regime, variant = case
    return f"{pattern}{'(' + variant + ')' if variant else ''}-{regime}"


def target_scores(regime, n, KB, gen):
    """float64 [n] (``n`` >= 1): ``masked_cases.target_scores`` and the regime ``ascending_wide``."""
    if regime == "ascending_wide":
        return torch.linspace(-WIDE_SCORE, WIDE_SCORE, n, dtype=torch.float64)
    return MC.target_scores(regime, n, KB, gen)


def build_from_scores(scores, C_pad, T, d, gen):
    """fp32 Q [B, T, d], K [B, C_pad, d], V [B, C_pad, d] as ``masked_cases.build`` makes them, for tasks whose valid keys are built
    for the target scores ``scores[b]`` (float64 [count_b], possibly empty), and the float64 [B, C_pad] targets of every row (the
    rows beyond a count: the task's maximum + 30)."""
    B = len(scores)
    Q, K, V = (torch.randn(B, n, d, generator=gen, dtype=torch.float64) for n in (T, C_pad, C_pad))
    u = torch.randn(d, generator=gen, dtype=torch.float64)
    u = u / u.norm()
    Q, K = (MC.NOISE * (X - (X @ u).unsqueeze(-1) * u) for X in (Q, K))  # (noise orthogonal to u)
    c = 2.0 * d ** 0.25
    a = torch.empty(B, C_pad, dtype=torch.float64)
    for b, s in enumerate(scores):
        n = s.numel()
        a[b, :n] = s
        a[b, n:] = (float(s.max()) if n else 0.0) + 30.0
    K = K + (a * math.sqrt(d) / c).unsqueeze(-1) * u
    Q = Q + c * u
    return Q.float(), K.float(), V.float(), a


def _dead(b, k, shift):
    return DEAD_WEIGHTS[(b + k + shift) % len(DEAD_WEIGHTS)]


def hole_keys(variant, n, KB):
    """The inadmissible keys (sorted list of indices below ``n``) of a ``holes`` task with ``n`` valid keys."""
    blocks = -(-n // KB)
    if variant == "a":
        dead = range(0, min(KB, n))
    elif variant == "b":
        dead = range(blocks // 2 * KB, min((blocks // 2 + 1) * KB, n))
    elif variant == "c":
        dead = range(0, n - 1)
    elif variant == "d":
        dead = range(1, n)
    elif variant == "e":
        dead = range(0, n)
    elif variant == "f":
        r = max(1, n // 32)
        dead = range(16 * r, 16 * r + 16) if 16 * r + 16 < n else range(0)
    elif variant == "g":
        dead = range(0, n, 2)
    else:
        raise ValueError(variant)
    return list(dead)


def weights(pattern, variant, a, counts, KB, shift, gen):
    """fp32 W [B, C_pad] of ``pattern``; ``a``: float64 [B, C_pad] target scores (``drop_top`` / ``counter``), else not looked at."""
    B, C_pad = len(counts), (a.shape[1] if a is not None else None)
    W = torch.ones(B, C_pad, dtype=torch.float32)
    if pattern == "wide":
        lo = torch.full((B, 1), -WIDE_LOG2, dtype=torch.float64)
        hi = torch.full((B, 1), WIDE_LOG2, dtype=torch.float64)
        for b, (l, h) in WIDE_SHIFTED.items():
            if b < B:
                lo[b], hi[b] = l, h
        W = torch.exp2(lo + (hi - lo) * torch.rand(B, C_pad, generator=gen, dtype=torch.float64)).float()
    for b, n in enumerate(counts):
        if pattern == "drop_top" and n:
            k = int(a[b, :n].argmax())
            W[b, k] = _dead(b, 0, shift)
        elif pattern == "counter":
            W[b, :n] = torch.exp(-a[b, :n]).float()
        elif pattern == "holes":
            for k in hole_keys(variant, n, KB):
                W[b, k] = _dead(b, k, shift)
        W[b, n:] = math.nan
    return W


class Case(SimpleNamespace):
    """Q [B, T, d], K, V [B, C_pad, d], dO [B, T, d], W [B, C_pad] (fp32, finite K / V everywhere), ``counts``, ``KB``, ``a`` (float64
    target scores [B, C_pad] or None), ``adm`` (bool [B, C_pad], the admissible keys) and ``dead`` (below the count, inadmissible)."""

    def poisoned(self):
        """(K, V) with NaN in the rows of the inadmissible keys below the count."""
        K, V = self.K.clone(), self.V.clone()
        K[self.dead], V[self.dead] = math.nan, math.nan
        return K, V

    def finite_weights(self):
        """W with every value that is not admissible replaced by 0.0 (finite; the keys stay inadmissible)."""
        return torch.where(self.adm, self.W, torch.zeros_like(self.W))


def _inputs(regime, counts, C_pad, T_, d, KB, gen):
    """(Q, K, V, a): ``a`` None where the regime has no target scores (``equal``, ``random``)."""
    B = len(counts)
    if regime == "equal":
        return MC.build("equal", counts, C_pad, T_, d, KB, gen) + (None,)
    if regime == "random":  # (as ``_random_case`` of tests/test_hip_masked_edges.py)
        return tuple(torch.randn(B, n, d, generator=gen) * s for n, s in ((T_, 1.5), (C_pad, 1.5), (C_pad, 1.0))) + (None,)
    scores = [target_scores(regime, n, KB, gen) if n else torch.zeros(0, dtype=torch.float64) for n in counts]
    return build_from_scores(scores, C_pad, T_, d, gen)


def _finish(Q, K, V, a, W, counts, KB, gen, T_, d):
    import keyweight_reference as KR

    V, dO = MC.scale_per_task(V, torch.randn(len(counts), T_, d, generator=gen))
    adm = KR.admissible(W, counts)
    below = torch.arange(K.shape[1]).view(1, -1) < torch.tensor(counts).view(-1, 1)
    return Case(Q=Q, K=K, V=V, dO=dO, W=W, counts=list(counts), KB=KB, a=a, adm=adm, dead=below & ~adm, d=d, C_pad=K.shape[1], T=T_)


def make(case, d, C_pad):
    """The inputs of ``case`` = (pattern, regime, variant) at the shape (d, C_pad): eight tasks, T = 70."""
    pattern, regime, variant = case
    KB = MC.key_block(d)
    counts = MC.key_counts(C_pad, KB)
    idx = CASES.index(case)
    gen = torch.Generator().manual_seed(7000 + 10 * idx + SHAPES.index((d, C_pad)))
    Q, K, V, a = _inputs(regime, counts, C_pad, T, d, KB, gen)
    W = weights(pattern, variant, a if a is not None else torch.zeros(len(counts), C_pad, dtype=torch.float64), counts, KB, idx + 1, gen)
    return _finish(Q, K, V, a, W, counts, KB, gen, T, d)


# ---- replicates of one stored context ------------------------------------------------------------------------------------------
REPLICATE_REGIMES = ("ascending", "descending")  # (where both ``drop_top`` and ``counter`` run)
REPLICATE_PATTERNS = ("ones", "drop_top", "counter")
REPLICATE_Q_COUNTS = [70, 0, 65, 1]


def make_replicates(regime, d, C_pad):
    """(case, W [3, 4, C_pad]): B = 4 context tasks (counts C_pad - 1, 1, 0, KB + 1) of ``regime`` and the weight rows of the S = 3
    replicates ``REPLICATE_PATTERNS``.  ``case.W`` / ``adm`` / ``dead`` are those of the first replicate (all ones)."""
    KB = MC.key_block(d)
    counts = [C_pad - 1, 1, 0, KB + 1]
    gen = torch.Generator().manual_seed(9000 + 10 * REPLICATE_REGIMES.index(regime) + SHAPES.index((d, C_pad)))
    Q, K, V, a = _inputs(regime, counts, C_pad, T, d, KB, gen)
    Ws = [weights(p, "", a, counts, KB, 3 + i, gen) for i, p in enumerate(REPLICATE_PATTERNS)]
    return _finish(Q, K, V, a, Ws[0], counts, KB, gen, T, d), torch.stack(Ws)


# ---- a shared prefix and an own tail -------------------------------------------------------------------------------------------
def prefix_cuts(regime, a_or_none, counts, KB, shift):
    """Per task the number of its valid keys that go into the prefix, rotating over 0, 1, KB - 1, KB, KB + 1, n - 1, n, the index of
    the largest target score and that index + 1 (clamped to 0 .. n)."""
    cuts = []
    for b, n in enumerate(counts):
        top = int(a_or_none[b, :n].argmax()) if (a_or_none is not None and n) else 0
        options = (0, 1, KB - 1, KB, KB + 1, n - 1, n, top, top + 1)
        cuts.append(max(0, min(n, options[(b + shift) % len(options)])))
    return cuts


def make_prefix(regime, d, C_pad):
    """The plain regime ``regime`` of ``masked_cases`` split into a prefix and a tail: a dict with Q [8, T, d], the whole K / V
    [8, C_pad, d] and ``counts``; ``k_pre`` / ``v_pre`` [8, C_pad, d] (the first ``n_prefix[b]`` keys, NaN behind them), ``k_tail`` /
    ``v_tail`` [16, C_pad, d] and ``n_tail`` [16] (task 8 s + b: sample s of prefix b; sample 0 holds the remaining valid keys in
    order, sample 1 the same in reverse order; NaN behind them), and ``order`` [16][n]: the key indices of every task in the order
    its walk meets them."""
    KB = MC.key_block(d)
    counts = MC.key_counts(C_pad, KB)
    ri = MC.REGIMES.index(regime)
    gen = torch.Generator().manual_seed(11000 + 10 * ri + SHAPES.index((d, C_pad)))
    if regime == "equal":
        Q, K, V = MC.build("equal", counts, C_pad, T, d, KB, gen)
        a = None
    else:
        scores = [MC.target_scores(regime, n, KB, gen) if n else torch.zeros(0, dtype=torch.float64) for n in counts]
        Q, K, V, a = build_from_scores(scores, C_pad, T, d, gen)
    (V,) = MC.scale_per_task(V)
    cuts = prefix_cuts(regime, a, counts, KB, ri)
    B = len(counts)
    k_pre, v_pre = torch.full_like(K, math.nan), torch.full_like(V, math.nan)
    k_tail, v_tail = (torch.full((2 * B, C_pad, d), math.nan) for _ in range(2))
    n_tail, order = [], []
    for s in range(2):
        for b, (n, p) in enumerate(zip(counts, cuts)):
            rest = list(range(p, n))
            if s == 1:
                rest.reverse()
            k_pre[b, :p], v_pre[b, :p] = K[b, :p], V[b, :p]
            k_tail[B * s + b, :n - p], v_tail[B * s + b, :n - p] = K[b, rest], V[b, rest]
            n_tail.append(n - p)
            order.append(list(range(p)) + rest)
    return dict(Q=Q, K=K, V=V, counts=counts, KB=KB, n_prefix=cuts, n_tail=n_tail, k_pre=k_pre, v_pre=v_pre, k_tail=k_tail,
                v_tail=v_tail, order=order)


# ---- the weighted mean ---------------------------------------------------------------------------------------------------------
MEAN_PTS = 70
MEAN_WIDTHS = (4, 256)
MEAN_VALUES = ("normal", "offset")  # randn, and 1e3 + 1e-3 randn: a spread a million times below the level
MEAN_CASES = tuple((p, v, r) for r in MEAN_VALUES for p in ("wide", "holes") for v in (HOLE_VARIANTS if p == "holes" else ("",)))


def make_mean(case, F):
    """(R [8, 70, F], W [8, 70], dOut [8, F], counts, adm, dead) of ``case`` = (pattern, variant, values); the point tile of the mean
    kernels (32 points) stands in for the key block."""
    pattern, variant, values = case
    counts = MC.key_counts(MEAN_PTS, 32)
    idx = MEAN_CASES.index(case)
    gen = torch.Generator().manual_seed(13000 + 10 * idx + MEAN_WIDTHS.index(F))
    R = torch.randn(len(counts), MEAN_PTS, F, generator=gen)
    if values == "offset":
        R = (1e3 + 1e-3 * R.double()).float()
    dOut = torch.randn(len(counts), F, generator=gen)
    W = weights(pattern, variant, torch.zeros(len(counts), MEAN_PTS, dtype=torch.float64), counts, 32, idx, gen)
    import keyweight_reference as KR

    adm = KR.admissible(W, counts)
    below = torch.arange(MEAN_PTS).view(1, -1) < torch.tensor(counts).view(-1, 1)
    return R, W, dOut, counts, adm, below & ~adm
