"""The inputs of tests/test_hip_loo_edges.py on the CPU: every regime of tests/loo_cases.py holds under the exclusion what it claims
(float64), the references are the function the older tests use, the fp32 evaluations stay inside the gates -- so a gate means
something -- and every slip a regime is there to catch, put into an fp32 FORMULA (never into a kernel), misses its gate."""
import math

import pytest
import torch

import loo_cases as LC
import masked_cases as MC

HOST_WIDTHS = tuple(sorted(set(LC.WIDTHS + (32,))))


def _others(S, n):
    """float64 [n, n]: the scores of the queries 0 .. n - 1 with their own key at -inf."""
    T = S[:n].clone()
    T.fill_diagonal_(-math.inf)
    return T


def _same(a, b):
    if a.shape != b.shape or a.numel() == 0:
        return a.shape == b.shape
    return float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


# ---- attention -----------------------------------------------------------------------------------------------------------------
def test_the_shape_family_crosses_every_edge():
    assert LC.C_PAD == 200 and (LC.C_PAD + 63) // 64 == 4 and (LC.C_PAD + 31) // 32 == 7 and (LC.C_PAD + 15) // 16 == 13
    assert LC.COUNTS == (200, 129, 128, 65, 64, 33, 17, 2) and len(LC.COUNTS) == 2 * len(MC.FACTORS)
    crossed = LC.Q_COUNTS["crossed"]
    below = [q for q, n in zip(crossed, LC.COUNTS) if q < n]
    above = [q for q, n in zip(crossed, LC.COUNTS) if q > n]
    assert {0, 16, 64} <= set(below) and LC.C_PAD in above and len(above) >= 3 and LC.Q_COUNTS["same"] == LC.COUNTS


@pytest.mark.parametrize("d", HOST_WIDTHS)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_inherited_regimes_under_the_exclusion(regime, d):
    """Per task with at least two valid keys, in float64: the special query loses the key that dominates its row, and what is left
    is what the docstring of tests/loo_cases.py says."""
    Q, K, V = LC.attn_case(regime, d)
    KB = MC.key_block(d)
    assert Q.shape == K.shape == V.shape == (len(LC.COUNTS), LC.C_PAD, d) and Q.dtype == torch.float32
    for b, n in enumerate(LC.COUNTS):
        S = MC.scores64(Q, K, b, n, d)
        what = f"{regime} d={d} task {b} count {n}"
        if n < LC.C_PAD and regime != "equal":  # (the padding rows score about 30 above the task's maximum)
            assert float(MC.scores64(Q, K, b, LC.C_PAD, d)[:, n:].min()) > float(S.max()) + 25, what
        j = LC.special_row(regime, S, n, KB)
        P = torch.softmax(_others(S, n), -1)
        if regime.startswith("one_key@"):
            assert j == MC.one_key_index(regime, n, KB)
            if n > 2:
                assert float(P[j].max()) < 0.5, f"{what}: query {j} without its key still has a weight of {float(P[j].max()):.3f}"
            else:  # (two points: the one key that is left has the weight 1, whatever it scores)
                assert float(P[j, 1 - j]) == 1.0, what
            rest = torch.cat([P[:j, j], P[j + 1:, j]])
            assert float(rest.min()) > 1 - 1e-9, what
            full = torch.softmax(S[:n], -1)
            assert float(full[j, j]) > 1 - 1e-9  # (with its own key the query would be like every other one)
        elif regime == "ascending":
            assert j == n - 1 and int(S[j].argmax()) == j, what
            last0 = (n - 1) // KB * KB  # the queries of the last key block: without the own key the maximum lies earlier
            for q in range(last0, n):
                with_own, without = int(S[q].argmax()), int(_others(S, n)[q].argmax())
                if with_own == q:
                    assert without < q, what
            assert int(_others(S, n)[j].argmax()) < j
        elif regime == "huge_pos":
            # the key built at 100.0 (the others lie up to 5 below; the noise of a single score has a deviation of 0.09, so for its
            # own query another key can come out a few tenths above it): the query loses a key within 0.5 of its row's maximum
            assert float(S[:n, j].mean()) > 99.9 and float(S[j, j]) > 99.5 and float(S[j, j]) >= float(S[j].max()) - 0.5, what
            assert float(torch.softmax(S[j], -1)[j]) >= 0.6 * float(torch.softmax(S[j], -1).max()), what
        elif regime == "equal":
            assert float((P - (1 - torch.eye(n, dtype=torch.float64)) / (n - 1)).abs().max()) < 1e-12, what


@pytest.mark.parametrize("d", (32, 64, 128, 256))
def test_own_dominant_gap_on_every_valid_row(d):
    Q, K, V = LC.attn_case("own_dominant", d)
    worst, top = math.inf, 0.0
    for b, n in enumerate(LC.COUNTS):
        S, own = LC.loo_scores64(Q, K, b, n, d)
        gap = own - _others(S, n).max(-1).values
        assert float(gap.min()) >= LC.OWN_GAP, f"d={d} task {b} (n={n}): own - max(other) = {float(gap.min()):.1f} < {LC.OWN_GAP}"
        worst, top = min(worst, float(gap.min())), max(top, float(own.max()))
    print(f"own_dominant d={d} gain {LC.own_gain(d)}: smallest gap {worst:.1f}, largest own score {top:.1f}")
    assert math.exp(-LC.OWN_GAP) < torch.finfo(torch.float32).tiny * torch.finfo(torch.float32).eps  # below the smallest denormal
    assert float(torch.exp(torch.tensor(-LC.OWN_GAP, dtype=torch.float32))) == 0.0


@pytest.mark.parametrize("d", (4, 16, 20, 28))
def test_own_dominant_is_refused_below_its_width(d):
    with pytest.raises(ValueError, match="own_dominant needs d >= 32"):
        LC.attn_case("own_dominant", d)
    assert not LC.regime_runs("own_dominant", d) and LC.regime_runs("own_dominant", 32) and LC.regime_runs("equal", d)


def test_the_reference_is_the_one_of_the_older_test_and_extends_it():
    """With query counts equal to the key counts ``loo_attention`` is ``_loo_attention`` of tests/test_hip_loo.py (written out here:
    that module needs a GPU to import); a row at or beyond the key count equals the plain attention; beyond n_q zeros.  "Equal": to
    1e-12 -- the products are taken on other row ranges, and a float64 matmul may then add in another order."""
    d, counts = 20, (40, 17, 2, 1, 0)
    g = torch.Generator().manual_seed(3)
    Q, K, V = (torch.randn(len(counts), 40, d, generator=g) for _ in range(3))
    scale = 1.0 / math.sqrt(d)
    old = torch.zeros_like(Q, dtype=torch.float64)
    for b, n in enumerate(counts):
        if n >= 2:
            S = Q[b, :n].double() @ K[b, :n].double().T * scale
            S.fill_diagonal_(-math.inf)
            old[b, :n] = torch.softmax(S, dim=-1) @ V[b, :n].double()
    assert _same(LC.loo_attention(Q, K, V, counts, counts, scale, torch.float64), old)
    q_counts = (17, 40, 40, 40, 40)
    new = LC.loo_attention(Q, K, V, counts, q_counts, scale, torch.float64)
    plain = LC.plain_attention(Q, K, V, counts, scale, torch.float64)
    none = LC.loo_attention(Q, K, V, counts, None, scale, torch.float64)
    assert torch.isfinite(new).all() and _same(new[0, :17], old[0, :17]) and not new[0, 17:].any()
    for b, n in enumerate(counts):
        assert _same(none[b, :n], old[b, :n]) and _same(none[b, n:], plain[b, n:])
    assert _same(new[1, 17:], plain[1, 17:]) and _same(new[1, :17], old[1, :17]) and plain[1, 17:].abs().max() > 0
    assert not new[3, 0].any() and _same(new[3, 1:], V[3, :1].double().expand(39, d)) and not new[4].any()


@pytest.mark.parametrize("regime,d", [(r, d) for r in LC.ATTN_REGIMES for d in LC.WIDTHS if LC.regime_runs(r, d)])
def test_the_fp32_walk_stays_inside_the_gates_and_its_slips_do_not(regime, d):
    """The kernel's walk in fp32 torch (``emulate_loo_kernel``) passes the per-task gate and the gate of every special row with all
    three query-count variants.  The same walk with one slip misses a gate where the regime says it would:
      own_in_max    on ``own_dominant`` (gap >= 110: every other weight is exp(-gap) = 0 in fp32, the rows come out as zeros).  On
                    ``one_key@...`` (gap 30), ``ascending`` and ``huge_pos`` it is NOT observable: exp(-30) = 1e-13 is a normal fp32
                    number, the weights keep their ratios and the normaliser divides the common factor out -- which is why
                    ``own_dominant`` exists;
      own_kept      on every regime but ``equal`` at task level or on a special row;
      pad_excluded  with no query count and with the crossed ones (rows n <= q < n_q);
      wrong_subblock on the special rows of ``one_key@...`` and on ``own_dominant``."""
    Q, K, V = LC.attn_case(regime, d)
    scale = 1.0 / math.sqrt(d)
    special = LC.special_rows(regime, Q, K, LC.COUNTS, d)

    def misses(got, r64, r32, qc):
        rows = [(b, j) for b, j in special if qc is None or j < qc[b]]
        bad_rows = [(b, j) for b, j in rows if not torch.isfinite(got[b, j]).all()
                    or float((got[b, j].double() - r64[b, j]).abs().max()) > LC.row_gate(r64[b, j], r32[b, j], 1e-5)]
        return LC.tasks_missing(got, r64, r32, 1e-5), bad_rows

    for name, qc in LC.Q_COUNTS.items():
        r64, r32 = (LC.loo_attention(Q, K, V, LC.COUNTS, qc, scale, dt) for dt in (torch.float64, torch.float32))
        assert torch.isfinite(r64).all() and float(r64.abs().max()) > 0
        tasks, rows = misses(LC.emulate_loo_kernel(Q, K, V, LC.COUNTS, qc, d), r64, r32, qc)
        assert not tasks and not rows, f"{regime} d={d} {name}: the fp32 walk misses tasks {tasks} rows {rows}"
        for slip in ("own_in_max", "own_kept", "pad_excluded", "wrong_subblock"):
            tasks, rows = misses(LC.emulate_loo_kernel(Q, K, V, LC.COUNTS, qc, d, slip=slip), r64, r32, qc)
            caught = bool(tasks or rows)
            if slip == "own_in_max":
                assert caught == (regime == "own_dominant"), f"{regime} d={d} {name} {slip}: caught = {caught}"
            if slip == "own_kept" and regime != "equal":
                assert caught, f"{regime} d={d} {name} {slip}"
            if slip == "pad_excluded" and name != "same":
                assert tasks, f"{regime} d={d} {name} {slip}"
            if slip == "wrong_subblock" and (regime == "own_dominant" or regime.startswith("one_key@")):
                assert caught, f"{regime} d={d} {name} {slip}"


@pytest.mark.parametrize("d,n", ((256, 200), (128, 128)))
def test_one_hot_values_show_the_probabilities(d, n):
    Q, K, V, counts = LC.one_hot_case(d, n, LC.C_PAD, seed=d + n)
    out = LC.loo_attention(Q, K, V, counts, None, 1.0 / math.sqrt(d), torch.float64)
    S = _others(MC.scores64(Q, K, 0, n, d), n)
    assert float((out[0, :n, :n] - torch.softmax(S, -1)).abs().max()) < 1e-14 and not out[0, :n, n:].any()
    assert not out[0, :n, :n].diagonal().any() and float((out[0, :n].sum(-1) - 1).abs().max()) < 1e-12
    kept = LC.emulate_loo_kernel(Q, K, V, counts, None, d, slip="own_kept")
    assert float(kept[0, :n, :n].diagonal().min()) > 0  # (a kernel that kept the own key has every diagonal entry positive)


# ---- loo_mean ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", LC.MEAN_F)
@pytest.mark.parametrize("regime", LC.MEAN_REGIMES)
def test_mean_regimes_hold_their_claims_and_the_gate_separates_the_formulas(regime, F):
    """The direct fp32 evaluation and the float64-sum formula stay inside the per-row gate on every case; the fp32-sum formula,
    ``(s - r_i) / (n - 1)`` as the kernel had it, does not on ``outlier`` -- on the outlying row of every task with one."""
    R = LC.mean_case(regime, F)
    counts = LC.MEAN_COUNTS
    assert R.shape == (len(counts), LC.MEAN_PTS, F) and R.dtype == torch.float32 and (LC.MEAN_PTS + 31) // 32 == 3
    ref, direct, f32, f64 = (LC.loo_mean_ref(R, counts, how) for how in ("float64", "direct32", "formula32", "formula64"))
    for b, n in enumerate(counts):
        assert not ref[b, n:].any() and (n > 1 or not ref[b].any())
        if n < 2:
            continue
        x = R[b, :n].double()
        assert float((ref[b, :n] - (x.sum(0, keepdim=True) - x) / (n - 1)).abs().max()) <= 1e-12 * float(x.abs().max())
        if regime.startswith("outlier@"):
            f = float(regime.split("@")[1])
            j = LC.outlier_row(b, n, LC.OUTLIER_FACTORS.index(f))
            big = x.abs().amax(-1)
            assert int(big.argmax()) == j and float(big[j]) > 0.1 * f and float(torch.cat([big[:j], big[j + 1:]]).max()) < 7
        elif regime == "offset":
            assert float((x.mean() - 1000).abs()) < 1
        elif regime == "mixed_sign_cancel":
            assert float(x.sum(0).abs().max()) < 1e-5 and float(x.abs().max()) > 1
    if regime.startswith("outlier@"):
        f = float(regime.split("@")[1])
        at = {LC.outlier_row(b, n, LC.OUTLIER_FACTORS.index(f)) for b, n in enumerate(counts) if n >= 2}
        assert len(at) >= 3 and {31, 32} <= at, at
    share = (direct.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp(min=1e-300)
    # the direct evaluation's own error: a few 1e-7 of the row; up to 2e-6 on ``mixed_sign_cancel``, where the sum over the others
    # of a row is itself a cancellation (the last row undoes the rest).  4 x that stays below 1e-5 of the row: the gate means something
    limit = 2.5e-6 if regime == "mixed_sign_cancel" else 5e-7
    assert float(share.max()) <= limit, f"{regime} F={F}: the direct fp32 evaluation errs by {float(share.max()):.2e} of a row"
    assert float(LC.mean_row_ratio(direct, ref, direct).max()) <= 1.0
    r64 = LC.mean_row_ratio(f64, ref, direct)
    assert float(r64.max()) <= 0.1, f"{regime} F={F}: float64 sum, one rounding: {float(r64.max()):.3f} of the gate"
    r32 = LC.mean_row_ratio(f32, ref, direct)
    print(f"{regime} F={F}: worst err/gate  fp32-sum formula {float(r32.max()):.3g}  float64-sum formula {float(r64.max()):.3g}")
    if regime.startswith("outlier@"):
        f = float(regime.split("@")[1])
        for b, n in enumerate(counts):
            if n >= 2:
                j = LC.outlier_row(b, n, LC.OUTLIER_FACTORS.index(f))
                assert float(r32[b, j]) > 1.0, f"{regime} F={F} task {b}: the fp32-sum formula passes on the outlying row {j}"
        # ... while the task-level gate of tests/test_hip_loo.py (1e-6 of the task's max|ref|) lets it through
        for b, n in enumerate(counts):
            if n >= 2:
                assert float((f32[b].double() - ref[b]).abs().max()) <= 1e-6 * float(ref[b].abs().max())


@pytest.mark.parametrize("F", LC.MEAN_F)
def test_two_points_swap_exactly_only_with_a_float64_sum(F):
    R = LC.pair_case(F, seed=F)
    x = R.double().abs()
    assert torch.isfinite(R).all() and float(x.min()) > 1e-30 and float(x.max() / x.min()) < 1e7
    counts = (2, 2, 2, 2)
    f64, f32 = LC.loo_mean_ref(R, counts, "formula64"), LC.loo_mean_ref(R, counts, "formula32")
    assert torch.equal(f64[:, 0], R[:, 1]) and torch.equal(f64[:, 1], R[:, 0])
    assert not torch.equal(f32[:, 0], R[:, 1])  # (an fp32 sum has rounded the smaller of the two)
