"""The inputs of the key-weighted edge tests (tests/weighted_cases.py) on the CPU, against the references alone
(``keyweight_reference.weighted_attention_and_grads`` in float64 and float32): every pattern does what it claims, every reference
tensor is finite and of moderate size, three deliberately wrong fp32 evaluations miss the per-task gate of
tests/test_hip_masked_edges.py (so a kernel that made the same mistake could not pass tests/test_hip_weighted_edges.py), and every
pattern meets every shape and both key-block sizes.  Nothing here reads a kernel's result: the input ranges are decided here."""
import math

import pytest
import torch

import keyweight_reference as KR
import masked_cases as MC
import weighted_cases as WC
from test_hip_masked_edges import assert_gated_per_task

BIG = 1e30
_DEAD_BITS = {torch.tensor(v, dtype=torch.float32).view(torch.int32).item() for v in WC.DEAD_WEIGHTS}
_refs = {}


def references(case, d, C_pad):
    """(inputs, r64, r32) of a case without query counts, computed once and shared (never modified)."""
    key = (case, d, C_pad)
    if key not in _refs:
        cs = WC.make(case, d, C_pad)
        _refs[key] = (cs,) + tuple(KR.weighted_attention_and_grads(cs.Q, cs.K, cs.V, cs.W, cs.dO, cs.counts, 1.0 / math.sqrt(d), dt)
                                   for dt in (torch.float64, torch.float32))
    return _refs[key]


def misses(got, r64, r32, tol):
    """Whether ``got`` fails the per-task gate on at least one task."""
    try:
        assert_gated_per_task(got, r64, r32, tol, "wrong evaluation")
    except AssertionError:
        return True
    return False


CASE_PARAMS = [pytest.param(c, id=WC.case_id(c)) for c in WC.CASES]


# ---- claims --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_patterns_hold_what_they_claim(case, d, C_pad):
    pattern, regime, variant = case
    cs = WC.make(case, d, C_pad)
    KB, counts = cs.KB, cs.counts
    assert KB == MC.key_block(d) and counts == MC.key_counts(C_pad, KB) and cs.Q.shape == (8, WC.T, d)
    assert all(torch.isfinite(x).all() for x in (cs.Q, cs.K, cs.V, cs.dO))
    Kp, Vp = cs.poisoned()
    for b, n in enumerate(counts):
        what = f"{WC.case_id(case)} d={d} task {b} count {n}"
        w = cs.W[b]
        assert torch.isnan(w[n:]).all(), what  # (NaN at and beyond the count)
        live = set(range(n))
        if pattern == "drop_top" and n:
            live -= {int(cs.a[b, :n].argmax())}
        elif pattern == "holes":
            dead = WC.hole_keys(variant, n, KB)
            live -= set(dead)
            blocks = -(-n // KB)
            if variant == "a":
                assert dead == list(range(min(KB, n))), what
            elif variant == "b" and blocks >= 3:  # (a block with live blocks on both sides)
                assert 0 < dead[0] and dead[-1] < n - 1 and dead[0] % KB == 0 and len(dead) == KB, what
            elif variant == "c" and n:
                assert live == {n - 1}, what
            elif variant == "d" and n:
                assert live == {0}, what
            elif variant == "e":
                assert not live, what
            elif variant == "f" and n >= 33:
                assert len(dead) == 16 and dead[0] % 16 == 0 and dead[0] - 1 in live and dead[-1] + 1 in live, what
            elif variant == "g":
                assert dead == list(range(0, n, 2)), what
        assert set(cs.adm[b].nonzero().flatten().tolist()) == live, what
        assert set(cs.dead[b].nonzero().flatten().tolist()) == set(range(n)) - live, what
        for k in set(range(n)) - live:  # (the values that remove a key, and NaN in its rows)
            assert w[k:k + 1].view(torch.int32).item() in _DEAD_BITS, what
            assert torch.isnan(Kp[b, k]).all() and torch.isnan(Vp[b, k]).all(), what
        assert torch.equal(Kp[b, sorted(live)], cs.K[b, sorted(live)]) and torch.isfinite(Kp[b, n:]).all(), what
        wl = w[sorted(live)].double()
        assert ((wl >= 2.0 ** -100) & (wl <= 2.0 ** 100)).all(), what  # (the scope of the module)
        if pattern in ("drop_top", "holes"):
            assert (wl == 1).all(), what
        if n < 2:
            continue
        S = MC.scores64(cs.Q, cs.K, b, n, d)
        if pattern == "counter":  # the weights cancel the scores: what is left of a + log w is the noise term
            assert float((cs.a[b, :n] + torch.log(w[:n].double())).abs().max()) < 1e-5, what
            eff = S + torch.log(w[:n].double())
            assert float((eff.max(-1).values - eff.min(-1).values).max()) < 1, what
            assert float(S.max() - S.min()) > (2 * WC.WIDE_SCORE - 5 if regime == "ascending_wide" else 75), what
        elif pattern == "drop_top":
            k = (set(range(n)) - live).pop()
            assert k == int(cs.a[b, :n].argmax()), what
            if regime == "huge_pos":  # (several keys within 5 of the top by construction: the removed one is among the dominant)
                assert float((S.max(-1).values - S[:, k]).max()) < 1, what
            else:
                assert (S.argmax(-1) == k).all(), what
        elif pattern == "wide":
            l2 = torch.log2(w[:n].double())
            lo, hi = WC.WIDE_SHIFTED.get(b, (-WC.WIDE_LOG2, WC.WIDE_LOG2))
            assert float(l2.min()) >= lo and float(l2.max()) <= hi, what
            if b not in WC.WIDE_SHIFTED and n >= 16:
                assert float(l2.max() - l2.min()) > 100, what
    if pattern == "drop_top":  # the tasks of count 1 became empty
        assert [not cs.adm[b].any() for b, n in enumerate(counts) if n == 1] == [True]
    if pattern == "holes":  # every removing value occurs
        assert {cs.W[cs.dead].view(torch.int32)[i].item() for i in range(int(cs.dead.sum()))} == _DEAD_BITS


def test_every_removing_value_meets_the_top_key_of_a_task_with_keys():
    """Over the ``drop_top`` cases, each of 0.0, -0.0, -1.0, NaN, +Inf and -Inf is the weight of the top key of a task with at least
    two keys, at every shape (the rotation starts at another value in every case)."""
    for d, C_pad in WC.SHAPES:
        seen = set()
        for case in WC.CASES:
            if case[0] == "drop_top":
                cs = WC.make(case, d, C_pad)
                seen |= {cs.W[b, int(cs.a[b, :n].argmax())].view(torch.int32).item() for b, n in enumerate(cs.counts) if n >= 2}
        assert seen == _DEAD_BITS, (d, seen)


# ---- finiteness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_references_are_finite_and_moderate(case, d, C_pad):
    cs, r64, r32 = references(case, d, C_pad)
    for name, x64, x32 in zip(("O", "dQ", "dK", "dV", "dW", "lse"), r64, r32):
        assert torch.isfinite(x64).all() and float(x64.abs().max()) <= BIG, f"{name} float64"
        assert torch.isfinite(x32).all(), f"{name} float32"
    wdw = cs.finite_weights().double() * r64[4]
    assert torch.isfinite(wdw).all() and float(wdw.abs().max()) <= BIG
    assert float(r64[0].abs().max()) > 0 or case[2] == "e"
    # the reference gives the keys that are not admissible, and the tasks without one, exact zeros
    assert not r64[2][~cs.adm].any() and not r64[3][~cs.adm].any() and not r64[4][~cs.adm].any()
    for b in range(len(cs.counts)):
        if not cs.adm[b].any():
            assert not r64[0][b].any() and not r64[1][b].any()
    # with query counts and NaN in the rows the references never read
    Kp, Vp = cs.poisoned()
    Qp, dOp = cs.Q.clone(), cs.dO.clone()
    for b, n in enumerate(WC.Q_COUNTS):
        Qp[b, n:], dOp[b, n:] = math.nan, math.nan
    for dt in (torch.float64, torch.float32):
        r = KR.weighted_attention_and_grads(Qp, Kp, Vp, cs.W, dOp, cs.counts, 1.0 / math.sqrt(d), dt, WC.Q_COUNTS)
        assert all(torch.isfinite(x).all() and float(x.abs().max()) <= BIG for x in r), dt


@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
def test_replicate_and_prefix_inputs_are_finite(d, C_pad):
    for regime in WC.REPLICATE_REGIMES:
        cs, W = WC.make_replicates(regime, d, C_pad)
        assert W.shape == (3, 4, C_pad) and (W[0][KR.admissible(W[0], cs.counts)] == 1).all()
        for s in range(3):
            r = KR.weighted_attention_and_grads(cs.Q, cs.K, cs.V, W[s], cs.dO, cs.counts, 1.0 / math.sqrt(d), torch.float64)
            assert torch.isfinite(r[0]).all() and float(r[0].abs().max()) > 0
    seen = set()
    for regime in MC.REGIMES:
        p = WC.make_prefix(regime, d, C_pad)
        for j, order in enumerate(p["order"]):
            b, n, cut = j % 8, p["counts"][j % 8], p["n_prefix"][j % 8]
            assert sorted(order) == list(range(n)) and order[:cut] == list(range(cut)) and p["n_tail"][j] == n - cut
            assert torch.equal(p["k_tail"][j, :n - cut], p["K"][b, order[cut:]]) and torch.isnan(p["k_tail"][j, n - cut:]).all()
            assert torch.equal(p["v_pre"][b, :cut], p["V"][b, :cut]) and torch.isnan(p["v_pre"][b, cut:]).all()
            if j >= 8:
                assert order[cut:] == p["order"][b][cut:][::-1]
            seen.add((cut == 0, cut == n, n - cut == 0 and cut == 0))
    assert {(True, False, False), (False, True, False), (True, True, True), (False, False, False)} <= seen


# ---- power: three wrong evaluations must miss the gate -------------------------------------------------------------------------
def _wrong_output(cs, d, mode):
    """fp32 O of a deliberately wrong evaluation.  ``max_over_all``: the logits a = s + log w of EVERY key below the count enter the
    running maximum (as fmaxf takes it: a NaN is passed over), whatever the weight; only the admissible keys enter the sum -- and a
    query whose sum is 0 gets zeros, as in the kernel.  ``weight_outside``: w exp(s - max s) in the place of exp(s + log w - m)."""
    scale = 1.0 / math.sqrt(d)
    O = torch.zeros_like(cs.Q)
    for b, n in enumerate(cs.counts):
        idx = cs.adm[b].nonzero().flatten()
        if idx.numel() == 0:
            continue
        q, k, v, w = cs.Q[b], cs.K[b, idx], cs.V[b, idx], cs.W[b, idx]
        s = q @ k.T * scale
        if mode == "max_over_all":
            a_all = cs.Q[b] @ cs.K[b, :n].T * scale + torch.log(cs.W[b, :n])
            m = torch.where(torch.isnan(a_all), torch.full_like(a_all, -math.inf), a_all).max(-1, keepdim=True).values
            p = torch.exp(s + torch.log(w) - m)
        else:
            p = w * torch.exp(s - s.max(-1, keepdim=True).values)
        l = p.sum(-1, keepdim=True)
        O[b] = torch.where(l > 0, (p @ v) / l, torch.zeros_like(l))
    return O


@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("regime", ("huge_pos", "one_key@first", "one_key@last", "one_key@edge"))
def test_a_maximum_over_inadmissible_keys_misses_the_gate(regime, d, C_pad):
    """(i) Where the top key carries +Inf the wrong maximum is +inf and every probability 0.  (A finite score that only enters the
    maximum is harmless up to a gap of 87, and no regime here is built wider.)"""
    cs, r64, r32 = references(("drop_top", regime, ""), d, C_pad)
    wrong = _wrong_output(cs, d, "max_over_all")
    assert misses(wrong, r64[0], r32[0], 1e-5)
    assert not misses(r32[0], r64[0], r32[0], 1e-5)  # (the gate passes what it should)


@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
def test_the_weight_outside_the_exponential_misses_the_gate(d, C_pad):
    """(ii) exp(s - max s) of a key 112 below the top is 0 in fp32 before its weight of 2e24 can restore it."""
    cs, r64, r32 = references(("counter", "ascending_wide", ""), d, C_pad)
    assert misses(_wrong_output(cs, d, "weight_outside"), r64[0], r32[0], 1e-5)
    assert not misses(_wrong_output(cs, d, "max_over_all"), r64[0], r32[0], 1e-5)  # (no key is removed: this one is right here)


@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("regime", WC.PATTERN_REGIMES["wide"])
def test_a_weight_gradient_without_the_division_misses_the_gate(regime, d, C_pad):
    """(iii) d_w = sum_q dA without / w, on the gate of d_w (1e-4) and on that of w * d_w."""
    cs, r64, r32 = references(("wide", regime, ""), d, C_pad)
    w = cs.finite_weights()
    wrong = r32[4] * w  # (sum_q dA of the fp32 evaluation)
    assert misses(wrong, r64[4], r32[4], 1e-4)
    assert misses(wrong.double() * w.double(), r64[4] * w.double(), r32[4].double() * w.double(), 1e-4)
    assert not misses(r32[4], r64[4], r32[4], 1e-4)


# ---- factor coverage -----------------------------------------------------------------------------------------------------------
def test_every_pattern_meets_every_shape_and_both_key_blocks():
    assert {MC.key_block(d) for d, _ in WC.SHAPES} == {16, 32}
    assert set(WC.PATTERN_REGIMES) == {"drop_top", "counter", "wide", "holes"} == {c[0] for c in WC.CASES}
    for pattern, regimes in WC.PATTERN_REGIMES.items():
        variants = WC.HOLE_VARIANTS if pattern == "holes" else ("",)
        assert {(p, r, v) for p, r, v in WC.CASES if p == pattern} == {(pattern, r, v) for r in regimes for v in variants}
    ids = [WC.case_id(c) for c in WC.CASES]
    assert len(set(ids)) == len(ids) == 26
    # (every test of the two modules is parametrised over CASES x SHAPES)
    assert {v for p, _, v in WC.CASES if p == "holes"} == set("abcdefg")
    assert {(p, v, r) for p, v, r in WC.MEAN_CASES} == {(p, v, r) for r in ("normal", "offset") for p, vs in
                                                         (("wide", ("",)), ("holes", tuple("abcdefg"))) for v in vs}


# ---- the weighted mean ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", WC.MEAN_WIDTHS)
@pytest.mark.parametrize("case", [pytest.param(c, id="-".join(x for x in c if x)) for c in WC.MEAN_CASES])
def test_mean_references_are_finite_and_the_rounded_mean_costs_the_offset_regime_its_digits(case, F):
    """Float64 out, dR and dW are finite and moderate.  And what the GPU test of the offset regime is there for: d_w =
    <d_out, r - out> / W evaluated in float64 throughout but with ``out`` rounded to fp32 first misses 1e-6 of max|d_w| of a task
    where the values are 1e3 + 1e-3 randn (1e3 * 2^-24 against a spread of 1e-3), and does not where they are randn."""
    R, W, dOut, counts, adm, dead = WC.make_mean(case, F)
    out, dR, dW = KR.weighted_mean_and_grads(R, W, dOut, counts, torch.float64)
    assert all(torch.isfinite(x).all() and float(x.abs().max()) <= BIG for x in (out, dR, dW))
    assert not dR[~adm].any() and not dW[~adm].any()
    worst = 0.0
    for b in range(len(counts)):
        idx = adm[b].nonzero().flatten()
        if idx.numel() < 2:
            continue
        rounded = ((R[b, idx].double() - out[b].float().double()) @ dOut[b].double()) / W[b, idx].double().sum()
        worst = max(worst, float((rounded - dW[b, idx]).abs().max() / dW[b].abs().max()))
    if case[1] == "e":
        assert worst == 0.0
    elif case[2] == "offset" and case[1] not in ("c", "d"):
        assert worst > 1e-4, worst
    elif case[2] == "normal":
        assert worst < 1e-6, worst
