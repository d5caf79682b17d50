"""The inputs of the distance-marginalised likelihood's edge suite (tests/loglike_dist_edge_cases.py) on the CPU, against the float64
reference alone: the size lists hold the kernels' own constants, every family holds the cases it names, ``scale_index`` is well
posed wherever the GPU test asserts it exactly (1e3 gates between the best and the runner-up, or between a planted tie set and the
next distinct value), the kernel's one-pass form in float64 meets 1e-2 of every gate on every case -- so a correct kernel can meet
the gates, the 1e6, tiny-scale and wide-grid cases included -- and the regimes reach what they aim at.  Nothing here reads a kernel's
result."""
import math
import os
import re

import pytest
import torch

import loglike_dist_edge_cases as E
import loglike_dist_reference as Dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(family, network) for family in E.FAMILIES for network in E.streams(family)]
IDS = [f"{f}-{'network' if n else 'single'}" for f, n in ALL]


def _rows(family, network):
    """[(tag, factors, case, scales, log_prior, parent reference, marginalised reference)] of a family (the references are cached)."""
    return [(tag, fac, case, s, p, *E.reference(network, case, s, p, no_grid=family == "shift_ties"))
            for tag, fac, case, s, p in E.cases(family, network)]


# ---- the edges are the kernels' own ------------------------------------------------------------------------------------------------
def test_the_size_lists_hold_the_constants_of_the_kernels():
    from npf_gwwaveform_amd import functional as FN

    csrc = os.path.join(ROOT, "npf_gwwaveform_amd", "csrc")
    dist = open(os.path.join(csrc, "waveform_dist_kernels.hip")).read()
    common = open(os.path.join(csrc, "waveform_common.hpp")).read()
    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    assert int(re.search(r"constexpr int kWfDistLdsTau = (\d+);", dist).group(1)) == E.LDS_TAU
    assert int(re.search(r"constexpr int kWfLlThreads = (\d+);", common).group(1)) == E.THREADS
    assert int(re.search(r"#define NPF_NET_MAX_DET (\d+)", header).group(1)) == E.MAX_DET
    assert FN.DIST_MAX_SCALES == E.MAX_SCALES and FN.DIST_SC == E.SC == Dd.SC and FN.LOGLIKE_I0_SWITCH == E.I0_SWITCH
    assert re.search(r"dim3\(kWfLlThreads\)", dist) and re.search(r"n <= kWfDistLdsTau", dist)  # both launches and the LDS rule use them
    assert E.A_SIZES == (E.THREADS - 1, E.THREADS, E.LDS_TAU - 1, E.LDS_TAU, E.LDS_TAU + 1) and E.A_LAST == 4099
    assert E.B_SIZES == (E.THREADS - 1, E.THREADS, E.MAX_SCALES - 1, E.MAX_SCALES)
    assert E.LDS_TAU * 8 == 32 * 1024 and E.MAX_SCALES // E.SC == 256  # the largest dynamic-LDS request; chunks in gridDim.y
    assert E.FLAT_N_TAU[-1] == E.LDS_TAU + 1


def test_every_family_holds_the_cases_it_names():
    for network in (False, True):
        a = [f for _, f, *_ in E.cases("time_edges", network)]
        want = {(n, r) for n in E.A_SIZES for r in ("planted", "noise")} | {(n, r) for n in (4096, 4097) for r in ("removed", "degenerate")}
        assert {(f["n_tau"], f["regime"]) for f in a} == want | {(4097, "loud"), (4099, "planted")}
        assert all(f["n_a"] == E.SC + 1 for f in a) and {f["sform"] for f in a} == {f["pform"] for f in a} == {"A", "BA"}
        assert all(f["counts"] == (E.T, 17, 0) and f["n_z"] == 3 for f in a if f["regime"] in ("removed", "degenerate"))
        last = E.cases("time_edges", network)[-1]
        assert last[1]["n_tau"] == 4099 and last[2]["j_star"] == 4098 and last[1]["n_z"] == 3
        b = [f for _, f, *_ in E.cases("scale_edges", network)]
        assert {(f["n_a"], f["n_tau"], f["kind"]) for f in b} == {(n, t, k) for n in E.B_SIZES for t, ks in E.B_KINDS.items() for k in ks}
        assert {k for ks in E.B_KINDS.values() for k in ks} == {"geo", "dead", "dead_last", "dead_first", "rev"}
        c = [f for _, f, *_ in E.cases("duplicated_best", network)]
        assert {(f["set"], f["sform"]) for f in c} == {(s, form) for s in E.TIE_SETS for form in ("A", "BA")} and all(f["n_a"] == 300 for f in c)
        flat = [f for _, f, *_ in E.cases("flat_evidence", network)]
        assert {(f["n_a"], f["n_tau"]) for f in flat} == {(n, t) for n in (2, 17, 257) for t in (None, 17, 4097)}
        assert {f["n_tau"] for _, f, *_ in E.cases("shift_ties", network)} == {17, 257, 1000}
        d = [f for _, f, *_ in E.cases("magnitudes", network)]
        assert [f["sub"] for f in d] == ["u1e6", "u1e6", "tiny", "tiny", "wide", "wide", "switch"]
        assert {f["regime"] for f in d if f["sub"] == "tiny"} == {"noise", "planted"}
        assert all((f["T"], f["n_tau"], f["n_z"], f["n_a"]) == (200, 17, 3, 65) for f in d if f["sub"] == "u1e6")
        assert {(f["regime"], f["perm"]) for _, f, *_ in E.cases("mixture_orders", network)} == \
            {(r, perm) for r in ("loud", "edge") for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))}
        for _, f, case, s, p in (row for family in E.FAMILIES if network in E.streams(family) for row in E.cases(family, network)):
            assert case["h"].shape[0] == f["n_z"] * E.B and f["n_z"] <= 3 and f["T"] in (37, 200)
            n = f["n_tau"] or 1
            assert f["n_z"] * E.B * f["n_a"] * n <= 1.1e6 or (f["n_a"], f["n_tau"]) == (257, 4097)  # (that one: evaluated in chunks)
            assert not (n > 4096 and f["n_a"] > 33 and f["regime"] != "degenerate") and not (f["n_a"] == 4096 and n > 17)
            if network:
                assert case["data"].shape[1] == f["D"]
    f8 = [f for _, f, *_ in E.cases("eight_detectors", True)]
    assert {(f["regime"], f["n_tau"]) for f in f8} == {(r, t) for r in ("noise", "planted") for t in (17, 4097)}
    assert all(f["D"] == 8 and f["n_a"] == 17 for f in f8)
    # the tie sets isolate the levels of launch B's reduction (thread = i mod 256, lane = thread mod 64, wave = thread / 64)
    thread, wave = (lambda i: i % E.THREADS), (lambda i: (i % E.THREADS) // 64)
    sets = dict(zip(("thread", "lanes32", "lanes", "neighbours", "waves", "later_wave", "three"), E.TIE_SETS))
    assert thread(sets["thread"][0]) == thread(sets["thread"][1])
    for k in ("lanes32", "lanes", "neighbours"):
        i, j = sets[k]
        assert wave(i) == wave(j) and thread(i) != thread(j)
    assert sets["lanes32"][1] - sets["lanes32"][0] == 32 and sets["neighbours"][1] - sets["neighbours"][0] == 1
    assert wave(sets["waves"][0]) < wave(sets["waves"][1])
    assert wave(200) > wave(257) and wave(70) > wave(299) and wave(130) > wave(299)  # the smaller index sits in the later wave
    # every member in another chunk of launch A, but for the two neighbours, which share one
    assert all(len({i // E.SC for i in s}) == (1 if s == sets["neighbours"] else len(s)) for s in E.TIE_SETS)


def test_chunked_reference_is_the_reference():
    tag, fac, case, s, p = E.cases("scale_edges", False)[4]
    ref = E.parent_reference(False, case)
    whole, parts = Dd.marginalise(ref, s, p), E.marginalise(ref, s, p, limit=ref["x"].numel() * 37)
    for k, v in whole.items():
        assert torch.equal(v.nan_to_num(7.0), parts[k].nan_to_num(7.0)), k


# ---- scale_index is well posed where it is asserted --------------------------------------------------------------------------------
def _wide_or_switch(fac):
    return fac.get("sub") in ("wide", "switch")


@pytest.mark.parametrize("family,network", ALL, ids=IDS)
def test_every_case_leaves_scale_index_well_posed(family, network):
    """1e3 gates between the best and the runner-up on every row with a live scale (``loglike_dist_reference.runner_up_in_gates``).
    A planted tie set counts as one value: its members lie within 1e-2 gates of each other in the reference and the next distinct
    value 1e3 gates below.  Flat evidence ties everywhere by construction (within 1e-2 gates).  The wide grid cannot meet the row
    gate (its S_r is that of a = 2^30; the evidence near the maximum is of order 1): it must meet the per-scale margin of
    ``loglike_dist_edge_cases.per_scale_margin``; the GPU test also asserts the fallback there.  The switch-point case is held to
    the same 1e3 (its maximum falls on a plain scale, clear of the 17 near-equal ones), so the GPU test asserts its index exactly."""
    closest = math.inf
    for tag, fac, case, s, p, ref, dist in _rows(family, network):
        rows = dist["live"].any(1)
        gate = (1e-10 * dist["S"] + 1e-12).view(-1, 1)
        u = dist["u"]
        if family == "flat_evidence":
            assert rows.all() and float(((u - u[:, :1]).abs() / gate).max()) <= 1e-2, tag
            continue
        if family == "duplicated_best":
            members = list(fac["set"])
            inside = u[:, members]
            assert float(((inside - inside[:, :1]).abs() / gate).max()) <= 1e-2, tag
            rest = u.clone()
            rest[:, members] = -math.inf
            g = float(((inside.min(1).values - rest.max(1).values) / gate.view(-1)).min())
            assert (u.max(1).values == inside.max(1).values).all(), tag
        elif fac.get("sub") == "wide":
            assert float(Dd.runner_up_in_gates(dist)[rows].max()) < 1.0, tag  # (the row gate says nothing here)
            g = float(E.per_scale_margin(ref, dist, s, p)[rows].min())
        else:
            g = float(Dd.runner_up_in_gates(dist)[rows].min())
        if fac.get("sub") == "switch":
            print(f"LOGLIKE_DIST_EDGES {tag}: the gap at the switch point, in gates: {g:.4g}")
        closest = min(closest, g)
        assert g >= 1e3, (tag, g)
    print(f"LOGLIKE_DIST_EDGES {family} {'network' if network else 'single'}: smallest gap best - runner-up, in gates: {closest:.4g}")


@pytest.mark.parametrize("family,network", ALL, ids=IDS)
def test_one_pass_form_meets_a_hundredth_of_every_gate(family, network):
    worst = 0.0
    for tag, fac, case, s, p, ref, dist in _rows(family, network):
        op = Dd.one_pass(ref, s, p)
        gate = 1e-10 * dist["S"] + 1e-12
        for name, g in (("u", gate.view(-1, 1).expand_as(dist["u"])), ("lnl_dist", gate)):
            x, r = op[name], dist[name]
            assert torch.equal(x == -math.inf, r == -math.inf) and not torch.isnan(x).any() and not torch.isnan(r).any(), (tag, name)
            fin = torch.isfinite(r)
            q = float(((x[fin] - r[fin]).abs() / g[fin]).max()) if fin.any() else 0.0
            worst = max(worst, q)
            assert q <= 1e-2, (tag, name, q)
    print(f"LOGLIKE_DIST_EDGES {family} {'network' if network else 'single'}: one-pass form vs direct log-sum-exp, worst error / gate {worst:.3g}")


# ---- the regimes reach what they aim at ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_regime_claims_hold_in_the_reference(network):
    # A: the planted maximiser stands where it was planted (the last index of the 4099 grid: the last chunk of launch 1); "loud" at
    # 4097: every term of S_i but a few underflows
    for tag, fac, case, s, p, ref, dist in _rows("time_edges", network):
        if fac["regime"] == "planted":
            assert (ref["tau_index"] == case["j_star"]).all(), tag
        if fac["regime"] == "loud":
            a = Dd._per_row(s, E.B, ref["x"].shape[0])
            arg = a.max(1).values.view(-1, 1) * (ref["x"] - ref["x"].max(1, keepdim=True).values)
            assert ((arg > -745).sum(1) <= 8).all(), tag  # (of 4097 terms at the largest scale)
        if fac["regime"] in ("removed", "degenerate"):
            assert ref["degenerate"].any() and (fac["regime"] == "degenerate" or not ref["degenerate"].all()), tag
    # B: a dead chunk holds -inf and the index skips it; "rev" puts the maximum at the last index
    for tag, fac, case, s, p, ref, dist in _rows("scale_edges", network):
        n_a, idx = fac["n_a"], dist["scale_index"]
        if fac["kind"] == "dead_last":
            assert (dist["post"][:, E.SC * ((n_a - 1) // E.SC):] == -math.inf).all() and (idx == 0).all(), tag
        if fac["kind"] == "dead_first":
            assert (dist["post"][:, :E.SC] == -math.inf).all() and (idx == E.SC).all(), tag
        if fac["kind"] == "rev":
            assert (idx == n_a - 1).all(), tag
        if fac["kind"] == "dead":
            assert (~dist["live"][:, [1, 2, 3, 5, 7, 9, 11]]).all() and dist["live"][:, 0].all(), tag
    # C: flat evidence has HH == 0 on every row; every shift of the tie grids gives the same x (to rounding, in the reference)
    for tag, fac, case, s, p, ref, dist in _rows("flat_evidence", network):
        assert (ref["hh"] == 0).all() and ref["degenerate"].all() and float((dist["lnl_dist"] - (E.FLAT_LP + math.log(fac["n_a"]))).abs().max()) <= 1e-14
    for tag, fac, case, s, p in E.cases("shift_ties", network):
        x = E.parent_reference(network, case)["x"]
        assert x.shape[1] == fac["n_tau"] and float(((x - x[:, :1]).abs() / x[:, :1].clamp_min(1e-300)).max()) <= 1e-13, tag
        assert float(case["freqs"].abs().max()) == 0
    # D
    for tag, fac, case, s, p, ref, dist in _rows("magnitudes", network):
        u, live = dist["u"], dist["live"]
        a = Dd._per_row(s, E.B, u.shape[0])
        if fac["sub"] == "u1e6":
            assert float(u.max(1).values.min()) > 1e6 and 2e6 < float(ref["hh"].max()) < 3e6, (tag, float(u.max()), float(ref["hh"].max()))
        if fac["sub"] == "tiny":
            live_rows = ~ref["degenerate"]
            assert float((a[live_rows] ** 2 * ref["hh"][live_rows].view(-1, 1)).max()) < 2.0 ** -34 and float((a ** 2).min()) == 0.0, tag
            assert torch.isfinite(u).all(), tag
        if fac["sub"] == "wide":
            assert float((0.5 * a ** 2 * ref["hh"].view(-1, 1)).max()) > 1e18 and torch.isfinite(u).all(), tag
            assert float(u.max() - u.min()) > 1e18 and torch.isfinite(a * ref["x"].max(1).values.view(-1, 1)).all(), tag
        if fac["sub"] == "switch":
            xb = ref["x"].max(1).values
            arg = (a * xb.view(-1, 1))[:, 4:4 + len(E.SWITCH_K)]
            assert float((arg / E.I0_SWITCH - 1.0).abs().max()) <= 2.0 ** -46, tag
            assert ((arg < E.I0_SWITCH).any(1) & (arg >= E.I0_SWITCH).any(1)).all(), tag
            assert fac["n_z"] == 1 and s.shape == (E.B, 9 + len(E.SWITCH_K))
    # E: the rows of a task lie more than 745 apart and the top block stands first, in the middle and last
    # (and in the "edge" orders the rows lie within 40 of each other: every row counts in the mixture, whichever comes first)
    where, near = set(), set()
    for tag, fac, case, s, p, ref, dist in _rows("mixture_orders", network):
        v = dist["lnl_dist"].view(3, E.B)
        srt = v.sort(0).values
        top = v.argmax(0)
        if not fac["apart"]:
            task_gate = (1e-10 * dist["S"] + 1e-12).view(3, E.B).max(0).values  # (what the rows below the top add: 1e3 gates and more)
            assert float((srt[-1] - srt[0]).max()) < 40 and float(((dist["lnl_dist_mix"] - (v.max(0).values - math.log(3.0))) / task_gate).min()) >= 1e3, tag
            near |= {tuple(v[:, b].argsort().tolist()) for b in range(E.B)}
            continue
        assert float((srt[1:] - srt[:-1]).min()) > 745, (tag, v)
        assert (top == top[0]).all() and fac["perm"][int(top[0])] == 0, tag  # (the block of template factor 1.0)
        where.add(int(top[0]))
        assert float((dist["lnl_dist_mix"] - (v.max(0).values - math.log(3.0))).abs().max()) == 0.0, tag
    assert where == {0, 1, 2} and len(near) == 6
