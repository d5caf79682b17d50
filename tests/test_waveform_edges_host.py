"""The inputs of the waveform edge suite (tests/waveform_edge_cases.py) on the CPU, against the float64 references alone: every case
claims what its family says -- a clear maximum wherever there is a choice, bit-equal columns where a tie is planted, the stated
constants where the correlation vanishes, mismatches of 1e-4 .. 1e-8 in the near-match family, invariance under the exact scalings
-- the near-match gate leaves the recurrence form a margin of ten and tells two wrong evaluations apart that the existing gate lets
through, and every family meets every entry point and shape listed for it.  Nothing here reads a kernel's result."""
import math

import pytest
import torch

import match_reference as M
import mismatch_reference as G
import waveform_edge_cases as W

FAMILY_ENTRY = [(f, e) for f, entries in W.FAMILIES.items() for e in entries if e != "grad"]
_refs = {}


def references(family, entry):
    """[(tag, factors, case, reference)] of a family and entry point, computed once and shared (never modified)."""
    key = (family, W._kind(entry))
    if key not in _refs:
        _refs[key] = [(tag, fac, case, W.reference(key[1], case)) for tag, fac, case in W.cases(family, entry)]
    return _refs[key]


def f32_sincos(x):
    """Sine and cosine rounded to float32 after a float64 range reduction (the wrong evaluation of tests/test_match_host.py)."""
    y = torch.remainder(x, M.TWO_PI).float()
    return torch.sin(y).double(), torch.cos(y).double()


def gap_of(kind, ref):
    """The smallest distance between the best and the runner-up candidate over the live rows, on the scale of the existing
    criterion: normalised |c| for the match, x / sqrt(hh dd) for the likelihoods.  inf without a choice."""
    live = ~ref["degenerate"]
    cand = ref["mag"] if kind == "match" else ref["x"]
    if cand.shape[1] < 2 or not live.any():
        return math.inf
    top = cand[live].topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    if kind != "match":
        gap = gap / (ref["hh"] * ref["dd_rows"]).sqrt()[live]
    return float(gap.min())


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_every_family_meets_its_entry_points_and_shapes():
    for family, entries in W.FAMILIES.items():
        for entry in entries:
            assert len(W.cases(family, entry)) >= 2, (family, entry)
    for entry in W.ENTRIES:
        facs = [fac for _, fac, _ in W.cases("thread_edges", entry)]
        assert {f["T"] for f in facs} == set(W.EDGE_T)
        for T in W.EDGE_T:
            mine = [f for f in facs if f["T"] == T]
            assert {f["counts"] is None for f in mine} == {True, False}, T
            assert {f["regime"] for f in mine} == {"random", "removed", "shift"}, T
            assert {f["n_tau"] for f in mine} == ({None, 1} if T == 1 else {None, 17, 257}), T
            for f in mine:
                assert f["counts"] in (None, (T, T - 1, min(17, T)), (T, min(128, T), 0)), (T, f["counts"])
                assert f["wform"] == f["fform"] == "BT" or f["regime"] != "removed", T
        assert {f["counts"] for f in facs} >= {None, (257, 256, 17), (257, 128, 0), (129, 128, 17), (65, 65, 0)}
        assert {f["n_z"] for f in facs} == {1, 3} and {f["h_ld"] for f in facs} == {2, 4}
        if entry == "net":
            assert {f["D"] for f in facs} == {1, 8} and {(f["T"], f["D"]) for f in facs} >= {(T, D) for T in W.EDGE_T for D in (1, 8)}
        grids = [(f["regime"], f["n_tau"], c.get("j_star")) for _, f, c in W.cases("long_grids", entry)]
        assert set(grids) == {("shift", n, j) for n in W.LONG_GRIDS for j in (n - 1, 992, 991)} | {("random", n, None) for n in W.LONG_GRIDS}
        assert all(f["T"] == 37 and f["n_z"] == 3 and f.get("D", 2) == 2 for _, f, _ in W.cases("long_grids", entry))
        tie = [f for _, f, _ in W.cases("ties", entry)]
        assert {(f["T"], f["n_tau"]) for f in tie} == {(T, n) for T in (37, 129) for n in (17, 257, 1000)}
        assert {f["wform"] for f in tie} == {None, "BT"} and {f["counts"] is None for f in tie} == {True, False}
        assert all(float(c["freqs"].abs().max()) == 0 and c.get("delays") is None for _, _, c in W.cases("ties", entry))
    longs = W.cases("long_rows", "match")
    assert [(f["regime"], f["T"], f["n_tau"], f["n_z"], f["counts"]) for _, f, _ in longs] == \
        [(r, 256 * 1024 + 37, 5, 1, (256 * 1024 + 37, 256 * 1024 + 1, 256 * 1024)) for r in ("shift", "random")]
    assert longs[0][2]["j_star"] == 3
    near = [f for _, f, _ in W.cases("near_match", "match")]
    assert {(f["eps"], f["T"], f["n_tau"]) for f in near} == {(e, T, n) for e in W.NEAR_EPS for T in (129, 257) for n in (None, 17, 257)}
    assert all(f["n_z"] == 3 and f["wform"] == f["fform"] == "BT" for f in near)
    assert [(f["T"], f["regime"]) for _, f, _ in W.cases("scaled", "match")] == [(65, "random"), (129, "removed"), (257, "random")]
    assert set(W.SEED_SHIFT) == {("thread_edges", "match", 70)}  # (the one case that needed another seed)


# ---- a clear maximum wherever there is a choice ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,entry", [fe for fe in FAMILY_ENTRY if fe[0] not in ("ties", "zero_corr")])
def test_every_grid_case_has_a_clear_maximum_and_finds_what_is_planted(family, entry):
    """The runner-up lies at least 1e-6 below the best in every live row of every case with a choice to make (the criterion of the
    feature suites); the planted index is the reference's; every reference value is finite."""
    closest = math.inf
    for tag, fac, case, ref in references(family, entry):
        for k in ("match", "overlap", "phase", "corr") if entry == "match" else ("lnl_max", "lnl_marg", "snr", "phase", "series"):
            assert torch.isfinite(ref[k]).all(), (tag, k)
        gap = gap_of(entry, ref)
        closest = min(closest, gap)
        assert gap >= 1e-6, (tag, gap)
        live = ~ref["degenerate"]
        if fac["regime"] == "shift":
            assert live.any() and (ref["tau_index"][live] == case["j_star"]).all(), tag
        if fac["counts"] is not None and fac["counts"][2] == 0:
            assert ref["degenerate"].view(fac["n_z"], W.B)[:, 2].all(), tag  # the task with a count of 0
    print(f"EDGES {family} {entry}: smallest gap between the best and the runner-up {closest:.3e}")


def test_long_rows_have_the_stated_gaps_and_the_recurrence_meets_the_match_gates():
    for tag, fac, case, ref in references("long_rows", "match"):
        rec = W.recurrence("match", case)
        r = M.ratios({k: rec[k] for k in ("overlap", "match", "mismatch", "corr", "hh", "gg", "phase", "tau_index")}, ref)
        print(f"EDGES long_rows {tag}: gap {gap_of('match', ref):.3e}; recurrence error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (tag, r)
        dM, s = G.closed_form(**M.call_args(case), ref=ref)
        assert torch.isfinite(dM).all() and float(dM.abs().max()) > 0
        beyond = torch.arange(fac["T"]).view(1, -1) >= torch.tensor(fac["counts"]).view(-1, 1)
        assert (dM[beyond] == 0).all() and (s[beyond] == 0).all() and int(beyond.sum()) == 36 + 37


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("match", "loglike", "net"))
def test_zero_frequencies_give_bit_equal_columns_in_the_recurrence_form(entry):
    """What the kernel forms (one sincos at every chunk's first shift, then rotations by (1, 0)) gives the same bits at every grid
    time; the reference of the same inputs without a grid is finite and, where a task has points, not degenerate."""
    for tag, fac, case, _ in references("ties", entry):
        rec = W.recurrence(entry, case)
        cols = rec["corr"] if entry == "match" else rec["series"]
        assert cols.shape[1] == fac["n_tau"], tag
        if entry == "net":
            # the detectors' sums are bit-equal; K = sum_k C_k kappa_k is formed here by torch's vectorised complex product, whose
            # body and tail round differently (the kernel forms every component by the same two products), so K to 1e-15 only
            kap = rec["kappa_det"]
            assert torch.equal(kap, kap[..., :1].expand_as(kap)), tag
            assert float((cols - cols[:, :1]).abs().max()) <= 1e-15 * max(1.0, float(cols.abs().max())), tag
        else:
            assert torch.equal(cols, cols[:, :1].expand_as(cols)), tag
            assert (rec["tau_index"] == 0).all(), tag
        ref0 = W.reference(entry, case, taus=None)
        for k in ("match", "overlap", "phase", "corr") if entry == "match" else ("lnl_max", "lnl_marg", "snr", "phase", "series"):
            assert torch.isfinite(ref0[k]).all(), (tag, k)
        deg = ref0["degenerate"].view(fac["n_z"], W.B)
        assert not deg[:, :2].any() and bool(deg[:, 2].all()) == (fac["counts"] is not None), tag
        d = (cols[:, 0] - (ref0["corr"] if entry == "match" else ref0["series"])[:, 0]).abs().max()
        assert float(d) <= 1e-12 * max(1.0, float(cols.abs().max())), (tag, float(d))


# ---- vanishing correlations ----------------------------------------------------------------------------------------------------------
def test_cancelling_points_leave_a_live_row_with_no_correlation():
    for tag, fac, case, ref in references("zero_corr", "match"):
        assert not ref["degenerate"].any() and float(ref["hh"].min()) > 0 and float(ref["gg"].min()) > 0, tag
        assert (ref["mag"] == 0).all() and (ref["match"] == 0).all() and (ref["mismatch"] == 1).all() and (ref["tau_index"] == 0).all(), tag
        assert (ref["overlap"] == 0).all() and (ref["corr"] == 0).all(), tag
        rec = W.recurrence("match", case)
        assert (rec["mag"] == 0).all(), tag  # (the kernel's form cancels exactly as well)
        a = case["h"][:, list(fac["live"]), 0].double() * case["g"][:, list(fac["live"]), 0].double().repeat(fac["n_z"], 1)
        assert (a[:, 0] == -a[:, 1]).all() and (a[:, 0] != 0).all(), tag


@pytest.mark.parametrize("entry", ("loglike", "net"))
def test_zero_data_give_the_stated_constants(entry):
    for tag, fac, case, ref in references("zero_corr", entry):
        live = ~ref["degenerate"]
        assert live.any() and (ref["x"] == 0).all() and (ref["dd"] == 0).all(), tag
        assert torch.equal(ref["lnl_max"], -0.5 * ref["hh"]), tag
        # (logsumexp of n equal values minus ln n: the reference rounds twice, the kernel's exp(0) sum to n exactly)
        assert float((ref["lnl_marg"] + 0.5 * ref["hh"]).abs().max()) <= 1e-14 * max(1.0, float(ref["hh"].max())), tag
        assert (ref["snr"] == 0).all() and (ref["tau_index"] == 0).all() and float(ref["hh"][live].min()) > 0, tag
        if entry == "net":
            assert (ref["snr_det"] == 0).all() and (ref["hh_det"][live] > 0).all(), tag


# ---- the near-match regime and its gate ----------------------------------------------------------------------------------------------
def test_near_match_mismatches_lie_where_the_family_says():
    band = {1e-2: (3e-5, 3e-4), 1e-3: (3e-7, 3e-6), 1e-4: (3e-9, 3e-8)}
    seen = {}
    for tag, fac, case, ref in references("near_match", "match"):
        lo, hi = float(ref["mismatch"].min()), float(ref["mismatch"].max())
        seen[fac["eps"]] = (min(lo, seen.get(fac["eps"], (1.0, 0.0))[0]), max(hi, seen.get(fac["eps"], (1.0, 0.0))[1]))
        assert band[fac["eps"]][0] <= lo and hi <= band[fac["eps"]][1], (tag, lo, hi)
        if fac["n_tau"] is not None:
            assert (ref["tau_index"] == 2).all(), tag  # (tau = 0 of the grid)
    print("EDGES near_match reference mismatches: " + ", ".join(f"eps={e:g}: {lo:.3e} .. {hi:.3e}" for e, (lo, hi) in seen.items()))


def test_near_match_gate_passes_the_recurrence_and_fails_two_wrong_evaluations():
    """Against ``|d| <= 2^-23 |ref| + 16 T 2^-53``: the float64 recurrence form stays below a tenth of the gate on every case; the
    recurrence with float32 sines, and ``1 - float32(match)`` in place of ``float32(1 - match)``, miss it on every case."""
    worst, low_span, cast_span = 0.0, [math.inf, 0.0], [math.inf, 0.0]
    for tag, fac, case, ref in references("near_match", "match"):
        T = fac["T"]
        r = max(W.near_ratios(W.recurrence("match", case), ref, T).values())
        worst = max(worst, r)
        assert r <= 0.1, (tag, r)
        low = max(W.near_ratios(W.recurrence("match", case, sincos=f32_sincos), ref, T).values())
        cast = W.near_ratios(dict(mismatch=1.0 - ref["match"].float().double()), ref, T)["mismatch"]
        assert low > 1.0 and cast > 1.0, (tag, low, cast)
        low_span, cast_span = [min(low_span[0], low), max(low_span[1], low)], [min(cast_span[0], cast), max(cast_span[1], cast)]
        right = W.near_ratios(dict(mismatch=(1.0 - ref["match"]).float()), ref, T)["mismatch"]  # (the right rounding passes)
        assert right <= 1.0, (tag, right)
    print(f"EDGES near_match gate: recurrence {worst:.3g}; float32 sines {low_span[0]:.3g} .. {low_span[1]:.3g}; "
          f"1 - float32(match) {cast_span[0]:.3g} .. {cast_span[1]:.3g}")


def test_the_existing_gate_lets_the_wrong_mismatch_rounding_through():
    """Why the near-match family is needed: on the "same" and "random" cases of the feature suite ``1 - float32(match)`` stays inside
    ``1e-9 + 2^-23 |ref|`` -- exact at match = 1, one rounding of a match of ~0.1 elsewhere."""
    worst, n = 0.0, 0
    for tag, fac, case in M.cases(W.JC):
        if fac["regime"] not in ("same", "random"):
            continue
        ref = M.reference(**M.call_args(case))
        r = M.ratios(dict(mismatch=1.0 - ref["match"].float().double()), ref)["mismatch"]
        worst, n = max(worst, r), n + 1
        assert r <= 1.0, (tag, r)
    assert n >= 28
    print(f"EDGES 1 - float32(match) against the existing gate on {n} feature-suite cases: {worst:.3g}")


# ---- exact scalings ------------------------------------------------------------------------------------------------------------------
def test_scaled_references_equal_the_unscaled_ones():
    for tag, fac, case, ref in references("scaled", "match"):
        base = M.reference(**M.call_args(fac["base"]))
        assert torch.equal(ref["tau_index"], base["tau_index"]) and torch.equal(ref["degenerate"], base["degenerate"]), tag
        for k in ("match", "overlap", "phase"):
            assert float((ref[k] - base[k]).abs().max()) <= 1e-15, (tag, k)
        assert gap_of("match", ref) >= 1e-6, tag
        hh_fac, gg_fac = fac["s_w"] * fac["s_h"] ** 2, fac["s_w"] * fac["s_g"] ** 2
        assert torch.equal(ref["hh"], base["hh"] * hh_fac) and torch.equal(ref["gg"], base["gg"] * gg_fac), tag
        assert 2.0 ** -120 < float(ref["hh"][~ref["degenerate"]].min()) and float(ref["hh"].max()) < 2.0 ** 110, tag
        assert 2.0 ** -120 < float(ref["gg"][ref["gg"] > 0].min()) and float(ref["gg"].max()) < 2.0 ** 110, tag
