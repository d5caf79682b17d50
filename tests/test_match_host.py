"""Host side of the waveform match (CPU, no kernel launched): the C ABI of ``npf_waveform_match``, its refusals and those of
``functional.waveform_match`` / ``HeadDistribution.match``, and the float64 reference of tests/match_reference.py itself --
Cauchy-Schwarz, the recurrence form against the direct form, what fp32 sines would cost, the planted time shift, the runner-up
margin of every input set the GPU test uses, and removed points against cut ones."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import match_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC = 16


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    assert FN.MATCH_JC == JC
    cases = R.cases(FN.MATCH_JC)
    return [(tag, fac, case, R.reference(**R.call_args(case))) for tag, fac, case in cases]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_waveform_match_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    m = re.search(r"\bint\s+npf_waveform_match\s*\(([^;]*)\)\s*;", header)
    assert m, "npf_waveform_match is not declared in include/npf_hip.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    res, args = L.SIGNATURES["npf_waveform_match"]
    assert res is C.c_int and len(args) == len(decl) == 24 and hasattr(lib, "npf_waveform_match")
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (a, t)
    assert [a.split()[-1].lstrip("*") for a in decl] == [
        "h", "h_ld", "g", "wgt", "wgt_rows", "freq", "freq_rows", "n_valid", "n_rows", "n_tasks", "pts", "tau0", "dtau", "n_tau", "hh", "gg",
        "overlap", "match", "mismatch", "tau_index", "phase", "corr", "workspace", "stream"]
    assert "const int32_t *n_valid" in m.group(1) and "int32_t *tau_index" in m.group(1) and decl[-1] == "void *stream"
    assert re.search(r"\bint64_t\s+npf_waveform_match_workspace_bytes\s*\(\s*int32_t n_rows,\s*int32_t n_tau\s*\)\s*;", header)
    assert L.SIGNATURES["npf_waveform_match_workspace_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert int(re.search(r"#define NPF_WAVEFORM_JC (\d+)", header).group(1)) == FN.MATCH_JC
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_workspace_bytes_and_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    ws = lib.npf_waveform_match_workspace_bytes
    for n_tau, slots in ((0, JC), (1, JC), (JC, JC), (JC + 1, 2 * JC), (65536, 65536)):
        assert ws(5, n_tau) == 5 * (4 + 2 * slots) * 8, n_tau  # per row: hh, gg, c_0/ and whole chunks of (Re, Im)
    assert ws(0, 4) == -1 and ws(-1, 4) == -1 and ws(3, -1) == -1 and ws(3, 65537) == -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(h=p, h_ld=2, g=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
              n_tau=3, hh=p, gg=p, overlap=p, match=p, mismatch=p, tau_index=p, phase=p, corr=p, workspace=p)
    none = dict(hh=None, gg=None, overlap=None, match=None, mismatch=None, tau_index=None, phase=None, corr=None)
    for change in (dict(n_rows=5), dict(h_ld=1), dict(h_ld=0), dict(wgt_rows=3), dict(wgt_rows=0), dict(freq_rows=3), dict(freq_rows=0),
                   dict(n_tau=-1), dict(n_tau=65537), dict(freq=None), none, dict(workspace=None), dict(h=None), dict(g=None),
                   dict(pts=0), dict(n_tasks=0), dict(n_rows=0)):
        a = dict(ok, **change)
        assert lib.npf_waveform_match(*a.values(), None) == -1, change


def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    FN = A.functional
    assert list(inspect.signature(FN.waveform_match).parameters) == ["h", "g", "weights", "freqs", "taus", "n_valid", "want", "corr"]
    assert inspect.signature(FN.waveform_match).parameters["want"].default == FN.MATCH_NAMES
    assert list(inspect.signature(A.HeadDistribution.match).parameters)[1:] == ["Y_ref", "weights", "freqs", "taus", "of", "corr"]
    assert inspect.signature(A.HeadDistribution.match).parameters["of"].default == "samples"
    assert A.Match._fields == ("overlap", "match", "mismatch", "tau", "tau_index", "phase", "corr")
    assert "Match" in A.__all__ and "Match" in A.neuralproc.__all__ and A.Match is A.neuralproc.Match


def test_every_listed_value_error_is_raised_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, Bn = 5, 2
    h, g, w, f = torch.zeros(4, T, 2), torch.zeros(Bn, T, 2), torch.ones(T), torch.ones(Bn, T)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, Bn, T)
    bad = [
        dict(g=torch.zeros(Bn, T, 3)), dict(g=torch.zeros(Bn, T + 1, 2)), dict(g=torch.zeros(T, 2)),  # a wrong g
        dict(weights=torch.ones(T + 1)), dict(weights=torch.ones(Bn + 1, T)), dict(weights=torch.ones(Bn, T, 1)),
        dict(freqs=torch.ones(T - 1), taus=(0.0, 1e-3, 4)), dict(freqs=torch.ones(1, 1, T)),
        dict(taus=(0.0, 1e-3, 4)),                                  # taus without freqs
        dict(freqs=f, taus=(0.0, 1e-3, 0)), dict(freqs=f, taus=(0.0, 1e-3, -2)), dict(freqs=f, taus=(0.0, 1e-3, 65537)),
        dict(freqs=f, taus=(math.inf, 1e-3, 4)), dict(freqs=f, taus=(0.0, math.nan, 4)), dict(freqs=f, taus=(0.0, 1e-3)),
        dict(freqs=f, taus=(0.0, 1e-3, 4.0)), dict(freqs=f, taus=torch.tensor([0.0, 1e-3, 4.0])),
        dict(g=torch.zeros(3, T, 2)),                               # R % B != 0
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            FN.waveform_match(h, **dict(dict(g=g), **kw))
        with pytest.raises(ValueError):
            p.match(**{"Y_ref" if k == "g" else k: v for k, v in dict(dict(g=g), **kw).items()})
    for hb in (torch.zeros(4, T, 1), torch.zeros(4, T), torch.zeros(0, T, 2)):
        with pytest.raises(ValueError):
            FN.waveform_match(hb, g)
    for want in (("matches",), "match", None, ()):
        with pytest.raises(ValueError, match="want"):
            FN.waveform_match(h, g, want=want)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T).match(g)
    with pytest.raises(ValueError, match="of must be"):
        p.match(g, of="median")
    # and once everything fits, the device check: there is no CPU path
    for kw in (dict(), dict(weights=w, freqs=f, taus=(0.0, 1e-3, 4)), dict(weights=f, corr=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FN.waveform_match(h, g, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.match(g, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.match(g, of="mean")
    assert p._base is None


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_cases_cover_every_factor_in_every_regime(all_cases):
    for regime in R.REGIMES:
        mine = [fac for _, fac, _, _ in all_cases if fac["regime"] == regime]
        n_taus = (JC + 1, 257) if regime == "shift" else (None, 1, 5, JC - 1, JC, JC + 1, 257)
        assert {f["n_tau"] for f in mine} == set(n_taus) and {f["T"] for f in mine} == {37, 200}, regime
        assert {f["counts"] is None for f in mine} == {True, False} and {f["n_z"] for f in mine} == {1, 3}, regime
        assert {f["h_ld"] for f in mine} == {2, 4}, regime
        assert {f["wform"] for f in mine} == ({"T", "BT"} if regime in ("removed", "degenerate") else {None, "T", "BT"}), regime
        assert {f["fform"] for f in mine} == ({"T", "BT"} if regime == "shift" else {None, "T", "BT"}), regime
    stars = {(f["n_tau"], c["j_star"]) for _, f, c, _ in all_cases if f["regime"] == "shift"}
    assert stars == {(JC + 1, 5), (JC + 1, JC - 1), (JC + 1, JC), (257, JC + 5), (257, 2 * JC - 1), (257, 2 * JC), (257, 256)}


def test_reference_obeys_cauchy_schwarz(all_cases):
    worst = 0.0
    for tag, _, _, ref in all_cases:
        assert torch.isfinite(ref["mag"]).all() and torch.isfinite(ref["overlap"]).all() and torch.isfinite(ref["phase"]).all(), tag
        worst = max(worst, float(ref["mag"].max()), float(ref["overlap"].abs().max()))
        assert float(ref["match"].max()) <= 1.0 + 1e-12 and float(ref["overlap"].abs().max()) <= 1.0 + 1e-12, tag
        assert float(ref["mismatch"].min()) >= -1e-12, tag
    print(f"MATCH reference: largest normalised |c| over the cases {worst:.17g}")


def test_recurrence_agrees_with_the_direct_form_and_fp32_sines_do_not(all_cases):
    """The recurrence form (what the kernel runs) against one exp per (t, j): <= 1e-12 on every normalised quantity.  The same
    recurrence with the sine and cosine rounded to float32 after a float64 range reduction moves them by more than the GPU gate's
    1e-9 somewhere: the gate tells the two apart."""
    def f32_sincos(x):
        y = torch.remainder(x, R.TWO_PI).float()
        return torch.sin(y).double(), torch.cos(y).double()

    worst, worst32 = 0.0, 0.0
    for tag, _, case, ref in all_cases:
        rec = R.recurrence(**R.call_args(case), jc=JC)
        assert torch.equal(rec["tau_index"], ref["tau_index"]), tag
        d = max(float((rec[k] - ref[k]).abs().max()) for k in ("overlap", "match", "mismatch", "corr"))
        worst = max(worst, d)
        assert d <= 1e-12, (tag, d)
        low = R.recurrence(**R.call_args(case), jc=JC, sincos=f32_sincos)
        worst32 = max(worst32, max(float((low[k] - ref[k]).abs().max()) for k in ("overlap", "match", "corr")))
    print(f"MATCH recurrence vs direct: {worst:.3e}; float32 sine / cosine vs direct: {worst32:.3e}")
    assert worst32 > 1e-9


def test_planted_shift_is_found_and_every_case_has_a_clear_maximum(all_cases):
    """The runner-up of max_j |c_j| (normalised) lies at least 1e-6 below the best in every row of every case with a choice to make
    -- a condition on the inputs; no case is excluded."""
    closest = math.inf
    for tag, fac, case, ref in all_cases:
        live = ~ref["degenerate"]
        if fac["regime"] == "shift":
            assert (ref["tau_index"][live] == case["j_star"]).all(), tag
            assert (ref["tau"][live] == case["taus"][0] + case["j_star"] * case["taus"][1]).all(), tag
            assert float(ref["mismatch"][live].max()) <= 1e-6, tag  # (what the fp32 rounding of the shifted phases leaves)
        if fac["regime"] in ("same", "offset"):
            assert float(ref["mismatch"][live].abs().max()) <= 1e-12, tag
            assert float((ref["phase"][live] - (R.PHI0 if fac["regime"] == "offset" else 0.0)).abs().max()) <= 1e-5, tag
            assert float((ref["overlap"][live] - (math.cos(R.PHI0) if fac["regime"] == "offset" else 1.0)).abs().max()) <= 1e-5, tag
        if ref["mag"].shape[1] >= 2 and live.any():
            top = ref["mag"][live].topk(2, dim=1).values
            gap = float((top[:, 0] - top[:, 1]).min())
            closest = min(closest, gap)
            assert gap >= 1e-6, (tag, gap)
    print(f"MATCH smallest gap between the best and the runner-up |c_j| over the cases: {closest:.3e}")


def test_degenerate_rows_hold_the_stated_constants(all_cases):
    seen = 0
    for tag, fac, case, ref in all_cases:
        deg = ref["degenerate"]
        seen += int(deg.sum())
        for name, value in (("overlap", 0.0), ("match", 0.0), ("mismatch", 1.0), ("tau_index", 0), ("phase", 0.0)):
            assert (ref[name][deg] == value).all(), (tag, name)
        assert (ref["corr"][deg] == 0).all(), tag
        if fac["counts"] is not None:
            assert deg.view(fac["n_z"], R.B)[:, 2].all(), tag  # the task with a count of 0
    assert seen > 0


@pytest.mark.parametrize("n_tau", (None, 1, JC + 1))
@pytest.mark.parametrize("T", (37, 200))
def test_removing_points_equals_cutting_them(T, n_tau):
    case = R.build("removed", T, n_z=3, h_ld=4, wform="T", fform="T" if n_tau else None, taus=R.grid(n_tau), seed=5)
    assert 0.15 * T < int(case["kill"][0].sum()) < 0.6 * T
    assert torch.isnan(case["h"][:, case["kill"][0]]).all() and torch.isnan(case["g"][:, case["kill"][0]]).all()
    full, short = R.reference(**R.call_args(case)), R.reference(**R.cut(case))
    assert torch.equal(full["tau_index"], short["tau_index"])
    for k in ("hh", "gg", "overlap", "match", "mismatch", "phase", "corr"):
        assert torch.isfinite(full[k]).all(), k
        assert float(((full[k] - short[k]).abs() / short[k].abs().clamp(min=1.0)).max()) <= 1e-12, k
