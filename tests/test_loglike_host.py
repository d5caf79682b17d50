"""Host side of the matched-filter log likelihood (CPU, no kernel launched): the C ABI of ``npf_waveform_loglike`` and its refusals,
the Python signatures and refusals, and the float64 reference of tests/loglike_reference.py itself -- ``ln I0`` against 50-digit
arithmetic, the runner-up margin of every input set the GPU test uses, the coverage of the factors, the recurrence form against the
direct form (the margin the GPU gate rests on), the planted identities, removed points against cut ones, and the mixture over
latent samples whose likelihoods lie 800 apart."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import loglike_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC = 16


@pytest.fixture(scope="module")
def x_s():
    from npf_gwwaveform_amd import functional as FN

    return FN.LOGLIKE_I0_SWITCH


@pytest.fixture(scope="module")
def all_cases(x_s):
    from npf_gwwaveform_amd import functional as FN

    assert FN.MATCH_JC == JC
    return [(tag, fac, case, R.reference(**R.call_args(case))) for tag, fac, case in R.cases(FN.MATCH_JC, x_s)]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_waveform_loglike_is_declared_exported_and_typed(x_s):
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    m = re.search(r"\bint\s+npf_waveform_loglike\s*\(([^;]*)\)\s*;", header)
    assert m, "npf_waveform_loglike is not declared in include/npf_hip.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    res, args = L.SIGNATURES["npf_waveform_loglike"]
    assert res is C.c_int and len(args) == len(decl) == 26 and hasattr(lib, "npf_waveform_loglike")
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (a, t)
    assert [a.split()[-1].lstrip("*") for a in decl] == [
        "h", "h_ld", "d", "wgt", "wgt_rows", "freq", "freq_rows", "n_valid", "n_rows", "n_tasks", "pts", "tau0", "dtau", "n_tau", "hh", "dd",
        "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix", "lnl_max_mix", "workspace", "stream"]
    for name in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "phase", "series", "lnl_mix", "lnl_max_mix"):
        assert f"double *{name}" in m.group(1), name  # every likelihood output is a double
    assert "int32_t *tau_index" in m.group(1) and "const float *d," in m.group(1)
    assert re.search(r"\bint64_t\s+npf_waveform_loglike_workspace_bytes\s*\(\s*int32_t n_rows,\s*int32_t n_tau\s*\)\s*;", header)
    assert L.SIGNATURES["npf_waveform_loglike_workspace_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert float(re.search(r"#define NPF_LOGLIKE_I0_SWITCH ([0-9.]+)", header).group(1)) == x_s
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_workspace_bytes_and_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    ws = lib.npf_waveform_loglike_workspace_bytes
    for n_tau, slots in ((0, JC), (1, JC), (JC, JC), (JC + 1, 2 * JC), (65536, 65536)):
        assert ws(5, n_tau) == 5 * (4 + 2 * slots) * 8, n_tau  # per row: hh, dd, kappa_0/ and whole chunks of (Re, Im)
        assert ws(5, n_tau) == lib.npf_waveform_match_workspace_bytes(5, n_tau)
    assert ws(0, 4) == -1 and ws(-1, 4) == -1 and ws(3, -1) == -1 and ws(3, 65537) == -1
    buf = (C.c_double * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(h=p, h_ld=2, d=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
              n_tau=3, hh=p, dd=p, snr=p, lnl_max=p, lnl_marg=p, tau_index=p, phase=p, series=p, lnl_mix=p, lnl_max_mix=p, workspace=p)
    none = dict(hh=None, dd=None, snr=None, lnl_max=None, lnl_marg=None, tau_index=None, phase=None, series=None, lnl_mix=None,
                lnl_max_mix=None)
    for change in (dict(n_rows=5), dict(h_ld=1), dict(h_ld=0), dict(wgt_rows=3), dict(wgt_rows=0), dict(freq_rows=3), dict(freq_rows=0),
                   dict(n_tau=-1), dict(n_tau=65537), dict(freq=None), none, dict(workspace=None), dict(h=None), dict(d=None),
                   dict(pts=0), dict(n_tasks=0), dict(n_rows=0)):
        a = dict(ok, **change)
        assert lib.npf_waveform_loglike(*a.values(), None) == -1, change


def test_signatures_and_exports(x_s):
    import npf_gwwaveform_amd as A

    FN = A.functional
    assert list(inspect.signature(FN.waveform_loglike).parameters) == ["h", "data", "weights", "freqs", "taus", "n_valid", "want", "series"]
    assert inspect.signature(FN.waveform_loglike).parameters["want"].default == FN.LOGLIKE_NAMES
    assert FN.LOGLIKE_NAMES == ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "lnl_mix", "lnl_max_mix")
    assert FN.WaveformLogLike._fields == FN.LOGLIKE_NAMES + ("series",)
    assert list(inspect.signature(A.HeadDistribution.loglike).parameters)[1:] == ["data", "weights", "freqs", "taus", "of", "series"]
    assert inspect.signature(A.HeadDistribution.loglike).parameters["of"].default == "samples"
    assert A.LogLike._fields == ("optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau", "tau_index", "lnl", "lnl_max_mix", "dd", "series")
    assert "LogLike" in A.__all__ and "LogLike" in A.neuralproc.__all__ and A.LogLike is A.neuralproc.LogLike
    assert 16.0 <= x_s <= 64.0
    for word in ("gradients", "sigma", "amplitude marginalisation", "non-uniform time priors", "sub-grid"):
        assert word in A.HeadDistribution.loglike.__doc__, word  # what is out of scope is said


def test_every_listed_value_error_is_raised_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, Bn = 5, 2
    h, d, w, f = torch.zeros(4, T, 2), torch.zeros(Bn, T, 2), torch.ones(T), torch.ones(Bn, T)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, Bn, T)
    bad = [
        dict(data=torch.zeros(Bn, T, 3)), dict(data=torch.zeros(Bn, T + 1, 2)), dict(data=torch.zeros(T, 2)), dict(data=None),
        dict(weights=torch.ones(T + 1)), dict(weights=torch.ones(Bn + 1, T)), dict(weights=torch.ones(Bn, T, 1)),
        dict(freqs=torch.ones(T - 1), taus=(0.0, 1e-3, 4)), dict(freqs=torch.ones(1, 1, T)),
        dict(taus=(0.0, 1e-3, 4)),                                  # taus without freqs
        dict(freqs=f, taus=(0.0, 1e-3, 0)), dict(freqs=f, taus=(0.0, 1e-3, 65537)), dict(freqs=f, taus=(math.inf, 1e-3, 4)),
        dict(freqs=f, taus=(0.0, 1e-3)), dict(freqs=f, taus=(0.0, 1e-3, 4.0)), dict(freqs=f, taus=torch.tensor([0.0, 1e-3, 4.0])),
        dict(data=torch.zeros(3, T, 2)),                            # R % B != 0
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            FN.waveform_loglike(h, **dict(dict(data=d), **kw))
        with pytest.raises(ValueError):
            p.loglike(**dict(dict(data=d), **kw))
    for hb in (torch.zeros(4, T, 1), torch.zeros(4, T), torch.zeros(0, T, 2)):
        with pytest.raises(ValueError):
            FN.waveform_loglike(hb, d)
    for want in (("lnl",), "lnl_marg", None, ()):
        with pytest.raises(ValueError, match="want"):
            FN.waveform_loglike(h, d, want=want)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T).loglike(d)
    with pytest.raises(ValueError, match="of must be"):
        p.loglike(d, of="median")
    for kw in (dict(), dict(weights=w, freqs=f, taus=(0.0, 1e-3, 4)), dict(weights=f, series=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FN.waveform_loglike(h, d, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.loglike(d, **kw)
    assert p._base is None


# ---- ln I0 -------------------------------------------------------------------------------------------------------------------------
def _i0_points(x_s):
    asked = [0.0, 1e-8, 1e-3, 1.0, x_s * (1 - 1e-6), x_s * (1 + 1e-6), 30.0, 700.0, 720.0, 1e4, 1e6]
    return asked + [0.03, 0.5, 1.0 - 1e-9, 1.0 + 1e-9, 3.0, 10.0]  # (and both sides of the reference's own branch at 1)


def test_log_i0_of_the_reference_meets_fifty_digit_arithmetic(x_s):
    """The reference's ln I0 against mpmath.besseli(0, x) at 50 digits: 1e-14 relative + 1e-17 absolute."""
    import mpmath as mp

    worst = 0.0
    with mp.workdps(50):
        for x in _i0_points(x_s):
            exact = mp.log(mp.besseli(0, mp.mpf(x)))
            got = float(R.log_i0(torch.tensor([x], dtype=torch.float64))[0])
            err, gate = float(abs(mp.mpf(got) - exact)), 1e-14 * float(abs(exact)) + 1e-17
            worst = max(worst, err / gate)
            assert math.isfinite(got) and err <= gate, (x, got, float(exact), err, gate)
    print(f"LOGLIKE ln I0 reference vs 50 digits: worst error / gate {worst:.3g}")


def test_log_i0_scheme_of_the_kernel_meets_fifty_digit_arithmetic(x_s):
    """The kernel's scheme (power series below x_s, 16 terms in 1 / (8 x) from there on) evaluated in Python doubles, at the same
    points and around the switch point, under the same gate; and the truncation of the 16 terms at x_s is below 1e-15 of I0."""
    import mpmath as mp

    worst = 0.0
    with mp.workdps(50):
        pts = _i0_points(x_s) + [x_s, x_s * 0.5, x_s * 0.9, x_s * 1.1, x_s * 2.0]
        for x in pts:
            exact = mp.log(mp.besseli(0, mp.mpf(x)))
            got = R.log_i0_scheme(x, x_s)
            err, gate = float(abs(mp.mpf(got) - exact)), 1e-14 * float(abs(exact)) + 1e-17
            worst = max(worst, err / gate)
            assert math.isfinite(got) and err <= gate, (x, got, float(exact), err, gate)
        a = s = mp.mpf(1)
        for k in range(1, R.I0_ASYM_TERMS + 1):
            a *= mp.mpf((2 * k - 1) ** 2) / (k * 8 * mp.mpf(x_s))
            s += a
        exact = mp.besseli(0, mp.mpf(x_s)) * mp.exp(-mp.mpf(x_s)) * mp.sqrt(2 * mp.pi * mp.mpf(x_s))
        trunc = float(abs(s - exact) / exact)
    print(f"LOGLIKE ln I0 scheme vs 50 digits: worst error / gate {worst:.3g}; truncation of {R.I0_ASYM_TERMS} terms at x_s {trunc:.3g}")
    assert trunc < 1e-15


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_cases_cover_every_factor_in_every_regime(all_cases):
    assert len(R.REGIMES) == 8
    for regime in R.REGIMES:
        mine = [fac for _, fac, _, _ in all_cases if fac["regime"] == regime]
        assert {f["n_tau"] for f in mine} == {None, 1, 5, JC - 1, JC, JC + 1, 257} and {f["T"] for f in mine} == {37, 200}, regime
        assert {f["counts"] is None for f in mine} == {True, False} and {f["n_z"] for f in mine} == {1, 3}, regime
        assert {f["h_ld"] for f in mine} == {2, 4}, regime
        assert {f["wform"] for f in mine} == ({"T", "BT"} if regime in ("removed", "degenerate") else {None, "T", "BT"}), regime
        assert {f["fform"] for f in mine} == {None, "T", "BT"}, regime
    stars = {(f["n_tau"], c["j_star"]) for _, f, c, _ in all_cases if f["regime"] == "planted"}
    assert stars >= {(JC + 1, 5), (JC + 1, JC - 1), (JC + 1, JC), (257, JC + 5), (257, 2 * JC - 1), (257, 2 * JC), (257, 256)}


def test_every_case_has_a_clear_maximum(all_cases):
    """The runner-up of max_j x_j lies at least 1e-6 sqrt(hh dd) below the best in every live row of every case with a choice to make
    -- a condition on the inputs; no case is excluded."""
    closest = math.inf
    for tag, fac, case, ref in all_cases:
        live = ~ref["degenerate"]
        for k in R.DOUBLES + ("series",):
            assert torch.isfinite(ref[k]).all(), (tag, k)
        if ref["x"].shape[1] >= 2 and live.any():
            top = ref["x"][live].topk(2, dim=1).values
            gap = (top[:, 0] - top[:, 1]) / (ref["hh"] * ref["dd_rows"]).sqrt()[live]
            closest = min(closest, float(gap.min()))
            assert float(gap.min()) >= 1e-6, (tag, float(gap.min()))
    print(f"LOGLIKE smallest gap between the best and the runner-up x_j over the cases, in sqrt(hh dd): {closest:.3e}")


def test_regimes_reach_what_they_aim_at(all_cases, x_s):
    """loud: x* ~ 1e4 and latent samples more than 745 apart; quiet: x* ~ 1e-3; edge: x_j on both sides of the switch point within
    one grid; bigphase: phases of 1e4 rad; degenerate: rows with hh == 0 that hold the stated zeros."""
    seen = dict(loud=0, apart=0, quiet=0, edge=0, big=0, deg=0)
    for tag, fac, case, ref in all_cases:
        xb = ref["x"].max(1).values
        deg = ref["degenerate"]
        seen["deg"] += int(deg.sum())
        for name in ("snr", "phase", "lnl_max", "lnl_marg", "tau_index"):
            assert (ref[name][deg] == 0).all(), (tag, name)
        assert (ref["series"][deg] == 0).all(), tag
        if fac["counts"] is not None:
            assert deg.view(fac["n_z"], R.B)[:, 2].all(), tag  # the task with a count of 0
        if fac["regime"] == "loud":
            seen["loud"] += int((xb > 3e3).sum())
            assert float(xb.max()) < 3e4, tag
            if fac["n_z"] == 3:
                v = ref["lnl_marg"].view(3, R.B)[:, 0]
                seen["apart"] += int((v.max() - v.min()) > 745)
                assert torch.isfinite(ref["lnl_mix"]).all()
        if fac["regime"] == "quiet":
            live = ~deg
            assert float(xb[live].max()) < 3e-3, tag
            seen["quiet"] += int((xb[live] > 1e-4).sum())
        if fac["regime"] == "edge" and fac["n_tau"] not in (None, 1):
            rows = ((ref["x"] >= x_s).any(1) & (ref["x"] < x_s).any(1) & ~deg)
            seen["edge"] += int(rows.sum())
        if fac["regime"] == "bigphase":
            seen["big"] += int(case["h"][..., 1].abs().max() > 1e4)
    print(f"LOGLIKE regimes: {seen}")
    assert all(v > 0 for v in seen.values()), seen
    assert seen["edge"] >= 6 and seen["apart"] >= 6


def test_recurrence_agrees_with_the_direct_form(all_cases):
    """kappa_j by the kernel's recurrence against one exp per (t, j): every double output within 1e-12 (sqrt(hh dd) + hh / 2) + 1e-15
    -- the margin the GPU gate (100 times that) rests on; the phase, an angle, within 1e-11 where x* >= 1e-3 sqrt(hh dd)."""
    worst, worst_phase = 0.0, 0.0
    for tag, _, case, ref in all_cases:
        rec = R.recurrence(**R.call_args(case), jc=JC)
        assert torch.equal(rec["tau_index"], ref["tau_index"]), tag
        scale = R.scale_of(ref)
        task_scale = scale.view(-1, R.B).max(0).values
        for k in R.DOUBLES:
            if k == "phase":
                continue
            gate = 1e-12 * (task_scale if ref[k].shape[0] == R.B and k in ("dd", "lnl_mix", "lnl_max_mix") else scale) + 1e-15
            q = float(((rec[k] - ref[k]).abs() / gate).max())
            worst = max(worst, q)
            assert q <= 1.0, (tag, k, q)
        q = float(((rec["series"][..., 0] - ref["series"][..., 0]).abs() / (1e-12 * scale + 1e-15).view(-1, 1)).max())
        worst = max(worst, q)
        assert q <= 1.0, (tag, "series", q)
        r = R.ratios(dict(phase=rec["phase"]), ref)["phase"] * 1e-9 / 1e-11
        worst_phase = max(worst_phase, r)
        assert r <= 1.0, (tag, "phase", r)
    print(f"LOGLIKE recurrence vs direct: worst error / (1e-12 scale + 1e-15) {worst:.3g}; phase error / 1e-11 {worst_phase:.3g}")


def test_planted_data_give_the_three_identities(all_cases):
    """d = h shifted to the grid index j* and rotated by a constant phase: tau_index = j*, snr = sqrt(hh), lnl_max = hh / 2, to
    1e-12 relative on the data before their rounding to fp32; on the fp32 data the index stays and the rest holds to 1e-6."""
    n = 0
    for tag, fac, case, ref in all_cases:
        if fac["regime"] != "planted":
            continue
        n += 1
        live = ~ref["degenerate"]
        exact = R.reference(**dict(R.call_args(case), data=case["data64"]))
        for name, r, tol in (("unrounded", exact, 1e-12), ("fp32", ref, 1e-6)):
            assert (r["tau_index"][live] == case["j_star"]).all(), (tag, name)
            hh = r["hh"][live]
            assert float(((r["snr"][live] - hh.sqrt()).abs() / hh.sqrt()).max()) <= tol, (tag, name)
            assert float(((r["lnl_max"][live] - 0.5 * hh).abs() / (0.5 * hh)).max()) <= tol, (tag, name)
            # arg kappa_{j*} = -PHI0: an angle, so the same figure in radians (PHI0 itself is one double away from 0.7)
            assert float((torch.remainder(r["phase"][live] + R.PHI0 + math.pi, R.TWO_PI) - math.pi).abs().max()) <= tol, (tag, name)
    assert n >= 14


@pytest.mark.parametrize("n_tau", (None, 1, JC + 1))
@pytest.mark.parametrize("T", (37, 200))
def test_removing_points_equals_cutting_them(T, n_tau, x_s):
    case = R.build("removed", T, n_z=3, h_ld=4, wform="T", fform="T" if n_tau else None, taus=R.grid(n_tau), seed=5, x_s=x_s)
    assert 0.15 * T < int(case["kill"][0].sum()) < 0.6 * T
    assert torch.isnan(case["h"][:, case["kill"][0]]).all() and torch.isnan(case["data"][:, case["kill"][0]]).all()
    full, short = R.reference(**R.call_args(case)), R.reference(**R.cut(case))
    assert torch.equal(full["tau_index"], short["tau_index"])
    for k in R.DOUBLES + ("series",):
        assert torch.isfinite(full[k]).all(), k
        assert float(((full[k] - short[k]).abs() / short[k].abs().clamp(min=1.0)).max()) <= 1e-12, k


def test_mixture_of_rows_800_apart_is_finite_and_the_maximum_minus_log_n_z(x_s):
    """Plain values 800 apart, and the "loud" inputs of the GPU test, whose latent samples lie about 800 and 2450 below the best."""
    for n_z in (2, 3, 8):
        v = torch.tensor([[-800.0 * s, 5000.0 - 800.0 * s, 800.0 * s - 9000.0] for s in range(n_z)], dtype=torch.float64).reshape(-1)
        mix = R.log_mean_exp_rows(v, 3)
        want = v.view(n_z, 3).max(0).values - math.log(n_z)
        assert torch.isfinite(mix).all()
        assert float(((mix - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-12, n_z
    case = R.build("loud", 200, n_z=3, h_ld=2, wform="T", fform="T", taus=R.grid(JC + 1), j_star=2, seed=1, x_s=x_s)
    ref = R.reference(**R.call_args(case))
    for name, rows in (("lnl_mix", ref["lnl_marg"].view(3, R.B)), ("lnl_max_mix", ref["lnl_max"].view(3, R.B))):
        top = rows.sort(0, descending=True).values
        assert float((top[0] - top[1]).min()) > 745, name
        want = top[0] - math.log(3)
        assert torch.isfinite(ref[name]).all() and float(((ref[name] - want).abs() / want.abs()).max()) <= 1e-12, name
