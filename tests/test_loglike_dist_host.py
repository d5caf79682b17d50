"""Host side of the distance-marginalised likelihood (CPU, no kernel launched): the C ABI of ``npf_waveform_loglike_dist`` /
``npf_waveform_loglike_net_dist`` and its refusals, the Python signatures and refusals, ``distance_prior``, and the float64 reference
of tests/loglike_dist_reference.py itself -- the kernel's ``ln I0`` scheme at ``a x`` on both sides of the switch point against
50-digit arithmetic, the one-pass form against the direct double log-sum-exp, and the runner-up margin of ``max_i u_i`` in every
input set the GPU test uses."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import loglike_dist_reference as Dd
import loglike_reference as R1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC = 16


@pytest.fixture(scope="module")
def all_cases():
    out = []
    for network in (False, True):
        for tag, fac, case, s, p in Dd.cases(network):
            ref = Dd.parent_reference(network, case)
            out.append((network, tag, fac, case, s, p, ref, Dd.marginalise(ref, s, p)))
    return out


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NEW_ARGS = ["scales", "scale_rows", "log_prior", "prior_rows", "n_a", "lnl_dist", "scale_index", "scale_hat", "lnl_amp_max", "lnl_dist_mix",
            "post", "post_mix", "workspace", "stream"]


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_both_entries_are_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    for name, parent in (("npf_waveform_loglike_dist", "npf_waveform_loglike"), ("npf_waveform_loglike_net_dist", "npf_waveform_loglike_net")):
        decl, pdecl = _declared(header, name), _declared(header, parent)
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl) == len(pdecl) + 12 and hasattr(lib, name), name
        for a, t in zip(decl, args):
            assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (name, a, t)
        names = [a.split()[-1].lstrip("*") for a in decl]
        assert names == [a.split()[-1].lstrip("*") for a in pdecl[:-2]] + NEW_ARGS, name  # the parent's list, then the new ones
        text = ", ".join(decl)
        for out in ("lnl_dist", "scale_hat", "lnl_amp_max", "lnl_dist_mix", "post", "post_mix"):
            assert f"double *{out}" in text, (name, out)
        assert "int32_t *scale_index" in text and "const double *scales" in text and "const double *log_prior" in text
    assert re.search(r"\bint64_t\s+npf_waveform_loglike_dist_workspace_bytes\s*\(\s*int32_t n_rows,\s*int32_t n_det,\s*int32_t n_tau,"
                     r"\s*int32_t n_a\s*\)\s*;", header)
    assert L.SIGNATURES["npf_waveform_loglike_dist_workspace_bytes"] == (C.c_int64, [C.c_int32] * 4)
    assert int(re.search(r"#define NPF_DIST_SC (\d+)", header).group(1)) == FN.DIST_SC == Dd.SC
    assert int(re.search(r"#define NPF_DIST_MAX_SCALES (\d+)", header).group(1)) == FN.DIST_MAX_SCALES == 4096
    for word in ("dead", "no live scale", "HH == 0", "not normalised"):
        assert word in header.lower() or word in header, word
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_workspace_bytes_and_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    ws = lib.npf_waveform_loglike_dist_workspace_bytes
    for n_tau in (0, 1, JC, JC + 1, 257):
        for n_a in (1, 17, 4096):
            assert ws(5, 0, n_tau, n_a) == lib.npf_waveform_loglike_workspace_bytes(5, n_tau) + 5 * (1 + n_a) * 8  # x* and the u_i
            assert ws(5, 3, n_tau, n_a) == lib.npf_waveform_loglike_net_workspace_bytes(5, 3, n_tau) + 5 * (1 + n_a) * 8
    for bad in ((0, 0, 4, 3), (3, -1, 4, 3), (3, 9, 4, 3), (3, 0, -1, 3), (3, 0, 65537, 3), (3, 0, 4, 0), (3, 0, 4, 4097)):
        assert ws(*bad) == -1, bad
    buf = (C.c_double * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    head = dict(h=p, h_ld=2, d=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None)
    outs = dict(hh=p, dd=p, snr=p, lnl_max=p, lnl_marg=p, tau_index=p, phase=p, series=p, lnl_mix=p, lnl_max_mix=p)
    new = dict(scales=p, scale_rows=1, log_prior=p, prior_rows=2, n_a=3, lnl_dist=p, scale_index=p, scale_hat=p, lnl_amp_max=p,
               lnl_dist_mix=p, post=p, post_mix=p, workspace=p)
    single = dict(head, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3, n_tau=3, **outs, **new)
    net = dict(head, delay=p, resp=p, n_rows=6, n_tasks=2, n_det=2, pts=4, tau0=0.0, dtau=1e-3, n_tau=3, **outs, hh_det=p, snr_det=p,
               dd_det=p, **new)
    none = {k: None for k in list(outs) + ["hh_det", "snr_det", "dd_det", "lnl_dist", "scale_index", "scale_hat", "lnl_amp_max",
                                           "lnl_dist_mix", "post", "post_mix"]}
    changes = [dict(n_a=0), dict(n_a=-1), dict(n_a=4097), dict(scales=None), dict(log_prior=None), dict(scale_rows=0), dict(scale_rows=3),
               dict(prior_rows=0), dict(prior_rows=6), dict(n_rows=5), dict(h_ld=1), dict(wgt_rows=3), dict(freq_rows=0), dict(n_tau=-1),
               dict(n_tau=65537), dict(freq=None), dict(workspace=None), dict(h=None), dict(d=None), dict(pts=0), dict(n_tasks=0)]
    for change in changes:
        assert lib.npf_waveform_loglike_dist(*dict(single, **change).values(), None) == -1, change
        assert lib.npf_waveform_loglike_net_dist(*dict(net, **change).values(), None) == -1, change
    assert lib.npf_waveform_loglike_dist(*dict(single, **{k: v for k, v in none.items() if k in single}).values(), None) == -1
    assert lib.npf_waveform_loglike_net_dist(*dict(net, **none).values(), None) == -1
    for change in (dict(n_det=0), dict(n_det=9), dict(resp=None)):
        assert lib.npf_waveform_loglike_net_dist(*dict(net, **change).values(), None) == -1, change


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    FN = A.functional
    assert list(inspect.signature(FN.waveform_loglike_distance).parameters) == [
        "h", "data", "scales", "log_prior", "weights", "freqs", "taus", "n_valid", "want", "posterior"]
    assert list(inspect.signature(FN.waveform_loglike_network_distance).parameters) == [
        "h", "data", "response", "delays", "scales", "log_prior", "weights", "freqs", "taus", "n_valid", "want", "posterior"]
    assert FN.LOGLIKE_DIST_NAMES == ("lnl_dist", "scale_index", "scale_hat", "lnl_amp_max", "lnl_dist_mix")
    assert inspect.signature(FN.waveform_loglike_distance).parameters["want"].default == FN.LOGLIKE_NAMES + FN.LOGLIKE_DIST_NAMES
    assert inspect.signature(FN.waveform_loglike_network_distance).parameters["want"].default == FN.LOGLIKE_NET_NAMES + FN.LOGLIKE_DIST_NAMES
    assert inspect.signature(FN.waveform_loglike_distance).parameters["posterior"].default is False
    assert FN.WaveformLogLikeDistance._fields == FN.LOGLIKE_DIST_NAMES + ("post", "post_mix", "base")
    assert list(inspect.signature(A.HeadDistribution.loglike_distance).parameters)[1:] == [
        "data", "scales", "log_prior", "weights", "freqs", "taus", "of", "posterior"]
    assert list(inspect.signature(A.HeadDistribution.loglike_network_distance).parameters)[1:] == [
        "data", "response", "delays", "scales", "log_prior", "weights", "freqs", "taus", "of", "posterior"]
    fields = ("lnl", "lnl_dist", "scale_hat", "lnl_amp_max", "scale_index", "scale_map", "post", "post_mix", "base")
    assert A.DistanceLogLike._fields == fields and A.NetworkDistanceLogLike._fields == fields
    for name in ("DistanceLogLike", "NetworkDistanceLogLike"):
        assert name in A.__all__ and name in A.neuralproc.__all__ and getattr(A, name) is getattr(A.neuralproc, name)
    assert list(inspect.signature(FN.distance_prior).parameters) == ["distances", "d_ref", "power"]
    # the two parents no longer list the distance marginalisation as out of scope; the new call says what is
    for parent in (A.HeadDistribution.loglike, A.HeadDistribution.loglike_network):
        scope = parent.__doc__.split("Out of scope:")[1]
        assert "distance" not in scope and "amplitude" not in scope, parent.__name__
    for word in ("gradients", "non-uniform time priors", "sigma", "continuous"):
        assert word in A.HeadDistribution.loglike_distance.__doc__.split("Out of scope:")[1], word


def test_every_listed_value_error_is_raised_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, Bn, D, n_a = 5, 2, 3, 4
    h, d, dn = torch.zeros(4, T, 2), torch.zeros(Bn, T, 2), torch.zeros(Bn, D, T, 2)
    resp = torch.ones(Bn, D, 2, dtype=torch.float64)
    s, lp = torch.ones(n_a, dtype=torch.float64), torch.zeros(Bn, n_a, dtype=torch.float64)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, Bn, T)
    bad = [dict(scales=torch.ones(n_a)), dict(log_prior=torch.zeros(n_a)),                       # not float64
           dict(scales=torch.ones(n_a + 1, dtype=torch.float64)),                                   # another n_a than log_prior
           dict(scales=torch.ones(Bn + 1, n_a, dtype=torch.float64)), dict(log_prior=torch.zeros(1, n_a, dtype=torch.float64)),
           dict(scales=torch.ones(1, Bn, n_a, dtype=torch.float64)), dict(scales=torch.tensor(1.0, dtype=torch.float64)),
           dict(scales=torch.ones(0, dtype=torch.float64), log_prior=torch.zeros(0, dtype=torch.float64)),
           dict(scales=torch.ones(4097, dtype=torch.float64), log_prior=torch.zeros(4097, dtype=torch.float64)),
           dict(scales=None), dict(log_prior=[0.0] * n_a)]
    for kw in bad:
        a = dict(dict(scales=s, log_prior=lp), **kw)
        with pytest.raises(ValueError):
            FN.waveform_loglike_distance(h, d, **a)
        with pytest.raises(ValueError):
            FN.waveform_loglike_network_distance(h, dn, resp, None, **a)
        with pytest.raises(ValueError):
            p.loglike_distance(d, **a)
        with pytest.raises(ValueError):
            p.loglike_network_distance(dn, resp, None, **a)
        with pytest.raises(ValueError):
            FN.check_loglike_distance_args((4, T, 2), d, a["scales"], a["log_prior"])
    # the parents' rules still hold
    with pytest.raises(ValueError):
        FN.waveform_loglike_distance(h, torch.zeros(Bn, T, 3), s, lp)
    with pytest.raises(ValueError):
        FN.waveform_loglike_network_distance(h, dn, resp.float(), None, s, lp)
    with pytest.raises(ValueError):
        FN.waveform_loglike_distance(h, d, s, lp, taus=(0.0, 1e-3, 4))  # taus without freqs
    for want in (("lnl",), "lnl_dist", None, (), ("hh_det",)):
        with pytest.raises(ValueError, match="want"):
            FN.waveform_loglike_distance(h, d, s, lp, want=want)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T).loglike_distance(d, s, lp)
    with pytest.raises(ValueError, match="of must be"):
        p.loglike_distance(d, s, lp, of="median")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FN.waveform_loglike_distance(h, d, s, lp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.loglike_network_distance(dn, resp, None, s, lp)
    geo, scale_rows, prior_rows, n = FN.check_loglike_distance_args((4, T, 2), d, s, lp)
    assert geo == FN.check_loglike_args((4, T, 2), d) and (scale_rows, prior_rows, n) == (1, Bn, n_a)
    assert p._base is None


def test_distance_prior():
    from npf_gwwaveform_amd import functional as FN

    d = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
    s, lp = FN.distance_prior(d, 2.0)
    assert torch.equal(s, torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64)) and lp.dtype == torch.float64
    # by hand: widths (0.5, 1.5, 1.0), masses d^2 x width = (0.5, 6, 16) of 22.5
    want = torch.tensor([0.5, 6.0, 16.0], dtype=torch.float64) / 22.5
    assert float((lp.exp() - want).abs().max()) <= 1e-15
    for power in (0.0, 2.0, 3.5):
        grid = torch.logspace(1.0, 3.0, 50, dtype=torch.float64)
        s, lp = FN.distance_prior(grid, 100.0, power)
        assert abs(float(torch.logsumexp(lp, 0))) <= 1e-14 and torch.equal(s, 100.0 / grid)
    both = torch.stack([torch.linspace(10.0, 500.0, 33, dtype=torch.float64), torch.logspace(1.0, 3.0, 33, dtype=torch.float64)])
    s2, lp2 = FN.distance_prior(both, 40.0)
    assert s2.shape == lp2.shape == (2, 33) and float(torch.logsumexp(lp2, 1).abs().max()) <= 1e-14
    for b in range(2):
        sb, lb = FN.distance_prior(both[b], 40.0)
        assert torch.equal(sb, s2[b]) and float((lb - lp2[b]).abs().max()) <= 1e-15
    one = FN.distance_prior(torch.tensor([7.0], dtype=torch.float64), 7.0)
    assert float(one[0]) == 1.0 and float(one[1]) == 0.0
    for bad in (torch.ones(3), torch.ones(2, 2, 2, dtype=torch.float64), [1.0, 2.0], torch.ones(0, dtype=torch.float64)):
        with pytest.raises(ValueError):
            FN.distance_prior(bad, 1.0)


# ---- ln I0 at a x ------------------------------------------------------------------------------------------------------------------
def test_log_i0_scheme_at_scaled_arguments_meets_fifty_digit_arithmetic():
    """The kernel's scheme at a x with x on both sides of the switch point 24 and a over the grid's range [2^-4, 2^4], so that the
    product crosses the switch along the scale axis: 1e-14 relative + 1e-17 absolute, the gate of tests/test_loglike_host.py."""
    import mpmath as mp

    from npf_gwwaveform_amd import functional as FN

    x_s = FN.LOGLIKE_I0_SWITCH
    worst, sides = 0.0, set()
    with mp.workdps(50):
        for x in (1e-3, 1.0, x_s * (1 - 1e-6), x_s * (1 + 1e-6), 30.0, 1e4):
            for a in (2.0 ** -4, 0.3, x_s / x if x > 1e-2 else 1.0, 1.0, 1.0 + 2.0 ** -30, 3.7, 16.0):
                z = a * x
                sides.add(z < x_s)
                exact = mp.log(mp.besseli(0, mp.mpf(z)))
                got = R1.log_i0_scheme(z, x_s)
                err, gate = float(abs(mp.mpf(got) - exact)), 1e-14 * float(abs(exact)) + 1e-17
                worst = max(worst, err / gate)
                assert math.isfinite(got) and err <= gate, (x, a, got, float(exact), err, gate)
    assert sides == {True, False}
    print(f"LOGLIKE_DIST ln I0 scheme at a x vs 50 digits: worst error / gate {worst:.3g}")


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_cases_cover_the_shapes_and_the_grids(all_cases):
    for network in (False, True):
        mine = [fac for net, _, fac, *_ in all_cases if net == network]
        assert len(mine) == len(R1.REGIMES) * len(Dd.N_AS)
        for regime in R1.REGIMES:
            r = [f for f in mine if f["regime"] == regime]
            assert {f["n_a"] for f in r} == set(Dd.N_AS) == {1, 2, Dd.SC - 1, Dd.SC, Dd.SC + 1, 64, 65, 257, 300}, regime
            assert {f["n_tau"] for f in r} == {None, 1, 16, 17, 257} and {f["T"] for f in r} == {37, 200}, regime
            assert {f["sform"] for f in r} == {"A", "BA"} and {f["pform"] for f in r} == {"A", "BA"}, regime
            assert {f["counts"] is None for f in r} == {True, False} and "dead" in {f["kind"] for f in r}, regime
        assert {f["n_z"] for f in mine} == {1, 3} and {f["kind"] for f in mine} == {"geo", "dead", "alldead"}
        if network:
            assert {f["D"] for f in mine} == {1, 2, 3}
    s, p = Dd.scale_grid(17, "BA", "A", "dead")
    assert (s[:, 1] == 0).all() and (s[:, 3] < 0).all() and torch.isnan(s[:, 5]).all() and torch.isinf(s[:, 7]).all()
    assert p[2] == -math.inf and p[9] == math.inf and math.isnan(p[11]) and torch.isnan(p[[1, 3, 5, 7]]).all()
    s, p = Dd.scale_grid(17, "A", "A", "alldead")
    assert not Dd.live_mask(s, p).any()


def test_regimes_reach_what_they_aim_at(all_cases):
    """edge: a x_j on both sides of the switch along the scale axis inside one row; loud: a x* reaches 1e5 and lnl_dist of
    neighbouring rows lies more than 745 apart; rows with HH == 0 hold the normalised prior; rows without a live scale hold -inf."""
    from npf_gwwaveform_amd import functional as FN

    x_s = FN.LOGLIKE_I0_SWITCH
    seen = dict(edge=0, loud=0, apart=0, deg=0, none=0)
    for network, tag, fac, case, s, p, ref, dist in all_cases:
        live, u = dist["live"], dist["u"]
        a = Dd._per_row(s, Dd.B, u.shape[0])
        xb = ref["x"].max(1).values
        none = ~live.any(1)
        seen["none"] += int(none.sum())
        assert (dist["lnl_dist"][none] == -math.inf).all() and (dist["post"][none] == -math.inf).all() and (dist["scale_index"][none] == 0).all()
        assert not torch.isnan(dist["post"]).any() and not torch.isnan(dist["post_mix"]).any() and not torch.isnan(dist["lnl_dist"]).any(), tag
        deg = ref["degenerate"] & ~none
        seen["deg"] += int(deg.sum())
        if deg.any():
            lp = torch.where(live, Dd._per_row(p, Dd.B, u.shape[0]), torch.full_like(u, -math.inf))[deg]
            assert float((dist["post"][deg] - (lp - torch.logsumexp(lp, 1, keepdim=True))).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= 1e-12, tag
        ax = torch.where(live, a * xb.view(-1, 1), torch.full_like(a, math.nan))
        if fac["regime"] == "edge":
            seen["edge"] += int(((ax >= x_s).any(1) & (ax < x_s).any(1)).sum())
        if fac["regime"] == "loud":
            seen["loud"] += int((ax >= 1e5).any())
            v = dist["lnl_dist"].view(-1, Dd.B)[:, 0]
            if torch.isfinite(v).all() and v.numel() > 1:
                seen["apart"] += int((v.max() - v.min()) > 745)
                assert torch.isfinite(dist["lnl_dist_mix"][0])
    print(f"LOGLIKE_DIST regimes: {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_every_case_leaves_scale_index_well_posed(all_cases):
    """In every case and every row with a live scale the runner-up of max_i u_i lies at least 1e3 gates below the best; no case is
    exempted (the cases that failed were rebuilt: loglike_dist_reference.DATA_SCALE, DATA_SCALE_OF)."""
    closest = math.inf
    for network, tag, fac, case, s, p, ref, dist in all_cases:
        rows = dist["live"].any(1)
        if not rows.any():
            continue
        g = float(Dd.runner_up_in_gates(dist)[rows].min())
        closest = min(closest, g)
        assert g >= 1e3, (tag, g)
    print(f"LOGLIKE_DIST smallest gap between the best and the runner-up u_i over the cases, in gates: {closest:.4g}")


def test_one_pass_form_agrees_with_the_direct_log_sum_exp(all_cases):
    """M_i and S_i with terms <= 1, then the shifted sum over i, against logsumexp of the full [R, n_a, n] array: below 0.1 of a gate
    for u_i and for lnl_dist on every case."""
    worst = 0.0
    for network, tag, fac, case, s, p, ref, dist in all_cases:
        op = Dd.one_pass(ref, s, p)
        gate = 1e-10 * dist["S"] + 1e-12
        for name, g in (("u", gate.view(-1, 1).expand_as(dist["u"])), ("lnl_dist", gate)):
            x, r = op[name], dist[name]
            assert torch.equal(x == -math.inf, r == -math.inf), (tag, name)
            fin = torch.isfinite(r)
            q = float(((x[fin] - r[fin]).abs() / g[fin]).max()) if fin.any() else 0.0
            worst = max(worst, q)
            assert q <= 0.1, (tag, name, q)
    print(f"LOGLIKE_DIST one-pass form vs direct log-sum-exp: worst error / gate {worst:.3g}")
