"""Host side of the coherent network log likelihood (CPU, no kernel launched): the float64 reference of
tests/loglike_net_reference.py itself -- against the single-stream reference at D = 1, the planted identities, three wrong
evaluations that must miss the gates, the runner-up margin and the phase gate's filter of every input set the GPU test uses, the
recurrence form against the direct form -- and the C ABI, the binding and the Python refusals of ``npf_waveform_loglike_net``."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import loglike_net_reference as N
import loglike_reference as R1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC = 16
NET_ARGS = ["h", "h_ld", "d", "wgt", "wgt_rows", "freq", "freq_rows", "n_valid", "delay", "resp", "n_rows", "n_tasks", "n_det", "pts",
            "tau0", "dtau", "n_tau", "hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix", "lnl_max_mix",
            "hh_det", "snr_det", "dd_det", "workspace", "stream"]
OUTPUTS = NET_ARGS[17:30]


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    assert FN.MATCH_JC == JC
    return [(tag, fac, case, N.reference(**N.call_args(case))) for tag, fac, case in N.cases(JC, FN.LOGLIKE_I0_SWITCH)]


def _worst(r):
    return max(r.values())


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ("planted", "noise", "removed", "degenerate", "bigphase"))
@pytest.mark.parametrize("n_tau", (None, 17))
def test_one_detector_unit_response_no_delay_is_the_single_stream_reference_to_the_last_bit(regime, n_tau):
    need_w = regime in ("removed", "degenerate")
    one = R1.build(regime, 37, n_z=3, h_ld=4, wform="BT" if need_w else "T", fform="T" if n_tau else None, taus=R1.grid(n_tau, regime),
                   counts=(37, 17, 0), j_star=3 if n_tau else None, seed=2)
    ref = R1.reference(**R1.call_args(one))
    w = one["weights"]
    unit = torch.tensor([1.0, 0.0], dtype=torch.float64).expand(N.B, 1, 2)
    for delays in (None, torch.zeros(N.B, 1, dtype=torch.float64)) if n_tau else (None,):
        net = N.reference(one["h"], one["data"].unsqueeze(1), unit, delays, w.unsqueeze(0) if w.dim() == 1 else w.unsqueeze(1),
                          one["freqs"], one["taus"], one["n_valid"])
        for name in ("hh", "dd", "dd_rows", "optimal_snr", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix",
                     "lnl_max_mix", "x", "degenerate"):
            assert torch.equal(net[name], ref[name]), (regime, n_tau, name)
        assert torch.equal(net["hh_det"][:, 0], ref["hh"]) and torch.equal(net["dd_det"][:, 0], ref["dd"])
        live = ~ref["degenerate"]
        assert torch.equal(net["snr_det"][live, 0], ref["snr"][live])


def test_planted_data_give_the_identities(all_cases):
    """On the unrounded planted data K_{j*} = HH e^{-i PHI0}: lnl_max = HH / 2, snr = sqrt(HH), phase = -PHI0, tau_index = j*, all to
    1e-12 of their scale.  Detector k holds d_k = C_k h, so kappa_{k,j*} = conj(C_k) hh_k e^{-i PHI0} and its own SNR is
    snr_det_k = |C_k| sqrt(hh_k) -- the detector's optimal SNR, sqrt(hh_k) where |C_k| = 1."""
    n = 0
    for tag, fac, case, _ in all_cases:
        if fac["regime"] != "planted":
            continue
        n += 1
        ref = N.reference(**dict(N.call_args(case), data=case["data64"]))
        live = ~ref["degenerate"]
        HH = ref["hh"][live]
        assert float(((ref["lnl_max"][live] - 0.5 * HH).abs() / HH).max()) <= 1e-12, tag
        assert float(((ref["snr"][live] - HH.sqrt()).abs() / HH.sqrt()).max()) <= 1e-12, tag
        assert float((torch.remainder(ref["phase"][live] + N.PHI0 + math.pi, N.TWO_PI) - math.pi).abs().max()) <= 1e-12, tag
        assert (ref["tau_index"][live] == case["j_star"]).all(), tag
        want = ref["optimal_snr_det"][live]
        assert float(((ref["snr_det"][live] - want).abs() / want.max(1, keepdim=True).values).max()) <= 1e-12, tag
    assert n >= 14


def test_three_wrong_evaluations_miss_the_gates(all_cases):
    """The incoherent sum, delays of the opposite sign and delays rounded to the grid: each is outside the GPU gates against the
    reference: the two delay errors on the planted and the noise cases that have delays, the incoherent sum on the noise cases with
    more than one detector.  On planted data d_k = C_k h every detector's term C_k kappa_{k,j} = |C_k|^2 e^{-i PHI0} sum_t w_k A^2
    e^{i 2 pi f (tau_j - tau_j*)} has the same phase at j* (and, with equal weights, at every j), so there the incoherent sum EQUALS
    the coherent one: it cannot miss a gate on planted data."""
    n = {"incoherent": 0, "sign": 0, "grid": 0}
    for tag, fac, case, ref in all_cases:
        if fac["regime"] not in ("planted", "noise") or ref["degenerate"].all():
            continue
        args = N.call_args(case)
        for kind in n:
            if (kind == "incoherent" and (fac["D"] == 1 or (fac["D"] == 2 and fac["zero_det"] is not None))) or \
                    (kind != "incoherent" and case["delays"] is None) or \
                    (kind == "incoherent" and fac["regime"] == "planted"):
                continue
            bad = N.wrong(kind, **args)
            r = N.ratios({k: bad[k] for k in ("snr", "lnl_max", "lnl_marg")}, ref)
            assert min(r.values()) > 1.0, (tag, kind, r)
            n[kind] += 1
    assert min(n.values()) >= 10, n


def test_every_case_has_a_clear_maximum_and_an_open_phase_filter(all_cases):
    worst, n_open = math.inf, 0
    for tag, fac, case, ref in all_cases:
        live = ~ref["degenerate"]
        if not live.any():
            continue
        norm = (ref["hh"] * ref["dd_rows"]).sqrt()[live]
        x = ref["x"][live]
        if x.shape[1] > 1:
            top = x.topk(2, dim=1).values
            gap = float(((top[:, 0] - top[:, 1]) / norm).min())
            worst = min(worst, gap)
            assert gap >= 1e-6, f"{tag}: runner-up within {gap:.3g} of the best"
        if fac["regime"] in ("planted", "loud", "edge", "bigphase", "noise"):
            ratio = float((x.max(1).values / norm).min())
            assert ratio >= 1e-3, f"{tag}: the phase gate's filter leaves out a row ({ratio:.3g})"
            n_open += 1
    print(f"LOGLIKE_NET smallest runner-up margin {worst:.3g}; phase filter open in {n_open} cases")
    assert n_open >= 5 * 14 - 5


def test_cases_cover_the_factors(all_cases):
    for regime in N.REGIMES:
        mine = [fac for _, fac, _, _ in all_cases if fac["regime"] == regime]
        assert len(mine) >= 14
        assert {f["D"] for f in mine} == set(N.DETS) and {f["n_z"] for f in mine} == {1, 3} and {f["h_ld"] for f in mine} == {2, 4}
        assert {f["T"] for f in mine} == {37, 200} and {f["n_tau"] for f in mine} == {None, 1, 5, JC - 1, JC, JC + 1, 257}
        assert {f["counts"] is None for f in mine} == {True, False}
        assert sum(f["zero_det"] is not None for f in mine) >= 1
    for _, fac, case, _ in all_cases:
        if case["delays"] is not None:
            step = case["taus"][1] if case["taus"] is not None else N.DTAU
            q = case["delays"] / step
            assert float((q - q.round()).abs().min()) >= 0.05  # no delay is a multiple of dtau
            assert float(case["delays"].abs().max()) <= (0.37 * max(fac["n_tau"] or 1, 1) + 0.25) * step
        mod = (case["response"] ** 2).sum(-1).sqrt()
        if fac["zero_det"] is None:
            assert float(mod.min()) >= 0.2 and float(mod.max()) <= 1.5
        else:
            assert (mod[:, fac["zero_det"]] == 0).all()


def test_recurrence_agrees_with_the_direct_form(all_cases):
    """The margin the GPU gate rests on: the recurrence of launch 1 against one complex exp per (k, t, j), error / gate <= 0.1."""
    worst = {}
    for tag, fac, case, ref in all_cases:
        rec = N.recurrence(**N.call_args(case), jc=JC)
        r = N.ratios({k: rec[k] for k in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "phase", "tau_index", "lnl_mix", "lnl_max_mix",
                                          "series", "hh_det", "dd_det", "snr_det")}, ref)
        for k, v in r.items():
            worst[(k, fac["D"])] = max(worst.get((k, fac["D"]), 0.0), v)
        assert _worst(r) <= 0.1, (tag, r)
    for D in N.DETS:
        print(f"LOGLIKE_NET recurrence against direct, D={D}: worst error / gate " +
              ", ".join(f"{k} {v:.3g}" for (k, d), v in sorted(worst.items()) if d == D))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_network_exports_are_declared_bound_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    m = re.search(r"\bint\s+npf_waveform_loglike_net\s*\(([^;]*)\)\s*;", header)
    assert m, "npf_waveform_loglike_net is not declared in include/npf_hip.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    res, args = L.SIGNATURES["npf_waveform_loglike_net"]
    assert res is C.c_int and len(args) == len(decl) == len(NET_ARGS) == 32 and hasattr(lib, "npf_waveform_loglike_net")
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (a, t)
    assert [a.split()[-1].lstrip("*") for a in decl] == NET_ARGS
    for name in OUTPUTS:
        assert (f"int32_t *{name}" if name == "tau_index" else f"double *{name}") in m.group(1), name
    assert "const double *delay" in m.group(1) and "const double *resp" in m.group(1) and "const float *d," in m.group(1)
    assert re.search(r"\bint64_t\s+npf_waveform_loglike_net_workspace_bytes\s*\(\s*int32_t n_rows,\s*int32_t n_det,\s*int32_t n_tau\s*\)\s*;",
                     header)
    assert L.SIGNATURES["npf_waveform_loglike_net_workspace_bytes"] == (C.c_int64, [C.c_int32] * 3)
    assert hasattr(lib, "npf_waveform_loglike_net_workspace_bytes")
    assert int(re.search(r"#define NPF_NET_MAX_DET (\d+)", header).group(1)) == 8
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_workspace_bytes_and_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    ws = lib.npf_waveform_loglike_net_workspace_bytes
    for n_tau, slots in ((0, JC), (1, JC), (JC, JC), (JC + 1, 2 * JC), (65536, 65536)):
        for D in (1, 3, 8):
            assert ws(5, D, n_tau) == 5 * (2 + 2 * D + 2 * slots) * 8, (n_tau, D)  # HH, DD, hh_k, dd_k and whole chunks of (Re, Im)
    assert ws(5, 3, 257) <= lib.npf_waveform_loglike_workspace_bytes(5, 257) + 5 * 8 * 8  # no per-detector series is kept
    for bad in ((0, 2, 4), (-1, 2, 4), (3, 2, -1), (3, 2, 65537), (3, 0, 4), (3, 9, 4), (3, -1, 4)):
        assert ws(*bad) == -1, bad
    buf = (C.c_double * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(h=p, h_ld=2, d=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None, delay=p, resp=p, n_rows=6, n_tasks=2, n_det=3,
              pts=4, tau0=0.0, dtau=1e-3, n_tau=3, **{k: p for k in OUTPUTS}, workspace=p)
    assert list(ok) == NET_ARGS[:-1]
    none = {k: None for k in OUTPUTS}
    for change in (dict(n_rows=5), dict(h_ld=1), dict(h_ld=0), dict(wgt_rows=3), dict(wgt_rows=0), dict(freq_rows=3), dict(freq_rows=0),
                   dict(n_tau=-1), dict(n_tau=65537), dict(freq=None), none, dict(workspace=None), dict(h=None), dict(d=None),
                   dict(pts=0), dict(n_tasks=0), dict(n_rows=0),  # ... what npf_waveform_loglike refuses, and the network's own:
                   dict(n_det=0), dict(n_det=9), dict(n_det=-1), dict(resp=None), dict(freq=None, n_tau=0),  # (delay without freq)
                   dict(freq=None, n_tau=0, delay=None, resp=None)):
        assert lib.npf_waveform_loglike_net(*dict(ok, **change).values(), None) == -1, change


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    FN = A.functional
    assert list(inspect.signature(FN.waveform_loglike_network).parameters) == [
        "h", "data", "response", "delays", "weights", "freqs", "taus", "n_valid", "want", "series"]
    assert FN.LOGLIKE_NET_NAMES == N.NET_NAMES and FN.LOGLIKE_NET_NAMES[:9] == FN.LOGLIKE_NAMES
    assert inspect.signature(FN.waveform_loglike_network).parameters["want"].default == FN.LOGLIKE_NET_NAMES
    assert FN.WaveformLogLikeNetwork._fields == FN.LOGLIKE_NET_NAMES + ("series",) and FN.NET_MAX_DET == 8
    assert list(inspect.signature(A.HeadDistribution.loglike_network).parameters)[1:] == [
        "data", "response", "delays", "weights", "freqs", "taus", "of", "series"]
    assert inspect.signature(A.HeadDistribution.loglike_network).parameters["of"].default == "samples"
    assert A.NetworkLogLike._fields == A.LogLike._fields + ("snr_det", "optimal_snr_det", "dd_det")
    assert "NetworkLogLike" in A.__all__ and "NetworkLogLike" in A.neuralproc.__all__ and A.NetworkLogLike is A.neuralproc.NetworkLogLike
    for word in ("sky position", "sky grid", "gradients", "distance marginalisation", "sub-grid"):
        assert word in A.HeadDistribution.loglike_network.__doc__, word  # what is out of scope is said


def test_every_listed_value_error_is_raised_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, Bn, D = 5, 2, 3
    h, d, f = torch.zeros(4, T, 2), torch.zeros(Bn, D, T, 2), torch.ones(Bn, T)
    resp, dl = torch.ones(Bn, D, 2, dtype=torch.float64), torch.zeros(Bn, D, dtype=torch.float64)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, Bn, T)
    grid = (0.0, 1e-3, 4)
    bad = [
        dict(data=torch.zeros(Bn, D, T, 3)), dict(data=torch.zeros(Bn, D, T + 1, 2)), dict(data=torch.zeros(Bn, T, 2)), dict(data=None),
        dict(data=torch.zeros(Bn, 9, T, 2), response=torch.ones(Bn, 9, 2, dtype=torch.float64)),   # more than NET_MAX_DET detectors
        dict(data=torch.zeros(Bn, 0, T, 2), response=torch.ones(Bn, 0, 2, dtype=torch.float64)),   # none
        dict(data=torch.zeros(3, D, T, 2), response=torch.ones(3, D, 2, dtype=torch.float64)),     # R % B != 0
        dict(response=None), dict(response=resp.float()), dict(response=torch.ones(Bn, D, dtype=torch.float64)),
        dict(response=torch.ones(Bn, D + 1, 2, dtype=torch.float64)), dict(response=torch.ones(D, 2, dtype=torch.float64)),
        dict(delays=dl.float(), freqs=f), dict(delays=torch.zeros(Bn, D + 1, dtype=torch.float64), freqs=f),
        dict(delays=torch.zeros(D, dtype=torch.float64), freqs=f), dict(delays=[0.0] * D, freqs=f),
        dict(delays=dl),                                            # delays without freqs
        dict(weights=torch.ones(T)), dict(weights=torch.ones(Bn, T)), dict(weights=torch.ones(D, T + 1)),
        dict(weights=torch.ones(Bn + 1, D, T)), dict(weights=torch.ones(Bn, D, T, 1)),
        dict(freqs=torch.ones(T - 1), taus=grid), dict(freqs=torch.ones(1, 1, T)), dict(freqs=torch.ones(D, T)),
        dict(taus=grid),                                            # taus without freqs
        dict(freqs=f, taus=(0.0, 1e-3, 0)), dict(freqs=f, taus=(0.0, 1e-3, 65537)), dict(freqs=f, taus=(math.inf, 1e-3, 4)),
        dict(freqs=f, taus=(0.0, 1e-3)), dict(freqs=f, taus=(0.0, 1e-3, 4.0)), dict(freqs=f, taus=torch.tensor([0.0, 1e-3, 4.0])),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            FN.waveform_loglike_network(h, **dict(dict(data=d, response=resp), **kw))
        with pytest.raises(ValueError):
            p.loglike_network(**dict(dict(data=d, response=resp), **kw))
    for hb in (torch.zeros(4, T, 1), torch.zeros(4, T), torch.zeros(0, T, 2)):
        with pytest.raises(ValueError):
            FN.waveform_loglike_network(hb, d, resp)
    for want in (("lnl",), "lnl_marg", None, ()):
        with pytest.raises(ValueError, match="want"):
            FN.waveform_loglike_network(h, d, resp, want=want)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T).loglike_network(d, resp)
    with pytest.raises(ValueError, match="of must be"):
        p.loglike_network(d, resp, of="median")
    for kw in (dict(), dict(delays=dl, freqs=f, taus=grid), dict(weights=torch.ones(D, T), series=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FN.waveform_loglike_network(h, d, resp, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.loglike_network(d, resp, **kw)
    assert p._base is None
