"""Host side of the differentiable waveform mismatch (CPU, no kernel launched): the C ABI of ``npf_waveform_match_ex`` /
``npf_waveform_match_bwd`` and its refusals, the refusals of ``functional.waveform_mismatch``, ``HeadDistribution.mismatch`` and
``MismatchLoss``, and the float64 reference of tests/mismatch_reference.py itself: the closed-form gradient against autograd of the
definition and against a central finite difference, and the runner-up margin of every input set the GPU test uses."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import match_reference as R
import mismatch_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JC = 16


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    assert FN.MATCH_JC == JC
    return [(tag, fac, case, R.reference(**R.call_args(case))) for tag, fac, case in G.cases(JC)]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
FWD_ARGS = ["h", "h_ld", "g", "wgt", "wgt_rows", "freq", "freq_rows", "n_valid", "n_rows", "n_tasks", "pts", "tau0", "dtau", "n_tau"]


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_new_entry_points_are_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    names = {"npf_waveform_match_ex": FWD_ARGS + ["hh", "gg", "overlap", "match", "mismatch", "tau_index", "phase", "corr", "workspace",
                                                  "saved", "stream"],
             "npf_waveform_match_bwd": FWD_ARGS + ["tau_index", "saved", "d_match", "n_bcast", "d_h", "dh_ld", "stream"]}
    for name, want in names.items():
        decl = _declared(header, name)
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl) == len(want) and hasattr(lib, name), name
        assert [a.split()[-1].lstrip("*") for a in decl] == want, name
        for a, t in zip(decl, args):
            assert t is (C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int32), (name, a, t)
    ex, bwd = _declared(header, "npf_waveform_match_ex"), _declared(header, "npf_waveform_match_bwd")
    assert _declared(header, "npf_waveform_match") == ex[:-2] + ex[-1:]  # the existing argument list plus ``saved``
    assert "double *saved" in ex and "const double *saved" in bwd and "const int32_t *tau_index" in bwd and "float *d_h" in bwd
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_backward_refusals_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(h=p, h_ld=2, g=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
              n_tau=3, tau_index=p, saved=p, d_match=p, n_bcast=1, d_h=p, dh_ld=4)
    for change in (dict(n_rows=5), dict(h_ld=1), dict(dh_ld=1), dict(dh_ld=0), dict(n_bcast=0), dict(n_bcast=-1), dict(wgt_rows=3),
                   dict(freq_rows=3), dict(n_tau=-1), dict(n_tau=65537), dict(freq=None), dict(tau_index=None), dict(saved=None),
                   dict(d_match=None), dict(d_h=None), dict(h=None), dict(g=None), dict(pts=0), dict(n_tasks=0), dict(n_rows=0),
                   dict(n_rows=(1 << 24) + 2)):
        a = dict(ok, **change)
        assert lib.npf_waveform_match_bwd(*a.values(), None) == -1, change
    fwd = dict(h=p, h_ld=2, g=p, wgt=p, wgt_rows=1, freq=p, freq_rows=2, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
               n_tau=3, hh=None, gg=None, overlap=None, match=None, mismatch=None, tau_index=None, phase=None, corr=None, workspace=p,
               saved=None)
    assert lib.npf_waveform_match_ex(*fwd.values(), None) == -1  # (no output at all: ``saved`` would have counted as one)
    assert lib.npf_waveform_match_ex(*dict(fwd, saved=p, workspace=None).values(), None) == -1


def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    FN = A.functional
    sig = inspect.signature(FN.waveform_mismatch).parameters
    assert list(sig)[:7] == ["h", "g", "weights", "freqs", "taus", "n_valid", "n_bcast"] and sig["n_bcast"].default == 1
    assert list(inspect.signature(A.HeadDistribution.mismatch).parameters)[1:] == ["Y_ref", "weights", "freqs", "taus", "of"]
    assert inspect.signature(A.HeadDistribution.mismatch).parameters["of"].default == "samples"
    loss = inspect.signature(A.MismatchLoss.__init__).parameters
    assert list(loss)[1:] == ["base", "lam", "weights", "freqs", "taus", "of", "reduction"]
    assert (loss["base"].default, loss["lam"].default, loss["of"].default, loss["reduction"].default) == (None, 1.0, "samples", "mean")
    assert "MismatchLoss" in A.__all__ and "MismatchLoss" in A.losses.__all__ and A.MismatchLoss is A.losses.MismatchLoss
    assert "sigma" in A.MismatchLoss.__doc__ and "subgradient" in FN.waveform_mismatch.__doc__


def test_every_listed_value_error_is_raised_before_the_device_check():
    import npf_gwwaveform_amd as A

    FN = A.functional
    T, Bn = 5, 2
    h, g, w, f = torch.zeros(4, T, 4), torch.zeros(Bn, T, 2), torch.ones(T), torch.ones(Bn, T)
    p = A.HeadDistribution(torch.zeros(4, T, 4), 2, False, 2, Bn, T)
    for kw in (dict(g=torch.zeros(Bn, T, 3)), dict(weights=torch.ones(T + 1)), dict(taus=(0.0, 1e-3, 4)), dict(freqs=f, taus=(0.0, 1e-3, 0)),
               dict(freqs=f, taus=(0.0, math.nan, 4)), dict(g=torch.zeros(3, T, 2))):
        with pytest.raises(ValueError):
            FN.waveform_mismatch(h, **dict(dict(g=g), **kw))
        with pytest.raises(ValueError):
            p.mismatch(**{"Y_ref" if k == "g" else k: v for k, v in dict(dict(g=g), **kw).items()})
    for name, t in (("g", g), ("weights", w), ("freqs", f)):  # no gradient with respect to these
        with pytest.raises(ValueError, match=f"no gradient with respect to {name}"):
            FN.waveform_mismatch(h, **dict(dict(g=g, weights=w, freqs=f), **{name: t.clone().requires_grad_()}))
    for kw in (dict(n_bcast=0), dict(n_bcast=2), dict(n_bcast=1.0), dict(n_bcast=True), dict(mean=torch.zeros(2, T, 2)),
               dict(n_bcast=3, mean=torch.zeros(2, T, 2)), dict(n_bcast=2, mean=torch.zeros(2, T + 1, 2)),
               dict(n_bcast=2, mean=torch.zeros(2, T, 1))):
        with pytest.raises(ValueError):
            FN.waveform_mismatch(h, g, **kw)
    with pytest.raises(ValueError, match="y_dim"):
        A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T).mismatch(g)
    with pytest.raises(ValueError, match="of must be"):
        p.mismatch(g, of="median")
    # and once everything fits, the device check: there is no CPU path
    for kw in (dict(), dict(weights=w, freqs=f, taus=(0.0, 1e-3, 4)), dict(n_bcast=2, mean=torch.zeros(2, T, 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FN.waveform_mismatch(h, g, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.mismatch(g, weights=w)
    assert p._base is None


def test_mismatch_loss_argument_checks_and_buffers():
    import npf_gwwaveform_amd as A

    T, Bn = 5, 2
    w, f = torch.ones(T), torch.ones(Bn, T)
    for kw in (dict(base="nll"), dict(lam=None), dict(lam=math.inf), dict(lam=torch.tensor(1.0)), dict(lam=True), dict(of="median"),
               dict(reduction="max"), dict(weights=[1.0]), dict(weights=torch.ones(T, dtype=torch.float64)), dict(freqs=torch.ones(1, 1, T)),
               dict(weights=torch.ones(T, requires_grad=True)), dict(taus=(0.0, 1e-3, 4)), dict(freqs=f, taus=(0.0, 1e-3)),
               dict(freqs=f, taus=(0.0, 1e-3, 0)), dict(freqs=f, taus=(0.0, 1e-3, 65537)), dict(freqs=f, taus=(0.0, math.inf, 3))):
        with pytest.raises(ValueError):
            A.MismatchLoss(**kw)
    loss = A.MismatchLoss(base=A.CNPFLoss(), lam=10, weights=w, freqs=f, taus=[0.0, 1e-3, 4], of="mean", reduction="sum")
    assert loss.lam == 10.0 and loss.taus == (0.0, 1e-3, 4) and isinstance(loss.base, A.CNPFLoss)
    assert dict(loss.named_buffers()).keys() == {"weights", "freqs"} and "weights" not in loss.state_dict() and "freqs" not in loss.state_dict()
    assert loss.double().freqs.dtype == torch.float64  # (buffers follow the module: .to(device) likewise)
    loss.eval()
    assert not loss.base.training
    plain = A.MismatchLoss()
    assert plain.base is None and plain.weights is None and plain.freqs is None and plain.taus is None
    with pytest.raises(ValueError, match="y_dim"):
        plain((A.HeadDistribution(torch.zeros(4, T, 2), 1, False, 2, Bn, T), None, None, None), torch.zeros(Bn, T, 1))
    with pytest.raises(ValueError, match="predictive distribution"):
        plain((torch.distributions.Normal(0.0, 1.0), None, None, None), torch.zeros(Bn, T, 2))


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_subset_covers_every_regime_and_factor_and_keeps_a_clear_maximum(all_cases):
    """The cases of the GPU test: every regime at both sizes with every n_tau of the subset, both n_z, both h_ld, with and without
    counts -- and in every row with a choice to make the runner-up of max_j |c_j| (normalised) lies at least 1e-6 below the best, so
    the index the gradient is taken at is well posed."""
    closest = math.inf
    for regime in R.REGIMES:
        mine = [fac for _, fac, _, _ in all_cases if fac["regime"] == regime and fac["T"] != 1]
        assert {f["n_tau"] for f in mine} == ({JC + 1, 257} if regime == "shift" else {None, 1, JC, JC + 1, 257}), regime
        assert {f["T"] for f in mine} == {37, 200} and {f["n_z"] for f in mine} == {1, 3} and {f["h_ld"] for f in mine} == {2, 4}, regime
        assert {f["counts"] is None for f in mine} == {True, False}, regime
    assert sum(fac["T"] == 1 for _, fac, _, _ in all_cases) == 1
    for tag, fac, case, ref in all_cases:
        live = ~ref["degenerate"]
        if fac["regime"] == "shift":
            assert (ref["tau_index"][live] == case["j_star"]).all(), tag
        if ref["mag"].shape[1] >= 2 and live.any():
            top = ref["mag"][live].topk(2, dim=1).values
            gap = float((top[:, 0] - top[:, 1]).min())
            closest = min(closest, gap)
            assert gap >= 1e-6, (tag, gap)
    print(f"MISMATCH smallest gap between the best and the runner-up |c_j| over the {len(all_cases)} cases: {closest:.3e}")


def test_differentiable_definition_equals_the_match_reference(all_cases):
    for tag, _, case, ref in all_cases:
        args = R.call_args(case)
        m = G.match_of(args.pop("h").double(), **args)
        assert float((m - ref["match"]).abs().max()) <= 1e-12, tag


def test_closed_form_equals_autograd_of_the_definition(all_cases):
    """Two float64 evaluations of one gradient -- the formulae at the reference's index against autograd through the maximum of the
    definition -- agree to a hundredth of the GPU gate, 2^-23 |ref| / 100 + 1e-11 s_t, in every element of every case; removed and
    padded points (NaN in the inputs) and degenerate rows get exact zeros from both."""
    worst = 0.0
    for tag, fac, case, ref in all_cases:
        args = R.call_args(case)
        h = args.pop("h").double().requires_grad_()
        m = G.match_of(h, **args)
        d_match = torch.randn(m.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        (m * d_match).sum().backward()
        want, s, _ = G.expected(case, d_match, ref=ref)
        assert torch.isfinite(want).all() and torch.isfinite(h.grad).all(), tag
        assert (h.grad[..., 2:] == 0).all(), tag
        r = G.gate_ratio(h.grad[..., :2], want, s)
        worst = max(worst, r)
        assert r <= 1e-2, (tag, r)
        dead = (s == 0)
        assert (want[dead] == 0).all() and (h.grad[..., :2][dead] == 0).all(), tag
        if fac["regime"] == "removed":
            assert dead[case["kill"].repeat(fac["n_z"], 1)].all(), tag
        if fac["regime"] == "degenerate":
            assert dead[ref["degenerate"]].all() and ref["degenerate"].any(), tag
    print(f"MISMATCH closed form vs autograd: worst error / GPU gate {worst:.3e}")


def test_fp32_row_scalars_would_fail_the_gate_where_the_match_is_one(all_cases):
    """Why the forward hands the row scalars over unrounded: in the regimes whose match is 1 up to a constant phase or a time shift
    the true gradient is ~0, and match, phase, hh and sqrt(hh gg) rounded to fp32 leave up to 2^-24 of s_t in it -- sixty times
    the gate's 1e-9 s_t.  (The "same" regime alone does not show it: there psi = 0, M = 1 and hh = N are exact in fp32 too.)"""
    worst = 0.0
    for tag, fac, case, ref in all_cases:
        if fac["regime"] not in ("same", "shift", "offset"):
            continue
        want, s = G.closed_form(**R.call_args(case), ref=ref)
        low, _ = G.closed_form(**R.call_args(case), ref=ref, fp32_scalars=True)
        worst = max(worst, G.gate_ratio(low, want, s))
    print(f"MISMATCH fp32 row scalars where the match is one: worst error / gate {worst:.3e}")
    assert worst > 1.0


def test_closed_form_equals_a_central_finite_difference():
    """One small case (T = 37, three rows, a grid of JC + 1 shifts, weights and counts): (M(h + e) - M(h - e)) / 2e with e = 1e-6 per
    element, through the maximum over the grid.  Truncation e^2 |M'''| ~ 1e-12 and rounding 2^-52 / e ~ 2e-10 against s_t of a few
    1e-2: the bound 1e-6 max s leaves two orders.  The step moves every |c_j| by ~1e-7, inside the 1e-6 margin of the index."""
    case = R.build("random", 37, n_z=1, h_ld=2, wform="BT", fform="T", taus=R.grid(JC + 1), counts=(37, 17, 0), seed=3)
    args = R.call_args(case)
    h = args.pop("h").double()
    want, s = G.closed_form(h, **args)
    eps, fd = 1e-6, torch.zeros_like(want)
    for t in range(37):
        for e in range(2):
            d = torch.zeros_like(h)
            d[:, t, e] = eps
            fd[:, t, e] = (G.match_of(h + d, **args) - G.match_of(h - d, **args)) / (2 * eps)
    err = float((fd - want).abs().max())
    print(f"MISMATCH finite difference vs closed form: max |d| {err:.3e}, max s {float(s.max()):.3e}")
    assert float(want.abs().max()) > 1e-3 and err <= 1e-6 * float(s.max())
    assert (want[1, 17:] == 0).all() and (want[2] == 0).all() and (fd[1, 17:] == 0).all() and (fd[2] == 0).all()


def test_trainer_start_is_one_where_the_objective_lowers_the_mismatch():
    """What the GPU suite's Trainer test relies on, shown on the CPU oracle with the float64 match: from the parameters
    ``specs.make_params(TRAIN_CASE, seed=2)``, 20 Adam steps of ``CNPFLoss + 10 mismatch`` on the fixed batch lower the mean mismatch
    at every second step, 0.417 -> 0.048.  This is a condition on the start, like the runner-up margin on the inputs: with the
    likelihood at ~160 against 10 x 0.3, the first Adam steps from a random start are led by the likelihood, and there are starts
    (seed 5: 0.192 -> 0.337 in this same oracle) where its transient raises the mismatch within 20 steps whatever the gradient of the
    mismatch does."""
    traj = G.oracle_trajectory()
    mm = [m for _, m in traj]
    print("MISMATCH oracle trajectory (NLL, mean mismatch) every 2 steps: " + ", ".join(f"({n:.1f}, {m:.4f})" for n, m in traj[::2]))
    assert len(mm) == 21 and all(b < a for a, b in zip(mm[::2], mm[2::2])), mm
    assert mm[-1] < 0.25 * mm[0] and traj[-1][0] < traj[0][0]
