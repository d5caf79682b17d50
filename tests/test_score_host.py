"""Host side of the predictive scores (CPU, no kernel launched): the C ABI of ``npf_mixture_score``, the refusals of
``functional.mixture_score`` and ``HeadDistribution.score``, and the float64 reference of tests/score_reference.py itself -- its CRPS
closed form against a numerical integral, and the margin the six input regimes of the GPU test leave a plain float32 evaluation."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import score_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixture_score_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    name = "npf_mixture_score"
    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    lib = C.CDLL(L.lib_path())
    assert hasattr(lib, name), f"{name} is not exported"
    res, args = L.SIGNATURES[name]
    decl = [a.strip() for a in m.group(1).split(",")]
    assert res is C.c_int and len(args) == len(decl) == 12
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_int32), (a, t)
    assert [a.split()[-1].lstrip("*") for a in decl] == ["suff", "Y", "n_valid", "n_z", "n_tasks", "pts", "dy", "homoskedastic",
                                                        "log_density", "pit", "crps", "stream"]
    assert "const int32_t *n_valid" in m.group(1) and decl[-1] == "void *stream"
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (a new export, the old ones unchanged: the ABI version stays)


def test_mixture_score_refuses_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(suff=p, Y=p, n_valid=None, n_z=2, n_tasks=1, pts=4, dy=1, homosk=0, log_density=p, pit=p, crps=p)
    for change in (dict(n_z=0), dict(n_z=129), dict(dy=0), dict(dy=17), dict(pts=0), dict(n_tasks=0), dict(n_tasks=65536),
                   dict(suff=None), dict(Y=None), dict(pts=(1 << 30) + 1), dict(pts=(1 << 27) + 1, dy=8),
                   dict(log_density=None, pit=None, crps=None)):
        a = dict(ok, **change)
        assert lib.npf_mixture_score(*a.values(), None) == -1, change


def test_signatures_and_exports():
    import npf_gwwaveform_amd as A

    assert list(inspect.signature(A.functional.mixture_score).parameters) == ["suff", "Y", "n_z", "dy", "homoskedastic", "n_valid", "want"]
    assert inspect.signature(A.functional.mixture_score).parameters["want"].default == ("log_density", "pit", "crps")
    assert list(inspect.signature(A.HeadDistribution.score).parameters)[1:] == ["Y_trgt", "want"]
    assert inspect.signature(A.HeadDistribution.score).parameters["want"].default == ("log_density", "pit", "crps")
    assert A.Score._fields == ("log_density", "pit", "crps")
    assert "Score" in A.__all__ and "Score" in A.neuralproc.__all__ and A.Score is A.neuralproc.Score


def test_cpu_tensors_wrong_shapes_and_unknown_names_are_refused():
    import npf_gwwaveform_amd as A

    suff, Y = torch.zeros(2, 3, 4), torch.zeros(2, 3, 2)
    p = A.HeadDistribution(suff, 2, False, 1, 2, 3)
    for bad in (("density",), ("pit", "CRPS"), "pit", (), None, 3, ("pit", 1)):
        with pytest.raises(ValueError, match="want"):
            A.functional.mixture_score(suff, Y, 1, 2, False, want=bad)
        with pytest.raises(ValueError, match="want"):
            p.score(Y, want=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.functional.mixture_score(suff, Y, 1, 2, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.score(Y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.score(Y, want=("pit",))
    assert p._base is None
    if torch.cuda.is_available():  # (the shape checks come after the device check, as in mixture_summary)
        d = torch.zeros(2, 3, 4, device="cuda")
        for n_z, dy, y_shape, exc in ((1, 3, (2, 3, 3), ValueError), (0, 2, (2, 3, 2), ValueError), (4, 2, (2, 3, 2), ValueError),
                                      (1, 2, (1, 2, 3, 2), ValueError), (1, 2, (2, 3, 1), ValueError), (2, 2, (2, 3, 2), ValueError)):
            with pytest.raises(exc):
                A.functional.mixture_score(d, torch.zeros(*y_shape, device="cuda"), n_z, dy, False)
        with pytest.raises(NotImplementedError, match="128"):
            A.functional.mixture_score(torch.zeros(129, 1, 2, device="cuda"), torch.zeros(1, 1, 1, device="cuda"), 129, 1, False)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def _crps_by_integration(mu, sg, y, n):
    """integral of (F(x) - 1[x >= y])^2 dx by the trapezoid rule in float64, split at y (the integrand jumps there): ``n`` intervals
    on [lo, y] and ``n`` on [y, hi], lo / hi 12 of the largest sigma beyond the extreme means and y (the tails left out are below
    exp(-72))."""
    lo = min(float(mu.min()), y) - 12.0 * float(sg.max())
    hi = max(float(mu.max()), y) + 12.0 * float(sg.max())
    F = lambda x: (0.5 * torch.special.erfc(-(x.unsqueeze(0) - mu.unsqueeze(1)) / (sg.unsqueeze(1) * math.sqrt(2.0)))).mean(0)  # noqa: E731
    left, right = torch.linspace(lo, y, n + 1, dtype=torch.float64), torch.linspace(y, hi, n + 1, dtype=torch.float64)
    return float(torch.trapezoid(F(left) ** 2, left) + torch.trapezoid((1.0 - F(right)) ** 2, right))


def test_reference_crps_equals_the_integral_of_the_squared_cdf_difference():
    """Grid: 2^15 intervals on either side of y (step about 1e-3 at these mixtures), against 2^14.  The trapezoid rule's error falls
    with the square of the step, so the finer integral is off by a third of what halving the step moved it; the closed form must
    agree with the finer integral within the whole of that move, per mixture, and with the Richardson-extrapolated integral
    (fine + (fine - coarse) / 3) to 1e-9 relative.  Measured: halving moves the integral by at most 6.2e-8 relative, closed form
    against the finer integral 2.1e-8; both are printed."""
    g = torch.Generator().manual_seed(5)
    worst, worst_halving, worst_rich = 0.0, 0.0, 0.0
    for K in (1, 2, 3, 8):
        for _ in range(3):
            mu = 3.0 * torch.randn(K, generator=g, dtype=torch.float64)
            sg = 0.3 + 1.7 * torch.rand(K, generator=g, dtype=torch.float64)
            y = float(4.0 * torch.randn((), generator=g, dtype=torch.float64))
            closed = float(R.scores(mu.view(K, 1), sg.view(K, 1), torch.tensor([y], dtype=torch.float64))[2])
            fine, coarse = _crps_by_integration(mu, sg, y, 1 << 15), _crps_by_integration(mu, sg, y, 1 << 14)
            assert abs(closed - fine) <= abs(fine - coarse), (K, closed, fine, coarse)
            worst = max(worst, abs(closed - fine) / closed)
            worst_halving = max(worst_halving, abs(fine - coarse) / closed)
            worst_rich = max(worst_rich, abs(closed - (fine + (fine - coarse) / 3.0)) / closed)
    print(f"SCORE reference CRPS: closed form vs integral {worst:.3e} relative, step halving moves the integral by {worst_halving:.3e}, "
          f"closed form vs the extrapolated integral {worst_rich:.3e}")
    assert worst_halving <= 1e-6 and worst_rich <= 1e-9


def test_reference_log_density_and_pit_of_one_gaussian():
    mu, sg, y = torch.tensor([[0.3]], dtype=torch.float64), torch.tensor([[1.7]], dtype=torch.float64), torch.tensor([2.0], dtype=torch.float64)
    ld, pit, crps = R.scores(mu, sg, y)
    n = torch.distributions.Normal(mu[0], sg[0])
    u = (y - mu[0]) / sg[0]
    assert abs(float(ld - n.log_prob(y))) <= 1e-14 and abs(float(pit - n.cdf(y))) <= 1e-14
    gauss = sg[0] * (u * (2 * n.cdf(y) - 1) + 2 * torch.exp(n.log_prob(y)) * sg[0] - 1 / math.sqrt(math.pi))  # Gneiting & Raftery (2007), eq. 21
    assert abs(float(crps - gauss)) <= 1e-14


@pytest.mark.parametrize("n_z", (1, 2, 8, 33, 128))
@pytest.mark.parametrize("name", R.REGIMES)
def test_regimes_leave_a_float32_evaluation_a_margin_of_four(name, n_z):
    """The gates are reachable in fp32 on these inputs: the closed forms evaluated in plain float32 torch (CPU) stay inside 0.25 of each
    gate against the float64 reference, 512 elements per regime."""
    mu, raw, y = R.regime(name, n_z, 512, seed=100 * n_z + R.REGIMES.index(name))
    ref = R.scores(mu.double(), R.sigma_of(raw.double()), y.double())
    got = R.scores(mu, R.sigma_of(raw), y)
    r = R.ratios(got, ref)
    print(f"SCORE float32 evaluation, {name} n_z={n_z}: error / gate " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(torch.isfinite(t).all() for t in ref) and float(ref[2].min()) > 0.0
    assert max(r.values()) <= 0.25, r
