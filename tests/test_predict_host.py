"""Host side of conditioned prediction (CPU, no kernel launched): the C ABI of ``npf_mixture_summary``, the methods on the four
model classes, the ``probs`` checks and the standard-normal quantiles of the host helper, and the refusals of ``condition`` /
``query`` (bf16 mode or self-attention with counts, CPU tensors) -- the ones ``forward`` raises."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("CNP", "LNP", "AttnCNP", "AttnLNP")


def _build(kind, r=128):
    return _model(kind, r, **(dict(encoded_path="latent") if kind == "LNP" else {}))


def test_mixture_summary_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    name = "npf_mixture_summary"
    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    lib = C.CDLL(L.lib_path())
    assert hasattr(lib, name), f"{name} is not exported"
    res, args = L.SIGNATURES[name]
    decl = [a.strip() for a in m.group(1).split(",")]
    assert res is C.c_int and len(args) == len(decl) == 14
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_int32), (a, t)
    assert "const int32_t *n_valid" in m.group(1) and decl[-1] == "void *stream"
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (a new export, the old ones unchanged: the ABI version stays)
    assert not hasattr(lib, "npf_debug_mixture_iters")  # the solver's step counter is compiled out of the shipped build


def test_mixture_summary_refuses_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    ok = dict(suff=p, n_valid=None, n_z=2, n_tasks=1, pts=4, dy=1, homosk=0, z_p=p, n_probs=1, probs=p, mean=p, std=p, quant=p)
    for change in (dict(n_z=0), dict(n_z=129), dict(dy=0), dict(dy=17), dict(pts=0), dict(n_tasks=0), dict(n_tasks=65536),
                   dict(suff=None), dict(mean=None), dict(std=None), dict(n_probs=-1), dict(z_p=None), dict(probs=None),
                   dict(quant=None)):
        a = dict(ok, **change)
        assert lib.npf_mixture_summary(*a.values(), None) == -1, change


@pytest.mark.parametrize("kind", KINDS)
def test_models_have_condition_query_predict(kind):
    import npf_gwwaveform_amd as A

    cls = getattr(A, kind)
    assert list(inspect.signature(cls.condition).parameters)[1:] == ["X_cntxt", "Y_cntxt", "n_cntxt", "n_z_samples"]
    assert list(inspect.signature(cls.predict).parameters)[1:] == ["X_cntxt", "Y_cntxt", "X_trgt", "n_cntxt", "n_trgt", "n_z_samples",
                                                                   "probs"]
    assert inspect.signature(cls.predict).parameters["probs"].default == (0.025, 0.5, 0.975)
    assert list(inspect.signature(A.Conditioned.query).parameters)[1:] == ["X_trgt", "n_trgt"]
    assert A.Prediction._fields == ("mean", "std", "quantiles", "probs")
    assert inspect.signature(A.HeadDistribution.summary).parameters["probs"].default == (0.025, 0.5, 0.975)
    assert list(inspect.signature(A.functional.mixture_summary).parameters) == ["suff", "n_z", "dy", "homoskedastic", "probs", "n_valid"]


def test_probs_are_checked_on_the_host():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(2, 3, 4), 2, False, 1, 2, 3)
    for bad in ((0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,), (float("nan"),), torch.tensor([0.1, 0.9]), (torch.tensor(0.5),), 0.5, "0.5"):
        with pytest.raises(ValueError, match="probs"):
            p.summary(bad)
        with pytest.raises(ValueError, match="probs"):
            A.functional.mixture_summary(torch.zeros(2, 3, 4), 1, 2, False, probs=bad)
        with pytest.raises(ValueError, match="probs"):
            _build("CNP").predict(torch.zeros(2, 4, 1), torch.zeros(2, 4, 2), torch.zeros(2, 3, 1), probs=bad)
    assert p._base is None


def test_normal_quantiles_equal_float64_ndtri():
    from npf_gwwaveform_amd import functional as FN

    probs = (1e-9, 1e-4, 0.025, 0.1, 0.31, 0.5, 0.69, 0.9, 0.975, 1 - 1e-4, 1 - 1e-9)
    z = FN.normal_quantiles(probs)
    ref = torch.special.ndtri(torch.tensor(probs, dtype=torch.float64))
    assert len(z) == len(probs) and all(isinstance(v, float) for v in z)
    assert (torch.tensor(z, dtype=torch.float64) - ref).abs().max().item() <= 1e-12
    assert z[5] == 0.0 and abs(z[2] + 1.959963984540054) <= 1e-12 and abs(z[8] - 1.959963984540054) <= 1e-12
    assert FN.normal_quantiles(()) == ()


def _xy(B=2, C=6, T=5):
    return torch.zeros(B, C, 1), torch.zeros(B, C, 2), torch.zeros(B, T, 1)


def test_refusals_with_counts_are_those_of_forward(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    Xc, Yc, Xt = _xy()
    n = torch.zeros(2, dtype=torch.int32)
    m = _model("AttnCNP", 128)
    with pytest.raises(NotImplementedError, match="n_cntxt.*bf16"):
        m.condition(Xc, Yc, n_cntxt=n)
    with pytest.raises(NotImplementedError, match="n_cntxt.*bf16"):
        m.predict(Xc, Yc, Xt, n_cntxt=n)
    post = A.Conditioned(m, None, None, None, None, None, 2, 0, False)
    with pytest.raises(NotImplementedError, match="n_trgt.*bf16"):
        post.query(Xt, n_trgt=n)
    sa = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)
    with pytest.raises(NotImplementedError, match="n_cntxt.*is_self_attn"):
        sa.condition(Xc, Yc, n_cntxt=n)
    with pytest.raises(NotImplementedError, match="n_trgt.*is_self_attn"):
        A.Conditioned(sa, None, None, None, None, None, 2, 0, False).query(Xt, n_trgt=n)


@pytest.mark.parametrize("kind", KINDS)
def test_cpu_tensors_and_bad_counts_are_refused(kind):
    import npf_gwwaveform_amd as A

    m = _build(kind)
    Xc, Yc, Xt = _xy()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.condition(Xc, Yc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(Xc, Yc, Xt)
    post = A.Conditioned(m, None, None, None, None, None, 2, 0, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post.query(Xt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.functional.mixture_summary(torch.zeros(2, 3, 4), 1, 2, False)
    with pytest.raises(ValueError, match="n_cntxt.*device"):  # (counts are device data, as in forward)
        m.condition(Xc, Yc, n_cntxt=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_trgt.*device"):
        post.query(Xt, n_trgt=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        post.query(Xt, n_trgt=torch.zeros(3, dtype=torch.int32))
    if kind in ("LNP", "AttnLNP"):
        with pytest.raises(ValueError, match="n_z_samples"):
            m.condition(Xc, Yc, n_z_samples=0)
