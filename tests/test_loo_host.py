"""Host side of the leave-one-out predictions (CPU, no kernel launched): the C ABI of ``npf_masked_attn_fwd_loo`` / ``npf_loo_mean``,
the argument checks of the library entries and of ``functional.masked_attention_loo`` / ``functional.loo_mean`` that need no device,
and the refusals of ``model.loo`` / ``Conditioned.loo``."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "npf_masked_attn_fwd_loo": ["const float *q", "const float *k", "const float *v", "const int32_t *n_valid", "const int32_t *n_q_valid",
                                "int32_t n_tasks", "int32_t n_keys", "int32_t n_queries", "int32_t d", "float scale", "float *out",
                                "void *stream"],
    "npf_loo_mean": ["const float *R_pt", "const int32_t *n_valid", "int32_t n_tasks", "int32_t pts_per_task", "int32_t F", "float *out",
                     "void *stream"],
}


@pytest.mark.parametrize("name", list(DECLS))
def test_exports_are_declared_exported_and_typed(name):
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    lib = C.CDLL(L.lib_path())
    assert hasattr(lib, name), f"{name} is not exported"
    res, args = L.SIGNATURES[name]
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert decl == DECLS[name]
    assert res is C.c_int and len(args) == len(decl)
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int32), (a, t)
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_exports_refuse_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def attn(q=p, k=p, v=p, n=p, nq=p, n_tasks=2, n_keys=8, T=8, d=32, out=p):
        return lib.npf_masked_attn_fwd_loo(q, k, v, n, nq, n_tasks, n_keys, T, d, 1.0, out, None)

    for bad in (dict(d=0), dict(d=18), dict(d=260), dict(n_tasks=-1), dict(n_keys=-1), dict(T=-1), dict(q=None), dict(out=None),
                dict(n=None), dict(k=None), dict(v=None), dict(q=p + 4), dict(v=p + 8), dict(out=p + 4)):
        assert attn(**bad) == -1, bad
    # nothing to do is not an error (and nothing is launched); the query count is optional
    assert attn(n_tasks=0) == 0 and attn(T=0) == 0 and attn(T=0, nq=None) == 0

    def mean(R=p, n=p, n_tasks=2, pts=8, F=32, out=p):
        return lib.npf_loo_mean(R, n, n_tasks, pts, F, out, None)

    for bad in (dict(R=None), dict(n=None), dict(out=None), dict(n_tasks=-1), dict(n_tasks=65536), dict(pts=0), dict(F=0), dict(F=36),
                dict(R=p + 4), dict(out=p + 8)):
        assert mean(**bad) == -1, bad
    assert mean(n_tasks=0) == 0


def test_wrapper_checks_need_no_device():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    assert list(inspect.signature(FN.masked_attention_loo).parameters) == [
        "q_pt", "k_pt", "v_pt", "n_valid", "n_tasks", "n_keys", "n_queries", "d", "scale", "n_q_valid"]
    assert inspect.signature(FN.masked_attention_loo).parameters["n_q_valid"].default is None
    assert list(inspect.signature(FN.loo_mean).parameters) == ["R_pt", "n_valid", "n_tasks", "pts", "F"]
    z = lambda n, r, d=32: torch.zeros(pt_shape(n, r, d))  # noqa: E731
    ops = lambda: [z(3, 40), z(3, 40), z(3, 40)]  # noqa: E731
    c3 = torch.zeros(3, dtype=torch.int32)  # (on the host: refused last)

    def call(o, n=3, d=32, counts=c3, nq=None):
        return FN.masked_attention_loo(o[0], o[1], o[2], counts, n, 40, 40, d, 1.0, n_q_valid=nq)

    for d in (18, 0, 260):
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            call(ops(), d=d)
    for i in range(3):
        o = ops()
        o[i].requires_grad_(True)
        with pytest.raises(RuntimeError, match="inference only"):
            call(o)
        with torch.no_grad(), pytest.raises(RuntimeError, match="inference only"):
            call(o)
    o = ops()
    o[1] = z(3, 70)
    with pytest.raises(ValueError, match="k_pt"):
        call(o)
    o = ops()
    o[2] = z(3, 40).double()
    with pytest.raises(ValueError, match="v_pt"):
        call(o)
    with pytest.raises(ValueError, match="negative size"):
        call(ops(), n=-1)
    with pytest.raises(ValueError, match="n_valid.*device"):
        call(ops())
    with pytest.raises(ValueError, match=r"n_valid must have shape \[3\]"):
        call(ops(), counts=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32 or int64"):
        call(ops(), counts=torch.zeros(3))

    R = z(3, 40, 128)
    with pytest.raises(ValueError, match="R_pt"):
        FN.loo_mean(R, c3, 3, 70, 128)
    with pytest.raises(ValueError, match="pts >= 1"):
        FN.loo_mean(R, c3, 3, 0, 128)
    with pytest.raises(RuntimeError, match="inference only"):
        FN.loo_mean(z(3, 40, 128).requires_grad_(True), c3, 3, 40, 128)
    with pytest.raises(ValueError, match="n_valid.*device"):
        FN.loo_mean(R, c3, 3, 40, 128)


def test_entry_points_and_their_refusals():
    import npf_gwwaveform_amd as A

    assert list(inspect.signature(A.NeuralProcessFamily.loo).parameters)[1:] == ["X_cntxt", "Y_cntxt", "n_cntxt"]
    assert inspect.signature(A.NeuralProcessFamily.loo).parameters["n_cntxt"].default is None
    assert list(inspect.signature(A.Conditioned.loo).parameters) == ["self"]
    X, Y = torch.zeros(2, 6, 1), torch.zeros(2, 6, 2)
    counts = torch.zeros(2, dtype=torch.int32)
    # latent models: q(z | C without i) differs per left-out point
    for kind, kw in (("LNP", dict(encoded_path="latent")), ("AttnLNP", {})):
        m = _model(kind, 128, **kw).eval()
        with pytest.raises(NotImplementedError, match="loo.*latent"):
            m.loo(X, Y)
        with pytest.raises(NotImplementedError, match="loo.*latent"):
            A.Conditioned(m, None, None, None, None, counts, 2, 6, False, capacity=10).loo()
    sa = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)
    with pytest.raises(NotImplementedError, match="loo.*is_self_attn"):
        sa.loo(X, Y)
    with pytest.raises(NotImplementedError, match="loo.*is_self_attn"):
        A.Conditioned(sa, None, None, None, None, None, 2, 6, False).loo()
    for kind in ("CNP", "AttnCNP"):
        m = _model(kind, 128).eval()
        with pytest.raises(ValueError, match="no context points"):
            m.loo(X[:, :0], Y[:, :0])
        with pytest.raises(ValueError, match="X_cntxt / Y_cntxt"):
            m.loo(X, Y[:, :5])
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # (valid arguments: on to the tensors)
            m.loo(X, Y)
        with pytest.raises(ValueError, match="n_cntxt.*device"):
            m.loo(X, Y, n_cntxt=counts)
    # states that do not hold the row tensors
    att, cnp = _model("AttnCNP", 128).eval(), _model("CNP", 128).eval()
    with pytest.raises(ValueError, match="n_cntxt.*capacity"):  # (stored for the fused target side, no counts)
        A.Conditioned(att, None, None, None, None, None, 2, 6, True).loo()
    with pytest.raises(ValueError, match="pooled representation.*capacity"):
        A.Conditioned(cnp, None, torch.zeros(2, 1, 128), None, None, None, 2, 6, False).loo()
    with pytest.raises(ValueError, match="no context points"):
        A.Conditioned(att, None, None, None, None, None, 2, 0, False).loo()


def test_refused_in_the_bf16_mode(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    m = _model("AttnCNP", 128).eval()
    with pytest.raises(NotImplementedError, match="loo.*bf16"):
        m.loo(torch.zeros(2, 6, 1), torch.zeros(2, 6, 2))
    with pytest.raises(NotImplementedError, match="loo.*bf16"):
        A.Conditioned(m, None, None, None, None, torch.zeros(2, dtype=torch.int32), 2, 6, False, capacity=10).loo()
