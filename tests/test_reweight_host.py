"""Host side of the reweighted contexts (CPU, no kernel launched): the float64 references of tests/reweight_cases.py against plain
attention / mean on physically repeated rows, ``bootstrap_weights`` and the k-fold weights on CPU tensors, the C ABI of
``npf_masked_attn_fwd_weighted`` / ``npf_weighted_mean`` and every refusal of the wrappers and of ``Conditioned.reweighted`` /
``kfold`` / ``bootstrap`` / ``model.kfold`` that needs no device."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import reweight_cases as RC
from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "npf_masked_attn_fwd_weighted": ["const float *q", "const float *k", "const float *v", "const float *w", "const int32_t *n_valid",
                                     "const int32_t *n_q_valid", "int32_t n_tasks", "int32_t n_ctx_tasks", "int32_t n_keys",
                                     "int32_t n_queries", "int32_t d", "float scale", "float *out", "void *stream"],
    "npf_weighted_mean": ["const float *R_pt", "const float *w", "const int32_t *n_valid", "int32_t n_tasks", "int32_t n_ctx_tasks",
                          "int32_t pts_per_task", "int32_t F", "float *out", "void *stream"],
}


# ---- the references: an integer weight is "the point appears w times" -------------------------------------------------------
def test_integer_weights_equal_physically_repeated_rows_in_float64():
    g = torch.Generator().manual_seed(3)
    B, C, T, d, S = 2, 11, 5, 8, 3
    Q, K, V = (torch.randn(B, n, d, generator=g, dtype=torch.float64) for n in (T, C, C))
    counts = (11, 7)
    W = torch.randint(0, 4, (S * B, C), generator=g).double()
    W[3] = 0  # (one replicate without any point)
    scale = 1.0 / math.sqrt(d)
    att = RC.weighted_attention(Q, K, V, W, counts, None, scale, torch.float64)
    mean = RC.weighted_mean_ref(V, W, counts, torch.float64)
    for j in range(S * B):
        b = j % B
        w = W[j].clone()
        w[counts[b]:] = 0
        k, v = RC.expand_context(K[b], V[b], w)
        assert k.shape[0] == int(w.sum())
        if k.shape[0] == 0:
            assert (att[j] == 0).all() and (mean[j] == 0).all()
            continue
        plain = torch.softmax(Q[b] @ k.T * scale, dim=-1) @ v
        assert float((att[j] - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
        assert float((mean[j] - v.mean(0)).abs().max()) <= 1e-12 * float(v.mean(0).abs().max())
    # a query count cuts rows only; weights that are negative, NaN or Inf remove the key like 0
    cut = RC.weighted_attention(Q, K, V, W, counts, (5, 2), scale, torch.float64)
    assert float((cut[1, :2] - att[1, :2]).abs().max()) <= 1e-12 and (cut[1, 2:] == 0).all()  # (a matmul of other sizes: not the bits)
    Wbad = W.clone()
    Wbad[W == 0] = torch.tensor([-1.0, math.nan, math.inf], dtype=torch.float64).repeat(C * S * B)[: int((W == 0).sum())]
    assert torch.equal(RC.weighted_attention(Q, K, V, Wbad, counts, None, scale, torch.float64), att)
    assert torch.equal(RC.weighted_mean_ref(V, Wbad, counts, torch.float64), mean)


def test_bootstrap_weights_on_cpu_tensors():
    import npf_gwwaveform_amd as A

    n = torch.tensor([9, 0, 1, 12, 40], dtype=torch.int32)  # (40: clamped to the rows)
    rows, S = 12, 64
    W = A.bootstrap_weights(n, S, rows, generator=torch.Generator().manual_seed(5))
    assert W.shape == (S, 5, rows) and W.dtype == torch.float32
    assert torch.equal(W, W.round()) and (W >= 0).all()
    want = n.clamp(0, rows).float()
    assert torch.equal(W.sum(-1), want.expand(S, 5))
    for b, nb in enumerate(n.clamp(0, rows).tolist()):
        assert (W[:, b, nb:] == 0).all(), f"task {b}: weight beyond its {nb} points"
    # draws with replacement: not the identity, every row of the full task is drawn about once per replicate
    assert (W[:, 3] != 1).any() and (W[:, 3].mean(0) - 1).abs().max() < 0.6
    again = A.bootstrap_weights(n, S, rows, generator=torch.Generator().manual_seed(5))
    assert torch.equal(W, again)
    one = A.bootstrap_weights(7, 3, 10, generator=torch.Generator().manual_seed(1), n_tasks=2)
    assert one.shape == (3, 2, 10) and torch.equal(one.sum(-1), torch.full((3, 2), 7.0)) and (one[:, :, 7:] == 0).all()
    for bad in (dict(S=0), dict(rows=0)):
        with pytest.raises(ValueError, match="S >= 1 and rows >= 1"):
            A.bootstrap_weights(n, **dict(dict(S=2, rows=4), **bad))
    with pytest.raises(ValueError, match="integer tensor"):
        A.bootstrap_weights(torch.zeros(3), 2, 4)


def test_kfold_weights_match_their_definition():
    import npf_gwwaveform_amd as A

    folds = torch.tensor([[0, 0, 1, 1, 2, 3, 3], [2, 2, 2, 2, 2, 2, 2]])
    W = A.kfold_weights(folds, 4)
    assert W.dtype == torch.float32 and torch.equal(W.double(), RC.kfold_weights_ref(folds, 4))
    assert (W[1, 1] == 1).all() and (W[2, 1] == 0).all()  # (a fold that holds no point / every point of the task)
    assert torch.equal(A.kfold_weights(folds.int(), 4), W)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
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
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_exports_refuse_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def attn(q=p, k=p, v=p, w=p, n=p, nq=p, n_tasks=4, n_ctx=2, n_keys=8, T=8, d=32, out=p):
        return lib.npf_masked_attn_fwd_weighted(q, k, v, w, n, nq, n_tasks, n_ctx, n_keys, T, d, 1.0, out, None)

    for bad in (dict(d=0), dict(d=18), dict(d=260), dict(n_tasks=-2), dict(n_keys=-1), dict(T=-1), dict(n_ctx=0), dict(n_ctx=-1),
                dict(n_tasks=5), dict(q=None), dict(out=None), dict(n=None), dict(k=None), dict(v=None), dict(w=None), dict(q=p + 4),
                dict(v=p + 8), dict(out=p + 4), dict(w=p + 2)):
        assert attn(**bad) == -1, bad
    # nothing to do is not an error (and nothing is launched); the query count is optional
    assert attn(n_tasks=0) == 0 and attn(T=0) == 0 and attn(T=0, nq=None) == 0

    def mean(R=p, w=p, n=p, n_tasks=4, n_ctx=2, pts=8, F=32, out=p):
        return lib.npf_weighted_mean(R, w, n, n_tasks, n_ctx, pts, F, out, None)

    for bad in (dict(R=None), dict(w=None), dict(n=None), dict(out=None), dict(n_tasks=-2), dict(n_ctx=0), dict(n_tasks=3), dict(pts=0),
                dict(F=0), dict(F=36), dict(R=p + 4), dict(out=p + 8), dict(w=p + 1)):
        assert mean(**bad) == -1, bad
    assert mean(n_tasks=0) == 0


def test_wrapper_checks_need_no_device():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    assert list(inspect.signature(FN.masked_attention_weighted).parameters) == [
        "q_pt", "k_pt", "v_pt", "w", "n_valid", "n_tasks", "n_ctx_tasks", "n_keys", "n_queries", "d", "scale", "n_q_valid"]
    assert list(inspect.signature(FN.weighted_mean).parameters) == ["R_pt", "w", "n_valid", "n_tasks", "n_ctx_tasks", "pts", "F"]
    z = lambda n, r, d=32: torch.zeros(pt_shape(n, r, d))  # noqa: E731
    ops = lambda: [z(3, 40), z(3, 40), z(3, 40)]  # noqa: E731
    c3 = torch.zeros(3, dtype=torch.int32)  # (on the host: refused last)
    w6 = torch.ones(2, 3, 40)

    def call(o, w=w6, n=6, nc=3, d=32, counts=c3):
        return FN.masked_attention_weighted(o[0], o[1], o[2], w, counts, n, nc, 40, 40, d, 1.0)

    for d in (18, 0, 260):
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            call(ops(), d=d)
    for n, nc in ((7, 3), (6, 0), (-3, 3)):
        with pytest.raises(ValueError, match="multiple of n_ctx_tasks"):
            call(ops(), n=n, nc=nc)
    o = ops()
    o[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        call(o)
    with pytest.raises(RuntimeError, match="inference only"):
        call(ops(), w=torch.ones(2, 3, 40, requires_grad=True))
    o = ops()
    o[1] = z(3, 70)
    with pytest.raises(ValueError, match="k_pt"):
        call(o)
    o = ops()
    o[0] = z(6, 40)  # (the queries are those of the context tasks, shared by the replicates)
    with pytest.raises(ValueError, match="q_pt"):
        call(o)
    with pytest.raises(ValueError, match="w must be a float"):
        call(ops(), w=torch.ones(2, 3, 40, dtype=torch.int32))
    with pytest.raises(ValueError, match="one weight per"):
        call(ops(), w=torch.ones(2, 3, 41))
    with pytest.raises(ValueError, match="one weight per"):
        call(ops(), w=torch.ones(3, 40))
    with pytest.raises(ValueError, match="w must live on the device"):
        call(ops())

    R = z(3, 40, 128)
    with pytest.raises(ValueError, match="R_pt"):
        FN.weighted_mean(R, w6, c3, 6, 3, 70, 128)
    with pytest.raises(ValueError, match="pts >= 1"):
        FN.weighted_mean(R, w6, c3, 6, 3, 0, 128)
    with pytest.raises(ValueError, match="multiple of n_ctx_tasks"):
        FN.weighted_mean(R, w6, c3, 5, 3, 40, 128)
    with pytest.raises(RuntimeError, match="inference only"):
        FN.weighted_mean(z(3, 40, 128).requires_grad_(True), w6, c3, 6, 3, 40, 128)
    with pytest.raises(ValueError, match="w must live on the device"):
        FN.weighted_mean(R, w6, c3, 6, 3, 40, 128)


# ---- the public interface -------------------------------------------------------------------------------------------------------
def _state(m, B=2, C=6, capacity=None, r=128, counts=None):
    """A conditioned state of CPU tensors that holds the row tensors (nothing is launched on it)."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.chain import PTensor, pt_shape

    rows = C if capacity is None else capacity
    Xc, R = (PTensor(torch.zeros(pt_shape(B, rows, r)), rows, r) for _ in range(2))
    return A.Conditioned(m, Xc, R if m._attentive else torch.zeros(B, 1, r), None, None, counts, B, C, False, capacity=capacity, R_pts=R)


def test_entry_points_and_their_refusals():
    import npf_gwwaveform_amd as A

    assert {"Reweighted", "KeyWeights", "bootstrap_weights"} <= set(A.__all__)
    assert list(inspect.signature(A.Conditioned.reweighted).parameters) == ["self", "W"]
    assert list(inspect.signature(A.Reweighted.query).parameters) == ["self", "X_trgt", "n_trgt"]
    assert list(inspect.signature(A.Conditioned.kfold).parameters) == ["self", "folds", "k"]
    assert list(inspect.signature(A.Conditioned.bootstrap).parameters) == ["self", "X_trgt", "n_samples", "generator"]
    assert list(inspect.signature(A.NeuralProcessFamily.kfold).parameters)[1:] == ["X_cntxt", "Y_cntxt", "folds", "k", "n_cntxt"]
    assert list(inspect.signature(A.bootstrap_weights).parameters)[:5] == ["n_cntxt_or_C", "S", "rows", "generator", "device"]
    X, Y = torch.zeros(2, 6, 1), torch.zeros(2, 6, 2)
    folds = torch.zeros(2, 6, dtype=torch.int64)
    for kind in ("CNP", "AttnCNP"):
        m = _model(kind, 128).eval()
        for capacity, rows in ((None, 6), (10, 10)):
            post = _state(m, capacity=capacity)
            for W, what in ((torch.ones(2, rows), r"\[S >= 1, B=2"), (torch.ones(3, 2, rows + 1), "rows="), (torch.ones(3, 3, rows), "B=2"),
                            (torch.ones(0, 2, rows), "S >= 1"), (torch.ones(3, 2, rows, dtype=torch.int64), "float"),
                            ([[1.0]], "float")):
                with pytest.raises(ValueError, match=what):
                    post.reweighted(W)
            with pytest.raises(ValueError, match="W lives on meta"):
                post.reweighted(torch.ones(3, 2, rows, device="meta"))
            with pytest.raises(RuntimeError, match="inference only"):
                post.reweighted(torch.ones(3, 2, rows, requires_grad=True))
            rw = post.reweighted(torch.ones(3, 2, rows))  # (valid arguments: nothing is launched until the query)
            assert isinstance(rw, A.Reweighted) and rw.S == 3 and rw.rows == rows
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                rw.query(torch.zeros(2, 4, 1))
            with pytest.raises(ValueError, match="n_samples must be at least 1"):
                post.bootstrap(torch.zeros(2, 4, 1), 0)
            f = torch.zeros(2, rows, dtype=torch.int64)
            for bad_k in (1, 0, -3):
                with pytest.raises(ValueError, match="k must be at least 2"):
                    post.kfold(f, bad_k)
            with pytest.raises(ValueError, match="folds must be an integer"):
                post.kfold(f.float(), 3)
            with pytest.raises(ValueError, match=r"folds must be \[B=2"):
                post.kfold(f[:, :-1], 3)
            with pytest.raises(ValueError, match="folds lives on meta"):
                post.kfold(f.to("meta"), 3)
        # the model-level form
        for bad_k in (1, 0):
            with pytest.raises(ValueError, match="k must be at least 2"):
                m.kfold(X, Y, folds, bad_k)
        with pytest.raises(ValueError, match="folds must be an integer"):
            m.kfold(X, Y, folds.double(), 3)
        with pytest.raises(ValueError, match=r"folds must be \[B=2, rows=6\]"):
            m.kfold(X, Y, folds[:1], 3)
        with pytest.raises(ValueError, match="no context points"):
            m.kfold(X[:, :0], Y[:, :0], folds[:, :0], 3)
        with pytest.raises(ValueError, match="X_cntxt / Y_cntxt"):
            m.kfold(X, Y[:, :5], folds, 3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # (valid arguments: on to the tensors)
            m.kfold(X, Y, folds, 3)
    # latent models: kfold is refused through a message of its own, reweighted is not
    for kind, kw in (("LNP", dict(encoded_path="latent")), ("AttnLNP", {})):
        m = _model(kind, 128, **kw).eval()
        with pytest.raises(NotImplementedError, match="kfold.*latent"):
            m.kfold(X, Y, folds, 3)
        with pytest.raises(NotImplementedError, match="kfold.*latent"):
            _state(m, capacity=10).kfold(torch.zeros(2, 10, dtype=torch.int64), 3)
        assert isinstance(_state(m, capacity=10).reweighted(torch.ones(1, 2, 10)), A.Reweighted)
    sa = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)
    with pytest.raises(NotImplementedError, match="kfold.*is_self_attn"):
        sa.kfold(X, Y, folds, 3)
    for call in (lambda p: p.reweighted(torch.ones(1, 2, 6)), lambda p: p.bootstrap(torch.zeros(2, 4, 1), 2)):
        with pytest.raises(NotImplementedError, match="reweighted.*is_self_attn"):
            call(A.Conditioned(sa, None, None, None, None, None, 2, 6, False))
    # states that do not hold the row tensors: the refusals of sample_functions
    att, cnp = _model("AttnCNP", 128).eval(), _model("CNP", 128).eval()
    for call, what in ((lambda p: p.reweighted(torch.ones(1, p.B, p.C)), "reweighted"),
                       (lambda p: p.kfold(torch.zeros(p.B, p.C, dtype=torch.int64), 2), "kfold")):
        with pytest.raises(ValueError, match=f"{what}.*n_cntxt.*capacity"):  # (stored for the fused target side, no counts)
            call(A.Conditioned(att, None, None, None, None, None, 2, 6, True))
        with pytest.raises(ValueError, match=f"{what}.*does not hold"):
            call(A.Conditioned(cnp, None, torch.zeros(2, 1, 128), None, None, None, 2, 6, False))
        with pytest.raises(ValueError, match=f"{what}: no context points"):
            call(A.Conditioned(att, None, None, None, None, None, 2, 0, False))


def test_refused_in_the_bf16_mode(bf16_mode):  # noqa: F811
    m = _model("AttnCNP", 128).eval()
    post = _state(m, capacity=10, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="reweighted.*bf16"):
        post.reweighted(torch.ones(2, 2, 10))
    with pytest.raises(NotImplementedError, match="reweighted.*bf16"):
        post.bootstrap(torch.zeros(2, 4, 1), 2)
    with pytest.raises(NotImplementedError, match="kfold.*bf16"):
        post.kfold(torch.zeros(2, 10, dtype=torch.int64), 3)
    with pytest.raises(NotImplementedError, match="kfold.*bf16"):
        m.kfold(torch.zeros(2, 6, 1), torch.zeros(2, 6, 2), torch.zeros(2, 6, dtype=torch.int64), 3)
