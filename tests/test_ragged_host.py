"""Host side of padded targets (CPU, no kernel launched): the C ABI of the new exports, the argument checks and refusals of
``forward(..., n_trgt=...)``, per-task target draws of ``GetRandomIndcs`` / ``CntxtTrgtGetter`` and the split of a padded data set
(``n_points``) without a host sync, and the batch keys ``Trainer`` / ``eval_loglike`` pass on."""
import ctypes as C
import os
import re

import pytest
import torch

from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

NEW = ("npf_masked_gauss_head_fwd", "npf_masked_gauss_head_bwd", "npf_masked_attn_fwd_nq", "npf_masked_attn_bwd_nq")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/npf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = L.SIGNATURES[name]
        decl = [a.strip() for a in m.group(1).split(",")]
        assert res is C.c_int and len(args) == len(decl), name
        for a, t in zip(decl, args):
            want = C.c_void_p if "*" in a else (C.c_float if a.startswith("float") else C.c_int32)
            assert t is want, (name, a, t)
        assert "const int32_t *n_valid" in m.group(1) and decl[-1] == "void *stream", name
        if name.endswith("_nq"):
            assert "const int32_t *n_q_valid" in m.group(1), name
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (new exports, the old ones unchanged: the ABI version stays)


def test_new_exports_refuse_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    # head: dy out of range, rows not a multiple of the tasks, no counts, a launch that writes nothing
    assert lib.npf_masked_gauss_head_fwd(p, p, 1, 1, 4, 17, 0, p, 1, p, p, p, None) == -1
    assert lib.npf_masked_gauss_head_fwd(p, p, 2, 3, 4, 1, 0, p, 1, p, p, p, None) == -1
    assert lib.npf_masked_gauss_head_fwd(p, None, 1, 1, 4, 1, 0, p, 1, p, p, p, None) == -1
    assert lib.npf_masked_gauss_head_fwd(p, p, 1, 1, 4, 1, 0, None, 0, None, None, None, None) == -1
    assert lib.npf_masked_gauss_head_bwd(p, None, None, p, 1, 1, 0, 1, 0, p, 1, None, None, p, p, None) == -1
    assert lib.npf_masked_gauss_head_bwd(p, None, None, None, 1, 1, 4, 1, 0, p, 1, None, None, p, p, None) == -1
    # attention: the checks of the exports without a query count, and a missing query count
    for d in (30, 260, 0):
        assert lib.npf_masked_attn_fwd_nq(p, p, p, p, p, 1, 4, 4, d, 1.0, p, None, None) == -1
        assert lib.npf_masked_attn_bwd_nq(p, p, p, p, p, p, p, p, 1, 4, 4, d, 1.0, p, p, p, None) == -1
    assert lib.npf_masked_attn_fwd_nq(p, p, p, p, None, 1, 4, 4, 32, 1.0, p, None, None) == -1
    assert lib.npf_masked_attn_bwd_nq(p, p, p, p, None, p, p, p, 1, 4, 4, 32, 1.0, p, p, p, None) == -1
    assert lib.npf_masked_attn_fwd_nq(p, p, p, p, p, 1, 4, -1, 32, 1.0, p, None, None) == -1


def _xyt(B=2, C=6, T=5):
    return torch.zeros(B, C, 1), torch.zeros(B, C, 2), torch.zeros(B, T, 1), torch.zeros(B, T, 2)


@pytest.mark.parametrize("kind", ("CNP", "LNP", "AttnCNP", "AttnLNP"))
def test_n_trgt_argument_is_checked(kind):
    kw = dict(encoded_path="latent") if kind == "LNP" else {}
    m = _model(kind, 128, **kw)
    Xc, Yc, Xt, Yt = _xyt()
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="shape"):
            m(Xc, Yc, Xt, Yt, n_trgt=bad)
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int16), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="int32 or int64"):
            m(Xc, Yc, Xt, Yt, n_trgt=bad)
    with pytest.raises(ValueError, match="n_trgt"):
        m(Xc, Yc, Xt, Yt, n_trgt=[1, 2])
    with pytest.raises(ValueError, match="n_trgt.*device"):   # a host tensor: the counts are device data
        m(Xc, Yc, Xt, Yt, n_trgt=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_cntxt.*device"):  # (both given: the context counts are checked first, as before)
        m(Xc, Yc, Xt, Yt, n_cntxt=torch.zeros(2, dtype=torch.int32), n_trgt=torch.zeros(2, dtype=torch.int32))


def test_refusals_name_the_option(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="n_trgt.*bf16"):
        _model("AttnCNP", 128)(*_xyt(), n_trgt=n)
    with pytest.raises(NotImplementedError, match="n_trgt.*is_self_attn"):
        A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)(*_xyt(), n_trgt=n)


def test_self_attention_is_refused_and_query_counts_need_key_counts():
    import npf_gwwaveform_amd as A

    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="n_trgt.*is_self_attn"):
        A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)(*_xyt(), n_trgt=n)
    with pytest.raises(NotImplementedError, match="n_q_valid needs n_valid"):
        A.DotAttender(32, 32, 32).attend_pt(torch.zeros(1), torch.zeros(1), torch.zeros(1), 4, 4, n_q_valid=n)


def test_head_distribution_and_gauss_head_take_the_counts():
    import inspect

    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import functional as FN

    assert inspect.signature(A.HeadDistribution.__init__).parameters["n_trgt"].default is None
    assert inspect.signature(FN.gauss_head).parameters["n_valid"].default is None
    assert inspect.signature(FN.masked_attention).parameters["n_q_valid"].default is None
    for cls in (A.CNP, A.LNP, A.AttnCNP, A.AttnLNP):
        assert list(inspect.signature(A.NeuralProcessFamily.forward).parameters)[1:] == \
            ["X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt"], cls
    with pytest.raises(ValueError, match="device"):  # (counts are device data for the head as well)
        FN.gauss_head(torch.zeros(2, 4, 2), None, 1, False, n_valid=torch.zeros(2, dtype=torch.int32))


# ---- the split -----------------------------------------------------------------------------------------------------------------
class _NoSync:
    """Inside the block ``Tensor.item`` / ``.cpu`` / ``.tolist`` / ``int(tensor)`` raise: nothing may read a count on the host."""

    NAMES = ("item", "cpu", "tolist", "__int__", "__index__", "__bool__", "numpy")

    def __enter__(self):
        self.saved = {n: getattr(torch.Tensor, n) for n in self.NAMES}
        for n in self.NAMES:
            def boom(*a, _n=n, **k):
                raise AssertionError(f"host read of a tensor ({_n}) in a path that must stay on the device")
            setattr(torch.Tensor, n, boom)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(torch.Tensor, n, f)


class _HostSelect:
    """``CntxtTrgtGetter`` whose gather is ``torch.gather`` (the launch needs a device; the indices and counts are what is tested)."""

    @staticmethod
    def make(**kw):
        import npf_gwwaveform_amd as A

        class G(A.CntxtTrgtGetter):
            def select(self, X, y, indcs, validate=True):
                take = lambda t: torch.gather(t, 1, indcs.unsqueeze(-1).expand(-1, -1, t.shape[-1]))  # noqa: E731
                return take(X), take(y)

        return G(**kw)


def test_targets_getter_per_task_returns_padded_targets_and_counts():
    import npf_gwwaveform_amd as A

    torch.manual_seed(0)
    B, N = 16, 60
    X, Y = torch.rand(B, N, 1) + 1.0, torch.rand(B, N, 2) + 1.0  # (no zero in the data: zero rows are padding)
    g = _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=5, b=20, is_per_task=True),
                         targets_getter=A.GetRandomIndcs(a=0, b=40, is_per_task=True))
    seen = set()
    for _ in range(5):
        with _NoSync():
            out = g(X, Y)
            batch = g.batch(X, Y)
        assert len(out) == 6 and set(batch) == {"X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt"}
        Xc, Yc, Xt, Yt, n_c, n_t = out
        assert Xt.shape == (B, 40, 1) and Yt.shape == (B, 40, 2) and Xc.shape == (B, 20, 1)
        assert n_t.shape == (B,) and n_t.dtype == torch.int64 and int(n_t.min()) >= 0 and int(n_t.max()) <= 40
        assert int(n_c.min()) >= 5 and int(n_c.max()) <= 20
        for b in range(B):
            k = int(n_t[b])
            assert (Xt[b, :k] != 0).all() and (Xt[b, k:] == 0).all() and (Yt[b, k:] == 0).all()
            assert len(set(Xt[b, :k, 0].tolist())) == k  # distinct points
        seen.update(n_t.tolist())
    assert len(seen) > 10  # one count per task
    # targets per task, contexts shared: the fifth value is None and the dict has no n_cntxt
    g2 = _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=8, b=8), targets_getter=A.GetRandomIndcs(a=0, b=40, is_per_task=True))
    out = g2(X, Y)
    assert len(out) == 6 and out[4] is None and out[5].shape == (B,)
    assert set(g2.batch(X, Y)) == {"X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_trgt"}
    # and the splits that existed keep their shape
    assert len(_HostSelect.make(contexts_getter=A.GetRandomIndcs(a=8, b=8))(X, Y)) == 4
    assert len(_HostSelect.make(contexts_getter=A.GetRandomIndcs(a=5, b=20, is_per_task=True))(X, Y)) == 5


def test_n_points_draws_among_the_real_points_only_and_never_syncs():
    import npf_gwwaveform_amd as A

    B, N = 12, 64
    gen = torch.Generator().manual_seed(3)
    n_points = torch.tensor([0, 1, 2, 5, 10, 16, 31, 32, 33, 63, 64, 64])
    X = torch.arange(N, dtype=torch.float32).view(1, N, 1).expand(B, N, 1) + 1.0  # (X holds index + 1: a row names its point)
    Y = torch.cat([X, -X], dim=-1)
    getter = A.GetRandomIndcs(a=0, b=32, is_per_task=True)
    for _ in range(10):
        with _NoSync():
            idx = getter(B, N, generator=gen, n_points=n_points)
        cnt = getter.last_counts
        assert idx.shape == (B, 32) and int(idx.min()) >= 0 and int(idx.max()) < N
        assert (cnt <= n_points).all() and (cnt >= 0).all()
        for b in range(B):
            row = idx[b, : int(cnt[b])].tolist()
            assert all(i < int(n_points[b]) for i in row), (b, row)
            assert len(set(row)) == len(row)
    g = _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=0, b=32, is_per_task=True), targets_getter=A.get_all_indcs)
    with _NoSync():
        batch = g.batch(X, Y, n_points=n_points.to(torch.int32))
    assert set(batch) == {"X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt"}
    assert torch.equal(batch["n_trgt"], n_points) and batch["X_trgt"].shape == (B, N, 1)
    assert (batch["n_cntxt"] <= n_points).all()
    for b in range(B):
        k, c = int(n_points[b]), int(batch["n_cntxt"][b])
        assert torch.equal(batch["X_trgt"][b, :k], X[b, :k]) and (batch["X_trgt"][b, k:] == 0).all() and (batch["Y_trgt"][b, k:] == 0).all()
        ctx = batch["X_cntxt"][b, :c, 0]
        assert ((ctx >= 1) & (ctx <= k)).all() and (batch["X_cntxt"][b, c:] == 0).all()
    # per-task targets with n_points: drawn among the real points too
    g3 = _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=0, b=32, is_per_task=True),
                          targets_getter=A.GetRandomIndcs(a=0, b=48, is_per_task=True))
    b3 = g3.batch(X, Y, n_points=n_points)
    assert (b3["n_trgt"] <= n_points).all() and b3["X_trgt"].shape == (B, 48, 1)
    for b in range(B):
        t = b3["X_trgt"][b, : int(b3["n_trgt"][b]), 0]
        assert ((t >= 1) & (t <= int(n_points[b]))).all()


def test_split_refusals():
    import npf_gwwaveform_amd as A

    X, Y = torch.rand(4, 20, 1), torch.rand(4, 20, 2)
    n = torch.tensor([3, 20, 0, 7])
    per = lambda **kw: A.GetRandomIndcs(a=0, b=8, is_per_task=True, **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="is_add_cntxts_to_trgts"):
        _HostSelect.make(contexts_getter=per(), is_add_cntxts_to_trgts=True)(X, Y, n_points=n)
    with pytest.raises(NotImplementedError, match="is_add_cntxts_to_trgts"):
        _HostSelect.make(contexts_getter=per(), targets_getter=per(), is_add_cntxts_to_trgts=True)(X, Y)
    with pytest.raises(NotImplementedError, match="n_points"):      # one shared context size cannot respect per-task lengths
        _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=4, b=4))(X, Y, n_points=n)
    with pytest.raises(NotImplementedError, match="n_points"):
        _HostSelect.make(contexts_getter=per(), targets_getter=A.GetRangeIndcs((0, 10)))(X, Y, n_points=n)
    with pytest.raises(NotImplementedError, match="n_points"):
        A.GetRandomIndcs(a=0, b=8)(4, 20, n_points=n)
    with pytest.raises(NotImplementedError, match="n_points"):
        A.GetRandomIndcs(a=0, b=8, is_per_task=True, is_batch_share=True)(4, 20, n_points=n)
    for bad in ([3, 20, 0, 7], torch.tensor([3.0, 20, 0, 7]), torch.tensor([3, 20, 0])):
        with pytest.raises(ValueError, match="n_points"):
            _HostSelect.make(contexts_getter=per())(X, Y, n_points=bad)
    # without the new arguments is_add_cntxts_to_trgts works as before
    out = _HostSelect.make(contexts_getter=A.GetRandomIndcs(a=4, b=4), is_add_cntxts_to_trgts=True)(X, Y)
    assert out[2].shape == (4, 20, 1)


def test_trainer_and_eval_pass_both_counts(monkeypatch):
    """``Trainer`` steps and ``eval_loglike`` hand ``batch["n_trgt"]`` to the model next to ``batch["n_cntxt"]``, and nothing when
    the batch has neither."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import train as TR
    from npf_gwwaveform_amd.evaluate import eval_loglike

    assert TR._counts_of({"X_cntxt": 1}) == {}
    assert TR._counts_of({"n_cntxt": 3, "n_trgt": None}) == {"n_cntxt": 3}
    assert TR._counts_of({"n_cntxt": 3, "n_trgt": 4, "X_trgt": 0}) == {"n_cntxt": 3, "n_trgt": 4}

    seen = []

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))

        def forward(self, Xc, Yc, Xt, Yt=None, **kw):
            seen.append(sorted(kw))
            return (Xt.sum() * self.w,)

    class Crit(torch.nn.Module):
        reduction = "mean"

        def forward(self, out, Y):
            return out[0].reshape(1) if self.reduction is None else out[0]

    Xc, Yc, Xt, Yt = _xyt()
    n = torch.ones(2, dtype=torch.int64)
    tr = TR.Trainer(M(), Crit(), world=1)
    tr.step(dict(X_cntxt=Xc, Y_cntxt=Yc, X_trgt=Xt, Y_trgt=Yt))
    tr.step(dict(X_cntxt=Xc, Y_cntxt=Yc, X_trgt=Xt, Y_trgt=Yt, n_trgt=n))
    tr.step(dict(X_cntxt=Xc, Y_cntxt=Yc, X_trgt=Xt, Y_trgt=Yt, n_cntxt=n, n_trgt=n))
    eval_loglike(M(), Crit(), [dict(X_cntxt=Xc, Y_cntxt=Yc, X_trgt=Xt, Y_trgt=Yt, n_trgt=n)])
    assert seen == [[], ["n_trgt"], ["n_cntxt", "n_trgt"], ["n_trgt"]]
    assert A.NeuralProcessFamily.forward.__doc__ and "n_trgt" in A.NeuralProcessFamily.forward.__doc__
