"""Host side of the padded-context feature (CPU, no kernel launched): the C ABI of the masked kernels, the per-task draw of
``GetRandomIndcs``, the argument checks of ``forward(..., n_cntxt=...)``, and that a call without ``n_cntxt`` consults the same
dispatch predicates as before."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from test_dispatch_rules import C_VALUES, T_VALUES, _model, _target_rule, bf16_mode  # noqa: F401  (read-only: the rule table)

MASKED = ("npf_masked_attn_fwd", "npf_masked_attn_bwd", "npf_masked_mean_fwd", "npf_masked_mean_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_symbols_are_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    lib = C.CDLL(L.lib_path())
    for name in MASKED:
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
    assert "float scale" in re.search(r"npf_masked_attn_fwd\s*\(([^;]*)\)", header).group(1)
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2


def test_masked_exports_refuse_bad_sizes_without_a_device():
    """Status -1 and nothing launched for a width that is not a multiple of 4 or above 256, and for negative counts of points
    (the checks come before any use of the device)."""
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    for d in (30, 260, 0):
        assert lib.npf_masked_attn_fwd(p, p, p, p, 1, 4, 4, d, 1.0, p, None, None) == -1
        assert lib.npf_masked_attn_bwd(p, p, p, p, p, p, p, 1, 4, 4, d, 1.0, p, p, p, None) == -1
    assert lib.npf_masked_attn_fwd(p, p, p, p, 1, -1, 4, 32, 1.0, p, None, None) == -1
    assert lib.npf_masked_attn_fwd(p, p, p, p, 1, 4, -1, 32, 1.0, p, None, None) == -1
    assert lib.npf_masked_mean_fwd(p, p, 1, -1, 32, p, None) == -1
    assert lib.npf_masked_mean_bwd(p, p, 1, 4, 30, p, 0, None) == -1


def test_per_task_counts_and_padded_indices():
    import npf_gwwaveform_amd as A

    gen = torch.Generator().manual_seed(5)
    getter = A.GetRandomIndcs(a=0, b=50, is_per_task=True)
    shapes, seen = set(), set()
    for _ in range(20):
        idx = getter(16, 128, generator=gen)
        n = getter.last_counts
        shapes.add(tuple(idx.shape))
        assert n.shape == (16,) and n.dtype == torch.int64 and int(n.min()) >= 0 and int(n.max()) <= 50
        assert int(idx.min()) >= 0 and int(idx.max()) < 128
        for row, k in zip(idx.tolist(), n.tolist()):
            assert len(set(row[:k])) == k
        seen.update(n.tolist())
    assert shapes == {(16, 50)}          # padded to the largest possible count, the same shape at every draw
    assert len(seen) > 20                # one count per task, not one per batch
    frac = A.GetRandomIndcs(a=0.25, b=0.5, is_per_task=True)
    assert frac(4, 40).shape == (4, 20) and int(frac.last_counts.min()) >= 10 and int(frac.last_counts.max()) <= 20
    one = A.GetRandomIndcs(a=0, b=0, is_per_task=True, is_ensure_one=True)
    assert one(3, 10).shape == (3, 1) and one.last_counts.tolist() == [1, 1, 1]
    with pytest.raises(NotImplementedError):
        A.GetRandomIndcs(is_per_task=True, is_beta_binomial=True)


def test_default_draw_is_unchanged():
    """is_per_task=False: the reference's behaviour -- the size from Python's ``random``, the same indices as before for a seed."""
    import npf_gwwaveform_amd as A

    def draw(getter):
        random.seed(7)
        np.random.seed(7)
        return getter(4, 30, generator=torch.Generator().manual_seed(11))

    a = draw(A.GetRandomIndcs(a=0.25, b=0.5))
    b = draw(A.GetRandomIndcs(a=0.25, b=0.5, is_per_task=False))
    # what the default path computes, written out: one size from random.randint, argsort of uniform noise
    random.seed(7)
    np.random.seed(7)
    np.random.uniform(size=1)
    n = random.randint(7, 15)
    want = torch.rand(4, 30, generator=torch.Generator().manual_seed(11)).argsort(dim=1)[:, :n]
    assert torch.equal(a, want) and torch.equal(b, want)
    state = random.getstate()
    A.GetRandomIndcs(a=0, b=10, is_per_task=True)(4, 30)
    assert random.getstate() == state    # the per-task draw leaves Python's generator alone


def _xyt(B=2, C=6, T=5):
    return torch.zeros(B, C, 1), torch.zeros(B, C, 2), torch.zeros(B, T, 1), torch.zeros(B, T, 2)


@pytest.mark.parametrize("kind", ("CNP", "LNP", "AttnCNP", "AttnLNP"))
def test_n_cntxt_argument_is_checked(kind):
    kw = dict(encoded_path="latent") if kind == "LNP" else {}
    m = _model(kind, 128, **kw)
    Xc, Yc, Xt, Yt = _xyt()
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="shape"):
            m(Xc, Yc, Xt, Yt, n_cntxt=bad)
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int16), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="int32 or int64"):
            m(Xc, Yc, Xt, Yt, n_cntxt=bad)
    with pytest.raises(ValueError, match="n_cntxt"):
        m(Xc, Yc, Xt, Yt, n_cntxt=[1, 2])
    with pytest.raises(ValueError, match="device"):   # a host tensor: the counts are device data
        m(Xc, Yc, Xt, Yt, n_cntxt=torch.zeros(2, dtype=torch.int32))


def test_refused_combinations_name_the_option(bf16_mode):  # noqa: F811
    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="bf16"):
        _model("AttnCNP", 128)(*_xyt(), n_cntxt=n)


def test_self_attention_and_4d_keys_are_refused():
    import npf_gwwaveform_amd as A

    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="is_self_attn"):
        A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)(*_xyt(), n_cntxt=n)
    with pytest.raises(NotImplementedError, match="4-D"):
        A.DotAttender(32, 32, 32)(torch.zeros(2, 5, 6, 32), torch.zeros(2, 5, 32), torch.zeros(2, 6, 32), n_valid=n)


@pytest.mark.parametrize("r", (128, 256))
def test_forward_without_n_cntxt_consults_the_same_predicates(r, monkeypatch):
    """A CPU forward without ``n_cntxt`` asks ``_fused_target_side`` / ``_fused_context_side`` with (C, T) exactly as before (it
    then stops at the device check: there is no CPU path), and the predicates still give the table of
    tests/test_dispatch_rules.py; with ``n_cntxt`` the fused target side is never asked."""
    m = _model("AttnCNP", r)
    asked = []
    real_t, real_c = m._fused_target_side, m._fused_context_side
    monkeypatch.setattr(m, "_fused_target_side", lambda C, T: asked.append(("t", C, T)) or real_t(C, T))
    monkeypatch.setattr(m, "_fused_context_side", lambda C: asked.append(("c", C)) or real_c(C))
    monkeypatch.setattr(m, "_validate_inputs", lambda *a: None)
    for C in C_VALUES:
        for T in T_VALUES:
            assert real_t(C, T) == _target_rule(r, C, T), (r, C, T)
            del asked[:]
            with pytest.raises(RuntimeError):  # (the first launch refuses host tensors)
                m(*_xyt(2, C, T))
            assert asked[:2] == [("t", C, T), ("c", C)], asked
