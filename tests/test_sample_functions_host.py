"""Host side of ``Conditioned.sample_functions`` (CPU, no kernel launched): the C ABI of ``npf_masked_attn_fwd_prefix`` and the
argument checks of the library entry and of ``functional.masked_attention_prefix`` that need no device, the argument checks of
``sample_functions``, the task order of the S x B (x heads) tasks, the rounding of the tail capacity and the pooled-mean
combination of CNP / LNP against numpy."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("CNP", "LNP", "AttnCNP", "AttnLNP")
NAME = "npf_masked_attn_fwd_prefix"


def _build(kind, r=128):
    return _model(kind, r, **(dict(encoded_path="latent") if kind == "LNP" else {}))


def test_prefix_export_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert m, f"{NAME} is not declared in include/npf_hip.h"
    lib = C.CDLL(L.lib_path())
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    res, args = L.SIGNATURES[NAME]
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert decl == ["const float *q", "const float *k_pre", "const float *v_pre", "const int32_t *n_prefix", "const float *k_tail",
                    "const float *v_tail", "const int32_t *n_tail", "const int32_t *n_q_valid", "int32_t n_tasks",
                    "int32_t n_prefix_tasks", "int32_t c_pad", "int32_t m_tail", "int32_t n_queries", "int32_t d", "float scale",
                    "float *out", "void *stream"]
    assert res is C.c_int and len(args) == len(decl)
    for a, t in zip(decl, args):
        assert t is (C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int32), (a, t)
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (a new export, the old ones unchanged: the ABI version stays)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_prefix_export_refuses_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def call(q=p, k_pre=p, v_pre=p, n_prefix=p, k_tail=p, v_tail=p, n_tail=p, n_q=None, n_tasks=6, n_pre=3, c_pad=8, m_tail=8, T=4,
             d=32, out=p):
        return lib.npf_masked_attn_fwd_prefix(q, k_pre, v_pre, n_prefix, k_tail, v_tail, n_tail, n_q, n_tasks, n_pre, c_pad, m_tail, T, d,
                                              1.0, out, None)

    for bad in (dict(d=0), dict(d=18), dict(d=260), dict(n_tasks=-1), dict(n_pre=0), dict(n_pre=-3), dict(n_tasks=7), dict(c_pad=-1),
                dict(m_tail=-1), dict(T=-1), dict(q=None), dict(out=None), dict(n_prefix=None), dict(n_tail=None), dict(k_pre=None),
                dict(v_tail=None), dict(q=p + 4), dict(k_tail=p + 8), dict(out=p + 4)):
        assert call(**bad) == -1, bad
    # nothing to do is not an error (and nothing is launched); an empty segment needs no tensors
    assert call(n_tasks=0) == 0 and call(T=0) == 0
    assert call(T=0, c_pad=0, k_pre=None, v_pre=None) == 0 and call(T=0, m_tail=0, k_tail=None, v_tail=None) == 0


def test_wrapper_checks_need_no_device():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    assert list(inspect.signature(FN.masked_attention_prefix).parameters) == [
        "q_pt", "k_pre", "v_pre", "n_prefix", "k_tail", "v_tail", "n_tail", "n_tasks", "n_prefix_tasks", "c_pad", "m_tail", "n_queries",
        "d", "scale", "n_q_valid"]
    z = lambda n, r, d=32: torch.zeros(pt_shape(n, r, d))  # noqa: E731
    ops = lambda: [z(6, 5), z(3, 70), z(3, 70), z(6, 40), z(6, 40)]  # noqa: E731
    c3, c6 = torch.zeros(3, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)  # (on the host: refused last)

    def call(o, n=6, p=3, d=32, n_pre=c3, n_tail=c6):
        return FN.masked_attention_prefix(o[0], o[1], o[2], n_pre, o[3], o[4], n_tail, n, p, 70, 40, 5, d, 1.0)

    for d in (18, 0, 260):
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            call(ops(), d=d)
    for n, p in ((7, 3), (6, 0), (6, 4)):
        with pytest.raises(ValueError, match="multiple of n_prefix_tasks"):
            call(ops(), n=n, p=p)
    for i in range(5):
        o = ops()
        o[i].requires_grad_(True)
        with pytest.raises(RuntimeError, match="inference only"):
            call(o)
        with torch.no_grad(), pytest.raises(RuntimeError, match="inference only"):
            call(o)
    o = ops()
    o[3] = z(6, 70)
    with pytest.raises(ValueError, match="k_tail"):
        call(o)
    with pytest.raises(ValueError, match="n_prefix.*device"):
        call(ops())


def sample_task(s, b, B):
    """Task index of sample ``s`` of task ``b`` in a sample-major batch of S x B tasks."""
    return s * B + b


def sample_head_task(s, h, b, B, H):
    """The same with heads as extra tasks: sample-major, then head, then task."""
    return s * (B * H) + h * B + b


def prefix_task(j, B, H=1):
    """The prefix task that task ``j`` reads: what the kernel computes, ``j % n_prefix_tasks``."""
    return j % (B * H)


def test_task_order():
    """Sample-major: j = s B + b reads prefix j % B; with heads as tasks j = s (B H) + h B + b reads prefix h B + b, the index
    ``npf_split_heads`` gives head h of task b -- and the two device permutations between that order and the head-major one of
    ``npf_split_heads`` over S x B tasks are inverses."""
    from npf_gwwaveform_amd import architectures as AR

    S, B, H = 3, 2, 4
    seen = set()
    for s in range(S):
        for b in range(B):
            j = sample_task(s, b, B)
            assert j == s * B + b and prefix_task(j, B) == b
            for h in range(H):
                jh = sample_head_task(s, h, b, B, H)
                assert jh == s * B * H + h * B + b and prefix_task(jh, B, H) == h * B + b
                seen.add(jh)
    assert seen == set(range(S * B * H))
    # head-major (what split_heads makes of the S x B tasks: task h (S B) + s B + b) -> sample-major and back
    head_major = torch.tensor([[h, s, b] for h in range(H) for s in range(S) for b in range(B)])
    sm = AR._sample_major(head_major, S, H, B)
    for s in range(S):
        for h in range(H):
            for b in range(B):
                assert sm[sample_head_task(s, h, b, B, H)].tolist() == [h, s, b]
    assert torch.equal(AR._head_major(sm, S, H, B), head_major)


def test_tail_capacity_is_whole_tiles():
    from npf_gwwaveform_amd.neuralproc import tail_capacity

    assert [tail_capacity(T) for T in (1, 31, 32, 33, 64, 65)] == [32, 32, 32, 64, 64, 96]


def test_pooled_mean_of_two_against_numpy():
    from npf_gwwaveform_amd.neuralproc import pooled_mean_of_two

    rng = np.random.default_rng(3)
    n_p, n_t = np.array([0, 0, 5, 12, 7, 1]), np.array([0, 4, 0, 6, 32, 1])
    rows_p = [rng.standard_normal((n, 8)) for n in n_p]
    rows_t = [rng.standard_normal((n, 8)) for n in n_t]
    mean = lambda rows: np.stack([r.mean(0) if len(r) else np.zeros(8) for r in rows])  # noqa: E731
    want = np.stack([np.concatenate([a, b]).mean(0) if len(a) + len(b) else np.zeros(8) for a, b in zip(rows_p, rows_t)])
    got = pooled_mean_of_two(torch.from_numpy(mean(rows_p)), torch.from_numpy(n_p).int(), torch.from_numpy(mean(rows_t)),
                             torch.from_numpy(n_t).int())
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-15)
    assert not got[0].any()  # total count 0: the zero representation


@pytest.mark.parametrize("kind", KINDS)
def test_argument_checks(kind):
    import npf_gwwaveform_amd as A

    assert list(inspect.signature(A.Conditioned.sample_functions).parameters)[1:] == ["X_trgt", "n_samples", "eps", "chunk"]
    assert inspect.signature(A.Conditioned.sample_functions).parameters["chunk"].default == 1
    assert list(inspect.signature(A.Conditioned.rollout).parameters)[1:] == ["X_trgt", "eps", "chunk"]  # (unchanged)
    m = _build(kind).eval()
    post = A.Conditioned(m, None, None, None, None, torch.zeros(2, dtype=torch.int32), 2, 6, False, capacity=10)
    X = torch.zeros(2, 4, 1)
    for bad in (torch.zeros(3, 4, 1), torch.zeros(2, 4, 2), torch.zeros(2, 4)):
        with pytest.raises(ValueError, match="X_trgt"):
            post.sample_functions(bad, 3)
    with pytest.raises(ValueError, match="no target points"):
        post.sample_functions(X[:, :0], 3)
    for S in (0, -1):
        with pytest.raises(ValueError, match="n_samples"):
            post.sample_functions(X, S)
    for bad in (torch.zeros(2, 4, 2), torch.zeros(3, 2, 3, 2), torch.zeros(2, 2, 4, 2), torch.zeros(3, 2, 4, 1)):
        with pytest.raises(ValueError, match="eps"):
            post.sample_functions(X, 3, eps=bad)
    with pytest.raises(ValueError, match="chunk"):
        post.sample_functions(X, 3, chunk=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (valid arguments: on to the tensors)
        post.sample_functions(X, 3, eps=torch.zeros(3, 2, 4, 2))
    # sample_functions needs no free rows in the state: the draws live in its own tails
    post.n_rows_bound = 10
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post.sample_functions(X, 3)
    post.z_samples = torch.zeros(3, 2, 1, 128)
    with pytest.raises(ValueError, match="n_z_samples=1"):
        post.sample_functions(X, 3)
    # a state stored for the fused target side (no counts, no capacity) is refused; with counts the same flag is not
    fused = A.Conditioned(m, None, None, None, None, None, 2, 6, True)
    with pytest.raises(ValueError, match="n_cntxt.*capacity"):
        fused.sample_functions(X, 3)
    counted = A.Conditioned(m, None, None, None, None, torch.zeros(2, dtype=torch.int32), 2, 6, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        counted.sample_functions(X, 3)


def test_refused_where_counts_are(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    X = torch.zeros(2, 4, 1)
    post = A.Conditioned(_model("AttnCNP", 128), None, None, None, None, torch.zeros(2, dtype=torch.int32), 2, 6, False, capacity=10)
    with pytest.raises(NotImplementedError, match="sample_functions.*bf16"):
        post.sample_functions(X, 3)
    sa = A.Conditioned(A.AttnCNP(1, 2, r_dim=32, is_self_attn=True), None, None, None, None, None, 2, 6, False)
    with pytest.raises(NotImplementedError, match="sample_functions.*is_self_attn"):
        sa.sample_functions(X, 3)
