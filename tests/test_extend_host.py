"""Host side of growing contexts (CPU, no kernel launched): the C ABI of ``npf_append_points``, the argument checks of the library
entry, of ``functional.append_points`` and of ``condition_with_capacity`` / ``Conditioned.extend`` / ``Conditioned.rollout`` that need
no device, and the host-side bound of the rows offered."""
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


def test_append_points_is_declared_exported_and_typed():
    from npf_gwwaveform_amd import _lib as L

    name = "npf_append_points"
    header = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/npf_hip.h"
    lib = C.CDLL(L.lib_path())
    assert hasattr(lib, name), f"{name} is not exported"
    res, args = L.SIGNATURES[name]
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert decl == ["const npf_append_pair_t *pairs", "int32_t n_pairs", "int32_t *n_valid", "const int32_t *n_new", "int32_t n_tasks",
                    "int32_t n_rows", "int32_t capacity", "void *stream"]
    assert res is C.c_int and len(args) == len(decl)
    assert args[0] is C.POINTER(L.NpfAppendPair) or args[0]._type_ is L.NpfAppendPair
    for a, t in zip(decl[1:], args[1:]):
        assert t is (C.c_void_p if "*" in a else C.c_int32), (a, t)
    # the pair as the header lays it out: two pointers, the feature count, one reserved word
    s = re.search(r"typedef struct npf_append_pair \{(.*?)\} npf_append_pair_t;", header, flags=re.S)
    fields = [" ".join(f.split()) for f in s.group(1).split(";") if f.strip()]
    assert fields == ["const float *src", "float *dst", "int32_t F", "int32_t reserved"]
    assert [f[0] for f in L.NpfAppendPair._fields_] == ["src", "dst", "F", "reserved"] and C.sizeof(L.NpfAppendPair) == 24
    assert int(re.search(r"#define NPF_APPEND_MAX_PAIRS (\d+)", header).group(1)) == L.NPF_APPEND_MAX_PAIRS == 3
    lib.npf_version.restype = C.c_int
    assert lib.npf_version() == 2  # (a new export, the old ones unchanged: the ABI version stays)


def test_append_points_refuses_bad_arguments_without_a_device():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def call(pairs=((p, p, 32),), n_pairs=None, n_valid=p, n_new=None, n_tasks=1, n_rows=4, capacity=8):
        arr = (L.NpfAppendPair * max(len(pairs), 1))()
        for i, (src, dst, F) in enumerate(pairs):
            arr[i].src, arr[i].dst, arr[i].F = src, dst, F
        return lib.npf_append_points(arr, len(pairs) if n_pairs is None else n_pairs, n_valid, n_new, n_tasks, n_rows, capacity, None)

    for bad in (dict(n_pairs=0), dict(n_pairs=4), dict(n_valid=None), dict(n_tasks=-1), dict(n_tasks=65536), dict(n_rows=-1),
                dict(capacity=0), dict(pairs=((None, p, 32),)), dict(pairs=((p, None, 32),)), dict(pairs=((p, p, 0),)),
                dict(pairs=((p, p, 20),)), dict(pairs=((p + 4, p, 32),)), dict(pairs=((p, p + 8, 32),)),
                dict(pairs=((p, p, 32), (p, p, 33)))):
        assert call(**bad) == -1, bad
    assert lib.npf_append_points(None, 1, p, None, 1, 4, 8, None) == -1
    # nothing to do is not an error (and nothing is launched): no tasks, no rows
    assert call(n_tasks=0) == 0 and call(n_rows=0) == 0


def test_wrapper_checks_need_no_device():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    assert list(inspect.signature(FN.append_points).parameters) == ["pairs", "n_valid", "n_new", "n_tasks", "n_rows", "capacity"]
    src, dst = torch.zeros(pt_shape(2, 5, 20)), torch.zeros(pt_shape(2, 70, 20))
    c = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="pairs"):
        FN.append_points([], c, None, 2, 5, 70)
    with pytest.raises(ValueError, match="pairs"):
        FN.append_points([(src, dst, 20)] * 4, c, None, 2, 5, 70)
    with pytest.raises(ValueError, match="capacity"):
        FN.append_points([(src, dst, 20)], c, None, 2, 5, 0)
    with pytest.raises(ValueError, match="n_valid.*int32"):
        FN.append_points([(src, dst, 20)], c.long(), None, 2, 5, 70)
    with pytest.raises(ValueError, match="n_valid.*device"):
        FN.append_points([(src, dst, 20)], c, None, 2, 5, 70)


@pytest.mark.parametrize("kind", KINDS)
def test_models_have_the_growing_context_interface(kind):
    import npf_gwwaveform_amd as A

    cls = getattr(A, kind)
    assert list(inspect.signature(cls.condition).parameters)[1:] == ["X_cntxt", "Y_cntxt", "n_cntxt", "n_z_samples"]  # (unchanged)
    assert list(inspect.signature(cls.condition_with_capacity).parameters)[1:] == ["X_cntxt", "Y_cntxt", "capacity", "n_cntxt",
                                                                                   "n_z_samples"]
    assert list(inspect.signature(A.Conditioned.extend).parameters)[1:] == ["X_new", "Y_new", "n_new"]
    assert list(inspect.signature(A.Conditioned.rollout).parameters)[1:] == ["X_trgt", "eps", "chunk"]
    assert inspect.signature(A.Conditioned.rollout).parameters["chunk"].default == 1
    post = A.Conditioned(_build(kind), None, None, None, None, None, 2, 6, False)  # (as ``condition`` makes it)
    assert post.capacity is None and post.eps is None and post.n_rows_bound == 6
    assert "extended" in A.Conditioned.rollout.__doc__  # the docstring says what is left behind


def _xy(Bn=2, N=4, dx=1, dy=2):
    return torch.zeros(Bn, N, dx), torch.zeros(Bn, N, dy)


@pytest.mark.parametrize("kind", KINDS)
def test_argument_checks_and_the_row_bound(kind):
    import npf_gwwaveform_amd as A

    m = _build(kind).eval()
    X, Y = _xy(N=6)
    frozen = A.Conditioned(m, None, None, None, None, None, 2, 6, False)
    with pytest.raises(ValueError, match="capacity"):
        frozen.extend(*_xy())
    with pytest.raises(ValueError, match="capacity"):
        frozen.rollout(X)
    for cap in (5, 0, -1):
        with pytest.raises(ValueError, match="capacity"):
            m.condition_with_capacity(X, Y, cap)
    with pytest.raises(ValueError, match="capacity"):
        m.condition_with_capacity(X[:, :0], Y[:, :0], 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (a valid capacity: on to the tensors)
        m.condition_with_capacity(X, Y, 6)
    if kind in ("LNP", "AttnLNP"):
        with pytest.raises(ValueError, match="n_z_samples"):
            m.condition_with_capacity(X, Y, 8, n_z_samples=0)

    post = A.Conditioned(m, None, None, None, None, torch.zeros(2, dtype=torch.int32), 2, 6, False, capacity=10)
    assert post.n_rows_bound == 6
    for bad_x, bad_y, what in ((torch.zeros(3, 4, 1), torch.zeros(3, 4, 2), "X_new"), (torch.zeros(2, 4, 2), torch.zeros(2, 4, 2), "X_new"),
                               (torch.zeros(2, 4), torch.zeros(2, 4, 2), "X_new"), (torch.zeros(2, 4, 1), torch.zeros(2, 4, 1), "Y_new"),
                               (torch.zeros(2, 4, 1), torch.zeros(2, 3, 2), "Y_new")):
        with pytest.raises(ValueError, match=what):
            post.extend(bad_x, bad_y)
    with pytest.raises(ValueError, match="exceed capacity=10"):  # 6 + 5 > 10
        post.extend(*_xy(N=5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # 6 + 4 <= 10: on to the tensors
        post.extend(*_xy(N=4))
    assert post.n_rows_bound == 6  # (a refused call reserves nothing)
    assert post.extend(*_xy(N=0)) is post and post.n_rows_bound == 6
    post.n_rows_bound = 10  # full: by the bound alone, whatever the device counts say
    with pytest.raises(ValueError, match="exceed capacity=10"):
        post.extend(*_xy(N=1))
    post.n_rows_bound = 6
    with pytest.raises(ValueError, match="exceed capacity=10"):  # rollout needs the bound + T rows
        post.rollout(torch.zeros(2, 5, 1))
    with pytest.raises(ValueError, match="X_trgt"):
        post.rollout(torch.zeros(3, 4, 1))
    with pytest.raises(ValueError, match="eps"):
        post.rollout(torch.zeros(2, 4, 1), eps=torch.zeros(2, 3, 2))
    with pytest.raises(ValueError, match="chunk"):
        post.rollout(torch.zeros(2, 4, 1), chunk=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post.rollout(torch.zeros(2, 4, 1))
    post.z_samples = torch.zeros(3, 2, 1, 128)
    with pytest.raises(ValueError, match="n_z_samples=1"):
        post.rollout(torch.zeros(2, 4, 1))


def test_capacity_is_refused_where_counts_are(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    X, Y = _xy(N=6)
    with pytest.raises(NotImplementedError, match="capacity.*bf16"):
        _model("AttnCNP", 128).condition_with_capacity(X, Y, 8)
    sa = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)
    with pytest.raises(NotImplementedError, match="capacity.*is_self_attn"):
        sa.condition_with_capacity(X, Y, 8)
