"""Leave-one-out predictions on the GPU: ``npf_masked_attn_fwd_loo`` and ``npf_loo_mean`` against float64, and ``model.loo`` /
``Conditioned.loo`` against the oracle run in float64 once per (task, left-out point) on the context cut to the OTHER points.

Gates.  Attention kernel: the expression ``tests/test_hip_masked.py`` applies to ``npf_masked_attn_fwd`` (``assert_gated`` with 1e-5),
taken per task.  ``loo_mean``: 1e-6 of max|ref| per task (an fp32 sum over at most 40 rows).  Models: the project's fp32 gate on loc
and scale, max|d| <= 1e-5 max|ref|, the loss (minus the mean over the tasks of the summed log density) to rtol 2e-5; the per-point
log densities to 2e-5 of their largest (a relative error of 1e-5 in sigma moves the z^2 / 2 term by 2e-5 of itself).  Model inputs: the first seed for which no ReLU pre-activation of the
float64 reference lies within 2e-7 of zero (the ``_well_posed_inputs`` rule of tests/test_hip_masked.py; it reads the reference
alone)."""
import math

import numpy as np
import pytest
import torch

import specs
from helpers import assert_close, build_model, launch_witness
from oracle import npf_oracle as O
from test_hip_dispatch import _c
from test_hip_masked_edges import _poison_feature_padding, _poison_rows
from test_hip_mha import assert_gated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RELU_TIE = 2e-7


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


# ---- 1. the attention kernel against float64 -------------------------------------------------------------------------------
K_B, K_CPAD, K_COUNTS = 4, 80, (80, 33, 1, 0)


def _loo_attention(Q, K, V, counts, scale, dtype):
    """[B, C_pad, d]: softmax over the task's valid keys without the query's own row; zeros beyond the count and without a key."""
    out = torch.zeros_like(Q, dtype=dtype)
    for b, n in enumerate(counts):
        if n < 2:
            continue
        q, k, v = (x[b, :n].to(dtype) for x in (Q, K, V))
        S = q @ k.T * scale
        S.fill_diagonal_(-math.inf)
        out[b, :n] = torch.softmax(S, dim=-1) @ v
    return out


def _loo_launch(q_pt, k_pt, v_pt, counts, C_pad, d, q_counts="same"):
    from npf_gwwaveform_amd import functional as FN

    n = _i32(counts)
    with launch_witness() as w:
        o = FN.masked_attention_loo(q_pt, k_pt, v_pt, n, len(counts), C_pad, C_pad, d, 1.0 / math.sqrt(d),
                                    n_q_valid=n if q_counts == "same" else q_counts)
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_loo"] == 1 and w["npf_masked_attn_fwd"] == 0 and w["npf_masked_attn_fwd_nq"] == 0, w
    return o


@pytest.mark.parametrize("d", (4, 24, 64, 100, 256))
def test_loo_attention_matches_float64(d):
    """Counts across the 16- / 32-key block edges and the 16- / 64-query edges, a one-key and a no-key task; NaN in every padding row
    and padding feature of the operands; exact zeros where no key is left; a second launch gives the same bits."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(500 + d)
    Q, K, V = (torch.randn(K_B, K_CPAD, d, generator=g) * a for a in (1.5, 1.5, 1.0))  # (as tests/test_hip_masked.py)
    scale = 1.0 / math.sqrt(d)
    ops = [_poison_feature_padding(_poison_rows(_pt(x), K_COUNTS), d) for x in (Q, K, V)]
    assert all(x.isnan().any() for x in ops)
    o_pt = _loo_launch(*ops, K_COUNTS, K_CPAD, d)
    out = FN.unpack_pt(o_pt, K_CPAD, d)
    r64, r32 = (_loo_attention(Q, K, V, K_COUNTS, scale, dt) for dt in (torch.float64, torch.float32))
    for b, n in enumerate(K_COUNTS):
        err = float((out[b].cpu().double() - r64[b]).abs().max())
        print(f"d={d} task {b} (n={n}): max|d|={err:.3e} max|ref|={float(r64[b].abs().max()):.3e}")
        assert_gated(out[b], r64[b], r32[b], 1e-5, f"d={d} task {b} (n={n})")
        assert (out[b, n:] == 0).all(), f"task {b}: rows beyond the count {n}"
        if n < 2:
            assert (out[b] == 0).all(), f"task {b}: no key is left for a task of {n} points"
    assert torch.isfinite(o_pt).all(), "NaN from the padding of the operands reached the result"
    assert torch.equal(_loo_launch(*ops, K_COUNTS, K_CPAD, d), o_pt), "a second launch gave other bits"
    # without a query count every row is a query: the rows below the key count keep their bits
    clean = [_pt(x) for x in (Q, K, V)]
    o_all = FN.unpack_pt(_loo_launch(*clean, K_COUNTS, K_CPAD, d, q_counts=None), K_CPAD, d)
    for b, n in enumerate(K_COUNTS):
        assert torch.equal(o_all[b, :n], out[b, :n]), f"task {b}: rows below the count without n_q_valid"


# ---- 2. the exclusion is real -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,i", ((64, 50, 37), (256, 50, 37), (32, 33, 32), (128, 17, 0)))
def test_an_infinite_own_value_does_not_reach_its_query(d, n, i):
    """One task whose value row ``i`` is Inf: query ``i`` stays finite and matches float64 (the others meet the Inf and are not
    looked at).  (33, 32): the query's own row is the only valid key of its block."""
    from npf_gwwaveform_amd import functional as FN

    C_pad = 64
    g = torch.Generator().manual_seed(d + n + i)
    Q, K, V = (torch.randn(1, C_pad, d, generator=g) for _ in range(3))
    r64, r32 = (_loo_attention(Q, K, V, (n,), 1.0 / math.sqrt(d), dt) for dt in (torch.float64, torch.float32))
    Vbad = V.clone()
    Vbad[0, i] = math.inf
    out = FN.unpack_pt(_loo_launch(_pt(Q), _pt(K), _pt(Vbad), (n,), C_pad, d), C_pad, d)
    assert torch.isfinite(out[0, i]).all(), "the query's own value row reached its output"
    assert_gated(out[0, i], r64[0, i], r32[0, i], 1e-5, f"d={d} n={n} query {i}")


@pytest.mark.parametrize("d,n", ((32, 33), (256, 40)))
def test_identical_keys_give_the_mean_of_the_other_values(d, n):
    """Every score ties, so query ``i`` gets the plain mean of the other n - 1 values."""
    from npf_gwwaveform_amd import functional as FN

    C_pad = 40
    g = torch.Generator().manual_seed(7 * d + n)
    Q, V = torch.randn(1, C_pad, d, generator=g), torch.randn(1, C_pad, d, generator=g)
    K = torch.randn(1, 1, d, generator=g).expand(1, C_pad, d).contiguous()
    out = FN.unpack_pt(_loo_launch(_pt(Q), _pt(K), _pt(V), (n,), C_pad, d), C_pad, d)
    v = V[0, :n].double()
    want = (v.sum(0, keepdim=True) - v) / (n - 1)
    assert_close(out[0, :n], want, tol=1e-5, what="identical keys")
    assert (out[0, n:] == 0).all()


# ---- 3. loo_mean against float64 ----------------------------------------------------------------------------------------------
M_COUNTS, M_PTS = (40, 33, 2, 1, 0), 40


@pytest.mark.parametrize("r", (36, 128, 256))
def test_loo_mean_matches_float64(r):
    from npf_gwwaveform_amd import functional as FN

    B = len(M_COUNTS)
    R = torch.randn(B, M_PTS, r, generator=torch.Generator().manual_seed(r))
    R_pt = _poison_rows(_pt(R), M_COUNTS)  # (rows and tiles beyond the count are not read)
    with launch_witness() as w:
        o_pt = FN.loo_mean(R_pt, _i32(M_COUNTS), B, M_PTS, r)
        torch.cuda.synchronize()
    assert w["npf_loo_mean"] == 1 and w["npf_masked_mean_fwd"] == 0, w
    out = FN.unpack_pt(o_pt, M_PTS, r)
    assert not o_pt.isnan().any()
    for b, n in enumerate(M_COUNTS):
        ref = torch.zeros(M_PTS, r, dtype=torch.float64)
        if n > 1:
            v = R[b, :n].double()
            ref[:n] = (v.sum(0, keepdim=True) - v) / (n - 1)
            err, top = float((out[b].cpu().double() - ref).abs().max()), float(ref.abs().max())
            print(f"r={r} task {b} (n={n}): max|d|={err:.3e} max|ref|={top:.3e}")
            assert err <= 1e-6 * top, f"r={r} task {b}: max|d|={err:.3e} > 1e-6 * {top:.3e}"
        else:
            assert (out[b] == 0).all(), f"task {b}: a task of {n} points has no other point"
        assert (out[b, n:] == 0).all(), f"task {b}: rows beyond the count {n}"
    assert torch.equal(FN.loo_mean(R_pt, _i32(M_COUNTS), B, M_PTS, r), o_pt)


# ---- 4. models against the oracle ---------------------------------------------------------------------------------------------
B, C_PAD, DY = 3, 40, 2
COUNTS = (40, 17, 1)
KW = dict(B=B, T=1)
CASES = {
    "cnp_r128": _c("CNP", 128, C_PAD, **KW),
    "attncnp_r64": _c("AttnCNP", 64, C_PAD, **KW),
    "attncnp_r128": _c("AttnCNP", 128, C_PAD, **KW),
    "attncnp_transformer_r128": _c("AttnCNP", 128, C_PAD, attention="transformer", **KW),
    "attncnp_r256": _c("AttnCNP", 256, C_PAD, **KW),
}
_CACHE = {}


def _oracle_loo(case, params64, X, Y, counts, margins=False):
    """float64 (loc, scale) [B, C, dy] (0 / 1 beyond the counts): for every task and valid ``i`` the oracle's forward on the context
    cut to the task's other points with ``x_i`` as the target.  ``margins``: -> the smallest |ReLU pre-activation| instead."""
    cfg = specs.cfg_of(case)
    Bn, C = X.shape[:2]
    loc, scale = torch.zeros(Bn, C, DY, dtype=torch.float64), torch.ones(Bn, C, DY, dtype=torch.float64)
    O.RELU_MARGINS = [] if margins else None
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the zero representations the oracle makes for an empty context follow the default)
    try:
        with torch.no_grad():
            for b, n in enumerate(counts):
                Xb, Yb = X[b:b + 1, :n].double(), Y[b:b + 1, :n].double()
                for i in range(n):
                    keep = [j for j in range(n) if j != i]
                    o = O.forward(cfg, params64, Xb[:, keep], Yb[:, keep], Xb[:, i:i + 1], None, eps=None, n_z=1, training=False)
                    loc[b, i], scale[b, i] = o["loc"][0, 0, 0], o["scale"][0, 0, 0]
        return min(O.RELU_MARGINS) if margins else (loc, scale)
    finally:
        O.RELU_MARGINS = None
        torch.set_default_dtype(default)


def _log_density(loc, scale, Y, counts):
    """float64 [B, C]: the diagonal Gaussian's log density of ``Y`` summed over the y-dims, 0 beyond the counts."""
    lp = (-0.5 * ((Y.double() - loc) / scale) ** 2 - scale.log() - 0.5 * math.log(2 * math.pi)).sum(-1)
    for b, n in enumerate(counts):
        lp[b, n:] = 0
    return lp


def _setup(name):
    """Model, well-posed inputs (C_PAD context rows and 8 more to extend by) and the float64 references -- computed once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    case = CASES[name]
    wide = dict(case, C=C_PAD + 8)
    params = specs.make_params(case, seed=11)
    params64 = {k: v.double() for k, v in params.items()}
    for seed in range(4321, 4321 + 200):
        inp = specs.make_inputs(wide, seed=seed)
        X, Y = inp["X_cntxt"], inp["Y_cntxt"]
        if min(_oracle_loo(case, params64, X[:, :C_PAD], Y[:, :C_PAD], COUNTS, margins=True),
               _oracle_loo(case, params64, X, Y, (C_PAD + 8,) * B, margins=True)) >= RELU_TIE:
            break
    else:
        raise AssertionError("no well-posed inputs in 200 seeds")
    model = build_model(case, DEV, params=params).eval()
    out = dict(case=case, model=model, seed=seed, X=X.to(DEV), Y=Y.to(DEV), Xc=X[:, :C_PAD].contiguous().to(DEV),
               Yc=Y[:, :C_PAD].contiguous().to(DEV), ref=_oracle_loo(case, params64, X[:, :C_PAD], Y[:, :C_PAD], COUNTS),
               ref_wide=_oracle_loo(case, params64, X, Y, (C_PAD + 8,) * B))
    _CACHE[name] = out
    return out


def _compare(tag, p, ref, Y, counts):
    loc, scale = p.base_dist.loc, p.base_dist.scale
    rows = ref[0].shape[1]
    assert tuple(p.batch_shape) == (1, B, rows) and tuple(p.event_shape) == (DY,) and loc.shape == (1, B, rows, DY)
    for what, got, want in (("loc", loc[0], ref[0]), ("scale", scale[0], ref[1])):
        err = float((got.cpu().double() - want).abs().max())
        print(f"{tag} {what}: max|d|={err:.3e} max|ref|={float(want.abs().max()):.3e}")
        assert_close(got, want, what=f"{tag} {what}")
    rel = float(((scale[0].cpu().double() - ref[1]) / ref[1]).abs().max())
    assert rel <= 1e-5, f"{tag}: sigma differs by {rel:.3e} relative"
    for b, n in enumerate(counts):
        assert (loc[0, b, n:] == 0).all() and (scale[0, b, n:] == 1).all(), f"{tag} task {b}: rows beyond the count {n}"
    # the per-point LOO log density, and the loss the project makes of it (minus the mean over the tasks of the sum over the points)
    lp = p.log_prob(Y.unsqueeze(0))[0]
    want = _log_density(ref[0], ref[1], Y.cpu(), counts)
    for b, n in enumerate(counts):
        lp[b, n:] = 0
    assert_close(lp, want, tol=2e-5, what=f"{tag} log density")
    np.testing.assert_allclose(-float(lp.double().sum(1).mean()), -float(want.sum(1).mean()), rtol=2e-5)
    slp = p.sum_log_prob(Y)  # (the loss-only launch reads the counts itself)
    np.testing.assert_allclose(-float(slp.double().mean()), -float(want.sum(1).mean()), rtol=2e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_loo_matches_the_oracle_on_the_cut_contexts(name):
    s = _setup(name)
    m, n = s["model"], _i32(COUNTS)
    attentive = s["case"]["kind"].startswith("Attn")
    with launch_witness() as w:
        p = m.loo(s["Xc"], s["Yc"], n_cntxt=n)
        p.base_dist
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_loo"] == int(attentive) and w["npf_loo_mean"] == int(not attentive), w
    assert w["npf_masked_attn_fwd"] == 0 and w["npf_masked_attn_fwd_nq"] == 0 and w["npf_masked_mean_fwd"] == 0, w
    _compare(f"{name} (input seed {s['seed']})", p, s["ref"], s["Yc"], COUNTS)
    q = p.summary((0.5,))  # (one Gaussian per point: its mean, standard deviation and median)
    assert_close(q.mean, p.base_dist.loc[0].cpu(), tol=1e-6, what="summary mean")
    assert_close(q.std, p.base_dist.scale[0].cpu(), tol=1e-6, what="summary std")
    assert_close(q.quantiles[0], p.base_dist.loc[0].cpu(), tol=1e-6, what="summary median")
    # model.loo equals post.loo() bit for bit on a capacity state
    post = m.condition_with_capacity(s["Xc"], s["Yc"], C_PAD, n_cntxt=n)
    d = post.loo().base_dist
    assert torch.equal(d.loc, p.base_dist.loc) and torch.equal(d.scale, p.base_dist.scale)
    # without counts every task holds all C rows
    full = m.loo(s["Xc"], s["Yc"]).base_dist
    same = m.loo(s["Xc"], s["Yc"], n_cntxt=_i32((C_PAD,) * B)).base_dist
    assert torch.equal(full.loc, same.loc) and torch.equal(full.scale, same.scale)


@pytest.mark.parametrize("name", list(CASES))
def test_after_extend_the_new_points_are_included(name):
    s = _setup(name)
    m = s["model"]
    post = m.condition_with_capacity(s["Xc"], s["Yc"], C_PAD + 8)
    post.extend(s["X"][:, C_PAD:].contiguous(), s["Y"][:, C_PAD:].contiguous())
    p, direct = post.loo(), m.loo(s["X"], s["Y"])
    for what in ("loc", "scale"):
        assert_close(getattr(p.base_dist, what), getattr(direct.base_dist, what).cpu(), what=f"{name} {what}: extended state against model.loo")
    _compare(f"{name} extended", p, s["ref_wide"], s["Y"], (C_PAD + 8,) * B)


def _state_tensors(post):
    return dict(n_cntxt=post.n_cntxt, R_pts=post._R_pts.t, R=post._R if torch.is_tensor(post._R) else post._R.t, Xc=post._Xc_pt.t)


@pytest.mark.parametrize("name", ["cnp_r128", "attncnp_r128", "attncnp_transformer_r128"])
def test_the_state_is_left_untouched(name):
    s = _setup(name)
    Xt = s["X"][:, :7].contiguous()
    post = s["model"].condition_with_capacity(s["Xc"], s["Yc"], C_PAD + 8, n_cntxt=_i32(COUNTS))
    before = {k: (t.data_ptr(), t.clone()) for k, t in _state_tensors(post).items()}
    d0 = post.query(Xt).base_dist
    a = post.loo().base_dist
    d1 = post.query(Xt).base_dist
    assert torch.equal(d0.loc, d1.loc) and torch.equal(d0.scale, d1.scale)
    for k, t in _state_tensors(post).items():
        assert t.data_ptr() == before[k][0] and torch.equal(t, before[k][1]), k
    b = post.loo().base_dist
    assert torch.equal(a.loc, b.loc) and torch.equal(a.scale, b.scale)
    assert post.n_rows_bound == C_PAD and post.n_cntxt.tolist() == list(COUNTS)


@pytest.mark.parametrize("name", ["attncnp_r128", "attncnp_transformer_r128"])
def test_states_conditioned_without_a_capacity(name):
    s = _setup(name)
    m, n = s["model"], _i32(COUNTS)
    want = m.loo(s["Xc"], s["Yc"], n_cntxt=n).base_dist
    got = m.condition(s["Xc"], s["Yc"], n_cntxt=n).loo().base_dist
    assert_close(got.loc, want.loc.cpu(), what=f"{name}: condition with n_cntxt")
    assert_close(got.scale, want.scale.cpu(), what=f"{name}: condition with n_cntxt")
    plain = m.condition(s["Xc"], s["Yc"])
    if plain._fused_t:
        with pytest.raises(ValueError, match="n_cntxt.*capacity"):
            plain.loo()
    else:
        full = m.loo(s["Xc"], s["Yc"]).base_dist
        assert_close(plain.loo().base_dist.loc, full.loc.cpu(), what=f"{name}: condition without counts")


def test_a_pooled_state_is_refused():
    s = _setup("cnp_r128")
    with pytest.raises(ValueError, match="capacity"):
        s["model"].condition(s["Xc"], s["Yc"]).loo()


# ---- 5. one graph, every mix of counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnp_r128", "attncnp_r128", "attncnp_transformer_r128"])
def test_one_graph_serves_every_mix_of_counts(name):
    """``model.loo`` captured once and replayed with two other count vectors equals the eager call bit for bit; a host sync inside
    the capture would make it fail."""
    s = _setup(name)
    m = s["model"]
    n = _i32(COUNTS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            m.loo(s["Xc"], s["Yc"], n_cntxt=n).base_dist
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d = m.loo(s["Xc"], s["Yc"], n_cntxt=n).base_dist
        loc, scale = d.loc, d.scale
    for counts in (COUNTS, (1, 40, 33), (0, 2, 16)):
        n.copy_(_i32(counts))
        graph.replay()
        torch.cuda.synchronize()
        e = m.loo(s["Xc"], s["Yc"], n_cntxt=_i32(counts)).base_dist
        assert torch.equal(loc, e.loc) and torch.equal(scale, e.scale), (name, counts)
        assert torch.isfinite(loc).all() and torch.isfinite(scale).all()
