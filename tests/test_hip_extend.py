"""Growing contexts on the GPU: ``condition_with_capacity`` + ``Conditioned.extend`` against ``condition`` on the union of the points
(the masked route the parent already gates against the oracle) and against the float64 oracle on the batch cut per task,
independence of the rows beyond the counts, one captured ``extend`` + ``query`` + ``summary`` replayed with new data, ``rollout``
against the loop it stands for, and the refusals.

Gate: the project's fp32 gate, max|d| <= 1e-5 max|ref| (``helpers.assert_close`` at its default), wherever two routes are compared;
``torch.equal`` wherever the same launches run on the same numbers."""
import pytest
import torch

import specs
from helpers import assert_close, build_model, launch_witness
from oracle import npf_oracle as O
from test_dispatch_rules import bf16_mode  # noqa: F401  (read-only: the bf16 fixture)
from test_hip_dispatch import _c

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C0, CAP, T = 4, 30, 96, 40
N1, N2 = 5, 33                      # the second extension crosses the 32-row tile boundary for every task
N_CNTXT = [0, 30, 17, 9]
N_NEW1 = [5, 0, 3, 5]               # ragged, one task adds nothing
S = dict(B=B, T=T)
CASES = {
    "cnp_r128": _c("CNP", 128, C0, **S),
    "lnp_latent_r128_nz4": _c("LNP", 128, C0, encoded_path="latent", n_z=4, **S),
    "lnp_both_r128_nz4": _c("LNP", 128, C0, encoded_path="both", n_z=4, **S),
    "attncnp_r128": _c("AttnCNP", 128, C0, **S),
    "attncnp_r256": _c("AttnCNP", 256, C0, **S),
    "attncnp_transformer_r128": _c("AttnCNP", 128, C0, attention="transformer", **S),
    "attnlnp_r256_nz8": _c("AttnLNP", 256, C0, n_z=8, **S),
}
_CACHE = {}


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _setup(name):
    """Model, the three blocks of context points, the targets, and the per-task union (host-built, zero padded) with its counts."""
    if name in _CACHE:
        return _CACHE[name]
    from npf_gwwaveform_amd.neuralproc import MultivariateNormalDiag

    case = CASES[name]
    params = specs.make_params(case, seed=11)
    model = build_model(case, DEV, params=params).eval()
    if hasattr(model, "LatentDistribution"):
        model.LatentDistribution = MultivariateNormalDiag  # (the package's own rsample: the tests seed the global RNG)
    inp = specs.make_inputs(dict(case, C=C0 + N1 + N2), seed=4321)
    X, Y = inp["X_cntxt"], inp["Y_cntxt"]
    blocks = [(X[:, :C0], Y[:, :C0]), (X[:, C0:C0 + N1], Y[:, C0:C0 + N1]), (X[:, C0 + N1:], Y[:, C0 + N1:])]
    n_total = [N_CNTXT[b] + N_NEW1[b] + N2 for b in range(B)]
    X_all, Y_all = torch.zeros_like(X), torch.zeros_like(Y)
    for b in range(B):
        for src, dst in ((X, X_all), (Y, Y_all)):
            rows = torch.cat([src[b, :N_CNTXT[b]], src[b, C0:C0 + N_NEW1[b]], src[b, C0 + N1:]])
            dst[b, :n_total[b]] = rows
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    out = dict(case=case, params=params, model=model, blocks=[(dev(a), dev(b_)) for a, b_ in blocks], Xt=dev(inp["X_trgt"]),
               X_all=dev(X_all), Y_all=dev(Y_all), n_total=n_total, cpu=dict(X_all=X_all, Y_all=Y_all, Xt=inp["X_trgt"]))
    _CACHE[name] = out
    return out


def _grown(s, seed=5, capacity=CAP):
    """Conditioned on the ragged first block, extended by the ragged second and the full third."""
    (X0, Y0), (X1, Y1), (X2, Y2) = s["blocks"]
    torch.manual_seed(seed)
    post = s["model"].condition_with_capacity(X0, Y0, capacity, n_cntxt=_i32(N_CNTXT))
    eps = None if post.eps is None else post.eps.clone()
    assert post.extend(X1, Y1, n_new=_i32(N_NEW1)) is post
    post.extend(X2, Y2)
    return post, eps


def _loc_scale(p):
    return p.base_dist.loc, p.base_dist.scale


# ---- extend equals conditioning on the union ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_extend_equals_conditioning_on_the_union(name):
    s = _setup(name)
    model, latent = s["model"], s["case"]["kind"] in ("LNP", "AttnLNP")
    post, eps0 = _grown(s)
    assert post.capacity == CAP and post.n_cntxt.dtype == torch.int32 and post.n_cntxt.tolist() == s["n_total"]
    assert post.n_rows_bound == C0 + N1 + N2
    torch.manual_seed(5)
    ref = model.condition(s["X_all"], s["Y_all"], n_cntxt=_i32(s["n_total"]))
    for got, want, what in zip(_loc_scale(post.query(s["Xt"])), _loc_scale(ref.query(s["Xt"])), ("loc", "scale")):
        assert got.shape == want.shape == (s["case"].get("n_z", 1), B, T, s["case"]["dy"])
        assert_close(got, want, what=f"{what} {name}")
    if latent:
        assert torch.equal(post.eps, eps0) and post.eps.shape == (s["case"]["n_z"], B, 1, model.z_dim)
        assert_close(post.z_samples, ref.z_samples, what=f"z_samples {name}")
        assert_close(post.q_zCc.base_dist.loc, ref.q_zCc.base_dist.loc, what=f"q_zCc loc {name}")
        assert_close(post.q_zCc.base_dist.scale, ref.q_zCc.base_dist.scale, what=f"q_zCc scale {name}")
    else:
        assert post.eps is None and post.z_samples is None and post.q_zCc is None


@pytest.mark.parametrize("name", ["cnp_r128", "attncnp_r128"])
def test_extended_model_matches_the_per_task_oracle(name):
    s = _setup(name)
    cfg, cpu = specs.cfg_of(s["case"]), s["cpu"]
    outs = [O.forward(cfg, s["params"], cpu["X_all"][b:b + 1, :n], cpu["Y_all"][b:b + 1, :n], cpu["Xt"][b:b + 1], None, eps=None,
                      n_z=1, training=False) for b, n in enumerate(s["n_total"])]
    post, _ = _grown(s)
    p = post.query(s["Xt"])
    assert_close(p.base_dist.loc, torch.cat([o["loc"].detach() for o in outs], 1), what=f"loc {name}")
    assert_close(p.base_dist.scale, torch.cat([o["scale"].detach() for o in outs], 1), what=f"scale {name}")


@pytest.mark.parametrize("name", list(CASES))
def test_empty_start_then_extend_equals_conditioning_on_the_extension(name):
    s = _setup(name)
    model, (X2, Y2) = s["model"], s["blocks"][2]
    torch.manual_seed(9)
    post = model.condition_with_capacity(X2[:, :0], Y2[:, :0], 64)
    assert post.n_cntxt.tolist() == [0] * B
    empty = _loc_scale(post.query(s["Xt"]))
    torch.manual_seed(9)
    for got, want in zip(empty, _loc_scale(model.condition(X2[:, :0], Y2[:, :0]).query(s["Xt"]))):
        assert_close(got, want, what=f"no context {name}")
    post.extend(X2, Y2)
    assert post.n_cntxt.tolist() == [N2] * B
    torch.manual_seed(9)
    ref = model.condition(X2, Y2)
    for got, want, what in zip(_loc_scale(post.query(s["Xt"])), _loc_scale(ref.query(s["Xt"])), ("loc", "scale")):
        assert_close(got, want, what=f"{what} {name}")


# ---- the rows beyond the counts ----------------------------------------------------------------------------------------------------
def _poison_beyond_counts(t, counts):
    """NaN into every row at and beyond the task's count of a PT32 tensor [B, tiles, F/4, 32, 4], tile padding included."""
    tiles = t.shape[1]
    row = torch.arange(32 * tiles, device=t.device).view(1, tiles, 1, 32, 1)
    t.masked_fill_(row >= counts.view(-1, 1, 1, 1, 1), float("nan"))


@pytest.mark.parametrize("name", list(CASES))
def test_rows_beyond_the_counts_have_no_influence(name):
    s = _setup(name)
    post, _ = _grown(s)
    before = [t.clone() for t in _loc_scale(post.query(s["Xt"]))]
    _poison_beyond_counts(post._R_pts.t, post.n_cntxt)
    if post._Xc_pt is not None:
        _poison_beyond_counts(post._Xc_pt.t, post.n_cntxt)
    assert torch.isnan(post._R_pts.t).any()
    for got, want in zip(_loc_scale(post.query(s["Xt"])), before):
        assert torch.equal(got, want), name
    # an extension that adds no row re-pools the stored rows and refreshes q(z | C): still the same numbers
    X1, Y1 = s["blocks"][1]
    post.extend(X1[:, :1].contiguous(), Y1[:, :1].contiguous(), n_new=_i32([0] * B))
    assert post.n_cntxt.tolist() == s["n_total"]
    for got, want in zip(_loc_scale(post.query(s["Xt"])), before):
        assert torch.equal(got, want), f"{name} after an empty extension"


# ---- one graph ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnp_r128", "lnp_both_r128_nz4", "attncnp_r128", "attnlnp_r256_nz8"])
def test_extend_query_summary_replay_from_one_graph(name):
    s = _setup(name)
    model, case = s["model"], s["case"]
    X0, Y0 = s["blocks"][0]

    def fresh():
        torch.manual_seed(23)
        return model.condition_with_capacity(X0, Y0, CAP, n_cntxt=_i32(N_CNTXT))

    post, twin, warm = fresh(), fresh(), fresh()
    Xq = s["Xt"]
    X_s, Y_s, n_s = torch.zeros(B, N1, case["dx"], device=DEV), torch.zeros(B, N1, case["dy"], device=DEV), _i32([0] * B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):  # (on an object of its own: an extension changes the state)
            warm.extend(X_s, Y_s, n_s).query(Xq).summary()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_g = post.extend(X_s, Y_s, n_s).query(Xq).summary()
    assert post.n_cntxt.tolist() == N_CNTXT  # (captured, not run)
    g = torch.Generator().manual_seed(8)
    total = list(N_CNTXT)
    for step in range(3):
        X_new = (torch.rand(B, N1, case["dx"], generator=g) * 2 - 1).to(DEV)
        Y_new = torch.randn(B, N1, case["dy"], generator=g).to(DEV)
        n_new = torch.randint(0, N1 + 1, (B,), generator=g, dtype=torch.int32)
        total = [a + int(b) for a, b in zip(total, n_new)]
        X_s.copy_(X_new)
        Y_s.copy_(Y_new)
        n_s.copy_(n_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = twin.extend(X_new, Y_new, n_new.to(DEV)).query(Xq).summary()
        for a, b in zip(s_g[:3], eager[:3]):
            assert torch.equal(a, b), (name, step)
        assert torch.equal(post.n_cntxt, twin.n_cntxt)
    assert post.n_cntxt.tolist() == total


# ---- rollout -----------------------------------------------------------------------------------------------------------------------
TR = 21


def _rollout_setup(name, n_z=None):
    s = _setup(name)
    X0, Y0 = s["blocks"][0]
    g = torch.Generator().manual_seed(77)
    eps = torch.randn(B, TR, s["case"]["dy"], generator=g).to(DEV)
    Xt = s["Xt"][:, :TR].contiguous()

    def fresh():
        torch.manual_seed(31)
        return s["model"].condition_with_capacity(X0, Y0, CAP, n_cntxt=_i32(N_CNTXT), n_z_samples=n_z)

    return s, fresh, Xt, eps


def _explicit_loop(post, Xt, eps, chunk):
    ys = []
    for lo in range(0, Xt.shape[1], chunk):
        x = Xt[:, lo:lo + chunk].contiguous()
        d = post.query(x).base_dist
        y = d.loc[0] + d.scale[0] * eps[:, lo:lo + chunk]
        post.extend(x, y)
        ys.append(y)
    return torch.cat(ys, 1)


@pytest.mark.parametrize("name,n_z", [("cnp_r128", None), ("attncnp_r128", None), ("attnlnp_r256_nz8", 1)])
def test_rollout_is_the_query_draw_extend_loop(name, n_z):
    s, fresh, Xt, eps = _rollout_setup(name, n_z)
    for chunk in (1, 7):
        post = fresh()
        Y = post.rollout(Xt, eps=eps, chunk=chunk)
        assert Y.shape == (B, TR, s["case"]["dy"])
        assert torch.equal(Y, _explicit_loop(fresh(), Xt, eps, chunk)), (name, chunk)
        assert post.n_cntxt.tolist() == [n + TR for n in N_CNTXT] and post.n_rows_bound == C0 + TR  # (left extended)
    if n_z is None:  # one block: nothing is fed back, the draw of one query
        d = fresh().query(Xt).base_dist
        assert torch.equal(fresh().rollout(Xt, eps=eps, chunk=TR), d.loc[0] + d.scale[0] * eps), name
    one, two = fresh(), fresh()
    torch.manual_seed(3)
    a = one.rollout(Xt)  # (eps drawn once with torch.randn)
    torch.manual_seed(3)
    assert torch.equal(a, two.rollout(Xt, eps=torch.randn(B, TR, s["case"]["dy"], device=DEV)))


def test_rollout_feeds_the_draws_back_for_cnp():
    s, fresh, Xt, eps = _rollout_setup("cnp_r128")
    Y = fresh().rollout(Xt, eps=eps)
    eps2 = eps.clone()
    eps2[:, 0] += 1.0
    Y2 = fresh().rollout(Xt, eps=eps2)
    assert not torch.equal(Y2[:, 0], Y[:, 0])
    assert (Y2[:, 1] != Y[:, 1]).any(dim=-1).all()  # every task: the second point saw another first draw
    # the one-shot predictive has no such feedback
    d = fresh().query(Xt).base_dist
    one, two = d.loc[0] + d.scale[0] * eps, d.loc[0] + d.scale[0] * eps2
    assert torch.equal(one[:, 1:], two[:, 1:])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    s = _setup("lnp_both_r128_nz4")
    model, (X0, Y0), (X1, Y1) = s["model"], s["blocks"][0], s["blocks"][1]
    with pytest.raises(ValueError, match="capacity"):
        model.condition(X0, Y0).extend(X1, Y1)
    with pytest.raises(ValueError, match="capacity"):
        model.condition(X0, Y0).rollout(s["Xt"])
    with pytest.raises(ValueError, match="capacity"):
        model.condition_with_capacity(X0, Y0, C0 - 1)
    post = model.condition_with_capacity(X0, Y0, C0 + N1)
    with pytest.raises(ValueError, match="capacity"):
        post.extend(s["blocks"][2][0], s["blocks"][2][1])  # 33 rows into 5 free ones
    cnp = _setup("cnp_r128")["model"].condition_with_capacity(X0, Y0, C0 + N1)
    with pytest.raises(ValueError, match="capacity"):
        cnp.rollout(s["Xt"][:, :N1 + 1].contiguous())
    with pytest.raises(ValueError, match="X_new"):
        post.extend(X1[:B - 1], Y1[:B - 1])
    with pytest.raises(ValueError, match="X_new"):
        post.extend(torch.cat([X1, X1], -1), Y1)
    with pytest.raises(ValueError, match="Y_new"):
        post.extend(X1, Y1[..., :1].contiguous())
    with pytest.raises(ValueError, match="Y_new"):
        post.extend(X1, Y1[:, :N1 - 1].contiguous())
    with pytest.raises(ValueError, match="n_new"):
        post.extend(X1, Y1, n_new=torch.zeros(B, dtype=torch.int32))  # (counts are device data)
    with pytest.raises(ValueError, match="n_z_samples=1"):
        post.rollout(s["Xt"][:, :2].contiguous())  # n_z = 4
    assert post.n_cntxt.tolist() == [C0] * B and post.n_rows_bound == C0  # (a refused call changes nothing)
    post.extend(X1, Y1)  # exactly full
    assert post.n_cntxt.tolist() == [C0 + N1] * B
    with pytest.raises(ValueError, match="capacity"):
        post.extend(X1[:, :1].contiguous(), Y1[:, :1].contiguous())


def test_capacity_is_refused_where_counts_are(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    s = _setup("attncnp_r128")
    X0, Y0 = s["blocks"][0]
    with pytest.raises(NotImplementedError, match="capacity.*bf16"):
        s["model"].condition_with_capacity(X0, Y0, CAP)
    sa = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True).to(DEV)
    with pytest.raises(NotImplementedError, match="capacity.*is_self_attn"):
        sa.condition_with_capacity(X0, Y0, CAP)


# ---- without a capacity nothing changes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnp_r128", "attncnp_r128", "attnlnp_r256_nz8"])
def test_condition_without_capacity_launches_what_forward_does(name):
    from test_hip_dispatch import SPY

    s = _setup(name)
    model, (X0, Y0) = s["model"], s["blocks"][0]
    torch.manual_seed(1)
    with torch.no_grad(), launch_witness(spy=SPY) as wf:
        model(X0, Y0, s["Xt"])
    torch.manual_seed(1)
    with launch_witness(spy=SPY) as wc:
        post = model.condition(X0, Y0)
    with launch_witness(spy=SPY) as wq:
        post.query(s["Xt"])
    assert post.capacity is None and post.eps is None
    for k in set(wf.calls) | set(wc.calls) | set(wq.calls) | set(SPY):
        assert wf[k] == wc[k] + wq[k], f"{k}: forward {wf[k]}, condition {wc[k]} + query {wq[k]}"
    assert wc["npf_append_points"] == 0 and wc["npf_masked_mean_fwd"] == 0 and wq["npf_masked_attn_fwd"] == 0
    # with a capacity: the per-point launches of the padded route, one append, and the masked kernels
    with launch_witness(spy=SPY) as wg:
        grown = model.condition_with_capacity(X0, Y0, CAP)
    with launch_witness(spy=SPY) as we:
        grown.extend(*s["blocks"][1])
    attentive = s["case"]["kind"].startswith("Attn")
    for w in (wg, we):
        assert w["npf_append_points"] == 1 and w["x6.target_side"] == 0, w
        assert w["npf_masked_mean_fwd"] == int(name != "attncnp_r128"), w
    with launch_witness(spy=SPY) as wq2:
        grown.query(s["Xt"])
    assert wq2["npf_masked_attn_fwd"] == int(attentive) and wq2["x6.target_side"] == 0 and wq2["npf_append_points"] == 0, wq2
