"""``Conditioned.sample_functions`` on the GPU: S function draws per task from ONE conditioned context against ``rollout`` on the batch
tiled S times (code from before this feature), with a float64 rollout built from the oracle as the judge of the later chunks.

Gates.  First chunk (no feedback yet): the project's fp32 gate, max|d| <= 1e-5 max|ref|, against the tiled rollout.  Later chunks
feed rounding differences back through the model; both routes are compared with the float64 rollout (the oracle run one task at a
time on the cut context plus the points drawn so far, in float64) and the new route's error must be
<= max(1e-5 max|ref|, 2 x the tiled rollout's error) -- the factor 2 for the different summation order of two equally good fp32
routes.  Inputs: the first seed for which no ReLU pre-activation of that float64 rollout lies within 2e-7 of zero (the
``_well_posed_inputs`` rule of tests/test_hip_masked.py; it reads the reference alone)."""
import pytest
import torch

import specs
from helpers import assert_close, build_model, launch_witness
from oracle import npf_oracle as O
from test_dispatch_rules import bf16_mode  # noqa: F401  (read-only: the bf16 fixture)
from test_hip_dispatch import _c

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, C_PAD, T, DY = 2, 3, 12, 6, 2
# (an empty task next to a partly filled one; a task at full C_PAD next to a partly filled one; a task at full C_PAD next to an empty one)
COUNTS = ((5, 0), (12, 7), (12, 0))
CHUNKS = (1, 4)
RELU_TIE = 2e-7
K = dict(B=B, T=T)
CASES = {
    "attncnp_r128": _c("AttnCNP", 128, C_PAD, **K),
    "attncnp_r64": _c("AttnCNP", 64, C_PAD, **K),
    "attncnp_transformer_r128": _c("AttnCNP", 128, C_PAD, attention="transformer", **K),
    "cnp_r128": _c("CNP", 128, C_PAD, **K),
    "lnp_latent_r128_nz1": _c("LNP", 128, C_PAD, encoded_path="latent", n_z=1, **K),
    "attnlnp_r128_nz1": _c("AttnLNP", 128, C_PAD, n_z=1, **K),
}
_CACHE = {}


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _oracle_rollout(case, params64, inp, counts, eps, chunk, margins=False):
    """float64 [S, B, T, dy]: the rollout recipe (query a block, y = loc + scale * eps, add (x, y) to the context) with the oracle's own
    forward, one task and one sample at a time on the context cut to its count.  ``margins``: -> the smallest |ReLU pre-activation|."""
    cfg = specs.cfg_of(case)
    Y = torch.zeros(S, B, T, DY, dtype=torch.float64)
    O.RELU_MARGINS = [] if margins else None
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the zero representations the oracle makes for an empty context follow the default)
    try:
        with torch.no_grad():
            for s in range(S):
                for b, n in enumerate(counts):
                    X_c, Y_c = inp["X_cntxt"][b:b + 1, :n].double(), inp["Y_cntxt"][b:b + 1, :n].double()
                    eps_z = inp["eps"][:, b:b + 1].double() if "eps" in inp else None
                    for lo in range(0, T, chunk):
                        x = inp["X_trgt"][b:b + 1, lo:lo + chunk].double()
                        o = O.forward(cfg, params64, X_c, Y_c, x, None, eps=eps_z, n_z=1, training=False)
                        y = o["loc"][0] + o["scale"][0] * eps[s, b:b + 1, lo:lo + chunk].double()
                        X_c, Y_c = torch.cat([X_c, x], 1), torch.cat([Y_c, y], 1)
                        Y[s, b, lo:lo + chunk] = y[0]
        return min(O.RELU_MARGINS) if margins else Y
    finally:
        O.RELU_MARGINS = None
        torch.set_default_dtype(default)


def _setup(name):
    """Model, well-posed inputs, the fixed noise, and per (counts, chunk) the float64 rollout -- computed once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    from npf_gwwaveform_amd.neuralproc import MultivariateNormalDiag

    case = CASES[name]
    params = specs.make_params(case, seed=11)
    params64 = {k: v.double() for k, v in params.items()}
    eps = torch.randn(S, B, T, DY, generator=torch.Generator().manual_seed(77))
    for seed in range(4321, 4321 + 200):
        inp = specs.make_inputs(case, seed=seed)
        if min(_oracle_rollout(case, params64, inp, c, eps, ch, margins=True) for c in COUNTS for ch in CHUNKS) >= RELU_TIE:
            break
    else:
        raise AssertionError("no well-posed inputs in 200 seeds")
    model = build_model(case, DEV, params=params).eval()
    if hasattr(model, "LatentDistribution"):
        model.LatentDistribution = MultivariateNormalDiag
    ref64 = {(c, ch): _oracle_rollout(case, params64, inp, c, eps, ch) for c in COUNTS for ch in CHUNKS}
    dev = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    out = dict(case=case, model=model, inp=dev, eps=eps.to(DEV), ref64=ref64, seed=seed, latent="eps" in inp)
    _CACHE[name] = out
    return out


def _post(s, counts, capacity=C_PAD):
    """The conditioned state under test: capacity = C_PAD, so it has NO free row -- the draws cannot live in it."""
    post = s["model"].condition_with_capacity(s["inp"]["X_cntxt"], s["inp"]["Y_cntxt"], capacity, n_cntxt=_i32(counts),
                                              n_z_samples=1 if s["latent"] else None)
    if s["latent"]:
        with torch.no_grad():  # (``_refresh`` writes into tensors made under no_grad, as ``extend`` calls it)
            post.eps.copy_(s["inp"]["eps"])
            post._refresh()
    return post


def _tiled_rollout(s, counts, eps, chunk, n_samples=S):
    """``rollout`` on the batch tiled S times (task s B + b), every sample of task b with the latent noise of task b."""
    inp = s["inp"]
    rep = lambda t: t.repeat(n_samples, 1, 1)  # noqa: E731
    post = s["model"].condition_with_capacity(rep(inp["X_cntxt"]), rep(inp["Y_cntxt"]), C_PAD + T, n_cntxt=_i32(list(counts) * n_samples),
                                              n_z_samples=1 if s["latent"] else None)
    if s["latent"]:
        with torch.no_grad():
            post.eps.copy_(inp["eps"].repeat(1, n_samples, 1, 1))
            post._refresh()
    Y = post.rollout(rep(inp["X_trgt"]), eps=eps.reshape(n_samples * B, T, DY), chunk=chunk)
    return Y.view(n_samples, B, T, DY)


def _gate(tag, got, tiled, ref64, chunk):
    first = slice(0, chunk)
    assert_close(got[:, :, first], tiled[:, :, first], what=f"{tag}: first chunk against the tiled rollout")
    scale = float(ref64.abs().max())
    e_new = float((got.cpu().double() - ref64).abs().max())
    e_old = float((tiled.cpu().double() - ref64).abs().max())
    print(f"{tag}: max|ref|={scale:.3e}  error against the float64 rollout: sample_functions {e_new:.3e}, tiled rollout {e_old:.3e}")
    assert torch.isfinite(got).all()
    assert e_new <= max(1e-5 * scale, 2 * e_old), f"{tag}: {e_new:.3e} > max(1e-5 * {scale:.3e}, 2 * {e_old:.3e})"


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("name", list(CASES))
def test_samples_equal_the_tiled_rollout(name, counts, chunk):
    s = _setup(name)
    post = _post(s, counts)
    with launch_witness() as w:
        Y = post.sample_functions(s["inp"]["X_trgt"], S, eps=s["eps"], chunk=chunk)
        torch.cuda.synchronize()
    assert Y.shape == (S, B, T, DY)
    steps = -(-T // chunk)
    attentive = s["case"]["kind"].startswith("Attn")
    assert w["npf_masked_attn_fwd_prefix"] == (steps if attentive else 0) and w["npf_masked_attn_fwd"] == 0, w
    assert w["npf_append_points"] == steps, w
    tag = f"{name} counts={counts} chunk={chunk} (input seed {s['seed']})"
    _gate(tag, Y, _tiled_rollout(s, counts, s["eps"], chunk), s["ref64"][(counts, chunk)], chunk)
    # S = 1 equals rollout within the same gates
    Y1 = _post(s, counts).sample_functions(s["inp"]["X_trgt"], 1, eps=s["eps"][:1], chunk=chunk)
    _gate(tag + " S=1", Y1, _tiled_rollout(s, counts, s["eps"][:1], chunk, n_samples=1), s["ref64"][(counts, chunk)][:1], chunk)


def _state_tensors(post):
    ts = dict(n_cntxt=post.n_cntxt, R_pts=post._R_pts.t, R=post._R if torch.is_tensor(post._R) else post._R.t)
    if post._Xc_pt is not None:
        ts["Xc"] = post._Xc_pt.t
    if post.z_samples is not None:
        ts.update(z=post.z_samples, eps=post.eps, q_loc=post.q_zCc.base_dist.loc, q_scale=post.q_zCc.base_dist.scale)
    return ts


@pytest.mark.parametrize("name", list(CASES))
def test_the_state_is_left_untouched(name):
    s = _setup(name)
    counts, Xt = COUNTS[1], s["inp"]["X_trgt"]
    post = _post(s, counts, capacity=C_PAD + T)  # (room for the rollout that follows)
    before = {k: (t.data_ptr(), t.clone()) for k, t in _state_tensors(post).items()}
    d0 = post.query(Xt).base_dist
    bound = post.n_rows_bound
    Y = post.sample_functions(Xt, S, eps=s["eps"], chunk=1)
    d1 = post.query(Xt).base_dist
    assert torch.equal(d0.loc, d1.loc) and torch.equal(d0.scale, d1.scale)
    assert post.n_rows_bound == bound and post.n_cntxt.tolist() == list(counts)
    for k, t in _state_tensors(post).items():
        assert t.data_ptr() == before[k][0] and torch.equal(t, before[k][1]), k
    # the same noise, the same bits; another eps[1] moves sample 1 only
    assert torch.equal(post.sample_functions(Xt, S, eps=s["eps"], chunk=1), Y)
    eps2 = s["eps"].clone()
    eps2[1] += 0.5
    Y2 = post.sample_functions(Xt, S, eps=eps2, chunk=1)
    assert torch.equal(Y2[0], Y[0]) and torch.equal(Y2[2], Y[2]) and not torch.equal(Y2[1], Y[1])
    # the default noise is one torch.randn draw
    torch.manual_seed(3)
    a = post.sample_functions(Xt, S)
    torch.manual_seed(3)
    assert torch.equal(a, post.sample_functions(Xt, S, eps=torch.randn(S, B, T, DY, device=DEV)))
    # a rollout on the same object gives what it gives on a fresh one
    fresh = _post(s, counts, capacity=C_PAD + T)
    assert torch.equal(post.rollout(Xt, eps=s["eps"][0]), fresh.rollout(Xt, eps=s["eps"][0]))


@pytest.mark.parametrize("name", ["attncnp_r128", "cnp_r128", "attncnp_transformer_r128"])
def test_states_conditioned_without_a_capacity(name):
    """``condition(..., n_cntxt=...)`` and, where the context was not stored for the fused target side, ``condition`` without counts
    (full counts built on the device) give the draws of the capacity state -- in one block of T targets, so that nothing is fed back
    and the fp32 gate applies as it stands."""
    s = _setup(name)
    inp, counts = s["inp"], COUNTS[1]
    want = _post(s, counts).sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=T)
    got = s["model"].condition(inp["X_cntxt"], inp["Y_cntxt"], n_cntxt=_i32(counts)).sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=T)
    assert_close(got, want, what=f"{name}: condition with n_cntxt")
    plain = s["model"].condition(inp["X_cntxt"], inp["Y_cntxt"])
    if plain._fused_t:
        with pytest.raises(ValueError, match="n_cntxt.*capacity"):
            plain.sample_functions(inp["X_trgt"], S)
    else:
        full = _post(s, (C_PAD, C_PAD)).sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=T)
        assert_close(plain.sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=T), full, what=f"{name}: condition without counts")


@pytest.mark.parametrize("name", ["attncnp_r128", "attncnp_transformer_r128", "cnp_r128"])
def test_a_state_conditioned_on_no_context_at_all(name):
    """``condition`` on C = 0 points (no prefix rows at all; with heads nothing to project) draws what a capacity state with counts
    (0, 0) draws."""
    s = _setup(name)
    inp = s["inp"]
    empty = s["model"].condition(inp["X_cntxt"][:, :0], inp["Y_cntxt"][:, :0])
    assert not empty._fused_t
    for chunk in (T, 2):
        got = empty.sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=chunk)
        want = _post(s, (0, 0)).sample_functions(inp["X_trgt"], S, eps=s["eps"], chunk=chunk)
        tiled = _tiled_rollout(s, (0, 0), s["eps"], chunk)
        assert_close(got[:, :, :chunk], want[:, :, :chunk], what=f"{name}: first chunk, C = 0 against counts (0, 0)")
        assert_close(got[:, :, :chunk], tiled[:, :, :chunk], what=f"{name}: first chunk, C = 0 against the tiled rollout")
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("name", ["attncnp_r128", "attncnp_transformer_r128", "cnp_r128", "attnlnp_r128_nz1"])
def test_one_step_replays_from_one_graph(name):
    """One captured step (query a block, draw, append to the tails) replayed for three blocks equals the eager call bit for bit."""
    s = _setup(name)
    counts, Xt, eps, n = COUNTS[0], s["inp"]["X_trgt"], s["eps"], 2
    post = _post(s, counts)
    eager = post.sample_functions(Xt, S, eps=eps, chunk=n)
    sampler = post._function_sampler(Xt, S, eps, n)[0]
    warm = post._function_sampler(Xt, S, eps, n)[0]
    dx = s["case"]["dx"]
    x_s, e_s = torch.zeros(S * B, n, dx, device=DEV), torch.zeros(S * B, n, DY, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):  # (on tails of its own)
            warm.step(x_s, e_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y_s = sampler.step(x_s, e_s)
    assert sampler.n_tail.tolist() == [0] * (S * B)  # (captured, not run)
    for i in range(3):
        x_s.copy_(Xt[:, i * n:(i + 1) * n].unsqueeze(0).expand(S, B, n, dx).reshape(S * B, n, dx))
        e_s.copy_(eps[:, :, i * n:(i + 1) * n].reshape(S * B, n, DY))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_s.view(S, B, n, DY), eager[:, :, i * n:(i + 1) * n]), (name, i)
    assert sampler.n_tail.tolist() == [3 * n] * (S * B)


def test_refusals():
    s = _setup("lnp_latent_r128_nz1")
    inp = s["inp"]
    post = s["model"].condition_with_capacity(inp["X_cntxt"], inp["Y_cntxt"], C_PAD, n_z_samples=4)
    with pytest.raises(ValueError, match="n_z_samples=1"):
        post.sample_functions(inp["X_trgt"], S)
    a = _setup("attncnp_r128")
    # a context stored for the fused target side: whatever size takes that route
    for C in (C_PAD, 64, 128):
        case = dict(a["case"], C=C)
        x = specs.make_inputs(case, seed=1)
        plain = a["model"].condition(x["X_cntxt"].to(DEV), x["Y_cntxt"].to(DEV))
        if plain._fused_t:
            with pytest.raises(ValueError, match="n_cntxt.*capacity"):
                plain.sample_functions(a["inp"]["X_trgt"], S)
            break
    else:
        pytest.fail("no context size took the fused target side")


def test_refused_in_the_bf16_mode_and_with_self_attention(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    s = _setup("attncnp_r128")
    post = _post_fp32_state(s)
    with pytest.raises(NotImplementedError, match="sample_functions.*bf16"):
        post.sample_functions(s["inp"]["X_trgt"], S)
    sa = A.Conditioned(A.AttnCNP(1, 2, r_dim=32, is_self_attn=True).to(DEV), None, None, None, None, None, B, C_PAD, False)
    with pytest.raises(NotImplementedError, match="sample_functions.*is_self_attn"):
        sa.sample_functions(s["inp"]["X_trgt"], S)


def _post_fp32_state(s):
    """A capacity state built by hand (``condition_with_capacity`` itself refuses the bf16 mode)."""
    import npf_gwwaveform_amd as A

    return A.Conditioned(s["model"], None, None, None, None, _i32([0] * B), B, C_PAD, False, capacity=C_PAD)
