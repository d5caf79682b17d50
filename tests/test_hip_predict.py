"""Conditioned prediction on the GPU: ``npf_mixture_summary`` against a float64 reference written here, ``condition`` + ``query``
against ``forward`` (bit for bit, on every dispatch route, with the launches recorded by the witness of tests/helpers.py), coherence
of the grids queried from one conditioned model, the memory ``summary`` needs, and a captured ``query`` + ``summary``.

Gates.  ``mean`` / ``std``: the project's fp32 gate, max|d| <= 1e-5 max|ref| (``helpers.assert_close``).  Quantiles are gated on the
CDF residual, |F64(x) - p| <= 1e-5 + 2 ulp32(x) f64(x): the project's figure on a quantity of scale 1, plus what the spacing of the
returned float costs where the density is f64(x) -- on a plateau between clusters x itself is ill-conditioned, the residual is not.
The bracket: x inside [min_k a_k, max_k a_k], a_k = mu_k + sg_k z_p in float64, widened by 2 ulp32(S), S = max_k(|mu_k| +
sg_k |z_p|): a_k is a sum of two fp32 terms of that magnitude (z_p itself reaches the kernel rounded to fp32), so the spacing of S is
the unit of its rounding whatever cancels in the sum."""
import math

import pytest
import torch

import specs
from helpers import assert_close, build_model, launch_witness
from test_hip_dispatch import SPY, _c, _expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBS = (0.025, 0.5, 0.975)


# ---- float64 reference -----------------------------------------------------------------------------------------------------------
def _components(suff, n_z, dy, homosk, n_valid):
    """float64 (mu, sg) [n_z, B, pts, dy] by the head's formulas; rows beyond the count hold mu = 0, sg = 1."""
    rows, pts, _ = suff.shape
    B = rows // n_z
    s = suff.double().view(n_z, B, pts, 2 * dy)
    nv = torch.full((B,), pts, device=suff.device) if n_valid is None else n_valid.clamp(0, pts).long()
    live = (torch.arange(pts, device=suff.device).view(1, pts) < nv.view(B, 1)).view(1, B, pts, 1)
    s = torch.where(live, s, torch.zeros_like(s))  # (padding may be NaN: never read)
    mu, raw = s[..., :dy], s[..., dy:]
    sg = 0.01 + 0.99 * torch.where(raw > 30.0, raw, torch.log1p(torch.exp(raw.clamp(max=30.0))))
    if homosk:
        pooled = (sg * live).sum(2, keepdim=True) / nv.clamp(min=1).view(1, B, 1, 1)
        sg = pooled.expand_as(sg)
    live = live.expand_as(mu)
    return torch.where(live, mu, torch.zeros_like(mu)), torch.where(live, sg, torch.ones_like(sg)), live[0]


def _cdf_pdf(x, mu, sg):
    u = (x.unsqueeze(0) - mu) / sg
    return (0.5 * torch.special.erfc(-u / math.sqrt(2.0))).mean(0), (torch.exp(-0.5 * u * u) / (sg * math.sqrt(2.0 * math.pi))).mean(0)


def _reference(suff, n_z, dy, homosk, probs, n_valid):
    from npf_gwwaveform_amd import functional as FN

    mu, sg, live = _components(suff, n_z, dy, homosk, n_valid)
    mean = mu.mean(0)
    std = (sg * sg + (mu - mean) ** 2).mean(0).sqrt()
    mean, std = torch.where(live, mean, torch.zeros_like(mean)), torch.where(live, std, torch.ones_like(std))
    quant, brackets = [], []
    for p, z in zip(probs, FN.normal_quantiles(probs)):
        a = mu + sg * z
        lo, hi = a.min(0).values, a.max(0).values
        brackets.append((lo.clone(), hi.clone(), (mu.abs() + sg * abs(z)).max(0).values))
        for _ in range(200):  # bisection on the float64 mixture CDF
            mid = 0.5 * (lo + hi)
            below = _cdf_pdf(mid, mu, sg)[0] < p
            lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
        quant.append(0.5 * (lo + hi))
    return mean, std, quant, brackets, (mu, sg, live)


def _ulp32(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _check_against_reference(suff, n_z, dy, homosk, n_valid, what):
    """Every gate of the module docstring for one launch; returns the worst CDF residual and the worst residual / gate ratio."""
    from npf_gwwaveform_amd import functional as FN

    mean, std, quant = FN.mixture_summary(suff, n_z, dy, homosk, probs=PROBS, n_valid=n_valid)
    mean0, std0, quant0 = FN.mixture_summary(suff, n_z, dy, homosk, n_valid=n_valid)  # the moments-only launch
    assert quant0.shape[0] == 0 and torch.equal(mean0, mean) and torch.equal(std0, std), what
    r_mean, r_std, r_quant, brackets, (mu, sg, live) = _reference(suff, n_z, dy, homosk, PROBS, n_valid)
    assert_close(mean, r_mean, what=f"mean {what}")
    assert_close(std, r_std, what=f"std {what}")
    z32 = torch.tensor(FN.normal_quantiles(PROBS), dtype=torch.float64).float()
    worst, worst_ratio, worst_br = 0.0, 0.0, 0.0
    for j, p in enumerate(PROBS):
        x = quant[j].double()
        assert torch.isfinite(x).all(), what
        F, f = _cdf_pdf(x, mu, sg)
        res = (F - p).abs()[live]
        gate = (1e-5 + 2.0 * _ulp32(x) * f)[live]
        if res.numel():
            worst = max(worst, res.max().item())
            worst_ratio = max(worst_ratio, (res / gate).max().item())
        lo, hi, S = brackets[j]
        out = torch.maximum(lo - x, x - hi)[live] / _ulp32(S)[live]
        if out.numel():
            worst_br = max(worst_br, out.max().item())
        dead = ~live
        assert (mean[dead] == 0).all() and (std[dead] == 1).all() and (quant[j][dead] == z32[j].item()).all(), f"padding {what}"
        if j:
            assert (quant[j] >= quant[j - 1]).all(), f"quantiles not monotone in p {what}"
    print(f"PREDICT {what}: worst |F64(x)-p| = {worst:.3e}, worst residual/gate = {worst_ratio:.3f}, "
          f"worst excursion from the float64 bracket = {worst_br:.2f} ulp32(S)")
    assert worst_ratio <= 1.0, f"CDF residual {what}: {worst:.3e} ({worst_ratio:.3f} of the gate)"
    assert worst_br <= 2.0, f"quantile outside the float64 bracket by {worst_br:.2f} ulp32(S) {what}"
    if n_z == 1:
        loc, scale, _ = FN.gauss_head(suff, None, dy, homosk, n_valid=n_valid)
        for j in range(len(PROBS)):
            assert_close(quant[j], loc.double() + scale.double() * float(z32[j].double()), what=f"n_z=1 quantile {what}")
    return worst, worst_ratio


def _random_suff(n_z, B, pts, dy, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n_z * B, pts, 2 * dy, generator=g).to(DEV)


def _adversarial(n_z, B, pts, dy, seed):
    """identical components; two well-separated clusters with tiny scales (raw scale -20); raw scale +30; mu of magnitude 10."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    same = torch.randn(1, B, pts, 2 * dy, generator=g).expand(n_z, B, pts, 2 * dy).reshape(n_z * B, pts, 2 * dy).contiguous()
    side = torch.where(torch.arange(n_z) % 2 == 0, -10.0, 10.0).view(n_z, 1, 1, 1)
    clusters = torch.cat([side + 0.01 * torch.randn(n_z, B, pts, dy, generator=g), torch.full((n_z, B, pts, dy), -20.0)], -1)
    wide = torch.cat([10.0 * torch.sign(torch.randn(n_z, B, pts, dy, generator=g)) + torch.randn(n_z, B, pts, dy, generator=g),
                      torch.full((n_z, B, pts, dy), 30.0)], -1)
    mixed = torch.cat([10.0 * torch.randn(n_z, B, pts, dy, generator=g),
                       torch.where(torch.rand(n_z, B, pts, dy, generator=g) < 0.5, -20.0, 30.0)], -1)
    return {"identical": same.to(DEV), "clusters": clusters.reshape(n_z * B, pts, 2 * dy).to(DEV),
            "raw+30": wide.reshape(n_z * B, pts, 2 * dy).to(DEV), "mixed": mixed.reshape(n_z * B, pts, 2 * dy).to(DEV)}


@pytest.mark.parametrize("homosk", (False, True), ids=("hetero", "homosk"))
@pytest.mark.parametrize("dy", (1, 2, 4))
@pytest.mark.parametrize("n_z", (1, 2, 8, 32, 33, 128))
def test_mixture_summary_matches_float64_reference(n_z, dy, homosk):
    from npf_gwwaveform_amd import functional as FN

    B = 3
    for pts in (1, 63, 256, 1000):
        suff = _random_suff(n_z, B, pts, dy, seed=1000 * n_z + 10 * dy + pts)
        tag = f"random n_z={n_z} dy={dy} pts={pts} {'homosk' if homosk else 'hetero'}"
        _check_against_reference(suff, n_z, dy, homosk, None, tag)
        counts = torch.tensor([0, pts, pts // 2], dtype=torch.int32, device=DEV)
        _check_against_reference(suff, n_z, dy, homosk, counts, tag + " counts")
        # NaN beyond the count changes nothing below it, bit for bit; full counts equal the launch without counts
        got = FN.mixture_summary(suff, n_z, dy, homosk, probs=PROBS, n_valid=counts)
        poisoned = suff.clone().view(n_z, B, pts, 2 * dy)
        for b in range(B):
            poisoned[:, b, int(counts[b]):] = float("nan")
        got_nan = FN.mixture_summary(poisoned.view_as(suff), n_z, dy, homosk, probs=PROBS, n_valid=counts)
        full = FN.mixture_summary(suff, n_z, dy, homosk, probs=PROBS, n_valid=torch.full((B,), pts, dtype=torch.int64, device=DEV))
        none = FN.mixture_summary(suff, n_z, dy, homosk, probs=PROBS)
        for a, b_, c, d in zip(got, got_nan, full, none):
            assert torch.equal(a, b_), f"NaN padding {tag}"
            assert torch.equal(c, d), f"full counts {tag}"


@pytest.mark.parametrize("homosk", (False, True), ids=("hetero", "homosk"))
@pytest.mark.parametrize("n_z", (1, 2, 8, 32, 33, 128))
def test_mixture_summary_adversarial_inputs(n_z, homosk):
    B = 3
    for dy, pts in ((1, 63), (2, 256), (4, 63)):
        for family, suff in _adversarial(n_z, B, pts, dy, seed=77 * n_z + dy).items():
            tag = f"{family} n_z={n_z} dy={dy} pts={pts} {'homosk' if homosk else 'hetero'}"
            _check_against_reference(suff, n_z, dy, homosk, None, tag)
            _check_against_reference(suff, n_z, dy, homosk, torch.tensor([pts, 0, 1], dtype=torch.int32, device=DEV), tag + " counts")


# ---- query equals forward --------------------------------------------------------------------------------------------------------
ROUTES = {
    "cnp_r256_c33": _c("CNP", 256, 33),
    "lnp_latent_r256_c33_nz4": _c("LNP", 256, 33, encoded_path="latent", n_z=4),
    "lnp_both_r128_c33_nz4": _c("LNP", 128, 33, encoded_path="both", n_z=4),
    "attncnp_r256_c256": _c("AttnCNP", 256, 256),                      # the fused target side
    "attncnp_r128_c128": _c("AttnCNP", 128, 128),                      # ... of the 128-wide programs
    "attncnp_r256_c128": _c("AttnCNP", 256, 128),                      # the chain
    "attncnp_r256_c257": _c("AttnCNP", 256, 257),                      # the blocked softmax
    "attncnp_r128_c0": _c("AttnCNP", 128, 0),
    "attncnp_r256_multihead_c128": _c("AttnCNP", 256, 128, attention="multihead"),
    "attncnp_r128_transformer_c256": _c("AttnCNP", 128, 256, attention="transformer"),
    "attncnp_r128_transformer_c257": _c("AttnCNP", 128, 257, attention="transformer"),
    "attnlnp_r256_c256_nz1": _c("AttnLNP", 256, 256, n_z=1),         # the fused target side with the latent merge
    "attnlnp_r256_c200_nz8": _c("AttnLNP", 256, 200, n_z=8),
    "attnlnp_r128_transformer_c33_nz1": _c("AttnLNP", 128, 33, attention="transformer", n_z=1),
}
TARGET_SIDE = ("x6.target_side", "x6.decoder_side", "x6.xenc_proj", "functional.mha", "attention_long.long_scaledot_attention")


def _model_and_inputs(case):
    from npf_gwwaveform_amd.neuralproc import MultivariateNormalDiag

    model = build_model(case, DEV, params=specs.make_params(case, seed=11)).eval()
    if hasattr(model, "LatentDistribution"):
        model.LatentDistribution = MultivariateNormalDiag  # (the package's own rsample: the test is about the global RNG stream)
    inp = specs.make_inputs(case, seed=4321)
    return model, inp["X_cntxt"].to(DEV), inp["Y_cntxt"].to(DEV), inp["X_trgt"].to(DEV)


def _counts(B, n, seed, ends):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, n + 1, (B,), generator=g)
    c[0] = ends
    return c.to(DEV)


def _same(p, q, what):
    assert p.batch_shape == q.batch_shape and p.event_shape == q.event_shape, what
    assert torch.equal(p.base_dist.loc, q.base_dist.loc), f"loc differs from forward {what}"
    assert torch.equal(p.base_dist.scale, q.base_dist.scale), f"scale differs from forward {what}"


@pytest.mark.parametrize("counts", ("none", "n_cntxt", "n_cntxt+n_trgt", "n_trgt"))
@pytest.mark.parametrize("name", list(ROUTES))
def test_query_equals_forward_bit_for_bit(name, counts):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    B, C, T = case["B"], case["C"], case["T"]
    kw_c = dict(n_cntxt=_counts(B, C, 5, C)) if "n_cntxt" in counts else {}
    kw_t = dict(n_trgt=_counts(B, T, 6, T // 2)) if "n_trgt" in counts else {}
    latent = case["kind"] in ("LNP", "AttnLNP")

    torch.manual_seed(99)
    with torch.no_grad(), launch_witness(spy=SPY) as wf:
        out = model(Xc, Yc, Xt, **kw_c, **kw_t)
    torch.manual_seed(99)
    with launch_witness(spy=SPY) as wc:
        post = model.condition(Xc, Yc, **kw_c)
    with launch_witness(spy=SPY) as wq:
        p = post.query(Xt, **kw_t)
    _same(p, out[0], name)
    assert not p.base_dist.loc.requires_grad
    if latent:
        assert torch.equal(post.z_samples, out[1]) and post.z_samples.shape[0] == case["n_z"]
        assert torch.equal(post.q_zCc.base_dist.loc, out[2].base_dist.loc) and torch.equal(post.q_zCc.base_dist.scale, out[2].base_dist.scale)
    else:
        assert post.z_samples is None and post.q_zCc is None and out[1] is None
    # the same launches, split in two: every entry point of the library and every side function of the package
    for k in set(wf.calls) | set(wc.calls) | set(wq.calls) | set(SPY):
        assert wf[k] == wc[k] + wq[k], f"{k}: forward {wf[k]}, condition {wc[k]} + query {wq[k]}\n{wf}\n{wc}\n{wq}"
    assert all(wc[k] == 0 for k in TARGET_SIDE), wc          # nothing of the target side runs at conditioning time
    assert wq["x6.context_side"] == 0, wq                      # and the context side is not run again
    if not kw_c:
        e = _expected(case, training=False)
        assert {k: wq[k] for k in TARGET_SIDE} == {k: e[k] for k in TARGET_SIDE}, f"{wq}\nexpected {e}"
        assert wc["x6.context_side"] == e["x6.context_side"], wc
    elif C > 0:
        assert wq["x6.target_side"] == 0, wq                   # (the padded route: masked attention, never the fused target side)
        if case["kind"] in ("AttnCNP", "AttnLNP") and case.get("attention", "scaledot") == "scaledot":
            assert wq["npf_masked_attn_fwd"] + wq["npf_masked_attn_fwd_nq"] == 1, wq
            assert wq["npf_masked_attn_fwd_nq"] == int(bool(kw_t)), wq
    if kw_t:  # the head reads the counts (loc / scale are materialised on demand: one masked launch)
        with launch_witness() as wh:
            post.query(Xt, **kw_t).base_dist
        assert wh["npf_masked_gauss_head_fwd"] == 1 and wh["npf_gauss_head_fwd"] == 0, wh
    # a second query of the same object, after a forward of the model on other sizes in between: same numbers again
    torch.manual_seed(5)
    with torch.no_grad():
        model(Xc[:, : max(C // 2, 0)], Yc[:, : max(C // 2, 0)], Xt[:, :7])
    _same(post.query(Xt, **kw_t), out[0], f"{name} (second query)")
    if counts == "none":  # and against the forward the autograd engine records
        torch.manual_seed(99)
        _same(p, model(Xc, Yc, Xt)[0], f"{name} (forward with autograd)")


def test_predict_is_condition_query_summary_and_respects_n_z_samples():
    case = ROUTES["attnlnp_r256_c200_nz8"]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    torch.manual_seed(3)
    pred = model.predict(Xc, Yc, Xt, n_z_samples=5, probs=(0.1, 0.9))
    torch.manual_seed(3)
    post = model.condition(Xc, Yc, n_z_samples=5)
    assert post.z_samples.shape[0] == 5
    p = post.query(Xt)
    want = p.summary((0.1, 0.9))
    assert pred.probs == (0.1, 0.9) and pred.quantiles.shape == (2, case["B"], case["T"], case["dy"])
    for a, b in zip(pred[:3], want[:3]):
        assert torch.equal(a, b)
    assert p._base is None  # summary() does not materialise loc / scale
    loc, scale = p.base_dist.loc.double(), p.base_dist.scale.double()
    assert_close(pred.mean, loc.mean(0), what="predict mean")
    assert_close(pred.std, (scale ** 2 + (loc - loc.mean(0)) ** 2).mean(0).sqrt(), what="predict std")
    assert (pred.quantiles[1] > pred.quantiles[0]).all()
    model.train()  # the mode decides the default number of samples
    model.n_z_samples_train = 3
    assert model.condition(Xc, Yc).z_samples.shape[0] == 3


# ---- coherence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bitwise", [("lnp_latent_r128", True), ("lnp_both_r128_c33_nz4", True), ("attnlnp_r256_c200_nz8", False),
                                          ("attnlnp_r256_c256_nz1", False)])
def test_grids_of_one_conditioned_model_are_coherent(name, bitwise):
    """Halves and the whole of one grid from one conditioned latent model: the same rows at the fp32 gate; bit for bit for LNP at
    128 features, whose decoder is the chain kernel on whole 32-point tiles at every T (T = 64 here, halves of 32): a point's
    value depends on its tile's program only."""
    case = dict(ROUTES.get(name) or _c("LNP", 128, 33, encoded_path="latent", n_z=4), T=64)
    model, Xc, Yc, Xt = _model_and_inputs(case)
    T = case["T"]
    torch.manual_seed(17)
    post = model.condition(Xc, Yc)
    other = model.condition(Xc, Yc)  # (no reseeding: another draw)
    assert not torch.equal(post.z_samples, other.z_samples)
    whole, first, second = post.query(Xt), post.query(Xt[:, : T // 2].contiguous()), post.query(Xt[:, T // 2:].contiguous())
    for attr in ("loc", "scale"):
        w = getattr(whole.base_dist, attr)
        parts = torch.cat([getattr(first.base_dist, attr), getattr(second.base_dist, attr)], dim=2)
        assert_close(parts, w, what=f"{attr} of the halves {name}")
        if bitwise:
            assert torch.equal(parts, w), f"{attr} of the halves {name}"
    # z_samples is what query uses: the other object answers differently until it is given these samples
    assert not torch.equal(other.query(Xt).base_dist.loc, whole.base_dist.loc)
    other.z_samples = post.z_samples
    assert torch.equal(other.query(Xt).base_dist.loc, whole.base_dist.loc)


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_summary_allocates_less_than_one_sample_tensor():
    import npf_gwwaveform_amd as A

    n_z, B, T, dy = 32, 64, 1024, 2
    p = A.HeadDistribution(_random_suff(n_z, B, T, dy, seed=1), dy, False, n_z, B, T)
    p.summary()  # (warm: the cached z_p)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    s = p.summary()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < n_z * B * T * dy * 4, grown
    # and nothing but the results: mean, std and three quantiles.  The caching allocator hands a request of 1 MiB or more (the
    # quantiles, 1.5 MiB) a cached block up to 1 MiB larger without splitting it, and rounds the small ones to 512 bytes
    assert grown <= 5 * B * T * dy * 4 + (1 << 20) + 3 * 512, grown
    assert p._base is None and s.mean.shape == (B, T, dy) and s.quantiles.shape == (3, B, T, dy)


# ---- one captured query + summary ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_n_cntxt", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True), ("lnp_both_r128_c33_nz4", False)])
def test_query_and_summary_replay_from_one_graph(name, with_n_cntxt):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    B, C, T = case["B"], case["C"], case["T"]
    torch.manual_seed(23)
    post = model.condition(Xc, Yc, **(dict(n_cntxt=_counts(B, C, 5, C)) if with_n_cntxt else {}))
    X_s, n_s = Xt.clone(), torch.full((B,), T, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            post.query(X_s, n_trgt=n_s).summary()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_g = post.query(X_s, n_trgt=n_s).summary()
    g = torch.Generator().manual_seed(8)
    for step in range(3):
        X_new = (torch.rand(B, T, case["dx"], generator=g) * 2 - 1).to(DEV)
        n_new = torch.randint(0, T + 1, (B,), generator=g, dtype=torch.int32).to(DEV)
        X_s.copy_(X_new)
        n_s.copy_(n_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = post.query(X_new, n_trgt=n_new).summary()
        for a, b in zip(s_g[:3], eager[:3]):
            assert torch.equal(a, b), (name, step)
