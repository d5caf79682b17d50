"""Predictive scores on the GPU: ``npf_mixture_score`` (log density, PIT, CRPS of the mixture over the latent samples) against the
float64 reference of tests/score_reference.py (checked on the CPU by tests/test_score_host.py), the padding convention, non-finite
observations, ``want`` subsets and the memory they need, ``HeadDistribution.score`` of deterministic and latent models against their
own ``base_dist``, leave-one-out scores against the float64 oracle, and a captured ``query`` + ``score``.

Gates, per element over the valid rows (score_reference.ratios): log density |d| <= 1e-5 max(1, |ref|); PIT |d| <= 1e-5 and
0 <= pit <= 1; CRPS |d| <= 1e-5 |ref| and crps >= 0.  Every test prints its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import score_reference as R
from test_hip_predict import ROUTES, _components, _counts, _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, PTS = 3, 37
COUNTS = (37, 17, 0)


def _inputs(name, n_z, dy, seed):
    """(suff [n_z * B, PTS, 2 dy], Y [B, PTS, dy]) on the device, every element drawn from the named regime."""
    mu, raw, y = R.regime(name, n_z, B * PTS * dy, seed)
    suff = torch.cat([mu.view(n_z, B, PTS, dy), raw.view(n_z, B, PTS, dy)], -1).view(n_z * B, PTS, 2 * dy).contiguous()
    return suff.to(DEV), y.view(B, PTS, dy).contiguous().to(DEV)


def _reference(suff, Y, n_z, dy, homosk, n_valid):
    mu, sg, live = _components(suff, n_z, dy, homosk, n_valid)  # float64, the head's formulas (rows beyond the count: mu 0, sg 1)
    return R.scores(mu, sg, Y.double()), live


def _check(got, ref, live, what):
    r = R.ratios(got, ref, live)
    print(f"SCORE {what}: error / gate " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    if got[1] is not None:
        assert ((got[1] >= 0) & (got[1] <= 1))[live].all(), f"{what}: PIT outside [0, 1]"
    if got[2] is not None:
        assert (got[2] >= 0)[live].all(), f"{what}: negative CRPS"
    return r


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("homosk", (False, True), ids=("hetero", "homosk"))
@pytest.mark.parametrize("dy", (1, 2, 4))
@pytest.mark.parametrize("n_z", (1, 2, 8, 32, 33, 128))
def test_mixture_score_matches_float64_reference(n_z, dy, homosk):
    from npf_gwwaveform_amd import functional as FN

    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    worst = {}
    for i, name in enumerate(R.REGIMES):
        suff, Y = _inputs(name, n_z, dy, seed=1000 * n_z + 10 * dy + i)
        for nv in (None, counts):
            tag = f"{name} n_z={n_z} dy={dy} {'homosk' if homosk else 'hetero'}{' counts' if nv is not None else ''}"
            got = FN.mixture_score(suff, Y, n_z, dy, homosk, n_valid=nv)
            ref, live = _reference(suff, Y, n_z, dy, homosk, nv)
            assert all(torch.isfinite(t[live]).all() for t in ref) and (not live.any() or float(ref[2][live].min()) > 0), tag
            for k, v in _check(got, ref, live, tag).items():
                worst[k] = max(worst.get(k, 0.0), v)
            dead = ~live
            assert (got[0][dead] == 0).all() and (got[1][dead] == 0.5).all() and (got[2][dead] == 0).all(), f"padding {tag}"
    print(f"SCORE worst over the regimes, n_z={n_z} dy={dy} {'homosk' if homosk else 'hetero'}: " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("homosk", (False, True), ids=("hetero", "homosk"))
@pytest.mark.parametrize("n_z", (1, 8, 32, 33, 128))
def test_padding_is_never_read_and_holds_the_neutral_values(n_z, homosk):
    from npf_gwwaveform_amd import functional as FN

    dy = 2
    suff, Y = _inputs("random", n_z, dy, seed=7 + n_z)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    got = FN.mixture_score(suff, Y, n_z, dy, homosk, n_valid=counts)
    bad_s, bad_y = suff.clone().view(n_z, B, PTS, 2 * dy), Y.clone()
    for b, n in enumerate(COUNTS):
        bad_s[:, b, n:] = float("nan")
        bad_y[b, n:] = float("nan")
    poisoned = FN.mixture_score(bad_s.view_as(suff), bad_y, n_z, dy, homosk, n_valid=counts)
    for a, p, neutral in zip(got, poisoned, (0.0, 0.5, 0.0)):
        assert torch.equal(a, p), "NaN beyond the counts changed a result"
        for b, n in enumerate(COUNTS):
            assert (a[b, n:] == neutral).all() and torch.isfinite(a[b, :n]).all()
    full = FN.mixture_score(suff, Y, n_z, dy, homosk, n_valid=torch.full((B,), PTS, dtype=torch.int64, device=DEV))
    for a, c in zip(full, FN.mixture_score(suff, Y, n_z, dy, homosk)):
        assert torch.equal(a, c), "full counts differ from the launch without counts"


@pytest.mark.parametrize("homosk", (False, True), ids=("hetero", "homosk"))
@pytest.mark.parametrize("n_z", (1, 8, 33))
def test_a_non_finite_observation_changes_its_own_element_only(n_z, homosk):
    from npf_gwwaveform_amd import functional as FN

    dy = 2
    suff, Y = _inputs("random", n_z, dy, seed=70 + n_z)
    clean = FN.mixture_score(suff, Y, n_z, dy, homosk)
    Yb = Y.clone()
    Yb[0, 5, 1], Yb[2, 36, 0] = float("nan"), float("inf")
    hit = torch.zeros_like(Y, dtype=torch.bool)
    hit[0, 5, 1] = hit[2, 36, 0] = True
    got = FN.mixture_score(suff, Yb, n_z, dy, homosk)
    for a, c in zip(got, clean):
        assert torch.equal(a[~hit], c[~hit])
    assert all(torch.isnan(a[0, 5, 1]) for a in got)
    assert got[0][2, 36, 0] == -math.inf and got[1][2, 36, 0] == 1.0 and got[2][2, 36, 0] == math.inf


# ---- want ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_z", (2, 32, 33))
def test_want_subsets_equal_the_full_call_bit_for_bit(n_z):
    import npf_gwwaveform_amd as A

    dy = 2
    suff, Y = _inputs("random", n_z, dy, seed=3 + n_z)
    p = A.HeadDistribution(suff, dy, False, n_z, B, PTS, n_trgt=torch.tensor(COUNTS, dtype=torch.int32, device=DEV))
    full = p.score(Y)
    assert isinstance(full, A.Score) and all(t.shape == (B, PTS, dy) for t in full)
    for want in (("log_density",), ("pit",), ("crps",), ("crps", "log_density"), ["pit", "crps"]):
        s = p.score(Y, want=want)
        for name in A.Score._fields:
            if name in want:
                assert torch.equal(getattr(s, name), getattr(full, name)), (want, name)
            else:
                assert getattr(s, name) is None, (want, name)
    assert p._base is None


def test_log_density_allocates_less_than_one_sample_tensor():
    import npf_gwwaveform_amd as A

    n_z, Bn, T, dy = 32, 64, 1024, 2
    g = torch.Generator().manual_seed(1)
    p = A.HeadDistribution(torch.randn(n_z * Bn, T, 2 * dy, generator=g).to(DEV), dy, False, n_z, Bn, T)
    Y = torch.randn(Bn, T, dy, generator=g).to(DEV)
    p.score(Y, want=("log_density",))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    s = p.score(Y, want=("log_density",))
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < n_z * Bn * T * dy * 4, grown
    assert grown <= Bn * T * dy * 4 + (1 << 20) + 512, grown  # nothing but the result (and what the caching allocator rounds it to)
    assert p._base is None and s.log_density.shape == (Bn, T, dy) and s.pit is None and s.crps is None


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _gauss_crps(loc, scale, Y):
    u = (Y.double() - loc.double()) / scale.double()
    n = torch.distributions.Normal(0.0, 1.0)
    return scale.double() * (u * torch.erf(u / math.sqrt(2.0)) + 2.0 * torch.exp(n.log_prob(u)) - 1.0 / math.sqrt(math.pi))


def _targets(case, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(case["B"], case["T"], case["dy"], generator=g).to(DEV)


@pytest.mark.parametrize("with_n_trgt", (False, True), ids=("full", "n_trgt"))
@pytest.mark.parametrize("name", ("cnp_r256_c33", "attncnp_r128_c128", "attnlnp_r256_c256_nz1"))
def test_one_gaussian_equals_base_dist(name, with_n_trgt):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Y = _targets(case, 31)
    Bn, T = case["B"], case["T"]
    n_trgt = _counts(Bn, T, 6, T // 2) if with_n_trgt else None
    torch.manual_seed(9)
    with torch.no_grad():
        p = model(Xc, Yc, Xt, **(dict(n_trgt=n_trgt) if with_n_trgt else {}))[0]
    s = p.score(Y)
    assert p._base is None and p.batch_shape[0] == 1
    base = p.base_dist
    live = (torch.arange(T, device=DEV).view(1, T) < (n_trgt if with_n_trgt else torch.full((Bn,), T, device=DEV)).view(Bn, 1))
    live = live.view(Bn, T, 1).expand(Bn, T, case["dy"])
    ref = (base.log_prob(Y.unsqueeze(0))[0], base.cdf(Y.unsqueeze(0))[0], _gauss_crps(base.loc[0], base.scale[0], Y))
    _check(s, ref, live, f"{name} {'n_trgt' if with_n_trgt else 'full'} against base_dist")
    # the joint log density of a point of a deterministic model is the sum over the output dimensions
    joint = p.log_prob(Y.unsqueeze(0))[0]
    assert torch.allclose(s.log_density.sum(-1)[live[..., 0]], joint[live[..., 0]], rtol=1e-5, atol=1e-5 * case["dy"])


@pytest.mark.parametrize("with_n_trgt", (False, True), ids=("full", "n_trgt"))
@pytest.mark.parametrize("name", ("attnlnp_r256_c200_nz8", "lnp_both_r128_c33_nz4"))
def test_latent_models_equal_the_float64_mixture_of_base_dist(name, with_n_trgt):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Y = _targets(case, 32)
    Bn, T = case["B"], case["T"]
    n_trgt = _counts(Bn, T, 6, T // 2) if with_n_trgt else None
    torch.manual_seed(9)
    post = model.condition(Xc, Yc)
    p = post.query(Xt, n_trgt=n_trgt)
    s = p.score(Y)
    assert p._base is None and p.batch_shape[0] == case["n_z"]
    ref = R.scores(p.base_dist.loc.double(), p.base_dist.scale.double(), Y.double())
    live = (torch.arange(T, device=DEV).view(1, T) < (n_trgt if with_n_trgt else torch.full((Bn,), T, device=DEV)).view(Bn, 1))
    live = live.view(Bn, T, 1).expand(Bn, T, case["dy"])
    _check(s, ref, live, f"{name} {'n_trgt' if with_n_trgt else 'full'} against the mixture of base_dist")
    dead = ~live
    assert (s.log_density[dead] == 0).all() and (s.pit[dead] == 0.5).all() and (s.crps[dead] == 0).all()


@pytest.mark.parametrize("name", ("cnp_r128", "attncnp_r128"))
def test_leave_one_out_scores_match_the_oracle_on_the_cut_contexts(name):
    """``model.loo(Xc, Yc, n_cntxt).score(Yc)`` against the scores of the float64 oracle's leave-one-out Gaussians (tests/test_hip_loo.py).
    The predictions themselves meet the oracle at the project's gate only (loc, scale: 1e-5 of max|ref|), so the scores are gated as
    that file gates the log density of the same predictions: max|d| <= 2e-5 max|ref| (PIT: max|ref| = 1).  Rows beyond the context
    counts hold the neutral values."""
    from test_hip_loo import COUNTS as LOO_COUNTS
    from test_hip_loo import _i32, _setup

    s = _setup(name)
    p = s["model"].loo(s["Xc"], s["Yc"], n_cntxt=_i32(LOO_COUNTS))
    sc = p.score(s["Yc"])
    loc, scale = s["ref"]
    ref = R.scores(loc.unsqueeze(0), scale.unsqueeze(0), s["Yc"].cpu().double())
    for what, got, want, neutral in zip(sc._fields, sc, ref, (0.0, 0.5, 0.0)):
        got, want = got.cpu().clone(), want.clone()
        for b, n in enumerate(LOO_COUNTS):
            assert (got[b, n:] == neutral).all(), f"{name} {what}: rows beyond the count"
            got[b, n:] = 0
            want[b, n:] = 0
        err, scale_ = float((got.double() - want).abs().max()), max(float(want.abs().max()), 1.0 if what == "pit" else 0.0)
        print(f"SCORE loo {name} {what}: max|d| = {err:.3e}, max|ref| = {scale_:.3e}, error / gate {err / (2e-5 * scale_):.3f}")
        assert err <= 2e-5 * scale_, f"{name} {what}"


# ---- one captured query + score ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_n_cntxt", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True)])
def test_query_and_score_replay_from_one_graph(name, with_n_cntxt):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, C, T = case["B"], case["C"], case["T"]
    torch.manual_seed(23)
    post = model.condition(Xc, Yc, **(dict(n_cntxt=_counts(Bn, C, 5, C)) if with_n_cntxt else {}))
    X_s, Y_s, n_s = Xt.clone(), _targets(case, 1), torch.full((Bn,), T, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            post.query(X_s, n_trgt=n_s).score(Y_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_g = post.query(X_s, n_trgt=n_s).score(Y_s)
    g = torch.Generator().manual_seed(8)
    for step in range(3):
        X_new = (torch.rand(Bn, T, case["dx"], generator=g) * 2 - 1).to(DEV)
        Y_new = torch.randn(Bn, T, case["dy"], generator=g).to(DEV)
        n_new = torch.randint(0, T + 1, (Bn,), generator=g, dtype=torch.int32).to(DEV)
        X_s.copy_(X_new)
        Y_s.copy_(Y_new)
        n_s.copy_(n_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = post.query(X_new, n_trgt=n_new).score(Y_new)
        for a, b in zip(s_g, eager):
            assert torch.equal(a, b), (name, step)
