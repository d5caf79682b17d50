"""Sky and distance marginalised jointly on the GPU: ``npf_waveform_loglike_sky_dist`` against the float64 reference of
tests/loglike_sky_dist_reference.py (checked on the CPU by tests/test_loglike_sky_dist_host.py, which also holds the condition that
every set here leaves the indices well posed): one sweep per axis from a base case (rows 1 / 16 / 17 / 33, pixels 1 .. 65 -- the
second correlation workgroup --, grid times around the chunk of 8, scales around the chunk of 8 and 65, points, detectors, latent
samples); the regimes quiet, loud (w near 1e6) and HH == 0; dead pixels (bit for bit against the cut call) and dead scales (within the
gates) with NaN in what must not be read; the two parents as special cases; a pixel permutation; NaN isolation; output subsets; a dirty
workspace; one captured graph; the four models.

Gates: loglike_sky_dist_reference.ratios, unchanged."""
import math

import pytest
import torch

import loglike_sky_dist_reference as J
import loglike_sky_reference as S
from test_hip_dispatch import _c
from test_hip_predict import _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {"cnp": _c("CNP", 64, 20, B=3, T=37), "attncnp": _c("AttnCNP", 64, 20, B=3, T=37),
          "lnp": _c("LNP", 64, 20, encoded_path="latent", n_z=3, B=3, T=37), "attnlnp": _c("AttnLNP", 64, 20, n_z=3, B=3, T=37)}
ALL = dict(posterior=True, joint=True, moments=True)


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _call(case, **kw):
    from npf_gwwaveform_amd import functional as FN

    return FN.waveform_loglike_sky_distance(**_dev(J.call_args(case)), **dict(ALL, **kw))


def _as_dict(m):
    return {k: (v.cpu() if v is not None else None) for k, v in m._asdict().items()}


def _check(got, ref, what, worst=None):
    r = J.ratios(got, ref)
    print(f"LOGLIKE_SKY_DIST {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    if worst is not None:
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)


def _same_bits(a, b, what):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (what, name)


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ("rows", "P", "n_tau", "n_a", "T", "D", "n_z"))
def test_axis_sweep_meets_the_reference(axis):
    worst, n = {}, 0
    for ax, tag, case in J.sweep_sets():
        if ax != axis:
            continue
        got = _as_dict(_call(case))
        Rn, Bn, P, n_a = case["h"].shape[0], case["data"].shape[0], case["response"].shape[0], case["scales"].shape[0]
        assert got["lnl_vol"].shape == (Rn,) and got["lnl"].shape == (Bn,) and got["post_joint"].shape == (Rn, P, n_a), tag
        assert got["post_sky"].shape == got["dist_mean"].shape == got["dist_std"].shape == (Rn, P), tag
        assert got["post_dist"].shape == (Rn, n_a) and got["post_sky_mix"].shape == (Bn, P) and got["post_dist_mix"].shape == (Bn, n_a)
        _check(got, J.cached(tag, case), tag, worst)
        n += 1
    print(f"LOGLIKE_SKY_DIST worst over the {n} sets of axis {axis}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_regimes_quiet_to_loud_and_posteriors_that_sum_to_one():
    case = J.regime_set()
    ref = J.cached("regimes", case)
    got = _as_dict(_call(case))
    _check(got, ref, "regimes")
    assert float(ref["w"].max()) > 9e5
    # the differences are formed before the logs: every posterior sums to one to rounding (n terms, each exp within a few ulp),
    # also where w ~ 1e6 and an ulp of w is 1e-10
    P, n_a = case["response"].shape[0], case["scales"].shape[0]
    for name, dims in (("post_sky", (1,)), ("post_dist", (1,)), ("post_joint", (1, 2))):
        total = got[name].exp().sum(dims)
        print(f"LOGLIKE_SKY_DIST regimes: |sum exp({name}) - 1| max {float((total - 1).abs().max()):.3g}")
        assert ((total - 1).abs() <= 16 * P * n_a * 2.0 ** -53).all(), name


def test_rows_without_power_take_the_priors():
    case = J.degenerate_set()
    got = _as_dict(_call(case))
    _check(got, J.cached("HH == 0 rows", case), "HH == 0 rows")
    lp, lpi = case["log_prior"], case["log_prior_scale"]
    for r in (1, 5):
        w = got["post_joint"][r] + got["lnl_vol"][r]
        assert ((w - (lp.view(-1, 1) + lpi.view(1, -1))).abs() <= 1e-12).all()
        assert got["snr"][r] == 0 and got["scale_hat"][r] == 0 and got["tau_index"][r] == 0


def test_dead_pixels_match_the_cut_call_bit_for_bit():
    from npf_gwwaveform_amd import functional as FN

    case = J.base_set()
    dead = torch.tensor([1, 4])
    for i, v in zip(dead, (-math.inf, math.nan)):
        case["log_prior"][i] = v
    case["response"][dead] = math.nan  # (what must not be read)
    case["delays"][dead] = math.nan
    got = _call(case)
    keep = torch.tensor([p for p in range(7) if p not in dead.tolist()])
    cut = dict(case, response=case["response"][keep], delays=case["delays"][keep], log_prior=case["log_prior"][keep])
    small = _call(cut)
    k = keep.to(DEV)
    for name in ("lnl_vol", "scale_index", "tau_index", "snr", "scale_hat", "lnl", "post_dist", "post_dist_mix"):
        assert torch.equal(getattr(got, name), getattr(small, name)), name
    assert torch.equal(k[small.pix_index.long()].int(), got.pix_index)
    for name in ("post_sky", "dist_mean", "dist_std", "post_sky_mix"):
        assert torch.equal(getattr(got, name)[:, k], getattr(small, name)), name
        assert (getattr(got, name)[:, dead.to(DEV)] == (0.0 if name.startswith("dist") else -math.inf)).all(), name
    assert torch.equal(got.post_joint[:, k], small.post_joint) and (got.post_joint[:, dead.to(DEV)] == -math.inf).all()
    _check(_as_dict(got), J.reference(**J.call_args(case)), "dead pixels")
    # no live pixel at all
    case["log_prior"][:] = math.inf
    none = _as_dict(_call(case))
    assert (none["lnl_vol"] == -math.inf).all() and (none["lnl"] == -math.inf).all() and (none["post_joint"] == -math.inf).all()
    assert all((none[k] == 0).all() for k in ("pix_index", "scale_index", "tau_index", "snr", "scale_hat", "dist_mean", "dist_std"))
    assert FN.SKYD_SC == J.SC


def test_dead_scales_match_the_cut_call_within_the_gates():
    case = J.base_set(13, "dead")  # scales 0, -1, NaN, inf and priors -inf, inf, NaN, NaN in the other tensor of each
    ref = J.cached("dead scales", case)
    got = _as_dict(_call(case))
    _check(got, ref, "dead scales")
    live = ref["live_i"]
    assert int(live.sum()) == 6
    cut = dict(case, scales=case["scales"][live], log_prior_scale=case["log_prior_scale"][live])
    ref_cut = J.reference(**J.call_args(cut), sky=ref["sky"])
    small = _as_dict(_call(cut))
    _check(small, ref_cut, "dead scales cut")
    idx = torch.nonzero(live)[:, 0]
    full_as_cut = dict(got, scale_index=torch.searchsorted(idx, got["scale_index"].long()).int(), post_dist=got["post_dist"][:, live],
                       post_dist_mix=got["post_dist_mix"][:, live], post_joint=got["post_joint"][:, :, live])
    _check(full_as_cut, ref_cut, "dead scales against the cut reference")
    assert (got["post_dist"][:, ~live] == -math.inf).all() and (got["post_joint"][:, :, ~live] == -math.inf).all()
    # no live scale at all
    case["scales"][:] = 0.0
    none = _as_dict(_call(case))
    assert (none["lnl_vol"] == -math.inf).all() and (none["post_sky"] == -math.inf).all() and (none["post_dist_mix"] == -math.inf).all()
    assert all((none[k] == 0).all() for k in ("pix_index", "scale_index", "tau_index", "snr", "scale_hat", "dist_mean", "dist_std"))


# ---- the parents as special cases ---------------------------------------------------------------------------------------------------
def test_one_scale_of_one_is_loglike_sky():
    from npf_gwwaveform_amd import functional as FN

    case = J.base_set()
    a = _dev(J.call_args(case))
    a["scales"], a["log_prior_scale"] = torch.ones(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    got = FN.waveform_loglike_sky_distance(**a, **ALL)
    sky_args = {k: v for k, v in a.items() if k not in ("scales", "log_prior_scale")}
    sky = FN.waveform_loglike_sky(**sky_args, posterior=True)
    ref = S.reference(**S.call_args(case))
    mine = dict(lnl_sky=got.lnl_vol, pix_index=got.pix_index, tau_index=got.tau_index, snr=got.snr, lnl_sky_mix=got.lnl, post=got.post_sky,
                post_mix=got.post_sky_mix)
    r = S.ratios({k: v.cpu() for k, v in mine.items()}, ref)
    print("LOGLIKE_SKY_DIST n_a=1 as loglike_sky: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0
    gate = (1e-10 * ref["scale"] + 1e-12).to(DEV)
    assert ((got.lnl_vol - sky.lnl_sky).abs() <= 2 * gate).all() and ((got.post_sky - sky.post).abs() <= 4 * gate.view(-1, 1)).all()
    assert torch.equal(got.pix_index, sky.pix_index) and torch.equal(got.tau_index, sky.tau_index) and torch.equal(got.snr, sky.snr)
    assert (got.dist_mean == 1).all() and (got.dist_std == 0).all() and (got.post_dist == 0).all()


def test_one_pixel_is_loglike_network_distance():
    from npf_gwwaveform_amd import functional as FN

    case = J.build(seed=310, **dict(J.BASE, P=1, n_a=9))
    a = _dev(J.call_args(case))
    a["log_prior"] = torch.zeros(1, dtype=torch.float64, device=DEV)
    got = FN.waveform_loglike_sky_distance(**a, **ALL)
    Bn = a["data"].shape[0]
    net = FN.waveform_loglike_network_distance(a["h"], a["data"], a["response"].expand(Bn, -1, -1).contiguous(),
                                               a["delays"].expand(Bn, -1).contiguous(), a["scales"], a["log_prior_scale"], a["weights"],
                                               a["freqs"], a["taus"], posterior=True)
    ref = J.reference(**dict(J.call_args(case), log_prior=torch.zeros(1, dtype=torch.float64)))
    g = (1e-10 * ref["S"] + 1e-12).to(DEV)
    g_task = g.view(-1, Bn).max(0).values
    q = {"lnl_vol": float(((got.lnl_vol - net.lnl_dist).abs() / (2 * g)).max()),
         "post_dist": float(((got.post_dist - net.post).abs() / (4 * g.view(-1, 1))).max()),
         "lnl": float(((got.lnl - net.lnl_dist_mix).abs() / (2 * g_task)).max()),
         "post_dist_mix": float(((got.post_dist_mix - net.post_mix).abs() / (4 * g_task.view(-1, 1))).max()),
         "scale_hat": float(((got.scale_hat - net.scale_hat).abs() / (2e-10 * net.scale_hat.abs() + 2e-12)).max())}
    print("LOGLIKE_SKY_DIST P=1 against waveform_loglike_network_distance: difference / both gates " +
          ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    assert max(q.values()) <= 1.0 and torch.equal(got.scale_index, net.scale_index) and torch.equal(got.tau_index, net.base.tau_index)
    assert (got.pix_index == 0).all() and (got.post_sky == 0).all()


# ---- order, isolation, subsets, repeats ---------------------------------------------------------------------------------------------
def test_a_pixel_permutation_permutes_the_maps_and_leaves_the_marginals():
    case = J.perm_set()
    ref = J.cached("permutations", case)
    first = _call(case)
    _check(_as_dict(first), ref, "permutations")
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(5))
    moved = dict(case, response=case["response"][perm], delays=case["delays"][perm], log_prior=case["log_prior"][perm])
    m = _call(moved)
    pd = perm.to(DEV)
    for name in ("post_sky", "dist_mean", "dist_std", "post_sky_mix"):
        assert torch.equal(getattr(m, name), getattr(first, name)[:, pd]), name
    assert torch.equal(m.post_joint, first.post_joint[:, pd])
    assert torch.equal(m.lnl_vol, first.lnl_vol) and torch.equal(m.lnl, first.lnl)
    assert torch.equal(pd[m.pix_index.long()].int(), first.pix_index) and torch.equal(m.scale_index, first.scale_index)
    g = (2.0 * (1e-10 * ref["S"] + 1e-12)).view(-1, 1).to(DEV)
    assert ((m.post_dist - first.post_dist).abs() <= g).all()


def test_a_nan_pixel_poisons_the_marginals_and_leaves_the_other_columns():
    case = J.base_set()
    clean = _call(case)
    case["response"][4, 1, 0] = math.nan
    m = _call(case)
    assert torch.isnan(m.lnl_vol).all() and torch.isnan(m.lnl).all() and torch.isnan(m.post_dist).all()
    others = torch.tensor([0, 1, 2, 3, 5, 6], device=DEV)
    for name in ("dist_mean", "dist_std"):
        assert torch.equal(getattr(m, name)[:, others], getattr(clean, name)[:, others]), name
        assert torch.isnan(getattr(m, name)[:, 4]).all(), name
    # a NaN at a live point of one row stays in its row and its task's mixtures
    case = J.base_set()
    case["h"][4, 3, 0] = math.nan
    m = _call(case)
    assert torch.isnan(m.lnl_vol[4]) and torch.isnan(m.lnl[1])
    rows = torch.tensor([0, 1, 2, 3, 5, 6, 7, 8], device=DEV)
    for name in ("lnl_vol", "pix_index", "scale_index", "tau_index", "snr", "scale_hat", "post_sky", "post_dist", "post_joint",
                 "dist_mean", "dist_std"):
        assert torch.equal(getattr(m, name)[rows], getattr(clean, name)[rows]), name
    assert torch.equal(m.lnl[[0, 2]], clean.lnl[[0, 2]]) and torch.equal(m.post_sky_mix[[0, 2]], clean.post_sky_mix[[0, 2]])


def test_subsets_of_the_outputs_and_a_dirty_workspace_give_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    case = J.base_set()
    args = _dev(J.call_args(case))
    full = FN.waveform_loglike_sky_distance(**args, **ALL)
    for want, post, joint, mom in ((("lnl",), False, False, False), ((), True, False, False), ((), False, True, False),
                                   ((), False, False, True), (["pix_index", "scale_hat"], False, False, True)):
        m = FN.waveform_loglike_sky_distance(**args, want=want, posterior=post, joint=joint, moments=mom)
        for name in m._fields:
            asked = name in want or (post and name.startswith("post_") and name != "post_joint") or (joint and name == "post_joint") or \
                (mom and name.startswith("dist_"))
            assert (getattr(m, name) is not None) == asked, (want, name)
            assert not asked or torch.equal(getattr(m, name), getattr(full, name)), (want, name)
    with pytest.raises(ValueError, match="at least one"):
        FN.waveform_loglike_sky_distance(**args, want=())
    # a larger call dirties the shared workspace; the same call again gives the same bits
    _call(J.perm_set())
    again = FN.waveform_loglike_sky_distance(**args, **ALL)
    _same_bits(full, again, "dirty workspace")
    for name, kw in (("scales", dict(scales=args["scales"].cpu())), ("log_prior_scale", dict(log_prior_scale=args["log_prior_scale"].cpu()))):
        with pytest.raises(ValueError, match="must live on the device"):
            FN.waveform_loglike_sky_distance(**dict(args, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FN.waveform_loglike_sky_distance(**dict(args, h=args["h"].cpu()))


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _predict(name):
    case = MODELS[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    torch.manual_seed(9)
    post = model.condition(Xc, Yc)
    return case, post, Xt, post.query(Xt)


def _observation(loc, P, seed, n_tau, n_a, D=3):
    """A sky grid, a scale grid and the data (times DATA_SCALE) of a signal planted with the waveforms ``loc`` [B, T, 2] at pixel P // 2."""
    import loglike_dist_reference as DR

    g = torch.Generator().manual_seed(seed)
    Bn, T = loc.shape[:2]
    resp, dl = S.sky(P, D, g)
    f, taus = torch.linspace(20.0, 512.0, T), S.grid(n_tau)
    data = S.plant(loc, resp[P // 2], dl[P // 2], f, taus[0] + 3 * taus[1]) + 0.02 * torch.randn(Bn, D, T, 2, generator=g, dtype=torch.float64)
    mass = 0.2 + torch.rand(P, generator=g, dtype=torch.float64)
    w = 0.5 + torch.rand(Bn, D, T, generator=g)
    a = DR.geometric(n_a)
    return dict(data=(J.DATA_SCALE * data).float(), response=resp, delays=dl, scales=a, log_prior_scale=DR.volume_prior(a),
                log_prior=torch.log(mass / mass.sum()), weights=w, freqs=f, taus=taus)


def _flat(m):
    d = {k: v for k, v in m._asdict().items() if v is not None and k not in ("tau", "scale_map")}
    per_task = ("lnl", "post_sky_mix", "post_dist_mix")
    tail = {"post_sky": 1, "post_dist": 1, "dist_mean": 1, "dist_std": 1, "post_joint": 2}
    return {k: (v if k in per_task else v.reshape(-1, *v.shape[v.dim() - tail.get(k, 0):])) for k, v in d.items()}


@pytest.mark.parametrize("name", list(MODELS))
def test_models_loglike_sky_distance_is_the_functional_call_and_meets_the_reference(name):
    import npf_gwwaveform_amd as A

    FN = A.functional
    case, post, Xt, p = _predict(name)
    Bn, T, n_z, P, n_a = case["B"], case["T"], case.get("n_z", 1), 19, 9
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2).cpu()
    obs = _observation(loc[:Bn], P, 41, FN.SKY_JC + 1, n_a)
    o = _dev(obs)
    m = p.loglike_sky_distance(joint=True, **o)
    plain = p.loglike_sky_distance(o["data"], o["response"], o["delays"], o["scales"], o["log_prior_scale"], freqs=o["freqs"],
                                   posterior=False, moments=False)
    mean = p.loglike_sky_distance(of="mean", **o)
    assert isinstance(m, A.SkyDistanceLogLike)
    lead = (n_z, Bn)
    assert all(getattr(m, k).shape == lead for k in ("lnl_vol", "pix_index", "scale_index", "scale_map", "tau_index", "tau", "snr",
                                                     "scale_hat")) and m.lnl.shape == (Bn,)
    assert m.post_sky.shape == m.dist_mean.shape == m.dist_std.shape == (*lead, P) and m.post_dist.shape == (*lead, n_a)
    assert m.post_joint.shape == (*lead, P, n_a) and m.post_sky_mix.shape == (Bn, P) and m.post_dist_mix.shape == (Bn, n_a)
    assert all(getattr(m, k).dtype == torch.int32 for k in ("pix_index", "scale_index", "tau_index"))
    assert torch.equal(m.scale_map, o["scales"][m.scale_index.long()])
    assert all(getattr(plain, k) is None for k in ("tau", "tau_index", "post_sky", "post_dist", "post_joint", "dist_mean", "dist_std"))
    assert mean.lnl_vol.shape == (1, Bn) and mean.post_sky.shape == (1, Bn, P) and mean.post_joint is None
    fn = FN.waveform_loglike_sky_distance(p._suff.reshape(n_z * Bn, T, 4), n_valid=None, **o, **ALL)
    for k in fn._fields:
        assert torch.equal(getattr(m, k).reshape(-1), getattr(fn, k).reshape(-1)), k
    ref = J.reference(loc, **obs)
    lead_sky, lead_dist, lead_x = J.margins(ref)
    assert lead_sky >= 1e3 and lead_dist >= 1e3 and lead_x >= 1e-6, f"{name}: the inputs leave the indices ill posed"
    _check(_flat(m), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().view(-1), obs["taus"][0] + ref["tau_index"].double() * obs["taus"][1]), name
    ref_mean = J.reference(p.summary().mean.double().cpu(), **obs)
    _check(_flat(mean), ref_mean, f"{name} of=mean against summary().mean")
    if n_z == 1:
        assert torch.equal(m.lnl, m.lnl_vol[0]), name
    with pytest.raises(ValueError, match="of must be"):
        p.loglike_sky_distance(o["data"], o["response"], o["delays"], o["scales"], o["log_prior_scale"], freqs=o["freqs"], of="median")


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    one = torch.ones(4, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike_sky_distance(torch.zeros(3, 2, 37, 2, device=DEV), torch.ones(5, 2, 2, dtype=torch.float64, device=DEV),
                               torch.zeros(5, 2, dtype=torch.float64, device=DEV), one, one, freqs=torch.ones(37, device=DEV))


def test_query_and_loglike_sky_distance_replay_from_one_graph_after_the_grids_are_overwritten():
    """response, delays, both priors and scales are overwritten in place; both replays are bit-equal to the eager call on the new
    values: the host reads none of them."""
    from npf_gwwaveform_amd import functional as FN

    case, post, Xt, p = _predict("attnlnp")
    Bn, T, n_z, P, n_a = case["B"], case["T"], case.get("n_z", 1), 19, 9
    loc0 = p.base_dist.loc.double().reshape(n_z * Bn, T, 2).cpu()[:Bn]
    o = _dev(_observation(loc0, P, 1, FN.SKY_JC + 1, n_a))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # (at the sizes, before capturing: the workspace is allocated here)
            post.query(Xt).loglike_sky_distance(joint=True, **o)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branches)
        m_g = post.query(Xt).loglike_sky_distance(joint=True, **o)
    new = _dev(_observation(loc0, P, 100, FN.SKY_JC + 1, n_a))
    new["log_prior"][5] = -math.inf  # (a dead pixel)
    new["scales"] = new["scales"] * 1.07
    new["scales"][2] = math.nan      # (and a dead scale)
    new["log_prior_scale"] = new["log_prior_scale"] + 0.25
    for k in ("response", "delays", "log_prior", "scales", "log_prior_scale"):
        o[k].copy_(new[k])
    eager = post.query(Xt).loglike_sky_distance(joint=True, **dict(o, **{k: new[k] for k in ("response", "delays", "log_prior", "scales",
                                                                                                 "log_prior_scale")}))
    for step in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(m_g._fields, m_g, eager):
            assert torch.equal(a, b), (step, name)
    assert (m_g.post_sky[..., 5] == -math.inf).all() and (m_g.post_dist[..., 2] == -math.inf).all()
    assert torch.isfinite(m_g.lnl_vol).all()
