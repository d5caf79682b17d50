"""Sky-grid network likelihood on the GPU: ``npf_waveform_loglike_sky`` against the float64 reference of
tests/loglike_sky_reference.py (checked on the CPU by tests/test_loglike_sky_host.py): one sweep per axis (rows, pixels, detectors,
points, grid times) across the tile, chunk, k-step and padding edges; ``ln I0`` on both sides of its switch point in one call; dead
points, dead pixels, a pixel without response, a zero template; NaN isolation between rows; bit-identical repeats, permutations and
copies; P = 1 against ``waveform_loglike_network``; ``HeadDistribution.loglike_sky`` of a deterministic and a latent model and one
captured ``query`` + ``loglike_sky`` replayed after the sky grid was overwritten in place; the refusals.

Gates (loglike_sky_reference.ratios): lnl_sky, lnl_sky_mix and u = post + lnl_sky |d| <= 1e-10 scale + 1e-12, scale = max_p
(sqrt(HH_p DD) + HH_p / 2); post, post_mix twice that; snr, snr_map 1e-10 relative + 1e-12; the indices exact; -inf by -inf only.
Every test prints its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import loglike_sky_reference as S
from test_hip_predict import ROUTES, _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = [("cnp_r256_c33", False), ("attnlnp_r256_c200_nz8", True)]


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _call(case, **kw):
    from npf_gwwaveform_amd import functional as FN

    return FN.waveform_loglike_sky(**_dev(S.call_args(case)), posterior=True, snr_map=True, **kw)


def _as_dict(m):
    return {k: (v.cpu() if v is not None else None) for k, v in m._asdict().items()}


def _check(got, ref, what, worst=None):
    r = S.ratios(got, ref)
    print(f"LOGLIKE_SKY {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    if worst is not None:
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return r


def _same_bits(a, b, what):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (what, name)


def _clone(case):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def _ref(case):
    return S.reference(**S.call_args(case))


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ("rows", "P", "D", "T", "n_tau", "combined"))
def test_axis_sweeps_meet_the_float64_reference(axis):
    """Every set of the axis: the gates on every output, the shapes and dtypes, only finite values, the planted pixel and time."""
    from npf_gwwaveform_amd import functional as FN

    worst, n = {}, 0
    for tag, case in S.sweep_sets(FN.SKY_JC):
        if not tag.startswith(axis):
            continue
        n += 1
        m = _call(case)
        got = _as_dict(m)
        Rn, Bn, P = case["h"].shape[0], case["data"].shape[0], case["response"].shape[0]
        assert all(v.dtype == (torch.int32 if k.endswith("index") else torch.float64) for k, v in got.items()), tag
        assert all(got[k].shape == (Rn,) for k in ("lnl_sky", "pix_index", "tau_index", "snr")) and got["lnl_sky_mix"].shape == (Bn,), tag
        assert got["post"].shape == (Rn, P) and got["snr_map"].shape == (Rn, P) and got["post_mix"].shape == (Bn, P), tag
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        _check(got, _ref(case), tag, worst)
        assert (got["pix_index"] == case["p0"]).all() and (got["tau_index"] == case["j0"]).all(), tag
    assert n >= 1
    print(f"LOGLIKE_SKY worst over the {n} sets of axis {axis}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_ln_i0_on_both_sides_of_its_switch_point_in_one_call():
    """Four tasks whose data scales put x at 0.1 and 20 (below 24), 30 at the peak with the rest of the grid below (across) and 1e6."""
    case = S.regime_set()
    got = _as_dict(_call(case))
    assert all(torch.isfinite(v).all() for v in got.values())
    _check(got, _ref(case), "x at 0.1, 20, 30 and 1e6")


def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    args = _dev(S.call_args(S.base_set()))
    full = FN.waveform_loglike_sky(**args, posterior=True, snr_map=True)
    for want, post, smap in ((("lnl_sky_mix",), False, False), ((), True, False), ((), False, True), (["pix_index", "snr"], False, True)):
        m = FN.waveform_loglike_sky(**args, want=want, posterior=post, snr_map=smap)
        for name in m._fields:
            asked = name in want or (post and name in ("post", "post_mix")) or (smap and name == "snr_map")
            assert (torch.equal(getattr(m, name), getattr(full, name)) if asked else getattr(m, name) is None), (want, name)
    with pytest.raises(ValueError, match="at least one"):
        FN.waveform_loglike_sky(**args, want=())


# ---- dead things -------------------------------------------------------------------------------------------------------------------
def test_dead_points_are_selected_out_and_nothing_of_them_is_read():
    """Weights 0, negative, NaN, Inf (another third per detector) and points beyond n_valid, NaN planted there in h and data: the
    reference, no NaN anywhere, and the bits of the call with zeros in place of the NaN."""
    case = S.dead_points_set()
    assert torch.isnan(case["data"]).any() and torch.isnan(case["h"]).any() and torch.isnan(case["weights"]).any()
    m = _call(case)
    got = _as_dict(m)
    assert all(torch.isfinite(v).all() for v in got.values())
    _check(got, _ref(case), "dead points")
    clean = S.poison(_clone(case), 0.0)
    assert not torch.isnan(clean["data"]).any() and not torch.isnan(clean["h"]).any()
    _same_bits(m, _call(clean), "NaN against zeros at dead points")


def test_dead_pixels_get_no_mass_and_reach_no_other_pixel():
    case = S.base_set()
    dead = [1, 3, 6]
    case["log_prior"][dead] = torch.tensor([-math.inf, math.nan, math.inf], dtype=torch.float64)
    clean = _clone(case)
    clean["log_prior"][dead] = -math.inf
    case["delays"][dead], case["response"][dead] = math.nan, math.nan
    m = _call(case)
    got = _as_dict(m)
    assert (got["post"][:, dead] == -math.inf).all() and (got["snr_map"][:, dead] == 0).all() and (got["post_mix"][:, dead] == -math.inf).all()
    live = [p for p in range(7) if p not in dead]
    assert all(torch.isfinite(got[k][:, live]).all() for k in ("post", "snr_map", "post_mix"))
    assert all(torch.isfinite(got[k]).all() for k in ("lnl_sky", "snr", "lnl_sky_mix"))
    _same_bits(m, _call(clean), "dead pixels: NaN against clean response and delays")
    _check(got, _ref(case), "three dead pixels")


def test_all_pixels_dead():
    case = S.base_set()
    case["log_prior"][:] = -math.inf
    case["log_prior"][2] = math.nan
    case["response"][:] = math.nan
    got = _as_dict(_call(case))
    assert (got["lnl_sky"] == -math.inf).all() and (got["lnl_sky_mix"] == -math.inf).all()
    assert (got["post"] == -math.inf).all() and (got["post_mix"] == -math.inf).all()
    assert (got["pix_index"] == 0).all() and (got["tau_index"] == 0).all() and (got["snr"] == 0).all() and (got["snr_map"] == 0).all()
    _check(got, _ref(case), "all pixels dead")


def test_a_pixel_without_response_and_a_zero_template_keep_the_prior():
    """C = 0 at every detector: HH_p = 0, Lambda = 1, u_p = log_prior_p to the gate.  A zero template: that of every pixel."""
    case = S.base_set()
    case["response"][4] = 0.0
    ref = _ref(case)
    got = _as_dict(_call(case))
    _check(got, ref, "pixel 4 without response")
    u4 = got["post"][:, 4] + got["lnl_sky"]
    assert ((u4 - case["log_prior"][4]).abs() <= 1e-10 * ref["scale"] + 1e-12).all() and (got["snr_map"][:, 4] == 0).all()
    case = S.base_set()
    case["h"][4, :, 0] = 0.0
    ref = _ref(case)
    got = _as_dict(_call(case))
    _check(got, ref, "row 4 with a zero template")
    lp = case["log_prior"]
    assert torch.equal(got["post"][4] + got["lnl_sky"][4], lp) or ((got["post"][4] + got["lnl_sky"][4] - lp).abs() <= 1e-12).all()
    assert got["pix_index"][4] == int(lp.argmax()) and got["tau_index"][4] == 0 and got["snr"][4] == 0 and (got["snr_map"][4] == 0).all()


# ---- isolation ----------------------------------------------------------------------------------------------------------------------
def test_a_nan_at_a_live_point_stays_in_its_row():
    case = S.base_set()  # nine rows, one tile; row 4 is latent sample 1 of task 1
    clean = _call(case)
    case["h"][4, 11, 1] = math.nan
    m = _call(case)
    assert torch.isnan(m.lnl_sky[4]) and torch.isnan(m.lnl_sky_mix[1])
    others = [r for r in range(9) if r != 4]
    for name in ("lnl_sky", "pix_index", "tau_index", "snr", "post", "snr_map"):
        assert torch.equal(getattr(m, name)[others], getattr(clean, name)[others]), name
    assert torch.equal(m.lnl_sky_mix[[0, 2]], clean.lnl_sky_mix[[0, 2]]) and torch.equal(m.post_mix[[0, 2]], clean.post_mix[[0, 2]])


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
def test_repeats_permutations_and_copies_give_the_same_bits():
    """33 rows x 40 pixels: several tiles and workgroups.  Pixels permuted; tasks permuted within every latent sample; the best pixel
    copied to a smaller index."""
    case = S.perm_set()
    first = _call(case)
    _same_bits(first, _call(case), "a second call")
    _check(_as_dict(first), _ref(case), "33 x 40")
    g = torch.Generator().manual_seed(5)
    P, Bn, n_z = 40, 11, 3
    pp = torch.randperm(P, generator=g)
    moved = _clone(case)
    for k in ("response", "delays", "log_prior"):
        moved[k] = case[k][pp]
    m = _call(moved)
    pd = pp.to(DEV)
    assert torch.equal(m.post, first.post[:, pd]) and torch.equal(m.snr_map, first.snr_map[:, pd]), "pixels permuted"
    assert torch.equal(m.post_mix, first.post_mix[:, pd]) and torch.equal(m.lnl_sky, first.lnl_sky) and torch.equal(m.snr, first.snr)
    assert torch.equal(pd[m.pix_index.long()], first.pix_index.long())
    bp = torch.randperm(Bn, generator=g)
    rows = (torch.arange(n_z).view(-1, 1) * Bn + bp.view(1, -1)).reshape(-1)
    moved = _clone(case)
    moved["h"], moved["data"], moved["weights"] = case["h"][rows], case["data"][bp], case["weights"][bp]
    m = _call(moved)
    rd, bd = rows.to(DEV), bp.to(DEV)
    for name in ("post", "snr_map", "lnl_sky", "pix_index", "tau_index", "snr"):
        assert torch.equal(getattr(m, name), getattr(first, name)[rd]), ("rows permuted", name)
    assert torch.equal(m.lnl_sky_mix, first.lnl_sky_mix[bd]) and torch.equal(m.post_mix, first.post_mix[bd])
    copied = _clone(case)
    p0, dst = case["p0"], case["p0"] - 17  # (another tile of 16)
    for k in ("response", "delays", "log_prior"):
        copied[k][dst] = case[k][p0]
    m = _call(copied)
    assert torch.equal(m.post[:, dst], m.post[:, p0]) and torch.equal(m.snr_map[:, dst], m.snr_map[:, p0])
    assert (m.pix_index == dst).all()


def test_a_small_call_gives_the_same_bits_before_and_after_the_largest_workspace():
    from npf_gwwaveform_amd import functional as FN

    small = S.build(Bn=3, n_z=1, P=3, seed=55)
    before = _call(small)
    big = S.sweep_sets(FN.SKY_JC)[-1][1]  # 33 x 40 x 3 x 129 x 17: the largest workspace of the suite
    _call(big)
    _same_bits(before, _call(small), "3 x 3 around the largest workspace")


# ---- consistency with the shipped kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tau", (None, 17))
def test_one_pixel_with_unit_prior_mass_meets_waveform_loglike_network(n_tau):
    from npf_gwwaveform_amd import functional as FN

    case = S.build(Bn=3, n_z=3, T=129, D=3, P=1, n_tau=n_tau, h_ld=4, wform="BT", seed=61, counts=(129, 60, 17))
    case["log_prior"] = torch.zeros(1, dtype=torch.float64)
    ref = _ref(case)
    a = _dev(S.call_args(case))
    sky = FN.waveform_loglike_sky(**a)
    net = FN.waveform_loglike_network(a["h"], a["data"], a["response"].expand(3, -1, -1).contiguous(), a["delays"].expand(3, -1).contiguous(),
                                      a["weights"], a["freqs"], a["taus"], a["n_valid"])
    gate = (1e-10 * ref["scale"] + 1e-12).to(DEV)
    q = {"lnl_sky": float(((sky.lnl_sky - net.lnl_marg).abs() / gate).max()),
         "snr": float(((sky.snr - net.snr).abs() / (1e-10 * net.snr.abs() + 1e-12)).max()),
         "lnl_sky_mix": float(((sky.lnl_sky_mix - net.lnl_mix).abs() / gate.view(3, 3).max(0).values).max())}
    print(f"LOGLIKE_SKY P=1 n_tau={n_tau} against waveform_loglike_network: difference / gate " + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))
    assert max(q.values()) <= 1.0 and torch.equal(sky.tau_index, net.tau_index) and (sky.pix_index == 0).all()


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _predict(name, latent):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    torch.manual_seed(9)
    post = model.condition(Xc, Yc) if latent else None
    if latent:
        p = post.query(Xt)
    else:
        with torch.no_grad():
            p = model(Xc, Yc, Xt)[0]
    return case, model, post, Xt, p


def _sky_observation(loc, P, seed, n_tau, D=3):
    """A sky grid and the data of a signal planted with the first latent sample's own waveform ``loc`` [B, T, 2] at pixel P // 2."""
    g = torch.Generator().manual_seed(seed)
    Bn, T = loc.shape[:2]
    resp, dl = S.sky(P, D, g)
    f, taus = torch.linspace(20.0, 512.0, T), S.grid(n_tau)
    data = S.plant(loc, resp[P // 2], dl[P // 2], f, taus[0] + 3 * taus[1]) + 0.02 * torch.randn(Bn, D, T, 2, generator=g, dtype=torch.float64)
    mass = 0.2 + torch.rand(P, generator=g, dtype=torch.float64)
    w = 0.5 + torch.rand(Bn, D, T, generator=g)
    return data.float().to(DEV), resp.to(DEV), dl.to(DEV), torch.log(mass / mass.sum()).to(DEV), w.to(DEV), f.to(DEV), taus


def _well_posed(ref, what):
    lead_u, lead_x = S.margins(ref)
    assert lead_u >= 1e3 and lead_x >= 1e-6, f"{what}: the inputs leave the indices ill posed ({lead_u:.3g}, {lead_x:.3g})"


def _flat(m):
    d = {k: v for k, v in m._asdict().items() if v is not None and k != "tau"}
    d["lnl_sky_mix"] = d.pop("lnl")
    return {k: (v.reshape(-1, v.shape[-1]) if k in ("post", "snr_map") else (v if k in ("post_mix", "lnl_sky_mix") else v.reshape(-1)))
            for k, v in d.items()}


@pytest.mark.parametrize("name,latent", MODELS)
def test_models_loglike_sky_meets_the_reference_on_their_own_decoder_output(name, latent):
    import npf_gwwaveform_amd as A

    FN = A.functional
    case, model, post, Xt, p = _predict(name, latent)
    Bn, T, n_z, P = case["B"], case["T"], case.get("n_z", 1), 19
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2).cpu()
    data, resp, dl, lp, w, f, taus = _sky_observation(loc[:Bn], P, 41, FN.SKY_JC + 1)
    m = p.loglike_sky(data, resp, dl, log_prior=lp, weights=w, freqs=f, taus=taus, snr_map=True)
    plain = p.loglike_sky(data, resp, dl, freqs=f, posterior=False)
    mean = p.loglike_sky(data, resp, dl, log_prior=lp, weights=w, freqs=f, taus=taus, of="mean")
    assert isinstance(m, A.SkyLogLike)  # (base_dist was read above, to plant the signal)
    assert all(getattr(m, k).shape == (n_z, Bn) for k in ("lnl_sky", "pix_index", "tau_index", "tau", "snr")) and m.lnl.shape == (Bn,)
    assert m.post.shape == (n_z, Bn, P) and m.snr_map.shape == (n_z, Bn, P) and m.post_mix.shape == (Bn, P)
    assert m.pix_index.dtype == torch.int32 and m.tau_index.dtype == torch.int32 and m.tau.dtype == torch.float64
    assert plain.tau is None and plain.tau_index is None and plain.post is None and plain.post_mix is None and plain.snr_map is None
    assert mean.lnl_sky.shape == (1, Bn) and mean.post.shape == (1, Bn, P) and mean.snr_map is None
    fn = FN.waveform_loglike_sky(p._suff.reshape(n_z * Bn, T, 4), data, resp, dl, lp, w, f, taus, posterior=True, snr_map=True)
    for mine, theirs in (("lnl", "lnl_sky_mix"), ("lnl_sky", "lnl_sky"), ("pix_index", "pix_index"), ("tau_index", "tau_index"),
                         ("snr", "snr"), ("post", "post"), ("post_mix", "post_mix"), ("snr_map", "snr_map")):
        assert torch.equal(getattr(m, mine).reshape(-1), getattr(fn, theirs).reshape(-1)), mine
    cpu = lambda t: t.cpu() if isinstance(t, torch.Tensor) else t  # noqa: E731
    args = [cpu(t) for t in (data, resp, dl, lp, w, f, taus)]
    ref = S.reference(loc, *args)
    _well_posed(ref, name)
    _check(_flat(m), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().view(-1), taus[0] + ref["tau_index"].double() * taus[1]), name
    _check(_flat(plain), S.reference(loc, args[0], args[1], args[2], None, None, args[5], None), f"{name} without prior, weights and grid")
    ref_mean = S.reference(p.summary().mean, *args)
    _well_posed(ref_mean, name)
    _check(_flat(mean), ref_mean, f"{name} of=mean against summary().mean")
    assert torch.equal(mean.lnl, mean.lnl_sky[0]), name
    if n_z == 1:
        assert torch.equal(m.lnl, m.lnl_sky[0]), name
    with pytest.raises(ValueError, match="of must be"):
        p.loglike_sky(data, resp, dl, freqs=f, of="median")


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike_sky(torch.zeros(3, 2, 37, 2, device=DEV), torch.ones(5, 2, 2, dtype=torch.float64, device=DEV),
                      torch.zeros(5, 2, dtype=torch.float64, device=DEV), freqs=torch.ones(37, device=DEV))


def test_query_and_loglike_sky_replay_from_one_graph_after_the_sky_grid_is_overwritten():
    """response, delays and log_prior are overwritten in place; both replays are bit-equal to the eager call on the new values: the
    host reads none of them."""
    from npf_gwwaveform_amd import functional as FN

    case, model, post, Xt, p = _predict("attnlnp_r256_c200_nz8", True)
    Bn, T, n_z, P = case["B"], case["T"], case.get("n_z", 1), 19
    loc0 = p.base_dist.loc.double().reshape(n_z * Bn, T, 2).cpu()[:Bn]
    data, c_s, dl_s, lp_s, w, f, taus = _sky_observation(loc0, P, 1, FN.SKY_JC + 1)
    kw = dict(weights=w, freqs=f, taus=taus, snr_map=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # (at the sizes, before capturing: the workspace is allocated here)
            post.query(Xt).loglike_sky(data, c_s, dl_s, log_prior=lp_s, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branches)
        p_g = post.query(Xt)
        m_g = p_g.loglike_sky(data, c_s, dl_s, log_prior=lp_s, **kw)
        loc_g = p_g.base_dist.loc
    _, c_new, dl_new, lp_new, _, _, _ = _sky_observation(loc0, P, 100, FN.SKY_JC + 1)
    lp_new[5] = -math.inf  # (and a dead pixel)
    for dst, src in ((c_s, c_new), (dl_s, dl_new), (lp_s, lp_new)):
        dst.copy_(src)
    eager = post.query(Xt).loglike_sky(data, c_new, dl_new, log_prior=lp_new, **kw)
    seen = []
    for step in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(m_g, eager):
            assert torch.equal(a, b), step
        seen.append(m_g.post.clone())
    assert torch.equal(seen[0], seen[1]) and (m_g.post[..., 5] == -math.inf).all()
    ref = S.reference(loc_g.double().reshape(n_z * Bn, T, 2).cpu(), data.cpu(), c_new.cpu(), dl_new.cpu(), lp_new.cpu(), w.cpu(), f.cpu(), taus)
    _well_posed(ref, "replay")
    _check(_flat(m_g), ref, "replay on the overwritten grid")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from npf_gwwaveform_amd import functional as FN

    a = _dev(S.call_args(S.build(Bn=3, n_z=1, P=3, seed=56)))
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_loglike_sky(**dict(a, h=a["h"].cpu()))
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_loglike_sky(**dict(a, h=a["h"].double()))
    with pytest.raises(ValueError, match="response"):
        FN.waveform_loglike_sky(**dict(a, response=a["response"].cpu()))
    with pytest.raises(ValueError, match="freqs"):
        FN.waveform_loglike_sky(**dict(a, freqs=a["freqs"].expand(3, -1).contiguous()))
    with pytest.raises(ValueError, match="freqs"):
        FN.waveform_loglike_sky(**dict(a, freqs=None))
    with pytest.raises(ValueError, match="pixels"):
        FN.waveform_loglike_sky(**dict(a, response=a["response"][:0], delays=a["delays"][:0]))
    nine = dict(a, data=a["data"][:, :1].expand(-1, 9, -1, -1).contiguous(), response=a["response"][:, :1].expand(-1, 9, -1).contiguous(),
                delays=a["delays"][:, :1].expand(-1, 9).contiguous())
    with pytest.raises(ValueError, match="detectors"):
        FN.waveform_loglike_sky(**nine)
