"""Distance-marginalised likelihood on the GPU: ``npf_waveform_loglike_dist`` and ``npf_waveform_loglike_net_dist`` against the float64
reference of tests/loglike_dist_reference.py (checked on the CPU by tests/test_loglike_dist_host.py) over the eight input regimes of
``loglike_reference.build``, scale grids of 1 .. 300 points with dead entries and without a live one; the identities (one unit scale
is ``lnl_marg``, a power-of-two scale is the scaled template, the posterior sums to one, a constant in the prior, a planted
amplitude); NaN in what is not read; bit-identical repeats and ``want`` subsets; a captured ``query`` + ``loglike_distance`` whose
scales and prior are overwritten in place; the model-level calls.

Gates (loglike_dist_reference.ratios), S_r = max over live i of (a_i sqrt(HH DD) + a_i^2 HH / 2 + |ln pi_i|): lnl_dist, lnl_dist_mix
|d| <= 1e-10 S_r + 1e-12 (per task: the largest S_r of its rows); post, post_mix twice that, -inf entries exact; scale_hat, lnl_amp_max
1e-10 relative + 1e-12; scale_index exact; every ``base`` field bit-equal to the plain call.  Every test prints its worst error /
gate ratio per quantity."""
import math

import pytest
import torch

import loglike_dist_reference as Dd
import loglike_net_reference as N
import loglike_reference as R1
from test_hip_dispatch import _c
from test_hip_predict import _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {"attnlnp": _c("AttnLNP", 64, 20, n_z=3, B=3, T=37), "cnp": _c("CNP", 64, 20, B=3, T=37)}
F64 = dict(dtype=torch.float64, device=DEV)


@pytest.fixture(scope="module")
def all_cases():
    out = {}
    for network in (False, True):
        rows = []
        for tag, fac, case, s, p in Dd.cases(network):
            ref = Dd.parent_reference(network, case)
            rows.append((tag, fac, case, s, p, ref, Dd.marginalise(ref, s, p)))
        out[network] = rows
    return out


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _call(network, case, scales, log_prior, **kw):
    from npf_gwwaveform_amd import functional as FN

    M = N if network else R1
    fn = FN.waveform_loglike_network_distance if network else FN.waveform_loglike_distance
    return fn(**_dev(M.call_args(case)), scales=scales.to(DEV), log_prior=log_prior.to(DEV), **kw)


def _plain(network, case, **kw):
    from npf_gwwaveform_amd import functional as FN

    M = N if network else R1
    return (FN.waveform_loglike_network if network else FN.waveform_loglike)(**_dev(M.call_args(case)), **kw)


def _new(m):
    return {k: v for k, v in m._asdict().items() if k != "base" and v is not None}


def _check(got, ref, dist, what, worst=None):
    r = Dd.ratios(got, ref, dist)
    print(f"LOGLIKE_DIST {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
    return r


def _same_bits(a, b, what):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        if name == "base":
            _same_bits(x, y, what)
            continue
        assert (x is None and y is None) or torch.equal(x, y), (what, name)  # (torch.equal: -inf == -inf, and no NaN is expected)


def _sums_to_one(post, live_any, what):
    """sum_i exp(post_i) = 1 to 1e-12 wherever a scale is live; -inf everywhere where none is."""
    total = torch.exp(post).sum(-1).cpu()
    worst = float((total[live_any] - 1.0).abs().max()) if live_any.any() else 0.0
    assert worst <= 1e-12, (what, worst)
    assert (post.cpu()[~live_any] == -math.inf).all(), what
    return worst


# ---- the kernels against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R1.REGIMES)
@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_distance_likelihood_meets_the_float64_reference(network, regime, all_cases):
    """Every case of the regime: the gates; scale_index exact; no NaN anywhere; the posterior sums to one; every ``base`` field is
    bit-equal to the plain call; a second call gives the same bits."""
    worst, n, sum_worst = {}, 0, 0.0
    for tag, fac, case, s, p, ref, dist in all_cases[network]:
        if fac["regime"] != regime:
            continue
        n += 1
        first = _call(network, case, s, p, posterior=True)
        _same_bits(first, _call(network, case, s, p, posterior=True), tag)
        got = _new(first)
        Rn, n_a = fac["n_z"] * Dd.B, fac["n_a"]
        assert got["post"].shape == (Rn, n_a) and got["post_mix"].shape == (Dd.B, n_a) and got["lnl_dist_mix"].shape == (Dd.B,), tag
        assert all(got[k].shape == (Rn,) for k in ("lnl_dist", "scale_index", "scale_hat", "lnl_amp_max")), tag
        assert not any(torch.isnan(v).any() for v in got.values()), f"{tag}: NaN"
        _check(got, ref, dist, tag, worst)
        live_any = dist["live"].any(1)
        sum_worst = max(sum_worst, _sums_to_one(first.post, live_any, tag),
                        _sums_to_one(first.post_mix, live_any.view(-1, Dd.B).any(0), tag))
        assert (got["lnl_dist"].cpu()[~live_any] == -math.inf).all() and (got["scale_index"].cpu()[~live_any] == 0).all(), tag
        deg = ref["degenerate"]
        assert (got["scale_hat"].cpu()[deg] == 0).all() and (got["lnl_amp_max"].cpu()[deg] == 0).all(), tag
        plain = _plain(network, case)
        for name in plain._fields:
            x, y = getattr(first.base, name), getattr(plain, name)
            assert (x is None and y is None) or torch.equal(x, y), (tag, "base", name)
    assert n == len(Dd.N_AS)
    print(f"LOGLIKE_DIST worst over the {n} cases of {'network ' if network else ''}regime {regime}: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; |sum exp(post) - 1| {sum_worst:.3g}")


# ---- identities --------------------------------------------------------------------------------------------------------------------
def _identity_case(network, n_tau, regime="noise", seed=3):
    M = N if network else R1
    kw = dict(D=2) if network else {}
    return M.build(regime, 200, n_z=3, h_ld=4, wform="BT", fform="T" if n_tau else None, taus=M.grid(n_tau, regime), counts=(200, 17, 0),
                   j_star=None if n_tau is None else 2, seed=seed, **kw)


@pytest.mark.parametrize("n_tau", (None, 17, 257))
@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_one_unit_scale_with_unit_mass_is_lnl_marg(network, n_tau):
    case = _identity_case(network, n_tau)
    ref = Dd.parent_reference(network, case)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    dist = Dd.marginalise(ref, one, zero)
    m = _call(network, case, one, zero, posterior=True)
    gate = 1e-10 * dist["S"] + 1e-12
    d = (m.lnl_dist - m.base.lnl_marg).abs().cpu()
    same = torch.equal(m.lnl_dist, m.base.lnl_marg) and torch.equal(m.lnl_dist_mix, m.base.lnl_mix)
    print(f"LOGLIKE_DIST n_a=1 a=1 ln pi=0 {'network ' if network else ''}n_tau={n_tau}: lnl_dist bit-equal to lnl_marg: {same}; "
          f"worst error / gate {float((d / gate).max()):.3g}")
    assert (d <= gate).all()
    assert (m.post == 0).all() and float(m.post_mix.abs().max()) <= 1e-14 and (m.scale_index == 0).all()


@pytest.mark.parametrize("k", (-3, 2))
@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_one_power_of_two_scale_is_the_scaled_template(network, k):
    """lnl_dist of h at the one scale 2^k against lnl_marg of the plain call on h with its amplitude column times 2^k: scaling by a
    power of two is exact through launch 1, so 4 ulp of S_r."""
    case = _identity_case(network, 17, regime="edge")
    ref = Dd.parent_reference(network, case)
    a, zero = torch.full((1,), 2.0 ** k, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    dist = Dd.marginalise(ref, a, zero)
    m = _call(network, case, a, zero)
    scaled = dict(case, h=case["h"].clone())
    scaled["h"][..., 0] *= 2.0 ** k
    plain = _plain(network, scaled)
    ulp = torch.tensor([math.ulp(v) if v > 0 else 5e-324 for v in dist["S"].tolist()], dtype=torch.float64)
    d = (m.lnl_dist - plain.lnl_marg).abs().cpu()
    print(f"LOGLIKE_DIST one scale 2^{k} {'network' if network else 'single'}: worst |lnl_dist - lnl_marg(2^k h)| in ulp of S_r "
          f"{float((d / ulp).max()):.3g}; bit-equal: {torch.equal(m.lnl_dist, plain.lnl_marg)}")
    assert (d <= 4.0 * ulp).all()


@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_a_constant_in_the_prior_moves_lnl_dist_and_leaves_the_posterior(network):
    case = _identity_case(network, 17, regime="loud")
    ref = Dd.parent_reference(network, case)
    s, p = Dd.scale_grid(65, "A", "BA")
    dist = Dd.marginalise(ref, s, p)
    c = 7.25
    m0, m1 = _call(network, case, s, p, posterior=True), _call(network, case, s, p + c, posterior=True)
    gate = (1e-10 * dist["S"] + 1e-12).to(DEV)
    task_gate = gate.view(-1, Dd.B).max(0).values
    assert ((m1.lnl_dist - m0.lnl_dist - c).abs() <= gate).all()
    assert ((m1.lnl_dist_mix - m0.lnl_dist_mix - c).abs() <= task_gate).all()
    assert ((m1.post - m0.post).abs() <= 2.0 * gate.view(-1, 1)).all() and ((m1.post_mix - m0.post_mix).abs() <= 2.0 * task_gate.view(-1, 1)).all()
    assert torch.equal(m1.scale_index, m0.scale_index) and torch.equal(m1.scale_hat, m0.scale_hat)


@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_a_planted_amplitude_is_found_on_the_grid(network):
    """Planted data times a_true, a grid point: scale_map == a_true and scale_hat within 1e-6 relative of it (the fp32 rounding of
    the data)."""
    M = N if network else R1
    kw = dict(D=3) if network else {}
    case = M.build("planted", 200, n_z=1, h_ld=2, wform="T", fform="T", taus=M.grid(17), j_star=5, seed=2, **kw)
    s = Dd.geometric(65)
    p = torch.full((65,), -math.log(65.0), dtype=torch.float64)
    for i_true in (32, 40, 47):  # (a >= 1: below, ln I0's -ln(a x) / 2 moves the peak of a template this quiet by a grid step)
        a_true = float(s[i_true])
        scaled = dict(case, data=case["data"] * a_true)
        m = _call(network, scaled, s, p)
        live = ~Dd.parent_reference(network, scaled)["degenerate"]
        assert live.all()
        assert (m.scale_index == i_true).all(), (i_true, m.scale_index)
        assert (s.to(DEV)[m.scale_index.long()] == a_true).all()
        rel = float(((m.scale_hat - a_true).abs() / a_true).max())
        print(f"LOGLIKE_DIST planted a_true={a_true:.6g} {'network' if network else 'single'}: scale_hat relative error {rel:.3g}")
        assert rel <= 1e-6
        assert (m.base.tau_index == 5).all()


# ---- untouched memory and determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", (False, True), ids=("single", "network"))
def test_nan_in_what_is_not_read_changes_no_bit(network):
    """Dead scales hold NaN in the other tensor, dead points and rows beyond the counts hold NaN (the "removed" regime) -- against
    zeros (ones for the scale of a dead prior entry) there: no output changes a bit."""
    M = N if network else R1
    kw = dict(D=3) if network else {}
    case = M.build("removed", 200, n_z=3, h_ld=4, wform="T", fform="T", taus=M.grid(17), counts=(200, 17, 0), seed=5, **kw)
    assert torch.isnan(case["data"]).any() and torch.isnan(case["h"]).any()
    clean = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    if network:
        N.poison(clean, 0.0)
    else:
        dead = case["kill"] | (torch.arange(200).view(1, -1) >= case["n_valid"].long().view(-1, 1))
        clean["data"][dead] = 0.0
        clean["h"].view(3, R1.B, 200, 4)[:, dead] = 0.0
        clean["freqs"] = torch.nan_to_num(clean["freqs"], nan=0.0)
    assert not any(torch.isnan(clean[k]).any() for k in ("data", "h", "freqs"))
    for sform, pform in (("A", "A"), ("BA", "BA")):
        s_nan, p_nan = Dd.scale_grid(65, sform, pform, "dead", math.nan)
        s_0, p_0 = Dd.scale_grid(65, sform, pform, "dead", 0.0)
        assert torch.isnan(s_nan).sum() > torch.isnan(s_0).sum() and torch.isnan(p_nan).sum() > torch.isnan(p_0).sum()
        full = _call(network, case, s_nan, p_nan, posterior=True)
        _same_bits(full, _call(network, clean, s_0, p_0, posterior=True), (sform, pform))
        ref = Dd.parent_reference(network, clean)
        _clear_scale(Dd.marginalise(ref, s_0, p_0), "removed")
        _check(_new(full), ref, Dd.marginalise(ref, s_0, p_0), f"NaN where nothing is read, scales {sform}, prior {pform}")


def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    for network in (False, True):
        M = N if network else R1
        kw = dict(D=2) if network else {}
        case = M.build("noise", 37, n_z=3, h_ld=4, wform="T", fform="BT", taus=M.grid(17), counts=(37, 17, 0), seed=9, **kw)
        s, p = Dd.scale_grid(Dd.SC + 1, "BA", "A")
        full = _call(network, case, s, p, posterior=True)
        for want, posterior in ((("lnl_dist",), False), (("lnl_dist_mix", "hh"), False), ((), True), (["scale_index", "tau_index"], True),
                                (("scale_hat", "lnl_amp_max"), False), (("lnl_marg", "dd"), False), (("snr",), True)):
            m = _call(network, case, s, p, want=want, posterior=posterior)
            for name in FN.LOGLIKE_DIST_NAMES + ("post", "post_mix"):
                if name in want or (name in ("post", "post_mix") and posterior):
                    assert torch.equal(getattr(m, name), getattr(full, name)), (want, name)
                else:
                    assert getattr(m, name) is None, (want, name)
            for name in m.base._fields:
                if name in want:
                    assert torch.equal(getattr(m.base, name), getattr(full.base, name)), (want, name)
                else:
                    assert getattr(m.base, name) is None, (want, name)
        a = _dev(M.call_args(case))
        fn = FN.waveform_loglike_network_distance if network else FN.waveform_loglike_distance
        for bad in (dict(scales=s), dict(log_prior=p)):  # on the CPU
            with pytest.raises(ValueError, match="device"):
                fn(**a, **dict(dict(scales=s.to(DEV), log_prior=p.to(DEV)), **bad))


def test_post_and_post_mix_are_written_whole():
    """The outputs come from the caching allocator: blocks of their sizes are filled with NaN and freed just before the call."""
    case = R1.build("noise", 37, n_z=3, h_ld=2, fform="T", taus=R1.grid(17), seed=4)
    for n_a, kind in ((300, "geo"), (257, "dead"), (Dd.SC + 1, "alldead")):
        s, p = Dd.scale_grid(n_a, "A", "A", kind)
        _call(False, case, s, p, posterior=True)
        torch.cuda.synchronize()
        junk = [torch.full(shape, math.nan, **F64) for shape in ((9, n_a), (3, n_a), (9,), (9,), (9,), (3,)) for _ in range(2)]
        del junk
        m = _call(False, case, s, p, posterior=True)
        assert not any(torch.isnan(v).any() for v in _new(m).values()), (n_a, kind)
        if kind == "alldead":
            assert (m.post == -math.inf).all() and (m.post_mix == -math.inf).all() and (m.lnl_dist == -math.inf).all()
            assert (m.lnl_dist_mix == -math.inf).all() and (m.scale_index == 0).all()


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _observation(Bn, T, seed):
    g = torch.Generator().manual_seed(seed)
    taus = R1.grid(17)
    return (torch.randn(Bn, T, 2, generator=g).to(DEV), (0.5 + torch.rand(Bn, T, generator=g)).to(DEV), torch.linspace(20.0, 512.0, T).to(DEV), taus)


def _predict(name):
    case = MODELS[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    torch.manual_seed(9)
    post = model.condition(Xc, Yc)
    return case, post, Xt, post.query(Xt)


def _clear_scale(dist, what):
    g = Dd.runner_up_in_gates(dist)
    assert float(g[dist["live"].any(1)].min()) >= 1e3, f"{what}: the inputs leave scale_index ill posed"


@pytest.mark.parametrize("name", list(MODELS))
def test_models_loglike_distance_is_the_functional_call_and_meets_the_reference(name):
    import npf_gwwaveform_amd as A

    FN = A.functional
    case, post, Xt, p = _predict(name)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    data, w, f, taus = _observation(Bn, T, 41)
    n_a = 65
    s, lp = (t.to(DEV) for t in Dd.scale_grid(n_a, "BA", "A"))
    m = p.loglike_distance(data, s, lp, weights=w, freqs=f, taus=taus, posterior=True)
    mean = p.loglike_distance(data, s, lp, weights=w, freqs=f, taus=taus, of="mean")
    assert p._base is None and isinstance(m, A.DistanceLogLike) and isinstance(m.base, A.LogLike)
    assert all(getattr(m, k).shape == (n_z, Bn) for k in ("lnl_dist", "scale_hat", "lnl_amp_max", "scale_index", "scale_map"))
    assert m.lnl.shape == (Bn,) and m.post.shape == (n_z, Bn, n_a) and m.post_mix.shape == (Bn, n_a)
    assert m.scale_index.dtype == torch.int32 and all(getattr(m, k).dtype == torch.float64 for k in ("lnl", "lnl_dist", "scale_map", "post"))
    assert mean.lnl_dist.shape == (1, Bn) and mean.post is None and mean.post_mix is None and mean.base.lnl_marg.shape == (1, Bn)
    assert torch.equal(mean.lnl, mean.lnl_dist[0])
    fn = FN.waveform_loglike_distance(p._suff.reshape(n_z * Bn, T, 4), data, s, lp, w, f, taus, posterior=True)
    assert torch.equal(m.lnl, fn.lnl_dist_mix) and torch.equal(m.lnl_dist.reshape(-1), fn.lnl_dist)
    assert torch.equal(m.post.reshape(-1, n_a), fn.post) and torch.equal(m.post_mix, fn.post_mix)
    assert torch.equal(m.scale_map, s.gather(1, m.scale_index.long().t()).t())
    base = p.loglike(data, weights=w, freqs=f, taus=taus)
    for k in base._fields:
        x, y = getattr(m.base, k), getattr(base, k)
        assert (x is None and y is None) or torch.equal(x, y), k
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2)
    ref = R1.reference(loc, data, w, f, taus)
    dist = Dd.marginalise(ref, s, lp)
    _clear_scale(dist, name)
    got = dict(lnl_dist=m.lnl_dist, lnl_dist_mix=m.lnl, scale_hat=m.scale_hat, lnl_amp_max=m.lnl_amp_max, scale_index=m.scale_index,
               post=m.post, post_mix=m.post_mix)
    _check(got, ref, dist, f"{name} of=samples against base_dist.loc")
    ref_mean = R1.reference(p.summary().mean, data, w, f, taus)
    dist_mean = Dd.marginalise(ref_mean, s, lp)
    _clear_scale(dist_mean, name)
    _check(dict(lnl_dist=mean.lnl_dist, lnl_dist_mix=mean.lnl, scale_index=mean.scale_index), ref_mean, dist_mean, f"{name} of=mean")
    # the network twin with one detector of unit response is the same likelihood
    unit = torch.tensor([1.0, 0.0], **F64).repeat(Bn, 1, 1)
    net = p.loglike_network_distance(data.unsqueeze(1), unit, None, s, lp, weights=w.unsqueeze(1), freqs=f, taus=taus, posterior=True)
    assert isinstance(net, A.NetworkDistanceLogLike) and isinstance(net.base, A.NetworkLogLike)
    _check(dict(lnl_dist=net.lnl_dist, lnl_dist_mix=net.lnl, scale_index=net.scale_index, post=net.post, post_mix=net.post_mix), ref, dist,
           f"{name} network twin, D = 1")


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    one = torch.ones(4, **F64)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike_distance(torch.zeros(3, 37, 2, device=DEV), one, one)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike_network_distance(torch.zeros(3, 2, 37, 2, device=DEV), torch.ones(3, 2, 2, **F64), None, one, one)


# ---- one captured query + loglike_distance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_query_and_loglike_distance_replay_from_one_graph(name):
    """Scales and prior are overwritten in place between the replays; every replay equals the eager call on the new values bit for
    bit: the host reads neither."""
    case, post, Xt, _ = _predict(name)
    Bn, T = case["B"], case["T"]
    data, w, f, taus = _observation(Bn, T, 1)
    n_a = Dd.SC + 1
    s_s, p_s = (t.to(DEV).clone() for t in Dd.scale_grid(n_a, "A", "BA"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            post.query(Xt).loglike_distance(data, s_s, p_s, weights=w, freqs=f, taus=taus, posterior=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branches)
        p_g = post.query(Xt)
        m_g = p_g.loglike_distance(data, s_s, p_s, weights=w, freqs=f, taus=taus, posterior=True)
    seen = []
    for step in range(2):
        s_new = Dd.geometric(n_a, -2.0 - step, 3.0).to(DEV)
        p_new = torch.stack([Dd.volume_prior(s_new.cpu(), 1.0 + step + 0.5 * b) for b in range(Bn)]).to(DEV)
        if step == 1:
            s_new[3] = 0.0  # (and a dead scale)
        s_s.copy_(s_new)
        p_s.copy_(p_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = p_g.loglike_distance(data, s_new, p_new, weights=w, freqs=f, taus=taus, posterior=True)  # (on the replay's own rows)
        _same_bits(m_g, eager, f"{name} replay {step}")
        seen.append(m_g.lnl_dist.clone())
    assert not torch.equal(seen[0], seen[1])
