"""Coherent network log likelihood on the GPU: ``npf_waveform_loglike_net`` against the float64 reference of
tests/loglike_net_reference.py (checked on the CPU by tests/test_loglike_net_host.py) over its eight input regimes with 1, 2, 3 and 8
detectors; one detector with unit response and no delay against ``waveform_loglike``; NaN in everything the kernel promises not to
read; a detector without response; bit-identical repeats and ``want`` subsets; ``HeadDistribution.loglike_network`` of a latent and
a deterministic model, padded targets, and a captured ``query`` + ``loglike_network`` whose delays and responses are overwritten
in place between replays.

Gates (loglike_net_reference.ratios): those of loglike_reference.ratios with HH and DD in place of hh and dd -- lnl_*, lnl_mix* and
the series' L_j |d| <= 1e-10 (sqrt(HH DD) + HH / 2) + 1e-12; hh, dd, hh_det, dd_det 2^-50 relative; snr and series SNR 1e-10
relative + 1e-12; snr_det absolute 1e-10 sqrt(dd_k) + 1e-12; phase 1e-9 mod 2 pi where x* >= 1e-3 sqrt(HH DD); tau_index exact.
tests/test_loglike_net_host.py measures the recurrence against the direct form at 0.03 of these gates at most.  Every test prints
its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import loglike_net_reference as N
import loglike_reference as R1
from test_hip_dispatch import _c
from test_hip_predict import _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_ROW = ("hh", "snr", "lnl_max", "lnl_marg", "tau_index", "phase")
MODELS = {"attnlnp": _c("AttnLNP", 64, 20, n_z=3, B=3, T=37), "attncnp": _c("AttnCNP", 64, 20, B=3, T=37)}
D_MODEL = 3


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    return [(tag, fac, case, N.reference(**N.call_args(case))) for tag, fac, case in N.cases(FN.MATCH_JC, FN.LOGLIKE_I0_SWITCH)]


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _as_dict(m):
    d = {k: v for k, v in m._asdict().items() if v is not None}
    if "hh" in d and "optimal_snr" not in d:
        d["optimal_snr"] = d["hh"].sqrt()
    if "lnl" in d:
        d["lnl_mix"] = d.pop("lnl")
    return d


def _check(got, ref, what, worst=None):
    r = N.ratios(got, ref)
    print(f"LOGLIKE_NET {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
    return r


def _same_bits(a, b, what):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), (what, name)


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", N.REGIMES)
def test_network_loglike_meets_the_float64_reference(regime, all_cases):
    """Every case of the regime (none is skipped): the gates; a second call gives the same bits and nothing but finite values;
    degenerate rows hold the stated zeros; the planted index is found."""
    from npf_gwwaveform_amd import functional as FN

    worst, n = {}, 0
    for tag, fac, case, ref in all_cases:
        if fac["regime"] != regime:
            continue
        n += 1
        args = _dev(N.call_args(case))
        first = FN.waveform_loglike_network(**args, series=True)
        _same_bits(first, FN.waveform_loglike_network(**args, series=True), tag)
        got = {k: v.cpu() for k, v in first._asdict().items()}
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        assert all(v.dtype == (torch.int32 if k == "tau_index" else torch.float64) for k, v in got.items()), tag
        Rn, n_grid, D = fac["n_z"] * N.B, max(fac["n_tau"] or 0, 1), fac["D"]
        assert got["series"].shape == (Rn, n_grid, 2) and got["dd"].shape == (N.B,) and got["lnl_mix"].shape == (N.B,), tag
        assert got["hh_det"].shape == (Rn, D) and got["snr_det"].shape == (Rn, D) and got["dd_det"].shape == (N.B, D), tag
        assert all(got[k].shape == (Rn,) for k in PER_ROW), tag
        _check(_as_dict(FN.WaveformLogLikeNetwork(**got)), ref, tag, worst)
        deg = ref["degenerate"]
        for name in ("snr", "lnl_max", "lnl_marg", "tau_index", "phase", "hh"):
            assert (got[name][deg] == 0).all(), (tag, name)
        assert (got["series"][deg] == 0).all(), tag
        if regime == "planted":
            assert (got["tau_index"][~deg] == case["j_star"]).all(), tag
        if fac["zero_det"] is not None and regime in ("noise", "bigphase", "removed"):  # no response: still its own SNR (its data are noise)
            live = ref["hh_det"][:, fac["zero_det"]] > 0
            assert live.any() and (got["snr_det"][live, fac["zero_det"]] > 0).all(), tag
    assert n >= 14
    print(f"LOGLIKE_NET worst over the {n} cases of regime {regime}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("n_tau", (None, 17, 257))
def test_one_detector_with_unit_response_and_no_delay_meets_the_gates_of_waveform_loglike(n_tau):
    """D = 1, C = 1, delay 0 (given as zeros and as None) on the inputs of a single-stream case: the single-stream reference within
    the single-stream gates, as ``waveform_loglike`` itself; whether the bits agree is printed (it is not required)."""
    from npf_gwwaveform_amd import functional as FN

    one = R1.build("noise", 200, n_z=3, h_ld=4, wform="BT", fform="T" if n_tau else None, taus=R1.grid(n_tau), counts=(200, 17, 0), seed=3)
    ref = R1.reference(**R1.call_args(one))
    a = _dev(R1.call_args(one))
    single = FN.waveform_loglike(**a, series=True)
    unit = torch.tensor([1.0, 0.0], dtype=torch.float64, device=DEV).repeat(N.B, 1, 1)
    for delays in ((None, torch.zeros(N.B, 1, dtype=torch.float64, device=DEV)) if n_tau else (None,)):
        net = FN.waveform_loglike_network(a["h"], a["data"].unsqueeze(1), unit, delays, a["weights"].unsqueeze(1), a["freqs"], a["taus"],
                                          a["n_valid"], series=True)
        shared = {k: getattr(net, k) for k in single._fields}
        r = R1.ratios(dict(shared, optimal_snr=net.hh.sqrt()), ref)
        r0 = R1.ratios(dict(single._asdict(), optimal_snr=single.hh.sqrt()), ref)
        same = all(torch.equal(shared[k], getattr(single, k)) for k in single._fields)
        print(f"LOGLIKE_NET D=1 n_tau={n_tau} delays={'zeros' if delays is not None else 'None'}: bits equal to waveform_loglike: {same}; "
              f"worst error / gate {max(r.values()):.3g} (waveform_loglike: {max(r0.values()):.3g})")
        assert max(r.values()) <= 1.0 and max(r0.values()) <= 1.0, (r, r0)
        assert torch.equal(net.hh_det[:, 0], net.hh) and torch.equal(net.dd_det[:, 0], net.dd)


@pytest.mark.parametrize("wform", ("T", "BT"))
def test_nan_in_what_is_not_read_changes_no_bit(wform):
    """Points removed per detector (another third in each) and rows beyond the counts: NaN in everything the kernel promises not to
    read against zeros there -- no output changes a bit -- and both meet the reference, which masks those points."""
    from npf_gwwaveform_amd import functional as FN

    case = N.build("removed", 200, D=3, n_z=3, h_ld=4, wform=wform, fform="T" if wform == "T" else "BT", taus=N.grid(17),
                   counts=(200, 17, 0), seed=5)
    assert not torch.equal(case["kill"][:, 0], case["kill"][:, 1])  # the detectors lose different points
    assert all(torch.isnan(case[k]).any() for k in ("data", "h", "freqs"))
    clean = N.poison({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}, 0.0)
    assert not any(torch.isnan(clean[k]).any() for k in ("data", "h", "freqs"))
    full = FN.waveform_loglike_network(**_dev(N.call_args(case)), series=True)
    _same_bits(full, FN.waveform_loglike_network(**_dev(N.call_args(clean)), series=True), wform)
    assert all(torch.isfinite(v).all() for v in full)
    _check(_as_dict(full), N.reference(**N.call_args(clean)), f"removed per detector, weights {wform}")


def test_a_detector_without_response_changes_no_network_output_and_reports_its_snr():
    from npf_gwwaveform_amd import functional as FN

    case = N.build("noise", 200, D=3, n_z=3, h_ld=2, wform="BT", fform="T", taus=N.grid(17), seed=11, zero_det=1)
    ref = N.reference(**N.call_args(case))
    keep = [0, 2]
    less = dict(N.call_args(case), data=case["data"][:, keep], response=case["response"][:, keep], delays=case["delays"][:, keep],
                weights=case["weights"][:, keep])
    ref_less = N.reference(**less)
    full = FN.waveform_loglike_network(**_dev(N.call_args(case)), series=True)
    part = FN.waveform_loglike_network(**_dev(less), series=True)
    _check(_as_dict(full), ref, "three detectors, the second without response")
    net = {k: getattr(full, k) for k in ("hh", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "lnl_mix", "lnl_max_mix", "series")}
    _check(net, ref_less, "the network outputs against the call without that detector")  # (dd: DD does count its data)
    assert torch.equal(full.tau_index, part.tau_index)
    assert (full.snr_det[:, 1] > 0).all() and (full.hh_det[:, 1] > 0).all()
    _check(dict(snr_det=full.snr_det[:, keep].contiguous(), hh_det=full.hh_det[:, keep].contiguous()),
           dict(ref_less, dd=ref_less["dd"]), "the other detectors' own outputs")


def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    case = _dev(N.call_args(N.build("noise", 37, D=8, n_z=3, h_ld=4, wform="T", fform="BT", taus=N.grid(FN.MATCH_JC + 1),
                                    counts=(37, 17, 0), seed=9)))
    full = FN.waveform_loglike_network(**case, series=True)
    for want, series in ((("lnl_mix",), False), (("hh", "dd_det"), False), (["tau_index", "snr_det"], True), ((), True),
                         (("hh_det",), False), (("lnl_max_mix", "snr", "dd"), False)):
        m = FN.waveform_loglike_network(**case, want=want, series=series)
        for name in m._fields:
            if name in want or (name == "series" and series):
                assert torch.equal(getattr(m, name), getattr(full, name)), (want, name)
            else:
                assert getattr(m, name) is None, (want, name)
    for kw, what in ((dict(response=case["response"].cpu()), "response"), (dict(delays=case["delays"].cpu()), "delays")):
        with pytest.raises(ValueError, match=what):
            FN.waveform_loglike_network(**dict(case, **kw))


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _observation(Bn, T, seed, D=D_MODEL):
    """(data [B, D, T, 2], response [B, D, 2], delays [B, D], weights [B, D, T], freqs [T], taus), on the device."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(seed)
    taus = N.grid(FN.MATCH_JC + 1)
    data, w = torch.randn(Bn, D, T, 2, generator=g), 0.5 + torch.rand(Bn, D, T, generator=g)
    return (data.to(DEV), N._response(D, g, None)[:Bn].to(DEV), N._delays(D, g, taus)[:Bn].to(DEV), w.to(DEV),
            torch.linspace(20.0, 512.0, T).to(DEV), taus)


def _clear_maximum(ref, what):
    live = ~ref["degenerate"]
    top = ref["x"][live].topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1]) / (ref["hh"] * ref["dd_rows"]).sqrt()[live]
    assert float(gap.min()) >= 1e-6, f"{what}: the inputs leave tau_index ill posed"


def _predict(name, n_trgt=None):
    case = MODELS[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    torch.manual_seed(9)
    post = model.condition(Xc, Yc)
    return case, post, Xt, post.query(Xt, n_trgt=n_trgt)


@pytest.mark.parametrize("name", list(MODELS))
def test_models_loglike_network_is_the_functional_call_and_meets_the_reference(name):
    import npf_gwwaveform_amd as A

    FN = A.functional
    case, post, Xt, p = _predict(name)
    Bn, T, n_z, D = case["B"], case["T"], case.get("n_z", 1), D_MODEL
    data, resp, dl, w, f, taus = _observation(Bn, T, 41)
    m = p.loglike_network(data, resp, dl, weights=w, freqs=f, taus=taus, series=True)
    plain = p.loglike_network(data, resp)
    mean = p.loglike_network(data, resp, dl, weights=w, freqs=f, taus=taus, of="mean")
    assert p._base is None and isinstance(m, A.NetworkLogLike)
    assert all(getattr(m, k).shape == (n_z, Bn) for k in ("optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau", "tau_index"))
    assert all(getattr(m, k).shape == (Bn,) for k in ("lnl", "lnl_max_mix", "dd"))
    assert m.snr_det.shape == (n_z, Bn, D) and m.optimal_snr_det.shape == (n_z, Bn, D) and m.dd_det.shape == (Bn, D)
    assert all(v.dtype == (torch.int32 if k == "tau_index" else torch.float64) for k, v in m._asdict().items())
    assert m.series.shape == (n_z, Bn, taus[2], 2)
    assert plain.tau is None and plain.tau_index is None and plain.series is None and plain.lnl_marg.shape == (n_z, Bn)
    assert mean.lnl_marg.shape == (1, Bn) and mean.series is None and mean.lnl.shape == (Bn,) and mean.snr_det.shape == (1, Bn, D)
    # bit for bit the functional call on the raw decoder output
    fn = FN.waveform_loglike_network(p._suff.reshape(n_z * Bn, T, 4), data, resp, dl, w, f, taus, series=True)
    for mine, theirs in (("snr", "snr"), ("lnl_max", "lnl_max"), ("lnl_marg", "lnl_marg"), ("phase", "phase"), ("tau_index", "tau_index"),
                         ("lnl", "lnl_mix"), ("lnl_max_mix", "lnl_max_mix"), ("dd", "dd"), ("series", "series"), ("snr_det", "snr_det"),
                         ("dd_det", "dd_det")):
        assert torch.equal(getattr(m, mine).reshape(-1), getattr(fn, theirs).reshape(-1)), mine
    assert torch.equal(m.optimal_snr.reshape(-1), fn.hh.sqrt())
    # and the float64 reference on the model's own loc / mixture mean
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2)
    ref = N.reference(loc, data, resp, dl, w, f, taus)
    _clear_maximum(ref, name)
    _check(_as_dict(m), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().view(-1), ref["tau"]), name
    _check(_as_dict(plain), N.reference(loc, data, resp), f"{name} without delays, weights and grid")
    ref_mean = N.reference(p.summary().mean, data, resp, dl, w, f, taus)
    _clear_maximum(ref_mean, name)
    _check(_as_dict(mean), ref_mean, f"{name} of=mean against summary().mean")
    assert torch.equal(mean.lnl, mean.lnl_marg[0]) and torch.equal(mean.lnl_max_mix, mean.lnl_max[0]), name
    if n_z == 1:  # a deterministic model: the marginal over the latent samples is the one row
        assert torch.equal(m.lnl, m.lnl_marg[0]) and torch.equal(m.lnl_max_mix, m.lnl_max[0]), name


def test_padded_targets_equal_the_cut_batch():
    counts = (37, 17, 5)
    n_trgt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    case, post, Xt, p = _predict("attnlnp", n_trgt=n_trgt)
    Bn, T, n_z = case["B"], case["T"], case["n_z"]
    data, resp, dl, w, f, taus = _observation(Bn, T, 43)
    data[1, :, 17:] = math.nan  # (nothing at or beyond a task's count is read)
    m = p.loglike_network(data, resp, dl, weights=w, freqs=f, taus=taus)
    assert all(torch.isfinite(v).all() for v in m if v is not None)
    loc = p.base_dist.loc.double().view(n_z, Bn, T, 2)
    for b, n in enumerate(counts):
        ref = N.reference(loc[:, b, :n], data[b:b + 1, :, :n], resp[b:b + 1], dl[b:b + 1], w[b:b + 1, :, :n], f[:n], taus)
        _clear_maximum(ref, f"task {b}")
        got = {k: getattr(m, k)[:, b] for k in ("optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau_index", "snr_det",
                                                "optimal_snr_det")}
        got.update(lnl_mix=m.lnl[b:b + 1], lnl_max_mix=m.lnl_max_mix[b:b + 1], dd=m.dd[b:b + 1], dd_det=m.dd_det[b:b + 1])
        _check(got, ref, f"padded task {b} against the batch cut to {n} points")


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike_network(torch.zeros(3, 2, 37, 2, device=DEV), torch.ones(3, 2, 2, dtype=torch.float64, device=DEV))


# ---- one captured query + loglike_network ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_query_and_loglike_network_replay_from_one_graph(name):
    """Delays and responses are overwritten in place between the replays and every replay meets the reference for its own: the
    host reads neither."""
    case, post, Xt, _ = _predict(name)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    d_s, c_s, dl_s, w_s, f, taus = _observation(Bn, T, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            post.query(Xt).loglike_network(d_s, c_s, dl_s, weights=w_s, freqs=f, taus=taus, series=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branches)
        p_g = post.query(Xt)
        m_g = p_g.loglike_network(d_s, c_s, dl_s, weights=w_s, freqs=f, taus=taus, series=True)
        loc_g = p_g.base_dist.loc
    seen = []
    for step in range(2):
        d_new, c_new, dl_new, w_new, _, _ = _observation(Bn, T, 100 + step)
        w_new[:, :, step::5] = 0.0  # (and some points removed)
        for dst, src in ((d_s, d_new), (c_s, c_new), (dl_s, dl_new), (w_s, w_new)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        ref = N.reference(loc_g.double().reshape(n_z * Bn, T, 2), d_new, c_new, dl_new, w_new, f, taus)
        _clear_maximum(ref, name)
        _check(_as_dict(m_g), ref, f"{name} replay {step}")
        seen.append(m_g.lnl_marg.clone())
    assert not torch.equal(seen[0], seen[1])
