"""Matched-filter log likelihood on the GPU: ``npf_waveform_loglike`` against the float64 reference of tests/loglike_reference.py
(checked on the CPU by tests/test_loglike_host.py) over its eight input regimes, bit-identical repeats into NaN-filled outputs,
``HeadDistribution.loglike`` of a latent and a deterministic model, padded targets, a captured ``query`` + ``loglike`` and the
refusals of the C ABI.

Gates (loglike_reference.ratios): lnl_max, lnl_marg, lnl_mix, lnl_max_mix and the series' L_j |d| <= 1e-10 (sqrt(hh dd) + hh / 2) +
1e-12; hh, dd 2^-50 relative; snr, optimal_snr, series SNR 1e-10 relative + 1e-12; phase: the difference mod 2 pi <= 1e-9 where
x* >= 1e-3 sqrt(hh dd); tau_index exact.  The 1e-10 is derived: double sums over at most 200 terms, a 16-step rotation and a sincos
argument of up to 1e4 rad cost about 1e-12 of the terms' scale sqrt(hh dd) + hh / 2 -- tests/test_loglike_host.py measures that between
the recurrence and the direct form -- and the gate is 100 times that.  The mixtures over the latent samples take the largest scale
among the task's rows.  Every test prints its worst error / gate ratio per quantity."""
import ctypes as C
import math

import pytest
import torch

import loglike_reference as R
from test_hip_dispatch import _c
from test_hip_predict import _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_ROW = ("hh", "snr", "lnl_max", "lnl_marg", "tau_index", "phase")
MODELS = {"attnlnp": _c("AttnLNP", 64, 20, n_z=3, B=3, T=37), "cnp": _c("CNP", 64, 20, B=3, T=37)}


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    return [(tag, fac, case, R.reference(**R.call_args(case))) for tag, fac, case in R.cases(FN.MATCH_JC, FN.LOGLIKE_I0_SWITCH)]


def _dev(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.call_args(case).items()}


def _check(got, ref, what, worst=None):
    r = R.ratios(got, ref)
    print(f"LOGLIKE {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
    return r


def _as_dict(m):
    d = {k: v for k, v in m._asdict().items() if v is not None}
    if "hh" in d and "optimal_snr" not in d:
        d["optimal_snr"] = d["hh"].sqrt()
    if "lnl" in d:
        d["lnl_mix"] = d.pop("lnl")
    return d


def _raw_call(args, fill=math.nan):
    """``npf_waveform_loglike`` through the C ABI into outputs filled with NaN (tau_index: -1) -> dict of the outputs."""
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    h, d, w, f, taus, nv = (args[k] for k in ("h", "data", "weights", "freqs", "taus", "n_valid"))
    Rn, T, ld = h.shape
    Bn = d.shape[0]
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 0)
    lib = L.load()
    ws = torch.full((lib.npf_waveform_loglike_workspace_bytes(Rn, n_tau) // 8,), math.nan, dtype=torch.float64, device=DEV)
    out = {k: torch.full((Bn if k in ("dd", "lnl_mix", "lnl_max_mix") else Rn,), fill, dtype=torch.float64, device=DEV)
           for k in FN.LOGLIKE_NAMES if k != "tau_index"}
    out["tau_index"] = torch.full((Rn,), -1, dtype=torch.int32, device=DEV)
    out["series"] = torch.full((Rn, max(n_tau, 1), 2), fill, dtype=torch.float64, device=DEV)
    rows = lambda t: 1 if t is None or t.dim() == 1 else Bn  # noqa: E731
    nv32 = nv.to(torch.int32) if nv is not None else None
    rc = lib.npf_waveform_loglike(h.data_ptr(), ld, d.data_ptr(), L.ptr(w), rows(w), L.ptr(f) if n_tau > 0 else None, rows(f),
                                  nv32.data_ptr() if nv32 is not None else None, Rn, Bn, T, tau0, dtau, n_tau,
                                  *(out[k].data_ptr() for k in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series",
                                                                "lnl_mix", "lnl_max_mix")), ws.data_ptr(), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.REGIMES)
def test_waveform_loglike_meets_the_float64_reference(regime, all_cases):
    """Every case of the regime (none is skipped): the gates; a second call, through the C ABI into NaN-filled outputs and a
    NaN-filled workspace, gives the same bits and nothing but finite values; degenerate rows hold the stated zeros; the planted
    index is found."""
    from npf_gwwaveform_amd import functional as FN

    worst, n = {}, 0
    for tag, fac, case, ref in all_cases:
        if fac["regime"] != regime:
            continue
        n += 1
        args = _dev(case)
        got = FN.waveform_loglike(**args, series=True)
        raw = _raw_call(args)
        for name, a in got._asdict().items():
            assert a is not None and torch.equal(a, raw[name]), f"{tag}: {name} differs between two calls"
        got = {k: v.cpu() for k, v in got._asdict().items()}
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        assert all(v.dtype == (torch.int32 if k == "tau_index" else torch.float64) for k, v in got.items()), tag
        Rn, n_grid = fac["n_z"] * R.B, max(fac["n_tau"] or 0, 1)
        assert got["series"].shape == (Rn, n_grid, 2) and got["dd"].shape == (R.B,) and got["lnl_mix"].shape == (R.B,), tag
        assert all(got[k].shape == (Rn,) for k in PER_ROW), tag
        _check(_as_dict(FN.WaveformLogLike(**got)), ref, tag, worst)
        deg = ref["degenerate"]
        for name in ("snr", "lnl_max", "lnl_marg", "tau_index", "phase"):
            assert (got[name][deg] == 0).all(), (tag, name)
        assert (got["series"][deg] == 0).all() and (got["hh"][deg] == 0).all(), tag
        if regime == "planted":
            assert (got["tau_index"][~deg] == case["j_star"]).all(), tag
        if regime == "degenerate" and fac["wform"] == "T":
            assert deg.all() and (got["lnl_mix"] == 0).all() and (got["lnl_max_mix"] == 0).all(), tag
    assert n >= 14
    print(f"LOGLIKE worst over the {n} cases of regime {regime}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    case = _dev(R.build("noise", 37, n_z=3, h_ld=4, wform="BT", fform="T", taus=R.grid(FN.MATCH_JC + 1), counts=(37, 17, 0), seed=9))
    full = FN.waveform_loglike(**case, series=True)
    for want, series in ((("lnl_mix",), False), (("hh", "dd"), False), (["tau_index", "phase"], True), ((), True), (("lnl_max_mix", "snr"), False)):
        m = FN.waveform_loglike(**case, want=want, series=series)
        for name in m._fields:
            if name in want or (name == "series" and series):
                assert torch.equal(getattr(m, name), getattr(full, name)), (want, name)
            else:
                assert getattr(m, name) is None, (want, name)
    over = FN.waveform_loglike(**dict(case, n_valid=torch.tensor([37 + 5, 17, 0], device=DEV)), series=True)  # (clamped to T)
    for name, a, b in zip(full._fields, full, over):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("n_tau", (None, 17))
def test_removing_points_equals_cutting_them_on_the_device(n_tau):
    """A third of the points removed by their weights (NaN planted there) against the same inputs with those points cut away: both
    meet the reference of the cut inputs, and the index is the same."""
    from npf_gwwaveform_amd import functional as FN

    case = R.build("removed", 200, n_z=3, h_ld=4, wform="T", fform="T" if n_tau else None, taus=R.grid(n_tau), seed=5,
                   x_s=FN.LOGLIKE_I0_SWITCH)
    ref = R.reference(**R.cut(case))
    full = FN.waveform_loglike(**_dev(case), series=True)
    short = FN.waveform_loglike(**_dev(R.cut(case)), series=True)
    assert all(torch.isfinite(v).all() for v in full), n_tau
    assert torch.equal(full.tau_index, short.tau_index)
    _check(_as_dict(full), ref, f"removed n_tau={n_tau}")
    _check(_as_dict(short), ref, f"cut n_tau={n_tau}")


def test_mixture_of_rows_more_than_745_apart_is_the_maximum_minus_log_n_z():
    from npf_gwwaveform_amd import functional as FN

    case = R.build("loud", 200, n_z=3, h_ld=2, wform="T", fform="T", taus=R.grid(FN.MATCH_JC + 1), j_star=2, seed=1,
                   x_s=FN.LOGLIKE_I0_SWITCH)
    got = FN.waveform_loglike(**_dev(case))
    for mix, rows in ((got.lnl_mix, got.lnl_marg), (got.lnl_max_mix, got.lnl_max)):
        top = rows.view(3, R.B).sort(0, descending=True).values
        assert float((top[0] - top[1]).min()) > 745
        want = top[0] - math.log(3)
        assert torch.isfinite(mix).all() and float(((mix - want).abs() / want.abs()).max()) <= 1e-12


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _observation(Bn, T, seed):
    """(data [B, T, 2] Gaussian (Re, Im), weights [B, T], freqs [T], taus)."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(seed)
    data = torch.randn(Bn, T, 2, generator=g)
    return data.to(DEV), (0.5 + torch.rand(Bn, T, generator=g)).to(DEV), torch.linspace(20.0, 512.0, T).to(DEV), R.grid(FN.MATCH_JC + 1)


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
def test_models_loglike_is_the_functional_call_and_meets_the_reference(name):
    import npf_gwwaveform_amd as A

    FN = A.functional
    case, post, Xt, p = _predict(name)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    data, w, f, taus = _observation(Bn, T, 41)
    m = p.loglike(data, weights=w, freqs=f, taus=taus, series=True)
    plain = p.loglike(data)
    mean = p.loglike(data, weights=w, freqs=f, taus=taus, of="mean")
    assert p._base is None and isinstance(m, A.LogLike)
    assert all(getattr(m, k).shape == (n_z, Bn) for k in ("optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau", "tau_index"))
    assert all(getattr(m, k).shape == (Bn,) for k in ("lnl", "lnl_max_mix", "dd"))
    assert all(v.dtype == (torch.int32 if k == "tau_index" else torch.float64) for k, v in m._asdict().items())
    assert m.series.shape == (n_z, Bn, taus[2], 2)
    assert plain.tau is None and plain.tau_index is None and plain.series is None and plain.lnl_marg.shape == (n_z, Bn)
    assert mean.lnl_marg.shape == (1, Bn) and mean.series is None and mean.lnl.shape == (Bn,)
    # bit for bit the functional call on the raw decoder output
    fn = FN.waveform_loglike(p._suff.reshape(n_z * Bn, T, 4), data, w, f, taus, series=True)
    for mine, theirs in (("snr", "snr"), ("lnl_max", "lnl_max"), ("lnl_marg", "lnl_marg"), ("phase", "phase"), ("tau_index", "tau_index"),
                         ("lnl", "lnl_mix"), ("lnl_max_mix", "lnl_max_mix"), ("dd", "dd"), ("series", "series")):
        assert torch.equal(getattr(m, mine).reshape(-1), getattr(fn, theirs).reshape(-1)), mine
    assert torch.equal(m.optimal_snr.reshape(-1), fn.hh.sqrt())
    # and the float64 reference on the model's own loc / mixture mean
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2)
    ref = R.reference(loc, data, w, f, taus)
    _clear_maximum(ref, name)
    _check(_as_dict(m), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().view(-1), ref["tau"]), name
    _check(_as_dict(plain), R.reference(loc, data), f"{name} without weights and grid")
    ref_mean = R.reference(p.summary().mean, data, w, f, taus)
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
    data, w, f, taus = _observation(Bn, T, 43)
    data[1, 17:] = math.nan  # (nothing at or beyond a task's count is read)
    m = p.loglike(data, weights=w, freqs=f, taus=taus)
    assert all(torch.isfinite(v).all() for v in m if v is not None)
    loc = p.base_dist.loc.double().view(n_z, Bn, T, 2)
    for b, n in enumerate(counts):
        ref = R.reference(loc[:, b, :n], data[b:b + 1, :n], w[b:b + 1, :n], f[:n], taus)
        _clear_maximum(ref, f"task {b}")
        got = {k: getattr(m, k)[:, b] for k in ("optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau_index")}
        got.update(lnl_mix=m.lnl[b:b + 1], lnl_max_mix=m.lnl_max_mix[b:b + 1], dd=m.dd[b:b + 1])
        _check(got, ref, f"padded task {b} against the batch cut to {n} points")


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    with pytest.raises(ValueError, match="y_dim"):
        p.loglike(torch.zeros(3, 37, 2, device=DEV))


# ---- one captured query + loglike --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_query_and_loglike_replay_from_one_graph(name):
    case, post, Xt, _ = _predict(name)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    d_s, w_s, f, taus = _observation(Bn, T, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            post.query(Xt).loglike(d_s, weights=w_s, freqs=f, taus=taus, series=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream, no parallel branches)
        p_g = post.query(Xt)
        m_g = p_g.loglike(d_s, weights=w_s, freqs=f, taus=taus, series=True)
        loc_g = p_g.base_dist.loc
    for step in range(2):
        d_new, w_new, _, _ = _observation(Bn, T, 100 + step)
        w_new[:, step::5] = 0.0  # (and some points removed)
        d_s.copy_(d_new)
        w_s.copy_(w_new)
        graph.replay()
        torch.cuda.synchronize()
        ref = R.reference(loc_g.double().reshape(n_z * Bn, T, 2), d_new, w_new, f, taus)
        _clear_maximum(ref, name)
        _check(_as_dict(m_g), ref, f"{name} replay {step}")
        eager = post.query(Xt).loglike(d_new, weights=w_new, freqs=f, taus=taus, series=True)
        for k, a, b in zip(m_g._fields, m_g, eager):
            assert torch.equal(a, b), (name, step, k)


# ---- the C ABI on device pointers --------------------------------------------------------------------------------------------------
def test_c_abi_refuses_what_the_contract_lists():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    for n_tau, slots in ((0, 16), (5, 16), (17, 32), (257, 17 * 16)):
        assert lib.npf_waveform_loglike_workspace_bytes(6, n_tau) == 6 * (4 + 2 * slots) * 8
    f32 = torch.ones(6 * 4 * 2, device=DEV)
    f64 = torch.full((6 * 3 * 2,), math.nan, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.npf_waveform_loglike_workspace_bytes(6, 3) // 8, dtype=torch.float64, device=DEV)
    p, q = f32.data_ptr(), f64.data_ptr()
    ok = dict(h=p, h_ld=2, d=p, wgt=p, wgt_rows=1, freq=p, freq_rows=1, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
              n_tau=3, hh=q, dd=q, snr=q, lnl_max=q, lnl_marg=q, tau_index=q, phase=q, series=q, lnl_mix=q, lnl_max_mix=q,
              workspace=ws.data_ptr())
    none = {k: None for k in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix", "lnl_max_mix")}
    for change in (dict(n_rows=5), dict(n_tau=65537), dict(freq=None), none):
        assert lib.npf_waveform_loglike(*dict(ok, **change).values(), L.stream_ptr()) == -1, change
    torch.cuda.synchronize()
    assert torch.isnan(f64).all()  # nothing was launched
    assert lib.npf_waveform_loglike(*dict(ok, **dict(none, lnl_mix=q)).values(), L.stream_ptr()) == 0  # one output is enough
    torch.cuda.synchronize()
    assert torch.isfinite(f64[:2]).all() and torch.isnan(f64[2:]).all()  # ... and only that one is written
