"""Waveform match on the GPU: ``npf_waveform_match`` against the float64 reference of tests/match_reference.py (checked on the CPU by
tests/test_match_host.py) over its seven input regimes, bit-identical repeats, ``want`` subsets, ``HeadDistribution.match`` of a
deterministic and a latent model against the reference on their own ``base_dist`` / ``summary``, leave-one-out, and a captured
``query`` + ``match``.

Gates (match_reference.ratios): overlap, match, mismatch and every corr component |d| <= 1e-9 + 2^-23 |ref|; hh, gg |d| <= 2^-23 |ref|;
phase: the difference mod 2 pi <= 1e-6 where the reference's normalised |c| >= 1e-3; tau_index exact.  The 1e-9 is derived: double sums
of T <= 200 terms after at most JC rotation steps with ulp-level sines err by about (T + JC) 2^-52 ~ 1e-13 on the normalised
quantities, the direct and the recurrence form differ by less than 1e-12 on the CPU -- three orders of margin, while float32 sines
(2e-7 on these inputs) fail it; 2^-23 is one fp32 rounding with a factor 2.  Every test prints its worst error / gate ratio per
quantity."""
import math

import pytest
import torch

import match_reference as R
from test_hip_predict import ROUTES, _counts, _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def all_cases():
    from npf_gwwaveform_amd import functional as FN

    return [(tag, fac, case, R.reference(**R.call_args(case))) for tag, fac, case in R.cases(FN.MATCH_JC)]


def _dev(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.call_args(case).items()}


def _check(got, ref, what, worst=None):
    r = R.ratios(got, ref)
    print(f"MATCH {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
    return r


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.REGIMES)
def test_waveform_match_meets_the_float64_reference(regime, all_cases):
    from npf_gwwaveform_amd import functional as FN

    worst, n = {}, 0
    for tag, fac, case, ref in all_cases:
        if fac["regime"] != regime:
            continue
        n += 1
        args = _dev(case)
        got = FN.waveform_match(**args, corr=True)
        again = FN.waveform_match(**args, corr=True)
        for name, a, b in zip(got._fields, got, again):
            assert torch.equal(a, b), f"{tag}: {name} differs between two calls"
        got = {k: v.cpu() for k, v in got._asdict().items()}
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        assert got["corr"].shape == (fac["n_z"] * R.B, max(fac["n_tau"] or 0, 1), 2) and got["gg"].shape == (R.B,), tag
        _check(got, ref, tag, worst)
        live, deg = ~ref["degenerate"], ref["degenerate"]
        for name, value in (("overlap", 0.0), ("match", 0.0), ("mismatch", 1.0), ("tau_index", 0), ("phase", 0.0)):
            assert (got[name][deg] == value).all(), (tag, name)
        assert (got["corr"][deg] == 0).all(), tag
        if regime == "same":
            assert (got["overlap"][live] == 1).all() and (got["match"][live] == 1).all(), tag
            assert (got["mismatch"][live].abs() <= 1e-9).all() and (got["phase"][live].abs() <= 1e-6).all(), tag
        if regime == "shift":
            assert (got["tau_index"][live] == case["j_star"]).all(), tag
            assert (got["mismatch"][live].abs() <= 1e-6).all(), tag
        if regime == "offset":
            assert (got["match"][live] == 1).all() and (got["mismatch"][live].abs() <= 1e-9).all(), tag
            assert ((got["overlap"][live] - math.cos(R.PHI0)).abs() <= 1e-5).all() and ((got["phase"][live] - R.PHI0).abs() <= 1e-5).all(), tag
        if regime == "degenerate" and fac["wform"] == "T":
            assert deg.all(), tag
    assert n >= 14
    print(f"MATCH worst over the {n} cases of regime {regime}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_full_counts_and_unit_weights_equal_the_plain_call_bit_for_bit():
    from npf_gwwaveform_amd import functional as FN

    T = 200
    case = _dev(R.build("random", T, n_z=3, h_ld=4, wform=None, fform="BT", taus=R.grid(FN.MATCH_JC + 1), seed=3))
    plain = FN.waveform_match(**case, corr=True)
    full = FN.waveform_match(**dict(case, n_valid=torch.full((R.B,), T, dtype=torch.int64, device=DEV),
                                    weights=torch.ones(T, device=DEV)), corr=True)
    over = FN.waveform_match(**dict(case, n_valid=torch.tensor([T + 5, 1 << 30, T], device=DEV)), corr=True)  # (clamped to T)
    for name, a, b, c in zip(plain._fields, plain, full, over):
        assert torch.equal(a, b) and torch.equal(a, c), name


# ---- want ---------------------------------------------------------------------------------------------------------------------------
def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    case = _dev(R.build("random", 37, n_z=3, h_ld=2, wform="BT", fform="T", taus=R.grid(5), counts=(37, 17, 0), seed=9))
    full = FN.waveform_match(**case, corr=True)
    assert full.tau_index.dtype == torch.int32 and all(t is not None for t in full)
    for want, corr in ((("mismatch",), False), (("hh", "gg"), False), (["tau_index", "phase"], True), ((), True), (("match", "overlap"), False)):
        m = FN.waveform_match(**case, want=want, corr=corr)
        for name in m._fields:
            if name in want or (name == "corr" and corr):
                assert torch.equal(getattr(m, name), getattr(full, name)), (want, name)
            else:
                assert getattr(m, name) is None, (want, name)
    with pytest.raises(ValueError, match="want"):
        FN.waveform_match(**case, want=())


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _observation(case, seed):
    """(Y_ref [B, T, 2] with a positive amplitude, weights [B, T], freqs [T], taus) for a model case."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(seed)
    Bn, T = case["B"], case["T"]
    Y = torch.stack([0.5 + torch.rand(Bn, T, generator=g), 3.0 * torch.randn(Bn, T, generator=g)], -1)
    return Y.to(DEV), (0.5 + torch.rand(Bn, T, generator=g)).to(DEV), torch.linspace(20.0, 512.0, T).to(DEV), R.grid(FN.MATCH_JC + 1)


def _clear_maximum(ref, what):
    top = ref["mag"][~ref["degenerate"]].topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-6, f"{what}: the inputs leave tau_index ill posed"


@pytest.mark.parametrize("name,latent", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True)])
def test_models_match_equals_the_reference_on_their_own_loc_and_mean(name, latent):
    import npf_gwwaveform_amd as A

    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    Y, w, f, taus = _observation(case, 41)
    n_trgt = _counts(Bn, T, 6, T // 2) if latent else None
    torch.manual_seed(9)
    if latent:
        p = model.condition(Xc, Yc).query(Xt, n_trgt=n_trgt)
    else:
        with torch.no_grad():
            p = model(Xc, Yc, Xt)[0]
    m = p.match(Y, weights=w, freqs=f, taus=taus, corr=True)
    plain = p.match(Y)
    mean = p.match(Y, weights=w, freqs=f, taus=taus, of="mean")
    assert p._base is None and isinstance(m, A.Match)
    assert all(getattr(m, k).shape == (n_z, Bn) for k in ("overlap", "match", "mismatch", "tau", "tau_index", "phase"))
    assert m.corr.shape == (n_z, Bn, taus[2], 2) and m.tau.dtype == torch.float64 and m.tau_index.dtype == torch.int32
    assert plain.tau is None and plain.tau_index is None and plain.corr is None and plain.match.shape == (n_z, Bn)
    assert mean.match.shape == (1, Bn) and mean.corr is None
    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2)
    ref = R.reference(loc, Y, w, f, taus, n_trgt)
    _clear_maximum(ref, name)
    _check(m._asdict(), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().view(-1), ref["tau"]), name
    _check(plain._asdict(), R.reference(loc, Y, n_valid=n_trgt), f"{name} without weights and grid")
    ref_mean = R.reference(p.summary().mean, Y, w, f, taus, n_trgt)
    _clear_maximum(ref_mean, name)
    _check(mean._asdict(), ref_mean, f"{name} of=mean against summary().mean")


def test_leave_one_out_match_runs():
    case = ROUTES["attncnp_r128_c128"]
    model, Xc, Yc, _ = _model_and_inputs(case)
    Bn, C = case["B"], case["C"]
    p = model.loo(Xc, Yc)
    w = torch.linspace(0.5, 1.5, C).to(DEV)
    m = p.match(Yc, weights=w)
    assert m.match.shape == (1, Bn) and torch.isfinite(m.match).all() and torch.isfinite(m.mismatch).all()
    _check(m._asdict(), R.reference(p.base_dist.loc.double().reshape(Bn, C, 2), Yc, w), "loo against base_dist.loc")


# ---- one captured query + match ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_n_cntxt", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True)])
def test_query_and_match_replay_from_one_graph(name, with_n_cntxt):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, C, T, n_z = case["B"], case["C"], case["T"], case.get("n_z", 1)
    torch.manual_seed(23)
    post = model.condition(Xc, Yc, **(dict(n_cntxt=_counts(Bn, C, 5, C)) if with_n_cntxt else {}))
    Y_s, w_s, f, taus = _observation(case, 1)
    n_s = torch.full((Bn,), T, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            post.query(Xt, n_trgt=n_s).match(Y_s, weights=w_s, freqs=f, taus=taus, corr=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p_g = post.query(Xt, n_trgt=n_s)
        m_g = p_g.match(Y_s, weights=w_s, freqs=f, taus=taus, corr=True)
        loc_g = p_g.base_dist.loc
    for step in range(3):
        Y_new, w_new, _, _ = _observation(case, 100 + step)
        w_new[:, step::5] = 0.0  # (and some points removed)
        n_new = torch.randint(1, T + 1, (Bn,), generator=torch.Generator().manual_seed(step), dtype=torch.int32).to(DEV)
        Y_s.copy_(Y_new)
        w_s.copy_(w_new)
        n_s.copy_(n_new)
        graph.replay()
        torch.cuda.synchronize()
        ref = R.reference(loc_g.double().reshape(n_z * Bn, T, 2), Y_new, w_new, f, taus, n_new)
        _clear_maximum(ref, name)
        _check(m_g._asdict(), ref, f"{name} replay {step}")
        assert torch.equal(m_g.tau.cpu().view(-1), ref["tau"]), (name, step)
        eager = post.query(Xt, n_trgt=n_new).match(Y_new, weights=w_new, freqs=f, taus=taus, corr=True)
        for a, b in zip(m_g, eager):
            assert torch.equal(a, b), (name, step)
