"""The float64 reference of the sky-grid likelihood (tests/loglike_sky_reference.py) and the host side of
``functional.waveform_loglike_sky``, on the CPU: every pixel of the reference is the network reference called with that pixel's
response and delays; every input set of the GPU test leaves ``pix_index`` and ``tau_index`` well posed; the three wrong evaluations
exceed the gates; ``check_loglike_sky_args`` accepts what fits and raises on what does not."""
import math

import pytest
import torch

import loglike_net_reference as N
import loglike_sky_reference as S


@pytest.fixture(scope="module")
def sets():
    from npf_gwwaveform_amd import functional as FN

    return [(tag, case, S.reference(**S.call_args(case))) for tag, case in S.gpu_sets(FN.SKY_JC)]


def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp(min=1e-300)).max()) if a.numel() else 0.0


@pytest.mark.parametrize("which", ("combined 33 x 40 x 3 x 129 x 17", "dead points", "n_tau=None", "D=8"))
def test_every_pixel_is_the_network_reference_with_that_pixels_response_and_delays(which, sets):
    """u_p = lnl_marg + log_prior_p, snr_map and the first index of max_j x of pixel p against ``loglike_net_reference.reference``
    with pixel p's response and delays broadcast over the tasks: 1e-12 relative."""
    (case, ref), = [(c, r) for tag, c, r in sets if tag == which]
    a = S.call_args(case)
    Bn, P = a["data"].shape[0], a["response"].shape[0]
    lp = ref["u"].new_full((P,), -math.log(P)) if a["log_prior"] is None else a["log_prior"]
    worst = 0.0
    for p in range(P):
        net = N.reference(a["h"], a["data"], a["response"][p].expand(Bn, -1, -1), a["delays"][p].expand(Bn, -1), a["weights"], a["freqs"],
                          a["taus"], a["n_valid"])
        worst = max(worst, _rel(ref["u"][:, p], net["lnl_marg"] + lp[p]), _rel(ref["snr_map"][:, p], net["snr"]))
        assert torch.equal(ref["tau_map"][:, p], net["tau_index"]), (which, p)
    print(f"SKY host {which}: pixels against the network reference, worst relative difference {worst:.3g}")
    assert worst <= 1e-12


def test_every_set_of_the_gpu_test_is_well_posed(sets):
    """The best pixel's u leads the runner-up by >= 1e3 gates and at the best pixel the best x_j leads by >= 1e-6 relative; the
    planted pixel and grid time are the ones found."""
    low_u, low_x = math.inf, math.inf
    for tag, case, ref in sets:
        lead_u, lead_x = S.margins(ref)
        low_u, low_x = min(low_u, lead_u), min(low_x, lead_x)
        assert lead_u >= 1e3 and lead_x >= 1e-6, (tag, lead_u, lead_x)
        loud = torch.ones_like(ref["pix_index"], dtype=torch.bool)
        if tag == "ln I0 regimes":  # (the quietest task, x = 0.1 at the peak, follows the prior: well posed, but not planted)
            loud = torch.arange(loud.numel()) % 4 != 0
        assert (ref["pix_index"][loud] == case["p0"]).all() and (ref["tau_index"][loud] == case["j0"]).all(), tag
        assert all(torch.isfinite(ref[k]).all() for k in ("u", "lnl_sky", "lnl_sky_mix", "post", "post_mix", "snr", "snr_map")), tag
    print(f"SKY host margins over {len(sets)} sets: smallest lead of u {low_u:.3g} gates, smallest relative lead of x {low_x:.3g}")


def test_the_regime_set_puts_x_on_both_sides_of_the_switch_point(sets):
    from npf_gwwaveform_amd import functional as FN

    (ref,) = [r for tag, _, r in sets if tag == "ln I0 regimes"]
    x, x_s = ref["x"][:4], FN.LOGLIKE_I0_SWITCH  # the first latent sample of the four tasks
    assert float(x[0].max()) < 1.0 and float(x[1].max()) < x_s  # below
    assert float(x[2].max()) > x_s and float(x[2].min()) < x_s  # across
    assert float(x[3].max()) > 1e5 and float(x[3].max()) < 1e7  # far above


@pytest.mark.parametrize("kind", ("incoherent", "sign", "shared"))
def test_wrong_evaluations_exceed_the_gates(kind, sets):
    worst = 0.0
    for tag, case, ref in sets:
        if tag not in ("combined 33 x 40 x 3 x 129 x 17", "base", "D=2"):
            continue
        bad = S.wrong(kind, **S.call_args(case))
        r = S.ratios({k: bad[k] for k in S.DOUBLES}, ref)
        worst = max(worst, max(r.values()))
    print(f"SKY host wrong[{kind}]: worst error / gate {worst:.3g}")
    assert worst > 1.0


def test_the_reference_meets_its_own_gates_and_ratios_sees_what_it_must(sets):
    tag, case, ref = sets[0]
    same = {k: ref[k].clone() for k in S.DOUBLES + ("pix_index", "tau_index")}
    assert max(S.ratios(same, ref).values()) <= 1e-3  # (u = post + lnl_sky rounds once more)
    same["post"][0, 0] = -math.inf  # a finite value lost
    assert S.ratios(same, ref)["post"] == math.inf
    dead = dict(case, log_prior=torch.full((case["response"].shape[0],), -math.inf, dtype=torch.float64))
    none = S.reference(**S.call_args(dead))
    assert (none["lnl_sky"] == -math.inf).all() and (none["post"] == -math.inf).all() and (none["pix_index"] == 0).all()
    assert (none["snr"] == 0).all() and (none["snr_map"] == 0).all() and (none["lnl_sky_mix"] == -math.inf).all()
    got = {k: none[k].clone() for k in S.DOUBLES}
    assert max(S.ratios(got, none).values()) == 0.0
    got["lnl_sky"][0] = 0.0  # -inf is met by -inf only
    assert S.ratios(got, none)["lnl_sky"] == math.inf


def test_check_loglike_sky_args_accepts_the_good_shapes_and_raises_on_each_bad_one():
    from npf_gwwaveform_amd import functional as FN

    R, T, B, D, P = 6, 37, 3, 2, 5
    f64 = torch.float64
    good = dict(data=torch.zeros(B, D, T, 2), response=torch.zeros(P, D, 2, dtype=f64), delays=torch.zeros(P, D, dtype=f64),
                log_prior=torch.zeros(P, dtype=f64), weights=torch.ones(B, D, T), freqs=torch.ones(T), taus=(0.0, 1e-3, 9))
    assert FN.check_loglike_sky_args((R, T, 4), **good) == (R, T, 4, B, D, P, B, 0.0, 1e-3, 9)
    assert FN.check_loglike_sky_args((R, T, 2), **dict(good, weights=torch.ones(D, T), log_prior=None, taus=None)) == \
        (R, T, 2, B, D, P, 1, 0.0, 0.0, 0)
    assert FN.check_loglike_sky_args((R, T, 2), **dict(good, weights=None))[6] == 1
    bad = dict(freqs_per_task=dict(freqs=torch.ones(B, T)), no_freqs=dict(freqs=None), no_pixels=dict(
        response=torch.zeros(0, D, 2, dtype=f64), delays=torch.zeros(0, D, dtype=f64), log_prior=None),
        too_many_pixels=dict(response=torch.zeros(FN.SKY_MAX_PIX + 1, D, 2, dtype=f64), delays=torch.zeros(FN.SKY_MAX_PIX + 1, D, dtype=f64),
                             log_prior=None),
        nine_detectors=dict(data=torch.zeros(B, 9, T, 2), response=torch.zeros(P, 9, 2, dtype=f64), delays=torch.zeros(P, 9, dtype=f64),
                            weights=None),
        response_fp32=dict(response=torch.zeros(P, D, 2)), response_per_task=dict(response=torch.zeros(B, P, D, 2, dtype=f64)),
        delays_fp32=dict(delays=torch.zeros(P, D)), delays_shape=dict(delays=torch.zeros(P, D + 1, dtype=f64)),
        delays_none=dict(delays=None), prior_fp32=dict(log_prior=torch.zeros(P)), prior_shape=dict(log_prior=torch.zeros(P + 1, dtype=f64)),
        weights_shape=dict(weights=torch.ones(T)), data_shape=dict(data=torch.zeros(B, D, T + 1, 2)), data_3d=dict(data=torch.zeros(B, T, 2)),
        taus_tensor=dict(taus=torch.zeros(3)), taus_empty=dict(taus=(0.0, 1e-3, 0)))
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            FN.check_loglike_sky_args((R, T, 2), **dict(good, **kw))
        assert what
    for shape in ((R, T, 1), (R, T), (R + 1, T, 2), (0, T, 2)):
        with pytest.raises(ValueError):
            FN.check_loglike_sky_args(shape, **good)
    assert FN.LOGLIKE_SKY_NAMES == ("lnl_sky", "pix_index", "tau_index", "snr", "lnl_sky_mix")
    assert FN.WaveformLogLikeSky._fields == FN.LOGLIKE_SKY_NAMES + ("post", "post_mix", "snr_map")
    with pytest.raises(ValueError, match="want"):
        FN.waveform_loglike_sky(torch.zeros(R, T, 2), **good, want=("hh",))
    with pytest.raises(RuntimeError, match="fp32 device tensors"):
        FN.waveform_loglike_sky(torch.zeros(R, T, 2), **good)


def test_the_header_and_the_python_constants_agree():
    import os

    from npf_gwwaveform_amd import functional as FN

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "npf_hip.h")).read()
    assert f"#define NPF_SKY_JC {FN.SKY_JC}\n" in hdr and f"#define NPF_SKY_MAX_PIX {FN.SKY_MAX_PIX}\n" in hdr
    lib = __import__("npf_gwwaveform_amd._lib", fromlist=["load"]).load()
    assert lib.npf_waveform_loglike_sky_workspace_bytes(64, 3, 1024, 768, 64) > 0
    for args in ((0, 3, 8, 8, 8), (8, 0, 8, 8, 8), (8, 9, 8, 8, 8), (8, 3, 0, 8, 8), (8, 3, 8, 0, 8), (8, 3, 8, FN.SKY_MAX_PIX + 1, 8),
                 (8, 3, 8, 8, -1), (8, 3, 8, 8, 65537)):
        assert lib.npf_waveform_loglike_sky_workspace_bytes(*args) == -1, args
    # the largest sizes the call takes stay in int64
    assert 0 < lib.npf_waveform_loglike_sky_workspace_bytes(1 << 24, 8, 2 ** 31 - 1, FN.SKY_MAX_PIX, 65536) < 2 ** 63
