"""Joint sky and distance marginal on the host (no GPU): the library's symbols and their signatures, the public surface, every
refusal before a launch, and the float64 reference of tests/loglike_sky_dist_reference.py -- its identities against the two parents'
references, an independent one-pass evaluation in the kernel's order below 0.1 of every gate, the well-posedness of the indices in
every input set of the GPU test (a condition of the sets, not a measurement), and four wrong evaluations that each miss a gate."""
import ctypes as C
import math

import pytest
import torch

import loglike_dist_reference as DR
import loglike_net_reference as N
import loglike_sky_dist_reference as J
import loglike_sky_reference as S
import npf_gwwaveform_amd as A
from npf_gwwaveform_amd import _lib
from npf_gwwaveform_amd import functional as FN

SETS = J.gpu_sets()


def test_the_library_exports_both_symbols_with_the_declared_signatures():
    lib = _lib.load()
    ws = lib.npf_waveform_loglike_sky_dist_workspace_bytes
    call = lib.npf_waveform_loglike_sky_dist
    assert ws.restype == C.c_int64 and len(ws.argtypes) == 6 and all(t == C.c_int32 for t in ws.argtypes)
    assert call.restype == C.c_int and len(call.argtypes) == 38
    assert list(call.argtypes[16:19]) == [C.c_double, C.c_double, C.c_int32] and call.argtypes[21] == C.c_int32
    assert ws(9, 3, 37, 7, 5, 5) > lib.npf_waveform_loglike_sky_workspace_bytes(9, 3, 37, 7, 5) > 0
    # refused sizes: -1; the largest accepted sizes stay inside int64
    assert ws(9, 3, 37, 7, 5, 0) == -1 and ws(9, 3, 37, 7, 5, FN.DIST_MAX_SCALES + 1) == -1 and ws(9, 3, 37, 0, 5, 5) == -1
    assert ws(9, 9, 37, 7, 5, 5) == -1 and 0 < ws(1 << 24, 1, 4, 65536, 65536, 4096) < 1 << 62
    assert lib.npf_version() == 2
    assert FN.SKYD_SC == J.SC


def test_the_public_surface_exists():
    assert hasattr(A.HeadDistribution, "loglike_sky_distance") and "SkyDistanceLogLike" in A.__all__
    assert A.SkyDistanceLogLike._fields == ("lnl", "lnl_vol", "pix_index", "scale_index", "scale_map", "tau_index", "tau", "snr",
                                            "scale_hat", "post_sky", "post_dist", "post_sky_mix", "post_dist_mix", "post_joint",
                                            "dist_mean", "dist_std")
    assert FN.LOGLIKE_SKY_DIST_NAMES == ("lnl_vol", "pix_index", "scale_index", "tau_index", "snr", "scale_hat", "lnl")


def test_every_refusal_is_a_value_error_before_any_launch():
    a = J.call_args(J.base_set())  # CPU tensors: a launch would be a RuntimeError, so a ValueError comes from the checks
    B = a["data"].shape[0]
    bad = [dict(scales=a["scales"].expand(B, -1).contiguous()), dict(log_prior_scale=a["log_prior_scale"].expand(B, -1).contiguous()),
           dict(scales=a["scales"].float()), dict(scales=a["scales"][:0], log_prior_scale=a["log_prior_scale"][:0]),
           dict(scales=a["scales"][:3]), dict(scales=None), dict(log_prior_scale=None),
           dict(scales=torch.ones(FN.DIST_MAX_SCALES + 1, dtype=torch.float64),
                log_prior_scale=torch.zeros(FN.DIST_MAX_SCALES + 1, dtype=torch.float64)),
           # what the sky call refuses
           dict(freqs=None), dict(freqs=a["freqs"].expand(B, -1).contiguous()), dict(response=a["response"].float()),
           dict(delays=a["delays"][:3]), dict(log_prior=a["log_prior"][:3]), dict(response=a["response"][:0], delays=a["delays"][:0]),
           dict(h=a["h"][:4]), dict(taus=(0.0, 1e-3, 0)), dict(want=("lnl_sky",)), dict(want="lnl_vol"), dict(want=())]
    for kw in bad:
        with pytest.raises(ValueError):
            FN.waveform_loglike_sky_distance(**dict(a, **kw))
    for name in ("h", "data", "scales", "log_prior_scale", "response", "log_prior"):  # inference only
        t = a[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="inference only"):
            FN.waveform_loglike_sky_distance(**dict(a, **{name: t}))
    with pytest.raises(ValueError):
        FN.check_loglike_sky_distance_args(a["h"].shape, a["data"], a["response"], a["delays"], a["scales"].view(1, -1), a["log_prior_scale"],
                                           a["log_prior"], a["weights"], a["freqs"], a["taus"])
    geo, n_a = FN.check_loglike_sky_distance_args(a["h"].shape, a["data"], a["response"], a["delays"], a["scales"], a["log_prior_scale"],
                                                  a["log_prior"], a["weights"], a["freqs"], a["taus"])
    assert n_a == 5 and geo[:6] == (9, 37, 2, 3, 3, 7)


def test_one_scale_of_one_is_the_sky_reference():
    case = J.base_set()
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    ref = J.reference(**dict(J.call_args(case), scales=one, log_prior_scale=zero))
    sky = ref["sky"]
    got = dict(lnl_sky=ref["lnl_vol"], pix_index=ref["pix_index"].int(), tau_index=ref["tau_index"].int(), snr=ref["snr"],
               lnl_sky_mix=ref["lnl"], post=ref["post_sky"], post_mix=ref["post_sky_mix"])
    q = S.ratios(got, sky)
    assert max(q.values()) <= 0.1, q
    assert (ref["post_dist"] == 0).all() and (ref["scale_index"] == 0).all()
    assert ((ref["dist_mean"] - 1).abs() <= 1e-15).all() and (ref["dist_std"] <= 1e-7).all()


def test_one_pixel_is_the_network_distance_reference():
    case = J.build(seed=310, **dict(J.BASE, P=1, n_a=9))
    a = J.call_args(case)
    ref = J.reference(**dict(a, log_prior=torch.zeros(1, dtype=torch.float64)))
    Bn = a["data"].shape[0]
    net = N.reference(a["h"], a["data"], a["response"].expand(Bn, -1, -1), a["delays"].expand(Bn, -1), a["weights"], a["freqs"], a["taus"])
    dist = DR.marginalise(net, a["scales"], a["log_prior_scale"])
    got = dict(lnl_dist=ref["lnl_vol"], post=ref["post_dist"], scale_index=ref["scale_index"].int(), scale_hat=ref["scale_hat"],
               lnl_dist_mix=ref["lnl"], post_mix=ref["post_dist_mix"])
    q = DR.ratios(got, net, dist)
    assert max(q.values()) <= 0.1, q


@pytest.mark.parametrize("tag,case", SETS, ids=[t for t, _ in SETS])
def test_reference_identities_one_pass_and_well_posed_indices(tag, case):
    ref = J.cached(tag, case)
    lse = lambda t, d: J._lse(t, d)  # noqa: E731
    live_rows = ref["lnl_vol"] > -math.inf
    for name, dims in (("post_sky", (1,)), ("post_dist", (1,)), ("post_joint", (1, 2))):
        assert (lse(ref[name], dims)[live_rows].abs() <= 1e-12).all(), (tag, name)
    for name in J.MIXES:
        assert (lse(ref[name], (1,)).abs() <= 1e-9).all(), (tag, name)
    d = (ref["post_sky"] - lse(ref["post_joint"], (2,)))
    assert (d[ref["post_sky"] > -math.inf].abs() <= 1e-12).all(), tag
    # float64 in the kernel's order stays below a tenth of every gate (the moments' included: the derivation holds)
    q = J.ratios(J.one_pass(ref, case["scales"], case["log_prior_scale"], case["log_prior"]), ref)
    assert max(q.values()) <= 0.1, (tag, q)
    lead_sky, lead_dist, lead_x = J.margins(ref)
    assert lead_sky >= 1e3 and lead_dist >= 1e3 and lead_x >= 1e-6, (tag, lead_sky, lead_dist, lead_x)


@pytest.mark.parametrize("kind", ("xstar", "aHH", "noprior", "separable"))
def test_a_wrong_evaluation_misses_a_gate(kind):
    case = J.base_set()
    ref = J.cached("base", case)
    bad = J.wrong(kind, case, sky=ref["sky"])
    got = {k: (bad[k].int() if k.endswith("index") else bad[k]) for k in FN.LOGLIKE_SKY_DIST_NAMES + J.POSTS + J.MIXES +
           ("dist_mean", "dist_std")}
    q = J.ratios(got, ref)
    assert max(q.values()) > 1.0, (kind, q)
    right = {k: (ref[k].int() if k.endswith("index") else ref[k]) for k in got}
    assert max(J.ratios(right, ref).values()) <= 1e-6  # (w = post_joint + lnl_vol rounds)
