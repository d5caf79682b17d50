"""Differentiable matched-filter likelihood on the GPU: ``npf_waveform_loglike_bwd`` / ``npf_waveform_loglike_net_bwd`` against the
float64 closed form of tests/loglike_grad_reference.py (checked on the CPU by tests/test_loglike_grad_host.py against central
differences in 50 digits) over the regimes of the forward suites and every upstream combination, the edges of the two new kernels,
known values, the bit-for-bit promises, ``HeadDistribution.lnl`` of a deterministic and a latent model down to the parameter
gradients, ``LogLikeLoss`` in a captured ``Trainer`` step and the refusals of the C ABI.

Gate per element (loglike_grad_reference.gate_ratio): |d| <= 2^-23 (1 + 2^-20) |ref| + (1e-10 S_r + 1e-12) S_{r,t}, plus 2^-149, the
spacing of fp32 below 2^-126 (outputs there arise where a mixture's weight underflows fp32: the "loud" regime).  Every test prints
its worst error / gate."""
import math

import numpy as np
import pytest
import torch

import loglike_grad_reference as G
import loglike_net_reference as RN
import loglike_reference as R1
import mismatch_reference as MM
from helpers import assert_close
from test_hip_dispatch import _c
from test_hip_predict import _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTS = ("lnl_marg", "lnl_max", "lnl_mix", "lnl_max_mix")
UPS = ("d_marg", "d_max", "d_mix", "d_max_mix")
TILE = 256  # kWfBwdTile
MODELS = {"attnlnp": _c("AttnLNP", 64, 20, n_z=3, B=3, T=37), "cnp": _c("CNP", 64, 20, B=3, T=37)}


def _jc():
    from npf_gwwaveform_amd import functional as FN

    return FN.MATCH_JC, FN.LOGLIKE_I0_SWITCH


@pytest.fixture(scope="module")
def single_cases():
    """(tag, factors, args, closed form) of every single-stream case, computed once and left unchanged."""
    return [(tag, fac, args, G.closed_form(args)) for tag, fac, args in G.cases(*_jc())]


@pytest.fixture(scope="module")
def net_cases():
    return [(tag, fac, args, G.closed_form(args)) for tag, fac, args in G.net_cases(*_jc())]


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _call(dargs, h=None, **extra):
    from npf_gwwaveform_amd import functional as FN

    fn = FN.waveform_lnl_network if "response" in dargs else FN.waveform_lnl
    return fn(**dict(dargs, **({} if h is None else dict(h=h))), **extra)


def _grad(dargs, ups, **extra):
    """(the forward result, h.grad) through the public path for the upstream gradients ``ups`` (None: that output stays unused)."""
    h = dargs["h"].clone().requires_grad_()
    m = _call(dargs, h, **extra)
    pairs = [(getattr(m, o), ups[u].to(DEV)) for o, u in zip(OUTS, UPS) if ups.get(u) is not None]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
    return m, h.grad


def _check(got, parts, ups, what, n_bcast=1):
    want, S = G.grad_of(parts, ups, n_bcast)
    got = got.detach().cpu()
    r = G.gate_ratio(got[..., :2], want, S, parts.ref)
    assert r <= 1.0, (what, r)
    assert torch.isfinite(got).all() and (got[..., 2:] == 0).all(), what
    assert (got[..., :2][S == 0] == 0).all(), what  # not live, beyond the counts, degenerate rows, a zero upstream: exact zeros
    return r


def _sweep(cases, regime, forward):
    worst, n = 0.0, 0
    for i, (tag, fac, args, parts) in enumerate(cases):
        if fac["regime"] != regime:
            continue
        n += 1
        dargs = _dev(args)
        Rn, T = args["h"].shape[:2]
        plain = forward(**dargs)
        for kind in G.UPSTREAMS:
            ups = G.upstream(kind, Rn, parts.Bn, i)
            m, got = _grad(dargs, ups)
            for name in OUTS + ("tau_index",):
                assert torch.equal(getattr(m, name), getattr(plain, name)), (tag, name)
            r = _check(got, parts, ups, f"{tag} upstream {kind}")
            worst = max(worst, r)
            if kind == "all":
                m2, again = _grad(dargs, ups)
                assert torch.equal(got, again) and all(torch.equal(a, b) for a, b in zip(m, m2)), f"{tag}: a second call differs"
                got = got.cpu()
                deg = parts.ref["degenerate"]
                assert (got[deg] == 0).all(), tag
                if fac["counts"] is not None:
                    beyond = (torch.arange(T).view(1, T) >= torch.tensor(fac["counts"]).view(-1, 1)).repeat(fac["n_z"], 1)
                    assert (got[beyond] == 0).all(), tag
                if regime == "degenerate" and fac["wform"] == "T":
                    assert deg.all() and (got == 0).all(), tag
                if regime == "removed":
                    assert torch.isnan(args["h"]).any() and torch.isnan(args["data"]).any(), tag  # (NaN where nothing may be read)
    print(f"LNLGRAD worst error / gate over the {n} cases of regime {regime}: {worst:.3g}")
    return n


# ---- the kernels against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R1.REGIMES)
def test_gradient_meets_the_float64_closed_form(regime, single_cases):
    """Every case of the regime at T in {37, 200}, n_tau in {none, 1, 16, 17, 257}, n_z in {1, 3}, upstream marg / max / mix only
    and all four with random signs: the gate, the forward's bits, exact zeros, the same bits on a second call."""
    from npf_gwwaveform_amd import functional as FN

    assert _sweep(single_cases, regime, FN.waveform_loglike) >= 10


@pytest.mark.parametrize("regime", RN.REGIMES)
def test_network_gradient_meets_the_float64_closed_form(regime, net_cases):
    """D in {1, 2, 3, 8}, with and without delays, one zero response per regime."""
    from npf_gwwaveform_amd import functional as FN

    assert _sweep(net_cases, regime, FN.waveform_loglike_network) >= 5
    mine = [fac for _, fac, _, _ in net_cases if fac["regime"] == regime]
    assert {f["D"] for f in mine} == set(RN.DETS) and any(f["zero_det"] is not None for f in mine)
    assert any(a["delays"] is None for _, f, a, _ in net_cases) and any(a["delays"] is not None for _, f, a, _ in net_cases)


# ---- the edges of the new kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,counts", [(255, None), (256, None), (257, (255, 256, 257))])
def test_points_at_the_workgroup_size(T, counts):
    args = R1.call_args(R1.build("noise", T, n_z=3, h_ld=4, wform="BT", fform="T", taus=R1.grid(17), counts=counts, seed=21))
    parts = G.closed_form(args)
    ups = G.upstream("all", 9, 3, T)
    _, got = _grad(_dev(args), ups)
    print(f"LNLGRAD T={T} counts={counts}: error / gate {_check(got, parts, ups, f'T={T}'):.3g}")


def test_grid_stride_loop_over_a_long_row():
    """256 * 1024 + 37 points: more than the largest grid covers in one pass."""
    T = 256 * 1024 + 37
    args = R1.call_args(R1.build("noise", T, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(1), seed=22))
    parts = G.closed_form(args)
    ups = G.upstream("all", 3, 3, 1)
    _, got = _grad(_dev(args), ups)
    assert float(got.abs().min()) > 0  # (every point of every pass is written)
    print(f"LNLGRAD T={T}: error / gate {_check(got, parts, ups, 'long row'):.3g}")


@pytest.mark.parametrize("n_tau", (TILE - 1, TILE, TILE + 1))
def test_grid_at_the_lds_tile_size(n_tau):
    args = R1.call_args(R1.build("noise", 37, n_z=3, h_ld=4, wform="T", fform="BT", taus=R1.grid(n_tau), counts=(37, 17, 0), seed=23))
    parts = G.closed_form(args)
    assert G.clear_maximum(parts.ref)
    ups = G.upstream("all", 9, 3, n_tau)
    _, got = _grad(_dev(args), ups)
    print(f"LNLGRAD n_tau={n_tau}: error / gate {_check(got, parts, ups, f'n_tau={n_tau}'):.3g}")


def test_maximiser_in_the_last_partial_chunk_of_a_long_grid():
    n_tau = 4099  # 16 tiles and three shifts
    case = R1.build("planted", 37, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(n_tau), j_star=n_tau - 1, seed=24)
    args = R1.call_args(case)
    parts = G.closed_form(args)
    assert (parts.ref["tau_index"] == n_tau - 1).all() and G.clear_maximum(parts.ref)
    for kind in ("max", "all"):
        ups = G.upstream(kind, 3, 3, 5)
        m, got = _grad(_dev(args), ups)
        assert (m.tau_index.cpu() == n_tau - 1).all()
        print(f"LNLGRAD n_tau={n_tau} upstream {kind}: error / gate {_check(got, parts, ups, kind):.3g}")


def _raw_bwd(dargs, m, saved, ups, n_bcast, dh_ld, offset=0):
    """``npf_waveform_loglike_bwd`` through the C ABI into a d_h poisoned with NaN (``offset`` floats into its allocation)."""
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    h = dargs["h"]
    Rn, T, ld = h.shape
    geo = FN.check_loglike_args(h.shape, dargs["data"], dargs["weights"], dargs["freqs"], dargs["taus"])
    nv = FN.counts_i32(dargs["n_valid"], R1.B) if dargs["n_valid"] is not None else None
    buf = torch.full((n_bcast * Rn * T * dh_ld + offset,), math.nan, device=DEV)
    d_h = buf[offset:].view(n_bcast * Rn, T, dh_ld)
    g = [ups[u].to(DEV) if ups.get(u) is not None else None for u in UPS]
    dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = L.load().npf_waveform_loglike_bwd(L.ptr(h), ld, L.ptr(dargs["data"]), L.ptr(dargs["weights"]), geo[4], L.ptr(dargs["freqs"]),
                                           geo[5], dptr(nv), Rn, R1.B, T, geo[6], geo[7], geo[8], m.tau_index.data_ptr(),
                                           saved.data_ptr(), m.lnl_marg.data_ptr(), m.lnl_max.data_ptr(), m.lnl_mix.data_ptr(),
                                           m.lnl_max_mix.data_ptr(), *(dptr(t) for t in g), n_bcast, d_h.data_ptr(), dh_ld,
                                           L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return d_h


def test_every_element_is_written_for_any_leading_dimension_and_n_bcast():
    """The raw call on a d_h poisoned with NaN: dh_ld = 2, 3 (the generic stores), 4 and 5, an unaligned d_h, n_bcast = 1 and 3, on a
    removed-points case with counts.  Every element is written; the row blocks are bit-identical; entries 0 and 1 equal those of
    the public path bit for bit, whatever dh_ld; with n_bcast = 3 they meet the gate of a third of the upstream gradient."""
    from npf_gwwaveform_amd import functional as FN

    jc, x_s = _jc()
    args = R1.call_args(R1.build("removed", 37, n_z=3, h_ld=4, wform="BT", fform="T", taus=R1.grid(jc + 1), counts=(37, 17, 0), seed=12,
                                 x_s=x_s))
    parts = G.closed_form(args)
    dargs = _dev(args)
    ups = G.upstream("all", 9, 3, 2)
    _, public = _grad(dargs, ups)
    geo = FN.check_loglike_args(dargs["h"].shape, dargs["data"], dargs["weights"], dargs["freqs"], dargs["taus"])
    nv = FN.counts_i32(dargs["n_valid"], R1.B)
    outs, saved = FN._lnl_forward(False, dargs["h"], dargs["data"], dargs["weights"], dargs["freqs"], nv, None, None, geo)
    m = FN.WaveformLnl(*outs)
    assert saved.shape == (9, 4 + 2 * (jc + 1)) and (saved.cpu()[2::3] == 0).all() and (saved.cpu()[0::3, 0] != 0).all()
    for dh_ld, offset in ((2, 0), (2, 1), (3, 0), (4, 0), (4, 2), (5, 0)):
        one = _raw_bwd(dargs, m, saved, ups, 1, dh_ld, offset)
        assert torch.isfinite(one).all(), dh_ld
        assert torch.equal(one[..., :2], public[..., :2]) and (one[..., 2:] == 0).all(), (dh_ld, offset)
        three = _raw_bwd(dargs, m, saved, ups, 3, dh_ld, offset).view(3, 9, 37, dh_ld)
        assert torch.isfinite(three).all() and torch.equal(three[0], three[1]) and torch.equal(three[0], three[2]), (dh_ld, offset)
        _check(three[0], parts, ups, f"n_bcast=3 dh_ld={dh_ld}", n_bcast=3)
    # and n_bcast through the public call: samples that hold anything, evaluated on their mean
    samples = torch.randn(3 * 9, 37, 4, device=DEV, requires_grad=True)
    mm = _call(dargs, samples, n_bcast=3, mean=dargs["h"])
    torch.autograd.backward([getattr(mm, o) for o in OUTS], [ups[u].to(DEV) for u in UPS])
    g3 = samples.grad.view(3, 9, 37, 4)
    assert torch.equal(g3[0], g3[1]) and torch.equal(g3[0], g3[2]) and torch.equal(mm.lnl_marg, m.lnl_marg)
    _check(g3[0], parts, ups, "n_bcast=3 public", n_bcast=3)


# ---- known values -------------------------------------------------------------------------------------------------------------------
def test_zero_data_give_minus_the_template_term_alone():
    """d = 0: kappa = 0, so u = 0 and rho = 0, and d_h = -(g_marg + g_max) (w A, 0) to one rounding, without a NaN."""
    case = R1.build("noise", 37, n_z=1, h_ld=2, wform="BT", fform="T", taus=R1.grid(17), seed=31)
    case["data"].zero_()
    dargs = _dev(R1.call_args(case))
    ups = G.upstream("all", 3, 3, 7)
    ups["d_mix"] = ups["d_max_mix"] = None
    _, got = _grad(dargs, ups)
    gs = (ups["d_marg"] + ups["d_max"]).view(3, 1)
    want = -gs * (case["weights"].double() * case["h"][..., 0].double())
    got = got.cpu().double()
    assert torch.isfinite(got).all() and (got[..., 1] == 0).all()
    assert ((got[..., 0] - want).abs() <= G.ONE_ROUNDING * want.abs()).all()


def test_all_ties_grid_with_zero_frequencies():
    """f = 0: every grid time gives the same kappa, p_j = 1 / n, and the max and marg gradients are those of the no-grid call with
    rho(x) in place of 1: tau_index is 0 and the lnl_max gradient equals the one without a grid bit for bit."""
    case = R1.build("noise", 37, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(17), seed=32)
    case["freqs"].zero_()
    dargs = _dev(R1.call_args(case))
    ups = dict(G.upstream("max", 3, 3, 8))
    m, tied = _grad(dargs, ups)
    _, plain = _grad(dict(dargs, freqs=None, taus=None), ups)
    assert (m.tau_index == 0).all() and torch.equal(tied, plain)
    parts = G.closed_form(R1.call_args(case))
    for kind in ("marg", "max"):
        u = G.upstream(kind, 3, 3, 8)
        _check(_grad(dargs, u)[1], parts, u, f"ties {kind}")


def test_dead_rows_and_points_get_exact_zeros_with_nan_in_everything_unread():
    """A degenerate task (all weights zero), removed points and padded points, with NaN planted in h, data and freqs there and in the
    upstream gradients of the degenerate rows."""
    jc, x_s = _jc()
    case = R1.build("removed", 37, n_z=3, h_ld=4, wform="BT", fform="BT", taus=R1.grid(jc + 1), counts=(37, 17, 37), seed=33, x_s=x_s)
    case["weights"][2] = 0.0  # task 2: no live point, hh == 0
    case["h"].view(3, 3, 37, 4)[:, 2] = math.nan
    case["data"][2] = math.nan
    case["freqs"][2] = math.nan
    args = R1.call_args(case)
    parts = G.closed_form(args)
    assert parts.ref["degenerate"].tolist() == [False, False, True] * 3
    ups = G.upstream("all", 9, 3, 9)
    poisoned = {k: v.clone() for k, v in ups.items()}
    poisoned["d_marg"][2::3] = math.nan
    poisoned["d_max"][2::3] = math.nan
    poisoned["d_mix"][2] = math.nan
    poisoned["d_max_mix"][2] = math.nan
    _, got = _grad(_dev(args), poisoned)
    _check(got, parts, ups, "dead rows and points")
    got = got.cpu()
    dead = case["kill"].repeat(3, 1) | (torch.arange(37).view(1, 37) >= torch.tensor([37, 17, 37]).view(3, 1)).repeat(3, 1)
    assert (got[dead] == 0).all() and (got[2::3] == 0).all() and float(got[0].abs().max()) > 0


def test_power_of_two_weights_scale_the_gradient_exactly():
    """w -> 4 w with A -> A / 2 and d -> d / 2: kappa, hh and every likelihood keep their bits, dphi keeps its bits and dA doubles
    exactly -- nothing in the launch depends on the scale but through exact powers of two."""
    case = R1.build("noise", 37, n_z=3, h_ld=2, wform="T", fform="T", taus=R1.grid(17), seed=34)
    dargs = _dev(R1.call_args(case))
    scaled = dict(dargs, weights=dargs["weights"] * 4.0, data=dargs["data"] * 0.5)
    h2 = dargs["h"].clone()
    h2[..., 0] *= 0.5
    scaled["h"] = h2
    ups = G.upstream("all", 9, 3, 10)
    m1, g1 = _grad(dargs, ups)
    m2, g2 = _grad(scaled, ups)
    assert all(torch.equal(a, b) for a, b in zip(m1, m2))
    assert torch.equal(g2[..., 0], 2.0 * g1[..., 0]) and torch.equal(g2[..., 1], g1[..., 1])


def test_mixture_of_rows_800_apart_sends_its_gradient_to_the_upper_row():
    """Latent samples whose lnl_marg lie more than 800 apart: exp(lnl_marg - lnl_mix) / n_z is 1 on the upper row (to an ulp) and
    exactly 0 on the others, so the mixture's gradient is d_mix times the upper row's own gradient and exact zeros elsewhere.  The
    weight is exp(lnl_marg - lnl_mix) / n_z with both likelihoods near 5e3, where an ulp of a double is 9e-13: the two gradients
    are two fp32 roundings of values up to 4e-12 S_{r,t} apart."""
    from npf_gwwaveform_amd import functional as FN

    jc, x_s = _jc()
    case = R1.build("loud", 200, n_z=3, h_ld=2, wform="T", fform="T", taus=R1.grid(jc + 1), j_star=2, seed=1, x_s=x_s)
    case["h"][3:6, :, 0] *= 0.8  # (amplitude factors 1, 0.48, 0.3 of x* = 1e4: lnl_marg about 5000, 3650, 2550)
    dargs = _dev(R1.call_args(case))
    rows = FN.waveform_loglike(**dargs).lnl_marg.view(3, 3)
    top = rows.sort(0, descending=True)
    assert float((top.values[0] - top.values[1]).min()) > 800
    d_mix = torch.tensor([0.5, -2.0, 1.0], dtype=torch.float64)
    _, got = _grad(dargs, dict(d_mix=d_mix))
    d_row = torch.zeros(3, 3, dtype=torch.float64)
    d_row[top.indices[0].cpu(), torch.arange(3)] = d_mix
    _, own = _grad(dargs, dict(d_marg=d_row.view(-1)))
    assert float(rows.abs().max()) < 8192  # (an ulp of 9e-13 at most)
    _, S = G.grad_of(G.closed_form(R1.call_args(case)), dict(d_marg=d_row.view(-1)))
    got, own = got.view(3, 3, 200, 2).double().cpu(), own.view(3, 3, 200, 2).double().cpu()
    bound = 2 * G.ONE_ROUNDING * own.abs() + 4e-12 * S.view(3, 3, 200, 1)
    assert float(own.abs().max()) > 0 and ((got - own).abs() <= bound).all()
    for b in range(3):
        for s in set(range(3)) - {int(top.indices[0][b])}:
            assert (got[s, b] == 0).all(), (s, b)


# ---- identities ---------------------------------------------------------------------------------------------------------------------
def test_single_detector_network_equals_the_single_stream(single_cases):
    """D = 1, C = 1, no delay: the network gradient meets the single stream's reference; whether it is bit for bit is printed."""
    tag, fac, args, parts = next(c for c in single_cases if c[1]["regime"] == "noise" and c[1]["n_tau"] == 257 and c[1]["T"] == 200)
    dargs = _dev(args)
    Bn = R1.B
    net = dict(dargs, data=dargs["data"].unsqueeze(1), weights=None if dargs["weights"] is None else dargs["weights"].unsqueeze(-2),
               response=torch.tensor([1.0, 0.0], dtype=torch.float64, device=DEV).expand(Bn, 1, 2).contiguous(), delays=None)
    ups = G.upstream("all", args["h"].shape[0], Bn, 11)
    m1, g1 = _grad(dargs, ups)
    m2, g2 = _grad(net, ups)
    print(f"LNLGRAD D=1 network against the single stream ({tag}): values bit for bit {all(torch.equal(a, b) for a, b in zip(m1, m2))}, "
          f"gradient bit for bit {torch.equal(g1, g2)}; error / gate {_check(g2, parts, ups, 'D=1 network'):.3g}")


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _observation(Bn, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Bn, T, 2, generator=g).to(DEV), (0.5 + torch.rand(Bn, T, generator=g)).to(DEV),
            torch.linspace(20.0, 512.0, T).to(DEV), R1.grid(_jc()[0] + 1))


def _forward(model, Xc, Yc, Xt, n_trgt=None, seed=9):
    torch.manual_seed(seed)
    return model(Xc, Yc, Xt, **(dict(n_trgt=n_trgt) if n_trgt is not None else {}))


@pytest.mark.parametrize("of", ("samples", "mean"))
@pytest.mark.parametrize("name", list(MODELS))
def test_models_lnl_has_the_bits_of_loglike_and_its_backward_is_the_closed_form(name, of):
    import npf_gwwaveform_amd as A

    case = MODELS[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    data, w, f, taus = _observation(Bn, T, 41)
    p = _forward(model, Xc, Yc, Xt)[0]
    suff = p._suff
    assert suff.requires_grad and tuple(suff.shape) == (n_z * Bn, T, 4)
    suff.retain_grad()
    m = p.lnl(data, weights=w, freqs=f, taus=taus, of=of)
    ll = p.loglike(data, weights=w, freqs=f, taus=taus, of=of)
    assert isinstance(m, A.Lnl) and p._base is None and m.lnl_marg.shape == ((n_z, Bn) if of == "samples" else (1, Bn))
    for mine, theirs in (("lnl", "lnl"), ("lnl_marg", "lnl_marg"), ("lnl_max", "lnl_max"), ("lnl_max_mix", "lnl_max_mix")):
        assert torch.equal(getattr(m, mine), getattr(ll, theirs)), (name, of, mine)
    assert not ll.lnl.requires_grad and m.lnl.requires_grad
    (m.lnl.sum() + 0.5 * m.lnl_max.sum()).backward()
    got = suff.grad.cpu()
    with torch.no_grad():
        h = suff.detach() if of == "samples" else p.summary().mean
    args = dict(h=h.cpu(), data=data.cpu(), weights=w.cpu(), freqs=f.cpu(), taus=taus, n_valid=None)
    parts = G.closed_form(args)
    assert G.clear_maximum(parts.ref), name
    rows = h.shape[0]
    ups = dict(d_mix=torch.ones(Bn, dtype=torch.float64), d_max=torch.full((rows,), 0.5, dtype=torch.float64))
    blocks = got.view(-1, rows, T, 4)
    for q in range(blocks.shape[0]):
        r = _check(blocks[q], parts, ups, f"{name} of={of}", n_bcast=n_z if of == "mean" else 1)
        print(f"LNLGRAD {name} of={of} block {q}: error / gate {r:.3g}")
        assert of == "samples" or torch.equal(blocks[q], blocks[0])


def test_parameter_gradients_of_the_sum_are_the_sum_of_the_parameter_gradients():
    import npf_gwwaveform_amd as A

    case = MODELS["attnlnp"]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Y = torch.stack([0.5 + torch.rand(case["B"], case["T"]), 3.0 * torch.randn(case["B"], case["T"])], -1).to(DEV)
    _, w, f, taus = _observation(case["B"], case["T"], 41)
    base, lam = A.NLLLossLNPF(), 0.1
    losses = dict(both=A.LogLikeLoss(base=base, lam=lam, weights=w, freqs=f, taus=taus), base=base,
                  lnl=A.LogLikeLoss(lam=lam, weights=w, freqs=f, taus=taus))
    values, grads = {}, {}
    for key, crit in losses.items():
        crit.to(DEV).train()
        model.zero_grad(set_to_none=True)
        loss = crit(_forward(model, Xc, Yc, Xt), Y)
        loss.backward()
        values[key] = float(loss.detach())
        grads[key] = {k: (q.grad.detach().clone() if q.grad is not None else torch.zeros_like(q)) for k, q in model.named_parameters()}
    np.testing.assert_allclose(values["both"], values["base"] + values["lnl"], rtol=1e-6)
    assert any(float(g.abs().max()) > 0 for g in grads["lnl"].values())
    for k in grads["both"]:
        assert_close(grads["both"][k], grads["base"][k] + grads["lnl"][k], tol=1e-5, what=f"attnlnp {k}")


def test_padded_targets_equal_the_cut_batch():
    case = MODELS["attnlnp"]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z = case["B"], case["T"], case["n_z"]
    counts = (37, 17, 5)
    n_trgt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    data, w, f, taus = _observation(Bn, T, 43)
    data[1, 17:] = math.nan
    p = _forward(model, Xc, Yc, Xt, n_trgt)[0]
    p._suff.retain_grad()
    m = p.lnl(data, weights=w, freqs=f, taus=taus)
    m.lnl.sum().backward()
    got = p._suff.grad.cpu().view(n_z, Bn, T, 4)
    assert torch.isfinite(got).all()
    h = p._suff.detach().cpu().view(n_z, Bn, T, 4)
    for b, n in enumerate(counts):
        args = dict(h=h[:, b, :n], data=data[b:b + 1, :n].cpu(), weights=w[b:b + 1, :n].cpu(), freqs=f[:n].cpu(), taus=taus, n_valid=None)
        parts = G.closed_form(args)
        _check(got[:, b, :n], parts, dict(d_mix=torch.ones(1, dtype=torch.float64)), f"padded task {b} cut to {n}")
        assert (got[:, b, n:] == 0).all()


def test_y_dim_1_raises():
    import npf_gwwaveform_amd as A

    p = A.HeadDistribution(torch.zeros(3, 37, 2, device=DEV), 1, False, 1, 3, 37)
    with pytest.raises(ValueError, match="y_dim"):
        p.lnl(torch.zeros(3, 37, 2, device=DEV))


# ---- the Trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_captures_the_loglike_loss_and_minus_lnl_falls():
    """``Trainer`` with ``LogLikeLoss(base=CNPFLoss(), ...)`` on the sizes of the mismatch Trainer test: the step is captured once, the
    replays read ``noise`` after it was overwritten in place, the first step's loss equals an eager step's bit for bit, and -lnl
    falls over the steps."""
    import npf_gwwaveform_amd as A
    import specs
    from helpers import build_model
    from npf_gwwaveform_amd.train import Trainer

    batch, freqs, taus = MM.train_setup()
    batch, freqs = {k: v.to(DEV) for k, v in batch.items()}, freqs.to(DEV)
    Bn, T = MM.TRAIN_CASE["B"], MM.TRAIN_CASE["T"]
    noises = [0.01 * torch.randn(Bn, T, 2, generator=torch.Generator().manual_seed(70 + i)).to(DEV) for i in range(MM.TRAIN_STEPS)]

    def minus_lnl(model):
        with torch.no_grad():
            p = model(batch["X_cntxt"], batch["Y_cntxt"], batch["X_trgt"])[0]
            crit = A.LogLikeLoss(freqs=freqs, taus=taus).to(DEV)
            return float(-p.loglike(crit.injection(batch["Y_trgt"]), freqs=freqs, taus=taus).lnl.mean())

    def run(use_graph):
        model = build_model(MM.TRAIN_CASE, DEV, params=specs.make_params(MM.TRAIN_CASE, seed=MM.TRAIN_SEED))
        crit = A.LogLikeLoss(base=A.CNPFLoss(), lam=1.0, freqs=freqs.clone(), taus=taus, noise=torch.zeros(Bn, T, 2)).to(DEV)
        tr = Trainer(model, crit, lr=MM.TRAIN_LR, world=1, use_graph=use_graph)
        before, losses = minus_lnl(model), []
        for n in noises:
            crit.noise.copy_(n)
            losses.append(float(tr.step(batch)))
        return losses, tr, before, minus_lnl(model)

    l_e, _, b_e, a_e = run(False)
    l_g, tr, b_g, a_g = run(True)
    print(f"LNLGRAD trainer: mean -lnl {b_g:.4f} -> {a_g:.4f} after {MM.TRAIN_STEPS} steps; loss {l_g[0]:.4f} -> {l_g[-1]:.4f}")
    assert tr._graph is not None and tr.n_captures == 1
    assert b_g == b_e and l_g[0] == l_e[0] and all(np.isfinite(l_g))
    np.testing.assert_allclose(l_g, l_e, rtol=1e-6)  # (the noise of every step was read by the replay)
    assert a_g < b_g and a_e < b_e


# ---- the C ABI on device pointers ---------------------------------------------------------------------------------------------------
def test_ex_outputs_are_bit_equal_and_the_c_abi_refuses_what_the_contract_lists():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    f32 = torch.rand(6 * 4 * 2, device=DEV) + 0.5
    ws = torch.zeros(lib.npf_waveform_loglike_workspace_bytes(6, 3) // 8, dtype=torch.float64, device=DEV)
    n_sv = lib.npf_waveform_loglike_saved_doubles(3)
    outs = {k: torch.full((6,), math.nan, dtype=torch.float64, device=DEV) for k in ("hh", "dd", "snr", "lnl_max", "lnl_marg", "phase",
                                                                                     "lnl_mix", "lnl_max_mix")}
    outs["tau_index"] = torch.full((6,), -1, dtype=torch.int32, device=DEV)
    outs["series"] = torch.full((6, 3, 2), math.nan, dtype=torch.float64, device=DEV)
    twin = {k: v.clone() for k, v in outs.items()}
    saved = torch.full((6, n_sv), math.nan, dtype=torch.float64, device=DEV)
    p = f32.data_ptr()
    head = (p, 2, p, p, 1, p, 1, None, 6, 2, 4, 0.0, 1e-3, 3)
    order = ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "series", "lnl_mix", "lnl_max_mix")
    assert lib.npf_waveform_loglike(*head, *(outs[k].data_ptr() for k in order), ws.data_ptr(), L.stream_ptr()) == 0
    assert lib.npf_waveform_loglike_ex(*head, *(twin[k].data_ptr() for k in order), None, ws.data_ptr(), L.stream_ptr()) == -1  # no saved
    assert lib.npf_waveform_loglike_ex(*head, *(twin[k].data_ptr() for k in order), saved.data_ptr(), ws.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in order:
        assert torch.equal(outs[k][:2] if k in ("dd", "lnl_mix", "lnl_max_mix") else outs[k],
                           twin[k][:2] if k in ("dd", "lnl_mix", "lnl_max_mix") else twin[k]), k
    assert torch.isfinite(saved).all() and (saved[:, 3] == 0).all() and torch.equal(saved[:, 0], outs["hh"])
    q = torch.complex(saved[:, 4::2], saved[:, 5::2]).sum(1).abs()
    assert float(q.max()) <= 1.0 and float(q.min()) > 0

    d_h = torch.full((6, 4, 2), math.nan, device=DEV)
    g = torch.ones(6, dtype=torch.float64, device=DEV)
    ok = dict(h=p, h_ld=2, d=p, wgt=p, wgt_rows=1, freq=p, freq_rows=1, n_valid=None, n_rows=6, n_tasks=2, pts=4, tau0=0.0, dtau=1e-3,
              n_tau=3, tau_index=twin["tau_index"].data_ptr(), saved=saved.data_ptr(), lnl_marg=twin["lnl_marg"].data_ptr(),
              lnl_max=twin["lnl_max"].data_ptr(), lnl_mix=twin["lnl_mix"].data_ptr(), lnl_max_mix=twin["lnl_max_mix"].data_ptr(),
              d_marg=g.data_ptr(), d_max=None, d_mix=g.data_ptr(), d_max_mix=None, n_bcast=1, d_h=d_h.data_ptr(), dh_ld=2)
    for change in (dict(n_rows=5), dict(n_tau=65537), dict(freq=None), dict(tau_index=None), dict(saved=None), dict(d_h=None),
                   dict(d_marg=None, d_mix=None), dict(lnl_mix=None), dict(lnl_marg=None), dict(d_max_mix=g.data_ptr(), lnl_max=None),
                   dict(n_bcast=0), dict(dh_ld=1), dict(wgt_rows=3)):
        assert lib.npf_waveform_loglike_bwd(*dict(ok, **change).values(), L.stream_ptr()) == -1, change
    net = dict(ok)
    resp = torch.ones(2, 1, 2, dtype=torch.float64, device=DEV)
    items = list(ok.items())
    net = dict(items[:8] + [("delay", None), ("resp", resp.data_ptr())] + items[8:10] + [("n_det", 1)] + items[10:])
    for change in (dict(n_det=0), dict(n_det=9), dict(resp=None), dict(delay=resp.data_ptr(), freq=None, n_tau=0), dict(d_marg=None, d_mix=None)):
        assert lib.npf_waveform_loglike_net_bwd(*dict(net, **change).values(), L.stream_ptr()) == -1, change
    torch.cuda.synchronize()
    assert torch.isnan(d_h).all()  # nothing was launched
    assert lib.npf_waveform_loglike_bwd(*ok.values(), L.stream_ptr()) == 0
    one = d_h.clone()
    assert lib.npf_waveform_loglike_net_bwd(*net.values(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(one).all() and torch.isfinite(d_h).all()
