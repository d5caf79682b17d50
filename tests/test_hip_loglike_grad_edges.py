"""The likelihood gradient's two kernels at their edges: ``waveform_loglike_coef_kernel`` and ``waveform_loglike_bwd_kernel<LD, NET>``
on the inputs of tests/loglike_grad_edge_cases.py (each proved well posed on the CPU by tests/test_loglike_grad_edges_host.py),
against the float64 closed form of tests/loglike_grad_reference.py under its unchanged gate (``gate_ratio``).  A: the row of
coefficients ``saved`` against ``saved_reference`` under the derived gate of ``saved_gates``.  B: one live point per task, where
every grid time ties -- the forward's ``tau_index`` and the coefficient kernel's own maximiser must be the same index.  C: the
network backward -- raw stores, the 256-point block, the 256-shift tile, per-detector liveness, a task without response, powers of
two, a long row.  D: the single stream's grid limits.  E: values.  F: the backward after the shared workspace was rewritten.
Every gradient also meets: exact zeros where S == 0, entries 2 .. ld - 1 zero, finite.  Every test prints ``LNLGRADEDGE ...``."""
import math

import pytest
import torch

import loglike_grad_edge_cases as E
import loglike_grad_reference as G
import loglike_reference as R1
from test_hip_loglike_grad import DEV, OUTS, UPS, _check, _dev, _grad

pytestmark = pytest.mark.gpu


def _rows(family):
    return [(tag, fac, args, G.closed_form(args)) for tag, fac, args in E.cases(family)]


def _prepared(dargs):
    """(net, the tensors ``FN._lnl_forward`` takes, geo) as the public calls prepare them."""
    from npf_gwwaveform_amd import functional as FN

    net = "response" in dargs
    if net:
        geo = FN.check_loglike_network_args(dargs["h"].shape, dargs["data"], dargs["response"], dargs["delays"], dargs["weights"],
                                            dargs["freqs"], dargs["taus"])
    else:
        geo = FN.check_loglike_args(dargs["h"].shape, dargs["data"], dargs["weights"], dargs["freqs"], dargs["taus"])
    delays = dargs.get("delays")
    freqs = dargs["freqs"] if dargs["freqs"] is not None and (geo[-1] > 0 or delays is not None) else None
    nv = FN.counts_i32(dargs["n_valid"], R1.B) if dargs["n_valid"] is not None else None
    return net, (dargs["h"].contiguous(), dargs["data"].contiguous(), dargs["weights"], freqs, nv, dargs.get("response"), delays), geo


def _forward(dargs):
    from npf_gwwaveform_amd import functional as FN

    net, t, geo = _prepared(dargs)
    outs, saved = FN._lnl_forward(net, *t, geo)
    return FN.WaveformLnl(*outs), saved, net, t, geo


def _raw_ex(net, t, geo, n_tau=None):
    """``npf_waveform_loglike_ex`` / ``npf_waveform_loglike_net_ex`` through the C ABI into a ``saved`` prefilled with NaN -> (rc,
    saved).  ``n_tau``: the grid length handed over in place of the case's (buffers stay those of the case)."""
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    lib = L.load()
    h, data, w, f, nv, resp, dl = t
    R, T, ld, B = geo[:4]
    wgt_rows, freq_rows, tau0, dtau, n = geo[-5:]
    ws_bytes = lib.npf_waveform_loglike_net_workspace_bytes(R, geo[4], n) if net else lib.npf_waveform_loglike_workspace_bytes(R, n)
    ws = FN._match_workspace(h.device, int(ws_bytes))
    saved = torch.full((R, int(lib.npf_waveform_loglike_saved_doubles(n))), math.nan, dtype=torch.float64, device=DEV)
    marg, mx = (torch.empty(R, dtype=torch.float64, device=DEV) for _ in range(2))
    mix, mxm = (torch.empty(B, dtype=torch.float64, device=DEV) for _ in range(2))
    idx = torch.empty(R, dtype=torch.int32, device=DEV)
    dptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    head = (L.ptr(h), ld, L.ptr(data), L.ptr(w), wgt_rows, L.ptr(f), freq_rows, dptr(nv))
    outs = (None, None, None, mx.data_ptr(), marg.data_ptr(), idx.data_ptr(), None, None, mix.data_ptr(), mxm.data_ptr())
    n_arg = n if n_tau is None else n_tau
    if net:
        rc = lib.npf_waveform_loglike_net_ex(*head, dptr(dl), dptr(resp), R, B, geo[4], T, tau0, dtau, n_arg, *outs, None, None, None,
                                             saved.data_ptr(), ws.data_ptr(), L.stream_ptr())
    else:
        rc = lib.npf_waveform_loglike_ex(*head, R, B, T, tau0, dtau, n_arg, *outs, saved.data_ptr(), ws.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, saved


def _raw_net_bwd(t, geo, m, saved, ups, n_bcast, dh_ld, offset=0):
    """``npf_waveform_loglike_net_bwd`` through the C ABI into a d_h poisoned with NaN (``offset`` floats into its allocation)."""
    from npf_gwwaveform_amd import _lib as L

    h, data, w, f, nv, resp, dl = t
    R, T, ld, B, D, wgt_rows, freq_rows, tau0, dtau, n = geo
    buf = torch.full((n_bcast * R * T * dh_ld + offset,), math.nan, device=DEV)
    d_h = buf[offset:].view(n_bcast * R, T, dh_ld)
    g = [ups[u].to(DEV) if ups.get(u) is not None else None for u in UPS]
    dptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    rc = L.load().npf_waveform_loglike_net_bwd(L.ptr(h), ld, L.ptr(data), L.ptr(w), wgt_rows, L.ptr(f), freq_rows, dptr(nv), dptr(dl),
                                               dptr(resp), R, B, D, T, tau0, dtau, n, m.tau_index.data_ptr(), saved.data_ptr(),
                                               m.lnl_marg.data_ptr(), m.lnl_max.data_ptr(), m.lnl_mix.data_ptr(),
                                               m.lnl_max_mix.data_ptr(), *(dptr(x) for x in g), n_bcast, d_h.data_ptr(), dh_ld,
                                               L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return d_h


def _standard(family, extra=None):
    """Every case of a family through the public path for each of its upstream kinds: the gate, exact zeros, the planted index."""
    worst, n = 0.0, 0
    for i, (tag, fac, args, parts) in enumerate(_rows(family)):
        dargs = _dev(args)
        Rn = args["h"].shape[0]
        for kind in fac["kinds"]:
            ups = E.ups_of(kind, Rn, parts.Bn, i)
            m, got = _grad(dargs, ups)
            if fac["j_star"] is not None:
                live = ~parts.ref["degenerate"]
                assert (m.tau_index.cpu()[live] == fac["j_star"]).all(), tag
            r = _check(got, parts, ups, f"{tag} upstream {kind}")
            print(f"LNLGRADEDGE {tag} upstream {kind}: error / gate {r:.3g}")
            worst = max(worst, r)
            if extra is not None:
                extra(tag, fac, args, parts, kind, m, got)
        n += 1
    print(f"LNLGRADEDGE family {family}: {n} cases, worst error / gate {worst:.3g}")
    return n


# ---- A: the coefficients against float64 --------------------------------------------------------------------------------------------
def test_a_saved_coefficients_meet_the_float64_reference():
    """Per row of ``saved``: q_j within |dq_j| <= p_j (delta_L + delta_K_j / 2) + 2^-52 |q_j|; entry 3 zero; entry 0 the forward's hh
    / HH bit for bit; the direction of modulus 1 within 4 ulp or exactly (0, 0), and equal to conj(K_ref / |K_ref|) at the GPU's own
    ``tau_index`` within delta_K / x; degenerate rows all zero; sum_j |q_j| <= 1; the raw entry writes every element of a row
    prefilled with NaN, with the same bits."""
    from npf_gwwaveform_amd import functional as FN

    worst, worst_dir, n = {False: 0.0, True: 0.0}, 0.0, 0
    for tag, fac, args, parts in _rows("A"):
        dargs = _dev(args)
        m, saved, net, t, geo = _forward(dargs)
        rc, raw = _raw_ex(net, t, geo)
        assert rc == 0 and torch.equal(raw, saved), tag  # (no NaN left: every element is written)
        plain = (FN.waveform_loglike_network if net else FN.waveform_loglike)(**dargs, want=("hh", "tau_index", "lnl_marg"))
        assert torch.equal(plain.tau_index, m.tau_index) and torch.equal(plain.lnl_marg, m.lnl_marg), tag
        sv = saved.cpu()
        ref = parts.ref
        nn = ref["x"].shape[1]
        assert sv.shape == (args["h"].shape[0], 4 + 2 * nn) and fac["c_off"] == (2 + 2 * fac["D"] if net else (2 if fac["n_tau"] is None else 4))
        assert torch.isfinite(sv).all() and (sv[:, 3] == 0).all() and torch.equal(sv[:, 0], plain.hh.cpu()), tag
        deg = ref["degenerate"]
        assert torch.equal(sv[:, 0] == 0, deg) and (sv[deg] == 0).all(), tag
        r = G.saved_ratio(sv, parts)
        print(f"LNLGRADEDGE {tag}: saved q_j error / gate {r:.3g}")
        assert r <= 1.0, (tag, r)
        worst[net] = max(worst[net], r)
        q = torch.complex(sv[:, 4::2], sv[:, 5::2])
        assert float(q.abs().sum(1).max()) <= 1.0, tag
        # the direction, at the index the forward returned
        idx = m.tau_index.cpu().long().view(-1, 1)
        kb, xb = ref["K"].gather(1, idx)[:, 0], ref["x"].gather(1, idx)[:, 0]
        u = torch.complex(sv[:, 1], sv[:, 2])
        live = ~deg & (xb > 0)
        assert ((u[live].abs() - 1.0).abs() <= 4 * 2.0 ** -52).all() and (u[~live] == 0).all(), tag
        d_K, _ = G.saved_gates(parts)
        bound = d_K.gather(1, idx)[:, 0][live] / xb[live] + 4 * 2.0 ** -52
        d = (u[live] - (kb[live] / xb[live]).conj()).abs()
        assert (d <= bound).all(), (tag, float((d / bound).max()))
        worst_dir = max(worst_dir, float((d / bound).max()) if d.numel() else 0.0)
        n += 1
    print(f"LNLGRADEDGE family A: {n} cases, saved q_j worst error / gate single {worst[False]:.3g} network {worst[True]:.3g}, "
          f"direction worst error / bound {worst_dir:.3g}")
    assert n == 25


# ---- B: the two kernels agree on the index at ties ----------------------------------------------------------------------------------
def test_b_forward_and_coefficient_kernel_choose_the_same_index_at_near_ties():
    """One live point per task: |kappa_j| is the same for every j up to rounding.  Whatever index the forward returns, the stored
    direction must be that index's: a pair that disagrees leaves dphi of order g_max w A |d|, thousands of gates."""
    seen = set()

    def extra(tag, fac, args, parts, kind, m, got):
        seen.update(m.tau_index.cpu()[~parts.ref["degenerate"]].tolist())

    assert _standard("B", extra) == 18
    print(f"LNLGRADEDGE family B: the forward returned {len(seen)} different indices, the largest {max(seen)}")


# ---- C: the network backward --------------------------------------------------------------------------------------------------------
def test_c1_network_raw_stores_for_any_leading_dimension_and_n_bcast():
    """dh_ld = 2, 3 (the generic stores), 4 and 5, an unaligned d_h, n_bcast = 1 and 3, D = 3 with delays on the removed-points
    case with counts (37, 17, 0): every element written, the row blocks bit-identical, entries 0 / 1 those of the public path bit
    for bit, n_bcast = 3 within the gate of a third of the upstream gradient."""
    tag, fac, args, parts = _rows("C1")[0]
    dargs = _dev(args)
    ups = E.ups_of("all", 9, 3, 2)
    _, public = _grad(dargs, ups)
    worst = _check(public, parts, ups, tag)
    m, saved, net, t, geo = _forward(dargs)
    assert net and geo[4] == 3 and t[6] is not None and (saved.cpu()[2::3] == 0).all() and (saved.cpu()[0::3, 0] != 0).all()
    for dh_ld, offset in E.C1_STORES:
        one = _raw_net_bwd(t, geo, m, saved, ups, 1, dh_ld, offset)
        assert torch.isfinite(one).all(), (dh_ld, offset)
        assert torch.equal(one[..., :2], public[..., :2]) and (one[..., 2:] == 0).all(), (dh_ld, offset)
        three = _raw_net_bwd(t, geo, m, saved, ups, 3, dh_ld, offset).view(3, 9, E.T, dh_ld)
        assert torch.isfinite(three).all() and torch.equal(three[0], three[1]) and torch.equal(three[0], three[2]), (dh_ld, offset)
        worst = max(worst, _check(three[0], parts, ups, f"C1 n_bcast=3 dh_ld={dh_ld} offset={offset}", n_bcast=3))
    print(f"LNLGRADEDGE family C1: {len(E.C1_STORES)} stores x n_bcast 1, 3: worst error / gate {worst:.3g}")


def test_c2_network_points_at_the_workgroup_size():
    assert _standard("C2") == 6


def test_c3_network_grid_at_the_lds_tile_and_a_maximiser_in_the_last_partial_tile():
    assert _standard("C3") == 4


def test_c4_network_per_detector_liveness():
    """Point t is live for detector t mod D only, every 7th point for none; removed weights are 0 or inf; NaN in the data of every
    dead (detector, point) and in h and freqs where a point is dead for all: exact zeros there, no NaN anywhere."""
    def extra(tag, fac, args, parts, kind, m, got):
        got = got.cpu()
        dead_all = ~fac["live"].any(0)
        assert (got[:, dead_all] == 0).all() and (got[:, ~dead_all, :2] != 0).all(), tag

    assert _standard("C4", extra) == 4


def test_c5_network_task_without_response_gets_zeros_with_nan_upstream():
    tag, fac, args, parts = _rows("C5")[0]
    b = fac["dead_task"]
    ups = E.ups_of("all", 9, 3, 5)
    poisoned = {k: v.clone() for k, v in ups.items()}
    poisoned["d_marg"][b::3] = math.nan
    poisoned["d_max"][b::3] = math.nan
    poisoned["d_mix"][b] = math.nan
    poisoned["d_max_mix"][b] = math.nan
    m, got = _grad(_dev(args), poisoned)
    r = _check(got, parts, ups, tag)
    assert (got.cpu()[b::3] == 0).all() and float(got.cpu()[0].abs().max()) > 0
    assert (m.lnl_marg.cpu()[b::3] == 0).all() and (m.lnl_max.cpu()[b::3] == 0).all()
    print(f"LNLGRADEDGE {tag}: error / gate {r:.3g}")


def test_c6_network_powers_of_two_in_the_response():
    """C_k 2^k with A 2^-k: K_j, HH and every likelihood keep their bits, dphi too, dA is multiplied by 2^k exactly.  C_k 2^k with
    d 2^-k, the scaling the issue names: K_j keeps its bits but HH is multiplied by 4^k, so the forward's bits are compared first,
    reported, and the check falls back to the gate of the scaled case's own closed form."""
    tag, fac, args, parts = _rows("C6")[0]
    ups = E.ups_of("all", 9, 3, 6)
    m1, g1 = _grad(_dev(args), ups)
    worst = _check(g1, parts, ups, tag)
    for k in fac["ks"]:
        for what in ("template", "data"):
            scaled = E.net_pow2(args, k, what)
            m2, g2 = _grad(_dev(scaled), ups)
            same = all(torch.equal(a, b) for a, b in zip(m1, m2))
            print(f"LNLGRADEDGE C6 C_k 2^{k}, {what} 2^{-k}: likelihood bits unchanged {same}")
            if same:
                assert torch.equal(g2[..., 0], g1[..., 0] * 2.0 ** k) and torch.equal(g2[..., 1], g1[..., 1]), (k, what)
            else:
                assert torch.equal(m2.tau_index, m1.tau_index), (k, what)
                worst = max(worst, _check(g2, G.closed_form(scaled), ups, f"C6 k={k} {what}"))
            assert same or what == "data", k  # (the template scaling is exact by construction)
    print(f"LNLGRADEDGE family C6: worst error / gate {worst:.3g}")


def test_c7_network_grid_stride_loop_over_a_long_row():
    def extra(tag, fac, args, parts, kind, m, got):
        counts = torch.tensor(args["n_valid"].tolist()).view(3, 1)
        inside = torch.arange(E.LONG_T).view(1, -1) < counts
        got = got.cpu()
        assert (got[inside] != 0).all() and (got[~inside] == 0).all()  # every point of every pass is written

    assert _standard("C7", extra) == 1


# ---- D: grid limits of the single stream --------------------------------------------------------------------------------------------
def test_d1_grids_of_4095_4096_4097_shifts():
    assert _standard("D1") == 3


def test_d2_the_longest_grid_and_one_shift_more():
    """n_tau = 65536 at T = 5, the maximiser planted at the last shift, the first shift of the last tile and both sides of the first
    tile seam; 65537 shifts are refused by the forward and the backward, and nothing is written."""
    from npf_gwwaveform_amd import _lib as L

    assert _standard("D2") == 4
    tag, fac, args = E.cases("D2")[0]
    dargs = _dev(args)
    m, saved, net, t, geo = _forward(dargs)
    rc, raw = _raw_ex(net, t, geo, n_tau=E.MAX_TAU + 1)
    assert rc == -1 and torch.isnan(raw).all()
    h, data, w, f, nv, _, _ = t
    d_h = torch.full((3, 5, 2), math.nan, device=DEV)
    g = torch.ones(3, dtype=torch.float64, device=DEV)
    rc = L.load().npf_waveform_loglike_bwd(L.ptr(h), 2, L.ptr(data), L.ptr(w), geo[4], L.ptr(f), geo[5], None, 3, 3, 5, geo[6], geo[7],
                                           E.MAX_TAU + 1, m.tau_index.data_ptr(), saved.data_ptr(), m.lnl_marg.data_ptr(),
                                           m.lnl_max.data_ptr(), m.lnl_mix.data_ptr(), m.lnl_max_mix.data_ptr(), g.data_ptr(), None, None,
                                           None, 1, d_h.data_ptr(), 2, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and torch.isnan(d_h).all()


def test_d3_grids_crossing_zero():
    assert _standard("D3") == 10


def test_d4_large_arguments():
    assert _standard("D4") == 1


# ---- E: values ----------------------------------------------------------------------------------------------------------------------
def test_e1_rho_on_both_sides_of_the_switch():
    assert _standard("E1") == 3


def test_e2_x_star_far_above_the_loud_regime():
    """x* = 1e6 and 1e8: every other p_j is exactly 0, the gate holds, and the marg-only gradient is rho(x*) times the max-only one
    within two gates."""
    for i, (tag, fac, args, parts) in enumerate(_rows("E2")):
        dargs = _dev(args)
        g = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)
        grads = {}
        for kind, key in (("marg", "d_marg"), ("max", "d_max")):
            ups = {key: g}
            m, grads[kind] = _grad(dargs, ups)
            assert (m.tau_index.cpu() == fac["j_star"]).all(), tag
            print(f"LNLGRADEDGE {tag} upstream {kind}: error / gate {_check(grads[kind], parts, ups, tag):.3g}")
        _, saved, *_ = _forward(dargs)
        q = torch.complex(saved[:, 4::2], saved[:, 5::2]).cpu()
        others = torch.ones(17, dtype=torch.bool)
        others[fac["j_star"]] = False
        assert (q[:, others] == 0).all() and (q[:, ~others].abs() > 0.999).all(), tag
        rho = G.rho(parts.ref["x"].max(1).values).view(3, 1, 1)
        _, S = G.grad_of(parts, dict(d_marg=g))
        r = G.gate_ratio(grads["marg"][..., :2], rho * grads["max"][..., :2].cpu().double(), S, parts.ref)
        print(f"LNLGRADEDGE {tag}: marg gradient against rho(x*) times the max gradient, difference / gate {r:.3g}")
        assert r <= 2.0, (tag, r)


def test_e3_cancelling_zero_and_scaled_upstream_gradients():
    """d_max = -d_marg exactly (g_sum == 0: the template term vanishes); d_marg with zeros in rows 0 and 4 and nothing else (exact
    zeros there); every upstream gradient times 2^+-60 (the gradient scales exactly)."""
    tag, fac, args, parts = _rows("E3")[0]
    dargs = _dev(args)
    base = E.ups_of("all", 9, 3, 3)
    ups = dict(d_marg=base["d_marg"], d_max=-base["d_marg"])
    _, got = _grad(dargs, ups)
    print(f"LNLGRADEDGE {tag} d_max = -d_marg: error / gate {_check(got, parts, ups, 'E3 g_sum == 0'):.3g}")
    assert float(got.abs().max()) > 0
    d = base["d_marg"].clone()
    d[[0, 4]] = 0.0
    _, got = _grad(dargs, dict(d_marg=d))
    print(f"LNLGRADEDGE {tag} zeros in d_marg: error / gate {_check(got, parts, dict(d_marg=d), 'E3 zero rows'):.3g}")
    assert (got[[0, 4]] == 0).all() and float(got[1].abs().max()) > 0
    _, g1 = _grad(dargs, base)
    _check(g1, parts, base, "E3 all")
    assert float(g1.abs().max()) * 2.0 ** 60 < 1e30 and float(g1[g1 != 0].abs().min()) * 2.0 ** -60 > 2.0 ** -126  # (fp32 holds both)
    for k in (60, -60):
        _, g2 = _grad(dargs, {key: v * 2.0 ** k for key, v in base.items()})
        assert torch.equal(g2, g1 * 2.0 ** k), k


def test_e4_degenerate_sample_inside_a_live_mixture():
    def extra(tag, fac, args, parts, kind, m, got):
        got = got.cpu()
        assert (got[fac["dead_row"]] == 0).all() and float(got[0].abs().max()) > 0 and float(got[6].abs().max()) > 0, tag
        assert float(m.lnl_marg.detach()[fac["dead_row"]]) == 0.0 and float(m.lnl_max.detach()[fac["dead_row"]]) == 0.0, tag

    assert _standard("E4", extra) == 2


def test_e5_one_latent_sample_mixture_is_the_row():
    tag, fac, args, parts = _rows("E5")[0]
    dargs = _dev(args)
    g = torch.tensor([0.75, -1.5, 3.0], dtype=torch.float64)
    m, g_mix = _grad(dargs, dict(d_mix=g))
    assert torch.equal(m.lnl_mix, m.lnl_marg) and torch.equal(m.lnl_max_mix, m.lnl_max)
    _, g_marg = _grad(dargs, dict(d_marg=g))
    assert torch.equal(g_mix, g_marg)
    _, g_mxm = _grad(dargs, dict(d_max_mix=g))
    _, g_max = _grad(dargs, dict(d_max=g))
    assert torch.equal(g_mxm, g_max)
    print(f"LNLGRADEDGE {tag}: error / gate {_check(g_mix, parts, dict(d_mix=g), tag):.3g}")


def test_e6_powers_of_two_beyond_a_factor_two():
    tag, fac, args, parts = _rows("E6")[0]
    ups = E.ups_of("all", 9, 3, 10)
    m1, g1 = _grad(_dev(args), ups)
    print(f"LNLGRADEDGE {tag}: error / gate {_check(g1, parts, ups, tag):.3g}")
    for k in fac["ks"]:
        m2, g2 = _grad(_dev(E.pow2(args, k)), ups)
        assert all(torch.equal(a, b) for a, b in zip(m1, m2)), k
        assert torch.equal(g2[..., 0], g1[..., 0] * 2.0 ** k) and torch.equal(g2[..., 1], g1[..., 1]), k


# ---- F: the backward reads ``saved``, not the workspace -----------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ("single", "network"))
def test_f_backward_after_the_workspace_was_rewritten(stream):
    from npf_gwwaveform_amd import functional as FN
    from test_hip_loglike_grad import _call

    rows = {tag: (args, parts) for tag, fac, args, parts in _rows("F")}
    (ax, px), (ay, py) = rows[f"F {stream} X"], rows[f"F {stream} Y"]
    dx, dy = _dev(ax), _dev(ay)
    ux, uy = E.ups_of("all", 3, 3, 1), E.ups_of("all", 9, 3, 2)
    _, gy0 = _grad(dy, uy)  # (the pool has Y's size from here on: X and Y share it)
    _, gx0 = _grad(dx, ux)
    print(f"LNLGRADEDGE F {stream}: error / gate X {_check(gx0, px, ux, 'F X'):.3g} Y {_check(gy0, py, uy, 'F Y'):.3g}")
    pool = FN._MATCH_WS[torch.cuda.current_device()][-1]

    def graph(dargs):
        h = dargs["h"].clone().requires_grad_()
        return h, _call(dargs, h)

    def backward(h, m, ups):
        torch.autograd.backward([getattr(m, o) for o in OUTS], [ups[u].to(DEV) for u in UPS])
        return h.grad

    for order in ("xy", "yx"):
        hx, mx = graph(dx)
        before = pool.clone()
        hy, my = graph(dy)  # more rows and a longer grid: X's workspace rows are overwritten
        assert FN._MATCH_WS[torch.cuda.current_device()][-1] is pool and not torch.equal(pool.view(torch.int64), before.view(torch.int64))
        if order == "xy":
            gx = backward(hx, mx, ux)
            gy = backward(hy, my, uy)
        else:
            gy = backward(hy, my, uy)
            gx = backward(hx, mx, ux)
        assert torch.equal(gx, gx0) and torch.equal(gy, gy0), order
