"""The distance-marginalised likelihood at its grid, scale, tie and size edges on the GPU: ``npf_waveform_loglike_dist`` and
``npf_waveform_loglike_net_dist`` (``waveform_scale_marg_kernel``, ``waveform_scale_finish_kernel``) on the inputs of
tests/loglike_dist_edge_cases.py (checked on the CPU by tests/test_loglike_dist_edges_host.py) against
``loglike_dist_reference.marginalise`` of the parent's float64 reference.

Gates, unchanged (``loglike_dist_reference.ratios``): lnl_dist, lnl_dist_mix |d| <= 1e-10 S_r + 1e-12; post, post_mix twice that, -inf
entries exact; scale_hat, lnl_amp_max 1e-10 relative + 1e-12; scale_index exact; no NaN; sum_i exp(post_i) = 1 to 1e-12 where a scale
is live; every ``base`` field bit-equal to the plain call; a second call gives the same bits.  Every test prints its worst error /
gate per quantity.

What is covered, by test:

A  the path beyond the LDS cache, the largest dynamic-LDS request, 4096 / 4097, the finishing stride at 255 / 256, the last partial
   stride at 4099             test_time_grid_edges_meet_the_reference, test_one_unit_scale_is_lnl_marg_across_the_lds_boundary
B  n_a at 255 / 256 / 4095 / 4096, dead first and last chunks, the maximum at the last index
                              test_scale_axis_edges_meet_the_reference, test_post_and_post_mix_are_written_whole_at_the_largest_grid
C  ties in scale_index at every level of the reduction, flat evidence, ties in x*
                              test_duplicated_best_scale_returns_the_smallest_index, test_flat_evidence_ties_every_scale,
                              test_tied_shifts_meet_the_reference
D  u at 1e6, scales of 2^-600, a grid over 2^+-30, a x* on the ln I0 switch point
                              test_magnitudes_meet_the_reference
E  both branches of the mixture's running log-sum-exp
                              test_mixture_does_not_depend_on_the_order_of_its_rows
F  the network twin at D = 8  test_eight_detectors_meet_the_reference
G  the shared workspace       test_results_do_not_depend_on_earlier_calls"""
import math

import pytest
import torch

import loglike_dist_edge_cases as E
import loglike_dist_reference as Dd
import match_reference as M
from test_hip_loglike_dist import DEV, F64, _call, _check, _dev, _new, _plain, _same_bits, _sums_to_one

pytestmark = pytest.mark.gpu
STREAMS = pytest.mark.parametrize("network", (False, True), ids=("single", "network"))


def _attains(idx, dist, tag):
    """The returned index attains the reference maximum within one gate (rows with a live scale)."""
    u, rows = dist["u"], dist["live"].any(1)
    at = u.gather(1, idx.long().cpu().view(-1, 1))[:, 0]
    assert (at[rows] >= u.max(1).values[rows] - (1e-10 * dist["S"] + 1e-12)[rows]).all(), f"{tag}: scale_index misses the maximum"


def _full(network, tag, fac, case, s, p, ref, dist, worst, index="exact"):
    """Every rule of the module's docstring on one case -> the first call's result.  ``index``: "exact" (against ``dist``, whose
    ``scale_index`` a caller may have set by construction) or "attains"."""
    first = _call(network, case, s, p, posterior=True)
    _same_bits(first, _call(network, case, s, p, posterior=True), tag)
    got = _new(first)
    Rn, n_a = fac["n_z"] * Dd.B, fac["n_a"]
    assert got["post"].shape == (Rn, n_a) and got["post_mix"].shape == (Dd.B, n_a) and got["lnl_dist_mix"].shape == (Dd.B,), tag
    assert all(got[k].shape == (Rn,) for k in ("lnl_dist", "scale_index", "scale_hat", "lnl_amp_max")), tag
    assert not any(torch.isnan(v).any() for v in got.values()), f"{tag}: NaN"
    if index == "attains":
        _attains(got.pop("scale_index"), dist, tag)
    _check(got, ref, dist, tag, worst)
    live_any = dist["live"].any(1)
    worst["sum"] = max(worst.get("sum", 0.0), _sums_to_one(first.post, live_any, tag),
                       _sums_to_one(first.post_mix, live_any.view(-1, Dd.B).any(0), tag))
    assert (first.lnl_dist.cpu()[~live_any] == -math.inf).all() and (first.scale_index.cpu()[~live_any] == 0).all(), tag
    deg = ref["degenerate"]
    assert (first.scale_hat.cpu()[deg] == 0).all() and (first.lnl_amp_max.cpu()[deg] == 0).all(), tag
    plain = _plain(network, case)
    for name in plain._fields:
        x, y = getattr(first.base, name), getattr(plain, name)
        assert (x is None and y is None) or torch.equal(x, y), (tag, "base", name)
    return first


def _rows(family, network):
    return [(tag, fac, case, s, p, *E.reference(network, case, s, p, no_grid=family == "shift_ties"))
            for tag, fac, case, s, p in E.cases(family, network)]


def _summary(what, network, n, worst):
    total = worst.pop("sum", 0.0)
    print(f"LOGLIKE_DIST_EDGES worst over the {n} cases of {what}, {'network' if network else 'single'}: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; |sum exp(post) - 1| {total:.3g}")


# ---- A: time-grid edges ------------------------------------------------------------------------------------------------------------
@STREAMS
def test_time_grid_edges_meet_the_reference(network):
    """n_tau 255, 256, 4095, 4096 (x_j in 32 KiB of dynamic LDS), 4097 (no LDS: the candidates are read again, with that path's own
    rule for HH == 0) and 4099 with the maximiser at the last index; two chunks of scales on the same candidates."""
    worst, rows = {}, _rows("time_edges", network)
    for tag, fac, case, s, p, ref, dist in rows:
        _full(network, tag, fac, case, s, p, ref, dist, worst)
    _summary("the time-grid edges", network, len(rows), worst)


@STREAMS
def test_one_unit_scale_is_lnl_marg_across_the_lds_boundary(network):
    """One scale a = 1 with ln pi = 0: lnl_dist is the parent's lnl_marg within the gate, on either side of n = 4096."""
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    sizes = set()
    for tag, fac, case, _, _ in E.cases("time_edges", network):
        if fac["regime"] != "noise" and fac["n_tau"] != E.A_LAST:
            continue
        sizes.add(fac["n_tau"])
        dist = Dd.marginalise(E.parent_reference(network, case), one, zero)
        m = _call(network, case, one, zero, posterior=True)
        gate = 1e-10 * dist["S"] + 1e-12
        d = (m.lnl_dist - m.base.lnl_marg).abs().cpu()
        print(f"LOGLIKE_DIST_EDGES n_a=1 a=1 ln pi=0 {'network ' if network else ''}n_tau={fac['n_tau']}: lnl_dist bit-equal to lnl_marg: "
              f"{torch.equal(m.lnl_dist, m.base.lnl_marg)}; worst error / gate {float((d / gate).max()):.3g}")
        assert (d <= gate).all(), tag
        assert ((m.lnl_dist_mix - m.base.lnl_mix).abs().cpu() <= gate.view(-1, Dd.B).max(0).values).all(), tag
        assert (m.post == 0).all() and float(m.post_mix.abs().max()) <= 1e-14 and (m.scale_index == 0).all(), tag
    assert sizes == set(E.A_SIZES) | {E.A_LAST}


# ---- B: scale-axis edges -----------------------------------------------------------------------------------------------------------
@STREAMS
def test_scale_axis_edges_meet_the_reference(network):
    """n_a 255, 256 (launch B's stride), 4095, 4096 (256 chunks, the last partial or full) with and without a time grid; a dead last
    chunk writes only -inf, a dead first chunk is skipped by scale_index (16), the descending grid has its maximum at n_a - 1."""
    worst, rows = {}, _rows("scale_edges", network)
    for tag, fac, case, s, p, ref, dist in rows:
        first = _full(network, tag, fac, case, s, p, ref, dist, worst)
        want = {"dead_first": E.SC, "rev": fac["n_a"] - 1}.get(fac["kind"], 0)
        assert (first.scale_index == want).all(), (tag, first.scale_index)
    _summary("the scale-axis edges", network, len(rows), worst)


def test_post_and_post_mix_are_written_whole_at_the_largest_grid():
    """n_a = 4096.  The outputs come from the caching allocator: blocks of their sizes are filled with NaN and freed just before the
    call."""
    import loglike_reference as R1

    case = R1.build("noise", 37, n_z=3, h_ld=2, fform="T", taus=R1.grid(17), seed=4)
    n_a = E.MAX_SCALES
    for kind in ("geo", "dead", "dead_last", "dead_first"):
        s, p = E.edge_grid(n_a, "A", "A", kind)
        _call(False, case, s, p, posterior=True)
        torch.cuda.synchronize()
        junk = [torch.full(shape, math.nan, **F64) for shape in ((9, n_a), (3, n_a), (9,), (9,), (9,), (3,)) for _ in range(2)]
        del junk
        m = _call(False, case, s, p, posterior=True)
        assert not any(torch.isnan(v).any() for v in _new(m).values()), kind
        live = Dd.live_mask(s, p)
        assert (m.post[:, ~live.to(DEV)] == -math.inf).all() and torch.isfinite(m.post[:, live.to(DEV)]).all(), kind
        assert (m.post_mix[:, ~live.to(DEV)] == -math.inf).all() and torch.isfinite(m.post_mix[:, live.to(DEV)]).all(), kind


# ---- C: ties ---------------------------------------------------------------------------------------------------------------------
@STREAMS
def test_duplicated_best_scale_returns_the_smallest_index(network):
    """The best (a, ln pi) pair stands at an index set: scale_index is the set's smallest member BY CONSTRUCTION (not taken from the
    reference, whose vectorised sums need not give bit-equal duplicates), and the members' posteriors are bit-equal: every u_i is
    summed in one fixed order, whichever workgroup computes it."""
    worst, rows = {}, _rows("duplicated_best", network)
    for tag, fac, case, s, p, ref, dist in rows:
        members = list(fac["set"])
        planted = dict(dist, scale_index=torch.full_like(dist["scale_index"], min(members)))
        first = _full(network, tag, fac, case, s, p, ref, planted, worst)
        assert (first.scale_index == min(members)).all(), (tag, first.scale_index)
        for i in members[1:]:
            assert torch.equal(first.post[:, i], first.post[:, members[0]]) and torch.equal(first.post_mix[:, i], first.post_mix[:, members[0]]), (tag, i)
    _summary("the duplicated best scale", network, len(rows), worst)


@STREAMS
def test_flat_evidence_ties_every_scale(network):
    """HH == 0 on every row and a constant log prior: u_i = ln pi exactly, so scale_index is 0, the posteriors of a row are bit-equal
    and lnl_dist = ln pi + ln n_a; n_tau = 4097 takes the degenerate rule of the path beyond the LDS cache."""
    worst, rows = {}, _rows("flat_evidence", network)
    for tag, fac, case, s, p, ref, dist in rows:
        planted = dict(dist, scale_index=torch.zeros_like(dist["scale_index"]))
        first = _full(network, tag, fac, case, s, p, ref, planted, worst)
        assert (first.scale_index == 0).all(), tag
        assert (first.post == first.post[:, :1]).all() and (first.post_mix == first.post_mix[:, :1]).all(), tag
        d = float((first.lnl_dist - (E.FLAT_LP + math.log(fac["n_a"]))).abs().max())
        assert d <= 1e-10 * abs(E.FLAT_LP) + 1e-12, (tag, d)
    _summary("flat evidence", network, len(rows), worst)


@STREAMS
def test_tied_shifts_meet_the_reference(network):
    """Zero frequencies: every shift gives the same candidate bit for bit, x* is that value, tau_index 0, every term of S_i is 1 and
    u_i = M_i -- the reference is that of the same inputs without a grid."""
    worst, rows = {}, _rows("shift_ties", network)
    for tag, fac, case, s, p, ref, dist in rows:
        first = _full(network, tag, fac, case, s, p, ref, dist, worst)
        assert (first.base.tau_index == 0).all(), tag
    _summary("tied shifts", network, len(rows), worst)


# ---- D: magnitudes -----------------------------------------------------------------------------------------------------------------
@STREAMS
def test_magnitudes_meet_the_reference(network):
    """u of 1e6 (sum exp(post) = 1 to 1e-12 is the header's claim); scales of 2^-600 .. 2^-20, where a^2 HH and the series argument
    underflow; 2^-30 .. 2^30, where a^2 HH / 2 reaches 1e18; 17 scales with a x* within 8 x 2^-50 of the ln I0 switch point, on
    whichever side the kernel's own x* puts them.  scale_index is exact everywhere: the host test finds the maximum clear in each
    case (on the wide grid by the per-scale margin, so the index must also attain the reference maximum within the row gate)."""
    worst, rows = {}, _rows("magnitudes", network)
    for tag, fac, case, s, p, ref, dist in rows:
        first = _full(network, tag, fac, case, s, p, ref, dist, worst)
        _attains(first.scale_index, dist, tag)
        assert torch.isfinite(first.post).all() and torch.isfinite(first.lnl_dist).all(), tag
        if fac["sub"] == "u1e6":
            assert float(first.lnl_dist.min()) > 1e6, tag
    _summary("the magnitudes", network, len(rows), worst)


# ---- E: the order of the mixture's rows ----------------------------------------------------------------------------------------------
@STREAMS
def test_mixture_does_not_depend_on_the_order_of_its_rows(network):
    """The latent blocks in all six orders: the running log-sum-exp of launch B meets a larger row after a smaller one and a smaller
    after a larger.  "edge": rows a few units apart, each counts.  "loud": rows more than 745 apart, the other rows add nothing:
    lnl_dist_mix = max_s lnl_dist - ln 3, post_mix = the top row's post."""
    worst, rows = {}, _rows("mixture_orders", network)
    for tag, fac, case, s, p, ref, dist in rows:
        first = _full(network, tag, fac, case, s, p, ref, dist, worst)
        if not fac["apart"]:
            continue
        task_gate = (1e-10 * dist["S"] + 1e-12).view(3, Dd.B).max(0).values.to(DEV)
        lnl = first.lnl_dist.view(3, Dd.B)
        top = lnl.argmax(0)
        d_mix = (first.lnl_dist_mix - (lnl.max(0).values - math.log(3.0))).abs()
        d_post = (first.post_mix - first.post.view(3, Dd.B, -1)[top, torch.arange(Dd.B, device=DEV)]).abs()
        print(f"LOGLIKE_DIST_EDGES {tag}: top row at {top.tolist()}; lnl_dist_mix - (max - ln 3) / gate {float((d_mix / task_gate).max()):.3g}, "
              f"post_mix - post[top] / gate {float((d_post / (2.0 * task_gate.view(-1, 1))).max()):.3g}")
        assert (d_mix <= task_gate).all() and (d_post <= 2.0 * task_gate.view(-1, 1)).all(), tag
    _summary("the mixture orders", network, len(rows), worst)


# ---- F: eight detectors --------------------------------------------------------------------------------------------------------------
def test_eight_detectors_meet_the_reference():
    worst, rows = {}, _rows("eight_detectors", True)
    for tag, fac, case, s, p, ref, dist in rows:
        _full(True, tag, fac, case, s, p, ref, dist, worst)
    _summary("D = 8", True, len(rows), worst)


# ---- G: the shared workspace -----------------------------------------------------------------------------------------------------------
@STREAMS
def test_results_do_not_depend_on_earlier_calls(network):
    """Launch B reads the tail [x*, u_i] launch A left in the workspace the match and the other likelihoods write into as well: the
    result is the same bits after a larger distance call on other data (which may move the workspace), a plain likelihood, a
    ``waveform_match`` and a call of the other stream."""
    from npf_gwwaveform_amd import functional as FN

    ind = E.independence(network)
    case, s, p = ind["target"]
    first = _call(network, case, s, p, posterior=True)
    ref, dist = E.reference(network, case, s, p)
    _check(_new(first), ref, dist, f"{'network' if network else 'single'} before any other call")
    between = (("a distance call with n_a = 300, n_tau = 257", lambda: _call(network, *ind["big"], posterior=True)),
               ("a plain likelihood", lambda: _plain(network, ind["big"][0], series=True)),
               ("waveform_match", lambda: FN.waveform_match(**_dev(M.call_args(ind["match"])), corr=True)),
               ("a call of the other stream", lambda: _call(not network, *ind["other"], posterior=True)))
    for what, run in between:
        run()
        _same_bits(first, _call(network, case, s, p, posterior=True), what)
        print(f"LOGLIKE_DIST_EDGES {'network' if network else 'single'}: the same bits after {what}")
