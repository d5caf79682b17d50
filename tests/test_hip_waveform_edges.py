"""The waveform kernels at their thread, grid and tie edges on the GPU: ``npf_waveform_match``, ``npf_waveform_match_bwd``,
``npf_waveform_loglike`` and ``npf_waveform_loglike_net`` on the inputs of tests/waveform_edge_cases.py (checked on the CPU by
tests/test_waveform_edges_host.py) against the float64 references of the feature suites.

Gates, unchanged: ``match_reference.ratios``, ``mismatch_reference.gate_ratio`` (at T = 262181 the worst-case error of a double sum,
T 2^-53 = 2.9e-11, is still 30 times inside its absolute 1e-9), ``loglike_reference.ratios`` and ``loglike_net_reference.ratios``.
The near-match family holds match, mismatch and overlap to ``|d| <= 2^-23 |ref| + 16 T 2^-53`` (``waveform_edge_cases.near_ratios``,
derived there).  Beyond the gates: the exact zeros of the gradient (padded rows, removed points, entries >= 2, degenerate rows), the
same bits from a second call, ``tau_index == 0`` and bit-equal ``corr`` / ``series`` columns where every grid time ties, the stated
constants where the correlation vanishes, and invariance under exact power-of-two scalings.  Every test prints its worst error /
gate."""
import math

import pytest
import torch

import loglike_net_reference as N
import loglike_reference as L1
import match_reference as M
import mismatch_reference as G
import waveform_edge_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID_FAMILIES = ("thread_edges", "long_grids")
_refs = {}


@pytest.fixture(scope="module")
def refs():
    """``refs(family, entry, **over)`` -> [(tag, factors, case, float64 reference, d_match [R])], computed once per module and left
    unchanged; ``over`` replaces arguments of the reference (the tie family's ``taus=None``)."""
    def get(family, entry, **over):
        kind = W._kind(entry)
        key = (family, kind, tuple(over))
        if key not in _refs:
            _refs[key] = [(tag, fac, case, W.reference(kind, case, **over),
                           torch.randn(case["h"].shape[0], generator=torch.Generator().manual_seed(700 + i)))
                          for i, (tag, fac, case) in enumerate(W.cases(family, entry))]
        return _refs[key]

    yield get
    _refs.clear()


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _report(what, r, worst):
    print(f"EDGES {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _same_bits(a, b, what):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: {name} differs between two calls"


def _ll_dict(got):
    d = {k: v for k, v in got.items() if v is not None}
    d["optimal_snr"] = d["hh"].sqrt()
    return d


# ---- one call of every entry point, twice ------------------------------------------------------------------------------------------------
def _match(case):
    from npf_gwwaveform_amd import functional as FN

    args = _dev(M.call_args(case))
    first = FN.waveform_match(**args, corr=True)
    _same_bits(first, FN.waveform_match(**args, corr=True), "match")
    got = {k: v.cpu() for k, v in first._asdict().items()}
    assert all(torch.isfinite(v).all() for v in got.values()), "a non-finite result"
    return got


def _grad(case, d_match):
    """(mismatch [R], d_h, forward tau_index) through the public path, for the incoming gradient ``d_match`` of the MATCH; twice."""
    from npf_gwwaveform_amd import functional as FN

    args = _dev(M.call_args(case))
    outs = []
    for _ in range(2):
        h = args["h"].clone().requires_grad_()
        mm = FN.waveform_mismatch(**dict(args, h=h))
        mm.backward(-d_match.to(DEV))
        outs.append((mm.detach(), h.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "d_h differs between two calls"
    fwd = FN.waveform_match(**args, want=("mismatch", "tau_index"))
    assert torch.equal(outs[0][0], fwd.mismatch), "the forward value differs from waveform_match(...).mismatch"
    got = outs[0][1].cpu()
    assert got.shape == case["h"].shape and torch.isfinite(got).all(), "a non-finite gradient"
    return outs[0][0].cpu(), got, fwd.tau_index.cpu()


def _loglike(case):
    from npf_gwwaveform_amd import functional as FN

    args = _dev(L1.call_args(case))
    first = FN.waveform_loglike(**args, series=True)
    _same_bits(first, FN.waveform_loglike(**args, series=True), "loglike")
    got = {k: v.cpu() for k, v in first._asdict().items()}
    assert all(torch.isfinite(v).all() for v in got.values()), "a non-finite result"
    return got


def _net(case):
    from npf_gwwaveform_amd import functional as FN

    args = _dev(N.call_args(case))
    first = FN.waveform_loglike_network(**args, series=True)
    _same_bits(first, FN.waveform_loglike_network(**args, series=True), "network")
    got = {k: v.cpu() for k, v in first._asdict().items()}
    assert all(torch.isfinite(v).all() for v in got.values()), "a non-finite result"
    return got


def _gradient_zeros(got, s, fac, case, ref, tag):
    """The exact zeros of tests/test_hip_mismatch.py: entries 2 .., removed points, points beyond the counts, degenerate rows."""
    n_z, T = fac["n_z"], fac["T"]
    assert (got[..., 2:] == 0).all(), tag
    assert (got[..., :2][s == 0] == 0).all(), tag
    if fac["regime"] == "removed":
        kill = case["kill"].repeat(n_z, 1)
        assert (kill.any() or T == 1) and torch.isnan(case["h"][kill]).all() and (got[kill] == 0).all(), tag
    if fac["counts"] is not None:
        beyond = (torch.arange(T).view(1, T) >= torch.tensor(fac["counts"]).view(-1, 1)).repeat(n_z, 1)
        assert (got[beyond] == 0).all(), tag
    assert (got[ref["degenerate"]] == 0).all(), tag


# ---- thread edges, long rows, long grids: the feature suites' gates --------------------------------------------------------------------
@pytest.mark.parametrize("family", GRID_FAMILIES + ("long_rows",))
def test_match_meets_the_float64_reference(family, refs):
    worst = {}
    for tag, fac, case, ref, _ in refs(family, "match"):
        got = _match(case)
        assert got["corr"].shape == (fac["n_z"] * W.B, max(fac["n_tau"] or 0, 1), 2) and got["gg"].shape == (W.B,), tag
        _report(f"{family} match {tag}", M.ratios(got, ref), worst)
        deg, live = ref["degenerate"], ~ref["degenerate"]
        for name, value in (("overlap", 0.0), ("match", 0.0), ("mismatch", 1.0), ("tau_index", 0), ("phase", 0.0)):
            assert (got[name][deg] == value).all(), (tag, name)
        assert (got["corr"][deg] == 0).all(), tag
        if fac["regime"] == "shift":
            assert (got["tau_index"][live] == case["j_star"]).all() and (got["mismatch"][live].abs() <= 1e-6).all(), tag
    print(f"EDGES worst of {family} match: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("family", GRID_FAMILIES + ("long_rows",))
def test_gradient_meets_the_float64_closed_form(family, refs):
    worst = 0.0
    for tag, fac, case, ref, d_match in refs(family, "grad"):
        _, got, index = _grad(case, d_match)
        want, s, _ = G.expected(case, d_match, ref=ref)
        r = G.gate_ratio(got[..., :2], want, s)
        print(f"EDGES {family} grad {tag}: error / gate {r:.3g}")
        worst = max(worst, r)
        assert r <= 1.0, (tag, r)
        assert torch.equal(index.long(), ref["tau_index"]), tag
        _gradient_zeros(got, s, fac, case, ref, tag)
        if fac["T"] > 1 and not ref["degenerate"].all():
            assert float(want.abs().max()) > 0, tag
    print(f"EDGES worst of {family} grad: {worst:.3g}")


@pytest.mark.parametrize("family", GRID_FAMILIES)
def test_loglike_meets_the_float64_reference(family, refs):
    worst = {}
    for tag, fac, case, ref, _ in refs(family, "loglike"):
        got = _loglike(case)
        assert got["series"].shape == (fac["n_z"] * W.B, max(fac["n_tau"] or 0, 1), 2), tag
        _report(f"{family} loglike {tag}", L1.ratios(_ll_dict(got), ref), worst)
        deg = ref["degenerate"]
        for name in ("snr", "lnl_max", "lnl_marg", "tau_index", "phase", "hh"):
            assert (got[name][deg] == 0).all(), (tag, name)
        assert (got["series"][deg] == 0).all(), tag
        if fac["regime"] == "shift":
            assert (got["tau_index"][~deg] == case["j_star"]).all(), tag
    print(f"EDGES worst of {family} loglike: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("family", GRID_FAMILIES)
def test_network_meets_the_float64_reference(family, refs):
    worst = {}
    for tag, fac, case, ref, _ in refs(family, "net"):
        got = _net(case)
        Rn, D = fac["n_z"] * W.B, fac["D"]
        assert got["hh_det"].shape == (Rn, D) and got["snr_det"].shape == (Rn, D) and got["dd_det"].shape == (W.B, D), tag
        _report(f"{family} net {tag}", N.ratios(_ll_dict(got), ref), worst)
        deg = ref["degenerate"]
        for name in ("snr", "lnl_max", "lnl_marg", "tau_index", "phase", "hh"):
            assert (got[name][deg] == 0).all(), (tag, name)
        assert (got["series"][deg] == 0).all(), tag
        if fac["regime"] == "shift":
            assert (got["tau_index"][~deg] == case["j_star"]).all(), tag
    print(f"EDGES worst of {family} net: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- ties: the smallest index, by construction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", W.ENTRIES)
def test_ties_take_the_smallest_index(entry, refs):
    """Zero frequencies: every grid time holds the same sum bit for bit, so the index is 0 in every row -- per lane, across the
    shuffles and across the waves -- and the values are those of the same inputs without a grid."""
    worst = {}
    for tag, fac, case, ref0, d_match in refs("ties", entry, taus=None):
        n = fac["n_tau"]
        if entry == "grad":
            _, got, index = _grad(case, d_match)
            assert (index == 0).all(), (tag, index)
            want, s, _ = G.expected(dict(case, taus=None), d_match, ref=ref0)
            r = dict(grad=G.gate_ratio(got[..., :2], want, s))
            _gradient_zeros(got, s, fac, case, ref0, tag)
        else:
            got = {"match": _match, "loglike": _loglike, "net": _net}[entry](case)
            assert (got["tau_index"] == 0).all(), (tag, got["tau_index"])
            cols = got["corr" if entry == "match" else "series"]
            assert cols.shape[1] == n and torch.equal(cols, cols[:, :1].expand_as(cols)), f"{tag}: the columns are not bit-equal"
            wide = "corr" if entry == "match" else "series"
            ref = dict(ref0, **{wide: ref0[wide].expand(-1, n, -1)})
            r = M.ratios(got, ref) if entry == "match" else (L1.ratios if entry == "loglike" else N.ratios)(_ll_dict(got), ref)
        _report(f"ties {entry} {tag}", r, worst)
    print(f"EDGES worst of ties {entry}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- vanishing correlations ----------------------------------------------------------------------------------------------------------
def test_cancelling_points_give_match_zero_and_a_zero_gradient(refs):
    """c_j = 0 to the last bit with hh gg > 0: match 0, mismatch 1, index 0, no NaN; the backward takes ``mag == 0`` and writes
    zeros; the saved row is finite."""
    from npf_gwwaveform_amd import functional as FN

    worst = {}
    for tag, fac, case, ref, d_match in refs("zero_corr", "match"):
        got = _match(case)
        for name, value in (("match", 0.0), ("mismatch", 1.0), ("tau_index", 0), ("overlap", 0.0), ("phase", 0.0)):
            assert (got[name] == value).all(), (tag, name, got[name])
        assert (got["corr"] == 0).all(), tag
        _report(f"zero_corr match {tag}", M.ratios({k: got[k] for k in ("hh", "gg", "match", "mismatch", "overlap", "corr", "tau_index")}, ref),
                worst)
        mm, grad, index = _grad(case, d_match)
        assert (mm == 1).all() and (index == 0).all() and (grad == 0).all(), tag
        args = _dev(M.call_args(case))
        geo = FN.check_match_args(args["h"].shape, args["g"], args["weights"], args["freqs"], args["taus"])
        saved = torch.full((case["h"].shape[0], 4), math.nan, dtype=torch.float64, device=DEV)
        FN._match_launch(args["h"], args["g"], args["weights"], args["freqs"] if geo[8] > 0 else None, None, geo, ("tau_index",), False, saved)
        sv = saved.cpu()
        assert torch.isfinite(sv).all() and (sv[:, 2:] == 0).all() and (sv[:, :2] > 0).all(), tag
        assert float(((sv[:, 0] - ref["hh"]).abs() / ref["hh"]).max()) <= 1e-12, tag
    print("EDGES worst of zero_corr match: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("entry", ("loglike", "net"))
def test_zero_data_give_minus_half_hh(entry, refs):
    """A live template against data that are all zero: x_j = 0 for every j, ln I0(0) = 0 and atan2(0, 0).  lnl_max = lnl_marg =
    -hh / 2 exactly (of the kernel's own hh), snr 0, phase 0, index 0, snr_det 0; everything else at the reference's gates."""
    worst = {}
    for tag, fac, case, ref, _ in refs("zero_corr", entry):
        got = (_loglike if entry == "loglike" else _net)(case)
        for name in ("snr", "phase", "tau_index", "dd"):
            assert (got[name] == 0).all(), (tag, name, got[name])
        assert torch.equal(got["lnl_max"], -0.5 * got["hh"]) and torch.equal(got["lnl_marg"], -0.5 * got["hh"]), tag
        live = ~ref["degenerate"]
        assert live.any() and (got["hh"][live] > 0).all() and (got["series"][..., 1] == 0).all(), tag
        assert torch.equal(got["series"][..., 0], (-0.5 * got["hh"]).view(-1, 1).expand_as(got["series"][..., 0])), tag
        if entry == "net":
            assert (got["snr_det"] == 0).all() and (got["dd_det"] == 0).all() and (got["hh_det"][live] > 0).all(), tag
        d = _ll_dict({k: v for k, v in got.items() if k != "phase"})  # (the reference's atan2 of signed zeros is not the constant)
        _report(f"zero_corr {entry} {tag}", (L1.ratios if entry == "loglike" else N.ratios)(d, ref), worst)
    print(f"EDGES worst of zero_corr {entry}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- mismatches of 1e-4 .. 1e-8 --------------------------------------------------------------------------------------------------------
def test_near_match_meets_the_tightened_gate(refs):
    worst, worst_near = {}, {}
    for tag, fac, case, ref, _ in refs("near_match", "match"):
        got = _match(case)
        _report(f"near_match match {tag} (the feature suite's gates)", M.ratios(got, ref), worst)
        _report(f"near_match match {tag} (2^-23 |ref| + 16 T 2^-53)", W.near_ratios(got, ref, fac["T"]), worst_near)
    print("EDGES worst of near_match match: " + ", ".join(f"{k} {v:.3g}" for k, v in worst_near.items()) +
          "; at the feature suite's gates: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_near_match_gradient_meets_the_float64_closed_form(refs):
    worst = 0.0
    for tag, fac, case, ref, d_match in refs("near_match", "grad"):
        _, got, index = _grad(case, d_match)
        want, s, _ = G.expected(case, d_match, ref=ref)
        r = G.gate_ratio(got[..., :2], want, s)
        print(f"EDGES near_match grad {tag}: error / gate {r:.3g}")
        worst = max(worst, r)
        assert r <= 1.0 and torch.equal(index.long(), ref["tau_index"]) and (got[..., 2:] == 0).all(), (tag, r)
    print(f"EDGES worst of near_match grad: {worst:.3g}")


# ---- exact scalings ------------------------------------------------------------------------------------------------------------------
def _ulp(x):
    x = x.abs().float()
    return (torch.nextafter(x, torch.full_like(x, math.inf)) - x).double()


def test_power_of_two_scalings_leave_the_match_unchanged(refs):
    """Amplitudes times 2^+-40, weights times 2^+-20: against the float64 reference of the scaled inputs (the feature suite's gates),
    and against the unscaled call on the device -- index equal; match, overlap and every corr component within one fp32 ulp; the
    gradient with respect to A the unscaled one divided by h's amplitude factor within ``gate_ratio``.  The bits agree as well, and
    that is asserted: every product and sum of the kernels scales by an exact power of two (no double over- or underflows at
    2^+-200), hh gg scales by the even power (s_w s_h s_g)^2, so its square root scales exactly, and the fp32 roundings of scaled
    normal numbers are the scaled roundings."""
    worst = {}
    for tag, fac, case, ref, d_match in refs("scaled", "match"):
        got, base = _match(case), _match(fac["base"])
        _report(f"scaled match {tag}", M.ratios(got, ref), worst)
        assert torch.equal(got["tau_index"], base["tau_index"]), tag
        for name in ("match", "overlap", "corr"):
            assert ((got[name].double() - base[name].double()).abs() <= _ulp(base[name])).all(), (tag, name)
        hh_fac, gg_fac = fac["s_w"] * fac["s_h"] ** 2, fac["s_w"] * fac["s_g"] ** 2
        bits = {k: torch.equal(got[k], base[k]) for k in ("match", "mismatch", "overlap", "phase", "corr")}
        bits.update(hh=torch.equal(got["hh"].double(), base["hh"].double() * hh_fac), gg=torch.equal(got["gg"].double(), base["gg"].double() * gg_fac))
        _, grad, _ = _grad(case, d_match)
        _, grad0, _ = _grad(fac["base"], d_match)
        back = torch.stack([grad[..., 0].double() * fac["s_h"], grad[..., 1].double()], -1)  # (a power of two: exact)
        bits["grad"] = torch.equal(back, grad0[..., :2].double())
        want, s, _ = G.expected(case, d_match, ref=ref)
        r = dict(grad=G.gate_ratio(grad[..., :2], want, s))
        _, s0, _ = G.expected(fac["base"], d_match)
        r["grad_vs_unscaled"] = G.gate_ratio(back, grad0[..., :2].double(), s0)
        _report(f"scaled grad {tag}", r, worst)
        _gradient_zeros(grad, s, fac, case, ref, tag)
        print(f"EDGES scaled {tag}: bits equal to the unscaled call: " + ", ".join(f"{k} {v}" for k, v in bits.items()))
        assert all(bits.values()), (tag, bits)
    print("EDGES worst of scaled: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
