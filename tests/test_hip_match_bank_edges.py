"""The bank match at its pass, wave, workgroup, grid, tie and scale edges on the GPU: ``npf_waveform_match_bank`` on the inputs of
tests/match_bank_edge_cases.py (which says what path of which launch every family reaches; checked on the CPU by
tests/test_match_bank_edges_host.py) against the float64 reference of tests/match_bank_reference.py.

Gates, unchanged (``match_bank_reference.ratios``): match, mismatch and best_match |d| <= 1e-9 + 2^-23 |ref|; hh, gg |d| <= 2^-23 |ref|;
phase 1e-6 where the reference match is >= 1e-3; dot |d| <= 1e-9 sqrt(hh gg); tau_index and best_index exact.  The derivation scales as
about 4 T 2^-53 on the normalised quantities (``waveform_edge_cases.near_ratios``): 4.6e-13 at T = 1025, the longest row here, still far
below the absolute 1e-9.  Beyond the gates: the same bits from a second call, removed points against cut ones bit for bit, the tie
rules (the smallest template index, the first shift index) at bit-exact ties whose expected indices are known by construction,
invariance under exact power-of-two scalings and under permutations of the templates and of the rows, and a workspace that carries
nothing from a larger call into a smaller one.  Every test prints its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import match_bank_edge_cases as E
import match_bank_reference as RB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = ("match", "mismatch", "tau_index", "phase", "dot")


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _bits(x):
    return x if not x.is_floating_point() else x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def _same_bits(a, b, what, names=None):
    for name in names or a:
        assert (a[name] is None) == (b[name] is None), (what, name)
        if a[name] is not None:
            assert a[name].shape == b[name].shape and torch.equal(_bits(a[name]), _bits(b[name])), f"{what}: {name} differs"


def _call(args, twice=True, **kw):
    """One call with every output and ``dot`` -> dict of CPU tensors; ``twice``: a second call must give the same bits."""
    from npf_gwwaveform_amd import functional as FN

    args = _dev(args)
    kw = dict(dict(dot=True), **kw)
    got = {k: (None if v is None else v.cpu()) for k, v in FN.waveform_match_bank(**args, **kw)._asdict().items()}
    if twice:
        again = {k: (None if v is None else v.cpu()) for k, v in FN.waveform_match_bank(**args, **kw)._asdict().items()}
        _same_bits(got, again, "two calls")
    return got


def _finite(got, what):
    assert all(torch.isfinite(v).all() for v in got.values() if v is not None), f"{what}: a non-finite result"


def _report(what, r, worst):
    print(f"BANK EDGES {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _worst(family, worst):
    print(f"BANK EDGES worst over {family}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 1: a second and a third pass over the points ------------------------------------------------------------------------------------
def test_point_passes_meet_the_reference():
    worst = {}
    for tag, fac, case, ref in E.references("point_passes"):
        got = _call(E.call_args(case))
        _finite(got, tag)
        _report(f"point_passes {tag}", RB.ratios(got, ref), worst)
    _worst("point_passes", worst)


# ---- 2: removed points in patterns ---------------------------------------------------------------------------------------------------
def test_removed_patterns_equal_the_cut_call_bit_for_bit():
    worst = {}
    for tag, fac, case, ref in E.references("removed_patterns"):
        got = _call(E.call_args(case))
        cut = _call(fac["cut"], twice=False)
        _same_bits(got, cut, f"{tag}: {int(fac['kill'].sum())} of {E.REMOVED_PTS} points removed against the same points cut")
        _finite(got, tag)
        if fac["tied"] == "all":  # one live point: every template and shift ties; the indices are not the reference's to give
            got = {k: got[k] for k in ("match", "hh", "gg", "dot")}
            assert float((cut["match"] - 1.0).abs().max()) <= 2.0 ** -23, tag
        _report(f"removed_patterns {tag}", RB.ratios(got, ref), worst)
    _worst("removed_patterns", worst)


# ---- 3: banks of several workgroups and strides ----------------------------------------------------------------------------------------
def test_wide_banks_find_the_planted_templates_in_every_tile_and_stride():
    from npf_gwwaveform_amd import functional as FN

    worst = {}
    for tag, fac, case, ref in E.references("wide_banks"):
        got = _call(E.call_args(case))
        _finite(got, tag)
        assert got["match"].shape == (7, fac["n_bank"]) and got["best_index"].shape == (7,), tag
        assert got["best_index"].tolist() == fac["pick"], f"{tag}: best_index {got['best_index'].tolist()}, planted {fac['pick']}"
        assert got["tau_index"][torch.arange(7), torch.tensor(fac["pick"])].tolist() == fac["j_star"], tag
        _report(f"wide_banks {tag}", RB.ratios(got, ref), worst)
        if fac["n_bank"] == 129:  # best_* without match: the workspace copy of the matches, with a row stride over 64
            args = _dev(E.call_args(case))
            for want in (("best_index",), ("best_match", "best_index", "hh")):
                part = FN.waveform_match_bank(**args, want=want)._asdict()
                for name, x in part.items():
                    assert (x is not None) == (name in want), (want, name)
                _same_bits({k: part[k].cpu() for k in want}, got, f"{tag} want={want}", names=want)
    _worst("wide_banks", worst)


# ---- 4: long grids -------------------------------------------------------------------------------------------------------------------
def test_long_grids_keep_the_maximiser_of_any_chunk():
    worst = {}
    for tag, fac, case, ref in E.references("long_grids"):
        got = _call(E.call_args(case))
        _finite(got, tag)
        pick = torch.tensor(fac["pick"])
        assert got["tau_index"][torch.arange(7), pick].tolist() == fac["j_star"], \
            f"{tag}: tau_index {got['tau_index'][torch.arange(7), pick].tolist()}, planted {fac['j_star']}"
        assert got["best_index"].tolist() == fac["pick"], tag
        _report(f"long_grids {tag}", RB.ratios(got, ref), worst)
    _worst("long_grids", worst)


# ---- 5: ties -------------------------------------------------------------------------------------------------------------------------
def test_tied_templates_give_the_smallest_index_and_tied_shifts_the_first():
    """The expected indices come by construction, not from the reference (its ``exp`` does not give bit-equal columns): a copy of
    template g1 is the same sequence of operations on the same operands in another tile, wave, workgroup or stride."""
    worst = {}
    for tag, fac, case, ref in E.references("ties"):
        got = _call(E.call_args(case))
        _finite(got, tag)
        if fac["tied"] in ("columns", "bank"):
            g1 = fac["g1"]
            for g2 in fac["copies"]:
                for name in PAIRS:
                    assert torch.equal(_bits(got[name][:, g2]), _bits(got[name][:, g1])), f"{tag}: {name} of template {g2} and of {g1} differ"
                assert torch.equal(_bits(got["gg"][g2]), _bits(got["gg"][g1])), tag
            assert got["best_index"].tolist() == fac["pick"], f"{tag}: best_index {got['best_index'].tolist()}, expected {fac['pick']}"
            assert torch.equal(_bits(got["best_match"]), _bits(got["match"][torch.arange(3), torch.tensor(fac["pick"])])), tag
            keep = {k: v for k, v in got.items() if k != "best_index"}  # (the reference may name a copy)
            _report(f"ties {tag}", RB.ratios(keep, ref), worst)
        else:
            assert (got["tau_index"] == 0).all(), f"{tag}: {int((got['tau_index'] != 0).sum())} pairs leave the first of the tied shifts"
            plain = _call(dict(E.call_args(case), taus=None), twice=False)
            _same_bits(got, plain, f"{tag} against the call without a grid")
            keep = {k: v for k, v in got.items() if k != "tau_index"}  # (the reference's shifts tie to rounding only)
            _report(f"ties {tag}", RB.ratios(keep, ref), worst)
    _worst("ties", worst)


# ---- 6: exact scalings -----------------------------------------------------------------------------------------------------------------
def test_power_of_two_scalings_keep_every_bit():
    """Every step is a multiplication by a power of two without underflow or overflow, which commutes with rounding; the square root
    of an even power of two is exact."""
    for tag, fac, case in E.cases("scaled"):
        got, base = _call(E.call_args(case)), _call(E.call_args(fac["base"]), twice=False)
        _finite(got, tag)
        a, b, c = fac["a"], fac["b"], fac["c"]
        _same_bits(got, base, tag, names=("match", "mismatch", "tau_index", "phase", "best_index", "best_match"))
        assert torch.equal(got["dot"], base["dot"] * 2.0 ** (a + b + c)), f"{tag}: dot is not the unscaled dot times 2^{a + b + c}"
        for name, p in (("hh", 2 * a + c), ("gg", 2 * b + c)):
            want = base[name].double() * 2.0 ** p
            assert (want > 2.0 ** -126).all() and (want < 2.0 ** 127).all(), tag  # (it fits fp32)
            assert torch.equal(got[name].double(), want), f"{tag}: {name} is not the unscaled {name} times 2^{p}"
        print(f"BANK EDGES scaled {tag}: every output keeps its bits")


# ---- 7: the ends of the fp32 range -----------------------------------------------------------------------------------------------------
def test_extreme_amplitudes_weights_and_phases_meet_the_reference():
    worst = {}
    for tag, fac, case, ref in E.references("extremes"):
        got = _call(E.call_args(case))
        for name in ("match", "mismatch", "phase", "dot", "best_match"):
            assert torch.isfinite(got[name]).all(), f"{tag}: {name} is not finite"
        assert (got["match"] > 0).all(), f"{tag}: a degenerate pair"
        r = RB.ratios({k: v for k, v in got.items() if k not in ("hh", "gg")}, ref)
        for name in ("hh", "gg"):  # the reference cast to fp32 may be inf, 0 or denormal: equal to that cast, or 2^-23 relative
            x, want = got[name], ref[name].float()
            d = (x.double() - ref[name]).abs() / (2.0 ** -23 * ref[name].abs())
            q = torch.where(_bits(x) == _bits(want), torch.zeros_like(d), d)
            r[name] = float(torch.where(torch.isfinite(q), q, torch.full_like(q, math.inf)).max())
        _report(f"extremes {tag}", r, worst)
    _worst("extremes", worst)


# ---- 8: permutations -------------------------------------------------------------------------------------------------------------------
def test_permuted_templates_and_rows_permute_every_output_bit_for_bit():
    """Every output element is the same sequence of operations on the same operands wherever its tile, wave and fragment position
    sit; the margins are >= 1e-6 (host test), so no winner moves for a tie."""
    for tag, fac, case in E.cases("permutations"):
        got, base = _call(E.call_args(case)), _call(E.call_args(fac["base"]), twice=False)
        _finite(got, tag)
        perm = fac["perm"]
        if fac["axis"] == "bank":
            inverse = torch.empty_like(perm)
            inverse[perm] = torch.arange(len(perm))
            want = {k: base[k][:, perm] for k in PAIRS}
            want.update(hh=base["hh"], gg=base["gg"][perm], best_match=base["best_match"],
                        best_index=inverse[base["best_index"].long()].to(torch.int32))
        else:
            want = {k: v[perm] for k, v in base.items() if k != "gg"}
            want["gg"] = base["gg"]
        for name in want:
            differ = _bits(got[name]) != _bits(want[name])
            where = differ.nonzero()[:4].tolist()
            assert not differ.any(), f"{tag}: {name} is not the permuted original at {int(differ.sum())} elements, the first at {where}"
        print(f"BANK EDGES permutations {tag}: every output is the permuted original")


# ---- 9: the shared workspace -----------------------------------------------------------------------------------------------------------
def test_a_small_call_after_the_largest_one_gives_the_bits_it_gave_before():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()

    def ws_bytes(fac, case):
        a = E.call_args(case)
        n_tau = a["taus"][2] if a["taus"] is not None else 0
        return int(lib.npf_waveform_match_bank_workspace_bytes(a["h"].shape[0], a["bank"].shape[0], a["h"].shape[1], n_tau))

    every = [(ws_bytes(fac, case), tag, fac, case) for family in E.FAMILIES for tag, fac, case in E.cases(family)]
    n_big, tag, fac, big = max(every, key=lambda x: x[0])
    small = RB.build(3, 3, 37, 5, seed=9900)
    n_small = ws_bytes(None, small)
    assert n_big > 20 * n_small
    first = _call(E.call_args(small), twice=False)
    large = _call(E.call_args(big), twice=False)
    again = _call(E.call_args(small), twice=False)
    _same_bits(first, again, f"3 x 3 x 37 x 5 before and after '{tag}'")
    _finite(first, "the small call")
    r = RB.ratios(again, RB.reference(**E.call_args(small)))
    print(f"BANK EDGES workspace of {n_small} bytes after one of {n_big} ({tag}): error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert large["match"].shape == (fac["n_rows"], fac["n_bank"])
