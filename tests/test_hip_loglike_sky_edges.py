"""The sky-grid likelihood at its pass, tile, workgroup, wave, stride, grid and tie edges on the GPU: ``npf_waveform_loglike_sky`` on
the inputs of tests/loglike_sky_edge_cases.py (which says what path of which launch every family reaches; checked on the CPU by
tests/test_loglike_sky_edges_host.py) against the float64 reference of tests/loglike_sky_reference.py.

Gates, unchanged (``loglike_sky_reference.ratios``): lnl_sky, lnl_sky_mix and u = post + lnl_sky |d| <= 1e-10 scale + 1e-12, scale =
max_p (sqrt(HH_p DD) + HH_p / 2); post, post_mix twice that; snr, snr_map 1e-10 relative + 1e-12; the indices exact; -inf by -inf only
(derivation: the docstring of loglike_sky_edge_cases).  Beyond the gates: the planted indices, dead pixels against cut ones bit for
bit, both tie rules at bit-exact ties whose expected indices are known by construction, invariance under exact power-of-two scalings
and under a permutation of the pixels, a NaN in one live pixel, the same bits from a second call of the largest case.  Every test
prints its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import loglike_sky_edge_cases as E
import loglike_sky_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = ("lnl_sky", "pix_index", "tau_index", "snr")
MAPS = ("post", "snr_map", "post_mix")


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _bits(x):
    return x if not x.is_floating_point() else x.contiguous().view(torch.int64)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), f"{what}: the bits differ"


def _call(args):
    """One call with every output -> dict of CPU tensors."""
    from npf_gwwaveform_amd import functional as FN

    return {k: v.cpu() for k, v in FN.waveform_loglike_sky(**_dev(args), posterior=True, snr_map=True)._asdict().items()}


def _shapes(got, fac, tag):
    Rn, Bn, P = fac["rows"], fac["Bn"], fac["P"]
    assert set(got) == set(ROWS + MAPS + ("lnl_sky_mix",)), tag
    assert all(v.dtype == (torch.int32 if k.endswith("index") else torch.float64) for k, v in got.items()), tag
    assert all(got[k].shape == (Rn,) for k in ROWS) and got["lnl_sky_mix"].shape == (Bn,), tag
    assert got["post"].shape == (Rn, P) and got["snr_map"].shape == (Rn, P) and got["post_mix"].shape == (Bn, P), tag


def _report(family, tag, got, ref, worst, drop=()):
    r = S.ratios({k: v for k, v in got.items() if k not in drop}, ref)
    print(f"LOGLIKE_SKY_EDGES {family} {tag}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{family} {tag}: {r}"
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _worst(family, worst, n):
    print(f"LOGLIKE_SKY_EDGES worst over the {n} cases of {family}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _planted(got, fac, tag):
    assert (got["pix_index"] == fac["p0"]).all(), f"{tag}: pix_index {got['pix_index'].tolist()}, planted {fac['p0']}"
    assert (got["tau_index"] == fac["j0"]).all(), f"{tag}: tau_index {got['tau_index'].tolist()}, planted {fac['j0']}"


# ---- 1: a second to fifth pass over the points -----------------------------------------------------------------------------------------
def test_point_passes_meet_the_reference():
    worst = {}
    refs = E.references("point_passes")
    for tag, fac, case, ref in refs:
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        _report("point_passes", tag, got, ref, worst)
    _worst("point_passes", worst, len(refs))


# ---- 2: counts -------------------------------------------------------------------------------------------------------------------------
def test_counts_at_zero_inside_the_second_pass_beyond_the_points_and_negative():
    worst = {}
    refs = E.references("counts")
    for tag, fac, case, ref in refs:
        assert torch.isnan(case["h"]).any() and torch.isnan(case["data"]).any()
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        lp = case["log_prior"]
        gate = 1e-10 * ref["scale"] + 1e-12
        for r in fac["empty_rows"]:  # no live point: hh = 0, u_p = log_prior_p, snr 0
            assert ((got["post"][r] + got["lnl_sky"][r] - lp).abs() <= gate[r]).all(), tag
            assert got["snr"][r] == 0 and (got["snr_map"][r] == 0).all() and got["tau_index"][r] == 0, tag
            assert got["pix_index"][r] == int(lp.argmax()), tag
        cmp = dict(got)
        for r in fac["tau_tied_rows"]:  # one live point: every shift ties but for rounding; any index of the grid
            assert 0 <= int(got["tau_index"][r]) < fac["n_tau"], tag
            cmp["tau_index"] = got["tau_index"].clone()
            cmp["tau_index"][r] = ref["tau_index"][r]
        _report("counts", tag, cmp, ref, worst)
    _worst("counts", worst, len(refs))


# ---- 3: skies of several workgroups, waves and strides -----------------------------------------------------------------------------------
def test_wide_skies_find_the_planted_pixel_in_every_workgroup_wave_and_stride():
    worst = {}
    refs = E.references("wide_skies")
    for tag, fac, case, ref in refs:
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        _planted(got, fac, tag)
        _report("wide_skies", tag, got, ref, worst)
    _worst("wide_skies", worst, len(refs))


# ---- 4: dead pixels in patterns ----------------------------------------------------------------------------------------------------------
def test_dead_patterns_equal_the_cut_call_bit_for_bit():
    worst = {}
    refs = E.references("dead_patterns")
    for tag, fac, case, ref in refs:
        got, cut = _call(E.call_args(case)), _call(fac["cut"])
        _shapes(got, fac, tag)
        dead = fac["dead"]
        live = (~dead).nonzero()[:, 0]
        what = f"{tag}: {int(dead.sum())} of {E.DEAD_P} pixels dead against the same pixels cut"
        for name in ("lnl_sky", "lnl_sky_mix", "snr", "tau_index"):
            _same(got[name], cut[name], f"{what}, {name}")
        for name in MAPS:
            _same(got[name][:, live], cut[name], f"{what}, {name} at the live pixels")
        assert torch.equal(got["pix_index"].long(), live[cut["pix_index"].long()]), what
        assert (got["post"][:, dead] == -math.inf).all() and (got["post_mix"][:, dead] == -math.inf).all(), tag
        assert (got["snr_map"][:, dead] == 0).all(), tag
        assert all(torch.isfinite(got[k]).all() for k in ("lnl_sky", "lnl_sky_mix", "snr")), tag
        _planted(got, fac, tag)
        _report("dead_patterns", tag, got, ref, worst)
    _worst("dead_patterns", worst, len(refs))


# ---- 5: long grids -----------------------------------------------------------------------------------------------------------------------
def test_long_grids_keep_the_maximiser_of_any_chunk():
    worst = {}
    refs = E.references("long_grids")
    for tag, fac, case, ref in refs:
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        _planted(got, fac, tag)
        _report("long_grids", tag, got, ref, worst)
    _worst("long_grids", worst, len(refs))


# ---- 6: ties -----------------------------------------------------------------------------------------------------------------------------
def test_tied_pixels_give_the_smallest_index_and_tied_shifts_the_first():
    """The expected indices come by construction: a copy of pixel g1 is the same sequence of operations on the same operands in
    another lane, tile, wavefront, workgroup or stride; with zero frequencies every shift is the same sum."""
    worst = {}
    refs = E.references("ties")
    for tag, fac, case, ref in refs:
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        tied = fac["tied"]
        if tied in ("pixels", "sky"):
            g1 = fac["g1"]
            for g2 in fac["copies"]:
                for name in MAPS:
                    _same(got[name][:, g2], got[name][:, g1], f"{tag}: {name} of pixel {g2} and of {g1}")
            assert (got["pix_index"] == g1).all(), f"{tag}: pix_index {got['pix_index'].tolist()}, expected {g1}"
            assert (got["tau_index"] == fac["j0"]).all(), tag
            if tied == "sky":
                gate = 2.0 * (1e-10 * ref["scale"] + 1e-12)
                assert ((got["post"] + math.log(fac["P"])).abs() <= gate.view(-1, 1)).all(), tag
            _report("ties", tag, got, ref, worst, drop=("pix_index",))  # (the reference may name a copy)
        elif tied == "zero":
            assert (got["lnl_sky"].abs() <= 1e-12).all() and (got["lnl_sky_mix"].abs() <= 1e-12).all(), tag
            assert (got["pix_index"] == 0).all() and (got["tau_index"] == 0).all() and (got["snr"] == 0).all(), tag
            assert (got["snr_map"] == 0).all(), tag
            _report("ties", tag, got, ref, worst)
        else:
            assert (got["tau_index"] == 0).all(), f"{tag}: tau_index {got['tau_index'].tolist()} leaves the first of the tied shifts"
            assert (got["pix_index"] == fac["p0"]).all(), tag
            _report("ties", tag, got, ref, worst, drop=("tau_index",))  # (the reference's shifts tie to rounding only)
    _worst("ties", worst, len(refs))


# ---- 7: exact scalings -------------------------------------------------------------------------------------------------------------------
def test_power_of_two_scalings_keep_every_bit():
    """Every product entering K, hh_k |C|^2 and w |d|^2 scale by exactly 1 without underflow or overflow on the way."""
    worst = {}
    refs = E.references("scaled")
    base_got = {}
    for tag, fac, case, ref in refs:
        key = id(fac["base"])
        if key not in base_got:
            base_got[key] = _call(E.call_args(fac["base"]))
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        for name in got:
            _same(got[name], base_got[key][name], f"{tag}: {name}")
        _report("scaled", tag, got, ref, worst)
    _worst("scaled", worst, len(refs))


# ---- 8: value extremes -------------------------------------------------------------------------------------------------------------------
def test_denormal_amplitudes_large_phases_and_long_delays_meet_the_reference():
    worst = {}
    refs = E.references("extremes")
    for tag, fac, case, ref in refs:
        got = _call(E.call_args(case))
        _shapes(got, fac, tag)
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        _planted(got, fac, tag)
        _report("extremes", tag, got, ref, worst)
    _worst("extremes", worst, len(refs))


# ---- 9: permutations ---------------------------------------------------------------------------------------------------------------------
def test_permuted_pixels_permute_the_sky_map_bit_for_bit():
    worst = {}
    (tag, fac, case, ref), = E.references("permutations")
    got, base = _call(E.call_args(case)), _call(E.call_args(fac["base"]))
    _shapes(got, fac, tag)
    perm = fac["perm"]
    for name in MAPS:
        _same(got[name], base[name][:, perm], f"{tag}: {name}")
    for name in ("lnl_sky", "lnl_sky_mix", "snr", "tau_index"):
        _same(got[name], base[name], f"{tag}: {name}")
    assert torch.equal(perm[got["pix_index"].long()], base["pix_index"].long()), tag
    _report("permutations", tag, got, ref, worst)
    _worst("permutations", worst, 1)


# ---- 10: a NaN in a live pixel -------------------------------------------------------------------------------------------------------------
def test_a_nan_in_a_live_pixels_response_stays_in_its_column_of_the_snr_map():
    worst = {}
    (tag, fac, case, ref), = E.references("pixel_nan")
    got, clean = _call(E.call_args(case)), _call(E.call_args(fac["base"]))
    _shapes(got, fac, tag)
    others = [p for p in range(fac["P"]) if p != fac["bad"]]
    _same(got["snr_map"][:, others], clean["snr_map"][:, others], f"{tag}: snr_map at the other pixels")
    assert torch.isnan(got["snr_map"][:, fac["bad"]]).all() and torch.isnan(got["lnl_sky"]).all() and torch.isnan(got["lnl_sky_mix"]).all(), tag
    _report("pixel_nan", "the clean call", clean, ref, worst)
    _worst("pixel_nan", worst, 1)


# ---- 11: repeats -------------------------------------------------------------------------------------------------------------------------
def test_the_largest_case_gives_the_same_bits_twice():
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()

    def ws_bytes(fac):
        return int(lib.npf_waveform_loglike_sky_workspace_bytes(fac["rows"], fac["D"], fac["T"], fac["P"], fac["n_tau"]))

    n_big, tag, fac, case = max(((ws_bytes(f), t, f, c) for family in E.FAMILIES for t, f, c in E.cases(family)), key=lambda x: x[0])
    assert n_big > 0
    a, b = _call(E.call_args(case)), _call(E.call_args(case))
    for name in a:
        _same(a[name], b[name], f"{tag}: {name} of two calls")
    print(f"LOGLIKE_SKY_EDGES repeat {tag} (workspace {n_big} bytes): every output keeps its bits")
