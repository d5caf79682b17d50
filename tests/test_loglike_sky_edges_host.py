"""The inputs of the sky-grid likelihood's edge suite (tests/loglike_sky_edge_cases.py) on the CPU, against the float64 reference
alone: the constants the families rest on are the source's; every case whose indices are compared with the reference leaves them well
posed (``loglike_sky_reference.margins``: the best pixel's u leads by >= 1e3 gates, the best x_j by >= 1e-6 relative) except at the tie
its family plants, where the margin to the next distinct value is stated; every family reaches the pass, tile, workgroup, wave, stride
and chunk it names; six deliberately wrong evaluations fail their families; the scaled and the cut references agree with their
partners.  Nothing here launches a kernel."""
import math
import os
import re
import time

import pytest
import torch

import loglike_sky_edge_cases as E
import loglike_sky_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME = {}


def _refs(family):
    t0 = time.perf_counter()
    out = E.references(family)
    TIME.setdefault(family, time.perf_counter() - t0)
    return out


def test_the_constants_are_the_sources():
    from npf_gwwaveform_amd import functional as FN

    sky = open(os.path.join(ROOT, "npf_gwwaveform_amd", "csrc", "waveform_sky_kernels.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    assert int(re.search(r"constexpr int kSkyPrepThreads = (\d+);", sky).group(1)) == E.PASS
    assert int(re.search(r"constexpr int kSkyCorrWaves = (\d+);", sky).group(1)) == E.CORR_WAVES
    assert int(re.search(r"constexpr int kSkyFinishThreads = (\d+);", sky).group(1)) == E.FINISH
    assert re.search(r"constexpr int kSkyJC = NPF_SKY_JC;", sky)
    assert int(re.search(r"#define NPF_SKY_JC (\d+)\n", hdr).group(1)) == E.JC == FN.SKY_JC
    assert int(re.search(r"#define NPF_SKY_MAX_PIX (\d+)\n", hdr).group(1)) >= 513
    assert re.search(r"dim3\(64 \* kSkyCorrWaves\)", sky) and re.search(r"p \+= kSkyFinishThreads", sky)  # one wave per tile; the stride


def test_every_family_holds_the_cases_the_issue_lists():
    pp = [f for _, f, _ in E.cases("point_passes")]
    assert [(f["T"], f["D"]) for f in pp] == [(255, 1), (256, 2), (257, 3), (511, 1), (513, 2), (1025, 3), (129, 8)]
    assert all(c["n_valid"] is None for _, _, c in E.cases("point_passes"))
    assert [f["n_valid"] for _, f, _ in E.cases("counts")] == [(0, 255, 257, 305), (-3, 1, 256, 300)]
    assert all(f["T"] == 300 and f["Bn"] == 4 for _, f, _ in E.cases("counts"))
    wide = [f for _, f, _ in E.cases("wide_skies")]
    assert [(f["P"], f["p0"]) for f in wide] == [(63, 62), (64, 63), (65, 64), (80, 79), (129, 128), (257, 255), (257, 256), (513, 512)]
    assert all(f["n_z"] == 5 for f in wide if f["P"] == 257) and [f["jitter"] for f in wide].count(0.5) == 1
    dead = E.cases("dead_patterns")
    assert [f["pattern"] for _, f, _ in dead] == ["tile 1", "workgroup 1", "stride 0", "every other", "only pixel 0", "only pixel 255",
                                                   "only pixel 256", "only pixel 299"]
    assert all(f["P"] == 300 for _, f, _ in dead)
    long = [f for _, f, _ in E.cases("long_grids")]
    assert {f["n_tau"] for f in long} == {64, 1000, 4099} and all((f["Bn"], f["D"], f["P"]) == (2, 2, 5) for f in long)
    assert {(f["n_tau"], f["j0"]) for f in long} >= {(64, 0), (64, 7), (64, 8), (64, 63), (1000, 991), (1000, 992), (1000, 999), (4099, 0),
                                                       (4099, 4096), (4099, 4098)}
    assert [f["kind"] for f in long].count("-") == 1 and [f["kind"] for f in long].count("tau0=1") == 1
    for _, f, c in E.cases("long_grids"):
        d = c["freqs"][1:] - c["freqs"][:-1]
        assert float(d.max() - d.min()) > 5.0, "the frequencies are equally spaced"
        assert (c["taus"][1] < 0) == (f["kind"] == "-") and (c["taus"][0] == 1.0) == (f["kind"] == "tau0=1")
    tie = E.cases("ties")
    assert [(f["g1"], f["copies"]) for _, f, _ in tie if f["tied"] == "pixels"] == [(4, (5,)), (15, (16,)), (3, (35,)), (3, (67,)),
                                                                                      (10, (266,)), (5, (70, 261))]
    assert [f["P"] for _, f, _ in tie if f["tied"] == "sky"] == [130] and [f["P"] for _, f, _ in tie if f["tied"] == "zero"] == [513]
    assert [f["n_tau"] for _, f, _ in tie if f["tied"] == "shifts"] == [17, 100]
    for _, f, c in tie:
        if f["tied"] in ("pixels", "sky"):
            assert all(torch.equal(c["response"][g], c["response"][f["g1"]]) and torch.equal(c["delays"][g], c["delays"][f["g1"]])
                       for g in f["copies"])
            assert c["log_prior"] is None or all(c["log_prior"][g] == c["log_prior"][f["g1"]] for g in f["copies"])
        if f["tied"] in ("sky", "zero"):
            assert c["log_prior"] is None
        if f["tied"] == "shifts":
            assert float(c["freqs"].abs().max()) == 0
        if f["tied"] == "zero":
            assert float(c["h"][..., 0].abs().max()) == 0
    assert [(f["kind"], f["k"]) for _, f, _ in E.cases("scaled")] == [("wad", 40), ("wad", -40), ("ca", 60), ("ca", -60)] * 2
    assert [(f["T"], f["P"]) for _, f, _ in E.cases("scaled")] == [(257, 5)] * 4 + [(37, 129)] * 4
    assert [f["what"] for _, f, _ in E.cases("extremes")] == ["denormal", "phase", "delay"]
    (_, f, c), = E.cases("permutations")
    assert (f["rows"], f["P"]) == (9, 300) and sorted(f["perm"].tolist()) == list(range(300))
    assert all(torch.equal(c[k], f["base"][k][f["perm"]]) for k in ("response", "delays", "log_prior"))
    (_, f, c), = E.cases("pixel_nan")
    assert f["P"] == 65 and f["bad"] != f["p0"] and torch.isnan(c["response"][f["bad"]]).any() and torch.isfinite(c["log_prior"]).all()
    assert all(1 <= f["rows"] <= 9 for fam in E.FAMILIES for _, f, _ in E.cases(fam))


@pytest.mark.parametrize("family", E.FAMILIES)
def test_every_case_is_well_posed_but_for_the_ties_its_family_names(family):
    """``margins`` of the reference with the planted ties taken out (``loglike_sky_edge_cases.margins``); at a planted tie the tied
    values agree to 1e-12 and the figure printed is the margin to the next distinct value."""
    low_u, low_x = math.inf, math.inf
    for tag, fac, case, ref in _refs(family):
        lead_u, lead_x = E.margins(fac, ref)
        tied = fac["tied"]
        assert tied in (None, "pixels", "sky", "zero", "shifts"), tag
        gate = 1e-10 * ref["scale"] + 1e-12
        if tied in ("pixels", "sky"):
            for g in fac["copies"]:
                assert float(((ref["u"][:, g] - ref["u"][:, fac["g1"]]).abs() / gate).max()) <= 1e-2, f"{tag}: the copies do not tie"
        if tied == "zero":
            P = fac["P"]
            assert float((ref["u"] + math.log(P)).abs().max()) <= 1e-12 and float(ref["x"].abs().max()) == 0.0, tag
        if tied == "shifts":
            xp = ref["x"][torch.arange(fac["rows"]), ref["pix_index"]]
            assert float(((xp.max(1).values - xp.min(1).values) / xp.max(1).values).max()) <= 1e-12, f"{tag}: the shifts do not tie"
        for r in fac.get("tau_tied_rows", ()):  # one live point: |K_j| is the same at every j
            xr = ref["x"][r]
            assert float(((xr.max(1).values - xr.min(1).values) / xr.max(1).values.clamp(min=1e-300)).max()) <= 1e-12, tag
        for r in fac.get("empty_rows", ()):
            assert float(ref["x"][r].abs().max()) == 0.0 and float(ref["HH"][r].abs().max()) == 0.0, tag
        print(f"SKY EDGES {family} {tag}: lead of u {lead_u:.3g} gates, relative lead of x {lead_x:.3g}"
              + (f" (beyond the planted tie: {tied})" if tied else ""))
        assert lead_u >= 1e3 and lead_x >= 1e-6, f"{tag}: the inputs leave the indices ill posed ({lead_u:.3g}, {lead_x:.3g})"
        low_u, low_x = min(low_u, lead_u), min(low_x, lead_x)
        if family != "pixel_nan":
            keep = ("u", "lnl_sky", "lnl_sky_mix", "snr", "snr_map")
            assert all(not torch.isnan(ref[k]).any() for k in keep), tag
    print(f"SKY EDGES {family}: smallest lead of u {low_u:.3g} gates, smallest relative lead of x {low_x:.3g}; references in "
          f"{TIME[family]:.2f} s")


@pytest.mark.parametrize("family", ["wide_skies", "dead_patterns", "long_grids", "ties", "extremes", "permutations"])
def test_the_reference_finds_the_planted_pixel_and_grid_time(family):
    for tag, fac, case, ref in _refs(family):
        if fac["tied"] in ("zero", "sky"):
            continue
        p0 = fac["p0"]
        if family == "permutations":
            p0 = int((fac["perm"] == fac["base"]["p0"]).nonzero()[0, 0])
        pix = ref["pix_index"].clone()
        for g in fac.get("copies", ()):  # (a copy stands for the planted pixel: the reference's columns need not be bit-equal)
            pix[pix == g] = fac["g1"]
        assert (pix == p0).all(), f"{tag}: pix_index {ref['pix_index'].tolist()} against the planted {p0}"
        if fac["tied"] != "shifts":
            assert (ref["tau_index"] == fac["j0"]).all(), f"{tag}: tau_index {ref['tau_index'].tolist()} against the planted {fac['j0']}"


def test_every_family_reaches_the_path_it_names():
    tile_wg = 16 * E.CORR_WAVES
    # point_passes: a second, third and fifth pass, and one exactly full
    passes = [-(-f["T"] // E.PASS) for _, f, _ in E.cases("point_passes")]
    assert passes == [1, 1, 2, 2, 3, 5, 1] and E.cases("point_passes")[1][1]["T"] == E.PASS
    f8 = E.cases("point_passes")[-1][1]
    assert (f8["D"], -(-f8["T"] // 4)) == (8, 33)  # t4 wraps 8 times with tq = 33
    # counts: T = 300 has a second pass of 44; the live counts and their remainders mod 4
    (_, fa, ca), (_, fb, cb) = E.cases("counts")
    assert fa["live"] == [0, 255, 257, 300] and fb["live"] == [0, 1, 256, 300]
    assert [n % 4 for n in fa["live"]] == [0, 3, 1, 0] and [n % 4 for n in fb["live"]] == [0, 1, 0, 0]
    assert any(E.PASS < n < 300 for n in fa["live"]) and 300 - E.PASS == 44  # a count that ends inside the second pass
    for f, c in ((fa, ca), (fb, cb)):
        beyond = torch.arange(300).view(1, 1, 300) >= torch.tensor(f["live"]).view(4, 1, 1)
        assert torch.isnan(c["data"][beyond.expand(4, 3, 300)]).all() and torch.isnan(c["h"][beyond[:, 0]][:, :2]).all()
        assert max(f["n_valid"]) > 300 or min(f["n_valid"]) < 0  # what clamp_count clamps
    assert torch.isnan(ca["weights"]).any() and (cb["weights"] > 0).all()
    # wide_skies: the planted pixel's tile, workgroup, wave and stride
    want = {62: dict(tile=3, corr_wg=0, corr_wave=3, stride=0, wave=0), 63: dict(tile=3, corr_wg=0, corr_wave=3, stride=0, wave=0),
            64: dict(tile=4, corr_wg=1, corr_wave=0, stride=0, wave=1), 79: dict(tile=4, corr_wg=1, corr_wave=0, stride=0, wave=1),
            128: dict(tile=8, corr_wg=2, corr_wave=0, stride=0, wave=2), 255: dict(tile=15, corr_wg=3, corr_wave=3, stride=0, wave=3),
            256: dict(tile=16, corr_wg=4, corr_wave=0, stride=1, wave=0), 512: dict(tile=32, corr_wg=8, corr_wave=0, stride=2, wave=0)}
    for _, f, _ in E.cases("wide_skies"):
        assert E.where(f["p0"]) == want[f["p0"]], f
        tiles = -(-f["P"] // 16)
        assert (-(-tiles // E.CORR_WAVES) > 1) == (f["P"] > tile_wg)
    # a wavefront without a tile in a workgroup other than the first: P = 65, 80 (tiles 5 .. 7), 129 (9 .. 11), 257, 513
    assert all(-(-P // 16) % E.CORR_WAVES != 0 and P > tile_wg for P in (65, 80, 129, 257, 513))
    # dead_patterns
    for _, f, c in E.cases("dead_patterns"):
        dead, lp = f["dead"], c["log_prior"]
        assert torch.equal(~torch.isfinite(lp), dead) and not dead[f["p0"]] and f["cut"]["response"].shape[0] == int((~dead).sum())
        assert torch.isnan(c["response"][dead]).all() and torch.isnan(c["delays"][dead]).all()
        if int(dead.sum()) >= 3:
            assert (lp[dead] == -math.inf).any() and torch.isnan(lp[dead]).any() and (lp[dead] == math.inf).any()
        assert torch.equal(f["cut"]["log_prior"], lp[~dead])
    d = {f["pattern"]: f["dead"] for _, f, _ in E.cases("dead_patterns")}
    assert d["tile 1"].nonzero()[:, 0].tolist() == list(range(16, 32))
    assert d["workgroup 1"].nonzero()[:, 0].tolist() == list(range(tile_wg, 2 * tile_wg))
    assert d["stride 0"].nonzero()[:, 0].tolist() == list(range(E.FINISH)) and int(d["every other"].sum()) == 150
    assert [int((~d[f"only pixel {p}"]).nonzero()[0, 0]) for p in (0, 255, 256, 299)] == [0, E.FINISH - 1, E.FINISH, 299]
    # long_grids: the chunk of the maximiser, both ends of a chunk, the partial last chunks
    chunks = {(f["n_tau"], f["j0"]): (f["j0"] // E.JC, f["j0"] % E.JC) for _, f, _ in E.cases("long_grids")}
    assert chunks[(64, 7)] == (0, E.JC - 1) and chunks[(64, 8)] == (1, 0) and chunks[(64, 63)] == (7, 7)
    assert chunks[(1000, 991)] == (123, 7) and chunks[(1000, 992)] == (124, 0) and chunks[(1000, 999)] == (124, 7)
    assert chunks[(4099, 4096)] == (512, 0) and chunks[(4099, 4098)] == (512, 2) and 4099 - 512 * E.JC == 3 and 1000 % E.JC == 0
    assert {-(-n // E.JC) for n in (64, 1000, 4099)} == {8, 125, 513}
    # ties: where the tied pixels sit
    at = {(f["g1"],) + f["copies"]: [E.where(p) for p in (f["g1"],) + f["copies"]] for _, f, _ in E.cases("ties") if f["tied"] == "pixels"}
    a, b = at[(4, 5)]
    assert a == b
    a, b = at[(15, 16)]
    assert (a["tile"], b["tile"], a["corr_wg"], b["corr_wg"], a["wave"], b["wave"]) == (0, 1, 0, 0, 0, 0)
    a, b = at[(3, 35)]
    assert (a["tile"], b["tile"], a["corr_wg"], b["corr_wg"], a["wave"], b["wave"]) == (0, 2, 0, 0, 0, 0)
    a, b = at[(3, 67)]
    assert (a["corr_wg"], b["corr_wg"], a["wave"], b["wave"], b["stride"]) == (0, 1, 0, 1, 0)
    a, b = at[(10, 266)]
    assert (a["stride"], b["stride"], a["wave"], b["wave"]) == (0, 1, 0, 0) and 266 - E.FINISH == 10  # the same thread, two strides
    a, b, c = at[(5, 70, 261)]
    assert (a["wave"], b["wave"], c["wave"], a["stride"], b["stride"], c["stride"]) == (0, 1, 0, 0, 0, 1)
    assert [(-(-f["n_tau"] // E.JC)) for _, f, _ in E.cases("ties") if f["tied"] == "shifts"] == [3, 13]
    # permutations: pixels cross workgroups and strides
    (_, f, _), = E.cases("permutations")
    q = torch.arange(300)
    assert int(((q // tile_wg) != (f["perm"] // tile_wg)).sum()) > 200 and int(((q // E.FINISH) != (f["perm"] // E.FINISH)).sum()) > 50
    (_, f, _), = E.cases("pixel_nan")
    assert E.where(f["bad"]) == dict(tile=4, corr_wg=1, corr_wave=0, stride=0, wave=1)
    # extremes
    den, ph, dl = [c for _, _, c in E.cases("extremes")]
    assert float(den["h"][..., 0].max()) < 2.0 ** -126 and float(den["h"][..., 0].min()) > 0
    assert ((ph["h"][:, :, 1].double().mean(1) - torch.tensor([1e4, -1e4, 1e6, -1e6], dtype=torch.float64)).abs() < 5.0).all()
    assert float(dl["delays"].abs().max()) <= 0.5 and float(dl["delays"].abs().max()) > 0.3 and 0.5 * 512 == 256


# ---- wrong evaluations ---------------------------------------------------------------------------------------------------------------
def _worst(r):
    return max(r.values())


def test_wrong_a_points_beyond_the_first_pass_dropped():
    """hh_k and K without the points >= 256: the reference with every count at 256."""
    worst = 0.0
    for tag, fac, case, ref in _refs("point_passes"):
        if fac["T"] <= E.PASS:
            continue
        bad = S.reference(**dict(E.call_args(case), n_valid=torch.full((fac["Bn"],), E.PASS, dtype=torch.int32)))
        r = _worst(S.ratios({k: bad[k] for k in S.DOUBLES}, ref))
        print(f"SKY EDGES wrong (a) points >= {E.PASS} dropped, {tag}: worst error / gate {r:.3g}")
        assert r > 1.0, tag
        worst = max(worst, r)
    print(f"SKY EDGES wrong (a): misses by {worst:.3g}")


def test_wrong_b_pixels_beyond_the_first_stride_dropped():
    """The pixel sum without the pixels >= 256."""
    worst = 0.0
    for tag, fac, case, ref in _refs("wide_skies"):
        if fac["P"] <= E.FINISH:
            continue
        lnl = torch.logsumexp(ref["u"][:, :E.FINISH], 1)
        r = _worst(S.ratios(dict(lnl_sky=lnl, post=ref["u"] - lnl.view(-1, 1)), ref))
        print(f"SKY EDGES wrong (b) pixels >= {E.FINISH} dropped, {tag}: worst error / gate {r:.3g}")
        worst = max(worst, r)
    assert worst > 1.0
    print(f"SKY EDGES wrong (b): misses by {worst:.3g}")


def test_wrong_c_the_largest_index_on_a_pixel_tie():
    n = 0
    for tag, fac, case, ref in _refs("ties"):
        if fac["tied"] not in ("pixels", "sky"):
            continue
        u = ref["u"].clone()
        u[:, list(fac["copies"])] = u[:, [fac["g1"]]]  # the tie made exact, as it is on the GPU
        P = u.shape[1]
        last = P - 1 - (u.flip(1) == u.max(1, keepdim=True).values).double().argmax(1)
        assert (last == max(fac["copies"])).all() and (last != fac["g1"]).all(), tag
        n += 1
    print(f"SKY EDGES wrong (c) the largest index on a pixel tie: pix_index differs in all {n} cases")
    assert n == 7


def test_wrong_d_the_arg_max_within_the_last_chunk_only():
    miss = []
    for tag, fac, case, ref in _refs("long_grids"):
        xp = ref["x"][torch.arange(fac["rows"]), ref["pix_index"]]
        j_last = E.JC * ((fac["n_tau"] - 1) // E.JC)
        tau = j_last + xp[:, j_last:].argmax(1)
        if not torch.equal(tau, ref["tau_index"]):
            miss.append(tag)
    print(f"SKY EDGES wrong (d) best_j reset per chunk: tau_index differs in {len(miss)} of {len(E.cases('long_grids'))} cases: {miss}")
    assert len(miss) >= 6  # every case whose maximiser sits before the last chunk


def test_wrong_e_the_last_index_on_a_shift_tie():
    n = 0
    for tag, fac, case, ref in _refs("ties"):
        if fac["tied"] != "shifts":
            continue
        xp = ref["x"][torch.arange(fac["rows"]), ref["pix_index"]]
        tied = xp >= xp.max(1, keepdim=True).values * (1.0 - 1e-12)
        last = fac["n_tau"] - 1 - tied.flip(1).double().argmax(1)
        assert (last == fac["n_tau"] - 1).all(), tag  # against the expected 0
        n += 1
    print(f"SKY EDGES wrong (e) the last index on a shift tie: tau_index n_tau - 1 against 0 in {n} cases")
    assert n == 2


def test_wrong_f_a_dead_pixel_given_its_finite_neighbours_mass():
    worst = 0.0
    for tag, fac, case, ref in _refs("dead_patterns"):
        dead = fac["dead"]
        u = ref["u"].clone()
        u[:, dead] = u[:, ~dead].mean(1, keepdim=True)
        lnl = torch.logsumexp(u, 1)
        r = S.ratios(dict(lnl_sky=lnl, post=u - lnl.view(-1, 1)), ref)
        print(f"SKY EDGES wrong (f) dead pixels with mass, {tag}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert r["post"] == math.inf, tag  # -inf is met by -inf only
        worst = max(worst, r["lnl_sky"])
    print(f"SKY EDGES wrong (f): post misses by inf in every pattern, lnl_sky by up to {worst:.3g}")


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())


def test_the_scaled_references_are_the_unscaled_ones():
    worst = 0.0
    base_refs = {}
    for tag, fac, case, ref in _refs("scaled"):
        key = id(fac["base"])
        if key not in base_refs:
            base_refs[key] = S.reference(**E.call_args(fac["base"]))
        base = base_refs[key]
        for name in ("u", "lnl_sky", "lnl_sky_mix", "snr", "snr_map", "x", "HH"):
            d = _rel(ref[name], base[name])
            worst = max(worst, d)
            assert d <= 1e-12, (tag, name, d)
        assert torch.equal(ref["pix_index"], base["pix_index"]) and torch.equal(ref["tau_index"], base["tau_index"]), tag
    print(f"SKY EDGES scaled against unscaled in the reference: worst relative difference {worst:.3g}")


def test_the_dead_references_are_the_cut_ones_at_the_live_columns():
    worst = 0.0
    for tag, fac, case, ref in _refs("dead_patterns"):
        live = ~fac["dead"]
        cut = S.reference(**fac["cut"])
        assert torch.equal(ref["live"], live), tag
        for name in ("u", "post", "post_mix", "snr_map"):
            d = _rel(ref[name][:, live], cut[name])
            worst = max(worst, d)
            assert d <= 1e-12, (tag, name, d)
        for name in ("lnl_sky", "lnl_sky_mix", "snr"):
            d = _rel(ref[name], cut[name])
            worst = max(worst, d)
            assert d <= 1e-12, (tag, name, d)
        assert torch.equal(live.nonzero()[:, 0][cut["pix_index"]], ref["pix_index"]) and torch.equal(cut["tau_index"], ref["tau_index"]), tag
        assert (ref["post"][:, ~live] == -math.inf).all() and (ref["snr_map"][:, ~live] == 0).all(), tag
    print(f"SKY EDGES dead against cut in the reference: worst relative difference {worst:.3g}")


def test_the_empty_task_keeps_the_prior_in_the_reference():
    for tag, fac, case, ref in _refs("counts"):
        for r in fac["empty_rows"]:
            lp = case["log_prior"]
            assert float((ref["u"][r] - lp).abs().max()) <= 1e-12 and ref["pix_index"][r] == int(lp.argmax()), tag
            assert ref["tau_index"][r] == 0 and ref["snr"][r] == 0 and (ref["snr_map"][r] == 0).all(), tag
