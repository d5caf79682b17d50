"""The inputs of the bank match's edge suite (tests/match_bank_edge_cases.py) on the CPU, against the float64 reference alone: every
case leaves ``tau_index`` and ``best_index`` well posed (runner-up margins >= 1e-6, normalised) except the pairs its family ties by
construction, the planted templates and shifts are the reference's, a removed pattern has the live and per-wave counts its name says
and the reference of the removed inputs is the reference of the cut ones, the reference's largest intermediate stays below 128 MiB,
and the extreme amplitudes leave no pair degenerate.  Nothing here launches a kernel."""
import math

import pytest
import torch

import match_bank_edge_cases as E
import match_bank_reference as RB

# pattern -> (live points, live points per wave of 64 threads over the three passes of 256; None: only the sum is stated)
FULL = [64] * 9 + [24]
REMOVED_EXPECT = {
    "wave 0": (536, [0] + FULL[1:]), "pass 0": (344, [0] * 4 + FULL[4:]), "middle pass": (344, FULL[:4] + [0] * 4 + FULL[8:]),
    "last pass": (512, FULL[:8] + [0, 0]), "every other": (300, [32] * 9 + [12]),
    "unequal waves": (297, [61, 54, 47, 40, 33, 26, 19, 12, 5, 0]),
    "live = 0 mod 4": (None, None), "live = 1 mod 4": (None, None), "live = 2 mod 4": (None, None), "live = 3 mod 4": (None, None),
    "only point 255": (1, [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]), "only point 256": (1, [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]),
    "only point 599": (1, [0] * 9 + [1]),
}


def test_every_family_holds_the_cases_the_issue_lists():
    assert [f["pts"] for _, f, _ in E.cases("point_passes")] == [255, 256, 257, 511, 512, 513, 1025]
    assert all((f["n_rows"], f["n_bank"], f["n_tau"]) == (3, 3, 5) and c["weights"] is not None for _, f, c in E.cases("point_passes"))
    rem = E.cases("removed_patterns")
    assert [f["pattern"] for _, f, _ in rem] == list(REMOVED_EXPECT) and {f["h_ld"] for _, f, _ in rem} == {3, 4}
    assert all(c["h"].shape == (17, 600, f["h_ld"]) and c["bank"].shape == (18, 600, 2) for _, f, c in rem)
    wide = E.cases("wide_banks")
    assert [f["n_bank"] for _, f, _ in wide] == [63, 64, 65, 80, 129, 130]
    for _, f, c in wide:
        G = f["n_bank"]
        assert f["pick"] == [0, 15, 16, min(63, G - 1), min(64, G - 1), G - 1, G - 2] and f["j_star"] == [1, 4, 2, 0, 3, 1, 4]
        assert c["h"].shape[:2] == (7, 37) and c["taus"][2] == 5
    long = E.cases("long_grids")
    assert [(f["n_tau"], f["dtau"]) for _, f, _ in long] == [(33, E.DTAU), (1000, E.DTAU), (4099, E.DTAU), (33, -E.DTAU)]
    assert long[0][1]["j_star"] == [0, 15, 16, 31, 32, 32, 32] and long[1][1]["j_star"] == [0, 15, 16, 991, 992, 999, 992]
    assert long[2][1]["j_star"] == [0, 15, 16, 991, 992, 4098, 4096] and long[3][2]["taus"] == (2 * E.DTAU, -E.DTAU, 33)
    # the chunks of 16 shifts the maximisers sit in, and both ends of a chunk
    assert {j // 16 for _, f, _ in long for j in f["j_star"]} >= {0, 1, 2, 61, 62, 256}
    for _, f, c in long:
        d = c["freqs"][1:] - c["freqs"][:-1]
        assert float(d.max() - d.min()) > 5.0, "the frequencies are equally spaced"
        tau = [c["taus"][0] + j * c["taus"][1] for j in (0, f["n_tau"] - 1)]
        assert max(abs(t) for t in tau) <= 2.01
    tie = E.cases("ties")
    assert [(f["g1"], f["copies"]) for _, f, _ in tie if f["tied"] == "columns"] == list(E.DUPLICATES)
    assert {(3, (4,)), (63, (64,)), (3, (67,)), (3, (67, 129)), (5, (21,)), (10, (70,)), (0, (129,))} <= set(E.DUPLICATES)
    assert all(f["n_bank"] == 130 for _, f, _ in tie if f["tied"] in ("columns", "bank"))
    assert [f["n_tau"] for _, f, _ in tie if f["tied"] == "shifts"] == [17, 33]
    assert all(float(c["freqs"].abs().max()) == 0 for _, f, c in tie if f["tied"] == "shifts")
    for _, f, c in tie:
        if f["tied"] in ("columns", "bank"):
            assert all(torch.equal(c["bank"][g], c["bank"][f["g1"]]) for g in f["copies"])
    assert [(f["a"], f["b"], f["c"]) for _, f, _ in E.cases("scaled")] == [(40, -60, 0), (-40, 40, 20), (0, 0, -20)]
    ext = E.cases("extremes")
    assert [f["w_power"] for _, f, _ in ext] == [-140, -100, 100, 120, 0]
    for _, f, c in ext[:4]:
        la, lb = c["h"][..., 0].log2().mean(1), c["bank"][..., 0].log2().mean(1)
        assert la.min() < -135 and la.max() > 115 and lb.min() < -135 and lb.max() > 115
        assert (c["h"][..., 0] < 2.0 ** -126).any() and (c["weights"] < 2.0 ** -126).all() == (f["w_power"] == -140)  # denormals
    assert float(ext[4][2]["h"][5, :, 1].abs().max()) > 9e5 and float(ext[4][2]["bank"][7, :, 1].abs().max()) > 9e3
    perm = E.cases("permutations")
    assert [(f["n_rows"], f["n_bank"], f["pts"], f["n_tau"], f["axis"]) for _, f, _ in perm] == \
        [(7, 129, 37, 5, "bank"), (7, 129, 37, 5, "rows"), (33, 40, 129, 17, "bank"), (33, 40, 129, 17, "rows")]


def test_the_default_build_of_the_reference_module_is_unchanged_by_pick_and_j_star():
    a = RB.build(7, 9, 37, 5, seed=3, h_ld=4)
    r = torch.arange(7)
    b = RB.build(7, 9, 37, 5, seed=3, h_ld=4, pick=((5 * r + 2) % 9).tolist(), j_star=((3 * r + 1) % 5).tolist())
    for k in ("h", "bank", "weights", "freqs"):
        assert torch.equal(a[k], b[k]), k
    assert a["taus"] == b["taus"]


@pytest.mark.parametrize("family", E.FAMILIES)
def test_every_case_is_well_posed_but_for_the_ties_its_family_names(family):
    worst_j, worst_g = math.inf, math.inf
    for tag, fac, case, ref in E.references(family):
        assert E.reference_bytes(fac, case) <= E.REFERENCE_BYTES, f"{tag}: the reference would take {E.reference_bytes(fac, case)} bytes"
        assert not ref["degenerate"].any() and torch.isfinite(ref["match"]).all() and torch.isfinite(ref["dot"]).all(), tag
        assert torch.isfinite(ref["phase"]).all() and (ref["match"] <= 1.0 + 1e-12).all(), tag
        tied = fac["tied"]
        assert tied in (None, "columns", "bank", "shifts", "all"), tag
        if tied == "all":  # one live point: every template matches perfectly at every shift
            assert float((ref["match"] - 1.0).abs().max()) <= 1e-12, tag
            continue
        over_j, over_g = E.margins(ref, skip_columns=fac.get("copies", ()))
        if tied == "shifts":
            top = ref["mag"].topk(2, dim=2).values
            assert float((top[..., 0] - top[..., 1]).max()) <= 1e-12, f"{tag}: the shifts do not tie"
            over_j = math.inf
        if tied == "bank":
            assert float((ref["match"] - ref["match"][:, :1]).abs().max()) <= 1e-12, tag
        if tied == "columns":
            for g in fac["copies"]:
                assert float((ref["match"][:, g] - ref["match"][:, fac["g1"]]).abs().max()) <= 1e-12, tag
        print(f"BANK EDGES {family} {tag}: runner-up margin over shifts {over_j:.3g}, over templates {over_g:.3g}")
        assert over_j >= 1e-6, f"{tag}: the runner-up of max_j |c_j| lies {over_j:.3g} below the best"
        assert over_g >= 1e-6, f"{tag}: the runner-up template lies {over_g:.3g} below best_match"
        worst_j, worst_g = min(worst_j, over_j), min(worst_g, over_g)
    print(f"BANK EDGES {family}: smallest runner-up margin over shifts {worst_j:.3g}, over templates {worst_g:.3g}")
    if family == "point_passes":  # (fixed seeds: the margins measured when the cases were chosen)
        assert worst_j >= 3.8e-3 and worst_g >= 0.09


@pytest.mark.parametrize("family", ["wide_banks", "long_grids", "ties"])
def test_the_reference_finds_the_planted_templates_and_shifts(family):
    for tag, fac, case, ref in E.references(family):
        if "pick" not in fac:
            continue  # (zero frequencies: nothing is planted beyond the feature builder's own rows)
        pick, j_star = torch.tensor(fac["pick"]), torch.tensor(fac["j_star"])
        best = ref["best_index"].clone()
        for g in fac.get("copies", ()):  # a copy of column g1 stands for g1: the reference's columns need not be bit-equal
            best[best == g] = fac["g1"]
        assert torch.equal(best, pick), f"{tag}: best_index {ref['best_index'].tolist()} against the planted {pick.tolist()}"
        assert torch.equal(ref["tau_index"][torch.arange(len(pick)), pick], j_star), \
            f"{tag}: tau_index {ref['tau_index'][torch.arange(len(pick)), pick].tolist()} against the planted {j_star.tolist()}"


def test_removed_patterns_have_the_stated_counts_and_the_reference_of_the_cut_call():
    worst = 0.0
    for tag, fac, case, ref in E.references("removed_patterns"):
        kill = fac["kill"]
        w = case["weights"]
        live = (w > 0) & torch.isfinite(w)
        assert torch.equal(live, ~kill), tag
        dead = w[kill]  # the four kinds of a dead weight all occur
        assert (dead == 0).any() and (dead == -1).any() and torch.isnan(dead).any() and (dead == math.inf).any(), tag
        assert torch.isnan(case["h"][:, kill]).all() and torch.isnan(case["bank"][:, kill]).all() and torch.isnan(case["freqs"][kill]).all()
        assert torch.isfinite(case["h"][:, ~kill]).all() and torch.isfinite(case["bank"][:, ~kill]).all(), tag
        n_live = int(live.sum())
        per_wave = [int(live[64 * k:64 * (k + 1)].sum()) for k in range(10)]
        want_live, want_waves = REMOVED_EXPECT[fac["pattern"]]
        if want_live is None:
            assert n_live % 4 == int(fac["pattern"].split()[2]) and 300 < n_live < 500, (tag, n_live)
        else:
            assert n_live == want_live and per_wave == want_waves, (tag, n_live, per_wave)
        if fac["pattern"] == "unequal waves":
            assert len(set(per_wave)) == 10
        assert fac["cut"]["h"].shape == (17, n_live, fac["h_ld"]) and fac["cut"]["bank"].shape == (18, n_live, 2), tag
        # the reference masks; the cut inputs are the same sums without the zeros
        masked = RB.reference(**E.call_args(case))
        for name in ("match", "mismatch", "hh", "gg", "dot"):
            scale = 1.0 if name in ("match", "mismatch") else float(ref[name].abs().max())
            d = float((masked[name] - ref[name]).abs().max()) / scale
            worst = max(worst, d)
            assert d <= 1e-12, (tag, name, d)
        if fac["tied"] is None:
            assert torch.equal(masked["tau_index"], ref["tau_index"]) and torch.equal(masked["best_index"], ref["best_index"]), tag
    print(f"BANK EDGES removed against cut in the reference: worst difference {worst:.3g}")


def test_the_extremes_stay_inside_double_and_leave_fp32_at_both_ends():
    m2_min, prod_max, hh32 = math.inf, 0.0, []
    for tag, fac, case, ref in E.references("extremes"):
        assert not ref["degenerate"].any(), tag
        assert all(torch.isfinite(ref[k]).all() for k in ("match", "mismatch", "phase", "dot", "hh", "gg")), tag
        m2 = ref["dot"].pow(2).sum(-1)
        assert (m2 > 0).all(), f"{tag}: |c|^2 underflows in double"
        m2_min = min(m2_min, float(m2.min()))
        prod_max = max(prod_max, float((ref["hh"].view(-1, 1) * ref["gg"].view(1, -1)).max()))
        hh32 += [ref["hh"].float(), ref["gg"].float()]
    hh32 = torch.cat(hh32)
    print(f"BANK EDGES extremes: smallest |c|^2 {m2_min:.3g}, largest hh gg {prod_max:.3g}; of {hh32.numel()} hh / gg values in fp32 "
          f"{int(torch.isinf(hh32).sum())} are inf, {int((hh32 == 0).sum())} zero, {int(((hh32 > 0) & (hh32 < 2.0 ** -126)).sum())} denormal")
    assert m2_min > 1e-300 and prod_max < 1e300
    assert torch.isinf(hh32).any() and (hh32 < 2.0 ** -126).any()


def test_scalings_and_permutations_are_exact_in_the_inputs():
    for tag, fac, case in E.cases("scaled"):
        base = fac["base"]
        for key, p in (("h", fac["a"]), ("bank", fac["b"])):
            assert torch.equal(case[key][..., 0].double(), base[key][..., 0].double() * 2.0 ** p), (tag, key)  # no bit lost
            assert torch.equal(case[key][..., 1], base[key][..., 1])
        assert torch.equal(case["weights"].double(), base["weights"].double() * 2.0 ** fac["c"]), tag
        ref = RB.reference(**E.call_args(base))
        for name, p in (("hh", 2 * fac["a"] + fac["c"]), ("gg", 2 * fac["b"] + fac["c"])):
            x = ref[name] * 2.0 ** p
            assert (x > 2.0 ** -120).all() and (x < 2.0 ** 120).all(), f"{tag}: scaled {name} leaves the normal fp32 range"
    for tag, fac, case in E.cases("permutations"):
        key = "bank" if fac["axis"] == "bank" else "h"
        assert torch.equal(case[key], fac["base"][key][fac["perm"]]) and sorted(fac["perm"].tolist()) == list(range(len(fac["perm"])))
        over_j, over_g = E.margins(RB.reference(**E.call_args(fac["base"])))
        assert over_j >= 1e-6 and over_g >= 1e-6, tag
