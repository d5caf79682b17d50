"""Input builders of the bank match's edge suite: ``npf_waveform_match_bank`` (csrc/waveform_bank_kernels.hip) at the pass, wave,
workgroup, grid, tie and scale edges that the feature suite (tests/match_bank_reference.py: rows <= 33, templates <= 40, points <= 200,
shifts <= 33) never reaches.  Everything is built with ``match_bank_reference.build`` and checked against its ``reference`` under its
``ratios``; tests/test_match_bank_edges_host.py checks on the CPU that every case is well posed.

``cases(family)`` -> list of (tag, factors, case); ``references(family)`` adds the float64 reference, computed once and shared.
Which path of the kernels each family reaches:

``point_passes``     pts in {255, 256, 257, 511, 512, 513, 1025}, all live: one pass of the preparation launch's 256 threads exactly
                     full, a SECOND pass of one point (257) up to a full one (512), a THIRD (513) and a fifth (1025); ``n_live`` is
                     carried over a pass and ``wave_cnt`` rewritten behind the barrier.
``removed_patterns`` pts = 600 (passes of 256, 256, 88) with removed points in patterns: wave 0, pass 0 (``n_live`` enters pass 1 at
                     0), the middle pass, the last pass, every other point, UNEQUAL WAVE COUNTS (61, 54, ..., 5, 0 live lanes in
                     waves 0 .. 9, so the cross-wave prefix ``wave_cnt[w]`` differs from 64 w and p != t), live counts of 0, 1, 2
                     and 3 mod 4 (the zero padding of the last k-step), and one live point at 255, 256 (the last thread of pass 0,
                     the first of pass 1) and 599.  Removed against cut, bit for bit.
``wide_banks``       n_bank in {63, 64, 65, 80, 129, 130}: ``blockIdx.y > 0`` in the correlation launch with ONE live wave (65, 80:
                     tile 4; 129, 130: tile 8) and with FOUR (129, 130: tiles 4 .. 7), the early return of a wavefront without a tile
                     in workgroups 1 and 2, and TWO (65 .. 80) and THREE (129, 130) strides of the best-template loop with winners in
                     tile 0, 1, 3, 4, 8 and at lanes 0, 15, 16, 63 and 0 / 1 of the later strides.
``long_grids``       n_tau in {33, 1000, 4099} on an unequally spaced frequency grid: the maximiser at shift 0, 15 and 16 (a chunk's
                     last index, CHUNK 1's first), 31 / 32 (CHUNK 2, partial, one shift), 991 and 992 (last of CHUNK 61, first of
                     CHUNK 62; 992 is also the first index of the partial last chunk of n_tau = 1000), n_tau - 1 and 4096 (CHUNK 256,
                     partial); and one grid that runs backwards (dtau < 0).
``ties``             BOTH TIE RULES, the expected indices by construction: duplicate templates (``best_index`` is the smallest
                     template index: neighbouring lanes, a tile edge, one lane in two and three strides, two tiles of a workgroup,
                     two workgroups, 130 identical templates) and zero frequencies (``tau_index`` is the first shift index, with
                     the register-held maximum carried over two and three chunks).
``scaled``           exact power-of-two scalings of amplitudes and weights: invariant bits.
``extremes``         amplitudes and weights times 2^-140 (fp32 denormals), 2^-100, 2^100, 2^120; phases of +-1e6 and +-1e4 rad.
``permutations``     templates and rows permuted: every output element moves with its row / template, bit for bit.

The gates are those of ``match_bank_reference.ratios``, unchanged: match, mismatch, best_match |d| <= 1e-9 + 2^-23 |ref|; hh, gg
2^-23 relative; phase 1e-6 where the match is >= 1e-3; dot 1e-9 sqrt(hh gg); tau_index, best_index exact.  Their derivation (double
sums whose error grows as about 4 T 2^-53 on the normalised quantities, see ``waveform_edge_cases.near_ratios``) gives 4.6e-13 at the
longest row here, T = 1025: still more than three orders of magnitude below the absolute 1e-9, so no gate moves.

A case whose first seed leaves an index ill posed (a runner-up within 1e-6, normalised) gets another seed through ``SEED_SHIFT``."""
import math

import torch

import match_bank_reference as RB

TWO_PI = RB.TWO_PI
DTAU = RB.DTAU
JC = 16
PASS = 256  # threads of the preparation launch (kBankPrepThreads)
FAMILIES = ("point_passes", "removed_patterns", "wide_banks", "long_grids", "ties", "scaled", "extremes", "permutations")
PASS_POINTS = (255, 256, 257, 511, 512, 513, 1025)
REMOVED_PTS = 600
WIDE_BANKS = (63, 64, 65, 80, 129, 130)
WIDE_SHIFTS = (1, 4, 2, 0, 3, 1, 4)
LONG_GRIDS = (33, 1000, 4099)
LONG_PICK = (2, 0, 4, 1, 3, 2, 0)
DUPLICATES = ((3, (4,)), (63, (64,)), (3, (67,)), (3, (67, 129)), (1, (65, 129)), (5, (21,)), (10, (70,)), (0, (129,)))
TIE_BANK = 130
SCALINGS = (("point_passes", "pts", 257, 40, -60, 0), ("wide_banks", "n_bank", 129, -40, 40, 20), ("point_passes", "pts", 1025, 0, 0, -20))
EXTREME_POWERS = (-140, -100, 100, 120)
REFERENCE_BYTES = 128 * 2 ** 20
# (family, case number) -> what is added to the case's seed, with the reason
SEED_SHIFT = {}


def _seed(family, number, base):
    return base + SEED_SHIFT.get((family, number), 0)


def _clone(case):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


call_args = RB.call_args


# ---- 1: passes of the preparation launch ---------------------------------------------------------------------------------------------
def point_passes():
    out = []
    for pts in PASS_POINTS:
        fac = dict(n_rows=3, n_bank=3, pts=pts, n_tau=5, tied=None)
        out.append((f"pts={pts}", fac, RB.build(3, 3, pts, 5, seed=pts)))
    return out


# ---- 2: removed points in patterns -------------------------------------------------------------------------------------------------
def _removed_masks():
    """name -> bool [600], True where the point is removed."""
    t = torch.arange(REMOVED_PTS)
    g = torch.Generator().manual_seed(600)
    third = torch.rand(REMOVED_PTS, generator=g) < 1.0 / 3.0
    out = {"wave 0": t < 64, "pass 0": t < PASS, "middle pass": (t >= PASS) & (t < 2 * PASS), "last pass": t >= 2 * PASS,
           "every other": t % 2 == 0, "unequal waves": (t % 64) < 7 * (t // 64) + 3}
    for m in range(4):  # a random third, then further live points from the front until the live count is m mod 4
        kill = third.clone()
        first_live = (~kill).nonzero()[:, 0]
        extra = (int((~kill).sum()) - m) % 4
        kill[first_live[:extra]] = True
        out[f"live = {m} mod 4"] = kill
    for only in (PASS - 1, PASS, REMOVED_PTS - 1):
        out[f"only point {only}"] = t != only
    return out


def removed_patterns():
    """The factors hold ``kill`` and ``cut``: the call arguments with the removed points cut out.  The three patterns with one live
    point come without a grid (one point matches every template perfectly at every shift) and are named by ``tied="all"``."""
    out = []
    kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])
    for i, (name, kill) in enumerate(_removed_masks().items()):
        h_ld = (3, 4)[i % 2]
        base = RB.build(17, 18, REMOVED_PTS, 17, seed=_seed("removed_patterns", i, 9100 + i), h_ld=h_ld)
        one = int((~kill).sum()) == 1
        taus = None if one else base["taus"]
        cut = dict(h=base["h"][:, ~kill].clone(), bank=base["bank"][:, ~kill].clone(), weights=base["weights"][~kill].clone(),
                   freqs=None if one else base["freqs"][~kill].clone(), taus=taus)
        case = _clone(base)
        case["taus"] = taus
        case["weights"][kill] = kinds[torch.arange(int(kill.sum())) % 4]  # the dead weights cycle through the four kinds
        case["h"][:, kill] = math.nan
        case["bank"][:, kill] = math.nan
        case["freqs"][kill] = math.nan
        fac = dict(n_rows=17, n_bank=18, pts=REMOVED_PTS, n_tau=0 if one else 17, h_ld=h_ld, pattern=name, kill=kill, cut=cut,
                   tied="all" if one else None)
        out.append((f"{name} h_ld={h_ld}", fac, case))
    return out


# ---- 3: banks of several workgroups and strides --------------------------------------------------------------------------------------
def wide_pick(G):
    return [0, 15, 16, min(63, G - 1), min(64, G - 1), G - 1, G - 2]


def wide_banks():
    out = []
    for i, G in enumerate(WIDE_BANKS):
        pick = wide_pick(G)
        fac = dict(n_rows=7, n_bank=G, pts=37, n_tau=5, pick=pick, j_star=list(WIDE_SHIFTS), tied=None)
        case = RB.build(7, G, 37, 5, seed=_seed("wide_banks", i, 9300 + i), h_ld=(2, 4)[i % 2], pick=pick, j_star=WIDE_SHIFTS)
        out.append((f"n_bank={G}", fac, case))
    return out


# ---- 4: long grids -----------------------------------------------------------------------------------------------------------------
def long_shifts(n_tau):
    late = (991, 992) if n_tau > 992 else (31, 32)
    return [0, 15, 16, late[0], late[1], n_tau - 1, JC * ((n_tau - 1) // JC)]


def uneven_freqs(pts):
    """20 + 492 x^1.5 + 3 sin(17 x) Hz: the equally spaced grid of ``match_bank_reference.build`` (492 / 36 Hz apart) makes |c(tau)|
    repeat every 73 ms, so a grid of 0.5 s or 2 s holds copies of the maximum and the planted shift is not the reference's."""
    x = torch.linspace(0.0, 1.0, pts, dtype=torch.float64)
    return (20.0 + 492.0 * x.pow(1.5) + 3.0 * torch.sin(17.0 * x)).float()


def long_grids():
    """Rows planted with ``build`` on its own templates without a shift, then shifted on the uneven grid: phi <- phi - 2 pi f tau_j*.
    |tau| stays below 2.01 s: the 1e-9 gate does not cover the rounding of the argument 2 pi f tau at hundreds of seconds."""
    out = []
    for i, (n_tau, back) in enumerate([(n, False) for n in LONG_GRIDS] + [(33, True)]):
        taus = (2 * DTAU, -DTAU, n_tau) if back else (-2 * DTAU, DTAU, n_tau)
        j_star = long_shifts(n_tau)
        case = RB.build(7, 5, 37, 0, seed=_seed("long_grids", i, 9400 + i), h_ld=(2, 4)[i % 2], pick=LONG_PICK)
        f = uneven_freqs(37)
        tau = taus[0] + torch.tensor(j_star, dtype=torch.float64) * taus[1]
        case["h"][..., 1] = (case["h"][..., 1].double() - TWO_PI * f.double().view(1, 37) * tau.view(7, 1)).float()
        case["freqs"], case["taus"] = f, taus
        fac = dict(n_rows=7, n_bank=5, pts=37, n_tau=n_tau, pick=list(LONG_PICK), j_star=j_star, dtau=taus[1], tied=None)
        out.append((f"n_tau={n_tau} dtau={'-' if back else '+'}", fac, case))
    return out


# ---- 5: ties -----------------------------------------------------------------------------------------------------------------------
def ties():
    """``tied``: "columns" (the factors hold ``g1`` and ``copies``: columns equal to column g1 bit for bit; rows 0 and 2 are planted
    on g1), "bank" (every template is template 0) or "shifts" (zero frequencies: every shift gives the same sum)."""
    out = []
    for g1, copies in DUPLICATES:
        i = len(out)
        pick = [g1, (g1 + 40) % TIE_BANK, g1]
        assert pick[1] not in copies and pick[1] != g1
        case = RB.build(3, TIE_BANK, 37, 5, seed=_seed("ties", i, 9500 + i), h_ld=(2, 4)[i % 2], pick=pick, j_star=[1, 4, 3])
        for g2 in copies:
            case["bank"][g2] = case["bank"][g1]
        fac = dict(n_rows=3, n_bank=TIE_BANK, pts=37, n_tau=5, pick=pick, j_star=[1, 4, 3], g1=g1, copies=copies, tied="columns")
        out.append((f"templates {copies} copy {g1}", fac, case))
    i = len(out)
    case = RB.build(3, TIE_BANK, 37, 5, seed=_seed("ties", i, 9500 + i), pick=[0, 0, 0], j_star=[1, 4, 3])
    case["bank"][:] = case["bank"][0]
    out.append((f"{TIE_BANK} identical templates", dict(n_rows=3, n_bank=TIE_BANK, pts=37, n_tau=5, pick=[0, 0, 0], j_star=[1, 4, 3], g1=0,
                                                         copies=tuple(range(1, TIE_BANK)), tied="bank"), case))
    for n_tau in (17, 33):
        i = len(out)
        case = RB.build(17, 18, 37, n_tau, seed=_seed("ties", i, 9500 + i), h_ld=(2, 4)[i % 2])
        case["freqs"] = torch.zeros_like(case["freqs"])  # step and start are (cos, sin) = (1, 0) exactly: z is the same at every shift
        out.append((f"freqs=0 n_tau={n_tau}", dict(n_rows=17, n_bank=18, pts=37, n_tau=n_tau, tied="shifts"), case))
    return out


# ---- 6: exact scalings ---------------------------------------------------------------------------------------------------------------
def scaled():
    """The factors hold ``base`` (the unscaled case) and the powers a, b, c of two on the rows' amplitudes, the templates' and the
    weights.  hh, gg and their scaled values stay normal fp32 numbers."""
    out = []
    for family, key, value, a, b, c in SCALINGS:
        tag, fac, base = next(x for x in cases(family) if x[1][key] == value)
        case = _clone(base)
        case["h"][..., 0] *= 2.0 ** a
        case["bank"][..., 0] *= 2.0 ** b
        case["weights"] = case["weights"] * 2.0 ** c
        out.append((f"{family} {tag} h*2^{a} bank*2^{b} w*2^{c}", dict(fac, base=base, a=a, b=b, c=c), case))
    return out


# ---- 7: the ends of the fp32 range ---------------------------------------------------------------------------------------------------
def extremes():
    """Row r's amplitudes times 2^P[r % 4], template g's times 2^P[(g + 1) % 4], the weights times 2^P[case], P = (-140, -100, 100,
    120): every combination of the four meets in some pair.  2^-140 leaves fp32 denormals (the inputs are what they are after the
    scaling; the reference reads the same).  By hand: |c|^2 is as small as (2^-140)^6 = 1e-253 times the sums and the match squared
    and hh gg as large as (2^120)^6 = 1e217 times the sums, both inside double (the host test measures 3.5e-252 and 7.8e218); hh and
    gg themselves leave the fp32 range at both ends, as inf and as 0.
    One more case: row 5 with phases of +-1e6 rad and template 7 with +-1e4 rad, amplitudes O(1)."""
    out = []
    P = EXTREME_POWERS
    for i, pw in enumerate(P):
        case = RB.build(17, 18, 37, 5, seed=_seed("extremes", i, 9700 + i), h_ld=(2, 4)[i % 2])
        case["h"][..., 0] *= torch.tensor([2.0 ** P[r % 4] for r in range(17)], dtype=torch.float64).view(17, 1).float()
        case["bank"][..., 0] *= torch.tensor([2.0 ** P[(g + 1) % 4] for g in range(18)], dtype=torch.float64).view(18, 1).float()
        case["weights"] = case["weights"] * 2.0 ** pw
        assert torch.isfinite(case["h"][..., 0]).all() and torch.isfinite(case["bank"]).all() and (case["weights"] > 0).all()
        assert (case["h"][..., 0] > 0).all() and (case["bank"][..., 0] > 0).all()
        out.append((f"weights*2^{pw}", dict(n_rows=17, n_bank=18, pts=37, n_tau=5, tied=None, w_power=pw), case))
    i = len(out)
    case = RB.build(17, 18, 37, 5, seed=_seed("extremes", i, 9700 + i))
    g = torch.Generator().manual_seed(9799)
    case["h"][5, :, 1] = (2.0 * torch.rand(37, generator=g) - 1.0) * 1e6
    case["bank"][7, :, 1] = (2.0 * torch.rand(37, generator=g) - 1.0) * 1e4
    out.append(("phases +-1e6 (row 5), +-1e4 (template 7)", dict(n_rows=17, n_bank=18, pts=37, n_tau=5, tied=None, w_power=0), case))
    return out


# ---- 8: permutations -----------------------------------------------------------------------------------------------------------------
def permutations():
    """The factors hold ``base``, ``axis`` ("bank" or "rows") and ``perm``: the permuted tensor is ``base[axis][perm]``."""
    big_tag, big_fac, big = RB.cases()[-1]
    assert (big_fac["n_rows"], big_fac["n_bank"], big_fac["pts"], big_fac["n_tau"]) == (33, 40, 129, 17)
    wide_tag, wide_fac, wide = next(x for x in cases("wide_banks") if x[1]["n_bank"] == 129)
    out = []
    for name, fac, base in ((f"wide_banks {wide_tag}", wide_fac, wide), ("feature suite " + big_tag, big_fac, big)):
        for axis, n in (("bank", fac["n_bank"]), ("rows", fac["n_rows"])):
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(9800 + len(out)))
            assert not torch.equal(perm, torch.arange(n))
            case = _clone(base)
            key = "bank" if axis == "bank" else "h"
            case[key] = base[key][perm].clone()
            out.append((f"{name}: {axis} permuted", dict(n_rows=fac["n_rows"], n_bank=fac["n_bank"], pts=fac["pts"], n_tau=fac["n_tau"],
                                                           base=base, axis=axis, perm=perm, tied=None), case))
    return out


_BUILDERS = dict(point_passes=point_passes, removed_patterns=removed_patterns, wide_banks=wide_banks, long_grids=long_grids, ties=ties,
                 scaled=scaled, extremes=extremes, permutations=permutations)
_CACHE, _REFS = {}, {}


def cases(family):
    """The (tag, factors, case) list of a family; built once, shared and never modified."""
    if family not in _CACHE:
        _CACHE[family] = _BUILDERS[family]()
    return _CACHE[family]


def reference_args(fac, case):
    """What the float64 reference is evaluated on: the cut call of a removed pattern, the case itself otherwise."""
    return fac["cut"] if "cut" in fac else call_args(case)


def reference_bytes(fac, case):
    """The size of the reference's largest intermediate, [R, G, T, n] in complex128."""
    a = reference_args(fac, case)
    return a["h"].shape[0] * a["bank"].shape[0] * a["h"].shape[1] * (a["taus"][2] if a["taus"] is not None else 1) * 16


def references(family):
    """[(tag, factors, case, float64 reference)] of a family; computed once for the host and the GPU tests and never modified."""
    if family not in _REFS:
        _REFS[family] = [(tag, fac, case, RB.reference(**reference_args(fac, case))) for tag, fac, case in cases(family)]
    return _REFS[family]


def margins(ref, skip_columns=()):
    """(smallest runner-up margin over the shifts of every pair, over the templates of every row) of a reference, normalised; inf
    without a choice.  ``skip_columns``: templates left out of the second (planted copies of another column)."""
    over_j = over_g = math.inf
    if ref["mag"].shape[2] >= 2:
        top = ref["mag"].topk(2, dim=2).values
        over_j = float((top[..., 0] - top[..., 1]).min())
    keep = [g for g in range(ref["match"].shape[1]) if g not in set(skip_columns)]
    if len(keep) >= 2:
        top = ref["match"][:, keep].topk(2, dim=1).values
        over_g = float((top[:, 0] - top[:, 1]).min())
    return over_j, over_g
