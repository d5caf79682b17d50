"""Input builders of the sky-grid likelihood's edge suite: ``npf_waveform_loglike_sky`` (csrc/waveform_sky_kernels.hip) at the pass,
tile, workgroup, wave, stride, grid and tie edges that the feature suite (tests/loglike_sky_reference.py: rows <= 33, pixels <= 40,
points <= 129, grid times <= 17, n_z <= 3) never reaches.  Everything is built with ``loglike_sky_reference.build``, ``plant``, ``sky``
and ``grid`` and checked against its ``reference`` under its ``ratios``; tests/test_loglike_sky_edges_host.py checks on the CPU that
every case is well posed and reaches the path its family names.

``cases(family)`` -> list of (tag, factors, case); ``references(family)`` adds the float64 reference, computed once and shared.
The kernel constants the families rest on: ``PASS`` (kSkyPrepThreads), ``CORR_WAVES`` (kSkyCorrWaves: pixel tiles of 16 per workgroup
of the correlation launch), ``FINISH`` (kSkyFinishThreads), ``JC`` (NPF_SKY_JC).  Which path of the kernels each family reaches:

``point_passes``   T in {255, 256, 257, 511, 513, 1025}, all live, D rotating over 1, 2, 3: one pass of ``sky_prep_kernel``'s 256 threads
                   exactly full, a SECOND pass of one point (257) up to a third (513) and a fifth (1025) in the U panel, the V panel
                   and the step / start tables; ``hh_k`` sums more than one point per thread.  D = 8, T = 129: the k-step counter
                   ``t4`` of ``sky_chunk`` wraps 8 times with tq = 33.
``counts``         T = 300 (passes of 256 and 44), four tasks with ``n_valid`` = (0, 255, 257, 305) and (-3, 1, 256, 300): no live point,
                   a count that ends one short of the pass, one inside the second pass, one beyond T and a negative one
                   (``clamp_count``); NaN in ``h`` and ``data`` beyond every count.
``wide_skies``     P in {63, 64, 65, 80, 129, 257, 513}: ``blockIdx.y > 0`` in ``sky_corr_kernel``, wave 3 of a workgroup, the early
                   return of a wavefront without a tile in a later workgroup; waves 1 .. 3 and the second and third stride of
                   ``sky_finish_kernel`` with the winner in each of them; ``red_*`` rewritten over five rows of a task (n_z = 5);
                   the rescaling branch of the mixture (jitter = 0.5).
``dead_patterns``  P = 300 with whole tiles, workgroups and strides of dead pixels (``best_p`` stays ``n_pix`` in a thread and must lose
                   the reduction), every other pixel, and all but one: dead against cut, bit for bit.
``long_grids``     n_tau in {64, 1000, 4099} on an unequally spaced frequency grid: ``best_j``, ``best``, ``lse_m``, ``lse_s`` carried
                   over 8, 125 and 513 chunks with the maximiser first (every later shift takes the ``else`` branch of the
                   log-sum-exp), at both ends of chunks and in the partial last chunk; a grid that runs backwards, one 1 s from zero.
``ties``           BOTH TIE RULES, the expected indices by construction: duplicate pixels in neighbouring lanes, across a tile edge, in
                   two tiles of a workgroup, in two workgroups (= two finish waves), in two finish strides and in three places
                   (``pix_index`` is the smallest); 130 identical pixels; a zero template at P = 513; zero frequencies (``tau_index``
                   is the first, the register-held maximum carried over 3 and 13 chunks).
``scaled``         exact power-of-two rescalings of weights, amplitudes, data and response: invariant bits.
``extremes``       fp32 denormal amplitudes (HH about 2^-160), phases of +-1e4 and +-1e6 rad, delays within +-0.5 s.
``permutations``   P = 300, 9 rows, the pixels permuted across workgroups and strides: every output moves with its pixel, bit for bit.
``pixel_nan``      a NaN in the response of one live pixel: the other columns of ``snr_map`` keep their bits, ``lnl_sky`` is NaN.

The gates are those of ``loglike_sky_reference.ratios``, unchanged: lnl_sky, lnl_sky_mix and u = post + lnl_sky |d| <= 1e-10 scale +
1e-12; post, post_mix twice that; snr, snr_map 1e-10 relative + 1e-12; the indices exact; -inf met by -inf only.  Why none moves: the
reference and the kernel sum K = D T terms in double; at the longest row here (D = 3, T = 1025) that is about 3075 2^-53 = 3.4e-13
relative, three hundred times below 1e-10.  At the longest grid the phase argument reaches about 2 pi 512 Hz 2 s = 6.4e3 rad; a few
ulp of that is about 2e-12, fifty times below the gate.  The fixed-point pixel sum errs by at most 513 2^-62.

A case whose first seed leaves an index ill posed gets another seed through ``SEED_SHIFT``, with the reason."""
import math

import torch

import loglike_sky_reference as S
from match_bank_edge_cases import uneven_freqs  # 20 + 492 x^1.5 + 3 sin(17 x) Hz: |K(tau)| does not repeat inside a 2 s grid

DTAU = S.DTAU
PASS = 256       # kSkyPrepThreads
CORR_WAVES = 4   # kSkyCorrWaves
FINISH = 256     # kSkyFinishThreads
JC = 8           # NPF_SKY_JC
FAMILIES = ("point_passes", "counts", "wide_skies", "dead_patterns", "long_grids", "ties", "scaled", "extremes", "permutations",
            "pixel_nan")
PASS_POINTS = (255, 256, 257, 511, 513, 1025)
COUNT_POINTS = 300
COUNTS = ((0, 255, 257, 305), (-3, 1, 256, 300))
# (P, planted pixel, n_z, jitter)
WIDE = ((63, 62, 1, 0.05), (64, 63, 1, 0.05), (65, 64, 1, 0.05), (80, 79, 1, 0.05), (129, 128, 3, 0.05), (257, 255, 5, 0.05),
        (257, 256, 5, 0.5), (513, 512, 1, 0.05))
DEAD_P = 300
# (n_tau, the planted shift, kind)
LONG = ((64, 0, "+"), (64, 7, "+"), (64, 8, "+"), (64, 63, "+"), (1000, 991, "+"), (1000, 992, "+"), (1000, 999, "+"), (4099, 0, "+"),
        (4099, 4096, "+"), (4099, 4098, "+"), (64, 63, "-"), (64, 7, "tau0=1"))
TIE_P = 300
DUPLICATES = ((4, (5,)), (15, (16,)), (3, (35,)), (3, (67,)), (10, (266,)), (5, (70, 261)))
SCALINGS = (("point_passes", "T", 257), ("wide_skies", "P", 129))
# (family, case number) -> what is added to the case's seed, with the reason
SEED_SHIFT = {
    # jitter = 0.5: the fifth latent sample's amplitude factor 1 + 0.5 g comes near 0 with the first seed, and that row follows the
    # prior (pixel 181), not the planted pixel in the second finish stride
    ("wide_skies", 6): 100,
}


def _seed(family, number, base):
    return base + SEED_SHIFT.get((family, number), 0)


def _clone(case):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


call_args = S.call_args


def _rotate(i):
    """h_ld, the form of the weights and the prior of case i, as in ``loglike_sky_reference.sweep_sets``."""
    return dict(h_ld=(2, 4)[i % 2], wform=(None, "T", "BT")[i % 3], prior=bool((i // 2) % 2))


def _shape(case):
    Rn, T = case["h"].shape[:2]
    Bn, D = case["data"].shape[:2]
    return dict(rows=Rn, Bn=Bn, n_z=Rn // Bn, T=T, D=D, P=case["response"].shape[0], n_tau=0 if case["taus"] is None else case["taus"][2],
                p0=case["p0"], j0=case["j0"])


def _replant(case, seed, p0=None, j0=None, noise=0.02):
    """The data planted anew, in place, on the first latent sample's own waveform ``h[:B]`` through pixel p0 at grid time j0 of the
    case's CURRENT response, delays, freqs and grid."""
    Bn, D, T = case["data"].shape[:3]
    p0, j0 = case["p0"] if p0 is None else p0, case["j0"] if j0 is None else j0
    taus = case["taus"]
    g = torch.Generator().manual_seed(92000 + seed)
    d = S.plant(case["h"][:Bn, :, :2], case["response"][p0], case["delays"][p0], case["freqs"], 0.0 if taus is None else taus[0] + j0 * taus[1])
    case["data"] = (d + noise * torch.randn(Bn, D, T, 2, generator=g, dtype=torch.float64)).float()
    case["p0"], case["j0"] = p0, j0
    return case


# ---- 1: passes of the preparation launch -----------------------------------------------------------------------------------------------
def point_passes():
    out = []
    for i, T in enumerate(PASS_POINTS):
        case = S.build(Bn=3, n_z=1, T=T, D=1 + i % 3, P=5, n_tau=5, seed=_seed("point_passes", i, 1000 + i), **_rotate(i))
        out.append((f"T={T} D={1 + i % 3}", dict(_shape(case), tied=None), case))
    i = len(out)
    case = S.build(Bn=3, n_z=1, T=129, D=8, P=5, n_tau=5, seed=_seed("point_passes", i, 1000 + i), **_rotate(i))
    out.append(("T=129 D=8", dict(_shape(case), tied=None), case))
    return out


# ---- 2: counts -------------------------------------------------------------------------------------------------------------------------
def counts():
    """Four tasks, one latent sample each.  The first case goes through ``kill_points`` (dead weights as well), the second has every
    weight live, so its tasks hold exactly min(max(n_valid, 0), T) live points at every detector.  ``tau_tied_rows``: a task with ONE
    live point, whose |K_j| does not depend on j but for rounding; its ``tau_index`` is anyone's."""
    out = []
    T = COUNT_POINTS
    for i, nv in enumerate(COUNTS):
        case = S.build(Bn=4, n_z=1, T=T, D=3, P=5, n_tau=5, h_ld=(4, 2)[i], wform=("BT", "T")[i], prior=True,
                       seed=_seed("counts", i, 1100 + i), counts=nv)
        if i == 0:
            S.kill_points(case, 1100)
        else:
            case["dead"] = (torch.arange(T).view(1, 1, T) >= case["n_valid"].long().clamp(0, T).view(4, 1, 1)).expand(4, 3, T).clone()
            S.poison(case, math.nan)
        live = [min(max(n, 0), T) for n in nv]
        fac = dict(_shape(case), tied=None, n_valid=nv, live=live, empty_rows=[r for r in range(4) if live[r] == 0],
                   tau_tied_rows=[r for r in range(4) if live[r] == 1])
        out.append((f"n_valid={nv}", fac, case))
    return out


# ---- 3: skies of several workgroups, waves and strides -----------------------------------------------------------------------------------
def wide_skies():
    out = []
    for i, (P, p0, n_z, jitter) in enumerate(WIDE):
        case = S.build(Bn=3 if n_z == 1 else (2 if n_z == 3 else 1), n_z=n_z, T=37, D=3, P=P, n_tau=5, p0=p0, jitter=jitter,
                       seed=_seed("wide_skies", i, 1200 + i), **_rotate(i))
        out.append((f"P={P} p0={p0} n_z={n_z} jitter={jitter}", dict(_shape(case), tied=None, jitter=jitter), case))
    return out


# ---- 4: dead pixels in patterns ----------------------------------------------------------------------------------------------------------
def _dead_masks():
    """name -> (bool [300], True where the pixel is dead; the planted pixel)."""
    p = torch.arange(DEAD_P)
    out = {"tile 1": (p // 16 == 1, 150), "workgroup 1": (p // (16 * CORR_WAVES) == 1, 150), "stride 0": (p < FINISH, 280),
           "every other": (p % 2 == 1, 150)}
    for only in (0, FINISH - 1, FINISH, DEAD_P - 1):
        out[f"only pixel {only}"] = (p != only, only)
    return out


def dead_patterns():
    """The factors hold ``dead`` and ``cut``: the call arguments with the dead pixels removed, ``log_prior`` unchanged at the rest."""
    out = []
    kinds = torch.tensor([-math.inf, math.nan, math.inf], dtype=torch.float64)
    for i, (name, (dead, p0)) in enumerate(_dead_masks().items()):
        case = S.build(Bn=3, n_z=2, T=37, D=3, P=DEAD_P, n_tau=5, h_ld=(2, 4)[i % 2], wform=(None, "T", "BT")[i % 3], prior=True,
                       p0=p0, seed=_seed("dead_patterns", i, 1300 + i))
        cut = dict(call_args(case), response=case["response"][~dead].clone(), delays=case["delays"][~dead].clone(),
                   log_prior=case["log_prior"][~dead].clone())
        case["log_prior"][dead] = kinds[torch.arange(int(dead.sum())) % 3]  # the three kinds of a dead prior in rotation
        case["response"][dead] = math.nan
        case["delays"][dead] = math.nan
        out.append((name, dict(_shape(case), tied=None, pattern=name, dead=dead, cut=cut), case))
    return out


# ---- 5: long grids -----------------------------------------------------------------------------------------------------------------------
def long_grids():
    """Two tasks, two detectors, five pixels on the uneven frequency grid: the linear one of ``build`` (492 / 36 Hz apart at T = 37)
    makes x repeat every 150 shifts, and the runner-up then lies within 2.3e-5 at n_tau = 4099."""
    out = []
    for i, (n_tau, j0, kind) in enumerate(LONG):
        case = S.build(Bn=2, n_z=1, T=37, D=2, P=5, n_tau=5, seed=_seed("long_grids", i, 1400 + i), **_rotate(i))
        case["freqs"] = uneven_freqs(37)
        case["taus"] = {"+": S.grid(n_tau), "-": (2 * DTAU, -DTAU, n_tau), "tau0=1": (1.0, DTAU, n_tau)}[kind]
        _replant(case, 1400 + i, j0=j0)
        out.append((f"n_tau={n_tau} j0={j0} {kind}", dict(_shape(case), tied=None, kind=kind), case))
    return out


# ---- 6: ties -----------------------------------------------------------------------------------------------------------------------------
def ties():
    """``tied``: "pixels" (the factors hold ``g1`` and ``copies``: pixels equal to the planted pixel g1 in response, delays and prior),
    "sky" (130 identical pixels, no prior), "zero" (a zero template: every pixel and shift ties at u = -ln P, x = 0) or "shifts"
    (zero frequencies: every shift gives the same sum)."""
    out = []
    for g1, copies in DUPLICATES:
        i = len(out)
        case = S.build(Bn=3, n_z=1, T=37, D=3, P=TIE_P, n_tau=5, h_ld=(2, 4)[i % 2], wform=(None, "T", "BT")[i % 3], prior=True, p0=g1,
                       seed=_seed("ties", i, 1500 + i))
        for g2 in copies:
            for k in ("response", "delays", "log_prior"):
                case[k][g2] = case[k][g1]
        out.append((f"pixels {copies} copy {g1}", dict(_shape(case), tied="pixels", g1=g1, copies=copies), case))
    i = len(out)
    case = S.build(Bn=3, n_z=1, T=37, D=2, P=130, n_tau=5, p0=0, seed=_seed("ties", i, 1500 + i))
    case["response"][:] = case["response"][0]
    case["delays"][:] = case["delays"][0]
    out.append(("130 identical pixels", dict(_shape(case), tied="sky", g1=0, copies=tuple(range(1, 130))), case))
    i = len(out)
    case = S.build(Bn=3, n_z=1, T=37, D=2, P=513, n_tau=5, seed=_seed("ties", i, 1500 + i))
    case["h"][..., 0] = 0.0
    out.append(("zero template P=513", dict(_shape(case), tied="zero"), case))
    for n_tau in (17, 100):
        i = len(out)
        case = S.build(Bn=3, n_z=1, T=37, D=3, P=5, n_tau=n_tau, seed=_seed("ties", i, 1500 + i), **_rotate(i))
        case["freqs"] = torch.zeros_like(case["freqs"])  # step and start are (1, 0) exactly: z is the same bits at every shift
        _replant(case, 1500 + i)
        out.append((f"freqs=0 n_tau={n_tau}", dict(_shape(case), tied="shifts"), case))
    return out


# ---- 7: exact scalings -------------------------------------------------------------------------------------------------------------------
def _normal(x):
    a = x[torch.isfinite(x) & (x != 0)].abs()
    return bool((a >= 2.0 ** -126).all() and (a < 2.0 ** 127).all())


def scaled():
    """The factors hold ``base`` and the kind: "wad" weights * 2^(2k), amplitudes * 2^-k, data * 2^-k (k = +-40); "ca" response *
    2^k, amplitudes * 2^-k (k = +-60).  In both HH and every product entering K scale by exactly 1.  No fp32 input leaves the
    normal range, so every scaling is exact."""
    out = []
    for family, key, value in SCALINGS:
        tag, fac, base = next(x for x in cases(family) if x[1][key] == value)
        assert base["weights"] is not None
        for kind, ks in (("wad", (40, -40)), ("ca", (60, -60))):
            for k in ks:
                case = _clone(base)
                case["h"][..., 0] *= 2.0 ** -k
                if kind == "wad":
                    case["weights"] = base["weights"] * 2.0 ** (2 * k)
                    case["data"] = base["data"] * 2.0 ** -k
                else:
                    case["response"] = base["response"] * 2.0 ** k
                for name in ("h", "weights", "data"):
                    assert _normal(case[name]) and _normal(base[name]), f"{tag} {kind} k={k}: {name} leaves the normal fp32 range"
                assert torch.equal(case["h"][..., 0].double(), base["h"][..., 0].double() * 2.0 ** -k)
                assert torch.equal(case["data"].double(), base["data"].double() * (2.0 ** -k if kind == "wad" else 1.0))
                assert torch.equal(case["weights"].double(), base["weights"].double() * (2.0 ** (2 * k) if kind == "wad" else 1.0))
                out.append((f"{family} {tag} {kind} k={k}", dict(fac, base=base, kind=kind, k=k), case))
    return out


# ---- 8: value extremes -------------------------------------------------------------------------------------------------------------------
def extremes():
    out = []
    # amplitudes * 2^-140: fp32 denormals, rounded there; the reference reads the rounded values the kernel sees
    case = S.build(Bn=3, n_z=1, T=37, D=3, P=5, n_tau=5, h_ld=2, wform="T", prior=True, seed=_seed("extremes", 0, 1700))
    case["h"][..., 0] *= 2.0 ** -140
    case["weights"] = case["weights"] * 2.0 ** 120
    case["data"] = case["data"] * 2.0 ** 20
    assert ((case["h"][..., 0] > 0) & (case["h"][..., 0] < 2.0 ** -126)).all() and torch.isfinite(case["weights"]).all()
    out.append(("amplitudes*2^-140 weights*2^120 data*2^20", dict(_shape(case), tied=None, what="denormal"), case))
    # phases of +-1e4 and +-1e6 rad added, one task each; the data planted on the shifted waveform
    case = S.build(Bn=4, n_z=1, T=37, D=2, P=5, n_tau=5, h_ld=4, wform="BT", seed=_seed("extremes", 1, 1701))
    case["h"][..., 1] += torch.tensor([1e4, -1e4, 1e6, -1e6]).view(4, 1)
    _replant(case, 1701)
    out.append(("phases +-1e4, +-1e6 rad", dict(_shape(case), tied=None, what="phase"), case))
    # delays within +-0.5 s: 256 cycles at 512 Hz
    case = S.build(Bn=3, n_z=1, T=37, D=3, P=5, n_tau=5, h_ld=2, prior=True, seed=_seed("extremes", 2, 1702))
    case["response"], case["delays"] = S.sky(5, 3, torch.Generator().manual_seed(1702), span=0.5 / DTAU)
    _replant(case, 1702)
    out.append(("delays within +-0.5 s", dict(_shape(case), tied=None, what="delay"), case))
    return out


# ---- 9: permutations ---------------------------------------------------------------------------------------------------------------------
def permutations():
    """The factors hold ``base`` and ``perm``: pixel q of the case is pixel perm[q] of the base."""
    base = S.build(Bn=3, n_z=3, T=37, D=3, P=300, n_tau=5, h_ld=2, wform="BT", prior=True, seed=_seed("permutations", 0, 1800))
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(1800))
    case = _clone(base)
    for k in ("response", "delays", "log_prior"):
        case[k] = base[k][perm].clone()
    return [("P=300 pixels permuted", dict(_shape(case), tied=None, base=base, perm=perm), case)]


# ---- 10: a NaN in a live pixel -------------------------------------------------------------------------------------------------------------
def pixel_nan():
    """The factors hold ``base`` (the clean case) and ``bad``: the live pixel whose response holds a NaN (the first pixel of the second
    correlation workgroup and of finish wave 1; the planted pixel is 32)."""
    base = S.build(Bn=3, n_z=2, T=37, D=3, P=65, n_tau=5, h_ld=2, wform="T", prior=True, seed=_seed("pixel_nan", 0, 1900))
    case = _clone(base)
    case["response"][64, 1, 0] = math.nan
    return [("P=65 NaN in the response of pixel 64", dict(_shape(case), tied=None, base=base, bad=64), case)]


_BUILDERS = dict(point_passes=point_passes, counts=counts, wide_skies=wide_skies, dead_patterns=dead_patterns, long_grids=long_grids,
                 ties=ties, scaled=scaled, extremes=extremes, permutations=permutations, pixel_nan=pixel_nan)
_CACHE, _REFS = {}, {}


def cases(family):
    """The (tag, factors, case) list of a family; built once, shared and never modified."""
    if family not in _CACHE:
        _CACHE[family] = _BUILDERS[family]()
    return _CACHE[family]


def references(family):
    """[(tag, factors, case, float64 reference)] of a family; computed once for the host and the GPU tests and never modified.
    ``pixel_nan``: the reference of the clean base (the case itself is NaN by construction)."""
    if family not in _REFS:
        _REFS[family] = [(tag, fac, case, S.reference(**call_args(fac["base"] if family == "pixel_nan" else case)))
                         for tag, fac, case in cases(family)]
    return _REFS[family]


def where(p):
    """Where pixel p is computed: (tile of 16, correlation workgroup, wave of that workgroup, finish stride, finish wave)."""
    return dict(tile=p // 16, corr_wg=p // (16 * CORR_WAVES), corr_wave=(p // 16) % CORR_WAVES, stride=p // FINISH, wave=(p % FINISH) // 64)


def margins(fac, ref):
    """``loglike_sky_reference.margins`` with the planted ties of the case taken out: the copies of the planted pixel leave the
    pixels, a row whose shifts tie leaves the rows of the second figure.  -> (lead_u in gates, relative lead_x)."""
    P = ref["u"].shape[1]
    copies = set(fac.get("copies", ()))
    cols = torch.tensor([p for p in range(P) if p not in copies])
    pix = ref["pix_index"].clone()
    if copies:
        pix[torch.tensor([int(p) in copies for p in pix])] = fac["g1"]
    pix = (cols.view(1, -1) == pix.view(-1, 1)).double().argmax(1)
    rows = torch.tensor([r for r in range(ref["u"].shape[0]) if r % fac["Bn"] not in fac.get("tau_tied_rows", ())])
    sub = dict(u=ref["u"][:, cols], x=ref["x"][:, cols], scale=ref["scale"], live=ref["live"][cols], pix_index=pix)
    lead_u = S.margins(sub)[0]
    sub = dict(u=sub["u"][rows], x=sub["x"][rows], scale=sub["scale"][rows], live=sub["live"], pix_index=pix[rows])
    lead_x = S.margins(sub)[1]
    if fac["tied"] in ("sky", "zero"):
        lead_u = math.inf
    if fac["tied"] in ("shifts", "zero"):
        lead_x = math.inf
    return lead_u, lead_x
