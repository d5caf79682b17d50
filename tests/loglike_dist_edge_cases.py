"""Input builders of the distance-marginalised likelihood's edge suite (``npf_waveform_loglike_dist`` / ``npf_waveform_loglike_net_dist``)
at the grid, scale, tie and size edges the feature suite's shapes (n_tau <= 257, n_a <= 300, one scale range 2^-4 .. 2^4, D <= 3)
never reach.  Everything is built with ``loglike_reference.build`` / ``loglike_net_reference.build``, the scale grids of
``loglike_dist_reference`` and, where they fit, the cases of ``waveform_edge_cases``; B = 3, T = 37 (200 in the one case that needs a
loud template).  The reference is always ``loglike_dist_reference.marginalise`` of the parent's float64 reference and the gates are
``loglike_dist_reference.ratios``, unchanged.

``cases(family, network)`` -> list of (tag, factors, case, scales, log_prior), built once, shared and never modified:

``time_edges``       n_tau at 255 / 256 (a finishing thread's stride), 4095 / 4096 / 4097 (the x_j of launch A in LDS or re-read) and
                     the 4099-shift grid of ``waveform_edge_cases.long_grids`` with the maximiser at its last index; n_a = SC + 1: two
                     chunks of scales read the same candidates.  "planted" and "noise" everywhere, "removed" and "degenerate" with
                     counts (T, 17, 0) at 4096 / 4097, "loud" at 4097.
``scale_edges``      n_a at 255 / 256 (launch B's stride) and 4095 / 4096 (NPF_DIST_MAX_SCALES: 256 chunks, the last partial or full),
                     without a grid and with 17 shifts; the grids "geo", "dead", the whole last or first chunk of SC scales dead, and
                     "rev": the geometric grid descending, so that the prior puts the maximum at the LAST index.
``duplicated_best``  a 300-point grid whose best (a, ln pi) pair is written to an index set: the maximum is attained on the set by
                     construction and ``scale_index`` is its smallest member.  The sets isolate the levels of the reduction.
``flat_evidence``    every weight zero (HH == 0) and a constant log prior: u_i = ln pi for every i, ``scale_index`` 0.
``shift_ties``       the zero-frequency grids of ``waveform_edge_cases.ties``: every shift ties, x* is any of them.
``magnitudes``       u ~ 1e6; scales of 2^-600 .. 2^-20; a grid over 2^-30 .. 2^30; 17 scales with a x* within 8 x 2^-50 of the
                     ``ln I0`` switch point.
``mixture_orders``   the three latent blocks of a "loud" case in all six orders, on a grid (2^-4 .. 1) that keeps them > 745 apart.
``eight_detectors``  the network twin at D = NPF_NET_MAX_DET.

``reference(network, case, scales, log_prior)`` -> (parent reference, ``marginalise`` of it), cached; a tensor [R, n_a, n] beyond
``REF_DOUBLES`` is evaluated in chunks of scales.  tests/test_loglike_dist_edges_host.py checks every claim made here on the CPU."""
import itertools
import math

import torch

import loglike_dist_reference as Dd
import loglike_net_reference as N
import loglike_reference as R1
import match_reference as M
import waveform_edge_cases as W

B = Dd.B
SC = Dd.SC
T = 37
THREADS = 256       # kWfLlThreads: the workgroup of both launches
LDS_TAU = 4096      # kWfDistLdsTau: the longest grid whose x_j launch A keeps in LDS
MAX_SCALES = 4096   # NPF_DIST_MAX_SCALES
MAX_DET = 8         # NPF_NET_MAX_DET
A_SIZES = (THREADS - 1, THREADS, LDS_TAU - 1, LDS_TAU, LDS_TAU + 1)
A_LAST = W.LONG_GRIDS[-1]  # 4099, the maximiser at index 4098
B_SIZES = (THREADS - 1, THREADS, MAX_SCALES - 1, MAX_SCALES)
B_KINDS = {None: ("geo", "dead_last", "rev"), 17: ("dead", "dead_first", "rev")}
# index sets of the duplicated best scale (the grid's own best index is 0): one thread of launch B at two strides; two lanes of a
# wave 32 and 37 apart (the first and several xor steps); neighbouring lanes; two waves; the smaller index in a later wave than the
# larger ((200, 257): wave 3 and wave 0; (70, 130, 299): waves 1, 2, 0) -- and in different chunks of launch A, but for the two neighbours
TIE_SETS = ((0, 256), (5, 37), (3, 40), (8, 9), (10, 100), (200, 257), (70, 130, 299))
FLAT_LP = -1.75  # the constant log prior of ``flat_evidence`` (not normalised: lnl_dist = FLAT_LP + ln n_a)
FLAT_N_A = (2, SC + 1, 257)
FLAT_N_TAU = (None, 17, LDS_TAU + 1)
I0_SWITCH = 24.0    # functional.LOGLIKE_I0_SWITCH, the default ``x_s`` of ``build``
SWITCH_K = tuple(range(-8, 9))
REF_DOUBLES = 1_000_000
FAMILIES = ("time_edges", "scale_edges", "duplicated_best", "flat_evidence", "shift_ties", "magnitudes", "mixture_orders", "eight_detectors")
# (family, network, case number) -> the factor on the data in place of ``loglike_dist_reference.DATA_SCALE``, for the cases that one
# left with ``scale_index`` ill posed (tests/test_loglike_dist_edges_host.py checks every case)
DATA_SCALE_OF = {}


def _mod(network):
    return N if network else R1


def _case(network, regime, n_tau, seed, key=None, T=T, j_star=None, **fac):
    """One input set of the parent's ``build`` with the data times DATA_SCALE -> (case, factors)."""
    Mod = _mod(network)
    need_w = regime in ("removed", "degenerate")
    fac = dict(dict(counts=None, n_z=1, h_ld=2, wform="BT" if need_w else None, fform="T" if n_tau else None), **fac)
    if network:
        fac.setdefault("D", 2)
    case = Mod.build(regime, T, taus=Mod.grid(n_tau, regime), j_star=j_star, seed=seed, **fac)
    case["data"] = case["data"] * DATA_SCALE_OF.get(key, Dd.DATA_SCALE)
    return case, dict(fac, regime=regime, T=T, n_tau=n_tau)


def _tag(network, fac, extra=""):
    keys = ("regime", "T", "n_tau", "n_a", "kind", "sform", "pform", "counts", "n_z", "h_ld", "wform", "fform", "D")
    return ("net " if network else "") + " ".join(f"{k}={fac[k]}" for k in keys if k in fac) + extra


def forms(a, sform, pform):
    """(scales, log_prior) of the grid ``a`` [n_a] with the volume prior, in the forms of ``loglike_dist_reference.scale_grid``."""
    s = torch.stack([a * 2.0 ** (b / 10.0) for b in range(B)]) if sform == "BA" else a
    p = torch.stack([Dd.volume_prior(a, 3.0 + 0.5 * b) for b in range(B)]) if pform == "BA" else Dd.volume_prior(a)
    return s, p


def _put(out, network, fac, case, s, p, extra=""):
    fac = dict(fac, n_a=s.shape[-1], sform="BA" if s.dim() == 2 else "A", pform="BA" if p.dim() == 2 else "A")
    out.append((_tag(network, fac, extra), fac, case, s, p))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
_PARENT, _DIST = {}, {}


def parent_reference(network, case, no_grid=False):
    """The parent's float64 reference of the case (``no_grid``: of the same inputs without a time grid), computed once."""
    key = (id(case), no_grid)
    if key not in _PARENT:
        Mod = _mod(network)
        _PARENT[key] = (case, Mod.reference(**dict(Mod.call_args(case), **(dict(taus=None) if no_grid else {}))))
    return _PARENT[key][1]


def marginalise(ref, scales, log_prior, limit=REF_DOUBLES):
    """``loglike_dist_reference.marginalise``; where its [R, n_a, n] tensor would pass ``limit`` doubles the evidence is evaluated
    over chunks of scales (each u_i depends on its own scale alone) and finished as there."""
    Rn, n = ref["x"].shape
    n_a = scales.shape[-1]
    if Rn * n_a * n <= limit:
        return Dd.marginalise(ref, scales, log_prior)
    step = max(1, limit // (Rn * n))
    parts = [Dd.evidence(ref, scales[..., i:i + step], log_prior[..., i:i + step]) for i in range(0, n_a, step)]
    u, live, a, lp = (torch.cat(t, 1) for t in zip(*parts))
    out = Dd._finish(u, ref)
    term = a * (ref["hh"] * ref["dd_rows"]).sqrt().view(-1, 1) + 0.5 * a ** 2 * ref["hh"].view(-1, 1) + lp.abs()
    out.update(live=live, S=torch.where(live, term, torch.zeros_like(term)).max(1).values)
    return out


def reference(network, case, scales, log_prior, no_grid=False):
    """(parent reference, marginalise(parent reference, scales, log_prior)), computed once per (case, scales, log_prior) object."""
    key = (id(case), id(scales), id(log_prior), no_grid)
    if key not in _DIST:
        ref = parent_reference(network, case, no_grid)
        _DIST[key] = (case, scales, log_prior, ref, marginalise(ref, scales, log_prior))
    return _DIST[key][3:]


def per_scale_margin(ref, dist, scales, log_prior):
    """Per row: the smallest (max_i u_i - u_k) / (1e-10 (S_best + S_k) + 2e-12) over the other live scales k, with S_i = a_i sqrt(HH DD)
    + a_i^2 HH / 2 + |ln pi_i| the size of the terms of u_i ALONE.  The row gate takes the largest S_i of the row, which on a grid
    up to 2^30 is 1e18 and says nothing about the small scales where the maximum lies; a double evaluation of u_i errs by a few ulp of
    its own terms, so two scales this many own-sized gates apart cannot swap.  Used only to decide whether ``scale_index`` may be
    asserted exactly on the wide grid; no output is gated by it."""
    Rn = dist["u"].shape[0]
    a, lp = Dd._per_row(scales, B, Rn), Dd._per_row(log_prior, B, Rn)
    live, u = dist["live"], dist["u"]
    own = torch.where(live, a * (ref["hh"] * ref["dd_rows"]).sqrt().view(-1, 1) + 0.5 * a ** 2 * ref["hh"].view(-1, 1) + lp.abs(),
                      torch.zeros_like(u))
    at = dist["scale_index"].view(-1, 1)
    margin = (u.gather(1, at) - u) / (1e-10 * (own.gather(1, at) + own) + 2e-12)
    margin = torch.where(live, margin, torch.full_like(margin, math.inf))
    margin.scatter_(1, at, math.inf)
    return margin.min(1).values


# ---- A: time-grid edges ------------------------------------------------------------------------------------------------------------
def time_edges(network):
    out = []
    for n_tau in A_SIZES:
        regimes = ["planted", "noise"] + (["removed", "degenerate"] if n_tau >= LDS_TAU else []) + (["loud"] if n_tau == LDS_TAU + 1 else [])
        for regime in regimes:
            i = len(out)
            if regime in ("removed", "degenerate"):
                kw = dict(counts=(T, 17, 0), n_z=3, wform=("T", "BT")[i % 2])
            else:
                kw = dict(n_z=3 if regime == "loud" else (1, 3)[i % 2], wform=(None, "T", "BT")[i % 3])
            j_star = {"planted": (n_tau - 1, 129)[(i // 2) % 2], "loud": 2}.get(regime)
            case, fac = _case(network, regime, n_tau, 300 + i, ("time_edges", network, i), j_star=j_star, fform=("T", "BT")[(i // 2) % 2],
                              h_ld=(2, 4)[i % 2], **kw)
            _put(out, network, fac, case, *Dd.scale_grid(SC + 1, ("A", "BA")[i % 2], ("A", "BA")[(i // 2) % 2]))
    tag, fac, case = next(c for c in W.cases("long_grids", "net" if network else "loglike")
                          if c[1]["n_tau"] == A_LAST and c[2].get("j_star") == A_LAST - 1)
    case = dict(case, data=case["data"] * Dd.DATA_SCALE)  # (a new dict and a new data tensor: the shared case stays as it is)
    _put(out, network, dict(fac, regime="planted"), case, *Dd.scale_grid(SC + 1, "BA", "A"), f" j*={A_LAST - 1}")
    return out


# ---- B: scale-axis edges -----------------------------------------------------------------------------------------------------------
def edge_grid(n_a, sform, pform, kind):
    """``loglike_dist_reference.scale_grid`` for "geo" and "dead"; "rev": the geometric grid and its prior descending; "dead_last":
    every scale of the last chunk of SC (index SC floor((n_a - 1) / SC) on) is 0, negative, NaN or +inf; "dead_first": ln pi of
    the first SC scales is -inf, +inf or NaN."""
    if kind in ("geo", "dead"):
        return Dd.scale_grid(n_a, sform, pform, kind)
    s, p = Dd.scale_grid(n_a, sform, pform, "geo")
    if kind == "rev":
        return s.flip(-1).contiguous(), p.flip(-1).contiguous()
    s, p = s.clone(), p.clone()
    if kind == "dead_last":
        lo = SC * ((n_a - 1) // SC)
        s[..., lo:] = torch.tensor([0.0, -1.0, math.nan, math.inf], dtype=torch.float64).repeat(SC // 4)[:n_a - lo]
    else:
        assert kind == "dead_first"
        p[..., :SC] = torch.tensor([Dd.NEG_INF, math.inf, math.nan, Dd.NEG_INF], dtype=torch.float64).repeat(SC // 4)
    return s, p


def scale_edges(network):
    out = []
    for n_a in B_SIZES:
        for n_tau, kinds in B_KINDS.items():
            for kind in kinds:
                i = len(out)
                case, fac = _case(network, "noise", n_tau, 400 + i, ("scale_edges", network, i), n_z=(1, 3)[i % 2],
                                  counts=(None, (T, 17, 0))[(i // 2) % 2], wform=(None, "T", "BT")[i % 3], h_ld=(2, 4)[(i // 3) % 2])
                s, p = edge_grid(n_a, ("A", "BA")[(i // 2) % 2], ("A", "BA")[i % 2], kind)
                _put(out, network, dict(fac, kind=kind), case, s, p)
    return out


# ---- C: ties ---------------------------------------------------------------------------------------------------------------------
def duplicated_best(network):
    """The factors hold ``set`` (the indices that attain the maximum) and ``i0`` (the best index of the grid before it was edited)."""
    out = []
    for sform, pform in (("A", "A"), ("BA", "BA")):
        case, fac = _case(network, "noise", 17, 500 + len(out), ("duplicated_best", network, len(out)), n_z=3, wform="BT", fform="BT")
        s0, p0 = Dd.scale_grid(300, sform, pform)
        idx0 = reference(network, case, s0, p0)[1]["scale_index"]
        i0 = int(idx0[0])
        assert (idx0 == i0).all() and i0 == 0, "the tie sets assume that every row's best scale is index 0: move them"
        for members in TIE_SETS:
            s, p = s0.clone(), p0.clone()
            if i0 not in members:  # the old best takes the pair of the set's first member: the maximum moves onto the set
                s[..., i0], p[..., i0] = s0[..., members[0]], p0[..., members[0]]
            for i in members:
                s[..., i], p[..., i] = s0[..., i0], p0[..., i0]
            _put(out, network, dict(fac, set=members, i0=i0), case, s, p, f" best at {members}")
    return out


def flat_evidence(network):
    out = []
    for n_a in FLAT_N_A:
        for n_tau in FLAT_N_TAU:
            i = len(out)
            case, fac = _case(network, "degenerate", n_tau, 600 + i, n_z=1 if n_tau == LDS_TAU + 1 else (3, 1)[i % 2], wform="T",
                              counts=(None, (T, 17, 0))[i % 2], h_ld=(2, 4)[i % 2])
            a = Dd.geometric(n_a)
            s = forms(a, ("A", "BA")[i % 2], "A")[0]
            p = torch.full((B, n_a) if (i // 2) % 2 else (n_a,), FLAT_LP, dtype=torch.float64)
            _put(out, network, fac, case, s, p)
    return out


def shift_ties(network):
    """The T = 37 cases of ``waveform_edge_cases.ties`` (n_tau 17, 257, 1000).  Their reference is that of the same inputs without a
    grid (``reference(..., no_grid=True)``): every x_j is the one candidate's, so S_i = n and u_i = M_i."""
    out = []
    for tag, fac, case in W.cases("ties", "net" if network else "loglike"):
        if fac["T"] != T:
            continue
        i = len(out)
        case = dict(case, data=case["data"] * Dd.DATA_SCALE)
        _put(out, network, dict(fac, regime="noise"), case, *Dd.scale_grid(SC + 1, ("A", "BA")[i % 2], ("BA", "A")[i % 2]), " freqs=0")
    return out


# ---- D: magnitudes -----------------------------------------------------------------------------------------------------------------
def switch_scales(x_best):
    """[B, 9 + 17]: a_{b,i} = (24 / x*_b) (1 + k 2^-50), k = -8 .. 8, between the lower four and the upper five of the nine scales
    2^-4 .. 2^4."""
    around = torch.tensor([1.0 + k * 2.0 ** -50 for k in SWITCH_K], dtype=torch.float64)
    plain = Dd.geometric(9)
    return torch.stack([torch.cat([plain[:4], (I0_SWITCH / x) * around, plain[4:]]) for x in x_best.tolist()])


def magnitudes(network):
    """The factors hold ``sub``: "u1e6", "tiny", "wide" or "switch"."""
    out = []
    for sform, pform in (("A", "A"), ("BA", "BA")):
        case, fac = _case(network, "loud", 17, 700 + len(out), ("magnitudes", network, len(out)), T=200, j_star=2, n_z=3, h_ld=4, wform="T")
        case["h"][..., 0] *= 16.0  # (exact)
        case["data"] = case["data"] * 16.0
        _put(out, network, dict(fac, sub="u1e6"), case, *Dd.scale_grid(65, sform, pform), " h, data x 2^4")
    for regime, sform, pform in (("noise", "A", "BA"), ("planted", "BA", "A")):
        case, fac = _case(network, regime, 17, 700 + len(out), ("magnitudes", network, len(out)), j_star=5 if regime == "planted" else None,
                          n_z=3, wform="BT")
        _put(out, network, dict(fac, sub="tiny"), case, *forms(Dd.geometric(33, -600.0, -20.0), sform, pform), " scales 2^-600 .. 2^-20")
    for n_tau, sform, pform in ((17, "A", "A"), (None, "BA", "BA")):
        case, fac = _case(network, "noise", n_tau, 700 + len(out), ("magnitudes", network, len(out)), n_z=3, wform="T")
        _put(out, network, dict(fac, sub="wide"), case, *forms(Dd.geometric(65, -30.0, 30.0), sform, pform), " scales 2^-30 .. 2^30")
    case, fac = _case(network, "edge", 17, 700 + len(out), ("magnitudes", network, len(out)), j_star=2, n_z=1, wform="BT", fform="BT")
    s = switch_scales(parent_reference(network, case)["x"].max(1).values)
    _put(out, network, dict(fac, sub="switch"), case, s, Dd.volume_prior(s), " a x* = 24 (1 + k 2^-50)")
    return out


# ---- E: the order of the mixture's rows ---------------------------------------------------------------------------------------------
def mixture_orders(network):
    """The three latent blocks of one case in every order (``perm`` in the factors: block ``perm[s]`` of the case stands at s).
    "loud" (``apart``): the grid ends at a = 1, below every row's own best scale, so the rows' evidences lie as far apart as the plain
    likelihoods do, more than 745: a later, larger row rescales the running sum to 0 and a later, smaller one adds 0.  "edge": rows a
    few units apart on the usual grid, where a later, smaller row adds a term that counts."""
    out = []
    for regime, (s, p) in (("loud", forms(Dd.geometric(SC + 1, -4.0, 0.0), "A", "BA")), ("edge", Dd.scale_grid(SC + 1, "BA", "A"))):
        case, fac = _case(network, regime, 17, 800, ("mixture_orders", network, len(out)), j_star=2, n_z=3, h_ld=4, wform="BT")
        for perm in itertools.permutations(range(3)):
            h = case["h"].view(3, B, T, -1)[list(perm)].reshape(case["h"].shape).clone()
            _put(out, network, dict(fac, perm=perm, apart=regime == "loud"), dict(case, h=h), s, p, f" blocks {perm}")
    return out


# ---- F: eight detectors ------------------------------------------------------------------------------------------------------------
def eight_detectors(network):
    assert network
    out = []
    for regime in ("noise", "planted"):
        for n_tau in (17, LDS_TAU + 1):
            i = len(out)
            case, fac = _case(True, regime, n_tau, 900 + i, ("eight_detectors", True, i), D=MAX_DET, j_star=n_tau - 1 if regime == "planted" else None,
                              n_z=(3, 1)[i % 2], counts=(None, (T, 17, 0))[(i // 2) % 2], wform=("BT", "T")[i % 2], fform=("T", "BT")[i % 2],
                              h_ld=(2, 4)[i % 2])
            _put(out, True, fac, case, *Dd.scale_grid(SC + 1, ("A", "BA")[i % 2], ("BA", "A")[i % 2]))
    return out


_BUILDERS = dict(time_edges=time_edges, scale_edges=scale_edges, duplicated_best=duplicated_best, flat_evidence=flat_evidence,
                 shift_ties=shift_ties, magnitudes=magnitudes, mixture_orders=mixture_orders, eight_detectors=eight_detectors)
_CACHE = {}


def cases(family, network):
    """The (tag, factors, case, scales, log_prior) list of a family, single stream or network; built once and never modified."""
    key = (family, bool(network))
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[family](bool(network))
    return _CACHE[key]


def streams(family):
    return (True,) if family == "eight_detectors" else (False, True)


# ---- G: independence from earlier calls --------------------------------------------------------------------------------------------
def independence(network):
    """dict(target, big: (case, scales, log_prior) of this stream -- n_a = n_tau = 17 and n_a = 300, n_tau = 257 on other data; match:
    a ``match_reference`` case; other: a (case, scales, log_prior) of the OTHER stream (the network's with D = 3))."""
    key = ("independence", bool(network))
    if key not in _CACHE:
        target = _case(network, "noise", 17, 950, n_z=3, wform="BT")[0]
        big = _case(network, "planted", 257, 951, j_star=200, n_z=3, T=65, wform="T", fform="BT")[0]
        other = _case(not network, "planted", 17, 952, j_star=9, n_z=3, **(dict() if network else dict(D=3)))[0]
        _CACHE[key] = dict(target=(target,) + Dd.scale_grid(SC + 1, "BA", "A"), big=(big,) + Dd.scale_grid(300, "A", "BA", "dead"),
                           match=M.build("random", 129, n_z=3, taus=M.grid(257), seed=7),
                           other=(other,) + Dd.scale_grid(65, "A", "A"))
    return _CACHE[key]
