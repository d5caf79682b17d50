"""Input builders of the waveform edge suite: the match (``npf_waveform_match``), its gradient (``npf_waveform_match_bwd``), the
likelihood (``npf_waveform_loglike``) and the detector network (``npf_waveform_loglike_net``) at the thread, grid and tie edges the
feature suites' common grid of shapes (T in {37, 200}, n_tau <= 257) never reaches.  Everything is built with the ``build`` functions
of match_reference, loglike_reference and loglike_net_reference and checked against their ``reference``; B = 3 as there.

``cases(family, entry)`` -> list of (tag, factors, case) for the entry points "match", "grad" (the match's inputs), "loglike" and "net":

``thread_edges``  T at 1 and around 64, 128 and 256 -- the wave and the 128-thread stride of launch 1, the 256-thread blocks of the
                  backward and of the network finish -- with counts None, (T, T - 1, 17) or (T, 128, 0), clipped to T.
``long_rows``     T = 256 * 1024 + 37 with counts (T, 256 * 1024 + 1, 256 * 1024): the backward's grid-stride loop (match and gradient
                  only: the likelihood's hh / dd gate of 2^-50 is against an exactly rounded sum, which 262181 terms in plain double
                  do not meet -- a property of that gate).
``long_grids``    n_tau in {1000, 4099} at T = 37: chunk numbers up to 256, the maximiser in the last, partial chunk, at the first
                  index of chunk 62 and at the last of chunk 61; up to 17 passes per thread in the finishing loops.
``ties``          zero frequencies: every grid time gives the same sum bit for bit, so ``tau_index`` is 0 BY CONSTRUCTION (it is not
                  taken from the reference, whose ``exp`` over [R, T, n] does not give bit-equal columns); the values are those of
                  the same inputs without a grid.
``zero_corr``     a live template against data that are all zero (likelihoods), and two points whose contributions cancel to the
                  last bit (match: c = 0 with hh gg > 0, where the backward has no direction to move in).
``near_match``    the "same" regime with the prediction's amplitude and phase perturbed by eps in {1e-2, 1e-3, 1e-4}: mismatches of
                  1e-4, 1e-6 and 1e-8, the range the match kernel is written for.
``scaled``        three thread-edge cases with the amplitudes times 2^+-40 and the weights times 2^+-20: exact scalings under which
                  match, overlap, phase and index are invariant.

Regimes are named as in match_reference; the likelihoods' "noise" stands for "random" and "planted" for "shift".  A case whose first
seed leaves ``tau_index`` ill posed gets another one through ``SEED_SHIFT`` (tests/test_waveform_edges_host.py checks every case).

``near_ratios`` is the one new gate: |d| <= 2^-23 |ref| + 16 T 2^-53 for match, mismatch and overlap.  The floor is derived: hh, gg and
c are double sums of T terms bounded by the sums' own size, each off by at most about T 2^-53 relative with ulp-level sines, so
m = |c| / sqrt(hh gg) is off by about 4 T 2^-53 (c counts twice: its two components); the gate allows four times that.  The
existing absolute 1e-9 is 10 % of a mismatch of 1e-8."""
import math

import torch

import loglike_net_reference as N
import loglike_reference as L1
import match_reference as M

JC = 16
B = M.B
EDGE_T = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LONG_T = 256 * 1024 + 37
LONG_COUNTS = (LONG_T, 256 * 1024 + 1, 256 * 1024)
LONG_GRIDS = (1000, 4099)
NEAR_EPS = (1e-2, 1e-3, 1e-4)
ENTRIES = ("match", "grad", "loglike", "net")
FAMILIES = {"thread_edges": ENTRIES, "long_rows": ("match", "grad"), "long_grids": ENTRIES, "ties": ENTRIES, "zero_corr": ENTRIES,
            "near_match": ("match", "grad"), "scaled": ("match", "grad")}
LL_REGIME = {"random": "noise", "removed": "removed", "shift": "planted"}
# (family, kind of input, case number) -> what is added to its seed.  Match case 70 of the thread edges ("random", T = 257, n_tau = 17,
# counts (257, 256, 17), freqs [T]): the 17 lowest of 257 shared frequencies span 20 .. 51 Hz, |c_j| varies slowly over the grid and
# the first seed left a gap of 4.9e-7 in the task of 17 points
SEED_SHIFT = {("thread_edges", "match", 70): 1000}


def _kind(entry):
    return "match" if entry in ("match", "grad") else entry


def _build(kind, regime, T, number, family, D=None, **kw):
    """``build`` of the entry point's reference module (a local wrapper: the likelihoods take their own regime names and D)."""
    seed = 100 + number + SEED_SHIFT.get((family, kind, number), 0)
    if kind == "match":
        return M.build(regime, T, seed=seed, **kw)
    if kind == "loglike":
        return L1.build(LL_REGIME[regime], T, seed=seed, **kw)
    return N.build(LL_REGIME[regime], T, D=D, seed=seed, **kw)


def _tag(regime, T, n_tau, j_star, fac):
    return f"{regime} T={T} n_tau={n_tau}" + (f" j*={j_star}" if j_star is not None else "") + "".join(f" {k}={v}" for k, v in fac.items())


def call_args(kind, case):
    return {"match": M.call_args, "loglike": L1.call_args, "net": N.call_args}[kind](case)


def reference(kind, case, **over):
    """The float64 reference of the entry point's reference module on the case's inputs (``over``: arguments to replace)."""
    mod = {"match": M, "loglike": L1, "net": N}[kind]
    return mod.reference(**dict(mod.call_args(case), **over))


def recurrence(kind, case, **over):
    mod = {"match": M, "loglike": L1, "net": N}[kind]
    return mod.recurrence(**dict(mod.call_args(case), **over), jc=JC)


# ---- the families ------------------------------------------------------------------------------------------------------------------
def edge_counts(T, i):
    """None, (T, T - 1, 17) or (T, 128, 0), clipped to T, by the case number."""
    return (None, (T, T - 1, min(17, T)), (T, min(128, T), 0))[i % 3]


def thread_edges(kind):
    out = []
    i = 0
    for T in EDGE_T:
        for regime in ("random", "removed", "shift"):
            for n_tau in ((None, 1) if T == 1 else (None, 17, 257)):  # (one point: every |c_j| is equal, so no grid with a choice)
                if regime == "shift" and n_tau is None:
                    continue
                j_star = None
                if regime == "shift":
                    stars = {1: [0], 17: [5, JC - 1, JC], 257: [JC + 5, 2 * JC - 1, 2 * JC, 256]}[n_tau]
                    j_star = stars[i % len(stars)]
                rem = regime == "removed"
                fac = dict(counts=edge_counts(T, i), n_z=(1, 3)[(i // 2) % 2], h_ld=(2, 4)[(i + i // 4) % 2],
                           wform="BT" if rem else (None, "T", "BT")[(i // 3) % 3], fform="BT" if rem else ("T", "BT")[(i // 5) % 2])
                if kind == "net":
                    fac["D"] = (1, 8)[i % 2]
                case = _build(kind, regime, T, len(out), "thread_edges", taus=M.grid(n_tau), j_star=j_star, **fac)
                out.append((_tag(regime, T, n_tau, j_star, fac), dict(fac, regime=regime, T=T, n_tau=n_tau), case))
                i += 1
    return out


def long_rows(kind):
    assert kind == "match"
    out = []
    for regime, j_star, fac in (("shift", 3, dict(counts=LONG_COUNTS, n_z=1, h_ld=4, wform=None, fform="T")),
                                ("random", None, dict(counts=LONG_COUNTS, n_z=1, h_ld=2, wform="BT", fform="BT"))):
        case = _build(kind, regime, LONG_T, len(out), "long_rows", taus=M.grid(5), j_star=j_star, **fac)
        out.append((_tag(regime, LONG_T, 5, j_star, fac), dict(fac, regime=regime, T=LONG_T, n_tau=5), case))
    return out


def long_grids(kind):
    out = []
    T = 37
    for n_tau in LONG_GRIDS:
        for regime, j_star in (("shift", n_tau - 1), ("shift", JC * 62), ("shift", JC * 62 - 1), ("random", None)):
            i = len(out)
            fac = dict(counts=(None, (T, 17, 0))[i % 2], n_z=3, h_ld=(2, 4)[(i // 2) % 2], wform=(None, "T", "BT")[i % 3],
                       fform=("T", "BT")[(i // 2) % 2])
            if kind == "net":
                fac["D"] = 2
            case = _build(kind, regime, T, i, "long_grids", taus=M.grid(n_tau), j_star=j_star, **fac)
            out.append((_tag(regime, T, n_tau, j_star, fac), dict(fac, regime=regime, T=T, n_tau=n_tau), case))
    return out


def ties(kind):
    out = []
    for T in (37, 129):
        for n_tau in (17, 257, 1000):
            i = len(out)
            fac = dict(counts=(None, (T, 17, 0))[(i // 2) % 2], n_z=(1, 3)[i % 2], h_ld=(2, 4)[(i // 3) % 2], wform=(None, "BT")[i % 2],
                       fform=("T", "BT")[(i // 2) % 2])
            if kind == "net":
                fac["D"] = 2
            case = _build(kind, "random", T, i, "ties", taus=M.grid(n_tau), **fac)
            case["freqs"] = torch.zeros_like(case["freqs"])  # the step is (cos, sin) = (1, 0) and every chunk restarts from sincos(theta + 0)
            if kind == "net":
                case["delays"] = None  # (a delay would enter through the frequencies, which are zero: keep the case clean)
            out.append((_tag("random", T, n_tau, None, fac) + " freqs=0", dict(fac, regime="random", T=T, n_tau=n_tau), case))
    return out


def _cancelling(T, live, n_tau, n_z, h_ld, seed):
    """A match case whose c_j are 0 to the last bit with hh gg > 0: the two live points have equal weights, equal amplitudes in ``h``
    (per row), theta = 0 and equal frequencies; the reference's amplitude has the opposite sign at the second (not a phase of pi,
    whose sine is not 0), so a_1 = -a_0 exactly and every rotation keeps that."""
    g_ = torch.Generator().manual_seed(9000 + seed)
    amp_h, amp_g = 0.5 + torch.rand(n_z * B, 1, generator=g_), 0.5 + torch.rand(B, 1, generator=g_)
    phase = 3.0 * torch.randn(B, T, generator=g_)
    h = torch.randn(n_z * B, T, h_ld, generator=g_)
    h[..., 0] = amp_h
    h[..., 1] = phase.repeat(n_z, 1)
    g = torch.stack([amp_g.expand(B, T).clone(), phase], -1)
    g[:, live[1], 0] = -g[:, live[1], 0]
    w = None
    if T > 2:  # every other point is removed
        w = torch.zeros(T)
        w[list(live)] = 0.75
    return dict(h=h, g=g, weights=w, freqs=torch.full((T,), 100.0), taus=M.grid(n_tau), n_valid=None)


def zero_corr(kind):
    out = []
    if kind == "match":
        for T, live in ((2, (0, 1)), (129, (5, 70)), (129, (3, 128))):  # the two points in one wave; in two waves; in one thread
            for n_tau in (None, 17):
                i = len(out)
                fac = dict(counts=None, n_z=(1, 3)[i % 2], h_ld=(2, 4)[(i // 2) % 2], wform=None if T == 2 else "T", fform="T", live=live)
                case = _cancelling(T, live, n_tau, fac["n_z"], fac["h_ld"], i)
                out.append((_tag("cancelling", T, n_tau, None, fac), dict(fac, regime="cancelling", T=T, n_tau=n_tau), case))
        return out
    T = 129
    for n_tau in (None, 17, 257):
        i = len(out)
        fac = dict(counts=(None, (T, 17, 0))[i % 2], n_z=(3, 1)[i % 2], h_ld=(2, 4)[i % 2], wform=(None, "BT", "T")[i % 3], fform=("T", "BT")[i % 2])
        if kind == "net":
            fac["D"] = (2, 3)[i % 2]
        case = _build(kind, "random", T, i, "zero_corr", taus=M.grid(n_tau), **fac)
        case["data"] = torch.zeros_like(case["data"])
        out.append((_tag("zero data", T, n_tau, None, fac), dict(fac, regime="zero data", T=T, n_tau=n_tau), case))
    return out


def near_match(kind):
    assert kind == "match"
    out = []
    for eps in NEAR_EPS:
        for T in (129, 257):
            for n_tau in (None, 17, 257):
                i = len(out)
                fac = dict(counts=None, n_z=3, h_ld=(2, 4)[i % 2], wform="BT", fform="BT")
                case = _build(kind, "same", T, i, "near_match", taus=M.grid(n_tau), **fac)
                g_ = torch.Generator().manual_seed(4000 + i)
                shape = case["h"].shape[:2]
                case["h"][..., 0] *= 1.0 + eps * torch.randn(shape, generator=g_)
                case["h"][..., 1] += eps * torch.randn(shape, generator=g_)
                out.append((_tag("same", T, n_tau, None, fac) + f" eps={eps:g}", dict(fac, regime="same", T=T, n_tau=n_tau, eps=eps), case))
    return out


# (T, regime, n_tau, factor of h's amplitudes, of g's, of the weights): the inverse and the same factor, both signs of every power
SCALINGS = ((65, "random", 17, 2.0 ** 40, 2.0 ** -40, 2.0 ** 20), (129, "removed", 257, 2.0 ** -40, 2.0 ** -40, 2.0 ** -20),
            (257, "random", None, 2.0 ** 40, 2.0 ** 40, 2.0 ** 20))


def scaled(kind):
    """The factors hold ``base`` (the unscaled thread-edge case) and the three powers of two.  hh and gg stay below 2^110."""
    assert kind == "match"
    edges = thread_edges("match")
    out = []
    for T, regime, n_tau, s_h, s_g, s_w in SCALINGS:
        tag, fac, base = next(c for c in edges if (c[1]["T"], c[1]["regime"], c[1]["n_tau"]) == (T, regime, n_tau))
        case = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in base.items()}
        if case["weights"] is None:
            base = dict(base, weights=torch.ones(T))  # (the same bits as None: tests/test_hip_match.py holds that)
            case["weights"] = torch.ones(T)
        case["h"][..., 0] *= s_h
        case["g"][..., 0] *= s_g
        case["weights"] = case["weights"] * s_w
        out.append((f"{tag} h*2^{round(math.log2(s_h))} g*2^{round(math.log2(s_g))} w*2^{round(math.log2(s_w))}",
                    dict(fac, base=base, s_h=s_h, s_g=s_g, s_w=s_w), case))
    return out


_BUILDERS = dict(thread_edges=thread_edges, long_rows=long_rows, long_grids=long_grids, ties=ties, zero_corr=zero_corr,
                 near_match=near_match, scaled=scaled)
_CACHE = {}


def cases(family, entry):
    """The (tag, factors, case) list of a family for an entry point; built once, shared and never modified ("grad": the match's)."""
    assert entry in FAMILIES[family], (family, entry)
    key = (family, _kind(entry))
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[family](key[1])
    return _CACHE[key]


# ---- the near-match gate -----------------------------------------------------------------------------------------------------------
def near_ratios(got, ref, T):
    """Worst |d| / (2^-23 |ref| + 16 T 2^-53) of match, mismatch and overlap (those ``got`` holds)."""
    out = {}
    for name in ("match", "mismatch", "overlap"):
        x = got.get(name)
        if x is None:
            continue
        x, r = x.detach().cpu().double().reshape(-1), ref[name].double().reshape(-1)
        assert x.shape == r.shape, (name, x.shape, r.shape)
        d = (x - r).abs()
        q = d / (2.0 ** -23 * r.abs() + 16.0 * T * 2.0 ** -53)
        out[name] = float(torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf)).max())
    return out
