"""The inputs of the likelihood gradient's edge suite (tests/test_hip_loglike_grad_edges.py on the GPU, tests/
test_loglike_grad_edges_host.py on the CPU): ``waveform_loglike_coef_kernel`` and ``waveform_loglike_bwd_kernel<LD, NET>`` at their
coefficient, tile, detector and value edges.  Every case is built with ``loglike_reference.build`` / ``loglike_net_reference.build``
and edited afterwards; B = 3 tasks.  ``cases(family)`` -> [(tag, factors, args)]; the factors every family sets:
    net      the network entry (``args`` holds response / delays) or the single stream
    kinds    the upstream combinations the GPU test runs through the standard check (``ups_of``)
    clear    the host test asserts ``clear_maximum`` (every case whose ``kinds`` reach lnl_max, outside family B)
    j_star   the grid index the maximiser is planted at, or None
Families: A (``saved`` against float64), B (one live point: every grid time ties), C1 .. C7 (the network backward), D1 .. D4 (grid
limits of the single stream), E1 .. E6 (values), F (workspace reuse)."""
import math

import torch

import loglike_grad_reference as G
import loglike_net_reference as RN
import loglike_reference as R1

JC, X_S = 16, 24.0        # NPF_WAVEFORM_JC, NPF_LOGLIKE_I0_SWITCH (the host test holds them against the sources)
TILE = 256                # kWfBwdTile == kWfBwdThreads == kWfLlThreads
MAX_TAU = 65536           # kWfMaxTau
B, T = R1.B, 37
DTAU = R1.DTAU
TWO_PI = R1.TWO_PI
LONG_T = 256 * 1024 + 37  # more points than the largest launch covers in one pass
FAMILIES = ("A", "B", "C1", "C2", "C3", "C4", "C5", "C6", "C7", "D1", "D2", "D3", "D4", "E1", "E2", "E3", "E4", "E5", "E6", "F")
A_SINGLE = (None, 1, 17, TILE - 1, TILE, TILE + 1, 1000)
A_NET = (None, 17, TILE + 1)
A_DETS = (1, 3, 8)
B_GRIDS = (17, TILE + 1, 1000)
B_WAYS = ("T1", "counts", "weights")
B_POINT = 20              # the one live point of the "weights" way
C1_STORES = ((2, 0), (2, 1), (3, 0), (4, 0), (4, 2), (5, 0))  # (dh_ld, floats d_h starts into its allocation)
D2_DTAU = 2.0 ** -17      # 65536 shifts span half a second: no two grid times alias at frequencies 20 .. 512 Hz
D2_STARS = (MAX_TAU - 1, MAX_TAU - TILE, TILE - 1, TILE)
D4_FMAX, D4_TAU = 4096.0, 0.5
E4_AMP = dict(quiet=1.1, loud=3.25)  # factors that put lnl_marg of task 0's live rows near -2 and near +50 (held by the host test)


def ups_of(kind, Rn, Bn, seed):
    """``loglike_grad_reference.upstream`` plus the kind "max_mix" (d_max_mix alone)."""
    if kind == "max_mix":
        full = G.upstream("all", Rn, Bn, seed)
        return {k: (v if k == "d_max_mix" else None) for k, v in full.items()}
    return G.upstream(kind, Rn, Bn, seed)


def _fac(net, kinds, clear=None, j_star=None, **more):
    reach_max = any(k in ("max", "all", "max_mix") for k in kinds)
    return dict(net=net, kinds=tuple(kinds), clear=reach_max if clear is None else clear, j_star=j_star, **more)


def _args(case):
    return RN.call_args(case) if "response" in case else R1.call_args(case)


def plant(case, j_star):
    """Single stream, n_z = 1: the data become the prediction shifted to grid index ``j_star`` and rotated by PHI0, with whatever
    ``freqs`` and ``taus`` the case holds now (``build`` plants before a case is edited)."""
    h, taus = case["h"].double(), case["taus"]
    f = case["freqs"].double().expand(B, h.shape[1])
    ang = h[..., 1] + TWO_PI * f * (taus[0] + j_star * taus[1]) + R1.PHI0
    case["data"] = torch.stack([h[..., 0] * torch.cos(ang), h[..., 0] * torch.sin(ang)], -1).float()
    case["j_star"] = j_star
    return case


def scale_x_star(case, target):
    """Single stream, n_z = 1: the data of task b times target / x*_b.  The rounding of the data to fp32 moves x* by 2^-24 relative
    at most."""
    x = R1.reference(**R1.call_args(case))["x"].max(1).values
    case["data"] = (case["data"].double() * (target / x).view(B, 1, 1)).float()
    return case


def pow2(args, k):
    """A and d times 2^-k, w times 2^2k: every likelihood keeps its bits, dphi too, dA is multiplied by 2^k."""
    out = dict(args, data=args["data"] * 2.0 ** -k, weights=args["weights"] * 2.0 ** (2 * k), h=args["h"].clone())
    out["h"][..., 0] *= 2.0 ** -k
    return out


def net_pow2(args, k, what):
    """C_k times 2^k and, ``what`` == "data": the data times 2^-k (K_j keeps its bits, HH does not: it is multiplied by 4^k, so
    the likelihoods change); ``what`` == "template": A times 2^-k (C_k h keeps its value: K_j, HH and every likelihood keep their
    bits, dphi too, dA is multiplied by 2^k)."""
    out = dict(args, response=args["response"] * 2.0 ** k)
    if what == "data":
        out["data"] = args["data"] * 2.0 ** -k
    else:
        out["h"] = args["h"].clone()
        out["h"][..., 0] *= 2.0 ** -k
    return out


# ---- A: the coefficients --------------------------------------------------------------------------------------------------------------
def _family_a():
    out = []
    for i, n_tau in enumerate(A_SINGLE):
        kw = dict(wform=(None, "T", "BT")[i % 3], fform=("T", "BT")[i % 2], counts=(None, (T, 17, 0))[i % 2], h_ld=(2, 4)[i % 2])
        case = R1.build("noise", T, n_z=3, taus=R1.grid(n_tau), seed=300 + i, x_s=X_S, **kw)
        out.append((f"A single n_tau={n_tau}", _fac(False, (), n_tau=n_tau, c_off=2 if n_tau is None else 4, **kw), _args(case)))
    i = 0
    for D in A_DETS:
        for delays in (True, False):
            for n_tau in A_NET:
                kw = dict(wform=(None, "T", "BT")[i % 3], fform=("T", "BT")[i % 2], counts=(None, (T, 17, 0))[(i // 2) % 2], h_ld=(2, 4)[i % 2])
                case = RN.build("noise", T, D=D, n_z=3, taus=RN.grid(n_tau), seed=320 + i, x_s=X_S, **kw)
                if not delays:
                    case["delays"] = None
                out.append((f"A network D={D} delays={delays} n_tau={n_tau}",
                            _fac(True, (), n_tau=n_tau, D=D, delays=delays, c_off=2 + 2 * D, **kw), _args(case)))
                i += 1
    return out


# ---- B: one live point per task -------------------------------------------------------------------------------------------------------
def _family_b():
    out = []
    i = 0
    for net in (False, True):
        for way in B_WAYS:
            for n_tau in B_GRIDS:
                Tn = 1 if way == "T1" else T
                kw = dict(n_z=3, h_ld=(2, 4)[i % 2], fform=("T", "BT")[i % 2], taus=R1.grid(n_tau), seed=340 + i, x_s=X_S,
                          wform=("T", "BT")[i % 2] if way == "weights" else None, counts=(1, 1, 1) if way == "counts" else None)
                case = RN.build("noise", Tn, D=2, **kw) if net else R1.build("noise", Tn, **kw)
                if net:
                    case["delays"] = None
                if way == "weights":
                    w = case["weights"].clone()
                    w[..., :B_POINT] = 0.0
                    w[..., B_POINT + 1:] = 0.0
                    case["weights"] = w
                out.append((f"B {'network D=2' if net else 'single'} {way} n_tau={n_tau}",
                            _fac(net, ("max", "all"), clear=False, way=way, n_tau=n_tau), _args(case)))
                i += 1
    return out


# ---- C: the network backward ----------------------------------------------------------------------------------------------------------
def _family_c(which):
    out = []
    if which == "C1":
        case = RN.build("removed", T, D=3, n_z=3, h_ld=4, wform="BT", fform="T", taus=RN.grid(JC + 1), counts=(T, 17, 0), seed=361, x_s=X_S)
        assert case["delays"] is not None
        out.append(("C1 removed D=3 with delays", _fac(True, ("all",), D=3), _args(case)))
    if which == "C2":
        for i, (Tn, D) in enumerate((t, d) for t in (TILE - 1, TILE, TILE + 1) for d in (2, 8)):
            case = RN.build("noise", Tn, D=D, n_z=3, h_ld=(2, 4)[i % 2], wform=("BT", "T")[i % 2], fform=("BT", "T")[(i // 2) % 2],
                            taus=RN.grid(17), counts=(Tn, Tn - 1, 17), seed=362 + i, x_s=X_S)
            out.append((f"C2 T={Tn} D={D}", _fac(True, ("all",), D=D, T=Tn), _args(case)))
    if which == "C3":
        for i, n_tau in enumerate((TILE - 1, TILE, TILE + 1)):
            case = RN.build("noise", T, D=2, n_z=3, h_ld=(4, 2)[i % 2], wform=("T", "BT", None)[i], fform=("BT", "T")[i % 2],
                            taus=RN.grid(n_tau), counts=(T, 17, 0), seed=370 + i, x_s=X_S)
            out.append((f"C3 n_tau={n_tau}", _fac(True, ("all",), n_tau=n_tau), _args(case)))
        n_tau = 16 * TILE + 3
        case = RN.build("planted", T, D=2, n_z=1, h_ld=2, wform="T", fform="T", taus=RN.grid(n_tau), j_star=n_tau - 1, seed=373, x_s=X_S)
        out.append((f"C3 n_tau={n_tau} planted at the end", _fac(True, ("max", "all"), j_star=n_tau - 1, n_tau=n_tau), _args(case)))
    if which == "C4":
        t = torch.arange(T).view(1, T)
        for i, (D, wform) in enumerate((d, w) for d in (3, 8) for w in ("BT", "T")):
            case = RN.build("noise", T, D=D, n_z=3, h_ld=(4, 2)[i % 2], wform=wform, fform="BT", taus=RN.grid(17), seed=380 + i, x_s=X_S)
            assert case["delays"] is not None
            live = (t % D == torch.arange(D).view(D, 1)) & (t % 7 != 0)  # [D, T]: point t for detector t mod D only, every 7th for none
            w = case["weights"]
            removed = torch.where(torch.arange(D) % 2 == 1, math.inf, 0.0).view(D, 1).expand(D, T)  # odd detectors: inf
            case["weights"] = torch.where(live.expand_as(w), w, removed.expand_as(w).to(w.dtype))
            case["kill"] = (~live).expand(B, D, T).clone()
            RN.poison(case, math.nan)
            out.append((f"C4 D={D} weights {wform}", _fac(True, ("all",), D=D, wform=wform, live=live), _args(case)))
    if which == "C5":
        case = RN.build("noise", T, D=3, n_z=3, h_ld=4, wform="T", fform="T", taus=RN.grid(17), seed=390, x_s=X_S)
        case["response"][1] = 0.0
        out.append(("C5 no response in task 1", _fac(True, ("all",), dead_task=1), _args(case)))
    if which == "C6":
        case = RN.build("noise", T, D=2, n_z=3, h_ld=2, wform="BT", fform="T", taus=RN.grid(17), seed=391, x_s=X_S)
        out.append(("C6 base", _fac(True, ("all",), ks=(20, -20)), _args(case)))
    if which == "C7":
        case = RN.build("noise", LONG_T, D=2, n_z=1, h_ld=2, wform="T", fform="T", taus=RN.grid(1), counts=(LONG_T, TILE * 1024 + 1, TILE * 1024),
                        seed=392, x_s=X_S)
        out.append((f"C7 T={LONG_T}", _fac(True, ("all",), T=LONG_T), _args(case)))
    return out


# ---- D: grid limits of the single stream ----------------------------------------------------------------------------------------------
def _family_d(which):
    out = []
    if which == "D1":
        for i, n_tau in enumerate((4095, 4096, 4097)):
            case = R1.build("noise", T, n_z=1, h_ld=(2, 4)[i % 2], wform=("T", None, "BT")[i], fform="BT", taus=R1.grid(n_tau), seed=400 + i,
                            x_s=X_S)
            out.append((f"D1 n_tau={n_tau}", _fac(False, ("marg", "all"), n_tau=n_tau), _args(case)))
    if which == "D2":
        for i, j_star in enumerate(D2_STARS):
            # (per-task frequencies with their scatter: five evenly spaced ones repeat |kappa| every 1 / 123 s)
            case = R1.build("planted", 5, n_z=1, h_ld=2, wform=(None, "T")[i % 2], fform="BT", taus=(-2 * D2_DTAU, D2_DTAU, MAX_TAU),
                            j_star=j_star, seed=410 + i, x_s=X_S)
            out.append((f"D2 n_tau={MAX_TAU} j*={j_star}", _fac(False, ("max", "all"), j_star=j_star, n_tau=MAX_TAU), _args(case)))
    if which == "D3":
        i = 0
        for n_tau in (17, TILE + 1):
            for zero_at in (n_tau // 2, n_tau - 1):  # tau0 = -(n / 2) dtau and -(n - 1) dtau
                for j_star in sorted({0, zero_at, n_tau - 1}):
                    case = R1.build("planted", T, n_z=1, h_ld=(2, 4)[i % 2], wform=(None, "T", "BT")[i % 3], fform=("T", "BT")[i % 2],
                                    taus=(-zero_at * DTAU, DTAU, n_tau), j_star=j_star, seed=420 + i, x_s=X_S)
                    out.append((f"D3 n_tau={n_tau} tau=0 at {zero_at} j*={j_star}",
                                _fac(False, ("max", "all"), j_star=j_star, n_tau=n_tau, zero_at=zero_at), _args(case)))
                    i += 1
    if which == "D4":
        n_tau = TILE + 1
        case = R1.build("noise", T, n_z=1, h_ld=2, wform="T", fform="T", taus=(-D4_TAU, 2 * D4_TAU / (n_tau - 1), n_tau), seed=440, x_s=X_S)
        case["freqs"] = torch.linspace(20.0, D4_FMAX, T)
        plant(case, 200)
        out.append((f"D4 f <= {D4_FMAX} Hz, |tau| <= {D4_TAU} s", _fac(False, ("marg", "max", "all"), j_star=200, n_tau=n_tau), _args(case)))
    return out


# ---- E: values ------------------------------------------------------------------------------------------------------------------------
def _family_e(which):
    out = []
    if which == "E1":
        for side, rel in (("below", -5e-7), ("above", 5e-7)):
            case = scale_x_star(R1.build("planted", T, n_z=1, h_ld=2, wform="T", fform=None, taus=None, seed=450, x_s=X_S), X_S * (1.0 + rel))
            out.append((f"E1 x* just {side} the switch, no grid", _fac(False, ("marg",), side=side), _args(case)))
        case = scale_x_star(R1.build("planted", T, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(17), j_star=2, seed=451, x_s=X_S),
                            X_S * 1.02)
        out.append(("E1 candidates on both sides of the switch", _fac(False, ("marg",), side="straddle", j_star=2), _args(case)))
    if which == "E2":
        for i, (x_star, k) in enumerate(((1e6, 10.0), (1e8, 100.0))):  # the loud regime (x* = 1e4) with A and d times k
            case = R1.build("loud", T, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(17), j_star=2, seed=455 + i, x_s=X_S)
            case["h"][..., 0] *= k
            case["data"] = case["data"] * k
            out.append((f"E2 x* = {x_star:g}", _fac(False, ("marg", "max"), j_star=2, x_star=x_star), _args(case)))
    if which == "E3":
        case = R1.build("noise", T, n_z=3, h_ld=4, wform="BT", fform="T", taus=R1.grid(17), seed=460, x_s=X_S)
        out.append(("E3 base", _fac(False, ("all",)), _args(case)))
    if which == "E4":
        for kind, regime in (("quiet", "noise"), ("loud", "planted")):
            case = R1.build(regime, T, n_z=3, h_ld=2, wform="T", fform="T", taus=R1.grid(17), j_star=2, seed=465, x_s=X_S)
            amp = case["h"].view(3, B, T, 2)[..., 0]
            amp *= E4_AMP[kind]
            if kind == "loud":  # (planted: x* = hh, so template and data grow together)
                case["data"] = case["data"] * E4_AMP[kind]
            amp[1] *= 1.01  # (the planted regime repeats one waveform: the samples differ in amplitude)
            amp[2] *= 0.97
            amp[1, 0] = 0.0  # sample 1 of task 0: hh == 0, Lambda = 1
            out.append((f"E4 {kind} mixture with a degenerate sample", _fac(False, ("mix", "max_mix"), kind=kind, dead_row=1 * B + 0), _args(case)))
    if which == "E5":
        case = R1.build("noise", T, n_z=1, h_ld=4, wform="BT", fform="BT", taus=R1.grid(17), seed=470, x_s=X_S)
        out.append(("E5 n_z = 1", _fac(False, ("mix", "marg")), _args(case)))
    if which == "E6":
        case = R1.build("noise", T, n_z=3, h_ld=2, wform="T", fform="T", taus=R1.grid(17), seed=471, x_s=X_S)
        out.append(("E6 base", _fac(False, ("all",), ks=(-20, 20, 40)), _args(case)))
    return out


# ---- F: workspace reuse ---------------------------------------------------------------------------------------------------------------
def _family_f():
    out = []
    for net in (False, True):
        build = (lambda *a, **k: RN.build(*a, D=2, **k)) if net else R1.build  # noqa: E731
        x = build("noise", T, n_z=1, h_ld=2, wform="T", fform="T", taus=R1.grid(17), seed=480, x_s=X_S)
        y = build("noise", T, n_z=3, h_ld=4, wform="BT", fform="BT", taus=R1.grid(TILE + 1), seed=481, x_s=X_S)
        for name, case in (("X", x), ("Y", y)):
            out.append((f"F {'network' if net else 'single'} {name}", _fac(net, ("all",), role=name), _args(case)))
    return out


def cases(family):
    """[(tag, factors, args)] of one family (``FAMILIES``); ``args`` are the keyword arguments of the public call, fp32 CPU tensors."""
    if family == "A":
        return _family_a()
    if family == "B":
        return _family_b()
    if family == "F":
        return _family_f()
    assert family in FAMILIES, family
    return _family_c(family) if family[0] == "C" else _family_d(family) if family[0] == "D" else _family_e(family)
