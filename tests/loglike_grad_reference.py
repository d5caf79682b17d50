"""float64 reference of the gradient of the matched-filter likelihoods (``npf_waveform_loglike_bwd`` / ``npf_waveform_loglike_net_bwd``)
and what its tests share.

Both likelihoods are written as a network of D detectors (the single stream: D = 1, C = 1, no delay), on the per-detector terms of
``loglike_reference._terms``.  With x_j = |K_j|, u_j = K_j / x_j (0 where x_j == 0), p_j = softmax_j ln I0(x_j), rho = I1 / I0:
    q_j = p_j rho(x_j) conj(u_j)
    G_t = g_marg sum_j q_j e^{i 2 pi f_t tau_j} + g_max conj(u_{j*}) e^{i 2 pi f_t tau_{j*}}
    E_{k,t} = C_k conj(d_{k,t}) e^{i (phi_t + 2 pi f_t delay_k)}
    dF/dA_t = sum_k w_{k,t} (Re(E_{k,t} G_t) - (g_marg + g_max) |C_k|^2 A_t),    dF/dphi_t = -sum_k w_{k,t} A_t Im(E_{k,t} G_t)
with g_marg[r] = d_marg[r] + d_mix[b] exp(lnl_marg[r] - lnl_mix[b]) / n_z and g_max likewise.  ``closed_form`` evaluates this with
direct sines and exactly rounded sums over t and j (``math.fsum``); ``recurrence`` forms K_j and G_t the way the kernels do -- chunks
of ``jc`` shifts, one direct sine / cosine pair per chunk, z <- z s inside, the kernels' ln I0 and I1 / I0 schemes.  Both return a
``Parts`` object; ``grad_of`` turns it into (d_h [R, T, 2], S [R, T]) for one set of upstream gradients, which is linear and cheap, so
the tests evaluate every upstream combination on one ``Parts``.  tests/test_loglike_grad_host.py checks ``closed_form`` against
central differences of the definition in 50-digit arithmetic.  ``saved_reference`` is the row of coefficients the forward keeps for the
backward (``waveform_loglike_coef_kernel``), with its own derived gate (``saved_gates``).

Gate per element (``gate_ratio``):  |d| <= 2^-23 (1 + 2^-20) |ref| + (1e-10 S_r + 1e-12) S_{r,t},  S_r = ``loglike_reference.scale_of``,
S_{r,t} = (|g_marg| + |g_max|) sum_k |C_k| w_{k,t} (|d_{k,t}| + |A_t|) max(1, |A_t|).  The first term is the one fp32 rounding of the
output; a relative error of p_j is an absolute error of L_j, which the forward suites gate at 1e-10 S_r + 1e-12; the rest is double
sums of at most n + T terms.  One fp32 rounding is relative only down to 2^-126: below it the format's spacing is 2^-149 whatever the
value, so ``gate_ratio`` adds that one spacing (``FP32_FLOOR``).  It is reached where a mixture hands a row the weight
exp(lnl_marg - lnl_mix) of e^-87 or less -- the "loud" regime with the mixture's gradient alone -- and is no allowance anywhere else."""
import math
from typing import NamedTuple

import torch
from scipy import special

import loglike_net_reference as RN
import loglike_reference as R1

TWO_PI = R1.TWO_PI
B = R1.B
ONE_ROUNDING = 2.0 ** -23 * (1.0 + 2.0 ** -20)
FP32_FLOOR = 2.0 ** -149  # the spacing of fp32 below 2^-126: what one rounding costs there
N_TAUS = lambda jc: (None, 1, jc, jc + 1, 257)  # noqa: E731
UPSTREAMS = ("marg", "max", "mix", "all")
POWER_TERMS, ASYM_TERMS = 48, 16


# ---- I1 / I0 ------------------------------------------------------------------------------------------------------------------------
def rho_scheme(x, x_s=24.0, terms=ASYM_TERMS):
    """The kernel's I1 / I0 of one host float: below ``x_s`` (x / 2) S1 / S0 with the two power series in x^2 / 4 (the stopping rule
    and the cap of ``loglike_reference.log_i0_scheme``), from there on the ratio of the two ``terms``-term series in 1 / (8 x)."""
    if x < x_s:
        q = 0.25 * x * x
        t0 = t1 = s0 = s1 = 1.0
        for k in range(1, POWER_TERMS + 1):
            t0 *= q * (1.0 / float(k * k))
            t1 *= q * (1.0 / float(k * (k + 1)))
            s0 += t0
            s1 += t1
            if t0 <= s0 * 2.0 ** -60:
                break
        return (0.5 * x) * (s1 / s0)
    u, a0, a1 = 0.125 / x, 0.0, 0.0
    for k in range(terms, 0, -1):
        a0 = u * (float((2 * k - 1) ** 2) / float(k)) * (1.0 + a0)
        a1 = u * (float((2 * k - 1) ** 2 - 4) / float(k)) * (1.0 + a1)
    return (1.0 + a1) / (1.0 + a0)


def rho(x):
    """I1 / I0 of a float64 tensor, x >= 0, from scipy's exponentially scaled functions (no overflow; rho(0) = 0)."""
    v = x.double().numpy()
    return torch.from_numpy(special.i1e(v) / special.i0e(v)).reshape(x.shape)


# ---- the parts ----------------------------------------------------------------------------------------------------------------------
class Parts(NamedTuple):
    Qm: torch.Tensor    # [R, T] complex: sum_j q_j e^{i 2 pi f_t tau_j}
    Mx: torch.Tensor    # [R, T] complex: conj(u_{j*}) e^{i 2 pi f_t tau_{j*}}
    Ew: list            # per detector [R, T] complex: w_k C_k conj(d_k) e^{i (phi + 2 pi f delay_k)} (0 where not live)
    wc2: list           # per detector [R, T]: w_k |C_k|^2
    s_k: torch.Tensor   # [R, T]: sum_k |C_k| w_k (|d_k| + |A|) max(1, |A|)
    A: torch.Tensor     # [R, T] (0 where no detector is live)
    ref: dict           # loglike_reference._finish of (K, HH, DD), plus "K"
    Bn: int


def _fsum_last(x):
    """Exactly rounded sum over the last axis of a real float64 tensor."""
    flat = x.reshape(-1, x.shape[-1]).tolist()
    return torch.tensor([math.fsum(row) for row in flat], dtype=torch.float64).reshape(x.shape[:-1])


def _csum_last(z):
    return torch.complex(_fsum_last(z.real), _fsum_last(z.imag))


def _detectors(args):
    """Per detector (c, phi, hh, dd, f, C, delay, w conj(d), w) of ``loglike_net_reference._per_detector``; the single stream is one
    detector with C = 1 and no delay."""
    h = args["h"].detach().cpu()
    if "response" in args:
        data, resp, dl, w = args["data"], args["response"], args["delays"], args["weights"]
    else:
        data, w = args["data"].unsqueeze(1), args["weights"]
        resp = torch.zeros(data.shape[0], 1, 2, dtype=torch.float64)
        resp[..., 0] = 1.0
        dl = None
        w = None if w is None else w.unsqueeze(w.dim() - 1)  # [T] -> [1, T], [B, T] -> [B, 1, T]
    f, nv = args["freqs"], args["n_valid"]
    h1 = h.clone()
    h1[..., 0] = 1.0
    ones = torch.zeros_like(data)
    ones[..., 0] = 1.0
    full = RN._per_detector(h, data, resp, dl, w, f, nv)
    wd = RN._per_detector(h1, data, resp, dl, w, f, nv)     # c = w conj(d)
    wo = RN._per_detector(h1, ones, resp, dl, w, f, nv)     # c = w
    return [t + (a[0], b[0].real) for t, a, b in zip(full, wd, wo)], data.shape[0]


def _grid(taus):
    return torch.zeros(1, dtype=torch.float64) if taus is None else taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]


def _amplitude(h, dets):
    live_any = torch.stack([d[8] > 0 for d in dets]).any(0)
    return torch.where(live_any, h.detach().cpu().double()[..., 0], torch.zeros_like(dets[0][8]))


def _assemble(args, dets, Bn, K, Qm_of, p_rho, tau_index=None):
    """The parts from the network sums K [R, n]; ``Qm_of(q, f)`` sums q_j e^{i 2 pi f tau_j}, ``p_rho(x)`` gives p_j rho(x_j).
    ``tau_index`` (an int or [R]): the grid index the ``lnl_max`` direction Mx is taken at, in place of the reference's own
    maximiser -- what a near tie leaves open; the likelihoods stay those of the maximum.  ``ref`` also gets "q" [R, n] (q_j)."""
    taus = args["taus"]
    HH = RN._fsum_cols([(d[5].real ** 2 + d[5].imag ** 2) * d[2] for d in dets])
    DD = RN._fsum_cols([d[3] for d in dets])
    ref = R1._finish(K, HH, DD, Bn, taus)
    ref["K"] = K
    x = ref["x"]
    u = torch.where(x > 0, K / torch.where(x > 0, x, torch.ones_like(x)), torch.zeros_like(K))
    q = p_rho(x) * u.conj()
    q = torch.where(ref["degenerate"].view(-1, 1), torch.zeros_like(q), q)
    ref["q"] = q
    if tau_index is not None:
        forced = torch.as_tensor(tau_index, dtype=torch.long).expand(ref["tau_index"].shape)
        ref["tau_index"] = torch.where(ref["degenerate"], torch.zeros_like(forced), forced)
    f = dets[0][4]
    for d in dets[1:]:  # the frequency of a point that is live for any detector
        f = torch.where(f != 0, f, d[4])
    A = _amplitude(args["h"], dets)
    Qm = Qm_of(q, f)
    idx = ref["tau_index"].view(-1, 1)
    tau_star = _grid(taus)[idx[:, 0]].view(-1, 1)
    Mx = u.conj().gather(1, idx) * torch.exp(1j * TWO_PI * f * tau_star)
    Mx = torch.where(ref["degenerate"].view(-1, 1), torch.zeros_like(Mx), Mx)
    Ew = [d[5].view(-1, 1) * d[7] * torch.exp(1j * (d[1] + TWO_PI * d[4] * d[6].view(-1, 1))) for d in dets]
    wc2 = [d[8] * (d[5].real ** 2 + d[5].imag ** 2).view(-1, 1) for d in dets]
    s_k = sum(d[5].abs().view(-1, 1) * (d[7].abs() + d[8] * A.abs()) for d in dets) * A.abs().clamp(min=1.0)
    return Parts(Qm, Mx, Ew, wc2, s_k, A, ref, Bn)


def closed_form(args, tau_index=None):
    """``Parts`` of one input set (the keys of ``loglike_reference.call_args`` or ``loglike_net_reference.call_args``) with direct
    sines and exactly rounded sums (``tau_index``: see ``_assemble``)."""
    dets, Bn = _detectors(args)
    tau = _grid(args["taus"])
    K = None
    for c, phi, _, _, f, C, dl, _, _ in dets:  # ascending k
        arg = phi.unsqueeze(1) + TWO_PI * f.unsqueeze(1) * (tau.view(1, -1, 1) + dl.view(-1, 1, 1))  # [R, n, T]
        term = C.view(-1, 1) * _csum_last(c.unsqueeze(1) * torch.exp(1j * arg))
        K = term if K is None else K + term

    def Qm_of(q, f):
        return _csum_last(q.unsqueeze(1) * torch.exp(1j * TWO_PI * f.unsqueeze(2) * tau.view(1, 1, -1)))  # [R, T, n] -> [R, T]

    def p_rho(x):
        return torch.softmax(R1.log_i0(x), 1) * rho(x)

    return _assemble(args, dets, Bn, K, Qm_of, p_rho, tau_index)


def recurrence(args, jc=16, x_s=24.0):
    """``Parts`` formed in the kernels' order: K_j by ``loglike_net_reference._recur``, p_j and rho by the kernels' schemes, G_t in
    chunks of ``jc`` shifts with one direct sine / cosine pair per chunk and z <- z s inside."""
    dets, Bn = _detectors(args)
    taus = args["taus"]
    K = None
    for c, phi, _, _, f, C, dl, _, _ in dets:
        term = C.view(-1, 1) * RN._recur(c, phi, f, taus, dl, jc)
        K = term if K is None else K + term
    tau0, dtau, n = taus if taus is not None else (0.0, 0.0, 1)

    def Qm_of(q, f):
        om = TWO_PI * f
        ss, sc = torch.sin(om * dtau), torch.cos(om * dtau)
        Gr, Gi = torch.zeros_like(f), torch.zeros_like(f)
        for j0 in range(0, n, jc):
            a = om * (tau0 + j0 * dtau)
            zr, zi = torch.cos(a), torch.sin(a)
            for j in range(j0, min(j0 + jc, n)):
                qr, qi = q[:, j].real.view(-1, 1), q[:, j].imag.view(-1, 1)
                Gr, Gi = Gr + (qr * zr - qi * zi), Gi + (qr * zi + qi * zr)
                zr, zi = zr * sc - zi * ss, zr * ss + zi * sc
        return torch.complex(Gr, Gi)

    def p_rho(x):
        rows = []
        for row in x.tolist():
            li0 = [R1.log_i0_scheme(v, x_s) for v in row]
            top = R1.log_i0_scheme(max(row), x_s)
            e = [math.exp(v - top) for v in li0]
            total = sum(e)
            rows.append([ev / total * rho_scheme(v, x_s) for ev, v in zip(e, row)])
        return torch.tensor(rows, dtype=torch.float64)

    return _assemble(args, dets, Bn, K, Qm_of, p_rho)


# ---- the coefficients the forward keeps for the backward ------------------------------------------------------------------------------
def saved_reference(parts):
    """float64 [R, 4 + 2 n] of what ``waveform_loglike_coef_kernel`` writes: hh, Re / Im conj(u_{j*}), 0, (Re q_j, Im q_j) j < n;
    rows with hh == 0 are all zero."""
    ref = parts.ref
    K, x, q = ref["K"], ref["x"], ref["q"]
    idx = ref["tau_index"].view(-1, 1)
    kb, xb = K.gather(1, idx)[:, 0], x.gather(1, idx)[:, 0]
    ub = torch.where(xb > 0, kb / torch.where(xb > 0, xb, torch.ones_like(xb)), torch.zeros_like(kb)).conj()
    head = torch.stack([ref["hh"], ub.real, ub.imag, torch.zeros_like(xb)], 1)
    out = torch.cat([head, torch.view_as_real(q.resolve_conj()).reshape(q.shape[0], -1)], 1)
    return torch.where(ref["degenerate"].view(-1, 1), torch.zeros_like(out), out)


def saved_gates(parts):
    """(delta_K [R, n], gate of q [R, n]).  q_j = p_j rho(x_j) conj(u_j): a relative error of p_j is an absolute error of L_j, which
    the forward suites gate at delta_L = 1e-10 S_r + 1e-12; ``loglike_reference.ratios`` gates series[j] = x_j / sqrt(hh) at 1e-10
    relative + 1e-12, which is delta_K_j = 1e-10 x_j + 1e-12 sqrt(hh) on K_j; d(rho u) = rho' dx u + rho du with rho' <= 1 / 2 and
    rho / x <= 1 / 2, so an absolute error of K_j is at most half of it on rho u; one rounding of the double that is stored:
        |dq_j| <= p_j (delta_L + delta_K_j / 2) + 2^-52 |q_j|."""
    ref = parts.ref
    x, q = ref["x"], ref["q"]
    deg = ref["degenerate"].view(-1, 1)
    p = torch.where(deg, torch.zeros_like(x), torch.softmax(R1.log_i0(x), 1))
    d_L = (1e-10 * R1.scale_of(ref) + 1e-12).view(-1, 1)
    d_K = 1e-10 * x + 1e-12 * ref["hh"].sqrt().view(-1, 1)
    return d_K, p * (d_L + 0.5 * d_K) + 2.0 ** -52 * q.abs()


def saved_ratio(got, parts):
    """Worst |q_j - reference| / gate over ``got`` [R, 4 + 2 n] (the coefficient columns only)."""
    want = saved_reference(parts)
    _, gate = saved_gates(parts)
    d = (got.detach().cpu().double() - want)[:, 4:].abs().view(want.shape[0], -1, 2)
    d = (d[..., 0] ** 2 + d[..., 1] ** 2).sqrt()
    r = torch.where(d == 0, torch.zeros_like(d), d / gate)
    r = torch.where(torch.isfinite(d), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


# ---- upstream gradients, the gradient, the gate -------------------------------------------------------------------------------------
def upstream(kind, Rn, Bn, seed):
    """dict(d_marg [R], d_max [R], d_mix [B], d_max_mix [B]) of float64 tensors or None: ``marg`` / ``max`` / ``mix`` only, or ``all``
    four at once with random signs."""
    g = torch.Generator().manual_seed(9100 + seed)
    draw = lambda n: torch.randn(n, generator=g, dtype=torch.float64)  # noqa: E731
    full = dict(d_marg=draw(Rn), d_max=draw(Rn), d_mix=draw(Bn), d_max_mix=draw(Bn))
    keep = dict(marg=("d_marg",), max=("d_max",), mix=("d_mix",), all=tuple(full))[kind]
    return {k: (v if k in keep else None) for k, v in full.items()}


def row_gradients(ref, ups, Bn, n_bcast=1):
    """(g_marg [R], g_max [R]) from the upstream gradients and the reference's likelihoods; 0 in degenerate rows."""
    Rn = ref["hh"].shape[0]
    n_z = Rn // Bn
    zero = torch.zeros(Rn, dtype=torch.float64)

    def total(d_row, d_task, rows, mix):
        g = zero.clone()
        if d_row is not None:
            g = g + d_row.double()
        if d_task is not None:
            g = g + d_task.double().repeat(n_z) * torch.exp(rows - mix.repeat(n_z)) / n_z
        return torch.where(ref["degenerate"], zero, g / n_bcast)

    return (total(ups.get("d_marg"), ups.get("d_mix"), ref["lnl_marg"], ref["lnl_mix"]),
            total(ups.get("d_max"), ups.get("d_max_mix"), ref["lnl_max"], ref["lnl_max_mix"]))


def grad_of(parts, ups, n_bcast=1):
    """(d_h [R, T, 2], S [R, T]) in float64 for the upstream gradients ``ups``."""
    gm, gx = row_gradients(parts.ref, ups, parts.Bn, n_bcast)
    G = gm.view(-1, 1) * parts.Qm + gx.view(-1, 1) * parts.Mx
    gs = (gm + gx).view(-1, 1)
    dA = torch.zeros_like(parts.A)
    dphi = torch.zeros_like(parts.A)
    for Ew, wc2 in zip(parts.Ew, parts.wc2):  # ascending k
        EG = Ew * G
        dA = dA + (EG.real - gs * wc2 * parts.A)
        dphi = dphi - parts.A * EG.imag
    S = (gm.abs() + gx.abs()).view(-1, 1) * parts.s_k
    return torch.stack([dA, dphi], -1), S


def gate_ratio(got, want, S, ref):
    """Worst |got - want| / gate over the elements of [R, T, 2] (0 / 0 of an exact zero counts as inside); the gate of the module's
    docstring plus ``FP32_FLOOR``."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    d = (got - want).abs()
    gate = ONE_ROUNDING * want.abs() + ((1e-10 * R1.scale_of(ref) + 1e-12).view(-1, 1) * S).unsqueeze(-1) + FP32_FLOOR
    q = torch.where(d == 0, torch.zeros_like(d), d / gate)
    q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
    return float(q.max()) if q.numel() else 0.0


# ---- the cases of the GPU suite -----------------------------------------------------------------------------------------------------
def cases(jc, x_s):
    """``loglike_reference.cases`` restricted to n_tau in {none, 1, jc, jc + 1, 257}: every regime at T in {37, 200}, n_z in {1, 3},
    h_ld in {2, 4}, counts or none.  -> list of (tag, factors, args)."""
    return [(tag, fac, R1.call_args(case)) for tag, fac, case in R1.cases(jc, x_s) if fac["n_tau"] in N_TAUS(jc)]


def net_cases(jc, x_s):
    """The same of ``loglike_net_reference.cases`` restricted to T = 37 (D in {1, 2, 3, 8}, with and without delays -- a case without
    frequencies has none -- and one zero response per regime)."""
    return [(tag, fac, RN.call_args(case)) for tag, fac, case in RN.cases(jc, x_s) if fac["n_tau"] in N_TAUS(jc) and fac["T"] == 37]


def clear_maximum(ref, gates=1e3):
    """Whether the runner-up of max_j x_j lies at least ``gates`` forward gates (1e-10 S_r + 1e-12) below the best in every live row
    with more than one grid time: what makes the lnl_max gradient well posed."""
    x = ref["x"]
    if x.shape[1] < 2:
        return True
    live = ~ref["degenerate"]
    top = x[live].topk(2, dim=1).values
    return bool(((top[:, 0] - top[:, 1]) >= gates * (1e-10 * R1.scale_of(ref)[live] + 1e-12)).all())
