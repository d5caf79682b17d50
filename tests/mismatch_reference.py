"""float64 reference of the gradient of the waveform match (``npf_waveform_match_bwd``) and what its tests share.

``match_of`` is the definition of include/npf_hip.h in float64 torch WITH autograd (``match_reference._terms`` detaches, so this is
its differentiable twin): removed and padded points are selected out with ``torch.where`` before anything is multiplied, so a NaN
there reaches neither the value nor the gradient.  ``closed_form`` is the gradient the kernel evaluates,
    dM/dA_t = w_t (A'_t cos(theta_t - psi) / N - M A_t / hh),    dM/dphi_t = -w_t A_t A'_t sin(theta_t - psi) / N,
at the index ``match_reference.reference`` finds, with the scale ``s_t = w_t (|A'_t| / N + M |A_t| / hh)`` of its gate;
tests/test_mismatch_host.py checks it against autograd of ``match_of`` and a central finite difference.  ``cases`` is the subset of
``match_reference.cases`` the GPU test uses plus a T = 1 case, ``gate_ratio`` the gate
    |d - ref| <= 2^-23 |ref| + 1e-9 |d_match| / n_bcast * s_t
per element: the forward's own gate shape.  2^-23 is one fp32 rounding with a factor 2; the absolute term covers the cancellation of
the two dA terms, whose double evaluation errs by some 1e-13 of s_t (sums of T <= 200 terms, ulp-level sines) -- four orders of
margin, while row scalars rounded to fp32 (6e-8 of s_t) fail it."""
import math

import torch

import match_reference as R

N_TAUS = lambda jc: (None, 1, jc, jc + 1, 257)  # noqa: E731


def _live(weights, n_valid, Bn, T):
    w = torch.ones(Bn, T, dtype=torch.float64) if weights is None else weights.detach().cpu().double().expand(Bn, T)
    nv = torch.full((Bn,), T) if n_valid is None else n_valid.detach().cpu().long().clamp(0, T)
    live = (w > 0) & torch.isfinite(w) & (torch.arange(T).view(1, T) < nv.view(Bn, 1))
    return torch.where(live, w, torch.zeros_like(w)), live


def match_of(h, g, weights=None, freqs=None, taus=None, n_valid=None, tau_index=None):
    """match [R] of the float64 tensor ``h`` [R, T, >= 2] (autograd flows into it), maximised over the grid -- or, with ``tau_index``
    [R], evaluated at those grid indices.  Degenerate rows: 0."""
    g = g.detach().cpu().double()
    Rn, T, Bn = h.shape[0], h.shape[1], g.shape[0]
    task = torch.arange(Rn) % Bn
    w, live = _live(weights, n_valid, Bn, T)
    w, live, g = w[task], live[task], g[task]
    zero = torch.zeros(Rn, T, dtype=torch.float64)
    A, ph = torch.where(live, h[..., 0], zero), torch.where(live, h[..., 1], zero)
    Ag, phg = torch.where(live, g[..., 0], zero), torch.where(live, g[..., 1], zero)
    a, theta = w * A * Ag, ph - phg
    hh, gg = (w * A * A).sum(1), (w * Ag * Ag).sum(1)
    if taus is None:
        c = (a * torch.exp(1j * theta)).sum(1).view(Rn, 1)
    else:
        f = torch.where(live, freqs.detach().cpu().double().expand(Bn, T)[task], zero)
        if tau_index is not None:
            tau = (taus[0] + tau_index.double() * taus[1]).view(Rn, 1, 1)
        else:
            tau = (taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]).view(1, 1, -1)
        c = (a.unsqueeze(2) * torch.exp(1j * (theta.unsqueeze(2) + R.TWO_PI * f.unsqueeze(2) * tau))).sum(1)
    prod = hh * gg
    deg = prod == 0
    mag = torch.where(deg.view(-1, 1), torch.zeros_like(c.real), c.abs() / torch.where(deg, torch.ones_like(prod), prod).sqrt().view(-1, 1))
    return mag.max(1).values


def closed_form(h, g, weights=None, freqs=None, taus=None, n_valid=None, ref=None, fp32_scalars=False):
    """(dM/dh [R, T, 2], s [R, T]) in float64 from the formulae, at ``ref["tau_index"]`` (``ref``: ``match_reference.reference`` of
    the same inputs; computed when not given).  Zeros at removed and padded points and in degenerate rows.  ``fp32_scalars``: start
    from the row scalars the forward rounds to fp32 -- match, phase, hh and sqrt(hh gg) -- to show what that would cost."""
    ref = ref if ref is not None else R.reference(h, g, weights, freqs, taus, n_valid)
    h, g = h.detach().cpu().double(), g.detach().cpu().double()
    Rn, T, Bn = h.shape[0], h.shape[1], g.shape[0]
    task = torch.arange(Rn) % Bn
    w, live = _live(weights, n_valid, Bn, T)
    w, live, g = w[task], live[task], g[task]
    zero = torch.zeros(Rn, T, dtype=torch.float64)
    A, ph = torch.where(live, h[..., 0], zero), torch.where(live, h[..., 1], zero)
    Ag, phg = torch.where(live, g[..., 0], zero), torch.where(live, g[..., 1], zero)
    theta = ph - phg
    if taus is not None:
        f = torch.where(live, freqs.detach().cpu().double().expand(Bn, T)[task], zero)
        theta = theta + R.TWO_PI * f * (taus[0] + ref["tau_index"].double() * taus[1]).view(Rn, 1)
    hh, gg = (w * A * A).sum(1), (w * Ag * Ag).sum(1)
    c = (w * A * Ag * torch.exp(1j * theta)).sum(1)
    deg = ref["degenerate"]
    one = torch.ones_like(hh)
    N, hh_ = torch.where(deg, one, (hh * gg).sqrt()).view(Rn, 1), torch.where(deg, one, hh).view(Rn, 1)
    M, psi = (c.abs().view(Rn, 1) / N), torch.atan2(c.imag, c.real).view(Rn, 1)
    if fp32_scalars:
        M, psi, N, hh_ = (x.float().double() for x in (M, psi, N, hh_))
    dA = w * (Ag * torch.cos(theta - psi) / N - M * A / hh_)
    dphi = -w * A * Ag * torch.sin(theta - psi) / N
    s = w * (Ag.abs() / N + M * A.abs() / hh_)
    keep = live & ~deg.view(Rn, 1)
    return torch.stack([torch.where(keep, dA, zero), torch.where(keep, dphi, zero)], -1), torch.where(keep, s, zero)


def expected(case, d_match, n_bcast=1, ref=None):
    """(d_h reference [R, T, 2] for the incoming gradient ``d_match`` [R] of the match, gate scale [R, T], ref)."""
    ref = ref if ref is not None else R.reference(**R.call_args(case))
    dM, s = closed_form(**R.call_args(case), ref=ref)
    k = d_match.detach().cpu().double().view(-1, 1) / n_bcast
    return dM * k.unsqueeze(-1), s * k.abs(), ref


def gate_ratio(got, want, s):
    """Worst |got - want| / (2^-23 |want| + 1e-9 s) over the elements of [R, T, 2] (0 / 0 of an exact zero counts as inside)."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    d = (got - want).abs()
    gate = 2.0 ** -23 * want.abs() + 1e-9 * s.unsqueeze(-1)
    q = torch.where(d == 0, torch.zeros_like(d), d / gate)
    q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
    return float(q.max()) if q.numel() else 0.0


def t1_case():
    """T = 1: one point per task and a grid of one shift away from 0.  M = 1 whatever the point holds (|c| = a = N), so the two dA
    terms cancel completely and dphi = 0: what is left is the rounding the gate's absolute term allows."""
    case = R.build("random", 1, n_z=3, h_ld=4, wform="BT", fform="BT", taus=(3 * R.DTAU, R.DTAU, 1), seed=77)
    return ("random T=1 n_tau=1", dict(regime="random", T=1, n_tau=1, n_z=3, h_ld=4, counts=None, wform="BT", fform="BT"), case)


def cases(jc):
    """``match_reference.cases(jc)`` restricted to n_tau in {none, 1, jc, jc + 1, 257} -- every regime at T in {37, 200}, n_z in
    {1, 3}, h_ld in {2, 4}, counts (T, 17, 0) or none -- plus the T = 1 case.  -> list of (tag, factors, case)."""
    return [c for c in R.cases(jc) if c[1]["n_tau"] in N_TAUS(jc)] + [t1_case()]


# ---- the start of the Trainer test --------------------------------------------------------------------------------------------------
TRAIN_CASE = dict(kind="AttnCNP", r=64, L_xy=2, L_dec=2, dx=1, dy=2, B=8, C=20, T=50)
TRAIN_SEED, TRAIN_LAM, TRAIN_LR, TRAIN_STEPS = 2, 10.0, 1e-3, 20


def train_setup():
    """(batch on the CPU, freqs [B, T] in Hz, taus) of the Trainer test: one synthetic batch, its inputs x in [-1, 1] mapped to
    20 .. 512 Hz, and a grid of 17 shifts."""
    from npf_gwwaveform_amd.train import synthetic_waveform_batch

    batch = synthetic_waveform_batch(TRAIN_CASE["B"], TRAIN_CASE["C"], TRAIN_CASE["T"], 500, "cpu")
    return batch, (266.0 + 246.0 * batch["X_trgt"][..., 0]).contiguous(), R.grid(17)


def oracle_trajectory(seed=TRAIN_SEED, steps=TRAIN_STEPS):
    """[(NLL, mean mismatch)] before each of ``steps`` Adam steps and after the last, of ``CNPFLoss + lam * mismatch`` on the CPU
    oracle with the float64 definition of the match: what the Trainer test's run is expected to do, from the same parameters."""
    import specs
    from oracle import npf_oracle as O

    cfg = specs.cfg_of(TRAIN_CASE)
    batch, freqs, taus = train_setup()
    params = {k: v.clone().requires_grad_() for k, v in specs.make_params(TRAIN_CASE, seed=seed).items()}
    opt = torch.optim.Adam(list(params.values()), lr=TRAIN_LR)
    traj = []
    for step in range(steps + 1):
        out = O.forward(cfg, params, batch["X_cntxt"], batch["Y_cntxt"], batch["X_trgt"], batch["Y_trgt"])
        loc = out["loc"].reshape(TRAIN_CASE["B"], TRAIN_CASE["T"], 2)
        mm = (1.0 - match_of(loc.double(), batch["Y_trgt"], None, freqs, taus)).mean()
        nll = O.cnpf_loss(out, batch["Y_trgt"])
        traj.append((float(nll.detach()), float(mm.detach())))
        if step < steps:
            opt.zero_grad()
            (nll + TRAIN_LAM * mm.float()).backward()
            opt.step()
    return traj
