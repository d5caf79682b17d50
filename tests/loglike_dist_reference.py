"""float64 reference of the distance-marginalised likelihood (``npf_waveform_loglike_dist`` / ``npf_waveform_loglike_net_dist``), its
gates and the input cases its tests share.

``marginalise`` evaluates the definitions of include/npf_hip.h directly on what ``loglike_reference.reference`` /
``loglike_net_reference.reference`` return (their ``x`` [R, n], ``hh``, ``dd_rows``): ``ln I0(a_i x_j) - a_i^2 HH / 2`` for every
(row, scale, grid time) with ``loglike_reference.log_i0``, ``torch.logsumexp`` over j, then over i, dead scales masked.
``one_pass`` restates the kernel's form (``M_i``, ``S_i`` with terms <= 1, the shifted sums) in float64 torch.
``cases`` lists the inputs of the GPU test; tests/test_loglike_dist_host.py checks on the CPU that in every one of them the runner-up
of ``max_i u_i`` lies at least 1e3 gates below the best, so ``scale_index`` is well posed."""
import math

import torch

import loglike_net_reference as N
import loglike_reference as R1

B = R1.B
SC = 16  # NPF_DIST_SC
N_TAUS = (None, 1, 16, 17, 257)
N_AS = (1, 2, SC - 1, SC, SC + 1, 64, 65, 257, 300)
DIST_DOUBLES = ("lnl_dist", "scale_hat", "lnl_amp_max", "lnl_dist_mix")
NEG_INF = -math.inf


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _per_row(t, Bn, Rn):
    """[n_a] or [B, n_a] -> [R, n_a] float64 (row s B + b takes task b's)."""
    t = t.detach().cpu().double()
    return t.expand(Bn, t.shape[-1])[torch.arange(Rn) % Bn]


def live_mask(a, lp):
    return (a > 0) & torch.isfinite(a) & torch.isfinite(lp)


def evidence(ref, scales, log_prior):
    """u [R, n_a] (dead scales -inf), live [R, n_a], a, lp [R, n_a] from a parent reference."""
    Bn, Rn = ref["dd"].shape[0], ref["hh"].shape[0]
    a, lp = _per_row(scales, Bn, Rn), _per_row(log_prior, Bn, Rn)
    live = live_mask(a, lp)
    a0, lp0 = torch.where(live, a, torch.ones_like(a)), torch.where(live, lp, torch.zeros_like(lp))
    hh = ref["hh"]
    x = torch.where((hh == 0).view(-1, 1), torch.zeros_like(ref["x"]), ref["x"])  # HH == 0: x_j = 0
    n = x.shape[1]
    L = R1.log_i0(a0.unsqueeze(2) * x.unsqueeze(1)) - (0.5 * a0 ** 2 * hh.view(-1, 1)).unsqueeze(2)  # [R, n_a, n]
    u = lp0 + (torch.logsumexp(L, 2) - math.log(n))
    return torch.where(live, u, torch.full_like(u, NEG_INF)), live, a, lp


def _finish(u, ref):
    Bn = ref["dd"].shape[0]
    Rn, n_a = u.shape
    n_z = Rn // Bn
    neg = torch.full_like(u, NEG_INF)
    lnl_dist = torch.logsumexp(u, 1)  # (every u -inf: -inf)
    dead = u == NEG_INF
    post = torch.where(dead, neg, u - torch.where(torch.isfinite(lnl_dist), lnl_dist, torch.zeros_like(lnl_dist)).view(-1, 1))
    best = u.max(1).values
    idx = (u == best.view(-1, 1)).double().argmax(1)  # the smallest index at the maximum (no live scale: 0)
    hh, xb = ref["hh"], ref["x"].max(1).values
    deg = hh == 0
    one = torch.ones_like(hh)
    scale_hat = torch.where(deg, torch.zeros_like(hh), xb / torch.where(deg, one, hh))
    lnl_amp_max = torch.where(deg, torch.zeros_like(hh), xb * xb / (2.0 * torch.where(deg, one, hh)))
    mix = torch.logsumexp(lnl_dist.view(n_z, Bn), 0) - math.log(n_z)
    u_mix = torch.logsumexp(u.view(n_z, Bn, n_a), 0) - math.log(n_z)
    post_mix = torch.where(u_mix == NEG_INF, torch.full_like(u_mix, NEG_INF),
                           u_mix - torch.where(torch.isfinite(mix), mix, torch.zeros_like(mix)).view(-1, 1))
    return dict(u=u, lnl_dist=lnl_dist, post=post, scale_index=idx, scale_hat=scale_hat, lnl_amp_max=lnl_amp_max, lnl_dist_mix=mix,
                post_mix=post_mix)


def marginalise(ref, scales, log_prior):
    """Every new output in float64 on the CPU (dict, plus ``u`` [R, n_a], ``live`` [R, n_a] and the gate scale ``S`` [R])."""
    u, live, a, lp = evidence(ref, scales, log_prior)
    out = _finish(u, ref)
    hh, dd = ref["hh"], ref["dd_rows"]
    term = a * (hh * dd).sqrt().view(-1, 1) + 0.5 * a ** 2 * hh.view(-1, 1) + lp.abs()
    out.update(live=live, S=torch.where(live, term, torch.zeros_like(term)).max(1).values)
    return out


def one_pass(ref, scales, log_prior):
    """The kernel's form in float64 torch: x* first, M_i, S_i = sum_j exp(ln I0(a_i x_j) - ln I0(a_i x*)) with every term <= 1,
    u_i = M_i + (ln S_i - ln n); then (u_i - max) - ln sum for the posterior."""
    Bn, Rn = ref["dd"].shape[0], ref["hh"].shape[0]
    a, lp = _per_row(scales, Bn, Rn), _per_row(log_prior, Bn, Rn)
    live = live_mask(a, lp)
    a0, lp0 = torch.where(live, a, torch.ones_like(a)), torch.where(live, lp, torch.zeros_like(lp))
    hh = ref["hh"]
    x = torch.where((hh == 0).view(-1, 1), torch.zeros_like(ref["x"]), ref["x"])
    n = x.shape[1]
    xb = x.max(1).values
    l0 = R1.log_i0(a0 * xb.view(-1, 1))  # [R, n_a]
    terms = torch.exp(R1.log_i0(a0.unsqueeze(2) * x.unsqueeze(1)) - l0.unsqueeze(2))
    assert float(terms.max()) <= 1.0 + 1e-15
    M = lp0 + (l0 - a0 * a0 * (0.5 * hh).view(-1, 1))
    u = M + (torch.log(terms.sum(2)) - math.log(n))
    u = torch.where(live, u, torch.full_like(u, NEG_INF))
    best = u.max(1).values
    none = best == NEG_INF
    shift = torch.where(none, torch.zeros_like(best), best)
    total = torch.exp(u - shift.view(-1, 1)).sum(1)
    lnl = torch.where(none, best, best + torch.log(torch.where(none, torch.ones_like(total), total)))
    return dict(u=u, lnl_dist=lnl)


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, dist, lnl_gate=1e-10, lnl_floor=1e-12):
    """Worst error / gate per new quantity ``got`` holds.  S_r = max over live i of (a_i sqrt(HH DD) + a_i^2 HH / 2 + |ln pi_i|):
    lnl_dist |d| <= lnl_gate S_r + lnl_floor, lnl_dist_mix the same with the largest S_r of the task's rows; post, post_mix twice
    that; -inf entries must match exactly; scale_hat, lnl_amp_max 1e-10 relative + 1e-12; scale_index exact."""
    out = {}
    S = dist["S"]
    Bn = ref["dd"].shape[0]
    task_S = S.view(-1, Bn).max(0).values

    def put(name, x, r, gate):
        inf_x, inf_r = x == NEG_INF, r == NEG_INF
        if not torch.equal(inf_x, inf_r):
            out[name] = math.inf
            return
        d = torch.where(inf_r, torch.zeros_like(r), (x - torch.where(inf_r, torch.zeros_like(r), r)).abs())
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)
        q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
        out[name] = float(q.max()) if q.numel() else 0.0

    for name in ("lnl_dist", "lnl_dist_mix", "scale_hat", "lnl_amp_max", "scale_index", "post", "post_mix"):
        x = got.get(name)
        if x is None:
            continue
        x = x.detach().cpu()
        r = dist[name]
        if name == "scale_index":
            assert x.dtype == torch.int32
            out[name] = 0.0 if torch.equal(x.reshape(-1).long(), r.long()) else math.inf
            continue
        assert x.dtype == torch.float64, (name, x.dtype)
        x = x.reshape(r.shape)
        if name in ("scale_hat", "lnl_amp_max"):
            put(name, x, r, 1e-10 * r.abs() + 1e-12)
        elif name == "lnl_dist":
            put(name, x, r, lnl_gate * S + lnl_floor)
        elif name == "lnl_dist_mix":
            put(name, x, r, lnl_gate * task_S + lnl_floor)
        elif name == "post":
            put(name, x, r, (2.0 * (lnl_gate * S + lnl_floor)).view(-1, 1).expand_as(r))
        else:
            put(name, x, r, (2.0 * (lnl_gate * task_S + lnl_floor)).view(-1, 1).expand_as(r))
    return out


def runner_up_in_gates(dist):
    """Per row with a live scale: (best - runner-up of u_i) / (1e-10 S_r + 1e-12); rows with fewer than two live scales: inf."""
    u = dist["u"]
    if u.shape[1] < 2:
        return torch.full((u.shape[0],), math.inf, dtype=torch.float64)
    top = u.topk(2, dim=1).values
    gap = torch.where(top[:, 1] == NEG_INF, torch.full_like(top[:, 0], math.inf), top[:, 0] - top[:, 1])
    gap = torch.where(top[:, 0] == NEG_INF, torch.full_like(gap, math.inf), gap)
    return gap / (1e-10 * dist["S"] + 1e-12)


# ---- scale grids -------------------------------------------------------------------------------------------------------------------
def geometric(n_a, lo=-4.0, hi=4.0):
    """n_a scales 2^lo .. 2^hi, geometric (one point: 1), float64."""
    if n_a == 1:
        return torch.ones(1, dtype=torch.float64)
    return torch.exp2(lo + torch.arange(n_a, dtype=torch.float64) * ((hi - lo) / (n_a - 1)))


def volume_prior(scales, power=3.0):
    """ln of the mass a prior uniform in volume puts on the points of a geometric scale grid, normalised: d^2 dd with dd ~ d is
    a^-3 -- strictly monotone along the grid, so that where the data say nothing (the "quiet" regime) the prior decides alone."""
    lp = -power * torch.log(scales)
    return lp - torch.logsumexp(lp, -1, keepdim=True)


def scale_grid(n_a, sform, pform, kind="geo", poison=math.nan):
    """(scales, log_prior), float64 [n_a] ("A") or [B, n_a] ("BA": task b's grid is shifted by 2^(b / 10), its prior has the power
    3 + b / 2).  kind "dead" (n_a >= 12): scales 0, negative, NaN, +inf at indices 1, 3, 5, 7 and log_prior -inf, +inf, NaN at 2, 9,
    11; the other tensor holds ``poison`` there (1 in ``scales`` when poison is not NaN: a live value).  kind "alldead": no live scale."""
    a = geometric(n_a)
    s = torch.stack([a * 2.0 ** (b / 10.0) for b in range(B)]) if sform == "BA" else a
    p = torch.stack([volume_prior(a, 3.0 + 0.5 * b) for b in range(B)]) if pform == "BA" else volume_prior(a)
    if kind == "geo":
        return s, p
    s, p = s.clone(), p.clone()
    clean_scale = poison if math.isnan(poison) else 1.0
    if kind == "dead":
        assert n_a >= 12
        for i, v in ((1, 0.0), (3, -1.0), (5, math.nan), (7, math.inf)):
            s[..., i] = v
            p[..., i] = poison
        for i, v in ((2, NEG_INF), (9, math.inf), (11, math.nan)):
            p[..., i] = v
            s[..., i] = clean_scale
        return s, p
    assert kind == "alldead"
    kinds_s, kinds_p = (0.0, -1.0, math.nan, math.inf), (NEG_INF, math.inf, math.nan)
    for i in range(n_a):
        if i % 2 == 0:
            s[..., i], p[..., i] = kinds_s[(i // 2) % 4], poison
        else:
            p[..., i], s[..., i] = kinds_p[(i // 2) % 3], clean_scale
    return s, p


# The builders plant the data at the template's own amplitude (times 1, 1 / 0.6, ... per latent sample), so the likelihood peaks at
# a = 1: midway between two points of every geometric grid with an even n_a, where the two neighbours tie but for the prior.  The
# data of every case are scaled by this factor, which moves the peak off that symmetry.
DATA_SCALE = 1.13


# ---- cases -------------------------------------------------------------------------------------------------------------------------
# (regime, combo number) -> the factor of the cases that DATA_SCALE left with scale_index ill posed: the peak of one of their rows
# (the latent samples' amplitudes differ by fixed factors) fell midway between two grid points again, whatever the seed
# (tests/test_loglike_dist_host.py checks every case)
DATA_SCALE_OF = {("edge", 7): 1.31}


def cases(network, x_s=24.0):
    """The inputs of the GPU test, single stream or network: every regime of ``loglike_reference.build`` with nine combinations that
    walk n_a through (1, 2, SC - 1, SC, SC + 1, 64, 65, 257, 300) and rotate n_tau in (none, 1, 16, 17, 257) (shifted by the regime's
    number, so every regime meets every n_tau), T in (37, 200), n_z in (1, 3), counts none or (T, 17, 0), D in (1, 2, 3), and the
    forms [n_a] / [B, n_a] of scales and log_prior.  Combination 2 (n_a = SC - 1) and 7 (n_a = 257) carry the grid with dead entries,
    combination 1 (n_a = 2) of "noise" and "loud" the grid without a live scale.  -> list of (tag, factors, case, scales, log_prior)."""
    out = []
    M = N if network else R1
    for ri, regime in enumerate(R1.REGIMES):
        for i, n_a in enumerate(N_AS):
            n_tau = N_TAUS[(i + ri) % 5]
            T = (37, 200)[i % 2]
            need_w = regime in ("removed", "degenerate")
            fform = (None, "T", "BT")[(i + ri) % 3]
            if fform is None and (n_tau is not None):
                fform = ("T", "BT")[i % 2]
            fac = dict(counts=(None, (T, 17, 0))[(i + 1) % 2], n_z=3 if regime == "loud" else (1, 3)[(i // 2) % 2], h_ld=(2, 4)[i % 2],
                       wform=("T", "BT")[i % 2] if need_w else (None, "T", "BT")[i % 3], fform=fform)
            if network:
                fac["D"] = (1, 2, 3)[(i + ri) % 3]
            kind = "dead" if i in (2, 7) else ("alldead" if i == 1 and regime in ("noise", "loud") else "geo")
            sform, pform = ("A", "BA")[(i // 3) % 2], ("A", "BA")[(i + ri) % 2]
            seed = 100 * ri + i
            j_star = None if n_tau is None else min(2, n_tau - 1)
            case = M.build(regime, T, taus=M.grid(n_tau, regime), j_star=j_star, seed=seed, x_s=x_s, **fac)
            case["data"] = case["data"] * DATA_SCALE_OF.get((regime, i), DATA_SCALE)
            scales, log_prior = scale_grid(n_a, sform, pform, kind)
            tag = f"{'net ' if network else ''}{regime} #{i} T={T} n_tau={n_tau} n_a={n_a} {kind} scales={sform} prior={pform}" + \
                "".join(f" {k}={v}" for k, v in fac.items())
            out.append((tag, dict(fac, regime=regime, T=T, n_tau=n_tau, n_a=n_a, kind=kind, sform=sform, pform=pform, combo=i), case,
                        scales, log_prior))
    return out


def parent_reference(network, case):
    M = N if network else R1
    return M.reference(**M.call_args(case))
