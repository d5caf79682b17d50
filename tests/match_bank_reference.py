"""float64 reference of the bank match (``npf_waveform_match_bank``) and the input sets its tests share.

``reference`` evaluates the definition of include/npf_hip.h directly: one complex ``exp`` per (t, j), no recurrence, no matrix
instruction, removed points masked (not cut).  ``cases`` lists the inputs of the GPU parity test, one sweep per axis over the sizes at
which the kernel changes path (a tile of 16 rows / 16 templates, a k-step of four points, a chunk of JC shifts);
tests/test_match_bank_host.py checks on the CPU that every one of them leaves the runner-up of max_j |c_j| and the runner-up template
at least 1e-6 (normalised) below the best, so ``tau_index`` and ``best_index`` are well posed in all of them."""
import math

import torch

import match_reference as M

TWO_PI = M.TWO_PI
DTAU = M.DTAU
ROWS = (1, 15, 16, 17, 33)
BANKS = (1, 15, 16, 17, 40)
POINTS = (1, 2, 3, 5, 127, 128, 129, 200)
SHIFTS = (0, 1, 15, 16, 17, 33)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def reference(h, bank, weights=None, freqs=None, taus=None):
    """Every output of ``npf_waveform_match_bank`` in float64 on the CPU (dict; ``mag`` [R, G, n]: the normalised |c_j|,
    ``degenerate`` [R, G], ``tau`` with a grid)."""
    h, bank = h.detach().cpu().double(), bank.detach().cpu().double()
    R, T, G = h.shape[0], h.shape[1], bank.shape[0]
    w = torch.ones(T, dtype=torch.float64) if weights is None else weights.detach().cpu().double()
    live = (w > 0) & torch.isfinite(w)
    sel = lambda x: torch.where(live, x, torch.zeros_like(x))  # noqa: E731  (selected, never multiplied in)
    w, A, ph, Ag, phg = sel(w), sel(h[..., 0]), sel(h[..., 1]), sel(bank[..., 0]), sel(bank[..., 1])
    hh, gg = (w * A * A).sum(1), (w * Ag * Ag).sum(1)
    u = (w * A) * torch.exp(1j * ph)  # [R, T]
    v = Ag * torch.exp(-1j * phg)     # [G, T]: conj
    if taus is None:
        E = torch.ones(T, 1, dtype=torch.complex128)
    else:
        f = sel(freqs.detach().cpu().double())
        tau = taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]
        E = torch.exp(1j * TWO_PI * f.view(T, 1) * tau.view(1, -1))  # one complex exp per (t, j)
    # an explicit sum over t keeps a NaN of row r in row r and of template g in column g (no 0 * NaN through a matrix product)
    c = ((u.view(R, 1, T, 1) * v.view(1, G, T, 1)) * E.view(1, 1, T, -1)).sum(2)  # [R, G, n]
    prod = hh.view(R, 1) * gg.view(1, G)
    deg = prod == 0
    nrm = torch.where(deg, torch.ones_like(prod), prod.sqrt())
    cn = torch.where(deg.unsqueeze(2), torch.zeros_like(c), c / nrm.unsqueeze(2))
    mag = cn.abs()
    best = mag.max(2).values
    idx = torch.where(deg, torch.zeros(R, G, dtype=torch.long), (mag == best.unsqueeze(2)).double().argmax(2))
    cb = torch.where(deg, torch.zeros_like(prod).to(c.dtype), c.gather(2, idx.unsqueeze(2))[..., 0])
    ranked = torch.where(torch.isnan(best), torch.full_like(best, -math.inf), best)
    top = ranked.max(1).values
    best_index = torch.where(torch.isinf(top), torch.zeros(R, dtype=torch.long), (ranked == top.view(R, 1)).double().argmax(1))
    out = dict(hh=hh, gg=gg, match=best, mismatch=1.0 - best, tau_index=idx,
               phase=torch.where(deg, torch.zeros_like(prod), torch.atan2(cb.imag, cb.real)), dot=torch.stack([cb.real, cb.imag], -1),
               best_index=best_index, best_match=best.gather(1, best_index.view(R, 1))[:, 0], mag=mag, degenerate=deg)
    if taus is not None:
        out["tau"] = taus[0] + idx.double() * taus[1]
    return out


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref):
    """Worst error / gate per quantity ``got`` holds: the gates of ``match_reference.ratios`` for hh, gg, match, mismatch, phase and
    tau_index; best_match under the gate of match; best_index exact; dot: |d| <= 1e-9 sqrt(hh gg) per component."""
    flat = {k: ref[k].reshape(-1) for k in ("match", "mismatch", "hh", "gg", "phase", "tau_index")}
    out = M.ratios({k: got.get(k) for k in flat}, flat)
    if got.get("best_match") is not None:
        out["best_match"] = M.ratios(dict(match=got["best_match"]), dict(match=ref["best_match"]))["match"]
    if got.get("best_index") is not None:
        out["best_index"] = 0.0 if torch.equal(got["best_index"].detach().cpu().long(), ref["best_index"]) else math.inf
    if got.get("dot") is not None:
        d = (got["dot"].detach().cpu().double() - ref["dot"]).abs()
        gate = 1e-9 * (ref["hh"].view(-1, 1) * ref["gg"].view(1, -1)).sqrt().unsqueeze(2).expand_as(d)
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)
        out["dot"] = float(torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf)).max())
    return out


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def build(n_rows, n_bank, pts, n_tau, seed=0, h_ld=2, weighted=True, pick=None, j_star=None):
    """One input set -> dict(h [n_rows, pts, h_ld], bank [n_bank, pts, 2], weights [pts] or None, freqs [pts], taus), fp32 CPU
    tensors.  The templates are chirps of distinct rates and phases with a falling amplitude; row r is template (5 r + 2) % n_bank
    shifted by the grid time of index (3 r + 1) % n_tau, with 5 % amplitude and 0.2 rad phase scatter, so ``best_index`` and
    ``tau_index`` take many values.  ``pick`` / ``j_star``: the template and the shift index of every row in the place of those
    two rules (the random draws are the same).  Columns of ``h`` beyond the second hold noise: never read."""
    g = torch.Generator().manual_seed(7919 * seed + 13)
    x = torch.linspace(0.0, 1.0, pts, dtype=torch.float64) if pts > 1 else torch.zeros(1, dtype=torch.float64)
    f = (20.0 + 492.0 * x).float()
    taus = None if not n_tau else (-min(2, n_tau - 1) * DTAU, DTAU, n_tau)
    amp = (1.0 + 2.0 * x).pow(-7.0 / 6.0).view(1, pts) * (1.0 + 0.1 * torch.randn(n_bank, pts, generator=g, dtype=torch.float64)).abs()
    k = torch.arange(n_bank, dtype=torch.float64).view(n_bank, 1)
    phase = (6.0 + 2.5 * k) * x.view(1, pts) ** 2 + 0.9 * k + 0.3 * torch.randn(n_bank, pts, generator=g, dtype=torch.float64)
    bank = torch.stack([amp, phase], -1).float()
    pick = (5 * torch.arange(n_rows) + 2) % n_bank if pick is None else torch.as_tensor(pick, dtype=torch.long)
    ra = bank[pick, :, 0].double() * (1.0 + 0.05 * torch.randn(n_rows, pts, generator=g, dtype=torch.float64)).abs()
    rp = bank[pick, :, 1].double() + 0.2 * torch.randn(n_rows, pts, generator=g, dtype=torch.float64)
    if taus is not None:
        j = (3 * torch.arange(n_rows) + 1) % n_tau if j_star is None else torch.as_tensor(j_star, dtype=torch.long)
        rp = rp - TWO_PI * f.double().view(1, pts) * (taus[0] + j.double() * taus[1]).view(n_rows, 1)
    h = torch.randn(n_rows, pts, h_ld, generator=g)
    h[..., 0], h[..., 1] = ra.float(), rp.float()
    w = (0.5 + torch.rand(pts, generator=g)) if weighted else None
    return dict(h=h, bank=bank, weights=w, freqs=f, taus=taus)


def cases():
    """The inputs of the GPU parity test: one sweep per axis with the others small, and one case with every axis past a boundary.
    One point matches every template perfectly and has the same |c_j| at every shift, so pts = 1 comes with one template and no
    grid.  ``h_ld`` (2, 4) and the weights (given, none) rotate with the case number.  -> list of (tag, sizes, case)."""
    sizes = [dict(n_rows=r, n_bank=3, pts=37, n_tau=5) for r in ROWS]
    sizes += [dict(n_rows=3, n_bank=b, pts=37, n_tau=5) for b in BANKS]
    sizes += [dict(n_rows=3, n_bank=1 if p == 1 else 3, pts=p, n_tau=0 if p == 1 else 5) for p in POINTS]
    sizes += [dict(n_rows=3, n_bank=5, pts=37, n_tau=n) for n in SHIFTS]
    sizes += [dict(n_rows=33, n_bank=40, pts=129, n_tau=17)]
    out = []
    for i, s in enumerate(sizes):
        fac = dict(s, h_ld=(2, 4)[i % 2], weighted=(i // 2) % 2 == 0)
        out.append((" ".join(f"{k}={v}" for k, v in fac.items()), fac, build(seed=i, **fac)))
    return out


def call_args(case):
    return {k: case[k] for k in ("h", "bank", "weights", "freqs", "taus")}
