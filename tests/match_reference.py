"""float64 reference of the waveform match (``npf_waveform_match``) and the input builders its tests share.

``reference`` evaluates the definition of include/npf_hip.h directly: one complex ``exp`` per (t, j), no recurrence, removed points
masked (not cut).  ``recurrence`` is the same quantity the way the kernel's first launch forms it -- one sine / cosine pair at the
first shift of every chunk of ``jc`` shifts and a complex rotation per further shift -- so the CPU suite can measure what the
recurrence costs.  ``cases`` lists the inputs of the GPU test: tests/test_match_host.py checks on the CPU that every one of them
leaves the runner-up of max_j |c_j| at least 1e-6 (normalised) below the best, so ``tau_index`` is well posed in all of them."""
import math

import torch

TWO_PI = 2.0 * math.pi
DTAU = 1.0 / 2048.0  # s: a power of two, so tau0 = -j dtau puts tau = 0 on the grid exactly
B = 3
PHI0 = 0.7
REGIMES = ("same", "shift", "offset", "random", "bigphase", "removed", "degenerate")


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _terms(h, g, weights, freqs, n_valid):
    """float64 (a [R, T] = w A A' with removed and padded points at 0, theta [R, T], w A^2, w A'^2, f [R, T], live [R, T])."""
    h, g = h.detach().cpu().double(), g.detach().cpu().double()
    R, T, Bn = h.shape[0], h.shape[1], g.shape[0]
    task = torch.arange(R) % Bn
    w = torch.ones(Bn, T, dtype=torch.float64) if weights is None else weights.detach().cpu().double().expand(Bn, T)
    nv = torch.full((Bn,), T) if n_valid is None else n_valid.detach().cpu().long().clamp(0, T)
    live = (w > 0) & torch.isfinite(w) & (torch.arange(T).view(1, T) < nv.view(Bn, 1))
    live_r, w_r, g_r = live[task], w[task], g[task]
    zero = torch.zeros(R, T, dtype=torch.float64)
    A, ph, Ag, phg = h[..., 0], h[..., 1], g_r[..., 0], g_r[..., 1]
    a = torch.where(live_r, w_r * A * Ag, zero)
    theta = torch.where(live_r, ph - phg, zero)
    f = zero if freqs is None else torch.where(live_r, freqs.detach().cpu().double().expand(Bn, T)[task], zero)
    return a, theta, torch.where(live_r, w_r * A * A, zero), torch.where(live_r, w_r * Ag * Ag, zero), f, live_r


def _finish(c, c0, hh, gg_rows, Bn, taus):
    """The outputs from the complex sums c [R, n] (the candidates of the maximum), c0 [R], hh [R], gg [R]."""
    prod = hh * gg_rows
    deg = prod == 0
    nrm = torch.where(deg, torch.ones_like(prod), prod.sqrt())
    cn = torch.where(deg.view(-1, 1), torch.zeros_like(c), c / nrm.view(-1, 1))
    mag = cn.abs()
    best, idx = mag.max(1)
    idx = torch.where(deg, torch.zeros_like(idx), (mag == best.view(-1, 1)).double().argmax(1))  # the smallest index at the maximum
    cb = cn.gather(1, idx.view(-1, 1))[:, 0]
    out = dict(hh=hh, gg=gg_rows[:Bn], overlap=torch.where(deg, torch.zeros_like(prod), c0.real / nrm), match=best, mismatch=1.0 - best,
               tau_index=idx, phase=torch.where(deg, torch.zeros_like(prod), torch.atan2(cb.imag, cb.real)),
               corr=torch.stack([cn.real, cn.imag], -1), mag=mag, degenerate=deg)
    if taus is not None:
        out["tau"] = taus[0] + idx.double() * taus[1]
    return out


def reference(h, g, weights=None, freqs=None, taus=None, n_valid=None):
    """Every output of ``npf_waveform_match`` in float64 on the CPU (dict; ``mag`` [R, n]: the normalised |c_j|, ``degenerate`` [R])."""
    a, theta, whh, wgg, f, _ = _terms(h, g, weights, freqs, n_valid)
    c0 = (a * torch.exp(1j * theta)).sum(1)
    if taus is None:
        c = c0.view(-1, 1)
    else:
        tau = taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]
        c = (a.unsqueeze(2) * torch.exp(1j * (theta.unsqueeze(2) + TWO_PI * f.unsqueeze(2) * tau.view(1, 1, -1)))).sum(1)
    return _finish(c, c0, whh.sum(1), wgg.sum(1), g.shape[0], taus)


def recurrence(h, g, weights=None, freqs=None, taus=None, n_valid=None, jc=16, sincos=None):
    """The same outputs with c_j formed as the kernel forms it: per chunk of ``jc`` shifts one sine / cosine pair at the chunk's
    first shift and one of the step 2 pi f dtau, then z <- z s.  ``sincos(x) -> (sin, cos)``: the sine / cosine used (default: float64),
    which lets a test put a float32 evaluation in their place."""
    sincos = sincos or (lambda x: (torch.sin(x), torch.cos(x)))
    a, theta, whh, wgg, f, _ = _terms(h, g, weights, freqs, n_valid)
    s0, c0_ = sincos(theta)
    c0 = torch.complex((a * c0_).sum(1), (a * s0).sum(1))
    if taus is None:
        c = c0.view(-1, 1)
    else:
        tau0, dtau, n_tau = taus
        om = TWO_PI * f
        ss, sc = sincos(om * dtau)
        cols = []
        for j0 in range(0, n_tau, jc):
            sn, cs = sincos(theta + om * (tau0 + j0 * dtau))
            zr, zi = a * cs, a * sn
            for _ in range(min(jc, n_tau - j0)):
                cols.append(torch.complex(zr.sum(1), zi.sum(1)))
                zr, zi = zr * sc - zi * ss, zr * ss + zi * sc
        c = torch.stack(cols, 1)
    return _finish(c, c0, whh.sum(1), wgg.sum(1), g.shape[0], taus)


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref):
    """Worst error / gate per quantity ``got`` holds (a mapping name -> tensor or None): overlap, match, mismatch and every corr
    component |d| <= 1e-9 + 2^-23 |ref|; hh, gg |d| <= 2^-23 |ref|; phase: the difference mod 2 pi <= 1e-6 where the reference's
    normalised |c| is at least 1e-3; tau_index: exact (ratio 0 or inf)."""
    out = {}
    for name in ("overlap", "match", "mismatch", "corr", "hh", "gg", "phase", "tau_index"):
        x = got.get(name)
        if x is None:
            continue
        x, r = x.detach().cpu().double().reshape(-1), ref[name].double().reshape(-1)
        assert x.shape == r.shape, (name, x.shape, r.shape)
        if name == "tau_index":
            out[name] = 0.0 if torch.equal(x, r) else math.inf
            continue
        d = (x - r).abs()
        if name == "phase":
            d = torch.remainder(x - r + math.pi, TWO_PI) - math.pi
            keep = ref["match"] >= 1e-3
            d, gate = d.abs()[keep], torch.full_like(d[keep], 1e-6)
        elif name in ("hh", "gg"):
            gate = 2.0 ** -23 * r.abs()
        else:
            gate = 1e-9 + 2.0 ** -23 * r.abs()
        bad = ~torch.isfinite(d)
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)  # (0 / 0 of an exact zero: inside the gate)
        q = torch.where(bad, torch.full_like(q, math.inf), q)
        out[name] = float(q.max()) if q.numel() else 0.0
    return out


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _freqs(T, form, g):
    if form == "T":
        return torch.linspace(20.0, 512.0, T)
    per_task = torch.stack([torch.linspace(20.0 + 3.0 * b, 512.0 - 40.0 * b, T) for b in range(B)])
    return per_task + 0.25 * torch.rand(B, T, generator=g)


def _weights(T, form, g):
    if form is None:
        return None
    return 0.5 + torch.rand((T,) if form == "T" else (B, T), generator=g)


def _waveform(T, g, phase_std):
    """[B, T, 2]: a positive, falling amplitude with 10 % scatter and a random phase of the given spread."""
    amp = torch.linspace(1.0, 3.0, T).pow(-7.0 / 6.0).view(1, T) * (1.0 + 0.1 * torch.randn(B, T, generator=g)).abs()
    return torch.stack([amp, phase_std * torch.randn(B, T, generator=g)], -1)


def build(regime, T, n_z=1, h_ld=2, wform=None, fform="T", taus=None, counts=None, j_star=None, seed=0):
    """One input set -> dict(h [n_z B, T, h_ld], g [B, T, 2], weights, freqs, taus, n_valid, plus what the regime plants), fp32 CPU
    tensors.  ``wform`` / ``fform``: None, "T" or "BT"; ``counts``: None or a tuple of B counts; ``j_star``: the planted index of
    the "shift" regime.  Columns of ``h`` beyond the second hold noise (the raw scale of a decoder row): never read."""
    g_ = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + seed)
    f = _freqs(T, fform, g_) if fform is not None else None
    w = _weights(T, wform, g_)
    ref_wave = _waveform(T, g_, 1e4 if regime == "bigphase" else 3.0)
    pred = ref_wave.unsqueeze(0).repeat(n_z, 1, 1, 1)  # [n_z, B, T, 2]: every latent sample predicts the reference ...
    plant = {}
    if regime == "shift":  # ... but for a time shift by a grid time: phi' = phi + 2 pi f tau_{j*}
        assert taus is not None and j_star is not None and 0 <= j_star < taus[2]
        t_star = taus[0] + j_star * taus[1]
        ref_wave[..., 1] = (ref_wave[..., 1].double() + TWO_PI * f.double().expand(B, T) * t_star).float()
        plant["j_star"] = j_star
    elif regime == "offset":  # ... but for a constant phase: phi' = phi - PHI0, so arg c = +PHI0
        ref_wave[..., 1] = ref_wave[..., 1] - PHI0
    elif regime in ("random", "bigphase", "removed", "degenerate"):  # unrelated prediction and reference, another per latent sample
        pred = torch.stack([_waveform(T, g_, 1e4 if regime == "bigphase" else 3.0) for _ in range(n_z)])
    h = torch.randn(n_z * B, T, h_ld, generator=g_)
    h[..., :2] = pred.reshape(n_z * B, T, 2)
    out = dict(h=h, g=ref_wave.clone(), weights=w, freqs=f, taus=taus,
               n_valid=None if counts is None else torch.tensor(counts, dtype=torch.int32), **plant)
    if regime == "removed":  # a third of the points: weight 0, negative, NaN or Inf, and NaN in everything else there
        assert w is not None
        kill = torch.rand(w.shape, generator=g_) < 1.0 / 3.0
        kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])[torch.randint(0, 4, w.shape, generator=g_)]
        out["weights"] = torch.where(kill, kinds, w)
        kill_b = kill.expand(B, T)
        out["g"][kill_b] = math.nan
        out["h"].view(n_z, B, T, h_ld)[:, kill_b] = math.nan
        if f is not None:
            kill_f = kill_b if f.dim() == 2 else kill_b.all(0)  # (a frequency row shared by the tasks: where every task lost the point)
            out["freqs"] = torch.where(kill_f, torch.full_like(f, math.nan), f)
        out["kill"] = kill_b
    if regime == "degenerate":  # all weights zero: of the last task ([B, T] weights) or of every task ([T])
        assert w is not None
        out["weights"] = w.clone()
        out["weights"][-1 if w.dim() == 2 else slice(None)] = 0.0
    if counts is not None and regime == "removed":  # the rows beyond the counts are NaN as well
        for b, n in enumerate(counts):
            out["g"][b, n:] = math.nan
            out["h"].view(n_z, B, T, h_ld)[:, b, n:] = math.nan
    return out


def cut(case):
    """The case with its removed points (``kill``, the same for every task) and nothing else cut away -- for 'removing equals cutting'."""
    keep = ~case["kill"][0]
    assert (case["kill"] == case["kill"][0]).all()
    sel = lambda t: None if t is None else t[..., keep]  # noqa: E731
    return dict(h=case["h"][:, keep], g=case["g"][:, keep], weights=sel(case["weights"]), freqs=sel(case["freqs"]), taus=case["taus"],
                n_valid=None)


def grid(n_tau, regime="same"):
    """(tau0, dtau, n_tau) with tau = 0 on the grid (index min(2, n_tau - 1)); the "bigphase" regime starts at -+1 s."""
    if n_tau is None:
        return None
    if regime == "bigphase":
        return (-1.0 if n_tau % 2 else 1.0, DTAU, n_tau)
    return (-min(2, n_tau - 1) * DTAU, DTAU, n_tau)


def cases(jc):
    """The inputs of the GPU test: every regime at T in {37, 200} and n_tau in {none, 1, 5, jc - 1, jc, jc + 1, 257}; the other
    factors -- counts (T, 17, 0) or none, n_z in {1, 3}, h_ld in {2, 4}, the form of weights and freqs -- rotate with the
    regime's case number at different periods (tests/test_match_host.py checks that every value of every factor meets every regime).  The "shift" regime
    needs a grid with room for the planted index: n_tau = jc + 1 (j* = 5 inside a chunk, jc - 1 a chunk's last index, jc a chunk's
    first) and 257 (j* = jc + 5, 2 jc - 1, 2 jc, 256).  -> list of (tag, factors, case)."""
    out = []
    for regime in REGIMES:
        i = 0  # the regime's running case number: the other factors rotate with it at different periods
        for T in (37, 200):
            for n_tau in (None, 1, 5, jc - 1, jc, jc + 1, 257):
                stars = [None]
                if regime == "shift":
                    stars = {jc + 1: [5, jc - 1, jc], 257: [jc + 5, 2 * jc - 1, 2 * jc, 256]}.get(n_tau, [])
                for j_star in stars:
                    need_w = regime in ("removed", "degenerate")
                    w_opts, f_opts = ["T", "BT"] if need_w else [None, "T", "BT"], [None, "BT", "T"]
                    fform = f_opts[(i // 3) % 3]
                    if fform is None and n_tau is not None:  # (a grid needs the frequencies)
                        fform = ("T", "BT")[i % 2]
                    fac = dict(counts=(None, (T, 17, 0))[i % 2], n_z=(1, 3)[(i // 2) % 2], h_ld=(2, 4)[(i + i // 4) % 2],
                               wform=w_opts[(i // 4) % 2 if need_w else i % 3], fform=fform)
                    i += 1
                    case = build(regime, T, taus=grid(n_tau, regime), j_star=j_star, seed=len(out), **fac)
                    tag = f"{regime} T={T} n_tau={n_tau}" + (f" j*={j_star}" if j_star is not None else "") + \
                        "".join(f" {k}={v}" for k, v in fac.items())
                    out.append((tag, dict(fac, regime=regime, T=T, n_tau=n_tau), case))
    return out


def call_args(case):
    return {k: case[k] for k in ("h", "g", "weights", "freqs", "taus", "n_valid")}
