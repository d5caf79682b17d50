"""float64 reference of the matched-filter log likelihood (``npf_waveform_loglike``) and the input builders its tests share.

``reference`` evaluates the definitions of include/npf_hip.h directly: one complex ``exp`` per (t, j), no recurrence, points that are
not live masked (not cut), ``ln I0(x) = x + log(i0e(x))`` with scipy's exponentially scaled Bessel function (below x = 1, where that sum
cancels, log1p of the power series), ``torch.logsumexp``;
hh and dd are exactly rounded sums (``math.fsum``), so their gate of 2^-50 is all the kernel's.  ``recurrence`` forms kappa_j the way
the kernel's first launch does -- one sine / cosine pair at the first shift of every chunk of ``jc`` shifts, a complex rotation per
further shift -- so the CPU suite measures what the recurrence costs.  ``log_i0_scheme`` is the kernel's ``ln I0`` in Python.
``cases`` lists the inputs of the GPU test; tests/test_loglike_host.py checks on the CPU that every one of them leaves the runner-up of
max_j x_j at least 1e-6 sqrt(hh dd) below the best, so ``tau_index`` is well posed in all of them."""
import math

import torch
from scipy import special

import match_reference as M

TWO_PI = M.TWO_PI
DTAU = M.DTAU
B = M.B
PHI0 = 0.7
REGIMES = ("planted", "noise", "loud", "quiet", "edge", "bigphase", "removed", "degenerate")
DOUBLES = ("hh", "dd", "optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "lnl_mix", "lnl_max_mix")
I0_ASYM_TERMS = 16  # terms of the kernel's 1 / (8 x) series from the switch point on


# ---- ln I0 -------------------------------------------------------------------------------------------------------------------------
def log_i0(x):
    """ln I0(x) of a float64 tensor, x >= 0.  From 1 on: x + log(i0e(x)), i0e = e^{-x} I0 (no overflow).  Below 1 that sum cancels
    (at x = 1e-3 it keeps 1e-16 of a value of 2.5e-7), so there: log1p(I0 - 1) with I0 - 1 = sum_{k = 1 .. 14} (x^2 / 4)^k / (k!)^2,
    whose first omitted term is below 1e-33 of the sum.  tests/test_loglike_host.py holds both branches against 50 digits."""
    x = x.double()
    big = x + torch.log(torch.from_numpy(special.i0e(x.numpy())).reshape(x.shape))
    q = 0.25 * x.clamp(max=1.0) ** 2
    s = torch.zeros_like(q)
    for k in range(14, 0, -1):  # Horner: s = q / k^2 (1 + s)
        s = q / float(k * k) * (1.0 + s)
    return torch.where(x < 1.0, torch.log1p(s), big)


def log_i0_scheme(x, x_s, terms=I0_ASYM_TERMS):
    """The kernel's ln I0 of one host float: below ``x_s`` log1p of the power series of I0 - 1, from there on x - ln(2 pi x) / 2 +
    log1p(the first ``terms`` terms of the series in 1 / (8 x)), by Horner's rule."""
    if x < x_s:
        q = 0.25 * x * x
        t = s = q
        for k in range(2, 49):
            t *= q * (1.0 / float(k * k))
            s += t
            if t <= s * 2.0 ** -60:
                break
        return math.log1p(s)
    u, acc = 0.125 / x, 0.0
    for k in range(terms, 0, -1):
        acc = u * (float((2 * k - 1) ** 2) / float(k)) * (1.0 + acc)
    return x - 0.5 * math.log(TWO_PI * x) + math.log1p(acc)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _fsum_rows(x):
    return torch.tensor([math.fsum(row) for row in x.tolist()], dtype=torch.float64)


def _terms(h, d, weights, freqs, n_valid):
    """float64 (c [R, T] complex = w A conj(d) with dead points at 0, phi [R, T], hh [R], dd [R], f [R, T])."""
    h, d = h.detach().cpu().double(), d.detach().cpu().double()
    R, T, Bn = h.shape[0], h.shape[1], d.shape[0]
    task = torch.arange(R) % Bn
    w = torch.ones(Bn, T, dtype=torch.float64) if weights is None else weights.detach().cpu().double().expand(Bn, T)
    nv = torch.full((Bn,), T) if n_valid is None else n_valid.detach().cpu().long().clamp(0, T)
    live = (w > 0) & torch.isfinite(w) & (torch.arange(T).view(1, T) < nv.view(Bn, 1))
    live_r, w_r, d_r = live[task], w[task], d[task]
    zero = torch.zeros(R, T, dtype=torch.float64)
    A, ph, dre, dim = h[..., 0], h[..., 1], d_r[..., 0], d_r[..., 1]
    wa = w_r * A
    c = torch.complex(torch.where(live_r, wa * dre, zero), torch.where(live_r, -(wa * dim), zero))
    phi = torch.where(live_r, ph, zero)
    f = zero if freqs is None else torch.where(live_r, freqs.detach().cpu().double().expand(Bn, T)[task], zero)
    hh = _fsum_rows(torch.where(live_r, wa * A, zero))
    dd = _fsum_rows(torch.where(live_r, w_r * (dre * dre + dim * dim), zero))
    return c, phi, hh, dd, f


def log_mean_exp_rows(v, Bn):
    """[R] -> [B]: logsumexp over the latent samples of every task (row s * B + b) - ln n_z."""
    n_z = v.shape[0] // Bn
    return torch.logsumexp(v.view(n_z, Bn), 0) - math.log(n_z)


def _finish(kappa, hh, dd, Bn, taus):
    """The outputs from the complex sums kappa [R, n] (the candidates), hh [R], dd [R]."""
    n = kappa.shape[1]
    deg = hh == 0
    x = kappa.abs()
    best, _ = x.max(1)
    idx = (x == best.view(-1, 1)).double().argmax(1)  # the smallest index at the maximum
    idx = torch.where(deg, torch.zeros_like(idx), idx)
    kb = kappa.gather(1, idx.view(-1, 1))[:, 0]
    rt = torch.where(deg, torch.ones_like(hh), hh.sqrt())
    z = torch.zeros_like(hh)
    L = torch.where(deg.view(-1, 1), torch.zeros_like(x), log_i0(x) - 0.5 * hh.view(-1, 1))
    lnl_max = torch.where(deg, z, best - 0.5 * hh)
    lnl_marg = torch.where(deg, z, torch.logsumexp(L, 1) - math.log(n))
    snr_j = torch.where(deg.view(-1, 1), torch.zeros_like(x), x / rt.view(-1, 1))
    out = dict(hh=hh, dd=dd[:Bn], dd_rows=dd, optimal_snr=hh.sqrt(), snr=torch.where(deg, z, best / rt), lnl_max=lnl_max,
               lnl_marg=lnl_marg, tau_index=idx, phase=torch.where(deg, z, torch.atan2(kb.imag, kb.real)),
               series=torch.stack([L, snr_j], -1), lnl_mix=log_mean_exp_rows(lnl_marg, Bn), lnl_max_mix=log_mean_exp_rows(lnl_max, Bn),
               x=x, degenerate=deg)
    if taus is not None:
        out["tau"] = taus[0] + idx.double() * taus[1]
    return out


def reference(h, data, weights=None, freqs=None, taus=None, n_valid=None):
    """Every output of ``npf_waveform_loglike`` in float64 on the CPU (dict; ``x`` [R, n]: |kappa_j|, ``dd_rows`` [R],
    ``degenerate`` [R])."""
    c, phi, hh, dd, f = _terms(h, data, weights, freqs, n_valid)
    if taus is None:
        kappa = (c * torch.exp(1j * phi)).sum(1).view(-1, 1)
    else:
        tau = taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]
        kappa = (c.unsqueeze(2) * torch.exp(1j * (phi.unsqueeze(2) + TWO_PI * f.unsqueeze(2) * tau.view(1, 1, -1)))).sum(1)
    return _finish(kappa, hh, dd, data.shape[0], taus)


def recurrence(h, data, weights=None, freqs=None, taus=None, n_valid=None, jc=16):
    """The same outputs with kappa_j formed as the kernel forms it: per chunk of ``jc`` shifts one sine / cosine pair at the chunk's
    first shift and one of the step 2 pi f dtau, then z <- z s."""
    c, phi, hh, dd, f = _terms(h, data, weights, freqs, n_valid)
    cr, ci = c.real, c.imag
    if taus is None:
        sn, cs = torch.sin(phi), torch.cos(phi)
        kappa = torch.complex((cs * cr - sn * ci).sum(1), (cs * ci + sn * cr).sum(1)).view(-1, 1)
    else:
        tau0, dtau, n_tau = taus
        om = TWO_PI * f
        ss, sc = torch.sin(om * dtau), torch.cos(om * dtau)
        cols = []
        for j0 in range(0, n_tau, jc):
            arg = phi + om * (tau0 + j0 * dtau)
            sn, cs = torch.sin(arg), torch.cos(arg)
            zr, zi = cs * cr - sn * ci, cs * ci + sn * cr
            for _ in range(min(jc, n_tau - j0)):
                cols.append(torch.complex(zr.sum(1), zi.sum(1)))
                zr, zi = zr * sc - zi * ss, zr * ss + zi * sc
        kappa = torch.stack(cols, 1)
    return _finish(kappa, hh, dd, data.shape[0], taus)


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def scale_of(ref):
    """sqrt(hh dd) + hh / 2 per row [R]: the size of the terms lnl is made of."""
    return (ref["hh"] * ref["dd_rows"]).sqrt() + 0.5 * ref["hh"]


def ratios(got, ref, lnl_gate=1e-10, lnl_floor=1e-12):
    """Worst error / gate per quantity ``got`` holds (a mapping name -> tensor or None).  lnl_max, lnl_marg, lnl_mix, lnl_max_mix
    and the series' L_j: |d| <= lnl_gate (sqrt(hh dd) + hh / 2) + lnl_floor (per task: the largest scale among its rows); hh, dd:
    2^-50 relative; snr, optimal_snr, series SNR: 1e-10 relative + 1e-12; phase: the difference mod 2 pi <= 1e-9 where
    x* >= 1e-3 sqrt(hh dd); tau_index: exact (ratio 0 or inf)."""
    out = {}
    scale = scale_of(ref)
    Bn = ref["dd"].shape[0]
    task_scale = scale.view(-1, Bn).max(0).values

    def put(name, d, gate):
        bad = ~torch.isfinite(d)
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)  # (0 / 0 of an exact zero: inside the gate)
        q = torch.where(bad, torch.full_like(q, math.inf), q)
        out[name] = max(out.get(name, 0.0), float(q.max()) if q.numel() else 0.0)

    for name in ("hh", "dd", "optimal_snr", "snr", "lnl_max", "lnl_marg", "phase", "tau_index", "lnl_mix", "lnl_max_mix", "series"):
        x = got.get(name)
        if x is None:
            continue
        x = x.detach().cpu()
        if name == "tau_index":
            out[name] = 0.0 if torch.equal(x.reshape(-1).long(), ref[name].long()) else math.inf
            continue
        assert x.dtype == torch.float64, (name, x.dtype)
        if name == "series":
            r = ref[name]
            x = x.reshape(r.shape)
            put("series_L", (x[..., 0] - r[..., 0]).abs(), (lnl_gate * scale + lnl_floor).view(-1, 1).expand_as(r[..., 0]))
            put("series_snr", (x[..., 1] - r[..., 1]).abs(), 1e-10 * r[..., 1].abs() + 1e-12)
            continue
        x, r = x.reshape(-1), ref[name].reshape(-1)
        assert x.shape == r.shape, (name, x.shape, r.shape)
        d = (x - r).abs()
        if name == "phase":
            d = (torch.remainder(x - r + math.pi, TWO_PI) - math.pi).abs()
            keep = ref["x"].max(1).values >= 1e-3 * (ref["hh"] * ref["dd_rows"]).sqrt()
            keep &= ~ref["degenerate"]
            put(name, d[keep], torch.full_like(d[keep], 1e-9))
        elif name in ("hh", "dd"):
            put(name, d, 2.0 ** -50 * r.abs())
        elif name in ("snr", "optimal_snr"):
            put(name, d, 1e-10 * r.abs() + 1e-12)
        elif name in ("lnl_mix", "lnl_max_mix"):
            put(name, d, lnl_gate * task_scale + lnl_floor)
        else:
            put(name, d, lnl_gate * scale + lnl_floor)
    return out


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _cartesian(wave):
    """(amplitude, phase) [.., 2] float tensor -> (Re, Im) in float64."""
    a, p = wave[..., 0].double(), wave[..., 1].double()
    return torch.stack([a * torch.cos(p), a * torch.sin(p)], -1)


def build(regime, T, n_z=1, h_ld=2, wform=None, fform="T", taus=None, counts=None, j_star=None, seed=0, x_s=24.0):
    """One input set -> dict(h [n_z B, T, h_ld], data [B, T, 2], weights, freqs, taus, n_valid, plus what the regime plants), fp32 CPU
    tensors.  ``wform`` / ``fform``: None, "T" or "BT"; ``counts``: None or a tuple of B counts; ``j_star``: the planted grid index
    of the "planted" regime.  Columns of ``h`` beyond the second hold noise (the raw scale of a decoder row): never read."""
    g_ = torch.Generator().manual_seed(5000 + 1000 * REGIMES.index(regime) + seed)
    f = M._freqs(T, fform, g_) if fform is not None else None
    w = M._weights(T, wform, g_)
    pspread = 1e4 if regime == "bigphase" else 3.0
    pred = torch.stack([M._waveform(T, g_, pspread) for _ in range(n_z)])  # [n_z, B, T, 2], another waveform per latent sample
    data = torch.stack([torch.randn(B, T, generator=g_), torch.randn(B, T, generator=g_)], -1)  # unrelated Gaussian (Re, Im)
    plant = {}
    if regime in ("planted", "loud", "quiet", "edge"):  # the data hold a waveform: d = h shifted to the grid index j* and rotated
        src = M._waveform(T, g_, pspread)
        j_star = 0 if (j_star is None or taus is None) else j_star
        t_star = 0.0 if taus is None else taus[0] + j_star * taus[1]
        shifted = src.double().clone()
        if f is not None:
            shifted[..., 1] += TWO_PI * f.double().expand(B, T) * t_star
        shifted[..., 1] += PHI0
        data = _cartesian(shifted).float()  # d = A e^{i (phi + 2 pi f tau* + PHI0)}: kappa_{j*} = hh e^{-i PHI0} but for fp32 rounding
        pred = src.unsqueeze(0).repeat(n_z, 1, 1, 1)
        plant["j_star"] = j_star
        if regime == "planted":
            plant["data64"] = _cartesian(shifted)  # before the rounding to fp32: the planted identities hold to double precision
        else:  # scale the template so that x* ~ hh sits where the regime wants it
            wd = torch.ones(B, T) if w is None else w.expand(B, T)
            hh0 = (wd.double() * src[..., 0].double() ** 2).sum(1)  # [B], at full counts
            target = {"loud": 1e4, "quiet": 1e-3, "edge": x_s}[regime]
            k = (target / hh0).sqrt().float().view(1, B, 1)
            # the latent samples differ in amplitude: loud rows lie > 745 apart in lnl_marg, edge rows straddle the switch point
            fac = {"loud": (1.0, 0.6, 0.3), "quiet": (1.0, 0.9, 1.1), "edge": (1.02, 0.98, 1.5)}[regime]
            data = data * k.view(B, 1, 1)
            pred = pred.clone()
            for s in range(n_z):
                pred[s, ..., 0] = pred[s, ..., 0] * k[0] * fac[s % 3]
    h = torch.randn(n_z * B, T, h_ld, generator=g_)
    h[..., :2] = pred.reshape(n_z * B, T, 2)
    out = dict(h=h, data=data.clone(), weights=w, freqs=f, taus=taus,
               n_valid=None if counts is None else torch.tensor(counts, dtype=torch.int32), **plant)
    if regime == "removed":  # a third of the points: weight 0, negative, NaN or Inf, and NaN in everything else there
        assert w is not None
        kill = torch.rand(w.shape, generator=g_) < 1.0 / 3.0
        kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])[torch.randint(0, 4, w.shape, generator=g_)]
        out["weights"] = torch.where(kill, kinds, w)
        kill_b = kill.expand(B, T)
        out["data"][kill_b] = math.nan
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
            out["data"][b, n:] = math.nan
            out["h"].view(n_z, B, T, h_ld)[:, b, n:] = math.nan
    return out


def cut(case):
    """The case with its removed points (``kill``, the same for every task) and nothing else cut away -- 'removing equals cutting'."""
    keep = ~case["kill"][0]
    assert (case["kill"] == case["kill"][0]).all()
    sel = lambda t: None if t is None else t[..., keep]  # noqa: E731
    return dict(h=case["h"][:, keep], data=case["data"][:, keep], weights=sel(case["weights"]), freqs=sel(case["freqs"]),
                taus=case["taus"], n_valid=None)


grid = M.grid


def cases(jc, x_s):
    """The inputs of the GPU test: every regime at T in {37, 200} and n_tau in {none, 1, 5, jc - 1, jc, jc + 1, 257}; the other
    factors -- counts (T, 17, 0) or none, n_z in {1, 3}, h_ld in {2, 4}, the form of weights and freqs -- rotate with the regime's
    case number at different periods, as in match_reference.cases.  The "planted" regime adds, at n_tau = jc + 1, the planted
    indices 5, jc - 1, jc and at 257: jc + 5, 2 jc - 1, 2 jc, 256; on the other grids it plants the last index.
    -> list of (tag, factors, case)."""
    out = []
    for regime in REGIMES:
        i = 0
        for T in (37, 200):
            for n_tau in (None, 1, 5, jc - 1, jc, jc + 1, 257):
                stars = [None]
                if regime == "planted":
                    stars = {jc + 1: [5, jc - 1, jc], 257: [jc + 5, 2 * jc - 1, 2 * jc, 256]}.get(n_tau, [None if n_tau is None else n_tau - 1])
                elif regime in ("loud", "quiet", "edge") and n_tau is not None:
                    stars = [min(2, n_tau - 1)]  # (tau = 0 of the grid)
                for j_star in stars:
                    need_w = regime in ("removed", "degenerate")
                    w_opts, f_opts = ["T", "BT"] if need_w else [None, "T", "BT"], [None, "BT", "T"]
                    fform = f_opts[(i // 3) % 3]
                    if fform is None and n_tau is not None:  # (a grid needs the frequencies)
                        fform = ("T", "BT")[i % 2]
                    fac = dict(counts=(None, (T, 17, 0))[i % 2], n_z=(1, 3)[(i // 2) % 2], h_ld=(2, 4)[(i + i // 4) % 2],
                               wform=w_opts[(i // 4) % 2 if need_w else i % 3], fform=fform)
                    i += 1
                    case = build(regime, T, taus=grid(n_tau, regime), j_star=j_star, seed=len(out), x_s=x_s, **fac)
                    tag = f"{regime} T={T} n_tau={n_tau}" + (f" j*={j_star}" if j_star is not None else "") + \
                        "".join(f" {k}={v}" for k, v in fac.items())
                    out.append((tag, dict(fac, regime=regime, T=T, n_tau=n_tau), case))
    return out


def call_args(case):
    return {k: case[k] for k in ("h", "data", "weights", "freqs", "taus", "n_valid")}
