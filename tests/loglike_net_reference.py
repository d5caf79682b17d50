"""float64 reference of the coherent network log likelihood (``npf_waveform_loglike_net``) and the input builders its tests share.

``reference`` evaluates the definitions of include/npf_hip.h directly: per detector one complex ``exp`` per (t, j) with the delay in
the argument, ``hh_k`` and ``dd_k`` exactly rounded (``math.fsum``), the detectors' complex sums added times ``C_k`` in ascending k,
and ``loglike_reference._finish`` applied to ``K``, ``HH``, ``DD``; ``snr_det`` from the detectors' own sums at the network's index.
The per-detector terms are ``loglike_reference._terms`` of that detector's data and weights, so with D = 1, ``C = 1`` and no delay
the result is ``loglike_reference.reference`` to the last bit.  ``recurrence`` forms ``kappa_{k,j}`` the way the kernel's first launch
does.  ``wrong`` holds three evaluations that must NOT pass: the incoherent sum, delays of the opposite sign, delays rounded to the
grid.  ``cases`` lists the inputs of the GPU test; tests/test_loglike_net_host.py checks on the CPU that each leaves ``tau_index``
well posed and the phase gate's filter open."""
import math

import torch

import loglike_reference as R1
import match_reference as M

TWO_PI = M.TWO_PI
DTAU = M.DTAU
B = M.B
PHI0 = R1.PHI0
REGIMES = R1.REGIMES
DETS = (1, 2, 3, 8)
# phase spread of the "bigphase" regime, rad.  The single-stream cases use 1e4; with that the recurrence differs from the direct form by
# up to 0.25 of the series-SNR gate (a RELATIVE gate, at grid times where |K_j| nearly cancels): one ulp of an argument of 3e4 rad
# is 3.6e-12.  At 1e3 the arguments (the +-1 s grid start adds 2 pi 512) stay below 8192 rad, an ulp of 9e-13.
BIGPHASE = 1e3
NET_NAMES = ("hh", "dd", "snr", "lnl_max", "lnl_marg", "tau_index", "phase", "lnl_mix", "lnl_max_mix", "hh_det", "snr_det", "dd_det")


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _det_weights(weights, k):
    """The weights of detector k in the form loglike_reference takes: None, [T] or [B, T]."""
    if weights is None:
        return None
    return weights[k] if weights.dim() == 2 else weights[:, k]


def _per_detector(h, data, response, delays, weights, freqs, n_valid):
    """Per detector k: (c [R, T] complex, phi [R, T], hh_k [R], dd_k [R], f [R, T], C [R] complex, delay [R]), float64."""
    Rn, Bn, D = h.shape[0], data.shape[0], data.shape[1]
    task = torch.arange(Rn) % Bn
    resp = response.detach().cpu().double()
    out = []
    for k in range(D):
        c, phi, hh, dd, f = R1._terms(h, data[:, k], _det_weights(weights, k), freqs, n_valid)
        C = torch.complex(resp[:, k, 0], resp[:, k, 1])[task]
        dl = torch.zeros(Rn, dtype=torch.float64) if delays is None else delays.detach().cpu().double()[:, k][task]
        out.append((c, phi, hh, dd, f, C, dl))
    return out


def _direct(c, phi, f, taus, dl):
    if taus is None:  # the one candidate tau = 0: the delay still enters
        return (c * torch.exp(1j * (phi + TWO_PI * f * dl.view(-1, 1)))).sum(1).view(-1, 1)
    tau = (taus[0] + torch.arange(taus[2], dtype=torch.float64) * taus[1]).view(1, 1, -1) + dl.view(-1, 1, 1)
    return (c.unsqueeze(2) * torch.exp(1j * (phi.unsqueeze(2) + TWO_PI * f.unsqueeze(2) * tau))).sum(1)


def _recur(c, phi, f, taus, dl, jc):
    cr, ci = c.real, c.imag
    om = TWO_PI * f
    tau0, dtau, n_tau = taus if taus is not None else (0.0, 0.0, 1)
    ss, sc = torch.sin(om * dtau), torch.cos(om * dtau)
    cols = []
    for j0 in range(0, n_tau, jc):
        arg = phi + om * ((tau0 + j0 * dtau) + dl.view(-1, 1))
        sn, cs = torch.sin(arg), torch.cos(arg)
        zr, zi = cs * cr - sn * ci, cs * ci + sn * cr
        for _ in range(min(jc, n_tau - j0)):
            cols.append(torch.complex(zr.sum(1), zi.sum(1)))
            zr, zi = zr * sc - zi * ss, zr * ss + zi * sc
    return torch.stack(cols, 1)


def _fsum_cols(cols):
    """Exactly rounded sum of a list of [R] tensors."""
    return torch.tensor([math.fsum(v) for v in zip(*(c.tolist() for c in cols))], dtype=torch.float64)


def _network(dets, kappas, Bn, taus):
    """The outputs from the detectors' terms and their complex sums kappa_k [R, n]."""
    K = None
    for (_, _, _, _, _, C, _), kap in zip(dets, kappas):  # ascending k
        term = C.view(-1, 1) * kap
        K = term if K is None else K + term
    HH = _fsum_cols([(C.real ** 2 + C.imag ** 2) * hh for (_, _, hh, _, _, C, _) in dets])
    DD = _fsum_cols([dd for (_, _, _, dd, _, _, _) in dets])
    out = R1._finish(K, HH, DD, Bn, taus)
    idx = out["tau_index"].view(-1, 1)
    hh_det = torch.stack([t[2] for t in dets], 1)
    dd_rows = torch.stack([t[3] for t in dets], 1)
    at = torch.stack([kap.gather(1, idx)[:, 0].abs() for kap in kappas], 1)  # |kappa_{k,j*}| [R, D]
    live = hh_det > 0
    out.update(hh_det=hh_det, dd_det=dd_rows[:Bn], dd_det_rows=dd_rows, kappa_det=torch.stack(kappas, 1),
               snr_det=torch.where(live, at / torch.where(live, hh_det, torch.ones_like(hh_det)).sqrt(), torch.zeros_like(at)),
               optimal_snr_det=torch.stack([t[5].abs() for t in dets], 1) * hh_det.sqrt(), K=K)
    return out


def reference(h, data, response, delays=None, weights=None, freqs=None, taus=None, n_valid=None):
    """Every output of ``npf_waveform_loglike_net`` in float64 on the CPU (dict; the keys of ``loglike_reference.reference`` over the
    network sums, plus ``hh_det`` / ``snr_det`` [R, D], ``dd_det`` [B, D], ``dd_det_rows`` [R, D], ``kappa_det`` [R, D, n], ``K`` [R, n])."""
    dets = _per_detector(h, data, response, delays, weights, freqs, n_valid)
    return _network(dets, [_direct(c, phi, f, taus, dl) for c, phi, _, _, f, _, dl in dets], data.shape[0], taus)


def recurrence(h, data, response, delays=None, weights=None, freqs=None, taus=None, n_valid=None, jc=16):
    """The same outputs with kappa_{k,j} formed as the kernel's first launch forms it: per chunk of ``jc`` shifts one sine / cosine
    pair of phi + 2 pi f (tau_c0 + delay_k) and one of the step 2 pi f dtau, then z <- z s."""
    dets = _per_detector(h, data, response, delays, weights, freqs, n_valid)
    return _network(dets, [_recur(c, phi, f, taus, dl, jc) for c, phi, _, _, f, _, dl in dets], data.shape[0], taus)


def wrong(kind, h, data, response, delays=None, weights=None, freqs=None, taus=None, n_valid=None):
    """Three evaluations that are NOT the network likelihood: ``incoherent`` (sum_k |C_k| |kappa_{k,j}| in place of |K_j|),
    ``sign`` (delays of the opposite sign), ``grid`` (delays rounded to multiples of dtau)."""
    if kind == "sign":
        return reference(h, data, response, None if delays is None else -delays, weights, freqs, taus, n_valid)
    if kind == "grid":
        step = taus[1] if taus is not None else DTAU
        return reference(h, data, response, None if delays is None else torch.round(delays / step) * step, weights, freqs, taus, n_valid)
    assert kind == "incoherent"
    dets = _per_detector(h, data, response, delays, weights, freqs, n_valid)
    kappas = [_direct(c, phi, f, taus, dl) for c, phi, _, _, f, _, dl in dets]
    x = sum(C.abs().view(-1, 1) * kap.abs() for (_, _, _, _, _, C, _), kap in zip(dets, kappas))
    out = _network(dets, kappas, data.shape[0], taus)
    fake = R1._finish(torch.complex(x, torch.zeros_like(x)), out["hh"], out["dd_rows"], data.shape[0], taus)
    return dict(out, **{k: fake[k] for k in ("snr", "lnl_max", "lnl_marg", "lnl_mix", "lnl_max_mix", "tau_index", "series", "x")})


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref):
    """Worst error / gate per quantity ``got`` holds: the gates of ``loglike_reference.ratios`` with HH and DD in place of hh and dd
    (``ref`` carries them under those names), hh_det and dd_det 2^-50 relative, snr_det absolute 1e-10 sqrt(dd_k) + 1e-12: its
    natural scale is snr_det_k <= sqrt(dd_k), and a relative gate would be ill posed where a detector's correlation cancels."""
    out = R1.ratios(got, ref)

    def put(name, d, gate):
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)
        q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
        out[name] = float(q.max()) if q.numel() else 0.0

    for name in ("hh_det", "dd_det", "snr_det", "optimal_snr_det"):
        x = got.get(name)
        if x is None:
            continue
        x = x.detach().cpu()
        assert x.dtype == torch.float64, (name, x.dtype)
        r = ref[name]
        x = x.reshape(r.shape)
        if name == "snr_det":
            put(name, (x - r).abs(), 1e-10 * ref["dd_det_rows"].sqrt() + 1e-12)
        elif name == "optimal_snr_det":
            put(name, (x - r).abs(), 1e-10 * r.abs() + 1e-12)
        else:
            put(name, (x - r).abs(), 2.0 ** -50 * r.abs())
    return out


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _response(D, g, zero_det):
    mod = 0.2 + 1.3 * torch.rand(B, D, generator=g, dtype=torch.float64)
    arg = TWO_PI * torch.rand(B, D, generator=g, dtype=torch.float64)
    resp = torch.stack([mod * torch.cos(arg), mod * torch.sin(arg)], -1)
    if zero_det is not None:
        resp[:, zero_det] = 0.0
    return resp


def _delays(D, g, taus):
    """Uniform in +- 0.37 dtau n_tau (no grid: +- 0.37 DTAU), none within a twentieth of a step of a multiple of dtau."""
    dtau, n = (taus[1], taus[2]) if taus is not None else (DTAU, 1)
    dl = 0.37 * dtau * n * (2.0 * torch.rand(B, D, generator=g, dtype=torch.float64) - 1.0)
    frac = dl / dtau - torch.round(dl / dtau)
    dl = torch.where(frac.abs() < 0.05, dl + 0.25 * dtau, dl)
    assert float((dl / dtau - torch.round(dl / dtau)).abs().min()) >= 0.05
    return dl


def build(regime, T, D=2, n_z=1, h_ld=2, wform=None, fform="T", taus=None, counts=None, j_star=None, seed=0, x_s=24.0, zero_det=None,
          pspread=None):
    """One input set -> dict(h [n_z B, T, h_ld], data [B, D, T, 2], response [B, D, 2] and delays [B, D] (float64; delays None
    without freqs), weights (None, [D, T] for "T", [B, D, T] for "BT"), freqs, taus, n_valid, plus what the regime plants).  The
    regimes are those of ``loglike_reference.build``; "planted" data are d_k = C_k h shifted by tau_{j*} + delay_k and rotated by
    PHI0, so K_{j*} = HH e^{-i PHI0}; "removed" kills a different third of the points in each detector; ``zero_det``: the detector
    whose response is zero."""
    g_ = torch.Generator().manual_seed(77000 + 1000 * REGIMES.index(regime) + seed)
    f = M._freqs(T, fform, g_) if fform is not None else None
    w = None if wform is None else torch.stack([M._weights(T, wform, g_) for _ in range(D)], 0 if wform == "T" else 1)
    resp = _response(D, g_, zero_det)
    dl = _delays(D, g_, taus) if f is not None else None
    pspread = pspread if pspread is not None else (BIGPHASE if regime == "bigphase" else 3.0)
    pred = torch.stack([M._waveform(T, g_, pspread) for _ in range(n_z)])  # [n_z, B, T, 2]
    data = torch.randn(B, D, T, 2, generator=g_)
    plant = {}
    if regime in ("planted", "loud", "quiet", "edge"):
        src = M._waveform(T, g_, pspread)
        j_star = 0 if (j_star is None or taus is None) else j_star
        t_star = 0.0 if taus is None else taus[0] + j_star * taus[1]
        a, p = src[..., 0].double(), src[..., 1].double()  # [B, T]
        when = torch.full((B, D, 1), t_star, dtype=torch.float64) + (dl.view(B, D, 1) if dl is not None else 0.0)
        ff = f.double().expand(B, T).view(B, 1, T) if f is not None else torch.zeros(B, 1, T, dtype=torch.float64)
        ang = p.view(B, 1, T) + TWO_PI * ff * when + PHI0
        C = torch.complex(resp[..., 0], resp[..., 1]).view(B, D, 1)
        d64 = C * (a.view(B, 1, T) * torch.exp(1j * ang))
        d64 = torch.stack([d64.real, d64.imag], -1)  # [B, D, T, 2]
        data = d64.float()
        pred = src.unsqueeze(0).repeat(n_z, 1, 1, 1)
        plant["j_star"] = j_star
        if regime == "planted":
            plant["data64"] = d64
        else:  # scale template and data so that x* ~ HH sits where the regime wants it
            wd = torch.ones(B, D, T) if w is None else w.expand(B, D, T)
            c2 = (resp ** 2).sum(-1)  # [B, D]
            HH0 = (c2 * (wd.double() * a.view(B, 1, T) ** 2).sum(2)).sum(1)  # [B], at full counts
            target = {"loud": 1e4, "quiet": 1e-3, "edge": x_s}[regime]
            k = (target / HH0).sqrt().float()
            fac = {"loud": (1.0, 0.6, 0.3), "quiet": (1.0, 0.9, 1.1), "edge": (1.02, 0.98, 1.5)}[regime]
            data = data * k.view(B, 1, 1, 1)
            pred = pred.clone()
            for s in range(n_z):
                pred[s, ..., 0] = pred[s, ..., 0] * k.view(B, 1) * fac[s % 3]
    h = torch.randn(n_z * B, T, h_ld, generator=g_)
    h[..., :2] = pred.reshape(n_z * B, T, 2)
    out = dict(h=h, data=data.clone(), response=resp, delays=dl, weights=w, freqs=f, taus=taus,
               n_valid=None if counts is None else torch.tensor(counts, dtype=torch.int32), **plant)
    if regime == "removed":  # a different third of the points per detector: weight 0, negative, NaN or Inf, NaN in what is not read
        assert w is not None
        kill = torch.rand(w.shape, generator=g_) < 1.0 / 3.0
        kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])[torch.randint(0, 4, w.shape, generator=g_)]
        out["weights"] = torch.where(kill, kinds, w)
        out["kill"] = kill.expand(B, D, T).clone()
    if regime == "degenerate":  # all weights zero: of the last task ([B, D, T] weights) or of every task ([D, T])
        assert w is not None
        out["weights"] = w.clone()
        if w.dim() == 3:
            out["weights"][-1] = 0.0
        else:
            out["weights"][:] = 0.0
    if regime == "removed":
        poison(out, math.nan)
    return out


def poison(case, value):
    """Write ``value`` into everything the kernel promises not to read (in place): per detector the data of its dead points (removed
    by ``kill`` or beyond the task's count); of ``h`` and ``freqs`` the points that are dead for every detector (``freqs`` [T]: for
    every task as well).  The weights keep what makes the points dead."""
    Bn, D, T = case["data"].shape[:3]
    dead = case["kill"].clone() if "kill" in case else torch.zeros(Bn, D, T, dtype=torch.bool)
    if case["n_valid"] is not None:
        dead |= (torch.arange(T).view(1, 1, T) >= case["n_valid"].long().clamp(0, T).view(Bn, 1, 1))
    case["data"][dead] = value
    all_dead = dead.all(1)  # [B, T]
    n_z = case["h"].shape[0] // Bn
    case["h"].view(n_z, Bn, T, -1)[:, all_dead] = value
    if case["freqs"] is not None:
        f = case["freqs"].clone()
        f[all_dead if f.dim() == 2 else all_dead.all(0)] = value
        case["freqs"] = f
    return case


grid = M.grid


def cases(jc, x_s):
    """The inputs of the GPU test: every regime at T in {37, 200} and n_tau in {none, 1, 5, jc - 1, jc, jc + 1, 257}; D in
    {1, 2, 3, 8}, counts (T, 17, 0) or none, n_z in {1, 3}, h_ld in {2, 4} and the form of weights and freqs rotate with the regime's
    case number at different periods, as in ``loglike_reference.cases``; the planted indices are those of that list.  In one case
    per regime (the regime's case 5) the first detector's response is zero.  -> list of (tag, factors, case)."""
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
                    D = DETS[(i + i // 4 + 1) % 4]
                    fac = dict(D=D, counts=(None, (T, 17, 0))[i % 2], n_z=(1, 3)[(i // 2) % 2], h_ld=(2, 4)[(i + i // 4) % 2],
                               wform=w_opts[(i // 4) % 2 if need_w else i % 3], fform=fform, zero_det=0 if (i == 5 and D > 1) else None)
                    i += 1
                    case = build(regime, T, taus=grid(n_tau, regime), j_star=j_star, seed=len(out) + SEED_SHIFT.get(len(out), 0),
                                 x_s=x_s, **fac)
                    tag = f"{regime} T={T} n_tau={n_tau}" + (f" j*={j_star}" if j_star is not None else "") + \
                        "".join(f" {k}={v}" for k, v in fac.items())
                    out.append((tag, dict(fac, regime=regime, T=T, n_tau=n_tau), case))
    return out


# case number -> what is added to its seed: the cases whose first seed left tau_index ill posed or closed the phase gate's filter
# (tests/test_loglike_net_host.py checks both for every case)
SEED_SHIFT = {}


def call_args(case):
    return {k: case[k] for k in ("h", "data", "response", "delays", "weights", "freqs", "taus", "n_valid")}
