"""float64 reference of the sky-grid network likelihood (``npf_waveform_loglike_sky``) and the input builders its tests share.

``reference`` evaluates the definitions of include/npf_hip.h directly: per pixel and detector one complex ``exp`` per (t, j) with
``tau_j + Delta_{p,k}`` in the argument (``loglike_net_reference._direct``), ``hh_k`` exactly rounded (``math.fsum``, through
``loglike_reference._terms``), the detectors' sums added times ``C_{p,k}`` in ascending k, ``ln I0`` of ``loglike_reference.log_i0``
and ``torch.logsumexp`` over the grid times, the pixels and the latent samples.  ``wrong`` holds three evaluations that must NOT pass:
the incoherent sum, delays of the opposite sign, pixel 0's delays at every pixel.  ``build`` plants a signal: the data of detector k
are ``C_{p0,k} h`` shifted by ``tau_{j0} + Delta_{p0,k}`` plus small noise, so the best pixel and the best grid time are known and
lead their runners-up by a wide margin; tests/test_loglike_sky_host.py checks on the CPU that every set of the GPU test is well posed.

Gates (``ratios``), the constants of ``loglike_reference.ratios``: lnl_sky, lnl_sky_mix (and u = post + lnl_sky) |d| <= 1e-10 scale +
1e-12 with scale = max_p (sqrt(HH_p DD) + HH_p / 2) over the live pixels of the row (the mix: the largest among the task's rows);
post, post_mix twice that; snr, snr_map 1e-10 relative + 1e-12; the indices exact; -inf is met by -inf only."""
import math

import torch

import loglike_net_reference as N
import loglike_reference as R1
import match_reference as M

TWO_PI = M.TWO_PI
DTAU = M.DTAU
PHI0 = R1.PHI0
DOUBLES = ("lnl_sky", "snr", "lnl_sky_mix", "post", "post_mix", "snr_map")


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _dets(h, data, weights, freqs, n_valid):
    """Per detector k: (c [R, T] complex = w_k A conj(d_k) with dead points at 0, phi [R, T], hh_k [R], dd_k [R], f [R, T])."""
    return [R1._terms(h, data[:, k], N._det_weights(weights, k), freqs, n_valid) for k in range(data.shape[1])]


def _live_pixels(log_prior, P):
    if log_prior is None:
        return torch.ones(P, dtype=torch.bool), torch.full((P,), -math.log(P), dtype=torch.float64)
    lp = log_prior.detach().cpu().double()
    return torch.isfinite(lp), lp


def _pixel_sums(dets, resp, delays, taus, mode="coherent"):
    """x [R, P, n] = |K_{j,p}| (``incoherent``: sum_k |C_{p,k}| |kappa_{k,j}|) and HH [R, P], pixel by pixel."""
    Rn, P = dets[0][0].shape[0], resp.shape[0]
    xs, HHs = [], []
    for p in range(P):
        K = None
        for k, (c, phi, hh, _, f) in enumerate(dets):  # ascending k
            C = torch.complex(resp[p, k, 0], resp[p, k, 1])
            kap = N._direct(c, phi, f, taus, delays[p, k].repeat(Rn))
            term = C.abs() * kap.abs() if mode == "incoherent" else C * kap
            K = term if K is None else K + term
        xs.append(K.abs())
        HHs.append(N._fsum_cols([(resp[p, k, 0] ** 2 + resp[p, k, 1] ** 2) * hh for k, (_, _, hh, _, _) in enumerate(dets)]))
    return torch.stack(xs, 1), torch.stack(HHs, 1)


def _finish(x, HH, DD, live, lp, Bn):
    """The outputs from x [R, P, n], HH [R, P], DD [R], the pixels' liveness and log prior mass."""
    Rn, P, n = x.shape
    n_z = Rn // Bn
    ninf = torch.full((), -math.inf, dtype=torch.float64)
    L = R1.log_i0(x) - 0.5 * HH.unsqueeze(2)
    u = torch.where(live.view(1, P), lp.view(1, P) + torch.logsumexp(L, 2) - math.log(n), ninf)
    lnl_sky = torch.logsumexp(u, 1) if live.any() else torch.full((Rn,), -math.inf, dtype=torch.float64)
    best_u = u.max(1).values
    pix = (u == best_u.view(-1, 1)).double().argmax(1) if live.any() else torch.zeros(Rn, dtype=torch.long)
    xm = x.max(2).values
    j_first = (x == xm.unsqueeze(2)).double().argmax(2)  # the smallest index at the maximum [R, P]
    ok = live.view(1, P) & (HH > 0)
    snr_map = torch.where(ok, xm / torch.where(ok, HH, torch.ones_like(HH)).sqrt(), torch.zeros_like(xm))
    at = pix.view(-1, 1)
    tau_index = torch.where(live[pix], j_first.gather(1, at)[:, 0], torch.zeros(Rn, dtype=torch.long))
    post = torch.where(live.view(1, P), u - lnl_sky.view(-1, 1), ninf) if live.any() else torch.full_like(u, -math.inf)
    mix = torch.logsumexp(lnl_sky.view(n_z, Bn), 0) - math.log(n_z) if live.any() else torch.full((Bn,), -math.inf, dtype=torch.float64)
    u_mix = torch.logsumexp(u.view(n_z, Bn, P), 0) - math.log(n_z)
    post_mix = torch.where(live.view(1, P), u_mix - mix.view(-1, 1), ninf) if live.any() else torch.full((Bn, P), -math.inf,
                                                                                                           dtype=torch.float64)
    term = torch.where(live.view(1, P), (HH * DD.view(-1, 1)).sqrt() + 0.5 * HH, torch.zeros_like(HH))
    return dict(u=u, lnl_sky=lnl_sky, pix_index=pix, tau_index=tau_index, snr=snr_map.gather(1, at)[:, 0], lnl_sky_mix=mix, post=post,
                post_mix=post_mix, snr_map=snr_map, x=x, HH=HH, DD=DD, live=live, scale=term.max(1).values, tau_map=j_first)


def _prepared(response, delays, log_prior):
    resp, dl = response.detach().cpu().double(), delays.detach().cpu().double()
    live, lp = _live_pixels(log_prior, resp.shape[0])
    # a dead pixel's response and delays are not read: zeros stand in for whatever they hold
    return torch.where(live.view(-1, 1, 1), resp, torch.zeros_like(resp)), torch.where(live.view(-1, 1), dl, torch.zeros_like(dl)), live, lp


def reference(h, data, response, delays, log_prior=None, weights=None, freqs=None, taus=None, n_valid=None, mode="coherent"):
    """Every output of ``npf_waveform_loglike_sky`` in float64 on the CPU (dict; plus ``u`` [R, P], ``x`` [R, P, n], ``HH`` [R, P],
    ``DD`` [R], ``live`` [P], ``tau_map`` [R, P]: the first index of max_j x, and the gate's ``scale`` [R])."""
    dets = _dets(h, data, weights, freqs, n_valid)
    resp, dl, live, lp = _prepared(response, delays, log_prior)
    x, HH = _pixel_sums(dets, resp, dl, taus, mode)
    DD = N._fsum_cols([dd for (_, _, _, dd, _) in dets])
    return _finish(x, HH, DD, live, lp, data.shape[0])


def wrong(kind, h, data, response, delays, log_prior=None, weights=None, freqs=None, taus=None, n_valid=None):
    """Three evaluations that are NOT the sky likelihood: ``incoherent`` (moduli added per detector), ``sign`` (delays negated),
    ``shared`` (pixel 0's delays used for every pixel)."""
    if kind == "sign":
        return reference(h, data, response, -delays, log_prior, weights, freqs, taus, n_valid)
    if kind == "shared":
        return reference(h, data, response, delays[:1].expand_as(delays).clone(), log_prior, weights, freqs, taus, n_valid)
    assert kind == "incoherent"
    return reference(h, data, response, delays, log_prior, weights, freqs, taus, n_valid, mode="incoherent")


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, lnl_gate=1e-10, lnl_floor=1e-12):
    """Worst error / gate per quantity ``got`` holds (a mapping name -> tensor or None); ``u`` is formed from post + lnl_sky when both
    are there.  Where the reference is -inf only -inf passes (ratio 0, else inf); a value that is not finite elsewhere: inf."""
    out = {}
    Bn = ref["lnl_sky_mix"].shape[0]
    scale = ref["scale"]
    task_scale = scale.view(-1, Bn).max(0).values

    def put(name, x, r, gate):
        x, r = x.detach().cpu(), r
        assert x.dtype == torch.float64 and x.shape == r.shape, (name, x.dtype, x.shape, r.shape)
        gate = gate.expand_as(r) if isinstance(gate, torch.Tensor) else torch.full_like(r, gate)
        minus = r == -math.inf
        d = torch.where(minus, torch.zeros_like(r), (x - r).abs())
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)
        q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
        q = torch.where(minus, torch.where(x == -math.inf, torch.zeros_like(q), torch.full_like(q, math.inf)), q)
        out[name] = float(q.max()) if q.numel() else 0.0

    g_row, g_task = lnl_gate * scale + lnl_floor, lnl_gate * task_scale + lnl_floor
    for name in ("pix_index", "tau_index"):
        if got.get(name) is not None:
            out[name] = 0.0 if torch.equal(got[name].detach().cpu().reshape(-1).long(), ref[name].long()) else math.inf
    if got.get("lnl_sky") is not None:
        put("lnl_sky", got["lnl_sky"].reshape(-1), ref["lnl_sky"], g_row)
    if got.get("lnl_sky_mix") is not None:
        put("lnl_sky_mix", got["lnl_sky_mix"].reshape(-1), ref["lnl_sky_mix"], g_task)
    if got.get("post") is not None:
        post = got["post"].detach().cpu().reshape(ref["post"].shape)
        put("post", post, ref["post"], 2.0 * g_row.view(-1, 1))
        if got.get("lnl_sky") is not None:
            put("u", post + got["lnl_sky"].detach().cpu().reshape(-1, 1), ref["u"], g_row.view(-1, 1))
    if got.get("post_mix") is not None:
        put("post_mix", got["post_mix"].reshape(ref["post_mix"].shape), ref["post_mix"], 2.0 * g_task.view(-1, 1))
    for name in ("snr", "snr_map"):
        if got.get(name) is not None:
            r = ref[name]
            put(name, got[name].reshape(r.shape), r, 1e-10 * r.abs() + 1e-12)
    return out


def margins(ref, tie=False):
    """How well posed the indices are: (the lead of the best pixel's u over the runner-up, in units of the u gate, the smallest over
    the rows; the relative lead of the best x_j over the runner-up at the best pixel, the smallest over the rows).  inf where there
    is no runner-up (one live pixel, one grid time)."""
    u, x = ref["u"], ref["x"]
    gate = 1e-10 * ref["scale"] + 1e-12
    lead_u = math.inf
    if int(ref["live"].sum()) >= 2:
        top = u.topk(2, dim=1).values
        lead_u = float(((top[:, 0] - top[:, 1]) / gate).min())
    lead_x = math.inf
    if x.shape[2] >= 2 and ref["live"].any():
        xp = x.gather(1, ref["pix_index"].view(-1, 1, 1).expand(-1, 1, x.shape[2]))[:, 0]  # [R, n] at the best pixel
        top = xp.topk(2, dim=1).values
        keep = top[:, 0] > 0
        if keep.any():
            lead_x = float(((top[:, 0] - top[:, 1]) / top[:, 0])[keep].min())
    return lead_u, lead_x


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def grid(n_tau):
    """(tau0, dtau, n_tau) with tau = 0 on the grid (index min(2, n_tau - 1)), or None."""
    return None if n_tau is None else (-min(2, n_tau - 1) * DTAU, DTAU, n_tau)


def sky(P, D, g, span=6.0):
    """A grid of P pixels: response [P, D, 2] (moduli in [0.4, 1.4], any argument), delays [P, D] within +- span DTAU, none within
    a twentieth of a step of a multiple of DTAU, float64."""
    mod = 0.4 + torch.rand(P, D, generator=g, dtype=torch.float64)
    arg = TWO_PI * torch.rand(P, D, generator=g, dtype=torch.float64)
    resp = torch.stack([mod * torch.cos(arg), mod * torch.sin(arg)], -1)
    dl = span * DTAU * (2.0 * torch.rand(P, D, generator=g, dtype=torch.float64) - 1.0)
    frac = dl / DTAU - torch.round(dl / DTAU)
    dl = torch.where(frac.abs() < 0.05, dl + 0.25 * DTAU, dl)
    return resp, dl


def plant(wave, resp_p, dl_p, f, tau_star):
    """float64 data [B, D, T, 2] of the waveforms ``wave`` [B, T, 2] = (A, phi) seen through one pixel: detector k holds C_k A
    e^{i (phi + 2 pi f (tau* + Delta_k) + PHI0)}."""
    Bn, T = wave.shape[:2]
    a, p = wave[..., 0].double(), wave[..., 1].double()
    ang = p.view(Bn, 1, T) + TWO_PI * f.double().view(1, 1, T) * (tau_star + dl_p.view(1, -1, 1)) + PHI0
    d = torch.complex(resp_p[:, 0], resp_p[:, 1]).view(1, -1, 1) * (a.view(Bn, 1, T) * torch.exp(1j * ang))
    return torch.stack([d.real, d.imag], -1)


def _waveform(Bn, T, g, spread=3.0):
    amp = torch.linspace(1.0, 3.0, T).pow(-7.0 / 6.0).view(1, T) * (1.0 + 0.1 * torch.randn(Bn, T, generator=g)).abs()
    return torch.stack([amp, spread * torch.randn(Bn, T, generator=g)], -1)


def build(Bn=3, n_z=1, T=37, D=3, P=5, n_tau=5, h_ld=2, wform=None, prior=False, seed=0, p0=None, j0=None, noise=0.02, data_scale=None,
          counts=None, jitter=0.05):
    """One input set -> dict(h [n_z Bn, T, h_ld], data [Bn, D, T, 2], response [P, D, 2], delays [P, D], log_prior (None or [P]),
    weights (None, [D, T] for "T", [Bn, D, T] for "BT"), freqs [T], taus, n_valid, p0, j0).  Every latent sample predicts the planted
    waveform with ``jitter`` relative scatter in the amplitude; ``data_scale`` [Bn]: a factor on every task's data."""
    g = torch.Generator().manual_seed(91000 + seed)
    f = torch.linspace(20.0, 512.0, T) if T > 1 else torch.tensor([20.0])
    taus = grid(n_tau)
    resp, dl = sky(P, D, g)
    p0 = P // 2 if p0 is None else p0
    j0 = 0 if taus is None else (min(2, n_tau - 1) if j0 is None else j0)
    src = _waveform(Bn, T, g)
    d64 = plant(src, resp[p0], dl[p0], f, 0.0 if taus is None else taus[0] + j0 * taus[1])
    data = d64 + noise * torch.randn(Bn, D, T, 2, generator=g, dtype=torch.float64)
    if data_scale is not None:
        data = data * torch.tensor(data_scale, dtype=torch.float64).view(Bn, 1, 1, 1)
    pred = src.unsqueeze(0).repeat(n_z, 1, 1, 1)
    pred[..., 0] = pred[..., 0] * (1.0 + jitter * torch.randn(n_z, Bn, 1, generator=g))
    h = torch.randn(n_z * Bn, T, h_ld, generator=g)
    h[..., :2] = pred.reshape(n_z * Bn, T, 2)
    w = None
    if wform is not None:
        w = 0.5 + torch.rand((D, T) if wform == "T" else (Bn, D, T), generator=g)
    lp = None
    if prior:
        mass = 0.2 + torch.rand(P, generator=g, dtype=torch.float64)
        lp = torch.log(mass / mass.sum())
    return dict(h=h, data=data.float(), response=resp, delays=dl, log_prior=lp, weights=w, freqs=f, taus=taus,
                n_valid=None if counts is None else torch.tensor(counts, dtype=torch.int32), p0=p0, j0=j0)


def kill_points(case, seed=0):
    """Dead points, in place: a third of the weights (another third per detector) become 0, negative, NaN or Inf, and NaN goes into
    everything the kernel promises not to read -- the data of a detector's dead points (those beyond the task's count as well) and
    ``h`` where the point is dead for every detector.  ``freqs`` stays finite: the pixel operand reads it everywhere."""
    g = torch.Generator().manual_seed(4400 + seed)
    w = case["weights"]
    Bn, D, T = case["data"].shape[:3]
    kill = torch.rand(w.shape, generator=g) < 1.0 / 3.0
    kill[..., 1::7] = True  # (some points dead for every detector)
    kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])[torch.randint(0, 4, w.shape, generator=g)]
    case["weights"] = torch.where(kill, kinds, w)
    dead = kill.expand(Bn, D, T).clone()
    if case["n_valid"] is not None:
        dead |= torch.arange(T).view(1, 1, T) >= case["n_valid"].long().clamp(0, T).view(Bn, 1, 1)
    case["dead"] = dead
    return poison(case, math.nan)


def poison(case, value):
    Bn, D, T = case["data"].shape[:3]
    dead = case["dead"]
    case["data"][dead] = value
    n_z = case["h"].shape[0] // Bn
    case["h"].view(n_z, Bn, T, -1)[:, dead.all(1)] = value
    return case


def call_args(case):
    return {k: case[k] for k in ("h", "data", "response", "delays", "log_prior", "weights", "freqs", "taus", "n_valid")}


def sweep_sets(jc):
    """The axis sweeps of the GPU test, one per axis with the others at small odd values, and the combined set: -> list of (tag,
    case).  h_ld, the form of the weights and the prior rotate with the set's number."""
    out = []

    def add(tag, **kw):
        i = len(out)
        kw.setdefault("h_ld", (2, 4)[i % 2])
        kw.setdefault("wform", (None, "T", "BT")[i % 3])
        kw.setdefault("prior", bool((i // 2) % 2))
        out.append((tag, build(seed=i, **kw)))

    for Bn, n_z in ((1, 1), (5, 3), (16, 1), (17, 1), (11, 3)):  # rows 1, 15, 16, 17, 33
        add(f"rows={Bn * n_z} n_z={n_z}", Bn=Bn, n_z=n_z)
    for P in (1, 15, 16, 17, 40):
        add(f"P={P}", P=P)
    for D in (1, 2, 3, 8):
        add(f"D={D}", D=D)
    for T in (1, 2, 3, 5, 127, 128, 129):
        add(f"T={T}", T=T, n_tau=5 if T > 1 else 1)  # (one point: |K_j| does not depend on j, so a grid of one time)
    for n_tau in (None, 1, jc - 1, jc, jc + 1, 2 * jc + 1):
        add(f"n_tau={n_tau}", n_tau=n_tau, j0=None if n_tau is None else n_tau - 1)
    add("combined 33 x 40 x 3 x 129 x 17", Bn=11, n_z=3, P=40, D=3, T=129, n_tau=17, j0=11, h_ld=4, wform="BT", prior=True)
    return out


# data scales that put x = |K| of the four tasks below (0.1, 20 at the peak), across (30 at the peak, the rest of the grid below)
# and far above (1e6) the switch point of ln I0 at 24: with the planted signal x_peak = scale * HH
def regime_set(T=37, D=3, n_tau=5, P=5):
    case = build(Bn=4, n_z=2, T=T, D=D, P=P, n_tau=n_tau, wform="T", prior=True, seed=77)
    HH0 = reference(**call_args(case))["HH"][:4, case["p0"]]  # of the first latent sample
    scales = [t / float(hh) for t, hh in zip((0.1, 20.0, 30.0, 1e6), HH0)]
    return build(Bn=4, n_z=2, T=T, D=D, P=P, n_tau=n_tau, wform="T", prior=True, seed=77, data_scale=scales)


def dead_points_set():
    """Points with weight 0, negative, NaN or Inf (another third per detector) and points beyond the counts, NaN planted there."""
    return kill_points(build(Bn=3, n_z=2, T=37, D=3, P=5, n_tau=5, h_ld=4, wform="BT", prior=True, seed=101, counts=(37, 17, 9)), 1)


def base_set():
    """Nine rows in one tile, seven pixels: the set the dead-pixel, isolation and repeat tests start from."""
    return build(Bn=3, n_z=3, T=37, D=3, P=7, n_tau=5, h_ld=2, wform="T", prior=True, seed=102)


def perm_set():
    """33 rows x 40 pixels: three row tiles, three pixel tiles, two workgroups of the correlation launch."""
    return build(Bn=11, n_z=3, T=37, D=2, P=40, n_tau=9, h_ld=2, wform="BT", prior=True, seed=103, j0=6)


def gpu_sets(jc):
    """Every input set of the GPU test whose indices must be well posed -> list of (tag, case)."""
    return sweep_sets(jc) + [("ln I0 regimes", regime_set()), ("dead points", dead_points_set()), ("base", base_set()),
                             ("permutations", perm_set())]
