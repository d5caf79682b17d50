"""float64 reference of the joint sky and distance marginal (``npf_waveform_loglike_sky_dist``), its gates and the input sets its
tests share.

``reference`` evaluates the definitions of include/npf_hip.h directly on what ``loglike_sky_reference.reference`` returns (``x``
[R, P, n], ``HH``, ``DD``, ``live``): ``ln I0(a_i x_{p,j})`` for every (row, pixel, scale, grid time) with
``loglike_reference.log_i0``, ``torch.logsumexp`` over j, then over i, over p, over both; dead scales by
``loglike_dist_reference.live_mask``.  ``one_pass`` restates the kernel's order (the x*-shifted sum, mm_p / s_p, the differences
before the logs) in float64 torch.  ``wrong`` holds four evaluations that must NOT pass.

Gates (``ratios``).  g_r = 1e-10 S_r + 1e-12 with S_r = max over live (p, i) of (a_i sqrt(HH_p DD) + a_i^2 HH_p / 2 + |ln pi_i|):
lnl_vol and w = post_joint + lnl_vol at g_r; post_sky, post_dist, post_joint at 2 g_r; lnl and the mixtures with the task's largest
S_r; snr, scale_hat 1e-10 |ref| + 1e-12; the indices exact; -inf is met by -inf only.

The moments are not logs; their gates follow from the log gates.  The weight of scale i at pixel p is q_i = exp(w_{p,i} - u_sky[p]),
sum_i q_i = 1.  w and u_sky are each within g_r, so the exponent is within 2 g_r and |dq_i| <= (e^{2 g} - 1) q_i <= 4 g q_i for
g <= 1/4.  With v_i = 1 / a_i:
  dist_mean = sum_i v_i q_i:            |d mean| <= sum_i v_i |dq_i| <= 4 g_r max_live(v)                     (+ 1e-12 |ref| rounding)
  dist_std^2 = sum_i (v_i - mean)^2 q_i: the term linear in d mean vanishes (sum_i (v_i - mean) q_i = 0), which leaves
               sum_i (v_i - mean)^2 |dq_i| + (d mean)^2 <= 4 g max(v)^2 + 16 g^2 max(v)^2 <= 8 g_r max_live(v)^2   (+ 1e-12 ref^2)
so the spread is compared squared.  tests/test_loglike_sky_dist_host.py checks that float64 itself stays below 0.1 of every gate."""
import math

import torch

import loglike_dist_reference as DR
import loglike_reference as R1
import loglike_sky_reference as S

NEG_INF = -math.inf
SC = 8  # NPF_SKYD_SC
DATA_SCALE = DR.DATA_SCALE  # the peak of the scale posterior sits at a = 1.13 / (1 + jitter): off the symmetry of the geometric grids
POSTS = ("post_sky", "post_dist", "post_joint")
MIXES = ("post_sky_mix", "post_dist_mix")


def _lse(t, dims):
    """logsumexp over ``dims`` that gives -inf (not NaN) where everything is -inf."""
    m = t.amax(dims, keepdim=True)
    m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (torch.log(torch.exp(t - m0).sum(dims, keepdim=True)) + m0).squeeze(dims)


def _minus(u, v):
    """u - v with -inf where u is -inf (whatever v is)."""
    return torch.where(u == NEG_INF, torch.full_like(u, NEG_INF), u - torch.where(v == NEG_INF, torch.zeros_like(v), v))


def evidence(sky, scales, log_prior_scale, log_prior, mode="joint"):
    """w [R, P, n_a] (-inf at dead pixels and dead scales), the scales' liveness [n_a] and the pixels' log prior mass [P]."""
    x, HH, live_p = sky["x"], sky["HH"], sky["live"]
    Rn, P, n = x.shape
    _, lp = S._live_pixels(log_prior, P)
    a, lpi = scales.detach().cpu().double(), log_prior_scale.detach().cpu().double()
    live_i = DR.live_mask(a, lpi)
    a0, lpi0 = torch.where(live_i, a, torch.ones_like(a)), torch.where(live_i, lpi, torch.zeros_like(lpi))
    lp0 = torch.where(live_p, lp, torch.zeros_like(lp))
    xz = torch.where((HH == 0).unsqueeze(2), torch.zeros_like(x), x)  # HH == 0: x_j = 0
    if mode == "xstar":  # WRONG: the grid time maximised, not marginalised
        over_j = R1.log_i0(a0.view(1, 1, -1) * xz.max(2).values.unsqueeze(2))
    else:
        over_j = torch.logsumexp(R1.log_i0(a0.view(1, 1, -1, 1) * xz.unsqueeze(2)), 3) - math.log(n)
    quad = 0.5 * (a0 if mode == "aHH" else a0 ** 2).view(1, 1, -1) * HH.unsqueeze(2)
    w = (0.0 if mode == "noprior" else lp0.view(1, P, 1)) + lpi0.view(1, 1, -1) + over_j - quad
    mask = live_p.view(1, P, 1) & live_i.view(1, 1, -1)
    return torch.where(mask, w, torch.full_like(w, NEG_INF)), live_i, a


def finish(sky, w, live_i, a, Bn, mode="joint"):
    Rn, P, n_a = w.shape
    n_z = Rn // Bn
    live_p = sky["live"]
    u_sky, u_dist, vol = _lse(w, (2,)), _lse(w, (1,)), _lse(w, (1, 2))
    none = vol == NEG_INF
    pix = torch.where(none, torch.zeros(Rn, dtype=torch.long), (u_sky == u_sky.max(1, keepdim=True).values).double().argmax(1))
    idx = torch.where(none, torch.zeros(Rn, dtype=torch.long), (u_dist == u_dist.max(1, keepdim=True).values).double().argmax(1))
    at = pix.view(-1, 1)
    HH_at, xm_at = sky["HH"].gather(1, at)[:, 0], sky["x"].max(2).values.gather(1, at)[:, 0]
    ok = ~none & live_p[pix] & (HH_at > 0)
    one, zero = torch.ones_like(HH_at), torch.zeros_like(HH_at)
    snr = torch.where(ok, xm_at / torch.where(ok, HH_at, one).sqrt(), zero)
    scale_hat = torch.where(ok, xm_at / torch.where(ok, HH_at, one), zero)
    tau_index = torch.where(~none & live_p[pix], sky["tau_map"].gather(1, at)[:, 0], torch.zeros(Rn, dtype=torch.long))
    post_sky, post_dist = _minus(u_sky, vol.view(-1, 1)), _minus(u_dist, vol.view(-1, 1))
    post_joint = _minus(w, vol.view(-1, 1, 1))
    if mode == "separable":  # WRONG: the product of the two marginals
        post_joint = post_sky.unsqueeze(2) + post_dist.unsqueeze(1)
    q = torch.exp(_minus(w, u_sky.unsqueeze(2)))  # the weights of the scales at every pixel (0 at dead entries)
    v = torch.where(live_i, 1.0 / torch.where(live_i, a, torch.ones_like(a)), torch.zeros_like(a)).view(1, 1, -1)
    mean = (v * q).sum(2)
    std = (((v - mean.unsqueeze(2)) ** 2) * q).sum(2).sqrt()
    lnl = _lse(vol.view(n_z, Bn), (0,)) - math.log(n_z)
    sky_mix = _minus(_lse(u_sky.view(n_z, Bn, P), (0,)) - math.log(n_z), lnl.view(-1, 1))
    dist_mix = _minus(_lse(u_dist.view(n_z, Bn, n_a), (0,)) - math.log(n_z), lnl.view(-1, 1))
    HH, DD = sky["HH"], sky["DD"]
    term = a.view(1, 1, -1) * (HH * DD.view(-1, 1)).sqrt().unsqueeze(2) + 0.5 * (a ** 2).view(1, 1, -1) * HH.unsqueeze(2)
    mask = live_p.view(1, P, 1) & live_i.view(1, 1, -1)
    return dict(w=w, u_sky=u_sky, u_dist=u_dist, lnl_vol=vol, pix_index=pix, scale_index=idx, tau_index=tau_index, snr=snr,
                scale_hat=scale_hat, lnl=lnl, post_sky=post_sky, post_dist=post_dist, post_joint=post_joint, dist_mean=mean,
                dist_std=std, post_sky_mix=sky_mix, post_dist_mix=dist_mix, live_p=live_p, live_i=live_i, mask=mask,
                _term=term, x=sky["x"], HH=HH, DD=DD,
                v_max=float(v.max()) if live_i.any() else 0.0)


def reference(h, data, response, delays, scales, log_prior_scale, log_prior=None, weights=None, freqs=None, taus=None, n_valid=None,
              mode="joint", sky=None):
    """Every output of ``npf_waveform_loglike_sky_dist`` in float64 on the CPU (dict; plus ``w``, ``u_sky``, ``u_dist``, the masks
    and the gate scale ``S`` [R]).  ``sky``: a ``loglike_sky_reference.reference`` of the same inputs, to share."""
    if sky is None:
        sky = S.reference(h, data, response, delays, log_prior, weights, freqs, taus, n_valid)
    w, live_i, a = evidence(sky, scales, log_prior_scale, log_prior, mode)
    out = finish(sky, w, live_i, a, data.shape[0], mode)
    lpi = log_prior_scale.detach().cpu().double()
    term = out.pop("_term") + torch.where(live_i, lpi, torch.zeros_like(lpi)).abs().view(1, 1, -1)
    out["S"] = torch.where(out["mask"], term, torch.zeros_like(term)).amax((1, 2))
    out["sky"] = sky
    return out


def wrong(kind, case, sky=None):
    """Four evaluations that are NOT the joint marginal: ``xstar`` (the scale marginal at the best grid time only), ``aHH`` (a HH
    in place of a^2 HH), ``noprior`` (the pixel prior dropped), ``separable`` (post_sky + post_dist in place of post_joint)."""
    assert kind in ("xstar", "aHH", "noprior", "separable")
    return reference(**call_args(case), mode=kind, sky=sky)


def one_pass(ref, scales, log_prior_scale, log_prior):
    """The kernel's order in float64 torch: x* first, the shifted sum over j with every term <= 1, w in the kernel's bracketing,
    mm_p / s_p over the scales, M = max w, total = sum_p exp(mm_p - M) s_p, the posteriors as differences first."""
    sky = ref["sky"]
    x, HH, live_p = sky["x"], sky["HH"], sky["live"]
    Rn, P, n = x.shape
    _, lp = S._live_pixels(log_prior, P)
    a, lpi = scales.detach().cpu().double(), log_prior_scale.detach().cpu().double()
    live_i = DR.live_mask(a, lpi)
    a0, lpi0 = torch.where(live_i, a, torch.ones_like(a)).view(1, 1, -1), torch.where(live_i, lpi, torch.zeros_like(lpi)).view(1, 1, -1)
    xz = torch.where((HH == 0).unsqueeze(2), torch.zeros_like(x), x)
    l0 = R1.log_i0(a0 * xz.max(2).values.unsqueeze(2))  # [R, P, n_a]
    terms = torch.exp(R1.log_i0(a0.unsqueeze(3) * xz.unsqueeze(2)) - l0.unsqueeze(3))
    assert float(terms.max()) <= 1.0 + 1e-15
    w = torch.where(live_p, lp, torch.zeros_like(lp)).view(1, P, 1) + ((lpi0 + (l0 - (a0 * a0) * (0.5 * HH).unsqueeze(2))) +
                                                                       (torch.log(terms.sum(3)) - math.log(n)))
    mask = live_p.view(1, P, 1) & live_i.view(1, 1, -1)
    w = torch.where(mask, w, torch.full_like(w, NEG_INF))
    fin = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))  # noqa: E731
    mm = w.amax(2)
    e = torch.where(w == NEG_INF, torch.zeros_like(w), torch.exp(w - fin(mm).unsqueeze(2)))
    s = e.sum(2)
    M = fin(mm.amax(1))
    total = (torch.exp(fin(mm) - M.view(-1, 1)) * s).sum(1)
    none = total == 0
    log_total = torch.log(torch.where(none, torch.ones_like(total), total))
    vol = torch.where(none, torch.full_like(M, NEG_INF), M + log_total)
    neg = lambda t: torch.full_like(t, NEG_INF)  # noqa: E731
    post_sky = torch.where(s == 0, neg(s), (fin(mm) - M.view(-1, 1)) + (torch.log(torch.where(s == 0, torch.ones_like(s), s)) -
                                                                        log_total.view(-1, 1)))
    md = w.amax(1)
    sd = torch.where(w == NEG_INF, torch.zeros_like(w), torch.exp(w - fin(md).unsqueeze(1))).sum(1)
    post_dist = torch.where(sd == 0, neg(sd), (fin(md) - M.view(-1, 1)) + (torch.log(torch.where(sd == 0, torch.ones_like(sd), sd)) -
                                                                           log_total.view(-1, 1)))
    post_joint = torch.where(w == NEG_INF, neg(w), (w - M.view(-1, 1, 1)) - log_total.view(-1, 1, 1))
    v = torch.where(live_i, 1.0 / a0.view(-1), torch.zeros_like(a)).view(1, 1, -1)
    s1 = torch.where(s == 0, torch.ones_like(s), s)
    mean = (v * e).sum(2) / s1
    std = ((((v - mean.unsqueeze(2)) ** 2) * e).sum(2) / s1).sqrt()
    return dict(lnl_vol=vol, post_sky=post_sky, post_dist=post_dist, post_joint=post_joint, dist_mean=mean, dist_std=std)


# ---- gates -------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, lnl_gate=1e-10, lnl_floor=1e-12):
    """Worst error / gate per quantity ``got`` holds (a mapping name -> tensor or None); ``w`` is formed from post_joint + lnl_vol
    when both are there.  -inf is met by -inf only (else inf); a value that is not finite elsewhere: inf."""
    out = {}
    Bn = ref["lnl"].shape[0]
    g_row = lnl_gate * ref["S"] + lnl_floor
    g_task = lnl_gate * ref["S"].view(-1, Bn).max(0).values + lnl_floor

    def put(name, x, r, gate):
        x = x.detach().cpu().reshape(r.shape)
        assert x.dtype == torch.float64, (name, x.dtype)
        gate = gate.expand_as(r) if isinstance(gate, torch.Tensor) else torch.full_like(r, gate)
        minus = r == NEG_INF
        d = torch.where(minus, torch.zeros_like(r), (x - torch.where(minus, torch.zeros_like(r), r)).abs())
        q = torch.where(d == 0, torch.zeros_like(d), d / gate)
        q = torch.where(torch.isfinite(d), q, torch.full_like(q, math.inf))
        q = torch.where(minus, torch.where(x == NEG_INF, torch.zeros_like(q), torch.full_like(q, math.inf)), q)
        out[name] = float(q.max()) if q.numel() else 0.0

    has = lambda k: got.get(k) is not None  # noqa: E731
    for name in ("pix_index", "scale_index", "tau_index"):
        if has(name):
            assert got[name].dtype == torch.int32, name
            out[name] = 0.0 if torch.equal(got[name].detach().cpu().reshape(-1).long(), ref[name].long()) else math.inf
    if has("lnl_vol"):
        put("lnl_vol", got["lnl_vol"], ref["lnl_vol"], g_row)
    if has("lnl"):
        put("lnl", got["lnl"], ref["lnl"], g_task)
    for name in POSTS:
        if has(name):
            put(name, got[name], ref[name], 2.0 * g_row.view(-1, *([1] * (ref[name].dim() - 1))))
    if has("post_joint") and has("lnl_vol"):
        pj = got["post_joint"].detach().cpu().reshape(ref["w"].shape)
        put("w", pj + got["lnl_vol"].detach().cpu().reshape(-1, 1, 1), ref["w"], g_row.view(-1, 1, 1))
    for name in MIXES:
        if has(name):
            put(name, got[name], ref[name], 2.0 * g_task.view(-1, 1))
    for name in ("snr", "scale_hat"):
        if has(name):
            put(name, got[name], ref[name], 1e-10 * ref[name].abs() + 1e-12)
    v = ref["v_max"]
    if has("dist_mean"):
        put("dist_mean", got["dist_mean"], ref["dist_mean"], 4.0 * g_row.view(-1, 1) * v + 1e-12 * ref["dist_mean"].abs())
    if has("dist_std"):
        x = got["dist_std"].detach().cpu().reshape(ref["dist_std"].shape)
        put("dist_std", x * x, ref["dist_std"] ** 2, 8.0 * g_row.view(-1, 1) * v * v + 1e-12 * ref["dist_std"] ** 2)
    return out


def margins(ref):
    """How well posed the indices are: the lead of the best u_sky and of the best u_dist over their runners-up in units of g_r (the
    smallest over the rows), and the relative lead of the best x_j at the best pixel.  inf where there is no runner-up."""
    gate = 1e-10 * ref["S"] + 1e-12

    def lead(u):
        if u.shape[1] < 2:
            return math.inf
        top = u.topk(2, dim=1).values
        gap = torch.where((top[:, 1] == NEG_INF) | (top[:, 0] == NEG_INF), torch.full_like(gate, math.inf), (top[:, 0] - top[:, 1]) / gate)
        return float(gap.min())

    x = ref["x"]
    lead_x = math.inf
    if x.shape[2] >= 2:
        xp = x.gather(1, ref["pix_index"].view(-1, 1, 1).expand(-1, 1, x.shape[2]))[:, 0]
        top = xp.topk(2, dim=1).values
        keep = (top[:, 0] > 0) & (ref["lnl_vol"] > NEG_INF) & (ref["HH"].gather(1, ref["pix_index"].view(-1, 1))[:, 0] > 0)
        if keep.any():
            lead_x = float(((top[:, 0] - top[:, 1]) / top[:, 0])[keep].min())
    return lead(ref["u_sky"]), lead(ref["u_dist"]), lead_x


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def build(n_a=5, kind="geo", data_scale=DATA_SCALE, **kw):
    """``loglike_sky_reference.build`` with every task's data scaled by ``data_scale`` (a number or a list per task), plus a
    geometric scale grid of ``n_a`` points with the volume prior of ``loglike_dist_reference`` (``kind``: its ``scale_grid``)."""
    Bn = kw.get("Bn", 3)
    scale = list(data_scale) if isinstance(data_scale, (list, tuple)) else [float(data_scale)] * Bn
    case = S.build(data_scale=scale, **kw)
    case["scales"], case["log_prior_scale"] = DR.scale_grid(n_a, "A", "A", kind)
    return case


def call_args(case):
    return {k: case[k] for k in ("h", "data", "response", "delays", "scales", "log_prior_scale", "log_prior", "weights", "freqs",
                                 "taus", "n_valid")}


BASE = dict(Bn=3, n_z=3, T=37, D=3, P=7, n_tau=5, n_a=5)


def sweep_sets():
    """One axis at a time from BASE -> list of (axis, tag, case).  h_ld, the form of the weights and the pixel prior rotate."""
    out = []

    def add(axis, tag, **kw):
        i = len(out)
        full = dict(BASE, **kw)
        full.setdefault("h_ld", (2, 4)[i % 2])
        full.setdefault("wform", (None, "T", "BT")[i % 3])
        full.setdefault("prior", bool((i // 2) % 2))
        out.append((axis, tag, build(seed=200 + i, **full)))

    for Bn, n_z in ((1, 1), (16, 1), (17, 1), (11, 3)):
        add("rows", f"rows={Bn * n_z}", Bn=Bn, n_z=n_z)
    for P in (1, 15, 16, 17, 40, 65):
        add("P", f"P={P}", P=P)
    for n_tau in (None, 1, S_JC - 1, S_JC, S_JC + 1, 2 * S_JC + 1):
        add("n_tau", f"n_tau={n_tau}", n_tau=n_tau, j0=None if n_tau is None else n_tau - 1)
    for n_a in (1, 2, SC - 1, SC, SC + 1, 65):
        add("n_a", f"n_a={n_a}", n_a=n_a)
    for T in (5, 37, 129):
        add("T", f"T={T}", T=T)
    for D in (1, 3):
        add("D", f"D={D}", D=D)
    for n_z in (1, 3):
        add("n_z", f"n_z={n_z}", n_z=n_z)
    return out


S_JC = 8  # NPF_SKY_JC


def regime_set():
    """Four tasks whose x = |K| at the planted pixel and a = 1 is 0.1 (quiet), 20, 30 (across the switch of ln I0) and 1e6 (loud:
    w near 1e6 at a = 1 and beyond), two latent samples; a grid of five scales 2^-1 .. 2^1."""
    case = S.regime_set()
    a = DR.geometric(5, -1.0, 1.0)
    case["scales"], case["log_prior_scale"] = a, DR.volume_prior(a)
    return case


def degenerate_set():
    """BASE with the amplitude of rows 1 and 5 at zero: HH_p == 0 at every pixel, w = lp_p + ln pi_i."""
    case = build(seed=301, prior=True, wform="T", **BASE)
    case["h"][[1, 5], :, 0] = 0.0
    return case


def base_set(n_a=5, kind="geo"):
    """Nine rows, seven pixels, a pixel prior: what the dead-entry, isolation, repeat and subset tests start from."""
    return build(seed=302, prior=True, wform="T", h_ld=2, **dict(BASE, n_a=n_a), kind=kind)


def perm_set():
    """33 rows x 40 pixels x 9 scales: three row tiles, three pixel tiles, two scale chunks."""
    return build(Bn=11, n_z=3, T=37, D=2, P=40, n_tau=9, n_a=9, h_ld=2, wform="BT", prior=True, seed=306, j0=6)


def gpu_sets():
    """Every input set of the GPU test whose indices must be well posed -> list of (tag, case)."""
    return [(tag, case) for _, tag, case in sweep_sets()] + [("regimes", regime_set()), ("HH == 0 rows", degenerate_set()),
                                                             ("base", base_set()), ("dead scales", base_set(13, "dead")),
                                                             ("permutations", perm_set())]


_CACHE = {}


def cached(tag, case):
    """The reference of a set, computed once per process and shared by the tests (never modified)."""
    if tag not in _CACHE:
        _CACHE[tag] = reference(**call_args(case))
    return _CACHE[tag]
