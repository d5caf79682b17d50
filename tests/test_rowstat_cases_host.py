"""The inputs of tests/test_hip_rowstat_edges.py on the CPU: every regime of tests/rowstat_cases.py holds what it claims (float64),
and on every regime and shape of the GPU test the reference-formula term of the gate stays small, so the gate means something.

The gate of the GPU test is  err <= max(tol * max|ref|, 4 * |fp32 formula - ref|)  per row (per task for the head).  The fp32
formulas are the ones in this module, plain torch: two-pass LayerNorm, the head as csrc/head_kernels.hip writes it, a running
logsumexp, a sequential sum.  They are the REFERENCE's rounding on the case -- never the kernel's output.  The condition checked
here: 4 x the formula's error is at most 1e-3 of max|ref| (per tensor), so a kernel that is wrong by more than 1e-3 of a row
cannot hide behind that term.  (The padded-sum variance of the chain LayerNorm before its repair erred by 5e-3 on ``offset``.)

Last, every slip a regime is there to catch is put into the fp32 FORMULA (not into a kernel) and must miss the gate on that
regime -- or the test states what is true instead, where a slip turned out not to be observable in fp32."""
import math

import pytest
import torch

import rowstat_cases as RC

CONDITION = 1e-3  # 4 x the fp32 formula's error, as a share of max|ref|
# The one exception, by name: the gradients (dx per row, dgamma, dbeta) of LayerNorm at F = 4 in the regimes that hold rows with a
# mean offset (``offset``, ``offset_big``, ``mixed``).  Four values of 30 + 0.1 randn can lie within 0.02 of each other; dx of such
# a row is rstd x (a difference of terms of the size of dy) and the rounding of xhat enters twice.  Measured on these inputs,
# 4 x the formula's error / max|ref|: offset dx 1.8e-3, offset_big dgamma 1.4e-3 and dx 1.8e-3, mixed dx 2.0e-3.  Everywhere else,
# and for y at F = 4 too, the share is CONDITION.
F4_OFFSET_GRAD = 3e-3


def ln_share(regime, F, tensor):
    return F4_OFFSET_GRAD if F == 4 and tensor != "y" and regime in ("offset", "offset_big", "mixed") else CONDITION

# the shapes of the GPU test
CHAIN_LN_F, CHAIN_LN_PTS = (24, 30, 100, 128, 200, 256), (33, 5)
ADD_LN_F, ADD_LN_PTS = (4, 48, 100, 128, 256), (33, 5, 64)
LN_B = 2
HEAD_ROWS, HEAD_B = 6, 3
HEAD_SHAPES = ((1, 1), (77, 3), (257, 16), (1030, 2))
MC_NZ, MC_B = (1, 2, 5, 33, 128), (1, 128, 129)
MEAN_PTS, MEAN_F, MEAN_B = (1, 33, 4096), 32, 2
SUMO_M = 5


def ln_seed(regime, pts, F):
    return 1000 * RC.LN_REGIMES.index(regime) + 10 * F + pts


def head_seed(regime, pts, dy):
    return 100000 * RC.HEAD_REGIMES.index(regime) + 20 * pts + dy


def mc_seed(regime, n_z, B):
    return 100000 * RC.MC_REGIMES.index(regime) + 200 * n_z + B


# ---- the formulas ----------------------------------------------------------------------------------------------------------------
def layernorm_and_grads(x, gamma, beta, dy, eps, dtype, variance="two_pass", eps_inside=True):
    """(y, dx, dgamma, dbeta) of LayerNorm over the last dimension in ``dtype``, two-pass: mean, then the mean of the squared
    centred values.  ``variance`` / ``eps_inside`` put a slip into the formula: ``one_pass`` E[x^2] - E[x]^2; ``padded``: the
    row padded with zeros to a multiple of 32, centred whole, the padding's share (Fp - F) mean^2 subtracted afterwards."""
    x, gamma, beta, dy = (t.to(dtype) for t in (x, gamma, beta, dy))
    F = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / F
    xc = x - mean
    if variance == "two_pass":
        var = (xc * xc).sum(-1, keepdim=True) / F
    elif variance == "one_pass":
        var = ((x * x).sum(-1, keepdim=True) / F - mean * mean).clamp(min=0)
    else:
        Fp = (F + 31) // 32 * 32
        xp = torch.nn.functional.pad(x, (0, Fp - F)) - mean
        var = (((xp * xp).sum(-1, keepdim=True) - (Fp - F) * mean * mean) / F).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + eps) if eps_inside else 1.0 / (torch.sqrt(var) + eps)
    xh = xc * rstd
    y = xh * gamma + beta
    g = dy * gamma
    dx = rstd * (g - g.sum(-1, keepdim=True) / F - xh * ((g * xh).sum(-1, keepdim=True) / F))
    flat = lambda t: t.reshape(-1, F)  # noqa: E731
    return y, dx, flat(dy * xh).sum(0), flat(dy).sum(0)


def layernorm_autograd64(x, gamma, beta, dy, eps):
    """The same four tensors from torch.nn.functional.layer_norm and autograd in float64: the reference."""
    x, gamma, beta = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    return (y.detach(),) + torch.autograd.grad((y * dy.double()).sum(), (x, gamma, beta))


HALF_LOG_2PI = 0.91893853320467274178


def head_and_grads(suff, Y, dy, homosk, w_loc, w_scale, w_slp, dtype, threshold=True, log1p=True):
    """(loc, scale, sum_logp, d_suff) of the Gaussian head in ``dtype`` as csrc/head_kernels.hip writes it: softplus with the
    x > 20 branch and log1p(exp(x)) below, scale = 0.01 + 0.99 softplus, optional pooling over the points, the Normal's log
    density summed over points and dimensions; the gradient from the closed forms of the backward kernel.  ``w_loc`` / ``w_scale``
    may be None (a loss-only launch).  ``threshold`` / ``log1p`` False put a slip into the softplus."""
    suff, Y, w_slp = suff.to(dtype), Y.to(dtype), w_slp.to(dtype)
    rows = suff.shape[0]
    mu, raw = suff.split(dy, dim=-1)
    soft = torch.log1p(torch.exp(raw)) if log1p else torch.log(1.0 + torch.exp(raw))
    sp = torch.where(raw > 20.0, raw, soft) if threshold else soft
    sg = 0.01 + 0.99 * sp
    if homosk:
        sg = (sg.sum(1, keepdim=True) / sg.shape[1]).expand_as(mu)
    diff = Y.repeat(rows // Y.shape[0], 1, 1) - mu
    lp = -(diff * diff) / (2.0 * sg * sg) - torch.log(sg) - HALF_LOG_2PI
    slp = lp.sum((1, 2))
    g = w_slp.view(rows, 1, 1)
    dmu = g * diff / (sg * sg)
    dsg = g * (diff * diff / (sg * sg * sg) - 1.0 / sg)
    if w_loc is not None:
        dmu = dmu + w_loc.to(dtype)
        dsg = dsg + w_scale.to(dtype)
    if homosk:
        dsg = (dsg.sum(1, keepdim=True) / dsg.shape[1]).expand_as(mu)
    spg = torch.where(raw > 20.0, torch.ones_like(raw), 1.0 / (1.0 + torch.exp(-raw)))
    return mu, sg, slp, torch.cat([dmu, dsg * 0.99 * spg], -1)


def head_autograd64(suff, Y, dy, homosk, w_loc, w_scale, w_slp):
    """The reference: torch's softplus, Normal.log_prob and autograd in float64, as ``test_gauss_head`` builds it."""
    s = suff.double().requires_grad_(True)
    rows, pts = s.shape[:2]
    loc, raw = s.split(dy, dim=-1)
    scale = 0.01 + 0.99 * torch.nn.functional.softplus(raw)
    if homosk:
        scale = scale.mean(1, keepdim=True).expand(rows, pts, dy)
    dist = torch.distributions.Independent(torch.distributions.Normal(loc, scale), 1)
    slp = dist.log_prob(Y.double().repeat(rows // Y.shape[0], 1, 1)).sum(-1)
    total = (slp * w_slp.double()).sum()
    if w_loc is not None:
        total = total + (loc * w_loc.double()).sum() + (scale * w_scale.double()).sum()
    (d,) = torch.autograd.grad(total, s)
    return loc.detach(), scale.detach(), slp.detach(), d


def sumo_weights(n_z, a=SUMO_M, alpha=85):
    """float64 [n_z]: the inverse-tail weights of ``_sumo_reference`` (tests/test_hip_objectives.py), entry K for the 0-based
    sample K (used for K >= a)."""
    kk = (torch.arange(1, n_z + 1) - a).clamp(min=1).double()
    al = float(alpha - a)
    return torch.where(kk < al, 1.0 / kk, (1.0 / al) * 0.9 ** (kk - al))


def running_lse(lw, dtype, skip_neg_inf=True, subtract_max=True):
    """[n_z, B]: the logsumexp of every prefix lw[: k + 1] by the running recurrence (maximum mx, sum acc of exp(v - mx)); a
    -inf sample is a term of weight 0.  ``skip_neg_inf`` False: the recurrence without that rule; ``subtract_max`` False:
    log(sum exp(v)) outright."""
    lw = lw.to(dtype)
    n_z, B = lw.shape
    out = torch.empty_like(lw)
    if not subtract_max:
        return torch.log(torch.cumsum(torch.exp(lw), 0))
    mx, acc = torch.full((B,), float("-inf"), dtype=dtype), torch.zeros(B, dtype=dtype)
    for k in range(n_z):
        v = lw[k]
        gt = v > mx
        new_acc = torch.where(gt, acc * torch.exp(mx - v) + 1.0, acc + torch.exp(v - mx))
        new_mx = torch.where(gt, v, mx)
        if skip_neg_inf:
            dead = v == float("-inf")
            new_acc, new_mx = torch.where(dead, acc, new_acc), torch.where(dead, mx, new_mx)
        mx, acc = new_mx, new_acc
        out[k] = mx + torch.log(acc)
    return out


def _sumo_coef(n_z, w, m):
    """coef[K] of lse_K in the SUMO estimate: [K == m - 1] + [K >= m] w[K] - [m <= K + 1 < n_z] w[K + 1]."""
    coef = torch.zeros(n_z, dtype=w.dtype)
    coef[m - 1] = 1.0
    coef[m:] += w[m:]
    coef[m - 1:n_z - 1] -= w[m:]
    return coef


def mc_and_grads(lw, mode, d_out, dtype, m=SUMO_M, **slip):
    """(out [B], d_lw [n_z, B]) of the Monte-Carlo objectives in ``dtype`` from the running logsumexp: mode 0 the mean (a sequential sum), 1 the
    log-mean-exp, 2 SUMO.  Gradients from the closed forms (softmax; for SUMO the sum over the prefixes K >= k of coef[K]
    exp(lw_k - lse_K)), with exactly 0 at a -inf sample."""
    n_z, B = lw.shape
    x, g = lw.to(dtype), d_out.to(dtype)
    if mode == 0:  # (added one after the other: on ``late_jump`` the halves at -100 and +100 cancel, and the order is the rounding)
        return sequential_mean(x.t(), dtype), (g / n_z).expand(n_z, B).clone()
    lse = running_lse(lw, dtype, **slip)
    live = x != float("-inf")
    if mode == 1:
        return lse[-1] - math.log(n_z), torch.where(live, g * torch.exp(x - lse[-1]), torch.zeros_like(x))
    w = sumo_weights(n_z).to(dtype)
    c = lse - torch.log(torch.arange(1, n_z + 1, dtype=dtype)).view(-1, 1)
    est = c[m - 1] + (w[m:].view(-1, 1) * (c[m:] - c[m - 1:-1])).sum(0)
    coef = _sumo_coef(n_z, w, m)
    p = torch.exp(x.unsqueeze(0) - lse.unsqueeze(1))  # [K, k, B]
    keep = (torch.arange(n_z).view(-1, 1) >= torch.arange(n_z).view(1, -1)).unsqueeze(-1) & live.unsqueeze(0) & (coef != 0).view(-1, 1, 1)
    d = (torch.where(keep, p, torch.zeros_like(p)) * coef.view(-1, 1, 1)).sum(0)
    return est, g * d


def mc_autograd64(lw, mode, d_out, m=SUMO_M):
    """The reference: float64 ``torch.logsumexp`` (of the prefixes K >= m - 1 for SUMO: the others carry no weight) and autograd."""
    x = lw.double().requires_grad_(True)
    n_z = x.shape[0]
    if mode == 0:
        out = x.mean(0)
    elif mode == 1:
        out = torch.logsumexp(x, 0) - math.log(n_z)
    else:
        w = sumo_weights(n_z)
        c = torch.stack([torch.logsumexp(x[:K + 1], 0) - math.log(K + 1) for K in range(m - 1, n_z)])
        out = c[0] + (w[m:].view(-1, 1) * (c[1:] - c[:-1])).sum(0)
    (d,) = torch.autograd.grad((out * d_out.double()).sum(), x)
    return out.detach(), d


def mc_modes(n_z, regime):
    """The modes a regime runs in: the mean has no meaning with a -inf sample, SUMO needs its five samples."""
    modes = [] if regime.startswith("neg_inf") else [0]
    return modes + [1] + ([2] if n_z >= SUMO_M else [])


def mc_runs(regime, n_z):
    return not (regime == "neg_inf_first" and n_z == 1)  # (the all -inf task is not covered)


def sequential_mean(x, dtype):
    """Mean over dimension 1 by adding the points one after the other in ``dtype``."""
    x = x.to(dtype)
    s = torch.zeros_like(x[:, 0])
    for t in range(x.shape[1]):
        s = s + x[:, t]
    return s / x.shape[1]


# ---- the gate's two terms, for the condition and the slips ---------------------------------------------------------------------
def _term(r32, r64):
    """(4 x max|fp32 formula - ref|, max|ref|)."""
    return 4 * float((r32.double() - r64).abs().max()), float(r64.abs().max())


def _holds(r32, r64, what, rows=False, share=CONDITION):
    assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), what
    if rows:
        r32, r64 = r32.double().reshape(-1, r32.shape[-1]), r64.reshape(-1, r64.shape[-1])
        t, m = 4 * (r32 - r64).abs().amax(-1), r64.abs().amax(-1)
        bad = (t > share * m).nonzero().flatten().tolist()
        assert not bad, f"{what} row {bad[0]}: 4 x fp32 formula error {float(t[bad[0]]):.3e} > {share:.0e} * max|ref| = {float(m[bad[0]]):.3e}"
        return
    t, m = _term(r32, r64)
    assert t <= share * m, f"{what}: 4 x fp32 formula error {t:.3e} > {share:.0e} * max|ref| = {m:.3e}"


def row_gates(ref64, ref32, tol):
    """The gate of every row (last dimension) of a tensor on its own: max(tol max|ref_row|, 4 x the fp32 formula's error on that row)."""
    F = ref64.shape[-1]
    ref, r32 = ref64.double().reshape(-1, F), ref32.double().reshape(-1, F)
    return torch.maximum(tol * ref.abs().amax(-1), 4 * (r32 - ref).abs().amax(-1))


def rows_missing(got, r32, r64, tol):
    """The number of rows of ``got`` beyond their gate; every row if ``got`` holds a non-finite value."""
    got = got.double().reshape(-1, r64.shape[-1])
    if not torch.isfinite(got).all():
        return got.shape[0]
    err = (got - r64.double().reshape(-1, r64.shape[-1])).abs().amax(-1)
    return int((err > row_gates(r64, r32, tol)).sum())


def misses_gate(got, r32, r64, tol):
    """Does ``got`` miss the gate on some row?"""
    return rows_missing(got, r32, r64, tol) > 0


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
def _row_stats(x):
    x = x.double()
    mean = x.mean(-1)
    return mean, ((x - mean.unsqueeze(-1)) ** 2).mean(-1)


def _check_ln_claim(regime, x):
    """The claim of a (non-mixed) regime on float64 rows [n, F]."""
    mean, var = _row_stats(x)
    std = var.sqrt()
    F = x.shape[-1]
    if regime == "plain":
        assert float((mean.abs() / std).median()) < 1.5, regime
    elif regime in ("offset", "offset_big"):
        centre, least = (30.0, 100.0) if regime == "offset" else (1000.0, 300.0)
        assert float((mean - centre).abs().max()) < 0.1 * centre and float((mean.abs() / std).min()) > least, regime
    elif regime == "tiny":
        assert float(var.max()) < 1e-2 * RC.LN_EPS and float(var.max()) > 0, regime
    elif regime == "constant":
        assert (var == 0).all() and (x == x[:, :1]).all() and (x != 0).all(), regime
        assert (x * 8 == (x * 8).round()).all() and float(x.abs().max()) <= 8, regime
        # every fp32 partial sum of up to 256 such values is a multiple of 1/8 below 2^24 / 8: exact in any order
        assert 256 * 8 * 8 < 2 ** 24
    elif regime == "outlier":
        top = x.double().abs().sort(-1).values
        assert (top[:, -1] == RC.OUTLIER).all() and (F == 1 or float(top[:, -2].max()) < 7), regime
    elif regime == "large":
        sq = (x.float() * x.float()).sum(-1)
        assert float(x.abs().max()) > 1e15 and torch.isfinite(sq).all() and float(sq.max()) < 1e36, regime
    else:
        raise ValueError(regime)


@pytest.mark.parametrize("F", sorted(set(CHAIN_LN_F + ADD_LN_F)))
@pytest.mark.parametrize("regime", RC.LN_REGIMES)
def test_layernorm_regimes_hold_their_claims_and_keep_the_gate_meaningful(regime, F):
    for pts in sorted(set(CHAIN_LN_PTS + ADD_LN_PTS)):
        x, claim = RC.ln_rows(regime, LN_B, pts, F, ln_seed(regime, pts, F))
        assert x.dtype == torch.float32 and x.shape == (LN_B, pts, F) and claim
        names = RC.ln_row_regimes(regime, LN_B, pts)
        for name in set(names[0]):
            pick = torch.tensor([[n == name for n in row] for row in names])
            _check_ln_claim(name, x[pick])
        if regime == "mixed" and pts >= 7:
            assert set(names[0]) == set(RC.LN_MIXED)
        gamma, beta = RC.ln_params(F, F)
        dy = torch.randn(LN_B, pts, F, generator=torch.Generator().manual_seed(F + pts))
        r64 = layernorm_autograd64(x, gamma, beta, dy, RC.LN_EPS)
        r32 = layernorm_and_grads(x, gamma, beta, dy, RC.LN_EPS, torch.float32)
        f64 = layernorm_and_grads(x, gamma, beta, dy, RC.LN_EPS, torch.float64)
        for i, what in enumerate(("y", "dx", "dgamma", "dbeta")):
            tag = f"{regime} pts={pts} F={F} {what}"
            if what == "dgamma" and regime == "constant":
                # xhat is exactly 0 in the formula; torch's layer_norm leaves a rounding residue of its own in float64
                assert not r32[i].any() and not f64[i].any() and float(r64[i].abs().max()) < 1e-9, tag
                continue
            assert float((f64[i] - r64[i]).abs().max()) <= 1e-9 * float(r64[i].abs().max()), f"{tag}: not the reference's function"
            _holds(r32[i], r64[i], tag, rows=i < 2, share=ln_share(regime, F, what))
        a, b = RC.split_exact(x)
        assert torch.equal(a + b, x) and torch.equal(a.double() + b.double(), x.double()), f"{regime}: a + b is not the regime's row"


@pytest.mark.parametrize("F", ADD_LN_F)
def test_cancelling_pair_cancels_before_the_statistics(F):
    for pts in ADD_LN_PTS:
        a, b, claim = RC.cancelling_pair(LN_B, pts, F, 7 * F + pts)
        x64 = a.double() + b.double()
        assert claim and torch.equal((a + b).double(), x64)  # (exact in fp32)
        assert float(a.abs().max()) > 100 and float(x64.abs().max()) < 1e-4 and float(x64.abs().max()) > 0
        assert float((x64.abs() / a.double().abs().clamp(min=1e-30)).max()) < 1e-6  # a few ulps of a
        assert float(_row_stats(a + b)[1].max()) < 1e-3 * RC.LN_EPS
        gamma, beta = RC.ln_params(F, F)
        dy = torch.randn(LN_B, pts, F, generator=torch.Generator().manual_seed(F + pts))
        r64 = layernorm_autograd64(a + b, gamma, beta, dy, RC.LN_EPS)
        r32 = layernorm_and_grads(a + b, gamma, beta, dy, RC.LN_EPS, torch.float32)
        for i, what in enumerate(("y", "dx", "dgamma", "dbeta")):
            _holds(r32[i], r64[i], f"cancelling pts={pts} F={F} {what}", rows=i < 2)


# ---- Gaussian head -------------------------------------------------------------------------------------------------------------
def head_weights(rows, pts, dy, regime, seed):
    """The upstream gradients (w_loc, w_scale [rows, pts, dy], w_slp [rows]); constant inside the groups of ``threshold``."""
    gen = torch.Generator().manual_seed(seed + 1)
    wl, ws = torch.randn(rows, pts, dy, generator=gen), torch.randn(rows, pts, dy, generator=gen)
    if regime == "threshold":
        wl, ws = RC.per_group(wl), RC.per_group(ws)
    return wl, ws, torch.randn(rows, generator=gen)


def per_task(t):
    """[rows, ...] -> [B, rows / B, ...]: the rows of task b = r % B together."""
    return t.reshape(HEAD_ROWS // HEAD_B, HEAD_B, *t.shape[1:]).transpose(0, 1)


@pytest.mark.parametrize("pts,dy", HEAD_SHAPES)
@pytest.mark.parametrize("regime", RC.HEAD_REGIMES)
def test_head_regimes_hold_their_claims_and_keep_the_gate_meaningful(regime, pts, dy):
    suff, Y, claim = RC.head_inputs(regime, HEAD_ROWS, HEAD_B, pts, dy, head_seed(regime, pts, dy))
    assert suff.shape == (HEAD_ROWS, pts, 2 * dy) and Y.shape == (HEAD_B, pts, dy) and suff.dtype == torch.float32 and claim
    loc, raw = suff.double().split(dy, dim=-1)
    flat = raw.reshape(HEAD_ROWS, -1)
    if regime == "threshold":
        cyc = torch.tensor(RC.THRESHOLD_CYCLE, dtype=torch.float32).double()
        assert torch.equal(flat, cyc[torch.arange(pts * dy) % 8].expand_as(flat))
        above = flat[0] > 20.0  # the branch of every element: 20 itself takes log1p(exp(x)), 20.1 the identity
        assert above.tolist() == [float(c) > 20.0 for c in (cyc[torch.arange(pts * dy) % 8]).tolist()]
        if pts * dy >= 8:
            assert above[:8].tolist() == [False, False, False, False, False, True, True, True]
            assert torch.equal(loc.reshape(HEAD_ROWS, -1)[:, 4], loc.reshape(HEAD_ROWS, -1)[:, 5])
            assert torch.equal(Y.reshape(HEAD_B, -1)[:, 4], Y.reshape(HEAD_B, -1)[:, 5])
    elif regime == "floor_far":
        assert (raw == -100).all()
        sc32 = 0.01 + 0.99 * torch.log1p(torch.exp(suff[..., dy:]))
        assert (sc32 == torch.tensor(0.01)).all()  # exactly the floor in fp32
        far = (Y.double().repeat(HEAD_ROWS // HEAD_B, 1, 1) - loc).abs().max()
        assert 40 <= float(far) <= 55
    elif regime == "wide":
        assert (raw == 80).all() and torch.isfinite(torch.exp(suff[..., dy:])).all()
    elif regime == "wide_overflow":
        assert (raw == 100).all() and torch.isinf(torch.exp(suff[..., dy:])).all()
    else:
        assert float(raw.abs().max()) < 7
    wl, ws, wp = head_weights(HEAD_ROWS, pts, dy, regime, head_seed(regime, pts, dy))
    for homosk in (False, True):
        for dist in (True, False):
            w = (wl, ws) if dist else (None, None)
            r64 = head_autograd64(suff, Y, dy, homosk, *w, wp)
            r32 = head_and_grads(suff, Y, dy, homosk, *w, wp, torch.float32)
            f64 = head_and_grads(suff, Y, dy, homosk, *w, wp, torch.float64)
            for i, what in enumerate(("loc", "scale", "sum_logp", "d_suff")):
                tag = f"{regime} pts={pts} dy={dy} homosk={homosk} dist={dist} {what}"
                assert float((f64[i] - r64[i]).abs().max()) <= 1e-9 * float(r64[i].abs().max()), f"{tag}: not the reference's function"
                a, b = per_task(r32[i]), per_task(r64[i])
                for t in range(HEAD_B):
                    _holds(a[t], b[t], f"{tag} task {t}")


# ---- Monte-Carlo objectives ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_z", MC_NZ)
@pytest.mark.parametrize("regime", RC.MC_REGIMES)
def test_mc_regimes_hold_their_claims_and_keep_the_gate_meaningful(regime, n_z):
    for B in MC_B:
        lw, claim = RC.mc_log_w(regime, n_z, B, mc_seed(regime, n_z, B))
        assert lw.shape == (n_z, B) and lw.dtype == torch.float32 and claim
        x = lw.double()
        if regime == "spread":
            for b in range(B):
                rest = torch.cat([x[:RC.spread_index(b, n_z), b], x[RC.spread_index(b, n_z) + 1:, b]])
                assert int(x[:, b].argmax()) == RC.spread_index(b, n_z)
                assert n_z == 1 or abs(float(x[:, b].max() - rest.max()) - RC.SPREAD) < 1
            assert n_z == 1 or torch.isinf(torch.exp(lw)).any(0).all()  # exp without the maximum overflows
        elif regime == "late_jump":
            d = x[1:] - x[:-1]
            assert (d >= 0).all() and (n_z == 1 or float(d[n_z // 2 - 1].min()) >= RC.JUMP)
        elif regime == "equal":
            assert (x == x[:1]).all()
        elif regime == "neg_inf_first":
            assert (x[0] == float("-inf")).all() and torch.isfinite(x[1:]).all()
        elif regime == "neg_inf_some":
            dead = x == float("-inf")
            assert torch.equal(dead, RC.neg_inf_some_mask(n_z, B)) and torch.isfinite(x[~dead]).all() and not dead[0].any()
            assert n_z == 1 or B == 1 or dead.any()
            assert n_z < SUMO_M or (~dead[:SUMO_M]).any(0).all()
        else:
            assert float((x + 100).abs().max()) < 60
        if not mc_runs(regime, n_z):
            continue
        d_out = torch.randn(B, generator=torch.Generator().manual_seed(B + n_z))
        for mode in mc_modes(n_z, regime):
            r64 = mc_autograd64(lw, mode, d_out)
            r32 = mc_and_grads(lw, mode, d_out, torch.float32)
            f64 = mc_and_grads(lw, mode, d_out, torch.float64)
            for i, what in enumerate(("out", "d_log_w")):
                tag = f"{regime} n_z={n_z} B={B} mode {mode} {what}"
                assert float((f64[i] - r64[i]).abs().max()) <= 1e-9 * float(r64[i].abs().max()), f"{tag}: not the reference's function"
                if what == "out":
                    _holds(r32[i].view(B, 1), r64[i].view(B, 1), tag, rows=True)
                else:  # (per task, a column of log_w, as the GPU test gates it)
                    _holds(r32[i].t(), r64[i].t(), tag, rows=True)
            if regime.startswith("neg_inf"):
                assert not r64[1][x == float("-inf")].any() and not r32[1][x == float("-inf")].any()


# ---- mean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", MEAN_PTS)
def test_mean_rows_keep_the_gate_meaningful(pts):
    x, claim = RC.mean_rows(MEAN_B, pts, MEAN_F, pts)
    assert claim and float((x.double().mean(1) - 1e4).abs().max()) < 5
    _holds(sequential_mean(x, torch.float32), x.double().mean(1), f"mean pts={pts}")


# ---- the slips -----------------------------------------------------------------------------------------------------------------
def _ln_case(regime, F, pts=33):
    x, _ = RC.ln_rows(regime, LN_B, pts, F, ln_seed(regime, pts, F))
    gamma, beta = RC.ln_params(F, F)
    dy = torch.randn(LN_B, pts, F, generator=torch.Generator().manual_seed(F + pts))
    return (x, gamma, beta, dy, RC.LN_EPS), layernorm_autograd64(x, gamma, beta, dy, RC.LN_EPS)


@pytest.mark.parametrize("slip,regime,F", [("one_pass", "offset", 128), ("one_pass", "offset", 24), ("padded", "offset", 24),
                                           ("padded", "offset", 100), ("padded", "offset", 200), ("padded", "offset_big", 30),
                                           ("eps_outside", "tiny", 128), ("eps_outside", "tiny", 24)])
def test_a_layernorm_slip_in_the_formula_misses_the_gate(slip, regime, F):
    """One-pass variance and the padded-sum correction on ``offset``, eps outside the root on ``tiny``: the fp32 formula with the
    slip misses the gate of the GPU test (y at 1e-5), the formula without it passes.  The padded-sum correction is exact where
    there is no padding (F % 32 == 0) and is not listed there."""
    args, r64 = _ln_case(regime, F)
    r32 = layernorm_and_grads(*args, torch.float32)
    kw = dict(eps_inside=False) if slip == "eps_outside" else dict(variance=slip)
    bad = layernorm_and_grads(*args, torch.float32, **kw)
    assert misses_gate(bad[0], r32[0], r64[0], 1e-5) and misses_gate(bad[1], r32[1], r64[1], 2e-5)
    assert not misses_gate(r32[0], r32[0], r64[0], 1e-5)


def test_the_padded_sum_correction_is_the_two_pass_variance_without_padding():
    args, r64 = _ln_case("offset", 128)
    r32, pad = layernorm_and_grads(*args, torch.float32), layernorm_and_grads(*args, torch.float32, variance="padded")
    assert not misses_gate(pad[0], r32[0], r64[0], 1e-5)


def layernorm_other_order(x, gamma, beta, eps, compensated):
    """fp32 two-pass LayerNorm that adds four interleaved partial sums and then those, as four lanes would.  ``compensated``: the
    mean of the centred values -- the rounding error of the fp32 mean -- is subtracted too, as the kernels do."""
    F = x.shape[-1]

    def s4(t):
        t = torch.nn.functional.pad(t, (0, (-F) % 4)).reshape(*t.shape[:-1], -1, 4)
        acc = torch.zeros_like(t[..., 0, :])
        for i in range(t.shape[-2]):
            acc = acc + t[..., i, :]
        return ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])).unsqueeze(-1)

    xc = x - s4(x) / F
    if compensated:
        xc = xc - s4(xc) / F
    return xc * (1.0 / torch.sqrt(s4(xc * xc) / F + eps)) * gamma + beta


@pytest.mark.parametrize("regime", ("offset", "offset_big", "mixed"))
def test_the_per_row_gate_needs_the_compensated_mean(regime):
    """Why both LayerNorm kernels subtract the mean of the centred values.  At a mean offset the error of y is the rounding of the
    row's fp32 mean (half an ulp of 1000 is 3e-5 next to a spread of 1: above 1e-5 of the row), and the formula term of ONE row is
    a single draw of that residue: a correct plain two-pass LayerNorm that merely adds in another order misses the per-row gate
    on some rows.  With the compensation the error is a few 1e-7 of the row and every row passes on the tolerance alone."""
    plain = 0
    for F in (24, 100, 128, 256):
        for pts in (33, 5, 64):
            (x, gamma, beta, dy, eps), r64 = _ln_case(regime, F, pts)
            r32 = layernorm_and_grads(x, gamma, beta, dy, eps, torch.float32)
            plain += rows_missing(layernorm_other_order(x, gamma, beta, eps, False), r32[0], r64[0], 1e-5)
            got = layernorm_other_order(x, gamma, beta, eps, True)
            assert rows_missing(got, r32[0], r64[0], 1e-5) == 0, (regime, F, pts)
            assert float(((got.double() - r64[0]).abs().amax(-1) / r64[0].abs().amax(-1)).max()) < 3e-6, (regime, F, pts)
    assert plain > 0


def _head_case(regime, pts=77, dy=3, homosk=False):
    suff, Y, _ = RC.head_inputs(regime, HEAD_ROWS, HEAD_B, pts, dy, head_seed(regime, pts, dy))
    w = head_weights(HEAD_ROWS, pts, dy, regime, head_seed(regime, pts, dy))
    return (suff, Y, dy, homosk, *w), head_autograd64(suff, Y, dy, homosk, *w)


def test_a_softplus_without_its_threshold_is_caught_where_exp_overflows():
    """``wide_overflow`` (raw = 100): log1p(exp(x)) is inf.  On ``wide`` (raw = 80) expf is still finite in fp32 and
    log1p(exp(80)) rounds to 80: there the slip is NOT observable, which is why ``wide_overflow`` exists."""
    args, r64 = _head_case("wide_overflow")
    bad = head_and_grads(*args, torch.float32, threshold=False)
    assert not torch.isfinite(bad[1]).all()
    args, r64 = _head_case("wide")
    r32, bad = head_and_grads(*args, torch.float32), head_and_grads(*args, torch.float32, threshold=False)
    assert not misses_gate(bad[1], r32[1], r64[1], 1e-5)


def test_log_of_one_plus_exp_is_not_observable_behind_the_floor():
    """log(1 + exp(x)) in place of log1p(exp(x)) loses the softplus below fp32's epsilon (x < -16.6), where it is under 6e-8 --
    next to the floor of 0.01 that is 6e-6 of the scale at the very most and 2e-7 at raw = -20; at raw = -100 both give the
    floor exactly.  No regime can catch this slip at the head's 1e-5 gate; the test records that instead of pretending."""
    for regime in ("floor_far", "threshold"):
        args, r64 = _head_case(regime)
        r32, bad = head_and_grads(*args, torch.float32), head_and_grads(*args, torch.float32, log1p=False)
        assert float(((bad[1] - r32[1]).abs() / r32[1]).max()) < 1e-6
        assert not misses_gate(bad[1], r32[1], r64[1], 1e-5)


@pytest.mark.parametrize("slip,regime", [(dict(skip_neg_inf=False), "neg_inf_first"), (dict(subtract_max=False), "spread")])
def test_a_logsumexp_slip_in_the_formula_misses_the_gate(slip, regime):
    n_z, B = 33, 129
    lw, _ = RC.mc_log_w(regime, n_z, B, mc_seed(regime, n_z, B))
    d_out = torch.randn(B, generator=torch.Generator().manual_seed(B + n_z))
    for mode in (1, 2):
        r64, r32 = mc_autograd64(lw, mode, d_out), mc_and_grads(lw, mode, d_out, torch.float32)
        bad = mc_and_grads(lw, mode, d_out, torch.float32, **slip)
        assert misses_gate(bad[0], r32[0], r64[0], 2e-6), (regime, mode)
        assert not misses_gate(r32[0], r32[0], r64[0], 2e-6)
