"""The kernels that compute a statistic per row, at the values where such kernels go wrong (tests/rowstat_cases.py): the chain's
LayerNorm step and ``npf_add_layernorm_fwd`` / ``_bwd`` at a mean offset, with eps dominating, on constant rows, with an outlier,
at 1e15 and with all of these inside one tile; the Gaussian head across its softplus branch point, on the scale floor and over
more points than one trip of its loops; the Monte-Carlo objectives with a dominant, a late and a -inf sample; the mean at 1e4.

The reference is torch autograd in float64.  The gate is the one of tests/test_hip_mha.py, ``assert_gated``:
err <= max(tol * max|ref|, 4 * |fp32 formula - ref|), applied PER ROW (per task for the head, ``assert_gated_per_task``), with
``tol`` the fp32 gate of each op's older test and the fp32 formulas of tests/test_rowstat_cases_host.py, which also shows on
the CPU that the formula term stays small on every case here.  On top: NaN in the padding points of the LayerNorm operands
changes no bit, ``da`` is ``db``, and the exports with counts give the bits of the ones without at full counts.

Every check prints a line ``ROWSTAT kernel | case | tensor | err | max|ref| | tol | fp32 formula error`` (the worst row), the source of
profiles/rowstat_edges.md."""
import numpy as np
import pytest
import torch

import rowstat_cases as RC
import test_rowstat_cases_host as H
from test_hip_masked_edges import assert_gated_per_task
from test_hip_mha import assert_gated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the gate ------------------------------------------------------------------------------------------------------------------
def _report(kernel, regime, what, got, ref, r32, tol):
    got, ref, r32 = (t.detach().cpu().double().reshape(-1, t.shape[-1] if t.dim() else 1) for t in (got, ref, r32))
    err, f32 = (got - ref).abs().amax(-1), (r32 - ref).abs().amax(-1)
    i = int((err / ref.abs().amax(-1).clamp(min=1e-300)).argmax())
    top = float(ref[i].abs().max())
    print(f"ROWSTAT {kernel} | {regime} | {what} | err {float(err[i]):.3e} | max|ref| {top:.3e} | tol {tol:.0e} | fp32 formula {float(f32[i]):.3e}")


def gated_rows(kernel, regime, what, got, ref64, ref32, tol):
    """``assert_gated`` on every row (last dimension) of the tensor on its own."""
    _report(kernel, regime, what, got, ref64, ref32, tol)
    F = ref64.shape[-1]
    got, ref64, ref32 = (t.detach().cpu().reshape(-1, F) for t in (got, ref64, ref32))
    for i in range(ref64.shape[0]):
        assert_gated(got[i], ref64[i], ref32[i], tol, f"{kernel} {regime} {what} row {i}")


def gated(kernel, regime, what, got, ref64, ref32, tol):
    _report(kernel, regime, what, got, ref64, ref32, tol)
    assert_gated(got, ref64, ref32, tol, f"{kernel} {regime} {what}")


def _ln_case(regime, pts, F):
    x, _ = RC.ln_rows(regime, H.LN_B, pts, F, H.ln_seed(regime, pts, F))
    gamma, beta = RC.ln_params(F, F)
    dy = torch.randn(H.LN_B, pts, F, generator=torch.Generator().manual_seed(F + pts))
    return x, gamma, beta, dy


def _ln_references(x, gamma, beta, dy):
    return H.layernorm_autograd64(x, gamma, beta, dy, RC.LN_EPS), H.layernorm_and_grads(x, gamma, beta, dy, RC.LN_EPS, torch.float32)


# ---- 1. the chain's LayerNorm step ---------------------------------------------------------------------------------------------
def _chain_layernorm(x, gamma, beta, dy):
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import Chain

    B, pts, F = x.shape
    xd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    ch = Chain(B, pts, DEV)
    ch.input_pt(FN.pack_pt(xd), F).layernorm(gd, bd, RC.LN_EPS).output_pt()
    y = FN.unpack_pt(ch.run()[0], pts, F)
    (y * dy.to(DEV)).sum().backward()
    return y.detach(), xd.grad, gd.grad, bd.grad


@pytest.mark.parametrize("F", H.CHAIN_LN_F)
@pytest.mark.parametrize("regime", RC.LN_REGIMES)
def test_chain_layernorm_regimes_match_float64_per_row(regime, F):
    """F = 24, 100, 200: padding features inside the last 32; 30: not a multiple of 4; 128 / 256: none.  Gates of
    ``test_layernorm_chain_step_matches_torch``: 1e-5 on y, 2e-5 on the gradients."""
    for pts in H.CHAIN_LN_PTS:
        case = _ln_case(regime, pts, F)
        r64, r32 = _ln_references(*case)
        y, dx, dg, db = _chain_layernorm(*case)
        tag = f"{regime} pts={pts} F={F}"
        gated_rows("chain_layernorm", tag, "y", y, r64[0], r32[0], 1e-5)
        gated_rows("chain_layernorm", tag, "dx", dx, r64[1], r32[1], 2e-5)
        gated("chain_layernorm", tag, "dgamma", dg, r64[2], r32[2], 2e-5)
        gated("chain_layernorm", tag, "dbeta", db, r64[3], r32[3], 2e-5)


@pytest.mark.parametrize("regime", ("plain", "offset"))
def test_chain_layernorm_in_the_bf16_compute_mode(regime):
    """F = 128 with ``set_compute_dtype("bf16")``: LayerNorm stays fp32 arithmetic there, so the result passes the bf16 mode's
    gate of tests/test_hip_bf16.py (relative L2 5e-3 / 1e-2, max-norm 3e-2) -- and the fp32 gate as well."""
    import npf_gwwaveform_amd as A
    from test_hip_bf16 import TOL_GRAD_L2, TOL_MAX, TOL_OUT_L2, _check

    case = _ln_case(regime, 33, 128)
    r64, r32 = _ln_references(*case)
    A.set_compute_dtype("bf16")
    try:
        got = _chain_layernorm(*case)
    finally:
        A.set_compute_dtype("fp32")
    for i, (what, tol_l2, tol) in enumerate((("y", TOL_OUT_L2, 1e-5), ("dx", TOL_GRAD_L2, 2e-5), ("dgamma", TOL_GRAD_L2, 2e-5),
                                             ("dbeta", TOL_GRAD_L2, 2e-5))):
        _check(got[i], r64[i], tol_l2, TOL_MAX, f"bf16 mode {regime} {what}")
        (gated_rows if i < 2 else gated)("chain_layernorm_bf16_mode", f"{regime} pts=33 F=128", what, got[i], r64[i], r32[i], tol)


# ---- 2. LayerNorm(a + b) -------------------------------------------------------------------------------------------------------
def _add_layernorm(a, b, gamma, beta, dy):
    from npf_gwwaveform_amd import functional as FN

    B, pts, F = a.shape
    ln = torch.nn.LayerNorm(F, eps=RC.LN_EPS).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = FN.unpack_pt(FN.add_layernorm(FN.pack_pt(ad), FN.pack_pt(bd), ln, B, pts), pts, F)
    (y * dy.to(DEV)).sum().backward()
    return y.detach(), ad.grad, bd.grad, ln.weight.grad, ln.bias.grad


def _check_add_layernorm(tag, a, b, gamma, beta, dy):
    """Gates of ``test_add_layernorm_matches_float64``: 1e-5 on y, 1e-4 on the gradients; da is db bit for bit."""
    r64, r32 = _ln_references(a + b, gamma, beta, dy)  # (a + b is exact in fp32 on every case: the host test)
    y, da, db, dg, dbt = _add_layernorm(a, b, gamma, beta, dy)
    assert torch.equal(da, db), f"{tag}: da and db differ"
    gated_rows("add_layernorm", tag, "y", y, r64[0], r32[0], 1e-5)
    gated_rows("add_layernorm", tag, "da", da, r64[1], r32[1], 1e-4)
    gated("add_layernorm", tag, "dgamma", dg, r64[2], r32[2], 1e-4)
    gated("add_layernorm", tag, "dbeta", dbt, r64[3], r32[3], 1e-4)


@pytest.mark.parametrize("F", H.ADD_LN_F)
@pytest.mark.parametrize("regime", RC.LN_REGIMES)
def test_add_layernorm_regimes_match_float64_per_row(regime, F):
    for pts in H.ADD_LN_PTS:
        x, gamma, beta, dy = _ln_case(regime, pts, F)
        a, b = RC.split_exact(x)
        _check_add_layernorm(f"{regime} pts={pts} F={F}", a, b, gamma, beta, dy)


@pytest.mark.parametrize("F", H.ADD_LN_F)
def test_add_layernorm_of_a_sum_that_cancels(F):
    for pts in H.ADD_LN_PTS:
        a, b, _ = RC.cancelling_pair(H.LN_B, pts, F, 7 * F + pts)
        gamma, beta = RC.ln_params(F, F)
        dy = torch.randn(H.LN_B, pts, F, generator=torch.Generator().manual_seed(F + pts))
        _check_add_layernorm(f"cancelling pts={pts} F={F}", a, b, gamma, beta, dy)


# ---- 3. NaN in the padding points ----------------------------------------------------------------------------------------------
def _padding_points(pt, pts):
    """Boolean mask, the shape of a PT32 tensor [B, tiles, Fp / 4, 32, 4]: the points p = 32 tile + lane >= pts
    (include/npf_hip.h: elem(task, p, f) = (((task tiles + p / 32) Fp / 4 + f / 4) 32 + p % 32) 4 + f % 4)."""
    tiles = pt.shape[1]
    p = 32 * torch.arange(tiles, device=pt.device).view(1, tiles, 1, 1, 1) + torch.arange(32, device=pt.device).view(1, 1, 1, 32, 1)
    return (p >= pts).expand_as(pt)


def _poison(pt, pts):
    out = pt.clone()
    out[_padding_points(pt, pts)] = float("nan")
    return out


def _padding_case(B, pts, F):
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(pts + F)
    rows = [torch.randn(B, pts, F, generator=g) for _ in range(3)]
    clean = [FN.pack_pt(r.to(DEV)).detach() for r in rows]
    bad = [_poison(t, pts) for t in clean]
    n_pad = int(_padding_points(clean[0], pts).sum())
    assert n_pad > 0 and all(int(t.isnan().sum()) == n_pad for t in bad)
    return clean, bad


@pytest.mark.parametrize("F", (100, 128))
def test_add_layernorm_ignores_nan_in_the_padding_points(F):
    """pts = 33: 31 padding points in the second tile.  NaN in all of them in a, b and dy: y at the real points, dx (zeros at the
    padding points), dgamma and dbeta keep every bit of the zero-padded launch (include/npf_hip.h)."""
    from npf_gwwaveform_amd import functional as FN

    B, pts = 2, 33
    gamma, beta = RC.ln_params(F, F)
    clean, bad = _padding_case(B, pts, F)
    res = []
    for a_pt, b_pt, dy_pt in (clean, bad):
        ln = torch.nn.LayerNorm(F, eps=RC.LN_EPS).to(DEV)
        with torch.no_grad():
            ln.weight.copy_(gamma)
            ln.bias.copy_(beta)
        a_pt, b_pt = a_pt.clone().requires_grad_(True), b_pt.clone().requires_grad_(True)
        y_pt = FN.add_layernorm(a_pt, b_pt, ln, B, pts)
        y_pt.backward(dy_pt)
        res.append((FN.unpack_pt(y_pt.detach(), pts, F), a_pt.grad, b_pt.grad, ln.weight.grad, ln.bias.grad))
    for what, c, p in zip(("y", "da", "db", "dgamma", "dbeta"), *res):
        assert torch.isfinite(p).all(), f"F={F} {what}: NaN from the padding points"
        assert torch.equal(p, c), f"F={F} {what}: NaN in the padding points changed the result"
        assert float(c.abs().max()) > 0
    assert not res[1][1][_padding_points(res[1][1], pts)].any(), "dx at the padding points"


@pytest.mark.parametrize("pts,wg_per_task", ((33, False), (70, True)))
@pytest.mark.parametrize("F", (100, 128))
def test_chain_layernorm_ignores_nan_in_the_padding_points(F, pts, wg_per_task):
    """The same through ``Program``: NPF_OP_LAYERNORM and NPF_OP_LAYERNORM_BWD on PT32 operands whose padding points hold NaN
    (pts = 70 with a workgroup per task: a third tile next to a tile slot without one)."""
    from npf_gwwaveform_amd import chain as CH
    from npf_gwwaveform_amd import functional as FN

    B = 2
    gamma, beta = (CH._pad_vec(t.to(DEV)) for t in RC.ln_params(F, F))
    res = []
    for x_pt, _, dy_pt in _padding_case(B, pts, F):
        y_pt, dx_pt, dyx_pt = (CH.pt_empty(B, pts, F, DEV) for _ in range(3))
        fwd = CH.Program(B, pts, wg_per_task)
        fwd.load_pt(x_pt, F)
        fwd.layernorm(gamma, beta, F, RC.LN_EPS)
        fwd.store_pt(y_pt, F)
        fwd.launch()
        bwd = CH.Program(B, pts, wg_per_task)
        bwd.load_pt(dy_pt, F)
        bwd.layernorm_bwd(x_pt, gamma, F, RC.LN_EPS, dy_xhat=dyx_pt)
        bwd.store_pt(dx_pt, F)
        bwd.launch()
        dgamma, dbeta = (FN.sum_points_pt(t, pts, F).sum(0)[:F] for t in (dyx_pt, dy_pt))
        res.append((FN.unpack_pt(y_pt, pts, F), FN.unpack_pt(dx_pt, pts, F), dgamma, dbeta, dx_pt))
    for what, c, p in zip(("y", "dx", "dgamma", "dbeta"), *res):
        assert torch.isfinite(p).all(), f"F={F} {what}: NaN from the padding points"
        assert torch.equal(p, c), f"F={F} {what}: NaN in the padding points changed the result"
        assert float(c.abs().max()) > 0
    assert not res[1][4][_padding_points(res[1][4], pts)].any(), "dx at the padding points"


# ---- 4. the Gaussian head ------------------------------------------------------------------------------------------------------
HEAD_TENSORS = (("loc", 1e-5), ("scale", 1e-5), ("sum_logp", 1e-5), ("d_suff", 2e-5))  # the gates of ``test_gauss_head``


def _head_launch(suff, Y, dy, homosk, wl, ws, wp, want_dist, n_valid):
    from npf_gwwaveform_amd import functional as FN

    s = suff.to(DEV).requires_grad_(True)
    loc, scale, slp = FN.gauss_head(s, Y.to(DEV), dy, homosk, want_dist=want_dist, n_valid=n_valid)
    total = (slp * wp.to(DEV)).sum()
    if want_dist:
        total = total + (loc * wl.to(DEV)).sum() + (scale * ws.to(DEV)).sum()
    total.backward()
    return loc.detach(), scale.detach(), slp.detach(), s.grad


@pytest.mark.parametrize("homosk", (False, True))
@pytest.mark.parametrize("pts,dy", H.HEAD_SHAPES)
@pytest.mark.parametrize("regime", RC.HEAD_REGIMES)
def test_gauss_head_regimes_match_float64_per_task(regime, pts, dy, homosk):
    """Six rows over three tasks (Y broadcast), one point up to 1030 (pts * dy beyond one trip of the 256 threads, pooling over
    more than 1000 points), with and without loc / scale, without counts and with full counts."""
    suff, Y, _ = RC.head_inputs(regime, H.HEAD_ROWS, H.HEAD_B, pts, dy, H.head_seed(regime, pts, dy))
    wl, ws, wp = H.head_weights(H.HEAD_ROWS, pts, dy, regime, H.head_seed(regime, pts, dy))
    full = torch.full((H.HEAD_B,), pts, dtype=torch.int32, device=DEV)
    for want_dist in (True, False):
        w = (wl, ws) if want_dist else (None, None)
        r64 = H.head_autograd64(suff, Y, dy, homosk, *w, wp)
        r32 = H.head_and_grads(suff, Y, dy, homosk, *w, wp, torch.float32)
        plain = _head_launch(suff, Y, dy, homosk, wl, ws, wp, want_dist, None)
        counted = _head_launch(suff, Y, dy, homosk, wl, ws, wp, want_dist, full)
        tag = f"{regime} pts={pts} dy={dy} homosk={int(homosk)} dist={int(want_dist)}"
        for i, (what, tol) in enumerate(HEAD_TENSORS):
            if not want_dist and i < 2:
                assert plain[i].numel() == 0 and counted[i].numel() == 0
                continue
            assert torch.equal(counted[i], plain[i]), f"{tag} {what}: full counts give other bits"
            _report("gauss_head", tag, what, plain[i], r64[i], r32[i], tol)
            assert_gated_per_task(H.per_task(plain[i].cpu()), H.per_task(r64[i]), H.per_task(r32[i]), tol, f"{tag} {what}")
        if want_dist:
            np.testing.assert_allclose(plain[1].cpu().numpy(), r64[1].numpy(), rtol=1e-5, err_msg=f"{tag} scale")
        if regime == "threshold" and pts * dy >= 8:
            _no_step_at_the_branch(plain[3].cpu().double(), r64[3], r32[3].double(), pts, dy, tag)


def _no_step_at_the_branch(got, ref, r32, pts, dy, tag):
    """d_suff of the raw scale at raw = 20 (log1p(exp(x)) branch) and at raw = 20.1 (identity branch), elements 4 and 5 of every
    group of 8, which share loc, Y and the upstream gradients (pooled or not): the two differ by no more than they do in float64
    plus the gate -- taken twice, since the step is the difference of TWO gated values, each of which may sit a gate away from
    its reference in opposite directions."""
    raw_grad = lambda t: t[..., dy:].reshape(H.HEAD_ROWS, -1)  # noqa: E731
    g, r, f = raw_grad(got), raw_grad(ref), raw_grad(r32)
    n = pts * dy // 8 * 8
    at20, at201 = torch.arange(4, n, 8), torch.arange(5, n, 8)
    for row in range(H.HEAD_ROWS):
        gate = max(2e-5 * float(ref[row].abs().max()), 4 * float((r32[row] - ref[row]).abs().max()))
        step_got = (g[row, at20] - g[row, at201]).abs()
        step_ref = (r[row, at20] - r[row, at201]).abs()
        assert (step_got <= step_ref + 2 * gate).all(), f"{tag} row {row}: a step in d_suff at the softplus branch point"


def test_gauss_head_rejects_seventeen_output_dimensions():
    from npf_gwwaveform_amd import _lib as L

    suff, out = torch.zeros(2, 3, 34, device=DEV), torch.zeros(2, 3, 17, device=DEV)
    lib = L.load()
    assert lib.npf_gauss_head_fwd(L.ptr(suff), 2, 3, 17, 0, None, 0, L.ptr(out), L.ptr(out.clone()), None, None) == -1
    assert lib.npf_gauss_head_bwd(L.ptr(suff), None, None, 2, 3, 17, 0, None, 0, None, None, None, L.ptr(suff.clone()), None) == -1


# ---- 5. the Monte-Carlo objectives ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", H.MC_B)
@pytest.mark.parametrize("n_z", H.MC_NZ)
def test_mc_objective_regimes_match_float64(n_z, B):
    """Gates of ``test_mc_objective_kernels_match_float64_torch``: 2e-6 forward, 2e-5 backward, per task (a column of log_w);
    the gradient at a -inf sample is exactly 0."""
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.losses import SUMOLossLNPF

    d_out = torch.randn(B, generator=torch.Generator().manual_seed(B + n_z))
    for regime in RC.MC_REGIMES:
        if not H.mc_runs(regime, n_z):
            continue
        lw, _ = RC.mc_log_w(regime, n_z, B, H.mc_seed(regime, n_z, B))
        for mode in H.mc_modes(n_z, regime):
            r64, r32 = H.mc_autograd64(lw, mode, d_out), H.mc_and_grads(lw, mode, d_out, torch.float32)
            x = lw.to(DEV).requires_grad_(True)
            out = SUMOLossLNPF().estimate(x) if mode == FN.MC_SUMO else FN.mc_objective(x, mode)
            out.backward(d_out.to(DEV))
            tag = f"{regime} n_z={n_z} B={B}"
            gated_rows(f"mc_objective_mode{mode}", tag, "out", out.detach().view(B, 1), r64[0].view(B, 1), r32[0].view(B, 1), 2e-6)
            gated_rows(f"mc_objective_mode{mode}", tag, "d_log_w", x.grad.t(), r64[1].t(), r32[1].t(), 2e-5)
            dead = lw == float("-inf")
            if dead.any():
                assert not x.grad.cpu()[dead].any(), f"{tag} mode {mode}: a gradient at a -inf sample"


# ---- 6. the mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", H.MEAN_PTS)
def test_mean_at_an_offset_matches_float64(pts):
    """1e4 + randn over 1, 33 and 4096 points, both exports (full counts: the same bits), gated by a sequential fp32 sum; the
    gate of ``test_mean_agg`` (1e-5) on the mean and on its gradient."""
    from npf_gwwaveform_amd import functional as FN

    B, F = H.MEAN_B, H.MEAN_F
    x, _ = RC.mean_rows(B, pts, F, pts)
    w = torch.randn(B, F, generator=torch.Generator().manual_seed(pts))
    ref, r32 = x.double().mean(1), H.sequential_mean(x, torch.float32)
    dref = (w.double() / pts).unsqueeze(1).expand(B, pts, F)
    full = torch.full((B,), pts, dtype=torch.int32, device=DEV)
    res = []
    for mean in (lambda pt: FN.mean_agg(pt, pts, F), lambda pt: FN.masked_mean(pt, full, B, pts, F)):
        xd = x.to(DEV).requires_grad_(True)
        m = mean(FN.pack_pt(xd))
        (m * w.to(DEV)).sum().backward()
        res.append((m.detach(), xd.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "full counts give other bits"
    gated_rows("mean", f"pts={pts}", "mean", res[0][0], ref, r32, 1e-5)
    gated_rows("mean", f"pts={pts}", "d_mean", res[0][1], dref, (w / pts).unsqueeze(1).expand(B, pts, F), 1e-5)
