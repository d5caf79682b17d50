"""Padded targets with per-task counts on the GPU (``forward(..., n_trgt=...)``; ``npf_masked_gauss_head_fwd`` / ``_bwd`` in
csrc/head_kernels.hip, the query counts of ``npf_masked_attn_fwd_nq`` / ``_bwd_nq`` in csrc/masked_kernels.hip).

The reference is never the code under test: float64 torch for the kernels, and for whole models the CPU oracle run ONCE PER TASK on
the batch cut to that task's target rows (and, with ``n_cntxt``, its context rows), the losses averaged and the gradients accumulated
on one parameter dict -- the scheme of tests/test_hip_masked.py with the targets cut as well.  Gates are the project's fp32 gates:
outputs 1e-5 of max|ref|, the loss to rtol 2e-5, gradients 1e-4 of max|ref| with the zero-reference rule of ``_compare_grads``; the
attention kernels use ``assert_gated`` of tests/test_hip_mha.py.  Whole-model inputs are chosen by the well-posedness rule of
tests/test_hip_masked.py (no ReLU pre-activation OF THE ORACLE within ``RELU_TIE`` of zero): a condition on the reference alone.

``attnlnp_scaledot_r256_nz8`` runs at ``T_pad = 70`` only: at ``T_pad = 300`` no seed in 4000 satisfies the rule (8 samples x 300
targets x 256 units leave too many pre-activations near zero); ``T_pad = 300`` of the latent attentive model is covered by
``attnlnp_scaledot_r256_nz1``."""
import copy
import math

import numpy as np
import pytest
import torch

import specs
from helpers import EpsIndependent, assert_close, build_loss, build_model, eps_latent_dist, launch_witness
from oracle import npf_oracle as O
from test_hip_dispatch import _compare_grads, _compare_outputs
from test_hip_masked import MODEL_CASES, RELU_TIE, _attention_and_grads, _case, _counts
from test_hip_mha import assert_gated
from test_hip_sweep import LOSSES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = ("npf_masked_gauss_head_fwd", "npf_masked_gauss_head_bwd", "npf_masked_attn_fwd_nq", "npf_masked_attn_bwd_nq")


# ---- 1. the head kernel against float64 ----------------------------------------------------------------------------------------
def _head_counts(n_tasks, T_pad):
    """Counts that include 0, 1, T_pad - 1, T_pad and a value either side of the block size 256 (clamped to T_pad)."""
    must = [0, 1, max(T_pad - 1, 0), T_pad, min(255, T_pad), min(257, T_pad)]
    rng = np.random.Generator(np.random.Philox(T_pad))
    return (must + rng.integers(0, T_pad + 1, size=max(n_tasks - len(must), 0)).tolist())[:n_tasks]


def _head_reference(suff, Y, counts, dy, homosk, n_z, d_loc, d_scale, d_slp):
    """float64: (loc, scale, sum_logp, d_suff) of the head of every row cut to its count; loc 0 / scale 1 / d_suff 0 beyond."""
    s = suff.double().clone().requires_grad_(True)
    n_rows, T_pad = s.shape[0], s.shape[1]
    n_tasks = len(counts)
    loc, scale = torch.zeros(n_rows, T_pad, dy, dtype=torch.float64), torch.ones(n_rows, T_pad, dy, dtype=torch.float64)
    slp = torch.zeros(n_rows, dtype=torch.float64)
    total = torch.zeros((), dtype=torch.float64)
    for r in range(n_rows):
        n = counts[r % n_tasks]
        if n == 0:
            continue
        mu, raw = s[r, :n, :dy], s[r, :n, dy:]
        sg = 0.01 + 0.99 * torch.nn.functional.softplus(raw)
        if homosk:
            sg = sg.mean(0, keepdim=True).expand(n, dy)
        y = Y[r % Y.shape[0], :n].double()
        lp = (-((y - mu) ** 2) / (2 * sg ** 2) - sg.log() - 0.5 * math.log(2 * math.pi)).sum()
        loc[r, :n], scale[r, :n], slp[r] = mu.detach(), sg.detach(), lp.detach()
        total = total + lp * d_slp[r].double()
        if d_loc is not None:
            total = total + (mu * d_loc[r, :n].double()).sum() + (sg * d_scale[r, :n].double()).sum()
    total.backward()
    return loc, scale, slp, s.grad


@pytest.mark.parametrize("T_pad", (1, 31, 32, 33, 257, 1024))
@pytest.mark.parametrize("n_z", (1, 3))
@pytest.mark.parametrize("homosk", (False, True))
@pytest.mark.parametrize("dy", (1, 2, 16))
def test_masked_head_matches_float64(dy, homosk, n_z, T_pad):
    from npf_gwwaveform_amd import functional as FN

    B = 8
    counts = _head_counts(B, T_pad)
    g = torch.Generator().manual_seed(1000 * dy + 10 * T_pad + n_z + int(homosk))
    suff = torch.randn(n_z * B, T_pad, 2 * dy, generator=g)
    Y = torch.randn(B, T_pad, dy, generator=g)
    d_slp = torch.randn(n_z * B, generator=g)
    d_loc, d_scale = torch.randn(n_z * B, T_pad, dy, generator=g), torch.randn(n_z * B, T_pad, dy, generator=g)
    Y_nan = Y.clone()
    for b, n in enumerate(counts):
        Y_nan[b, n:] = float("nan")  # (beyond the count Y is never read)
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    for materialised in (True, False):
        ref = _head_reference(suff, Y, counts, dy, homosk, n_z, d_loc if materialised else None, d_scale, d_slp)
        sd = suff.to(DEV).requires_grad_(True)
        with launch_witness() as w:
            loc, scale, slp = FN.gauss_head(sd, Y_nan.to(DEV), dy, homosk, want_dist=materialised, n_valid=n_valid)
            tot = (slp * d_slp.to(DEV)).sum()
            if materialised:
                tot = tot + (loc * d_loc.to(DEV)).sum() + (scale * d_scale.to(DEV)).sum()
            tot.backward()
            torch.cuda.synchronize()
        assert w["npf_masked_gauss_head_fwd"] == 1 and w["npf_masked_gauss_head_bwd"] == 1 and w["npf_gauss_head_fwd"] == 0, w
        what = f"dy={dy} homosk={homosk} n_z={n_z} T_pad={T_pad} materialised={materialised}"
        for name, got, want, tol in (("sum_logp", slp, ref[2], 1e-5), ("d_suff", sd.grad, ref[3], 1e-4)):
            print(f"{what} {name}: max|d|={float((got.detach().cpu().double() - want).abs().max()):.3e} "
                  f"max|ref|={float(want.abs().max()):.3e}")
            assert_close(got, want, tol=tol, what=f"{name} {what}")
        if materialised:
            assert_close(loc, ref[0], tol=1e-5, what=f"loc {what}")
            assert_close(scale, ref[1], tol=1e-5, what=f"scale {what}")
        else:
            assert loc.numel() == 0 and scale.numel() == 0
        for r in range(n_z * B):
            n = counts[r % B]
            assert (sd.grad[r, n:] == 0).all(), f"{what}: d_suff of row {r} beyond the count {n}"
            if materialised:
                assert (loc[r, n:] == 0).all() and (scale[r, n:] == 1).all(), f"{what}: loc / scale of row {r} beyond the count {n}"
            if n == 0:
                assert float(slp[r].detach()) == 0.0


@pytest.mark.parametrize("rows,T,dy", ((6, 300, 2), (2, 1, 1), (4, 257, 16)))
@pytest.mark.parametrize("homosk", (False, True))
def test_masked_head_at_full_counts_is_the_unmasked_head_bit_for_bit(homosk, rows, T, dy):
    """Counts at and above T (clamped) against ``npf_gauss_head_fwd`` / ``_bwd``: the same loops in the same order.  T = 1: a single
    point, 255 idle threads in every reduction; 257 * 16 elements: more than one stride of the element loop at the widest dy.
    ``want_dist=False``: the backward pass recomputes loc / scale (and the pooled scale) from ``suff``."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(5)
    suff, Y = torch.randn(rows, T, 2 * dy, generator=g).to(DEV), torch.randn(2, T, dy, generator=g).to(DEV)
    for want_dist in (True, False):
        outs = []
        for n_valid in (None, torch.tensor([T, 10 ** 6], device=DEV)):
            s = suff.clone().requires_grad_(True)
            loc, scale, slp = FN.gauss_head(s, Y, dy, homosk, want_dist=want_dist, n_valid=n_valid)
            (slp.sum() + (loc * scale).sum()).backward()
            outs.append((loc, scale, slp, s.grad))
        for a, b in zip(*outs):
            assert torch.equal(a, b), f"want_dist={want_dist}"
        assert (loc.numel() > 0) == want_dist and float(s.grad.abs().max()) > 0


# ---- 2. attention with query counts --------------------------------------------------------------------------------------------
def _q_counts(B, T_pad, seed):
    must = [0, 1, T_pad, max(T_pad - 1, 0), min(64, T_pad), min(65, T_pad), min(16, T_pad)]
    rng = np.random.Generator(np.random.Philox(seed))
    return (must + rng.integers(0, T_pad + 1, size=max(B - len(must), 0)).tolist())[:B]


@pytest.mark.parametrize("T_pad", (1, 70, 200))
@pytest.mark.parametrize("C_pad", (33, 257))
@pytest.mark.parametrize("d", (16, 128, 256))
def test_query_counts_match_the_existing_export_and_float64(d, C_pad, T_pad):
    from npf_gwwaveform_amd import functional as FN

    B = 8
    counts = _counts(B, C_pad, seed=d + C_pad + T_pad)
    q_counts = _q_counts(B, T_pad, seed=7 * d + C_pad + T_pad)
    g = torch.Generator().manual_seed(1000 * d + C_pad + T_pad)
    Q, K, V = (torch.randn(B, n, d, generator=g) * a for n, a in ((T_pad, 1.5), (C_pad, 1.5), (C_pad, 1.0)))
    w = torch.randn(B, T_pad, d, generator=g)
    w0 = w.clone()  # dO zeroed beyond the query count: what the existing export needs to compute the same d_k / d_v
    for b, n in enumerate(q_counts):
        w0[b, n:] = 0
    scale = 1.0 / math.sqrt(d)
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    n_q = torch.tensor(q_counts, dtype=torch.int32, device=DEV)

    def run(n_q_valid, dO, poison):
        Qx = Q.clone()
        if poison:  # (queries and dO beyond the count are never read: NaN there changes nothing)
            dO = dO.clone()
            for b, n in enumerate(q_counts):
                Qx[b, n:] = float("nan")
                dO[b, n:] = float("nan")
        Qd, Kd, Vd = (x.to(DEV).requires_grad_(True) for x in (Qx, K, V))
        with launch_witness() as wit:
            o_pt = FN.masked_attention(FN.pack_pt(Qd), FN.pack_pt(Kd), FN.pack_pt(Vd), n_valid, B, C_pad, T_pad, d, scale,
                                       n_q_valid=n_q_valid)
            o_pt.backward(FN.pack_pt(dO.to(DEV)))
            torch.cuda.synchronize()
        return FN.unpack_pt(o_pt.detach(), T_pad, d), Qd.grad, Kd.grad, Vd.grad, wit

    o1, dq1, dk1, dv1, w1 = run(n_q, w, poison=True)
    o0, dq0, dk0, dv0, w0_ = run(None, w0, poison=False)
    assert w1["npf_masked_attn_fwd_nq"] == 1 and w1["npf_masked_attn_bwd_nq"] == 1 and w1["npf_masked_attn_fwd"] == 0, w1
    assert w0_["npf_masked_attn_fwd"] == 1 and w0_["npf_masked_attn_fwd_nq"] == 0, w0_
    for b, n in enumerate(q_counts):
        assert torch.equal(o1[b, :n], o0[b, :n]) and torch.equal(dq1[b, :n], dq0[b, :n]), f"task {b}: rows below the query count {n}"
        assert (o1[b, n:] == 0).all() and (dq1[b, n:] == 0).all(), f"task {b}: rows beyond the query count {n}"
    assert torch.equal(dk1, dk0) and torch.equal(dv1, dv0)
    # against float64: the batch whose queries beyond the count carry no gradient
    r64 = _attention_and_grads(Q, K, V, w0, counts, scale, torch.float64)
    r32 = _attention_and_grads(Q, K, V, w0, counts, scale, torch.float32)
    for b, n in enumerate(q_counts):
        for r in (r64, r32):
            r[0][b, n:] = 0
            r[1][b, n:] = 0
    for i, (name, got, tol) in enumerate((("output", o1, 1e-5), ("dQ", dq1, 1e-4), ("dK", dk1, 1e-4), ("dV", dv1, 1e-4))):
        err = float((got.detach().cpu().double() - r64[i]).abs().max())
        print(f"d={d} C_pad={C_pad} T_pad={T_pad} {name}: max|d|={err:.3e} max|ref|={float(r64[i].abs().max()):.3e}")
        assert_gated(got, r64[i], r32[i], tol, f"{name} d={d} C_pad={C_pad} T_pad={T_pad}")


def test_query_counts_outside_the_range_are_clamped():
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(0)
    Q, K, V = (torch.randn(2, n, 64, generator=g).to(DEV) for n in (40, 50, 50))
    nv = torch.tensor([50, 20], device=DEV)
    run = lambda c: FN.masked_attention(FN.pack_pt(Q), FN.pack_pt(K), FN.pack_pt(V), nv, 2, 50, 40, 64, 0.125,  # noqa: E731
                                        n_q_valid=torch.tensor(c, device=DEV))
    assert torch.equal(run([-3, 10 ** 6]), run([0, 40]))
    full = FN.masked_attention(FN.pack_pt(Q), FN.pack_pt(K), FN.pack_pt(V), nv, 2, 50, 40, 64, 0.125)
    assert torch.equal(run([40, 40]), full)


# ---- whole models --------------------------------------------------------------------------------------------------------------
def _ragged_step(case, params, inp, t_counts, c_counts=None, train=True, spy=("x6.target_side",)):
    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    if "eps" in dinp:
        EpsIndependent.eps = dinp["eps"]
    kw = {}
    if t_counts is not None:
        kw["n_trgt"] = torch.tensor(t_counts, device=DEV)
    if c_counts is not None:
        kw["n_cntxt"] = torch.tensor(c_counts, device=DEV)
    crit = build_loss(case)
    model.train(train)
    crit.train(train)
    with launch_witness(spy=spy) as w:
        if not train:
            with torch.no_grad():
                out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], **kw)
            torch.cuda.synchronize()
            return model, out, None, w
        out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"], **kw)
        loss = crit(out, dinp["Y_trgt"])
        loss.backward()
        torch.cuda.synchronize()
    return model, out, loss, w


# ---- 3. padding is inert -------------------------------------------------------------------------------------------------------
INERT_CASES = {
    "cnp": ("CNP", 128, {}),
    "attncnp_scaledot_r256": ("AttnCNP", 256, {}),
    "attncnp_transformer_r128": ("AttnCNP", 128, dict(attention="transformer")),
    "attnlnp_qzcct_nz2": ("AttnLNP", 128, dict(is_q_zCct=True, n_z=2)),
}


@pytest.mark.parametrize("with_n_cntxt", (False, True))
@pytest.mark.parametrize("name", list(INERT_CASES))
def test_target_padding_is_inert(name, with_n_cntxt):
    """The same batch with the target padding rows refilled by other finite values in [-1, 1]: bit-identical loc / scale in the valid
    rows, loss and every gradient.  The zero rows the masked head stores in d_suff are what carries this through the decoder, the
    attention and the encoders without further masks."""
    kind, r, kw = INERT_CASES[name]
    C_pad = 200 if name == "attncnp_scaledot_r256" else 40  # (r = 256, 128 < C <= 256: the fused target side without n_cntxt)
    case = _case(kind, r, C_pad, **kw)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    t_counts = [0, 1, 33, 69, 70]
    c_counts = [0, 1, 33, C_pad - 1, C_pad] if with_n_cntxt else None
    inp["Y_cntxt"], inp["Y_trgt"] = inp["Y_cntxt"].clamp(-1, 1), inp["Y_trgt"].clamp(-1, 1)
    other = copy.deepcopy(inp)
    g = torch.Generator().manual_seed(9)
    for b, n in enumerate(t_counts):
        for k in ("X_trgt", "Y_trgt"):
            other[k][b, n:] = torch.rand(other[k][b, n:].shape, generator=g) * 2 - 1
    m1, o1, l1, w1 = _ragged_step(case, params, inp, t_counts, c_counts)
    m2, o2, l2, _ = _ragged_step(case, params, other, t_counts, c_counts)
    if name == "attncnp_scaledot_r256" and not with_n_cntxt:
        assert w1["x6.target_side"] == 1, w1  # the step kept its path: the fused target side ran
    assert w1["npf_masked_gauss_head_fwd"] >= 1 and w1["npf_masked_gauss_head_bwd"] == 1 and w1["npf_gauss_head_fwd"] == 0, w1
    if with_n_cntxt and kind.startswith("Attn"):
        assert w1["npf_masked_attn_fwd_nq"] == 1 and w1["npf_masked_attn_bwd_nq"] == 1 and w1["npf_masked_attn_fwd"] == 0, w1
    else:
        assert w1["npf_masked_attn_fwd_nq"] == 0, w1
    loc1, loc2, sc1, sc2 = o1[0].base_dist.loc, o2[0].base_dist.loc, o1[0].base_dist.scale, o2[0].base_dist.scale
    for b, n in enumerate(t_counts):
        assert torch.equal(loc1[:, b, :n], loc2[:, b, :n]) and torch.equal(sc1[:, b, :n], sc2[:, b, :n]), b
        assert (loc1[:, b, n:] == 0).all() and (sc1[:, b, n:] == 1).all() and (loc2[:, b, n:] == 0).all(), b
    assert torch.isfinite(l1) and torch.equal(l1, l2)
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), k
        if p1.grad is not None:
            assert torch.equal(p1.grad, p2.grad), k


# ---- 4. whole models against the per-task oracle -------------------------------------------------------------------------------
def _cut(inp, b, n_c, n_t):
    Xc, Yc = inp["X_cntxt"][b:b + 1], inp["Y_cntxt"][b:b + 1]
    if n_c is not None:
        Xc, Yc = Xc[:, :n_c], Yc[:, :n_c]
    return Xc, Yc, inp["X_trgt"][b:b + 1, :n_t], inp["Y_trgt"][b:b + 1, :n_t]


def _per_task_oracle(case, inp, params, c_counts, t_counts, training=True):
    """The oracle once per task on the batch cut to its counts; losses averaged, gradients accumulated on one dict.  loc / scale come
    back padded to T_pad with the documented padding values (0 / 1)."""
    cfg = specs.cfg_of(case)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    B, n_z, T_pad = case["B"], case.get("n_z", 1), case["T"]
    outs, total = [], 0.0
    for b, n_t in enumerate(t_counts):
        Xc, Yc, Xt, Yt = _cut(inp, b, None if c_counts is None else c_counts[b], n_t)
        eps = inp["eps"][:, b:b + 1] if "eps" in inp else None
        out = O.forward(cfg, p, Xc, Yc, Xt, Yt if training else None, eps=eps, n_z=n_z, training=training)
        if training:
            loss = LOSSES[specs.loss_name(case)](out, Yt, reduction=None).sum() / B
            loss.backward()
            total += float(loss.detach().double())
        outs.append(out)
    cat = lambda xs, dim: torch.cat([x.detach() for x in xs], dim=dim)  # noqa: E731

    def padded(key, fill):
        rows = []
        for o in outs:
            x = o[key].detach()
            rows.append(torch.cat([x, torch.full((x.shape[0], 1, T_pad - x.shape[2], x.shape[3]), fill, dtype=x.dtype)], dim=2))
        return torch.cat(rows, dim=1)

    ref = dict(loc=padded("loc", 0.0), scale=padded("scale", 1.0), z_samples=None, q_zCc=None, q_zCct=None)
    if outs[0]["z_samples"] is not None:
        ref["z_samples"] = cat([o["z_samples"] for o in outs], 1)
        for key in ("q_zCc", "q_zCct"):
            if outs[0][key] is not None:
                ref[key] = tuple(cat([o[key][i] for o in outs], 0) for i in range(2))
    return p, ref, total


def _reference_margin(case, inp, params, c_counts, t_counts):
    """The smallest |ReLU pre-activation| of the per-task oracle's train-mode forward on the cut batch (``O.RELU_MARGINS``)."""
    O.RELU_MARGINS = []
    try:
        with torch.no_grad():
            for b, n_t in enumerate(t_counts):
                Xc, Yc, Xt, Yt = _cut(inp, b, None if c_counts is None else c_counts[b], n_t)
                eps = inp["eps"][:, b:b + 1] if "eps" in inp else None
                O.forward(specs.cfg_of(case), params, Xc, Yc, Xt, Yt, eps=eps, n_z=case.get("n_z", 1), training=True)
        return min(O.RELU_MARGINS)
    finally:
        O.RELU_MARGINS = None


def _well_posed_inputs(case, params, c_counts, t_counts, first_seed=4321, tries=20000):
    """The rule of tests/test_hip_masked.py::_well_posed_inputs on the batch cut on both sides: the first seed from ``first_seed`` on
    for which no ReLU pre-activation of the oracle lies within ``RELU_TIE`` of zero.  It reads the reference alone."""
    for seed in range(first_seed, first_seed + tries):
        inp = specs.make_inputs(case, seed=seed)
        if _reference_margin(case, inp, params, c_counts, t_counts) >= RELU_TIE:
            return inp, seed
    raise AssertionError(f"no well-posed inputs in {tries} seeds")


RAGGED_CASES = dict(MODEL_CASES, cnp_homosk_r128=dict(kind="CNP", r=128, is_heteroskedastic=False))
RAGGED_PARAMS = [(name, T_pad) for name in RAGGED_CASES for T_pad in (70, 300)
                 if not (name == "attnlnp_scaledot_r256_nz8" and T_pad == 300)]  # (see the module docstring)


@pytest.mark.parametrize("both", (False, True), ids=("n_trgt", "n_trgt+n_cntxt"))
@pytest.mark.parametrize("name,T_pad", RAGGED_PARAMS)
def test_ragged_models_match_the_per_task_oracle(name, T_pad, both):
    """Train step (outputs, loss, every gradient) and evaluation forward against the oracle run once per task on the cut batch."""
    kw = dict(RAGGED_CASES[name])
    C_pad = 200
    case = _case(kw.pop("kind"), kw.pop("r"), C_pad, **dict(kw, T=T_pad))
    params = specs.make_params(case, seed=11)
    t_counts = [1, 33, T_pad - 1, T_pad, 17]
    c_counts = [0, 1, 33, 199, 200] if both else None
    inp, seed = _well_posed_inputs(case, params, c_counts, t_counts)
    for b, n in enumerate(t_counts):  # (zeros are the documented padding)
        inp["X_trgt"][b, n:] = 0
        inp["Y_trgt"][b, n:] = 0
        if both:
            inp["X_cntxt"][b, c_counts[b]:] = 0
            inp["Y_cntxt"][b, c_counts[b]:] = 0
    ref_p, ref_out, ref_loss = _per_task_oracle(case, inp, params, c_counts, t_counts)
    model, out, loss, w = _ragged_step(case, params, inp, t_counts, c_counts)
    print(f"{name} T_pad={T_pad} both={both}: input seed {seed}, loss {loss.item():.8g} ref {ref_loss:.8g}")
    _compare_outputs(out, ref_out)
    for b, n in enumerate(t_counts):
        assert (out[0].base_dist.loc[:, b, n:] == 0).all() and (out[0].base_dist.scale[:, b, n:] == 1).all()
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=2e-5)
    _compare_grads(model, ref_p)
    # the path: the masked head always; query counts in the masked attention with n_cntxt only
    attentive = case["kind"].startswith("Attn")
    assert w["npf_masked_gauss_head_fwd"] >= 1 and w["npf_masked_gauss_head_bwd"] == 1, w
    assert w["npf_gauss_head_fwd"] == 0 and w["npf_gauss_head_bwd"] == 0, w
    assert w["npf_masked_attn_fwd_nq"] == w["npf_masked_attn_bwd_nq"] == int(attentive and both), w
    assert w["npf_masked_attn_fwd"] == 0 and w["npf_masked_attn_bwd"] == 0, w
    if not both:
        fused = (case["kind"] == "AttnCNP" or case.get("n_z") == 1) and case["r"] == 256 and "attention" not in case and attentive
        assert w["x6.target_side"] == int(fused), w  # (without n_cntxt the step keeps its path)
    # evaluation-mode forward without targets
    _, out_e, _, _ = _ragged_step(case, params, inp, t_counts, c_counts, train=False)
    _, ref_e, _ = _per_task_oracle(case, inp, params, c_counts, t_counts, training=False)
    _compare_outputs(out_e, ref_e, what="(eval)")


# ---- 5. full counts reproduce the call without n_trgt; 6. without it none of the new exports runs --------------------------
@pytest.mark.parametrize("with_n_cntxt", (False, True))
@pytest.mark.parametrize("name", ["cnp_r256", "cnp_homosk_r128", "lnp_latent_nz4", "attncnp_scaledot_r128", "attncnp_scaledot_r256",
                                  "attncnp_transformer_r128", "attnlnp_scaledot_r256_nz1"])
def test_full_target_counts_reproduce_the_call_without_them(name, with_n_cntxt):
    kw = dict(RAGGED_CASES[name])
    case = _case(kw.pop("kind"), kw.pop("r"), 200, **kw)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    c_counts = [0, 1, 33, 199, 200] if with_n_cntxt else None
    m1, o1, l1, w1 = _ragged_step(case, params, inp, [70] * 5, c_counts)
    m0, o0, l0, w0 = _ragged_step(case, params, inp, None, c_counts)
    assert all(w0[k] == 0 for k in NEW), w0  # 6. a step without n_trgt calls none of the new exports
    assert w1["npf_masked_gauss_head_fwd"] >= 1 and w1["npf_masked_gauss_head_bwd"] == 1, w1
    assert w1["x6.target_side"] == w0["x6.target_side"], (w1, w0)
    # loc / scale: only the head changed on the path without n_cntxt, and the query-count instances are bit-identical below
    # the counts on the path with it (the target-side latent mean is a different kernel: gated there)
    if case["kind"] in ("CNP", "AttnCNP"):
        assert torch.equal(o1[0].base_dist.loc, o0[0].base_dist.loc) and torch.equal(o1[0].base_dist.scale, o0[0].base_dist.scale)
    else:
        assert_close(o1[0].base_dist.loc, o0[0].base_dist.loc.detach().cpu(), what="loc")
        assert_close(o1[0].base_dist.scale, o0[0].base_dist.scale.detach().cpu(), what="scale")
    np.testing.assert_allclose(l1.item(), l0.item(), rtol=2e-5)
    _compare_grads(m1, {k: p for k, p in m0.named_parameters()})


def test_library_version_is_unchanged():
    from npf_gwwaveform_amd import _lib as L

    assert L.load().npf_version() == 2


def test_sum_log_prob_and_eval_loglike_mask_themselves():
    """The loss classes keep their signature: the distribution carries the counts.  ``reduction=None`` gives per-task sums over the
    valid rows, a task without targets contributes 0, and ``eval_loglike`` passes ``batch["n_trgt"]``."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.evaluate import eval_loglike

    case = _case("CNP", 128, 40)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    model = build_model(case, DEV, params=params)
    d = {k: v.to(DEV) for k, v in inp.items()}
    t_counts = [0, 1, 33, 69, 70]
    batch = dict(X_cntxt=d["X_cntxt"], Y_cntxt=d["Y_cntxt"], X_trgt=d["X_trgt"], Y_trgt=d["Y_trgt"],
                 n_trgt=torch.tensor(t_counts, device=DEV))
    ll = eval_loglike(model, A.CNPFLoss(), [batch])
    assert ll.shape == (5,) and ll[0] == 0.0
    for b, n in enumerate(t_counts):
        if n == 0:
            continue
        one = dict(X_cntxt=d["X_cntxt"][b:b + 1], Y_cntxt=d["Y_cntxt"][b:b + 1], X_trgt=d["X_trgt"][b:b + 1, :n].contiguous(),
                   Y_trgt=d["Y_trgt"][b:b + 1, :n].contiguous())
        np.testing.assert_allclose(ll[b], eval_loglike(model, A.CNPFLoss(), [one])[0], rtol=2e-5)


# ---- 7. one graph, many sizes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("AttnCNP", "AttnLNP"))
def test_one_captured_graph_serves_every_mix_of_both_counts(kind):
    """Trainer(use_graph=True), r = 128, C_pad = 64, T_pad = 50, 12 Adam steps whose context AND target counts change every step
    (some steps with a task at n_trgt = 0), against an eager Trainer on a copy of the model fed the same batches: same losses and
    final parameters, and the step is captured exactly once."""
    import warnings

    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer, synthetic_waveform_batch

    B, C_pad, T_pad = 8, 64, 50
    eps = torch.randn(1, B, 1, 128, generator=torch.Generator().manual_seed(1)).to(DEV)

    def batch(i):
        b = synthetic_waveform_batch(B, C_pad, T_pad, 500 + i, DEV)
        g = torch.Generator().manual_seed(i)
        n_c = torch.randint(0, C_pad + 1, (B,), generator=g).to(DEV)
        n_t = torch.randint(1, T_pad + 1, (B,), generator=g)
        if i % 3 == 0:
            n_t[i % B] = 0  # a task without targets
        n_t = n_t.to(DEV)
        for cnt, keys, P in ((n_c, ("X_cntxt", "Y_cntxt"), C_pad), (n_t, ("X_trgt", "Y_trgt"), T_pad)):
            pad = (torch.arange(P, device=DEV).unsqueeze(0) >= cnt.unsqueeze(1)).unsqueeze(-1)
            for k in keys:
                b[k] = b[k].masked_fill(pad, 0.0)
        b["n_cntxt"], b["n_trgt"] = n_c, n_t
        return b

    def run(use_graph):
        torch.manual_seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if kind == "AttnCNP":
                model, crit = A.AttnCNP(1, 2, r_dim=128).to(DEV), A.CNPFLoss()
            else:
                # (the same injected noise eagerly and in the replayed graph, as test_graph_captured_step_equals_eager_step_latent_model)
                model = A.AttnLNP(1, 2, r_dim=128, is_q_zCct=True, n_z_samples_train=1, n_z_samples_test=1,
                                  LatentDistribution=eps_latent_dist).to(DEV)
                EpsIndependent.eps = eps
                crit = A.ELBOLossLNPF()
        tr = Trainer(model, crit, lr=1e-3, world=1, use_graph=use_graph)
        losses, graphs = [], []
        for i in range(12):
            losses.append(float(tr.step(batch(i))))
            graphs.append(tr._graph)
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, tr, graphs

    l_e, p_e, _, _ = run(False)
    l_g, p_g, tr, graphs = run(True)
    assert tr._graph is not None and tr.n_captures == 1
    assert all(g is tr._graph for g in graphs[3:]), "the graph was captured again"
    print("losses eager", l_e, "graph", l_g)
    assert all(math.isfinite(x) for x in l_e)
    np.testing.assert_allclose(l_g, l_e, rtol=1e-6)
    for k in p_e:
        assert torch.allclose(p_g[k], p_e[k], rtol=1e-6, atol=1e-8), k
