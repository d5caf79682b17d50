"""Parity gate of the bf16 compute mode (BASELINE configs 3 and 4-bf16): the HIP path
with ``set_compute_dtype("bf16")`` against the oracle's bf16 emulation (``oracle.npf_oracle.matmul_mode``:
the pinned fp32 restatement with every contraction's operands rounded to bfloat16 exactly where the kernels
round them -- weights, layer inputs, keys / values, probabilities, and in the backward pass dZ, dO, dS and
the saved activations).  Forward outputs, latent statistics, the loss and EVERY gradient tensor in full are
compared.

What the tolerance is made of (measured on MI355X, gpurun_out/r2c/diag.log): on about half of the cases the
HIP result equals the emulation to fp32 rounding (outputs 1e-7, gradients 1e-6 of max|ref|) -- the emulation
models every rounding point of the kernels.  On the others a handful of activations sit within fp32
summation-order noise of a bf16 rounding boundary (expected: 5e-5 of the elements) and round the other way on
the GPU; one such flip moves that point's outputs by ~1e-3 .. 1e-2 of max|ref| and, summed over the points,
a gradient tensor by up to a few 1e-3 in relative L2 norm.  Both results are valid bf16-mode results.  The gate
is therefore a full-tensor relative L2 error (outputs 5e-3, gradients 1e-2) plus a max-norm cap of 3e-2, and
the requirement that the HIP result is closer to the bf16 emulation than to the fp32 oracle (which is 2e-2 ..
4e-1 away on the gradients): a wrong-but-correlated bf16 backward cannot pass this, a missing rounding
step shows up as a distance of the fp32-vs-bf16 size.

That end-to-end comparison is a SANITY bound.  The gate proper is teacher-forced (tests/teacher.py,
``test_bf16_mode_teacher_forced`` and inside every end-to-end case): each LINEAR, softmax, attention contraction, dgrad
step and weight / key / value gradient of the step is recomputed from the tensors the HIP launch itself stored as that
step's input and compared at fp32-accumulation tolerances (2e-6 of max|ref| per step, 1e-5 for sums over all points) --
a flipped rounding cannot propagate through such a check, so it has no exception list.  The end-to-end bound may only
be exceeded when the teacher-forced gate is clean AND the run contains flipped roundings, which the test prints."""
import numpy as np
import pytest
import torch

import specs
from helpers import EpsIndependent, assert_close, build_loss, build_model
from test_hip_sweep import SWEEP, _oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_OUT_L2, TOL_GRAD_L2, TOL_MAX = 5e-3, 1e-2, 3e-2
# the end-to-end bound on a gradient tensor when (and only when) the run holds flipped roundings that the test lists and
# every teacher-forced check is clean: one flipped unit of a contraction over a handful of rows is a visible share of
# every upstream gradient (8 tasks x 2 latent samples: 5.5e-2 L2 / 1.4e-1 max-norm with outputs at 1.6e-3)
SANITY_L2, SANITY_MAX = 1e-1, 2.5e-1


def _errs(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    d = got - ref
    return float(d.norm() / max(float(ref.norm()), 1e-30)), float(d.abs().max() / max(float(ref.abs().max()), 1e-30))


def _check(got, ref, tol_l2, tol_max, what):
    l2, mx = _errs(got, ref)
    assert l2 <= tol_l2 and mx <= tol_max, f"{what}: rel L2 {l2:.2e} (<= {tol_l2:.0e}), max-norm {mx:.2e} (<= {tol_max:.0e})"
    return l2

CASES = {k: specs.CASES[k] for k in ("g1_cnp_c1", "g2_lnp_both_c1", "g2_lnp_latent_c1", "g3s_attncnp_r64", "g4s_attnlnp_r64",
                                     "g4s_attnlnp_r64_noqzcct", "g6_attncnp_ragged", "g6_attncnp_c1pt", "g6_cnp_homosk",
                                     "g6_attncnp_r128", "g10_attnlnp_nll_nz8")}
CASES.update({k: SWEEP[k] for k in ("cnp_r48", "cnp_r100_dx3_dy1", "cnp_r200_L1", "lnp_latent_nz3_r40", "lnp_both_nz2_r72",
                                    "attncnp_r96", "attncnp_r160_c255", "attncnp_r256_c256_t100", "attncnp_r44",
                                    "attnlnp_nz3_r64", "attnlnp_nz2_r104_noq",
                                    # BASELINE config 3's model and point counts (batch 2): full gradients
                                    "attncnp_c2_full", "attnlnp_c2_full",
                                    # residual layers on the ring pipeline, kq width != value width
                                    "attncnp_r256_res", "attncnp_xt128_r256")})
# r = 256 on both sides of the fused target side's switch (C = 128 / 129: chain attention / b16 program) and past one score row
# (C = 257: the attention in fp32, blocked, the decoder in bf16)
CASES.update({f"attncnp_r256_c{C}": dict(kind="AttnCNP", r=256, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=C, T=70) for C in (128, 129, 257)})


def _hip_bf16(case, inp, params, trace=None):
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import chain as CH

    CH.TRACE = trace
    try:
        return _hip_bf16_run(A, case, inp, params)
    finally:
        CH.TRACE = None


def _hip_bf16_run(A, case, inp, params):
    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    if "eps" in dinp:
        EpsIndependent.eps = dinp["eps"]
    crit = build_loss(case)
    model.train()
    crit.train()
    A.set_compute_dtype("bf16")
    try:
        out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
        loss = crit(out, dinp["Y_trgt"])
        loss.backward()
    finally:
        A.set_compute_dtype("fp32")
    return model, out, loss


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_mode_matches_the_bf16_oracle(name):
    case = CASES[name]
    _gate(name, case, specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321))


@pytest.mark.parametrize("name", ["g14_cnp_res", "g14_attncnp_res", "g14_cnp_xt", "g14_lnp_xt", "g14_attncnp_xt", "g14_attnlnp_xt"])
def test_bf16_mode_variants(name):
    """Residual MLPs and x_transf_dim != r_dim in the bf16 compute mode (the residual itself is an fp32 add of the
    layer's fp32 input on both sides), on the reference-constructed parameters of the G14 fixtures."""
    case = specs.VARIANT_CASES[name]
    _gate(name, case, specs.golden_params(specs.load_golden(name)), specs.make_inputs(case, seed=4321))


def _teacher_forced(trace, name):
    """The gate proper: every step of every chain launch against the launch's own stored inputs (tests/teacher.py)."""
    import teacher

    rep = teacher.check_trace(trace)
    bad = rep.failures()
    assert rep.rows and not bad, f"{name}: teacher-forced checks failed:\n" + "\n".join(f"  {w}: {e:.3e} > {t:.0e}" for w, e, t in bad[:20])
    print(f"{name}: {rep.summary()}")
    return rep


# the shape of the randomised sweep's case that landed at 5.5e-3 on ``loc`` against the 5e-3 end-to-end bound in round 2 (CNP,
# r = 256, residual layers, TWO tasks: one flipped rounding in the pooled representation moves a whole task's outputs)
CNP_RES_2TASKS = dict(kind="CNP", r=256, L_xy=2, L_dec=3, dx=1, dy=2, B=2, C=31, T=65, is_res=True)


@pytest.mark.parametrize("name", ["g3_attncnp_c2", "g4_attnlnp_c2", "cnp_r256_res_2tasks"])
def test_bf16_mode_teacher_forced(name):
    """BASELINE config 3's models at batch 2 (AttnCNP; AttnLNP with the target-side latent encode) and a two-task CNP with
    residual 256-wide layers: every layer's output, dX and dW from the HIP path's own stored inputs (tests/teacher.py)."""
    if name == "cnp_r256_res_2tasks":
        case = CNP_RES_2TASKS
        params, inp = specs.make_params(case, seed=170), specs.make_inputs(case, seed=270)
    else:
        case = specs.CASES[name]
        params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    trace = []
    _hip_bf16(case, inp, params, trace=trace)
    rep = _teacher_forced(trace, name)
    assert any(rec[1].bf16 if rec[0] == "prog" else (rec[0] in ("fwd", "bwd") and rec[5]) for rec in trace), \
        "nothing ran on the bf16 instances"
    for f in rep.flips:
        print("  flip:", f)


def _gate(name, case, params, inp):
    ref_p, ref_out, ref_loss = _oracle(case, inp, params, mode="bf16")
    fp_p, fp_out, _ = _oracle(case, inp, params, mode="fp32")
    trace = []
    model, out, loss = _hip_bf16(case, inp, params, trace=trace)
    rep = _teacher_forced(trace, name)

    _check(out[0].base_dist.loc, ref_out["loc"], TOL_OUT_L2, TOL_MAX, "loc")
    _check(out[0].base_dist.scale, ref_out["scale"], TOL_OUT_L2, TOL_MAX, "scale")
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    if out[1] is not None:
        _check(out[1], ref_out["z_samples"], TOL_OUT_L2, TOL_MAX, "z_samples")
        _check(out[2].base_dist.loc, ref_out["q_zCc"][0], TOL_OUT_L2, TOL_MAX, "q_zCc.loc")
        _check(out[2].base_dist.scale, ref_out["q_zCc"][1], TOL_OUT_L2, TOL_MAX, "q_zCc.scale")
    worst = worst32 = 0.0
    over = []
    for k, p in model.named_parameters():
        ref = ref_p[k].grad if ref_p[k].grad is not None else torch.zeros_like(ref_p[k])
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        if float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, k
            continue
        l2, mx = _errs(got, ref)
        if l2 > TOL_GRAD_L2 or mx > TOL_MAX:
            over.append((k, l2, mx))
            _check(got, ref, SANITY_L2, SANITY_MAX, f"grad {k}")
        worst = max(worst, l2)
        if fp_p[k].grad is not None:
            worst32 = max(worst32, _errs(got, fp_p[k].grad)[0])
    if over:
        # beyond the end-to-end bound: only with flipped roundings on record (the teacher-forced gate above was clean)
        assert rep.n_flips > 0, f"{name}: gradients beyond the end-to-end bound without a flipped rounding: {over}"
        print(f"{name}: {len(over)} gradient tensor(s) beyond the end-to-end bound ({TOL_GRAD_L2:.0e} L2 / {TOL_MAX:.0e} max), "
              f"worst {max(o[1] for o in over):.2e} L2; {rep.n_flips} flipped roundings in the run, e.g.")
        for f in rep.flips[:6]:
            print("  flip:", f)
    # the bf16 instances really ran, and the emulation -- not the fp32 oracle -- is what they compute
    l2_16, l2_32 = _errs(out[0].base_dist.loc, ref_out["loc"])[0], _errs(out[0].base_dist.loc, fp_out["loc"])[0]
    assert l2_32 > 1e-4 and l2_16 < 0.6 * l2_32, (l2_16, l2_32)
    if not over:
        assert worst < 0.6 * worst32, (worst, worst32)
    print(f"{name}: loc rel L2 {l2_16:.1e} (fp32 oracle: {l2_32:.1e}); worst gradient rel L2 {worst:.1e} (fp32 oracle: {worst32:.1e})")


@pytest.mark.parametrize("name", ["g3_attncnp_c2", "g4_attnlnp_c2", "g1_cnp_c1"])
def test_fused_layer_stores_change_nothing(name, monkeypatch):
    """NPF_F_STORE_IN / NPF_F_STORE_BITS (a STORE_PT in front of a bf16 LINEAR and a STORE_MASK behind a ReLU layer ride
    inside the layer) move stores, not arithmetic, and PAD_SMALL_K (a <= 32-input layer behind LOAD_ROWS run
    as a zero-padded 256-input pipelined layer) only adds exact zeros: outputs, loss and every gradient are BIT-identical
    to the same step with both switched off (NPF_NO_FUSED_STORE, NPF_NO_PAD_SMALL_K)."""
    from npf_gwwaveform_amd import chain as CH

    case = specs.CASES[name] if name in specs.CASES else CASES[name]
    params = specs.make_params(case, seed=11)
    inp = specs.make_inputs(case, seed=4321)
    runs = []
    for fuse in (True, False):
        monkeypatch.setattr(CH, "FUSE_STORES", fuse)
        monkeypatch.setattr(CH, "PAD_SMALL_K", fuse)
        model, out, loss = _hip_bf16(case, inp, params)
        runs.append((out[0].base_dist.loc.detach().clone(), out[0].base_dist.scale.detach().clone(), loss.detach().clone(),
                     {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}))
    (loc_a, sc_a, loss_a, g_a), (loc_b, sc_b, loss_b, g_b) = runs
    assert torch.equal(loc_a, loc_b) and torch.equal(sc_a, sc_b) and torch.equal(loss_a, loss_b)
    for k in g_a:
        assert (g_a[k] is None) == (g_b[k] is None), k
        if g_a[k] is not None:
            assert torch.equal(g_a[k], g_b[k]), k


def test_full_size_config3_properties():
    """BASELINE config 3 at full size (bf16 mode, 1024 tasks x 1024 targets): the size-independent properties
    of test_hip_models.py::test_full_size_config2_properties, in the bf16 compute mode.  Task and target
    independence hold exactly in exact arithmetic and to fp32 rounding here (the rounding points do not depend
    on the batch); gradient linearity over the batch to the bf16 gate."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import synthetic_waveform_batch

    B = 1024
    case = dict(specs.CASES["g3_attncnp_c2"], B=B)
    model = build_model(case, DEV).train()
    batch = synthetic_waveform_batch(B, case["C"], case["T"], 7, DEV)
    crit = A.CNPFLoss()
    A.set_compute_dtype("bf16")
    try:
        p = model(batch["X_cntxt"], batch["Y_cntxt"], batch["X_trgt"], batch["Y_trgt"])[0]
        loc, scale = p.base_dist.loc.detach(), p.base_dist.scale.detach()
        assert torch.isfinite(loc).all() and torch.isfinite(scale).all() and (scale >= 0.01).all()
        for i in (0, 517, 1023):
            one = {k: v[i:i + 1] for k, v in batch.items()}
            pi = model(one["X_cntxt"], one["Y_cntxt"], one["X_trgt"], one["Y_trgt"])[0]
            assert_close(pi.base_dist.loc, loc[:, i:i + 1], tol=1e-5, what=f"task {i} alone: loc")
            assert_close(pi.base_dist.scale, scale[:, i:i + 1], tol=1e-5, what=f"task {i} alone: scale")
        sub = slice(100, 357)
        ps = model(batch["X_cntxt"], batch["Y_cntxt"], batch["X_trgt"][:, sub], batch["Y_trgt"][:, sub])[0]
        assert_close(ps.base_dist.loc, loc[:, :, sub], tol=1e-5, what="target subset: loc")
        perm = torch.randperm(batch["X_cntxt"].shape[1], device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        pp = model(batch["X_cntxt"][:, perm], batch["Y_cntxt"][:, perm], batch["X_trgt"], batch["Y_trgt"])[0]
        _check(pp.base_dist.loc, loc, TOL_OUT_L2, TOL_MAX, "context permutation: loc")

        def grads(lo, hi):
            model.zero_grad(set_to_none=True)
            b = {k: v[lo:hi] for k, v in batch.items()}
            out = model(b["X_cntxt"], b["Y_cntxt"], b["X_trgt"], b["Y_trgt"])
            loss = crit(out, b["Y_trgt"])
            loss.backward()
            return loss.item(), {k: q.grad.clone() for k, q in model.named_parameters()}

        l_full, g_full = grads(0, B)
        l_a, g_a = grads(0, B // 2)
        l_b, g_b = grads(B // 2, B)
    finally:
        A.set_compute_dtype("fp32")
    np.testing.assert_allclose(l_full, 0.5 * (l_a + l_b), rtol=1e-5)
    for k in g_full:
        assert_close(g_full[k], 0.5 * (g_a[k] + g_b[k]), tol=1e-4, what=f"grad linearity {k}")
