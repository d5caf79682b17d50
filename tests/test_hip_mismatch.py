"""Differentiable waveform mismatch on the GPU: ``npf_waveform_match_bwd`` against the float64 closed form of
tests/mismatch_reference.py (checked on the CPU by tests/test_mismatch_host.py against autograd of the definition and a finite
difference) over the seven input regimes, exact zeros, ``n_bcast``, the bit-for-bit promises, ``HeadDistribution.mismatch`` of a
deterministic and a latent model down to the parameter gradients, the bf16 compute mode, and ``MismatchLoss`` in a captured
``Trainer`` step.

Gate per element (mismatch_reference.gate_ratio): |d - ref| <= 2^-23 |ref| + 1e-9 |d_match| / n_bcast * s_t with
s_t = w_t (|A'_t| / N + M |A_t| / hh) -- the forward's own gate shape: double arithmetic rounded to fp32 once (2^-23: one rounding with
a factor 2), the absolute term for the cancellation of the two dA terms (double sums of T <= 200 terms with ulp-level sines err by
some 1e-13 of s_t; the CPU suite shows that fp32 row scalars would exceed it 17 times).  Every test prints its worst error / gate."""
import numpy as np
import pytest
import torch

import match_reference as R
import mismatch_reference as G
from helpers import assert_close
from test_hip_match import _clear_maximum, _observation
from test_hip_predict import ROUTES, _counts, _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# round(x / 3) against round(x) / 3: half an ulp of each, 2^-24 |x / 3| twice, measured on round(x) / 3 (a further 2^-24 relative);
# 2^-148 for results in the subnormal range
ONE_ROUNDING = 2.0 ** -23 * (1.0 + 2.0 ** -20)


@pytest.fixture(scope="module")
def all_cases():
    """(tag, factors, case, reference, d_match [R]) of every case, computed once and left unchanged."""
    from npf_gwwaveform_amd import functional as FN

    out = []
    for i, (tag, fac, case) in enumerate(G.cases(FN.MATCH_JC)):
        ref = R.reference(**R.call_args(case))
        out.append((tag, fac, case, ref, torch.randn(case["h"].shape[0], generator=torch.Generator().manual_seed(300 + i))))
    return out


def _dev(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.call_args(case).items()}


def _grad(args, d_match):
    """(mismatch [R], d_h) through the public path: h.grad for the incoming gradient ``d_match`` of the MATCH (mismatch = 1 - match,
    and the negation of an fp32 number is exact)."""
    from npf_gwwaveform_amd import functional as FN

    h = args["h"].clone().requires_grad_()
    mm = FN.waveform_mismatch(**dict(args, h=h))
    mm.backward(-d_match.to(DEV))
    return mm.detach(), h.grad


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.REGIMES)
def test_gradient_meets_the_float64_closed_form(regime, all_cases):
    from npf_gwwaveform_amd import functional as FN

    worst, n = 0.0, 0
    for tag, fac, case, ref, d_match in all_cases:
        if fac["regime"] != regime:
            continue
        n += 1
        args = _dev(case)
        mm, got = _grad(args, d_match)
        fwd = FN.waveform_match(**args)
        assert torch.equal(mm, fwd.mismatch), f"{tag}: the forward value differs from waveform_match(...).mismatch"
        mm2, again = _grad(args, d_match)
        assert torch.equal(mm, mm2) and torch.equal(got, again), f"{tag}: d_h differs between two calls"
        got = got.cpu()
        assert got.shape == case["h"].shape and torch.isfinite(got).all(), tag
        want, s, _ = G.expected(case, d_match, ref=ref)
        r = G.gate_ratio(got[..., :2], want, s)
        print(f"MISMATCH {tag}: error / gate {r:.3g}")
        worst = max(worst, r)
        assert r <= 1.0, (tag, r)
        # exact zeros: entries 2 .. of a raw decoder row, removed points, points beyond the counts, degenerate rows
        n_z, T = fac["n_z"], fac["T"]
        assert (got[..., 2:] == 0).all(), tag
        assert (got[..., :2][s == 0] == 0).all(), tag
        if regime == "removed":
            kill = case["kill"].repeat(n_z, 1)
            assert kill.any() and torch.isnan(case["h"][kill]).all() and torch.isnan(case["g"][case["kill"]]).all(), tag
            assert (got[kill] == 0).all(), tag
        if fac["counts"] is not None:
            beyond = (torch.arange(T).view(1, T) >= torch.tensor(fac["counts"]).view(-1, 1)).repeat(n_z, 1)
            assert (got[beyond] == 0).all(), tag
        assert (got[ref["degenerate"]] == 0).all(), tag
        if regime == "degenerate" and fac["wform"] == "T":
            assert ref["degenerate"].all() and (got == 0).all(), tag
        live = ~ref["degenerate"]
        if regime == "same":  # (the reference mismatch is ~0: the regime fine-tuning lives in, and the same gate holds)
            assert float(ref["mismatch"][live].abs().max()) <= 1e-12, tag
        if regime == "shift":  # (the gradient is taken at the planted index)
            assert (fwd.tau_index.cpu()[live] == case["j_star"]).all() and (ref["tau_index"][live] == case["j_star"]).all(), tag
    assert n >= 10
    print(f"MISMATCH worst error / gate over the {n} cases of regime {regime}: {worst:.3g}")


def test_every_element_is_written_for_any_leading_dimension_and_n_bcast():
    """The raw call on a d_h poisoned with NaN: dh_ld = 2, 3 (the generic stores), 4 and 5, n_bcast = 1 and 3, on a removed-points
    case with counts.  Every element is written; the row blocks are bit-identical; entries 0 and 1 equal those of the public path
    (dh_ld = h_ld) bit for bit, whatever dh_ld; with n_bcast = 3 they equal a third of them within one fp32 rounding."""
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    case = R.build("removed", 37, n_z=3, h_ld=4, wform="BT", fform="T", taus=R.grid(FN.MATCH_JC + 1), counts=(37, 17, 0), seed=12)
    args = _dev(case)
    Rn, T = case["h"].shape[:2]
    d_match = torch.randn(Rn, generator=torch.Generator().manual_seed(8)).to(DEV)
    _, public = _grad(args, d_match.cpu())
    geo = FN.check_match_args(args["h"].shape, args["g"], args["weights"], args["freqs"], args["taus"])
    nv = FN.counts_i32(args["n_valid"], R.B)
    saved = torch.empty(Rn, 4, dtype=torch.float64, device=DEV)
    m = FN._match_launch(args["h"], args["g"], args["weights"], args["freqs"], nv, geo, ("tau_index",), False, saved)
    assert (saved.cpu()[2::3] == 0).all() and (saved.cpu()[0::3] != 0).all()  # (the task with no point: a degenerate row saves zeros)

    def raw(n_bcast, dh_ld):
        d_h = torch.full((n_bcast * Rn, T, dh_ld), float("nan"), device=DEV)
        rc = L.load().npf_waveform_match_bwd(L.ptr(args["h"]), 4, L.ptr(args["g"]), L.ptr(args["weights"]), geo[4], L.ptr(args["freqs"]),
                                             geo[5], nv.data_ptr(), Rn, R.B, T, geo[6], geo[7], geo[8], m.tau_index.data_ptr(),
                                             saved.data_ptr(), L.ptr(d_match), n_bcast, L.ptr(d_h), dh_ld, L.stream_ptr())
        assert rc == 0
        return d_h

    for dh_ld in (2, 3, 4, 5):
        one = raw(1, dh_ld)
        assert torch.isfinite(one).all(), dh_ld
        assert torch.equal(one[..., :2], public[..., :2]) and (one[..., 2:] == 0).all(), dh_ld
        three = raw(3, dh_ld).view(3, Rn, T, dh_ld)
        assert torch.isfinite(three).all(), dh_ld
        assert torch.equal(three[0], three[1]) and torch.equal(three[0], three[2]) and (three[..., 2:] == 0).all(), dh_ld
        third = one.double()[..., :2] / 3.0
        d = (three[0].double()[..., :2] - third).abs()
        assert (d <= ONE_ROUNDING * third.abs() + 2.0 ** -148).all(), (dh_ld, float(d.max()))
        assert (three[0][..., :2][one[..., :2] == 0] == 0).all(), dh_ld


def test_n_bcast_through_the_public_call(all_cases):
    """``waveform_mismatch(samples, ..., n_bcast=3, mean=h)``: the gradient of the samples is the n_bcast = 1 gradient of ``h`` divided
    by 3 within one fp32 rounding, in three bit-identical row blocks, whatever the samples hold."""
    from npf_gwwaveform_amd import functional as FN

    tag, fac, case, ref, d_match = next(c for c in all_cases if c[1]["regime"] == "random" and c[1]["n_tau"] == 257 and c[1]["T"] == 200)
    args = _dev(case)
    Rn, T = case["h"].shape[:2]
    mm1, g1 = _grad(args, d_match)
    samples = torch.randn(3 * Rn, T, 4, device=DEV, requires_grad=True)
    mm = FN.waveform_mismatch(**dict(args, h=samples), n_bcast=3, mean=args["h"])
    assert torch.equal(mm, mm1), tag
    mm.backward(-d_match.to(DEV))
    g3 = samples.grad.view(3, Rn, T, 4)
    assert torch.equal(g3[0], g3[1]) and torch.equal(g3[0], g3[2]) and (g3[..., 2:] == 0).all(), tag
    third = g1.double()[..., :2] / 3.0
    assert ((g3[0].double()[..., :2] - third).abs() <= ONE_ROUNDING * third.abs() + 2.0 ** -148).all(), tag
    want, s, _ = G.expected(case, d_match, n_bcast=3, ref=ref)
    r = G.gate_ratio(g3[0][..., :2], want, s)
    print(f"MISMATCH n_bcast=3 {tag}: error / gate {r:.3g}")
    assert r <= 1.0


def test_saved_scalars_leave_every_other_output_unchanged(all_cases):
    """``npf_waveform_match_ex`` with ``saved``: every output of ``npf_waveform_match`` keeps its bits, and ``saved`` holds hh, gg and
    c at the index in double: hh and gg (plain sums of T <= 200 terms) to 1e-12 of the float64 reference, c / sqrt(hh gg) to 1e-10 --
    the recurrence form differs from the direct one by up to 1e-12 on the CPU, and 1e-10 is still 600 times below one fp32 rounding,
    which is what shows that the values are unrounded; zeros for a degenerate row."""
    from npf_gwwaveform_amd import functional as FN

    seen = 0
    for tag, fac, case, ref, _ in all_cases:
        if fac["T"] == 200 and fac["n_tau"] not in (None, 257):
            continue
        seen += 1
        args = _dev(case)
        plain = FN.waveform_match(**args, corr=True)
        geo = FN.check_match_args(args["h"].shape, args["g"], args["weights"], args["freqs"], args["taus"])
        nv = FN.counts_i32(args["n_valid"], R.B) if args["n_valid"] is not None else None
        Rn = case["h"].shape[0]
        saved = torch.full((Rn, 4), float("nan"), dtype=torch.float64, device=DEV)
        f = args["freqs"] if geo[8] > 0 else None
        ex = FN._match_launch(args["h"], args["g"], args["weights"], f, nv, geo, FN.MATCH_NAMES, True, saved)
        for name, a, b in zip(plain._fields, plain, ex):
            assert torch.equal(a, b), f"{tag}: {name} changes when saved is given"
        sv, deg = saved.cpu(), ref["degenerate"]
        assert torch.isfinite(sv).all() and (sv[deg] == 0).all(), tag
        nrm = (ref["hh"] * ref["gg"].repeat(Rn // R.B)).sqrt()
        cb = ref["corr"][torch.arange(Rn), ref["tau_index"]]  # normalised (Re, Im) at the index
        live = ~deg
        assert ((sv[live, 0] - ref["hh"][live]).abs() <= 1e-12 * ref["hh"][live]).all(), tag
        assert ((sv[live, 1] - ref["gg"].repeat(Rn // R.B)[live]).abs() <= 1e-12 * ref["gg"].repeat(Rn // R.B)[live]).all(), tag
        assert ((sv[live, 2:] / nrm[live].view(-1, 1) - cb[live]).abs() <= 1e-10).all(), tag
    assert seen >= 30


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _forward(model, Xc, Yc, Xt, n_trgt, seed=9):
    torch.manual_seed(seed)  # (a latent model draws its samples from the global stream)
    return model(Xc, Yc, Xt, **(dict(n_trgt=n_trgt) if n_trgt is not None else {}))


@pytest.mark.parametrize("of", ("samples", "mean"))
@pytest.mark.parametrize("name,latent", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True)])
def test_gradient_at_the_raw_decoder_output_equals_the_closed_form(name, latent, of):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    Y, w, f, taus = _observation(case, 41)
    n_trgt = _counts(Bn, T, 6, T // 2) if latent else None
    p = _forward(model, Xc, Yc, Xt, n_trgt)[0]
    suff = p._suff
    assert suff.requires_grad and suff.dtype == torch.float32 and tuple(suff.shape) == (n_z * Bn, T, 4)
    suff.retain_grad()
    mm = p.mismatch(Y, weights=w, freqs=f, taus=taus, of=of)
    assert mm.shape == ((n_z, Bn) if of == "samples" else (1, Bn)) and p._base is None
    with torch.no_grad():
        assert torch.equal(mm, p.match(Y, weights=w, freqs=f, taus=taus, of=of).mismatch), name
        h = suff.detach() if of == "samples" else p.summary().mean
    mm.sum().backward()
    got = suff.grad.cpu()
    assert torch.isfinite(got).all() and (got[..., 2:] == 0).all(), name  # (the scale entries get zero)
    obs = dict(h=h.cpu(), g=Y.cpu(), weights=w.cpu(), freqs=f.cpu(), taus=taus, n_valid=None if n_trgt is None else n_trgt.cpu())
    ref = R.reference(**obs)
    _clear_maximum(ref, name)
    rows = h.shape[0]
    want, s, _ = G.expected(obs, -torch.ones(rows), n_bcast=n_z if of == "mean" else 1, ref=ref)  # (d mismatch = -d match)
    assert float(want.abs().max()) > 0
    blocks = got.view(-1, rows, T, 4)
    for q in range(blocks.shape[0]):
        r = G.gate_ratio(blocks[q][..., :2], want, s)
        print(f"MISMATCH {name} of={of} block {q}: error / gate {r:.3g}")
        assert r <= 1.0, (name, of, q, r)
        assert torch.equal(blocks[q], blocks[0]) or of == "samples", (name, q)
    if n_trgt is not None:
        beyond = (torch.arange(T).view(1, T) >= n_trgt.cpu().view(-1, 1)).repeat(n_z, 1)
        assert (got[beyond] == 0).all(), name


@pytest.mark.parametrize("name,latent", [("attncnp_r128_c128", False), ("attnlnp_r256_c200_nz8", True)])
def test_parameter_gradients_of_the_sum_are_the_sum_of_the_parameter_gradients(name, latent):
    """``MismatchLoss(base, lam)`` against its two parts run on their own: per parameter tensor max|d| <= 1e-5 max|ref|, the
    project's fp32 gate."""
    import npf_gwwaveform_amd as A

    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T = case["B"], case["T"]
    Y, w, f, taus = _observation(case, 41)
    n_trgt = _counts(Bn, T, 6, T // 2) if latent else None
    base = A.NLLLossLNPF() if latent else A.CNPFLoss()
    lam = 10.0
    losses = dict(both=A.MismatchLoss(base=base, lam=lam, weights=w, freqs=f, taus=taus),
                  base=base, mismatch=A.MismatchLoss(lam=lam, weights=w, freqs=f, taus=taus))
    values, grads = {}, {}
    for key, crit in losses.items():
        crit.to(DEV).train()
        model.zero_grad(set_to_none=True)
        loss = crit(_forward(model, Xc, Yc, Xt, n_trgt), Y)
        loss.backward()
        values[key] = float(loss.detach())
        grads[key] = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    np.testing.assert_allclose(values["both"], values["base"] + values["mismatch"], rtol=1e-6)
    assert values["mismatch"] > 0 and any(float(g.abs().max()) > 0 for g in grads["mismatch"].values())
    for k in grads["both"]:
        assert_close(grads["both"][k], grads["base"][k] + grads["mismatch"][k], tol=1e-5, what=f"{name} {k}")


def test_bf16_compute_mode_hands_the_head_an_fp32_raw_output():
    """The bf16 compute mode keeps the raw decoder output fp32 (the head reads the same tensor), so the objective works there
    unchanged: the gradient arriving at it meets the same gate."""
    import npf_gwwaveform_amd as A

    case = ROUTES["attncnp_r128_c128"]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Y, w, f, taus = _observation(case, 41)
    A.set_compute_dtype("bf16")
    try:
        p = model(Xc, Yc, Xt)[0]
        suff = p._suff
        assert suff.dtype == torch.float32
        suff.retain_grad()
        p.mismatch(Y, weights=w, freqs=f, taus=taus).sum().backward()
        assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    finally:
        A.set_compute_dtype("fp32")
    obs = dict(h=suff.detach().cpu(), g=Y.cpu(), weights=w.cpu(), freqs=f.cpu(), taus=taus, n_valid=None)
    ref = R.reference(**obs)
    _clear_maximum(ref, "bf16")
    want, s, _ = G.expected(obs, -torch.ones(suff.shape[0]), ref=ref)
    r = G.gate_ratio(suff.grad.cpu()[..., :2], want, s)
    print(f"MISMATCH bf16 compute mode: error / gate {r:.3g}")
    assert r <= 1.0 and (suff.grad[..., 2:] == 0).all()


# ---- the Trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_captures_the_mismatch_loss_and_the_mismatch_falls():
    """``Trainer`` with ``MismatchLoss(base=CNPFLoss(), lam=10, freqs, taus=grid(17))`` on the smallest AttnCNP (r = 64, two-layer
    encoder and decoder) and one fixed synthetic batch: the graph-replayed steps give the losses and parameters of eagerly launched
    steps from the same start (the tolerance of test_hip_models.test_graph_captured_step_equals_eager_step: the same kernels in
    the same order), the step is captured once -- the three eager warm-up steps allocate the match workspace, a capture that had
    to grow it would raise -- and after 20 steps the mean mismatch lies below that of step 0.  The start is the one
    tests/test_mismatch_host.py shows on the CPU oracle to be led by the mismatch and not by the likelihood's transient (0.417 ->
    0.048 there); from ``torch.manual_seed(3)`` default initialisation, a start of the other kind, the same run went 0.178 -> 0.251
    with the likelihood falling 160 -> 129, on the oracle's seed 5 likewise."""
    import npf_gwwaveform_amd as A
    import specs
    from helpers import build_model
    from npf_gwwaveform_amd.train import Trainer

    batch, freqs, taus = G.train_setup()
    batch, freqs = {k: v.to(DEV) for k, v in batch.items()}, freqs.to(DEV)

    def mean_mismatch(model):
        with torch.no_grad():
            p = model(batch["X_cntxt"], batch["Y_cntxt"], batch["X_trgt"])[0]
            return float(p.match(batch["Y_trgt"], freqs=freqs, taus=taus).mismatch.mean())

    def run(use_graph):
        model = build_model(G.TRAIN_CASE, DEV, params=specs.make_params(G.TRAIN_CASE, seed=G.TRAIN_SEED))
        crit = A.MismatchLoss(base=A.CNPFLoss(), lam=G.TRAIN_LAM, freqs=freqs.clone(), taus=taus).to(DEV)
        tr = Trainer(model, crit, lr=G.TRAIN_LR, world=1, use_graph=use_graph)
        before = mean_mismatch(model)
        losses = [float(tr.step(batch)) for _ in range(G.TRAIN_STEPS)]
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, tr, before, mean_mismatch(model)

    l_e, p_e, _, b_e, a_e = run(False)
    l_g, p_g, tr, b_g, a_g = run(True)
    print(f"MISMATCH trainer: mean mismatch {b_g:.6f} -> {a_g:.6f} after 20 steps; loss {l_g[0]:.4f} -> {l_g[-1]:.4f}")
    assert tr._graph is not None and tr.n_captures == 1
    assert b_g == b_e and all(np.isfinite(l_g))
    np.testing.assert_allclose(l_g, l_e, rtol=1e-6)
    for k in p_e:
        assert torch.allclose(p_g[k], p_e[k], rtol=1e-6, atol=1e-8), k
    assert a_g < b_g and a_e < b_e
