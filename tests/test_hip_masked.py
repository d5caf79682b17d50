"""Padded contexts with per-task counts on the GPU (csrc/masked_kernels.hip; ``forward(..., n_cntxt=...)``).

The reference for a padded batch is the reference run once per task on the context cut to that task's count: for the kernels a
float64 softmax / mean restricted to the valid rows, for whole models the CPU oracle with ``B = 1`` per task (``reduction=None``),
the losses averaged and the gradients accumulated on one parameter dict.  Gates are the project's fp32 gates: outputs 1e-5 of
max|ref|, the loss to rtol 2e-5, gradients 1e-4 of max|ref| with the zero-reference rule of tests/test_hip_dispatch.py; the kernel
tests use the gate of tests/test_hip_mha.py including its allowance for ill-conditioned cases (``assert_gated``)."""
import copy
import math

import numpy as np
import pytest
import torch

import specs
from helpers import EpsIndependent, assert_close, build_loss, build_model, launch_witness
from oracle import npf_oracle as O
from test_hip_dispatch import _compare_grads, _compare_outputs
from test_hip_mha import assert_gated
from test_hip_sweep import LOSSES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASKED = ("npf_masked_attn_fwd", "npf_masked_attn_bwd", "npf_masked_mean_fwd", "npf_masked_mean_bwd")


# ---- 1. kernels against float64 -----------------------------------------------------------------------------------------
def _counts(B, C_pad, seed):
    """Per-task counts that include 0, 1, a block boundary (32 / 33 / 16) and C_pad, the rest random."""
    must = [0, 1, C_pad, min(32, C_pad), min(33, C_pad), min(16, C_pad), max(C_pad - 1, 0)]
    rng = np.random.Generator(np.random.Philox(seed))
    extra = rng.integers(0, C_pad + 1, size=max(B - len(must), 0)).tolist()
    return (must + extra)[:B]


def _attention_and_grads(Q, K, V, dO, counts, scale, dtype):
    """(O, dQ, dK, dV) of softmax over the first counts[b] keys, in the form the kernels evaluate (log-sum-exp, P = exp(S - lse),
    D = rowsum(dO O), dS = P (dO V^T - D)), per task; zeros for an empty task and in the rows beyond the count."""
    outs = [torch.zeros_like(x, dtype=dtype) for x in (Q, Q, K, V)]
    for b, n in enumerate(counts):
        if n == 0:
            continue
        q, k, v, g = (x[b].to(dtype) for x in (Q, K[:, :n], V[:, :n], dO))
        S = q @ k.T * scale
        P = torch.exp(S - torch.logsumexp(S, dim=-1, keepdim=True))
        o = P @ v
        D = (g * o).sum(-1, keepdim=True)
        dS = P * (g @ v.T - D) * scale
        outs[0][b], outs[1][b], outs[2][b, :n], outs[3][b, :n] = o, dS @ k, dS.T @ q, P.T @ g
    return outs


@pytest.mark.parametrize("T", (1, 70))
@pytest.mark.parametrize("C_pad", (1, 31, 32, 33, 256, 257, 700))
@pytest.mark.parametrize("d", (16, 32, 64, 128, 256))
def test_masked_attention_matches_float64(d, C_pad, T):
    from npf_gwwaveform_amd import functional as FN

    B = 8
    counts = _counts(B, C_pad, seed=d + C_pad + T)
    g = torch.Generator().manual_seed(1000 * d + C_pad + T)
    Q, K, V = (torch.randn(B, n, d, generator=g) * a for n, a in ((T, 1.5), (C_pad, 1.5), (C_pad, 1.0)))  # (as tests/test_hip_mha.py)
    w = torch.randn(B, T, d, generator=g)
    scale = 1.0 / math.sqrt(d)
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    Qd, Kd, Vd = (x.to(DEV).requires_grad_(True) for x in (Q, K, V))
    out = FN.unpack_pt(FN.masked_attention(FN.pack_pt(Qd), FN.pack_pt(Kd), FN.pack_pt(Vd), n_valid, B, C_pad, T, d, scale), T, d)
    (out * w.to(DEV)).sum().backward()
    r64 = _attention_and_grads(Q, K, V, w, counts, scale, torch.float64)
    r32 = _attention_and_grads(Q, K, V, w, counts, scale, torch.float32)
    for i, (name, got, tol) in enumerate((("output", out, 1e-5), ("dQ", Qd.grad, 1e-4), ("dK", Kd.grad, 1e-4), ("dV", Vd.grad, 1e-4))):
        err = float((got.detach().cpu().double() - r64[i]).abs().max())
        print(f"d={d} C_pad={C_pad} T={T} {name}: max|d|={err:.3e} max|ref|={float(r64[i].abs().max()):.3e}")
        assert_gated(got, r64[i], r32[i], tol, f"{name} d={d} C_pad={C_pad} T={T}")
    for b, n in enumerate(counts):
        assert (Kd.grad[b, n:] == 0).all() and (Vd.grad[b, n:] == 0).all(), f"task {b}: d_k / d_v beyond the count {n}"
        if n == 0:
            assert (out[b] == 0).all() and (Qd.grad[b] == 0).all(), f"task {b}: empty context"


@pytest.mark.parametrize("F", (32, 128, 256))
@pytest.mark.parametrize("C_pad", (1, 31, 32, 33, 256, 257, 700))
def test_masked_mean_matches_float64(C_pad, F):
    from npf_gwwaveform_amd import functional as FN

    B = 8
    counts = _counts(B, C_pad, seed=F + C_pad)
    g = torch.Generator().manual_seed(F + C_pad)
    R, w = torch.randn(B, C_pad, F, generator=g), torch.randn(B, F, generator=g)
    Rd = R.to(DEV).requires_grad_(True)
    out = FN.masked_mean(FN.pack_pt(Rd), torch.tensor(counts, device=DEV), B, C_pad, F)[:, :F]
    (out * w.to(DEV)).sum().backward()
    ref, dref = torch.zeros(B, F, dtype=torch.float64), torch.zeros(B, C_pad, F, dtype=torch.float64)
    for b, n in enumerate(counts):
        if n:
            ref[b] = R[b, :n].double().mean(0)
            dref[b, :n] = w[b].double() / n
    assert_close(out, ref, tol=1e-5, what="masked mean")
    assert_close(Rd.grad, dref, tol=1e-4, what="masked mean backward")
    for b, n in enumerate(counts):
        assert (Rd.grad[b, n:] == 0).all(), f"task {b}: gradient beyond the count {n}"
        if n == 0:
            assert (out[b] == 0).all()


@pytest.mark.parametrize("pts", (1, 31, 32, 33, 70))
@pytest.mark.parametrize("F", (32, 96))
def test_masked_mean_at_full_counts_is_the_unmasked_mean_bit_for_bit(F, pts):
    """Counts at and above ``pts`` (clamped) against ``npf_mean_agg_fwd`` / ``_bwd``: the same thread mapping and summation order.
    The sizes sit either side of the tile boundary (32 points) with a partly filled last tile; F = 96 gives three feature blocks."""
    from npf_gwwaveform_amd import functional as FN

    B = 3
    g = torch.Generator().manual_seed(100 * F + pts)
    R, w = torch.randn(B, pts, F, generator=g).to(DEV), torch.randn(B, F, generator=g).to(DEV)
    n_valid = torch.tensor([pts, pts + 5, 10 ** 6], device=DEV)
    outs = []
    for mean in (lambda pt: FN.mean_agg(pt, pts, F), lambda pt: FN.masked_mean(pt, n_valid, B, pts, F)):
        pt = FN.pack_pt(R).detach().requires_grad_(True)
        with launch_witness() as wit:
            out = mean(pt)
            out.backward(w)
            torch.cuda.synchronize()
        outs.append((out.detach(), pt.grad, wit))
    (o0, g0, w0), (o1, g1, w1) = outs
    assert w0["npf_mean_agg_fwd"] == 1 and w0["npf_mean_agg_bwd"] == 1 and w0["npf_masked_mean_fwd"] == 0, w0
    assert w1["npf_masked_mean_fwd"] == 1 and w1["npf_masked_mean_bwd"] == 1 and w1["npf_mean_agg_fwd"] == 0, w1
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    assert float(o0.abs().max()) > 0 and float(g0.abs().max()) > 0  # (not two tensors of zeros)


def test_masked_exports_refuse_bad_sizes():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import chain as CH

    x = CH.pt_empty(1, 32, 288, DEV)
    n = torch.ones(1, dtype=torch.int32, device=DEV)
    lib, p, ip = L.load(), L.ptr(x), n.data_ptr()
    assert lib.npf_masked_attn_fwd(p, p, p, ip, 1, 32, 32, 30, 1.0, p, None, None) == -1   # width not a multiple of 4
    assert lib.npf_masked_attn_fwd(p, p, p, ip, 1, 32, 32, 260, 1.0, p, None, None) == -1  # width above 256
    assert lib.npf_masked_attn_fwd(p, p, p, ip, 1, -1, 32, 32, 1.0, p, None, None) == -1   # negative count of keys
    assert lib.npf_masked_attn_bwd(p, p, p, ip, p, p, p, 1, 32, -1, 32, 1.0, p, p, p, None) == -1
    assert lib.npf_masked_mean_fwd(p, ip, 1, -1, 32, p, None) == -1
    assert lib.npf_masked_mean_bwd(p, ip, 1, 32, 30, p, 0, None) == -1
    assert lib.npf_version() == 2


def test_counts_outside_the_range_are_clamped():
    """Counts below 0 / above n_keys behave as 0 / n_keys (the kernel clamps; nothing is read out of bounds)."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(0)
    Q, K, V = (torch.randn(2, n, 64, generator=g).to(DEV) for n in (40, 50, 50))
    run = lambda c: FN.masked_attention(FN.pack_pt(Q), FN.pack_pt(K), FN.pack_pt(V), torch.tensor(c, device=DEV), 2, 50, 40, 64, 0.125)  # noqa: E731
    assert torch.equal(run([-3, 10 ** 6]), run([0, 50]))


# ---- 2. padding is inert ---------------------------------------------------------------------------------------------------
def _case(kind, r, C_pad, **kw):
    return dict(dict(kind=kind, r=r, C=C_pad, B=5, dx=1, dy=2, L_xy=2, L_dec=2, T=70), **kw)


def _counts_of(C_pad):
    return [0, 1, 33, C_pad - 1, C_pad]


def _masked_step(case, params, inp, counts, train=True):
    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    if "eps" in dinp:
        EpsIndependent.eps = dinp["eps"]
    n = torch.tensor(counts, device=DEV)
    crit = build_loss(case)
    model.train(train)
    crit.train(train)
    with launch_witness(spy=("x6.target_side",)) as w:
        if not train:
            with torch.no_grad():
                out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], n_cntxt=n)
            torch.cuda.synchronize()
            return model, out, None, w
        out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"], n_cntxt=n)
        loss = crit(out, dinp["Y_trgt"])
        loss.backward()
        torch.cuda.synchronize()
    return model, out, loss, w


@pytest.mark.parametrize("kind,kw", [("AttnCNP", {}), ("CNP", {}), ("AttnLNP", dict(is_q_zCct=True, n_z=2)),
                                     ("AttnCNP", dict(attention="transformer"))])
def test_padding_rows_are_inert(kind, kw):
    """The same batch with the padding rows refilled by other finite values in [-1, 1]: bit-identical outputs and gradients."""
    case = _case(kind, 128, 40, **kw)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    counts = _counts_of(40)
    inp["Y_cntxt"] = inp["Y_cntxt"].clamp(-1, 1)
    other = copy.deepcopy(inp)
    g = torch.Generator().manual_seed(9)
    for b, n in enumerate(counts):
        for k in ("X_cntxt", "Y_cntxt"):
            other[k][b, n:] = torch.rand(other[k][b, n:].shape, generator=g) * 2 - 1
    m1, o1, l1, _ = _masked_step(case, params, inp, counts)
    m2, o2, l2, _ = _masked_step(case, params, other, counts)
    assert torch.equal(o1[0].base_dist.loc, o2[0].base_dist.loc) and torch.equal(o1[0].base_dist.scale, o2[0].base_dist.scale)
    assert torch.equal(l1, l2)
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), k
        if p1.grad is not None:
            assert torch.equal(p1.grad, p2.grad), k


# ---- 3. whole models against the per-task oracle ---------------------------------------------------------------------------
def _per_task_oracle(case, inp, params, counts, training=True):
    """The oracle once per task on the context cut to its count; losses averaged, gradients accumulated on one dict."""
    cfg = specs.cfg_of(case)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    B, n_z = case["B"], case.get("n_z", 1)
    outs, total = [], 0.0
    for b, n in enumerate(counts):
        eps = inp["eps"][:, b:b + 1] if "eps" in inp else None
        Yt = inp["Y_trgt"][b:b + 1] if training else None
        out = O.forward(cfg, p, inp["X_cntxt"][b:b + 1, :n], inp["Y_cntxt"][b:b + 1, :n], inp["X_trgt"][b:b + 1], Yt, eps=eps,
                        n_z=n_z, training=training)
        if training:
            loss = LOSSES[specs.loss_name(case)](out, Yt, reduction=None).sum() / B
            loss.backward()
            total += float(loss.detach().double())
        outs.append(out)
    cat = lambda xs, dim: torch.cat([x.detach() for x in xs], dim=dim)  # noqa: E731
    ref = dict(loc=cat([o["loc"] for o in outs], 1), scale=cat([o["scale"] for o in outs], 1), z_samples=None, q_zCc=None, q_zCct=None)
    if outs[0]["z_samples"] is not None:
        ref["z_samples"] = cat([o["z_samples"] for o in outs], 1)
        for key in ("q_zCc", "q_zCct"):
            if outs[0][key] is not None:
                ref[key] = tuple(cat([o[key][i] for o in outs], 0) for i in range(2))
    return p, ref, total


RELU_TIE = 2e-7  # (the tie threshold of tests/test_hip_stress.py for fp32)


def _reference_margin(case, inp, params, counts):
    """The smallest |ReLU pre-activation| of the per-task oracle's train-mode forward (``O.RELU_MARGINS``)."""
    O.RELU_MARGINS = []
    try:
        with torch.no_grad():
            for b, n in enumerate(counts):
                eps = inp["eps"][:, b:b + 1] if "eps" in inp else None
                O.forward(specs.cfg_of(case), params, inp["X_cntxt"][b:b + 1, :n], inp["Y_cntxt"][b:b + 1, :n], inp["X_trgt"][b:b + 1],
                          inp["Y_trgt"][b:b + 1], eps=eps, n_z=case.get("n_z", 1), training=True)
        return min(O.RELU_MARGINS)
    finally:
        O.RELU_MARGINS = None


def _well_posed_inputs(case, params, counts, first_seed=4321, tries=20000):
    """Inputs whose reference gradient is defined in fp32: the first seed from ``first_seed`` on for which no ReLU pre-activation of
    the oracle lies within ``RELU_TIE`` of zero.  A pre-activation closer to zero than fp32 rounding of its own sum has a sign --
    and with it a derivative -- that rounding noise decides, so two correct fp32 evaluations differ by that unit's whole gradient
    contribution (the project's randomised sweep sets such cases aside at the same threshold; seed 4321 itself has pre-activations
    down to 1e-8 in several of these cases, and there the existing unmasked model, run one task at a time, differs from the
    oracle by up to 4e-3 on single gradient tensors).  The choice reads the reference alone, never the code under test."""
    for seed in range(first_seed, first_seed + tries):
        inp = specs.make_inputs(case, seed=seed)
        if _reference_margin(case, inp, params, counts) >= RELU_TIE:
            return inp, seed
    raise AssertionError(f"no well-posed inputs in {tries} seeds")


MODEL_CASES = {
    "cnp_r256": dict(kind="CNP", r=256),
    "lnp_latent_nz4": dict(kind="LNP", r=128, encoded_path="latent", is_q_zCct=True, n_z=4),
    "attncnp_scaledot_r128": dict(kind="AttnCNP", r=128),
    "attncnp_scaledot_r256": dict(kind="AttnCNP", r=256),
    "attncnp_multihead_r128": dict(kind="AttnCNP", r=128, attention="multihead"),
    "attncnp_transformer_r128": dict(kind="AttnCNP", r=128, attention="transformer"),
    "attnlnp_scaledot_r256_nz1": dict(kind="AttnLNP", r=256, is_q_zCct=True, n_z=1),
    "attnlnp_scaledot_r256_nz8": dict(kind="AttnLNP", r=256, is_q_zCct=True, n_z=8),
}


@pytest.mark.parametrize("C_pad", (40, 200, 300))
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_padded_models_match_the_per_task_oracle(name, C_pad):
    """Train step (outputs, loss, every gradient) and evaluation forward against the oracle run once per task on the cut context,
    on inputs whose reference gradient is well defined (``_well_posed_inputs``)."""
    kw = dict(MODEL_CASES[name])
    case = _case(kw.pop("kind"), kw.pop("r"), C_pad, **kw)
    params, counts = specs.make_params(case, seed=11), _counts_of(C_pad)
    inp, seed = _well_posed_inputs(case, params, counts)
    for b, n in enumerate(counts):  # (zeros are the documented padding)
        inp["X_cntxt"][b, n:] = 0
        inp["Y_cntxt"][b, n:] = 0
    ref_p, ref_out, ref_loss = _per_task_oracle(case, inp, params, counts)
    model, out, loss, w = _masked_step(case, params, inp, counts)
    print(f"{name} C_pad={C_pad}: input seed {seed}, loss {loss.item():.8g} ref {ref_loss:.8g}")
    _compare_outputs(out, ref_out)
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=2e-5)
    _compare_grads(model, ref_p)
    # 5. the path: the masked kernels run, the fused target side does not
    attentive = case["kind"].startswith("Attn")
    assert w["x6.target_side"] == 0, w
    if attentive:
        assert w["npf_masked_attn_fwd"] == 1 and w["npf_masked_attn_bwd"] == 1, w
    else:
        assert w["npf_masked_attn_fwd"] == 0, w
    n_mean = int(case["kind"] in ("CNP", "LNP", "AttnLNP"))
    assert w["npf_masked_mean_fwd"] == n_mean and w["npf_masked_mean_bwd"] == n_mean, w
    # evaluation-mode forward without targets
    _, out_e, _, _ = _masked_step(case, params, inp, counts, train=False)
    _, ref_e, _ = _per_task_oracle(case, inp, params, counts, training=False)
    _compare_outputs(out_e, ref_e, what="(eval)")


# ---- 4. equal counts reproduce the unmasked model; 5. without n_cntxt none of the new exports runs -----------------------
@pytest.mark.parametrize("name", ["cnp_r256", "attncnp_scaledot_r128", "attncnp_scaledot_r256", "attncnp_transformer_r128",
                                  "attnlnp_scaledot_r256_nz1"])
def test_full_counts_reproduce_the_unmasked_model(name):
    kw = dict(MODEL_CASES[name])
    case = _case(kw.pop("kind"), kw.pop("r"), 200, **kw)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    m1, o1, l1, w1 = _masked_step(case, params, inp, [200] * 5)
    m0 = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    crit = build_loss(case)
    m0.train()
    crit.train()
    with launch_witness() as w0:
        o0 = m0(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
        l0 = crit(o0, dinp["Y_trgt"])
        l0.backward()
        torch.cuda.synchronize()
    assert all(w0[k] == 0 for k in MASKED), w0
    assert sum(w1[k] for k in MASKED) > 0, w1
    assert_close(o1[0].base_dist.loc, o0[0].base_dist.loc.detach().cpu(), what="loc")
    assert_close(o1[0].base_dist.scale, o0[0].base_dist.scale.detach().cpu(), what="scale")
    np.testing.assert_allclose(l1.item(), l0.item(), rtol=2e-5)
    _compare_grads(m1, {k: p for k, p in m0.named_parameters()})


def test_zero_padded_rows_behave_like_no_context():
    case = _case("AttnCNP", 128, 0)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    _, o1, l1, w = _masked_step(case, params, inp, [0] * 5)
    assert all(w[k] == 0 for k in MASKED), w
    m0 = build_model(case, DEV, params=params)
    o0 = m0(*(inp[k].to(DEV) for k in ("X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt")))
    assert torch.equal(o1[0].base_dist.loc, o0[0].base_dist.loc)


# ---- 6. one graph, many sizes ----------------------------------------------------------------------------------------------
def test_one_captured_graph_serves_every_context_size():
    """Trainer(use_graph=True) on AttnCNP r = 128, C_pad = 64, 12 Adam steps whose counts change every step, against an eager
    Trainer on a copy of the model fed the same batches: same losses and final parameters (the gates of
    tests/test_hip_models.py::test_graph_captured_step_equals_eager_step), and the step is captured exactly once."""
    import warnings

    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer, synthetic_waveform_batch

    B, C_pad, T = 8, 64, 50

    def batch(i):
        b = synthetic_waveform_batch(B, C_pad, T, 500 + i, DEV)
        n = torch.randint(0, C_pad + 1, (B,), generator=torch.Generator().manual_seed(i)).to(DEV)
        pad = (torch.arange(C_pad, device=DEV).unsqueeze(0) >= n.unsqueeze(1)).unsqueeze(-1)
        b["X_cntxt"], b["Y_cntxt"] = b["X_cntxt"].masked_fill(pad, 0.0), b["Y_cntxt"].masked_fill(pad, 0.0)
        b["n_cntxt"] = n
        return b

    def run(use_graph):
        torch.manual_seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = A.AttnCNP(1, 2, r_dim=128).to(DEV)
        tr = Trainer(model, A.CNPFLoss(), lr=1e-3, world=1, use_graph=use_graph)
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
    np.testing.assert_allclose(l_g, l_e, rtol=1e-6)
    for k in p_e:
        assert torch.allclose(p_g[k], p_e[k], rtol=1e-6, atol=1e-8), k
