"""Training through context weights on the GPU: ``functional.key_weighted_attention`` / ``key_weighted_mean`` (the kernels behind
``npf_masked_attn_fwd_weighted_ex`` / ``npf_masked_attn_bwd_weighted`` / ``npf_weighted_mean_bwd``) against the float64 closed forms
of tests/keyweight_reference.py, and ``forward(w_cntxt=...)`` / ``influence`` / the Trainer on whole models.

Gates.  Kernels: the expression of tests/test_hip_masked.py (``assert_gated`` of tests/test_hip_mha.py): max|got - ref64| <=
max(tol * max|ref64|, 4 * max|the same formula in fp32 torch - ref64|) with tol = 1e-5 for the output and 1e-4 for dQ, dK, dV and dW;
the weighted mean and its two gradients at 1e-6 of max|ref64| (double arithmetic with one rounding, as ``weighted_mean`` forward).
Models: loc and scale 1e-5, the loss rtol 2e-5, parameter gradients 1e-4 with the zero-reference rule of tests/test_hip_dispatch.py.
Every case prints ``KW <regime> <tensor> err/gate`` so that the worst ratio per regime can be collected from a run's output.

NaN / Inf in the rows and weights of inadmissible keys, and NaN in the Q / dO rows of queries at and beyond the query count, are
data here: the kernels must never let the former meet a multiply and never read the latter."""
import math
import warnings

import numpy as np
import pytest
import torch

import keyweight_reference as KR
import specs
from helpers import assert_close, build_loss, build_model, launch_witness
from oracle import npf_oracle as O
from test_hip_dispatch import _compare_grads
from test_hip_mha import assert_gated
from test_hip_sweep import LOSSES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 4
PATTERNS = ("ones", "integers", "loguniform", "zero_block", "zero_on_top_key", "bad_weights_nan_rows")


def _counts(C_pad):
    return [C_pad, (C_pad + 1) // 2, 1, 0]


def _weights(pattern, Q, K, counts, d, g):
    """(W [B, C_pad], K, V poison mask [B, C_pad] of the rows to fill with NaN)"""
    C = K.shape[1]
    poison = torch.zeros(B, C, dtype=torch.bool)
    if pattern == "ones":
        W = torch.ones(B, C)
    elif pattern == "integers":
        W = torch.randint(0, 4, (B, C), generator=g).float()
    elif pattern == "loguniform":
        W = torch.exp((torch.rand(B, C, generator=g) * 2 - 1) * math.log(1e3))
    elif pattern == "zero_block":  # the first staged key block (32 keys, 16 at the 256-wide instance) without weight
        W = torch.exp(torch.rand(B, C, generator=g) * 2 - 1)
        W[:, :16 if d > 128 else 32] = 0
    elif pattern == "zero_on_top_key":  # the key with the highest score of any query, per task, has weight 0
        W = torch.exp(torch.rand(B, C, generator=g) * 2 - 1)
        top = torch.einsum("bqd,bkd->bqk", Q, K).amax(1).argmax(-1)
        W[torch.arange(B), top] = 0
    else:  # negative, NaN and Inf weights on a third of the keys, NaN in their K / V rows and in all padding (weights too)
        W = torch.exp(torch.rand(B, C, generator=g) * 2 - 1)
        bad = torch.rand(B, C, generator=g) < 1 / 3
        vals = torch.tensor([-1.0, math.nan, math.inf, -math.inf]).repeat(B * C)[: B * C].view(B, C)
        W = torch.where(bad, vals, W)
        poison = bad.clone()
        for b, n in enumerate(counts):
            poison[b, n:] = True
            W[b, n:] = math.nan
    return W, poison


def _report(regime, name, got, r64, r32, tol):
    got, ref, r32 = (t.detach().cpu().double() for t in (got, r64, r32))
    err, gate = float((got - ref).abs().max()), max(tol * float(ref.abs().max()), 4 * float((r32 - ref).abs().max()))
    print(f"KW {regime} {name} err/gate={err / gate if gate > 0 else 0.0:.3f} err={err:.3e} gate={gate:.3e}")


SHAPES = [(d, C, T) for d in (16, 64, 128, 256) for C in (1, 31, 32, 33, 70) for T in (1, 64, 65, 130)]
SHAPES += [(256, C, T) for C in (15, 16, 17) for T in (1, 64, 65, 130)]


@pytest.mark.parametrize("d,C_pad,T", SHAPES)
def test_key_weighted_attention_matches_float64(d, C_pad, T):
    from npf_gwwaveform_amd import functional as FN

    counts = _counts(C_pad)
    scale = 1.0 / math.sqrt(d)
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    for pi, pattern in enumerate(PATTERNS):
        g = torch.Generator().manual_seed(100000 * pi + 1000 * d + 10 * C_pad + T)
        Q, K, V = (torch.randn(B, n, d, generator=g) * a for n, a in ((T, 1.5), (C_pad, 1.5), (C_pad, 1.0)))
        dO = torch.randn(B, T, d, generator=g)
        W, poison = _weights(pattern, Q, K, counts, d, g)
        Kp, Vp = K.clone(), V.clone()
        Kp[poison], Vp[poison] = math.nan, math.nan
        for q_counts in (None, (T, 1, 0, 65)):
            regime = f"{pattern}{'' if q_counts is None else '+nq'}"
            r64 = KR.weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, torch.float64, q_counts)
            r32 = KR.weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, torch.float32, q_counts)
            Qp, dOp = Q.clone(), dO.clone()
            if q_counts is not None:  # (queries at and beyond the count are never read: NaN in their Q and dO rows)
                for b_, n_q in enumerate(q_counts):
                    Qp[b_, n_q:], dOp[b_, n_q:] = math.nan, math.nan
            Qd, Kd, Vd, Wd = (x.to(DEV).requires_grad_(True) for x in (Qp, Kp, Vp, W))
            nq = None if q_counts is None else torch.tensor(q_counts, dtype=torch.int32, device=DEV)
            with launch_witness() as wit:
                out = FN.unpack_pt(FN.key_weighted_attention(FN.pack_pt(Qd), FN.pack_pt(Kd), FN.pack_pt(Vd), Wd, n_valid, B, C_pad, T, d,
                                                             scale, n_q_valid=nq), T, d)
                out.backward(dOp.to(DEV))
                torch.cuda.synchronize()
            assert wit["npf_masked_attn_fwd_weighted_ex"] == 1 and wit["npf_masked_attn_bwd_weighted"] == 1, wit
            assert wit["npf_masked_attn_fwd_weighted"] == 0 and wit["npf_masked_attn_bwd"] == 0, wit
            tag = f"{regime} d={d} C_pad={C_pad} T={T}"
            for i, (name, got, tol) in enumerate((("output", out, 1e-5), ("dQ", Qd.grad, 1e-4), ("dK", Kd.grad, 1e-4),
                                                  ("dV", Vd.grad, 1e-4), ("dW", Wd.grad, 1e-4))):
                assert torch.isfinite(got).all(), f"{name} {tag}: NaN / Inf"
                _report(regime, name, got, r64[i], r32[i], tol)
                assert_gated(got, r64[i], r32[i], tol, f"{name} {tag}")
            adm = KR.admissible(W, counts).to(DEV)
            assert (Kd.grad[~adm] == 0).all() and (Vd.grad[~adm] == 0).all() and (Wd.grad[~adm] == 0).all(), f"{tag}: inadmissible keys"
            for b in range(B):
                n_q = T if q_counts is None else min(q_counts[b], T)
                assert (out[b, n_q:] == 0).all() and (Qd.grad[b, n_q:] == 0).all(), f"{tag}: task {b}, queries beyond the count"
                if not bool(adm[b].any()):
                    assert (out[b] == 0).all() and (Qd.grad[b] == 0).all(), f"{tag}: task {b} has no admissible key"


@pytest.mark.parametrize("d,C_pad,T", [(64, 33, 65), (256, 17, 130)])
def test_forward_with_lse_keeps_the_bits_and_lse_is_the_log_sum(d, C_pad, T):
    """``O`` of ``npf_masked_attn_fwd_weighted_ex`` is bit-identical to ``npf_masked_attn_fwd_weighted`` (and, with all-ones
    weights, to ``npf_masked_attn_fwd_nq``); ``lse`` matches float64 and is 0 where a query has no key or lies beyond its count."""
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import functional as FN

    counts, q_counts, scale = _counts(C_pad), (T, 1, 0, 65), 1.0 / math.sqrt(d)
    g = torch.Generator().manual_seed(d + C_pad + T)
    Q, K, V = (torch.randn(B, n, d, generator=g) for n in (T, C_pad, C_pad))
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    nq = torch.tensor(q_counts, dtype=torch.int32, device=DEV)
    q, k, v = (FN.pack_pt(x.to(DEV)) for x in (Q, K, V))
    for pattern in ("ones", "integers"):
        W = _weights(pattern, Q, K, counts, d, g)[0]
        Wd = W.to(DEV)
        plain = FN.masked_attention_weighted(q, k, v, Wd, n_valid, B, B, C_pad, T, d, scale, n_q_valid=nq)
        out, lse = torch.full_like(plain, math.nan), torch.full((B, T), math.nan, device=DEV)
        L.check(L.load().npf_masked_attn_fwd_weighted_ex(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(Wd), n_valid.data_ptr(), nq.data_ptr(), B, B,
                                                         C_pad, T, d, scale, L.ptr(out), L.ptr(lse), L.stream_ptr()), "ex")
        assert torch.equal(out, plain), pattern
        if pattern == "ones":
            assert torch.equal(out, FN.masked_attention(q, k, v, n_valid, B, C_pad, T, d, scale, n_q_valid=nq))
        ref = KR.weighted_attention_and_grads(Q, K, V, W, torch.zeros_like(Q), counts, scale, torch.float64, q_counts)[5]
        assert_close(lse, ref, tol=1e-5, what=f"lse {pattern}")
        for b in range(B):
            assert (lse[b, min(q_counts[b], T):] == 0).all()
    assert (lse[3] == 0).all()  # (a task without keys)


@pytest.mark.parametrize("pts", (1, 33, 70))
@pytest.mark.parametrize("F", (4, 128, 256))
def test_key_weighted_mean_matches_float64(F, pts):
    from npf_gwwaveform_amd import functional as FN

    counts = _counts(pts)
    n_valid = torch.tensor(counts, dtype=torch.int32, device=DEV)
    for pi, pattern in enumerate(PATTERNS):
        g = torch.Generator().manual_seed(1000 * pi + 10 * F + pts)
        R, dOut = torch.randn(B, pts, F, generator=g), torch.randn(B, F, generator=g)
        W, poison = _weights(pattern, R[:, :1], R, counts, 64, g)
        Rp = R.clone()
        Rp[poison] = math.nan
        r64 = KR.weighted_mean_and_grads(R, W, dOut, counts, torch.float64)
        Rd, Wd = Rp.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
        with launch_witness() as wit:
            out = FN.key_weighted_mean(FN.pack_pt(Rd), Wd, n_valid, B, pts, F)[:, :F]
            (out * dOut.to(DEV)).sum().backward()
            torch.cuda.synchronize()
        assert wit["npf_weighted_mean"] == 1 and wit["npf_weighted_mean_bwd"] == 1, wit
        plain = FN.weighted_mean(FN.pack_pt(Rp.to(DEV)), W.to(DEV), n_valid, B, B, pts, F)[:, :F]
        assert torch.equal(out.detach(), plain), f"{pattern}: not the bits of weighted_mean"
        for name, got, ref in (("out", out, r64[0]), ("dR", Rd.grad, r64[1]), ("dW", Wd.grad, r64[2])):
            assert torch.isfinite(got).all(), f"{name} {pattern}: NaN / Inf"
            err, m = float((got.detach().cpu().double() - ref).abs().max()), float(ref.abs().max())
            print(f"KW mean:{pattern} {name} err/gate={err / (1e-6 * m) if m > 0 else 0.0:.3f} err={err:.3e} gate={1e-6 * m:.3e}")
            if m > 0:
                assert_close(got, ref, tol=1e-6, what=f"{name} {pattern} F={F} pts={pts}")
            else:
                assert (got == 0).all(), f"{name} {pattern}"
        adm = KR.admissible(W, counts).to(DEV)
        assert (Rd.grad[~adm] == 0).all() and (Wd.grad[~adm] == 0).all(), f"{pattern}: inadmissible points"


def test_new_exports_refuse_bad_sizes():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import chain as CH

    x = CH.pt_empty(1, 32, 288, DEV)
    n = torch.ones(1, dtype=torch.int32, device=DEV)
    lib, p, ip = L.load(), L.ptr(x), n.data_ptr()
    assert lib.npf_masked_attn_fwd_weighted_ex(p, p, p, p, ip, None, 1, 1, 32, 32, 32, 1.0, p, None, None) == -1   # no lse
    assert lib.npf_masked_attn_fwd_weighted_ex(p, p, p, p, ip, None, 1, 1, 32, 32, 30, 1.0, p, p, None) == -1     # width % 4
    assert lib.npf_masked_attn_bwd_weighted(p, p, p, p, ip, None, p, p, p, 1, 32, 32, 260, 1.0, p, p, p, p, None) == -1
    assert lib.npf_masked_attn_bwd_weighted(p, p, p, p, ip, None, p, p, p, 1, 32, 32, 32, 1.0, p, p, p, None, None) == -1  # no d_w
    assert lib.npf_weighted_mean_bwd(p, p, ip, p, p, 1, 32, 30, p, p, None) == -1
    assert lib.npf_weighted_mean_bwd(p, p, ip, p, p, 1, 0, 32, p, p, None) == -1


# ---- whole models -----------------------------------------------------------------------------------------------------------
MODELS = {
    "cnp_r64": dict(kind="CNP", r=64),
    "attncnp_scaledot_r64": dict(kind="AttnCNP", r=64),
    "attncnp_multihead_r128": dict(kind="AttnCNP", r=128, attention="multihead"),
    "attncnp_transformer_r128": dict(kind="AttnCNP", r=128, attention="transformer"),
}
COUNTS, T_COUNTS = [20, 7, 13], [50, 31, 1]
RELU_TIE = 2e-7  # (the tie threshold of tests/test_hip_masked.py)


def _case(name):
    kw = dict(MODELS[name])
    return dict(dict(kind=kw.pop("kind"), r=kw.pop("r"), C=20, B=3, dx=1, dy=2, L_xy=2, L_dec=2, T=50), **kw)


def _step(case, params, inp, train=True, **kw):
    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    crit = build_loss(case)
    model.train(train)
    crit.train(train)
    with launch_witness() as wit:
        out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"], **kw)
        loss = crit(out, dinp["Y_trgt"])
        loss.backward()
        torch.cuda.synchronize()
    return model, out, loss, wit


@pytest.mark.parametrize("name", list(MODELS))
def test_all_ones_weights_give_the_bits_of_the_counted_forward(name):
    case = _case(name)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    n, nt = torch.tensor(COUNTS, device=DEV), torch.tensor(T_COUNTS, device=DEV)
    m0, o0, l0, w0 = _step(case, params, inp, n_cntxt=n, n_trgt=nt)
    w = torch.ones(3, 20, device=DEV, requires_grad=True)
    m1, o1, l1, w1 = _step(case, params, inp, n_cntxt=n, n_trgt=nt, w_cntxt=w)
    attentive = case["kind"] == "AttnCNP"
    if attentive:  # (the weighted attention walks the keys as the counted one does: log 1 = 0 and s + 0 = s exactly)
        assert torch.equal(o1[0].base_dist.loc, o0[0].base_dist.loc) and torch.equal(o1[0].base_dist.scale, o0[0].base_dist.scale)
        assert torch.equal(l1, l0)
    else:  # (CNP: the weighted mean sums in double with one rounding, the counted mean in fp32 -- the project gates, not the bits)
        assert_close(o1[0].base_dist.loc, o0[0].base_dist.loc.detach().cpu(), tol=1e-5, what="loc")
        assert_close(o1[0].base_dist.scale, o0[0].base_dist.scale.detach().cpu(), tol=1e-5, what="scale")
        np.testing.assert_allclose(l1.item(), l0.item(), rtol=2e-5)
    _compare_grads(m1, {k: p for k, p in m0.named_parameters()}, what="(ones against n_cntxt)")
    assert w1["npf_masked_attn_fwd_weighted_ex"] == int(attentive) == w1["npf_masked_attn_bwd_weighted"], w1
    assert w1["npf_weighted_mean_bwd"] == int(not attentive) == w1["npf_weighted_mean"], w1
    assert w1["npf_masked_attn_fwd"] + w1["npf_masked_attn_fwd_nq"] + w1["npf_masked_mean_fwd"] == 0, w1
    assert all(v == 0 for k, v in w0.calls.items() if "weighted" in k), w0
    assert w.grad is not None and torch.isfinite(w.grad).all()
    for b, c in enumerate(COUNTS):
        assert (w.grad[b, c:] == 0).all()
    # n_cntxt=None: every row lies below the count
    full = torch.full((3,), 20, device=DEV)
    _, o2, l2, _ = _step(case, params, inp, n_cntxt=full)
    _, o3, l3, _ = _step(case, params, inp, w_cntxt=torch.ones(3, 20, device=DEV))
    if attentive:
        assert torch.equal(o3[0].base_dist.loc, o2[0].base_dist.loc) and torch.equal(l3, l2)
    else:
        assert_close(o3[0].base_dist.loc, o2[0].base_dist.loc.detach().cpu(), tol=1e-5, what="loc (no counts)")


def _expanded_oracle(case, inp, params, W_int, margins=None):
    """The oracle once per task on the context with row k repeated W_int[b, k] times; losses averaged over the B tasks, gradients
    accumulated on one dict."""
    cfg = specs.cfg_of(case)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    locs, scales, total = [], [], 0.0
    O.RELU_MARGINS = margins
    try:
        for b in range(case["B"]):
            Xc, Yc = (KR.repeat_rows(inp[k][b], W_int[b]).unsqueeze(0) for k in ("X_cntxt", "Y_cntxt"))
            Yt = inp["Y_trgt"][b:b + 1]
            out = O.forward(cfg, p, Xc, Yc, inp["X_trgt"][b:b + 1], Yt, training=True)
            loss = LOSSES[specs.loss_name(case)](out, Yt, reduction=None).sum() / case["B"]
            loss.backward()
            total += float(loss.detach().double())
            locs.append(out["loc"].detach())
            scales.append(out["scale"].detach())
    finally:
        O.RELU_MARGINS = None
    return p, torch.cat(locs, 1), torch.cat(scales, 1), total


@pytest.mark.parametrize("name", list(MODELS))
def test_integer_weights_match_the_oracle_on_the_expanded_context(name):
    """Train step (loc, scale, loss, every parameter gradient) with integer weights 0..3 against the oracle run per task on the
    context with its rows repeated, on inputs whose reference gradient is well defined (no ReLU pre-activation of the oracle
    within ``RELU_TIE`` of zero: the choice reads the reference alone)."""
    case = _case(name)
    params = specs.make_params(case, seed=11)
    W_int = torch.randint(0, 4, (3, 20), generator=torch.Generator().manual_seed(7))
    W_int[0, 0], W_int[1, :2], W_int[2, 5] = 3, 0, 2
    for seed in range(4321, 4321 + 2000):
        inp, margins = specs.make_inputs(case, seed=seed), []
        ref_p, ref_loc, ref_scale, ref_loss = _expanded_oracle(case, inp, params, W_int, margins)
        if min(margins) >= RELU_TIE:
            break
    else:
        raise AssertionError("no well-posed inputs")
    model, out, loss, wit = _step(case, params, inp, w_cntxt=W_int.float().to(DEV))
    print(f"{name}: input seed {seed}, loss {loss.item():.8g} ref {ref_loss:.8g}")
    assert_close(out[0].base_dist.loc, ref_loc, tol=1e-5, what="loc")
    assert_close(out[0].base_dist.scale, ref_scale, tol=1e-5, what="scale")
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=2e-5)
    _compare_grads(model, ref_p)


@pytest.mark.parametrize("name", list(MODELS))
def test_influence_matches_the_float64_gradient(name):
    """``influence`` against float64 autograd through the oracle's stages with the weights in them
    (``KR.oracle_forward_weighted``; multihead / transformer: log w on every head's logits, so the reference sums over the heads)."""
    case = _case(name)
    params, inp = specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321)
    model = build_model(case, DEV, params=params)
    model.train()
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    n, nt = torch.tensor(COUNTS, device=DEV), torch.tensor(T_COUNTS, device=DEV)
    got = model.influence(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"], n_cntxt=n, n_trgt=nt)
    assert model.training and all(p.grad is None for p in model.parameters())
    assert tuple(got.shape) == (3, 20) and not got.requires_grad
    cfg, p64 = specs.cfg_of(case), {k: v.double() for k, v in params.items()}
    ref = torch.zeros(3, 20, dtype=torch.float64)
    for b, (c, t) in enumerate(zip(COUNTS, T_COUNTS)):
        w = torch.ones(1, c, dtype=torch.float64, requires_grad=True)
        loc, scale = KR.oracle_forward_weighted(O, cfg, p64, inp["X_cntxt"][b:b + 1, :c].double(), inp["Y_cntxt"][b:b + 1, :c].double(),
                                                inp["X_trgt"][b:b + 1, :t].double(), w)
        ll = torch.distributions.Normal(loc, scale).log_prob(inp["Y_trgt"][b:b + 1, :t].double()).sum()
        ref[b, :c] = torch.autograd.grad(ll, w)[0][0]
    print(f"{name}: influence max|ref| {float(ref.abs().max()):.4g} max|d| {float((got.cpu().double() - ref).abs().max()):.3e}")
    assert_close(got, ref, tol=1e-4, what="influence")
    for b, c in enumerate(COUNTS):
        assert (got[b, c:] == 0).all()
    model.eval()
    model.influence(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
    assert not model.training


def test_captured_step_sees_weights_overwritten_in_place():
    """Trainer(use_graph=True) on AttnCNP r = 128 with ``batch["w_cntxt"]`` changing every step against an eager Trainer fed the same
    batches: the same losses (rtol 1e-6), one capture."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer, synthetic_waveform_batch

    Bt, C, T = 8, 64, 50

    def batch(i):
        b = synthetic_waveform_batch(Bt, C, T, 500 + i, DEV)
        g = torch.Generator().manual_seed(i)
        b["w_cntxt"] = (torch.exp(torch.rand(Bt, C, generator=g) * 2 - 1) * (torch.rand(Bt, C, generator=g) > 0.2)).to(DEV)
        b["n_cntxt"] = torch.randint(1, C + 1, (Bt,), generator=g).to(DEV)
        return b

    def run(use_graph):
        torch.manual_seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = A.AttnCNP(1, 2, r_dim=128).to(DEV)
        tr = Trainer(model, A.CNPFLoss(), lr=1e-3, world=1, use_graph=use_graph)
        return [float(tr.step(batch(i))) for i in range(8)], tr

    l_e, _ = run(False)
    l_g, tr = run(True)
    assert tr._graph is not None and tr.n_captures == 1
    print("losses eager", l_e, "graph", l_g)
    np.testing.assert_allclose(l_g, l_e, rtol=1e-6)
    assert len(set(l_e)) == len(l_e)


def test_refusals_on_the_device():
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import chain as CH

    x = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    args, w = (x(2, 4, 1), x(2, 4, 2), x(2, 3, 1), x(2, 3, 2)), torch.ones(2, 4, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = dict(r=64, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=4, T=3)
        latent = [build_model(dict(base, kind="LNP", encoded_path="latent"), DEV), build_model(dict(base, kind="AttnLNP"), DEV)]
        selfattn = A.AttnCNP(1, 2, r_dim=32, is_self_attn=True).to(DEV)
        cnp = A.CNP(1, 2, r_dim=32).to(DEV)
    for m in latent:
        with pytest.raises(NotImplementedError, match="w_cntxt.*latent"):
            m(*args, w_cntxt=w)
    with pytest.raises(NotImplementedError, match="w_cntxt.*is_self_attn"):
        selfattn(*args, w_cntxt=w)
    CH.set_compute_dtype("bf16")
    try:
        with pytest.raises(NotImplementedError, match="w_cntxt.*bf16"):
            cnp(*args, w_cntxt=w)
    finally:
        CH.set_compute_dtype("fp32")
