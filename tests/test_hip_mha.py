"""GPU parity test of the fused multihead attention kernel (csrc/mha_kernel.hip, ``npf_mha_fwd`` / ``npf_mha_bwd``) through the C
ABI: per-head scaled-dot attention with 16-feature heads (MultiheadAttender.forward between the projections and the concatenation,
npf/architectures/attention.py:505-527; DotAttender :204-220 per head with the head size in the scale) against a float64
evaluation -- fp32 arithmetic, so the fp32 gates of SURVEY.md 8c: 1e-5 of max|ref| on the output, 1e-4 on gradients.  The model
level (multihead / transformer goldens G8 / G9 / G11, the sweep) runs on this kernel too whenever the heads are 16 wide."""
import math

import pytest
import torch

from test_hip_x6 import DEV, assert_close

pytestmark = pytest.mark.gpu


def _ref(Q, K, V, H):
    B, T, F = Q.shape
    d = F // H
    heads = lambda x: x.view(B, -1, H, d).permute(0, 2, 1, 3)  # noqa: E731
    S = heads(Q) @ heads(K).transpose(-1, -2) / math.sqrt(d)
    return (S.softmax(-1) @ heads(V)).permute(0, 2, 1, 3).reshape(B, T, F)


@pytest.mark.parametrize("B,C,T,H,D", [(3, 128, 256, 8, 16), (2, 37, 70, 2, 16), (2, 200, 33, 8, 16), (1, 256, 100, 4, 16), (2, 5, 1, 1, 16),
                                       (4, 50, 128, 8, 16), (2, 64, 257, 3, 16),
                                       (2, 128, 96, 8, 32), (3, 37, 70, 2, 32), (2, 100, 33, 1, 32), (1, 64, 257, 3, 32),
                                       # the edges of both instances: one key, a ragged last key tile, one query
                                       (2, 1, 70, 8, 32), (2, 31, 33, 8, 32), (3, 33, 1, 8, 32), (2, 127, 96, 4, 32),
                                       (2, 1, 1, 8, 16), (2, 255, 70, 8, 16), (1, 255, 1, 8, 16)])
def test_mha_matches_float64(B, C, T, H, D):
    from npf_gwwaveform_amd import functional as FN

    F = D * H
    assert FN.mha_usable(D, D, C)
    g = torch.Generator().manual_seed(B * 1000 + C + T)
    Q, K, V = (torch.randn(B, n, F, generator=g) * s for n, s in ((T, 1.5), (C, 1.5), (C, 1.0)))
    w = torch.randn(B, T, F, generator=g)
    Qd, Kd, Vd = (x.to(DEV).requires_grad_(True) for x in (Q, K, V))
    out = FN.unpack_pt(FN.mha(FN.pack_pt(Qd), FN.pack_pt(Kd), FN.pack_pt(Vd), B, C, T, H, D), T, F)
    (out * w.to(DEV)).sum().backward()
    Qr, Kr, Vr = (x.double().requires_grad_(True) for x in (Q, K, V))
    ref = _ref(Qr, Kr, Vr, H)
    (ref * w.double()).sum().backward()
    assert_close(out, ref, tol=1e-5, what="attention output")
    if C == 1:  # (one key: its weight is 1 whatever the scores, dQ and dK are exactly zero -- gated by the fp32 formula's rounding)
        r32 = attention_and_grads(Q, K, V, w, H, torch.float32)
        assert_gated(Qd.grad, Qr.grad, r32[1], 1e-4, "dQ")
        assert_gated(Kd.grad, Kr.grad, r32[2], 1e-4, "dK")
    else:
        assert_close(Qd.grad, Qr.grad, tol=1e-4, what="dQ")
        assert_close(Kd.grad, Kr.grad, tol=1e-4, what="dK")
    assert_close(Vd.grad, Vr.grad, tol=1e-4, what="dV")


def _regime(regime, B, C, T, F, H, g):
    """Q, K, V [B, n, F] whose scaled scores q.k / sqrt(head) are ``large`` (max about 40), dominated by ONE key for every query
    (``one_key``: that key's score about 30 above the rest), or the same for every key (``equal``: identical keys)."""
    d = F // H
    Q, K, V = (torch.randn(B, n, F, generator=g) for n in (T, C, C))
    if regime == "large":
        s = torch.einsum("bthd,bchd->bhtc", Q.view(B, T, H, d), K.view(B, C, H, d)).abs().max() / math.sqrt(d)
        Q = Q * (40.0 / float(s))
    elif regime == "one_key":
        u = torch.randn(F, generator=g)
        u = u / u.view(H, d).norm(dim=1).repeat_interleave(d)  # (unit length in every head)
        Q, K = 0.3 * Q + 4.0 * u, 0.3 * K
        K[:, C // 2] = 7.5 * math.sqrt(d) * u
    else:
        K[:] = K[:, :1]
    return Q, K, V


def attention_and_grads(Q, K, V, dO, H, dtype):
    """(O, dQ, dK, dV) of per-head softmax(Q K^T / sqrt(head)) V in ``dtype``, written out in the form the kernels evaluate
    (score row with its log-sum-exp, P = exp(S - lse), D = rowsum(dO * O), dS = P (dO V^T - D)) -- in float32 it measures how
    much rounding the formula itself suffers on the case."""
    B, T, F = Q.shape
    d = F // H
    heads = lambda x: x.to(dtype).view(B, -1, H, d).permute(0, 2, 1, 3)  # noqa: E731
    merge = lambda x: x.permute(0, 2, 1, 3).reshape(B, -1, F)  # noqa: E731
    q, k, v, g = heads(Q), heads(K), heads(V), heads(dO)
    S = q @ k.transpose(-1, -2) / math.sqrt(d)
    P = torch.exp(S - torch.logsumexp(S, dim=-1, keepdim=True))
    O = P @ v
    D = (g * O).sum(-1, keepdim=True)
    dS = P * (g @ v.transpose(-1, -2) - D) / math.sqrt(d)
    return merge(O), merge(dS @ k), merge(dS.transpose(-1, -2) @ q), merge(P.transpose(-1, -2) @ g)


def assert_gated(got, ref64, ref32, tol, what):
    """max|got - ref| <= max(tol * max|ref|, 4 * max|fp32 evaluation - ref|) -- for cases whose float64 result is ill-conditioned
    in the rounding of the inputs (large scores: exp amplifies the rounding of q.k; a dominant key or identical keys: dQ / dK
    cancel to ~0, one key: they are exactly 0)."""
    got, ref, r32 = (t.detach().cpu().double() for t in (got, ref64, ref32))
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err, gate = float((got - ref).abs().max()), max(tol * float(ref.abs().max()), 4 * float((r32 - ref).abs().max()))
    assert err <= gate, f"{what}: max|d|={err:.3e} > gate {gate:.3e}"


@pytest.mark.parametrize("regime", ["large", "one_key", "equal"])
@pytest.mark.parametrize("B,C,T,H,D", [(2, 128, 70, 8, 32), (2, 33, 33, 8, 32), (2, 256, 70, 8, 16), (2, 129, 1, 8, 16)])
def test_mha_score_regimes(regime, B, C, T, H, D):
    """Scores where a missing max-subtraction overflows (large), where a mis-masked key tail or a wrong normaliser shows (one key
    that dominates every query; all keys equal: uniform weights).  Against float64; these float64 results are ill-conditioned
    (see ``assert_gated``), so the gate is max(fp32 gate, 4 x the error of the same formula evaluated in fp32 torch)."""
    from npf_gwwaveform_amd import functional as FN

    F = D * H
    g = torch.Generator().manual_seed(C + T + H + D)
    Q, K, V = _regime(regime, B, C, T, F, H, g)
    w = torch.randn(B, T, F, generator=g)
    Qd, Kd, Vd = (x.to(DEV).requires_grad_(True) for x in (Q, K, V))
    out = FN.unpack_pt(FN.mha(FN.pack_pt(Qd), FN.pack_pt(Kd), FN.pack_pt(Vd), B, C, T, H, D), T, F)
    (out * w.to(DEV)).sum().backward()
    r64, r32 = (attention_and_grads(Q, K, V, w, H, dt) for dt in (torch.float64, torch.float32))
    for i, (name, got, tol) in enumerate((("attention output", out, 1e-5), ("dQ", Qd.grad, 1e-4), ("dK", Kd.grad, 1e-4),
                                          ("dV", Vd.grad, 1e-4))):
        assert_gated(got, r64[i], r32[i], tol, f"{regime} {name}")


def test_mha_inference_equals_training_forward():
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(0)
    Q, K, V = (torch.randn(2, n, 128, generator=g).to(DEV) for n in (96, 50, 50))
    with torch.no_grad():
        a = FN.mha(FN.pack_pt(Q), FN.pack_pt(K), FN.pack_pt(V), 2, 50, 96, 8)
    b = FN.mha(FN.pack_pt(Q.requires_grad_(True)), FN.pack_pt(K), FN.pack_pt(V), 2, 50, 96, 8)
    assert torch.equal(a, b.detach())


def test_mha_rejects_other_head_sizes_and_too_many_keys():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import chain as CH

    x = CH.pt_empty(1, 32, 128, DEV)
    lib = L.load()
    assert lib.npf_mha_fwd(L.ptr(x), L.ptr(x), L.ptr(x), 1, 2, 32, 32, 128, L.ptr(x), None, None) == -1   # 64-feature heads
    assert lib.npf_mha_fwd(L.ptr(x), L.ptr(x), L.ptr(x), 1, 4, 129, 32, 128, L.ptr(x), None, None) == -1  # 32-feature heads: <= 128 keys
    assert lib.npf_mha_fwd(L.ptr(x), L.ptr(x), L.ptr(x), 1, 8, 257, 32, 128, L.ptr(x), None, None) == -1  # keys > 256


@pytest.mark.parametrize("B,T,F", [(3, 256, 128), (2, 70, 128), (2, 33, 32), (1, 5, 256), (2, 64, 48)])
def test_add_layernorm_matches_float64(B, T, F):
    """LayerNorm(a + b) on PT32 tensors (npf_add_layernorm_fwd / _bwd; TransformerAttender.forward's first LayerNorm,
    attention.py:566-575) against torch.nn.functional.layer_norm in float64: output, both input gradients, dgamma, dbeta."""
    from npf_gwwaveform_amd import functional as FN

    torch.manual_seed(T)
    ln = torch.nn.LayerNorm(F).to(DEV)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(B + T)
    a, b, w = (torch.randn(B, T, F, generator=g) for _ in range(3))
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = FN.unpack_pt(FN.add_layernorm(FN.pack_pt(ad), FN.pack_pt(bd), ln, B, T), T, F)
    (y * w.to(DEV)).sum().backward()
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    gam, bet = ln.weight.detach().double().cpu().requires_grad_(True), ln.bias.detach().double().cpu().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(ar + br, (F,), gam, bet, ln.eps)
    (ref * w.double()).sum().backward()
    assert_close(y, ref, tol=1e-5, what="LayerNorm(a + b)")
    assert_close(ad.grad, ar.grad, tol=1e-4, what="da")
    assert_close(bd.grad, br.grad, tol=1e-4, what="db")
    assert_close(ln.weight.grad, gam.grad, tol=1e-4, what="dgamma")
    assert_close(ln.bias.grad, bet.grad, tol=1e-4, what="dbeta")
