"""Host side of training through context weights (CPU, no kernel launched): the closed-form gradients of
tests/keyweight_reference.py against float64 autograd of the direct definition and against a central finite difference, integer
weights against physically repeated rows, the declarations of the new exports, and every refusal of
``functional.key_weighted_attention`` / ``key_weighted_mean`` / ``forward(w_cntxt=...)`` / ``influence`` that needs no device."""
import inspect
import math
import os
import re

import pytest
import torch

import keyweight_reference as KR
from test_dispatch_rules import _model, bf16_mode  # noqa: F401  (read-only: the model builder and the bf16 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _problem(seed, B=3, C=9, T=6, d=8):
    g = torch.Generator().manual_seed(seed)
    Q, K, V, dO = (torch.randn(B, n, d, generator=g, dtype=F64) for n in (T, C, C, T))
    W = torch.exp(torch.rand(B, C, generator=g, dtype=F64) * 4 - 2)
    W[0, 2], W[1, 0], W[2, 5] = 0.0, -1.0, math.nan  # (removed points)
    return Q, K, V, dO, W, (C, 6, 7), (T, 4, 0)


# ---- closed forms against autograd and finite differences ------------------------------------------------------------------
def test_attention_closed_form_equals_float64_autograd():
    Q, K, V, dO, W, counts, q_counts = _problem(1)
    scale = 1.0 / math.sqrt(Q.shape[-1])
    O, dQ, dK, dV, dW, lse = KR.weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, F64, q_counts)
    adm = KR.admissible(W, counts)
    for b in range(Q.shape[0]):
        idx, nq = adm[b].nonzero().flatten(), q_counts[b]
        assert (dK[b][~adm[b]] == 0).all() and (dV[b][~adm[b]] == 0).all() and (dW[b][~adm[b]] == 0).all()
        assert (O[b, nq:] == 0).all() and (dQ[b, nq:] == 0).all() and (lse[b, nq:] == 0).all()
        if nq == 0:
            assert (dK[b] == 0).all() and (dW[b] == 0).all()
            continue
        q, k, v, w = (x.clone().requires_grad_(True) for x in (Q[b, :nq], K[b, idx], V[b, idx], W[b, idx]))
        o = KR.weighted_attention_direct(q, k, v, w, scale)
        (o * dO[b, :nq]).sum().backward()
        for name, got, ref in (("O", O[b, :nq], o.detach()), ("dQ", dQ[b, :nq], q.grad), ("dK", dK[b, idx], k.grad),
                               ("dV", dV[b, idx], v.grad), ("dW", dW[b, idx], w.grad)):
            assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0), (b, name)
        a = q.detach() @ k.detach().T * scale + torch.log(w.detach())
        assert float((lse[b, :nq] - torch.logsumexp(a, -1)).abs().max()) <= 1e-12


def test_attention_dw_equals_a_central_finite_difference():
    Q, K, V, dO, W, counts, q_counts = _problem(2)
    scale = 1.0 / math.sqrt(Q.shape[-1])
    dW = KR.weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, F64, q_counts)[4]
    loss = lambda w: float((KR.weighted_attention_and_grads(Q, K, V, w, dO, counts, scale, F64, q_counts)[0] * dO_full).sum())  # noqa: E731
    dO_full = dO.clone()
    for b, nq in enumerate(q_counts):
        dO_full[b, nq:] = 0
    adm = KR.admissible(W, counts)
    h = 1e-6
    for b, k in ((0, 0), (0, 8), (1, 3), (1, 5)):
        assert adm[b, k]
        wp, wm = W.clone(), W.clone()
        wp[b, k] += h
        wm[b, k] -= h
        fd = (loss(wp) - loss(wm)) / (2 * h)
        assert abs(fd - float(dW[b, k])) <= 1e-6 * max(abs(float(dW[b, k])), 1.0), (b, k, fd, float(dW[b, k]))


def test_mean_closed_form_equals_float64_autograd_and_finite_difference():
    g = torch.Generator().manual_seed(5)
    B, C, F = 3, 9, 7
    R, dOut = torch.randn(B, C, F, generator=g, dtype=F64), torch.randn(B, F, generator=g, dtype=F64)
    W = torch.exp(torch.rand(B, C, generator=g, dtype=F64) * 4 - 2)
    W[0, 1], W[1, 0], W[1, 4], W[2] = 0.0, math.inf, math.nan, 0.0
    counts = (C, 6, C)
    out, dR, dW = KR.weighted_mean_and_grads(R, W, dOut, counts, F64)
    adm = KR.admissible(W, counts)
    assert (out[2] == 0).all() and (dR[2] == 0).all() and (dW[2] == 0).all()  # (no admissible weight)
    for b in range(2):
        idx = adm[b].nonzero().flatten()
        r, w = R[b, idx].clone().requires_grad_(True), W[b, idx].clone().requires_grad_(True)
        o = KR.weighted_mean_direct(r, w)
        (o * dOut[b]).sum().backward()
        for name, got, ref in (("out", out[b], o.detach()), ("dR", dR[b, idx], r.grad), ("dW", dW[b, idx], w.grad)):
            assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0), (b, name)
        assert (dR[b][~adm[b]] == 0).all() and (dW[b][~adm[b]] == 0).all()
    h = 1e-6
    wp, wm = W.clone(), W.clone()
    wp[0, 3] += h
    wm[0, 3] -= h
    f = lambda w: float((KR.weighted_mean_and_grads(R, w, dOut, counts, F64)[0] * dOut).sum())  # noqa: E731
    assert abs((f(wp) - f(wm)) / (2 * h) - float(dW[0, 3])) <= 1e-6 * max(abs(float(dW[0, 3])), 1.0)


def test_integer_weights_equal_physically_repeated_rows_in_float64():
    g = torch.Generator().manual_seed(3)
    B, C, T, d = 3, 11, 5, 8
    Q, K, V, dO = (torch.randn(B, n, d, generator=g, dtype=F64) for n in (T, C, C, T))
    W = torch.randint(0, 4, (B, C), generator=g).double()
    counts, scale = (11, 7, 4), 1.0 / math.sqrt(d)
    O, dQ = KR.weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, F64)[:2]
    mean = KR.weighted_mean_and_grads(V, W, dO[:, 0], counts, F64)[0]
    for b in range(B):
        w = W[b].clone()
        w[counts[b]:] = 0
        k, v = KR.repeat_rows(K[b], w), KR.repeat_rows(V[b], w)
        assert k.shape[0] == int(w.sum()) > 0
        q = Q[b].clone().requires_grad_(True)
        plain = torch.softmax(q @ k.T * scale, dim=-1) @ v
        (plain * dO[b]).sum().backward()
        assert float((O[b] - plain.detach()).abs().max()) <= 1e-12 * float(plain.detach().abs().max())
        assert float((dQ[b] - q.grad).abs().max()) <= 1e-12 * float(q.grad.abs().max())
        assert float((mean[b] - v.mean(0)).abs().max()) <= 1e-12 * float(v.mean(0).abs().max())


@pytest.mark.parametrize("kind,kw", [("CNP", {}), ("AttnCNP", {}), ("AttnCNP", dict(attention="multihead")),
                                     ("AttnCNP", dict(attention="transformer"))])
def test_weighted_oracle_reference_equals_the_oracle_on_repeated_rows(kind, kw):
    """``KR.oracle_forward_weighted`` (the float64 reference of ``influence``): with all-ones weights it is the oracle's forward,
    with integer weights the oracle's forward on the context with its rows repeated."""
    import specs
    from oracle import npf_oracle as O

    case = dict(dict(kind=kind, r=64 if not kw else 128, C=7, B=2, dx=1, dy=2, L_xy=2, L_dec=2, T=5), **kw)
    cfg = specs.cfg_of(case)
    p64 = {k: v.double() for k, v in specs.make_params(case, seed=11).items()}
    inp = {k: v.double() for k, v in specs.make_inputs(case, seed=4321).items()}
    Xc, Yc, Xt = inp["X_cntxt"], inp["Y_cntxt"], inp["X_trgt"]
    ref = O.forward(cfg, p64, Xc, Yc, Xt, None, training=False)
    loc, scale = KR.oracle_forward_weighted(O, cfg, p64, Xc, Yc, Xt, torch.ones(2, 7, dtype=F64))
    assert float((loc - ref["loc"]).abs().max()) <= 1e-12 and float((scale - ref["scale"]).abs().max()) <= 1e-12
    W = torch.tensor([[1, 2, 0, 3, 1, 0, 2], [0, 0, 1, 0, 0, 3, 0]])
    for b in range(2):
        keep = W[b] > 0
        loc, scale = KR.oracle_forward_weighted(O, cfg, p64, Xc[b:b + 1, keep], Yc[b:b + 1, keep], Xt[b:b + 1], W[b:b + 1, keep].double())
        ref = O.forward(cfg, p64, KR.repeat_rows(Xc[b], W[b]).unsqueeze(0), KR.repeat_rows(Yc[b], W[b]).unsqueeze(0), Xt[b:b + 1], None,
                        training=False)
        assert float((loc - ref["loc"]).abs().max()) <= 1e-12 * max(1.0, float(ref["loc"].abs().max())), (kind, kw, b)
        assert float((scale - ref["scale"]).abs().max()) <= 1e-12, (kind, kw, b)


# ---- the C ABI and the public interface --------------------------------------------------------------------------------------
def test_header_declares_the_new_exports_and_the_binding_lists_them():
    from npf_gwwaveform_amd import _lib as L

    hdr = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(npf_\w+)\s*\(", hdr, flags=re.M))
    for name, n_args in (("npf_masked_attn_fwd_weighted_ex", 15), ("npf_masked_attn_bwd_weighted", 19), ("npf_weighted_mean_bwd", 11)):
        assert name in declared and name in L.SIGNATURES
        args = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(args.split(",")) == n_args == len(L.SIGNATURES[name][1]), name
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    # npf_masked_attn_fwd_weighted keeps its signature
    plain = re.search(r"npf_masked_attn_fwd_weighted\s*\(([^;]*)\);", hdr).group(1)
    assert len(plain.split(",")) == 14 and "lse" not in plain


def test_forward_and_influence_signatures():
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import functional as FN

    for cls in (A.CNP, A.AttnCNP):  # (the base class keeps the reference's argument list plus the counts)
        assert list(inspect.signature(cls.forward).parameters) == [
            "self", "X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt", "w_cntxt"], cls
    assert list(inspect.signature(A.NeuralProcessFamily.influence).parameters) == [
        "self", "X_cntxt", "Y_cntxt", "X_trgt", "Y_trgt", "n_cntxt", "n_trgt"]
    assert list(inspect.signature(FN.key_weighted_attention).parameters) == [
        "q_pt", "k_pt", "v_pt", "w", "n_valid", "n_tasks", "n_keys", "n_queries", "d", "scale", "n_q_valid"]
    assert list(inspect.signature(FN.key_weighted_mean).parameters) == ["R_pt", "w", "n_valid", "n_tasks", "pts", "F"]
    assert hasattr(A, "TrainKeyWeights")


def test_functional_refusals_need_no_device():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    B, C, T, d = 2, 5, 3, 8
    q, k = torch.zeros(pt_shape(B, T, d)), torch.zeros(pt_shape(B, C, d))
    w, n = torch.ones(B, C), torch.ones(B, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        FN.key_weighted_attention(q, k, k, w, n, B, C, T, 6, 1.0)
    with pytest.raises(NotImplementedError, match="up to 256"):
        FN.key_weighted_attention(q, k, k, w, n, B, C, T, 260, 1.0)
    with pytest.raises(ValueError, match="negative size"):
        FN.key_weighted_attention(q, k, k, w, n, B, -1, T, d, 1.0)
    with pytest.raises(ValueError, match="k_pt must be an fp32 PT32 tensor"):
        FN.key_weighted_attention(q, k[:1], k, w, n, B, C, T, d, 1.0)
    with pytest.raises(ValueError, match="q_pt must be an fp32 PT32 tensor"):
        FN.key_weighted_attention(q.double(), k, k, w, n, B, C, T, d, 1.0)
    with pytest.raises(ValueError, match="w must be a float device tensor"):
        FN.key_weighted_attention(q, k, k, w.long(), n, B, C, T, d, 1.0)
    with pytest.raises(ValueError, match="one weight per"):
        FN.key_weighted_attention(q, k, k, torch.ones(B, C + 1), n, B, C, T, d, 1.0)
    with pytest.raises(ValueError, match="w must live on the device"):
        FN.key_weighted_attention(q, k, k, w, n, B, C, T, d, 1.0)
    with pytest.raises(ValueError, match="pts >= 1"):
        FN.key_weighted_mean(k, w, n, B, 0, d)
    with pytest.raises(ValueError, match="R_pt must be an fp32 PT32 tensor"):
        FN.key_weighted_mean(k[:1], w, n, B, C, d)
    with pytest.raises(ValueError, match="w must be a float device tensor"):
        FN.key_weighted_mean(k, [1.0], n, B, C, d)
    with pytest.raises(ValueError, match="w must live on the device"):
        FN.key_weighted_mean(k, w, n, B, C, d)


def _xyt(B=2, C=4, T=3):
    return torch.zeros(B, C, 1), torch.zeros(B, C, 2), torch.zeros(B, T, 1), torch.zeros(B, T, 2)


def test_model_refusals_name_the_option(bf16_mode):  # noqa: F811
    import npf_gwwaveform_amd as A

    w = torch.ones(2, 4)
    with pytest.raises(NotImplementedError, match="w_cntxt.*bf16"):
        _model("AttnCNP", 128)(*_xyt(), w_cntxt=w)
    with pytest.raises(NotImplementedError, match="w_cntxt.*bf16"):
        _model("CNP", 128).influence(*_xyt())
    with pytest.raises(NotImplementedError, match="w_cntxt.*is_self_attn"):
        A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)(*_xyt(), w_cntxt=w)


def test_model_refusals_in_fp32_mode():
    import npf_gwwaveform_amd as A

    w = torch.ones(2, 4)
    with pytest.raises(NotImplementedError, match="w_cntxt.*is_self_attn"):
        A.AttnCNP(1, 2, r_dim=32, is_self_attn=True)(*_xyt(), w_cntxt=w)
    for kind, kw in (("LNP", dict(encoded_path="latent")), ("AttnLNP", {})):
        with pytest.raises(NotImplementedError, match="w_cntxt.*latent models"):
            _model(kind, 128, **kw)(*_xyt(), w_cntxt=w)
        with pytest.raises(NotImplementedError, match="w_cntxt.*latent models"):
            _model(kind, 128, **kw).influence(*_xyt())
    m = _model("CNP", 128)
    with pytest.raises(ValueError, match=r"w_cntxt must have shape \[2, 4\]"):
        m(*_xyt(), w_cntxt=torch.ones(2, 5))
    with pytest.raises(ValueError, match="w_cntxt must be a float device tensor"):
        m(*_xyt(), w_cntxt=torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (accepted: the refusal is the device check of every forward)
        m(*_xyt(), w_cntxt=w)


def test_existing_weighted_wrappers_still_refuse_gradients():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    k = torch.zeros(pt_shape(2, 5, 8))
    w = torch.ones(2, 5, requires_grad=True)
    n = torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="inference only"):
        FN.masked_attention_weighted(k, k, k, w, n, 2, 2, 5, 5, 8, 1.0)
    with pytest.raises(RuntimeError, match="inference only"):
        FN.weighted_mean(k, w, n, 2, 2, 5, 8)


def test_trainer_passes_the_weights_on():
    from npf_gwwaveform_amd.train import _counts_of

    w = torch.ones(2, 4)
    assert _counts_of(dict(X_cntxt=None, w_cntxt=w)) == {"w_cntxt": w}
    assert _counts_of(dict(X_cntxt=None)) == {}
