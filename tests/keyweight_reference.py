"""Reference definitions for training through context weights (``forward(w_cntxt=...)``): weighted attention, weighted mean and
their gradients in closed form, in plain torch at a chosen dtype (float64 for the reference, float32 for the "same formula in fp32"
term of the project's gate).  Shared by tests/test_keyweight_host.py (CPU) and tests/test_hip_keyweight.py (GPU).

A key (point) ``k`` of task ``b`` is admissible iff ``k < counts[b]`` and ``0 < w[b, k] < inf``.  Everything is evaluated on the
admissible rows alone (picked by index), so whatever the other rows hold -- NaN included -- never enters the arithmetic, and every
gradient of an inadmissible row is an exact zero.  Queries at or beyond ``q_counts[b]`` are not read and get zeros."""
import math

import torch


def admissible(W, counts):
    """bool [B, C]"""
    B, C = W.shape
    below = torch.arange(C).view(1, C) < torch.as_tensor(counts).clamp(0, C).view(B, 1)
    return below & (W > 0) & (W < math.inf)


def _q_count(q_counts, b, T):
    return T if q_counts is None else max(0, min(int(q_counts[b]), T))


def weighted_attention_direct(q, k, v, w, scale):
    """One task, admissible rows only, as a composition autograd can differentiate: softmax_k(scale <q, k> + log w_k) v."""
    return torch.softmax(q @ k.T * scale + torch.log(w), dim=-1) @ v


def weighted_attention_and_grads(Q, K, V, W, dO, counts, scale, dtype, q_counts=None):
    """(O, dQ, dK, dV, dW, lse) in the form the kernels evaluate: a = scale <q, k> + log w, lse = logsumexp_k a, p = exp(a - lse),
    D = <dO, O>, dA = p (<dO, v> - D); dq = scale dA k, dk = scale dA^T q, dv = p^T dO, dw = (sum_q dA) / w."""
    B, T, d = Q.shape
    C = K.shape[1]
    adm = admissible(W, counts)
    O, dQ = torch.zeros(B, T, d, dtype=dtype), torch.zeros(B, T, d, dtype=dtype)
    dK, dV = torch.zeros(B, C, d, dtype=dtype), torch.zeros(B, C, d, dtype=dtype)
    dW, lse = torch.zeros(B, C, dtype=dtype), torch.zeros(B, T, dtype=dtype)
    for b in range(B):
        idx, nq = adm[b].nonzero().flatten(), _q_count(q_counts, b, T)
        if idx.numel() == 0 or nq == 0:
            continue
        q, g = Q[b, :nq].to(dtype), dO[b, :nq].to(dtype)
        k, v, w = K[b, idx].to(dtype), V[b, idx].to(dtype), W[b, idx].to(dtype)
        a = q @ k.T * scale + torch.log(w)
        L = torch.logsumexp(a, dim=-1, keepdim=True)
        p = torch.exp(a - L)
        o = p @ v
        D = (g * o).sum(-1, keepdim=True)
        dA = p * (g @ v.T - D)
        O[b, :nq], lse[b, :nq], dQ[b, :nq] = o, L[:, 0], scale * dA @ k
        dK[b, idx], dV[b, idx], dW[b, idx] = scale * dA.T @ q, p.T @ g, dA.sum(0) / w
    return O, dQ, dK, dV, dW, lse


def weighted_mean_direct(r, w):
    """One task, admissible rows only: sum_k w_k r_k / sum_k w_k."""
    return (w.unsqueeze(-1) * r).sum(0) / w.sum()


def weighted_mean_and_grads(R, W, dOut, counts, dtype):
    """(out, dR, dW): out = sum w r / Wsum, dr_k = (w_k / Wsum) dOut, dw_k = <dOut, r_k - out> / Wsum."""
    B, C, F = R.shape
    adm = admissible(W, counts)
    out, dR, dW = torch.zeros(B, F, dtype=dtype), torch.zeros(B, C, F, dtype=dtype), torch.zeros(B, C, dtype=dtype)
    for b in range(B):
        idx = adm[b].nonzero().flatten()
        if idx.numel() == 0:
            continue
        r, w, g = R[b, idx].to(dtype), W[b, idx].to(dtype), dOut[b].to(dtype)
        Ws = w.sum()
        o = (w.unsqueeze(-1) * r).sum(0) / Ws
        out[b], dR[b, idx], dW[b, idx] = o, (w / Ws).unsqueeze(-1) * g, ((r - o) @ g) / Ws
    return out, dR, dW


def repeat_rows(X, w_int):
    """One task's rows [C, .] with row k repeated ``w_int[k]`` times (0: dropped)."""
    return X.repeat_interleave(torch.as_tensor(w_int, dtype=torch.long), dim=0)


# ---- whole models with a weight per context point, composed of the oracle's stages ------------------------------------------
def _scaledot_weighted(keys, queries, values, w):
    """The oracle's ``scaledot_attend`` with log w[b, k] added to the logits of key k: p_k ~ w_k exp(s_k)."""
    logits = torch.einsum("bkd,bqd->bqk", keys, queries) / math.sqrt(queries.size(-1)) + torch.log(w).unsqueeze(1)
    return torch.bmm(logits.softmax(dim=-1), values)


def _multihead_weighted(params, prefix, keys, queries, values, w, n_heads, post_process=True):
    """The oracle's ``multihead_attend`` (heads stacked as extra batches, index h * B + b, the head size in the scale) with the
    weights of task b on every one of its heads."""
    lin = torch.nn.functional.linear
    K = lin(keys, params[f"{prefix}.key_transform.weight"])
    Q = lin(queries, params[f"{prefix}.query_transform.weight"], params[f"{prefix}.query_transform.bias"])
    V = lin(values, params[f"{prefix}.value_transform.weight"])
    B, hs = keys.shape[0], K.shape[-1] // n_heads
    heads = lambda x: x.view(B, -1, n_heads, hs).permute(2, 0, 1, 3).contiguous().view(B * n_heads, -1, hs)  # noqa: E731
    ctx = _scaledot_weighted(heads(K), heads(Q), heads(V), w.repeat(n_heads, 1))
    ctx = ctx.view(n_heads, B, -1, hs).permute(1, 2, 0, 3).contiguous().view(B, -1, n_heads * hs)
    if post_process:
        ctx = lin(ctx, params[f"{prefix}.post_processor.weight"], params[f"{prefix}.post_processor.bias"])
    return ctx


def _transformer_weighted(O, params, prefix, keys, queries, values, w, n_heads):
    """The oracle's ``transformer_attend`` around the weighted multihead attention."""
    d, ln = queries.shape[-1], torch.nn.functional.layer_norm
    ctx = _multihead_weighted(params, prefix, keys, queries, values, w, n_heads, post_process=False)
    ctx = ln(ctx + queries, (d,), params[f"{prefix}.layer_norm1.weight"], params[f"{prefix}.layer_norm1.bias"])
    return ln(ctx + O.mlp(params, f"{prefix}.mlp", ctx), (d,), params[f"{prefix}.layer_norm2.weight"], params[f"{prefix}.layer_norm2.bias"])


def oracle_forward_weighted(O, cfg, params, Xc, Yc, Xt, w):
    """(loc, scale) [1, B, T, dy] of the oracle's forward pass in which context point k of task b carries weight w[b, k] > 0: the
    oracle's own per-point stages and decoder around a weighted mean (CNP) or the oracle's attention (scaled-dot, multihead,
    transformer) with log w added to the logits of every head (AttnCNP)."""
    Xc_enc, Xt_enc = O.mlp(params, "x_encoder", Xc), O.mlp(params, "x_encoder", Xt)
    R_pts = O.merge_flat(cfg, params, "xy_encoder", Xc_enc, Yc)
    if cfg.kind == "CNP":
        R = (w.unsqueeze(-1) * R_pts).sum(1, keepdim=True) / w.sum(1).view(-1, 1, 1)
        R_trgt = R.expand(Xt.shape[0], Xt.shape[1], cfg.r_dim).unsqueeze(0)
    else:
        assert cfg.kind == "AttnCNP"
        if cfg.attention == "scaledot":
            R_det = _scaledot_weighted(Xc_enc, Xt_enc, R_pts, w)
        elif cfg.attention == "multihead":
            R_det = _multihead_weighted(params, "attender", Xc_enc, Xt_enc, R_pts, w, cfg.n_heads)
        else:
            R_det = _transformer_weighted(O, params, "attender", Xc_enc, Xt_enc, R_pts, w, cfg.n_heads)
        R_trgt = R_det.unsqueeze(0)
    return O.decode(cfg, params, Xt_enc, R_trgt)
