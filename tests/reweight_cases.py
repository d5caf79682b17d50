"""Float64 references of the reweighted contexts, as direct formulas, shared by tests/test_reweight_host.py (CPU) and
tests/test_hip_reweight.py (GPU).  A key / point of replicate task ``j = s * B + b`` is admissible iff it lies below the count of
context task ``b`` and its weight is positive and finite."""
import math

import torch


def admissible(w, n):
    """bool [len(w)]: below the count ``n`` and 0 < w < inf (NaN fails both comparisons)."""
    return (torch.arange(w.shape[0]) < n) & (w > 0) & (w < math.inf)


def weighted_attention(Q, K, V, W, counts, q_counts, scale, dtype):
    """[S B, T, d] in ``dtype``: out(j, q) = sum_adm w_k exp(scale <Q_q, K_k>) V_k / sum_adm w_k exp(scale <Q_q, K_k>) with Q / K / V /
    counts of context task ``j % B`` (Q [B, T, d], K / V [B, C, d]) and ``W`` [S B, C]; zeros where no key is admissible and in the
    rows beyond a query count (``q_counts`` None: every row is a query)."""
    B, T, d = Q.shape
    n_tasks = W.shape[0]
    out = torch.zeros(n_tasks, T, d, dtype=dtype)
    for j in range(n_tasks):
        b = j % B
        adm = admissible(W[j], counts[b])
        nq = T if q_counts is None else q_counts[b]
        if not adm.any() or nq == 0:
            continue
        q, k, v, w = Q[b, :nq].to(dtype), K[b, adm].to(dtype), V[b, adm].to(dtype), W[j, adm].to(dtype)
        s = q @ k.T * scale
        p = w * torch.exp(s - s.max(dim=1, keepdim=True).values)  # (the shift cancels in the ratio)
        out[j, :nq] = (p @ v) / p.sum(dim=1, keepdim=True)
    return out


def weighted_mean_ref(R, W, counts, dtype):
    """[S B, F] in ``dtype``: sum_adm w_k R_k / sum_adm w_k of context task ``j % B`` (R [B, pts, F], W [S B, pts]); zeros where no
    point is admissible."""
    B = R.shape[0]
    out = torch.zeros(W.shape[0], R.shape[2], dtype=dtype)
    for j in range(W.shape[0]):
        b = j % B
        adm = admissible(W[j], counts[b])
        if adm.any():
            w = W[j, adm].to(dtype)
            out[j] = (w.unsqueeze(1) * R[b, adm].to(dtype)).sum(0) / w.sum()
    return out


def expand_context(X, Y, w_int):
    """One task's context with row ``i`` repeated ``w_int[i]`` times (0: removed): X [C, dx], Y [C, dy], w_int integer [C] ->
    (X', Y') of ``w_int.sum()`` rows, in the order of the rows."""
    idx = torch.repeat_interleave(torch.arange(w_int.shape[0]), w_int.long())
    return X[idx], Y[idx]


def kfold_weights_ref(folds, k):
    """float64 [k, B, rows] by the definition: W[f, b, i] = 1 if folds[b, i] != f else 0."""
    B, rows = folds.shape
    W = torch.zeros(k, B, rows, dtype=torch.float64)
    for f in range(k):
        for b in range(B):
            for i in range(rows):
                W[f, b, i] = 0.0 if int(folds[b, i]) == f else 1.0
    return W
