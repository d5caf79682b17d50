"""Inputs of the masked-attention edge tests (tests/test_hip_masked_edges.py): score regimes placed relative to every task's key
count and to the key blocks the kernels walk (csrc/masked_kernels.hip: KB = 32 keys, 16 at the 256-wide instance).

Keys are ``a_k u + noise`` and queries ``c u + noise`` with ``u`` a unit vector and the noise orthogonal to it, so the scaled score
of query q and key k is ``a_k c / sqrt(d) + NOISE^2 <n_q, n_k> / sqrt(d)``: the wanted score plus a term of standard deviation
NOISE^2 = 0.09 at every width.  Every property holds for a task's VALID keys; the rows beyond the count score about 30 above the
task's largest valid score, so a kernel that let one of them through would be dominated by it."""
import math

import torch

REGIMES = ("ascending", "descending", "huge_pos", "huge_neg", "one_key@first", "one_key@last", "one_key@edge", "equal")
FACTORS = (1.0, 1e-2, 1e2, 1e-1)  # per-task magnitudes of V and dO (the operation is linear in both)
NOISE = 0.3
ONE_KEY_GAP = 30.0
EQUAL_FREE = 4


def key_block(d):
    """Keys per block of the instance that computes width ``d``."""
    return 16 if d > 128 else 32


def one_key_index(regime, n, KB):
    """Index of the dominant key of a ``one_key@...`` task with ``n`` >= 1 valid keys: 0, the last valid key (inside the partial last
    block), or the largest multiple of KB below the count (first row of a block; 0 for counts up to KB)."""
    where = regime.split("@")[1]
    return {"first": 0, "last": n - 1, "edge": (n - 1) // KB * KB}[where]


def target_scores(regime, n, KB, gen):
    """float64 [n]: the scores the valid keys of one task are built for (``n`` >= 1; every query of the task sees the same)."""
    r = torch.rand(n, generator=gen, dtype=torch.float64)
    if regime == "ascending":
        return torch.linspace(-40.0, 40.0, n, dtype=torch.float64)
    if regime == "descending":
        return torch.linspace(40.0, -40.0, n, dtype=torch.float64)
    if regime == "huge_pos":  # (the maximum at a random key, the rest up to 5 below it: several keys share the weight)
        s = 100.0 - 5.0 * r
        s[int(torch.randint(n, (1,), generator=gen))] = 100.0
        return s
    if regime == "huge_neg":
        return -100.0 + 0.8 * (r - 0.5)
    if regime.startswith("one_key@"):
        s = 2.0 * r - 1.0
        s[one_key_index(regime, n, KB)] = ONE_KEY_GAP
        return s
    raise ValueError(regime)


def build(regime, counts, C_pad, T, d, KB, gen):
    """fp32 Q [B, T, d], K [B, C_pad, d], V [B, C_pad, d] of ``regime`` for tasks with ``counts[b]`` valid keys.

    ``equal``: the valid keys of a task are identical in the features 0 .. d - 5 and every query holds 0 in the last EQUAL_FREE = 4,
    where the keys differ.  Every score of a query is then the same number bit for bit and the weights are 1 / count, as with
    wholly identical keys (``_regime`` of tests/test_hip_mha.py), but dQ = scale * sum_k dS_k K_k is a number.  With wholly
    identical keys it is (sum_k dS_k) K_0 = 0 for every task, and was replaced for that: measured on the references alone (CPU,
    the three shapes of the GPU test), the float64 dQ was at most 7e-12 over the whole batch while the same formula in fp32
    missed it by up to 5e-3, with errors of one task's rows a factor 20 apart (each row's error is one rounding residue of
    sum_k dS_k times K_0) -- so the gate was 4 x one such residue, and for a task with a single valid query row a single draw
    of it against a single draw of the kernel's.  As built now the fp32 formula errs by at most 3e-6 of each task's max|dQ|."""
    B = len(counts)
    Q, K, V = (torch.randn(B, n, d, generator=gen, dtype=torch.float64) for n in (T, C_pad, C_pad))
    if regime == "equal":
        for b, n in enumerate(counts):
            K[b, :n, :d - EQUAL_FREE] = K[b, :1, :d - EQUAL_FREE]
        Q[..., d - EQUAL_FREE:] = 0
        return Q.float(), K.float(), V.float()
    u = torch.randn(d, generator=gen, dtype=torch.float64)
    u = u / u.norm()
    Q, K = (NOISE * (X - (X @ u).unsqueeze(-1) * u) for X in (Q, K))  # (noise orthogonal to u)
    c = 2.0 * d ** 0.25
    a = torch.empty(B, C_pad, dtype=torch.float64)
    for b, n in enumerate(counts):
        s = target_scores(regime, n, KB, gen) if n else torch.zeros(0, dtype=torch.float64)
        a[b, :n] = s
        a[b, n:] = (float(s.max()) if n else 0.0) + 30.0
    K = K + (a * math.sqrt(d) / c).unsqueeze(-1) * u
    Q = Q + c * u
    return Q.float(), K.float(), V.float()


def scores64(Q, K, b, n, d):
    """float64 [T, n]: the scaled scores of task ``b`` over its valid keys."""
    return Q[b].double() @ K[b, :n].double().T / math.sqrt(d)


def scale_per_task(*tensors):
    """Each tensor [B, ...] with task b multiplied by FACTORS[b % 4]."""
    B = tensors[0].shape[0]
    f = torch.tensor([FACTORS[b % len(FACTORS)] for b in range(B)], dtype=tensors[0].dtype).view(B, 1, 1)
    return tuple(t * f for t in tensors)


def key_counts(C_pad, KB):
    """Eight counts: 0, 1, KB, KB + 1, C_pad - 1, C_pad and two in the middle, the edge counts on the small per-task factors."""
    return [C_pad // 2 + 5, 1, C_pad, KB, 0, KB + 1, 3 * C_pad // 4 + 2, C_pad - 1]
