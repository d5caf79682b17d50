"""Inputs and references of the multihead-attention edge tests (tests/test_hip_mha_edges.py, checked on the CPU by
tests/test_mha_cases_host.py): the fused kernel (csrc/mha_kernel.hip) treats every (task, head) as one attention problem of width
D = 16 or 32 over 16-key blocks, so the cases are built per (task, head) -- ``masked_cases.build`` with B * H tasks of width D and
the kernel's key block KB = 16 (NOT ``masked_cases.key_block(d)``), every count equal to C -- and the heads merged afterwards: head
h is the feature slice D h : D h + D.  V and dO carry ``masked_cases.FACTORS`` over the B * H axis, so neighbouring heads of one
task differ by up to 1e4 and the gate (``assert_gated_per_task`` of tests/test_hip_masked_edges.py on tensors split to
[B * H, n, D]) is taken per (task, head).

The references are ``attention_and_grads`` of tests/test_hip_mha.py in float64 and float32, and the float64 log-sum-exp of the
scaled scores per (task, head, query).

Which branch of the gate governs, from the references alone (``test_which_branch_governs_per_regime`` of the host test, B = 2, H = 3,
T = 17; the figure is the largest 4 max|fp32 - f64| / (tol max(max|ref_b|, 1e-3 max|ref|)) over the regime's shapes and (task,
head)s: above 1 the fp32 branch governs somewhere, below 1 the tolerance branch everywhere):

    regime         D   output      dQ      dK      dV
    ascending      16     3.09    25.5    8.16   0.182
    descending     16     3.53    19.4    3.68   0.167
    huge_pos       16     6.88    12.2   0.399   0.739
    huge_neg       16      5.8      14   0.472   0.678
    one_key@first  16  1.5e-05 1.56e+09 1.19e+09 0.00601
    one_key@last   16  1.47e-05 2.2e+09 5.18e+09 0.00714
    one_key@edge   16  1.44e-05 2.8e+09 2.65e+09 0.00572
    equal          16    0.319  0.0276  0.0145  0.0181
    ascending      32        3    37.8    20.8    0.12
    descending     32     2.79    22.1    3.67   0.204
    huge_pos       32     7.46    14.5    1.16   0.571
    huge_neg       32     7.03    14.8   0.447   0.603
    one_key@first  32  7.48e-06 1.4e+09 1.83e+09 0.00834
    one_key@last   32  7.31e-06 2.27e+09 2.79e+09 0.00815
    one_key@edge   32  7.8e-06 2.34e+09 1.75e+09 0.00524
    equal          32    0.268  0.0425  0.0109  0.0128

(``one_key@*``: the weights are one-hot to 1e-13, so the float64 dQ / dK cancel to about 1e-10 while the fp32 formula keeps a
rounding residue of dO.V - dO.O: there the gate is 4 x that residue, see tests/test_hip_mha_edges.py.)

The random cases (``RANDOM_CASES``) all stay below 1 on all four tensors (``test_random_cases_are_not_ill_conditioned``: at most 0.50
on the output, 0.07 on a gradient; dQ / dK at C == 1 excepted, which are 0 -- the float64 formula leaves 1e-12 -- and have the
bound of ``single_key_bounds`` for their rounding residue)."""
import math

import torch

import masked_cases as MC
from test_hip_mha import attention_and_grads

KB = 16  # keys per block of csrc/mha_kernel.hip, both head sizes
TENSORS = (("output", 1e-5), ("dQ", 1e-4), ("dK", 1e-4), ("dV", 1e-4))

# ---- shapes --------------------------------------------------------------------------------------------------------------------
REGIME_B, REGIME_H, REGIME_T = 2, 3, 17
REGIME_SHAPES = tuple((16, C) for C in (17, 65, 129, 255, 256)) + tuple((32, C) for C in (17, 65, 127, 128))  # (D, C)

KEY_EDGES = {16: (1, 15, 16, 17, 64, 65, 128, 129, 255, 256), 32: (1, 15, 16, 17, 63, 64, 65, 127, 128)}  # at T = 17, H = 3
QUERY_EDGES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)                                                  # at C = 65, H = 3
HEAD_COUNTS = ((16, 1), (16, 2), (16, 8), (32, 1), (32, 4))                                               # (D, H)
HEAD_SIZES = ((33, 33), (64, 64))                                                                         # (C, T)
RANDOM_B = 2
RANDOM_CASES = tuple(dict.fromkeys(  # (D, H, C, T), each once: (C, T) = (65, 17) is a key edge and a query edge
    [(D, 3, C, 17) for D in (16, 32) for C in KEY_EDGES[D]] + [(D, 3, 65, T) for D in (16, 32) for T in QUERY_EDGES]
    + [(D, H, C, T) for D, H in HEAD_COUNTS for C, T in HEAD_SIZES]))


# ---- heads ---------------------------------------------------------------------------------------------------------------------
def split_heads(x, H):
    """[B, n, H * D] -> [B * H, n, D]: head h of task b (the features D h : D h + D) is row b * H + h."""
    B, n, F = x.shape
    return x.reshape(B, n, H, F // H).permute(0, 2, 1, 3).reshape(B * H, n, F // H)


def merge_heads(x, H):
    """[B * H, n, D] -> [B, n, H * D], the inverse of ``split_heads``."""
    BH, n, D = x.shape
    return x.reshape(BH // H, H, n, D).permute(0, 2, 1, 3).reshape(BH // H, n, H * D)


# ---- builders ------------------------------------------------------------------------------------------------------------------
def regime_case(regime, D, C, B=REGIME_B, H=REGIME_H, T=REGIME_T):
    """fp32 Q, dO [B, T, H * D] and K, V [B, C, H * D]: every (task, head) is one task of ``masked_cases.build`` with all C keys
    valid; the scale 1 / sqrt(D) the builder assumes is the kernel's.  ``one_key@edge`` sits on row (C - 1) // 16 * 16."""
    g = torch.Generator().manual_seed(1000 * D + 10 * C + MC.REGIMES.index(regime))
    Q, K, V = MC.build(regime, [C] * (B * H), C, T, D, KB, g)
    V, dO = MC.scale_per_task(V, torch.randn(B * H, T, D, generator=g))
    return tuple(merge_heads(x, H) for x in (Q, K, V, dO))


def random_case(D, H, C, T, B=RANDOM_B):
    """Q, K ~ 1.5 N(0, 1), V ~ N(0, 1) as tests/test_hip_mha.py draws them, V and dO with the per-(task, head) factors."""
    F = D * H
    g = torch.Generator().manual_seed(100000 * D + 1000 * H + 300 * C + T)
    Q, K, V = (torch.randn(B, n, F, generator=g) * s for n, s in ((T, 1.5), (C, 1.5), (C, 1.0)))
    dO = torch.randn(B, T, F, generator=g)
    V, dO = (merge_heads(x, H) for x in MC.scale_per_task(split_heads(V, H), split_heads(dO, H)))
    return Q, K, V, dO


# ---- references ----------------------------------------------------------------------------------------------------------------
def references(Q, K, V, dO, H):
    """((O, dQ, dK, dV) in float64, the same formula in float32), merged [B, n, H * D]."""
    return tuple(attention_and_grads(Q, K, V, dO, H, dt) for dt in (torch.float64, torch.float32))


def scores(Q, K, H, dtype=torch.float64):
    """[B * H, T, C]: the scaled scores q . k / sqrt(D) of every (task, head) in ``dtype``."""
    q, k = split_heads(Q.to(dtype), H), split_heads(K.to(dtype), H)
    return q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])


def scores_in_order(Q, K, H):
    """float64 [B * H, T, C] like ``scores``, summed feature by feature in the same order for every key -- what ``equal`` claims
    (every score of a query is the same number bit for bit) holds for any fixed order of the sum; a BLAS product may block the
    keys differently and then rounds them differently on some hosts."""
    q, k = split_heads(Q.double(), H), split_heads(K.double(), H)
    S = torch.zeros(q.shape[0], q.shape[1], k.shape[1], dtype=torch.float64)
    for f in range(q.shape[-1]):
        S += q[:, :, None, f] * k[:, None, :, f]
    return S / math.sqrt(q.shape[-1])


def lse_references(Q, K, H):
    """(float64, float32) log-sum-exp of the scaled scores, [B, H, T] as the kernel stores it."""
    B, T = Q.shape[:2]
    return tuple(torch.logsumexp(scores(Q, K, H, dt), -1).view(B, H, T) for dt in (torch.float64, torch.float32))


def single_key_bounds(Q, K, V, dO, H):
    """C == 1: the weight of the one key is 1, dQ and dK are exactly 0 in float64 and one rounding residue of dO.V - dO.O in the
    kernel.  Per (task, head) [B * H] the project's 1e-4 of the magnitude the terms have BEFORE they cancel, from the float64 inputs
    alone: (1e-4 scale max_q sum_d |dO_d V_d| max|K|  for dQ,  the same with max|Q|  for dK)."""
    assert K.shape[1] == 1
    q, k, v, g = (split_heads(x.double(), H) for x in (Q, K, V, dO))
    terms = (g.abs() * v.abs()).sum(-1).amax(-1)  # [B * H]
    scale = 1.0 / math.sqrt(q.shape[-1])
    return 1e-4 * scale * terms * k.abs().amax((-1, -2)), 1e-4 * scale * terms * q.abs().amax((-1, -2))


def branch_ratio(ref64, ref32, tol, H):
    """[B * H]: 4 max|fp32 - f64| / (tol max(max|ref_b|, 1e-3 max|ref|)) per (task, head): the fp32 branch of the gate over its
    tolerance branch."""
    r, s = split_heads(ref64, H), split_heads(ref32.double(), H)
    err = (s - r).abs().amax((-1, -2))
    return 4 * err / (tol * torch.clamp(r.abs().amax((-1, -2)), min=1e-3 * float(r.abs().max())))
