"""The prefix + tail instance of the masked attention forward kernel (csrc/masked_kernels.hip: ``npf_masked_attn_fwd_prefix``,
``functional.masked_attention_prefix``): task ``j`` of ``S * P`` attends over the first ``n_prefix[j % P]`` rows of prefix task
``j % P`` followed by the first ``n_tail[j]`` rows of its own tail.

The reference is a float64 evaluation of ``softmax(q [K_pre[:n_p]; K_tail[:n_t]]^T scale) [V_pre; V_tail]`` per task; the gate is the
per-task fp32 gate of tests/test_hip_masked_edges.py (``assert_gated_per_task``, which lives in that file: 1e-5 of the task's output or
4 x the error of the same formula in fp32), with tasks whose magnitudes differ (``masked_cases.scale_per_task``)."""
import math

import pytest
import torch

import masked_cases as MC
from helpers import launch_witness
from test_hip_masked_edges import _poison_feature_padding, assert_gated_per_task

gpu = pytest.mark.gpu
DEV = "cuda:0"
P, C_PAD, M_TAIL = 3, 70, 40
PRE_COUNTS = (0, 1, 31, 32, 33, 70)
TAIL_COUNTS = (0, 1, 15, 16, 17, 32, 40)


def _counts(S, T):
    """Prefix counts [P] and tail counts [S * P] of one case.  Deterministic: over the three query sizes (and the two S) of a width
    the prefix cycles through all six listed counts and the tails through all seven, so every tile instance sees every listed count
    in both segments; (0, 0) and (k, 0) occur in every case, (0, k) in every case with S = 2 (task P reads the empty prefix task 0)."""
    t = (1, 17, 65).index(T)
    pre = [0, PRE_COUNTS[1 + (2 * t + S - 1) % 5], PRE_COUNTS[1 + (2 * t + S + 1) % 5]]
    free = [TAIL_COUNTS[1 + (k + 2 * t + 3 * (S - 1)) % 6] for k in range(S * P)]
    tail = [0, 0] + free[:S * P - 2]   # task 0: (0, 0); task 1: (k, 0); every other task has a tail
    assert pre[1] > 0 and pre[2] > 0 and tail[2] > 0 and (S == 1 or tail[P] > 0)
    cases = {(pre[j % P] > 0, tail[j] > 0) for j in range(S * P)}
    assert {(False, False), (True, False), (True, True)} <= cases and (S == 1 or (False, True) in cases)
    return pre, tail


def test_every_instance_sees_every_listed_count():
    """The cases of ``test_prefix_tail_matches_float64_per_task`` at one width (the counts do not depend on it): every listed prefix
    and tail count occurs, and an empty prefix meets a non-empty tail (S = 2: task P reads prefix task 0)."""
    pre_seen, tail_seen, empty_prefix_with_tail = set(), set(), False
    for S in (1, 2):
        for T in (1, 17, 65):
            pre, tail = _counts(S, T)
            pre_seen |= set(pre)
            tail_seen |= set(tail)
            empty_prefix_with_tail |= any(pre[j % P] == 0 and tail[j] > 0 for j in range(S * P))
    assert pre_seen == set(PRE_COUNTS) and tail_seen == set(TAIL_COUNTS) and empty_prefix_with_tail


def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _poison_rows(pt, counts):
    out, tiles = pt.clone(), pt.shape[1]
    row = torch.arange(32 * tiles, device=pt.device).view(1, tiles, 1, 32, 1)
    out.masked_fill_(row >= _i32(counts).view(-1, 1, 1, 1, 1), float("nan"))
    return out


def _reference(Q, Kp, Vp, Kt, Vt, pre, tail, q_counts, d, dtype):
    """[S P, T, d] in ``dtype``: the formula per task; zeros without a key and in the rows beyond a query count."""
    n_tasks, T = Q.shape[0], Q.shape[1]
    out = torch.zeros(n_tasks, T, d, dtype=dtype)
    for j in range(n_tasks):
        n_p, n_t = pre[j % P], tail[j]
        K = torch.cat([Kp[j % P, :n_p], Kt[j, :n_t]]).to(dtype)
        V = torch.cat([Vp[j % P, :n_p], Vt[j, :n_t]]).to(dtype)
        if n_p + n_t:
            out[j] = torch.softmax(Q[j].to(dtype) @ K.T / math.sqrt(d), -1) @ V
        if q_counts is not None:
            out[j, q_counts[j]:] = 0
    return out


def _random_case(S, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    n = S * P
    Q, Kp, Kt = (torch.randn(b, r, d, generator=g) * 1.5 for b, r in ((n, T), (P, C_PAD), (n, M_TAIL)))
    (Vp,), (Vt,) = MC.scale_per_task(torch.randn(P, C_PAD, d, generator=g)), MC.scale_per_task(torch.randn(n, M_TAIL, d, generator=g))
    return Q, Kp, Vp, Kt, Vt


def _query_counts(n_tasks, T):
    edge = [0, T, min(16, T), min(64, T), max(T - 1, 0), min(17, T)]
    return [edge[j % len(edge)] for j in range(n_tasks)]


def _launch(ops, pre, tail, q_counts, T, d):
    from npf_gwwaveform_amd import functional as FN

    n = len(tail)
    with launch_witness() as wit:
        o = FN.masked_attention_prefix(ops[0], ops[1], ops[2], _i32(pre), ops[3], ops[4], _i32(tail), n, P, C_PAD, M_TAIL, T, d,
                                       1.0 / math.sqrt(d), n_q_valid=None if q_counts is None else _i32(q_counts))
        torch.cuda.synchronize()
    assert wit["npf_masked_attn_fwd_prefix"] == 1 and wit["npf_masked_attn_fwd"] == 0 and wit["npf_masked_attn_fwd_nq"] == 0, wit
    return o


def _check(tag, case, pre, tail, T, d, with_nq):
    from npf_gwwaveform_amd import functional as FN

    Q, Kp, Vp, Kt, Vt = case
    n = len(tail)
    q_counts = _query_counts(n, T) if with_nq else None
    ops = [_pt(x) for x in case]
    clean = _launch(ops, pre, tail, q_counts, T, d)
    got = FN.unpack_pt(clean, T, d)
    r64, r32 = (_reference(*case, pre, tail, q_counts, d, dt) for dt in (torch.float64, torch.float32))
    worst = assert_gated_per_task(got, r64, r32, 1e-5, tag)
    print(f"{tag}: worst err/gate {worst:.3f}")
    got = got.cpu()
    for j in range(n):
        if pre[j % P] + tail[j] == 0:
            assert not got[j].any(), f"{tag} task {j}: no key in either segment"
        if q_counts is not None:
            assert not got[j, q_counts[j]:].any(), f"{tag} task {j}: rows beyond the query count"
    # a second launch gives the same bits; NaN beyond every count (rows and padding features) changes none
    assert torch.equal(_launch(ops, pre, tail, q_counts, T, d), clean), f"{tag}: a second launch gave other bits"
    rows = [[T] * n if q_counts is None else q_counts, pre, pre, tail, tail]
    bad = [_poison_feature_padding(_poison_rows(x, c), d) for x, c in zip(ops, rows)]
    assert all(x.isnan().any() for x in bad[1:])
    poisoned = _launch(bad, pre, tail, q_counts, T, d)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, clean), f"{tag}: NaN beyond the counts changed the result"
    return ops, clean, q_counts


@gpu
@pytest.mark.parametrize("with_nq", (False, True))
@pytest.mark.parametrize("T", (1, 17, 65))
@pytest.mark.parametrize("d", (16, 20, 32, 128, 256))
@pytest.mark.parametrize("S", (1, 2))
def test_prefix_tail_matches_float64_per_task(S, d, T, with_nq):
    """Every width instance (20 between two: its padding features poisoned), counts on every edge of both walks, query sizes inside
    a wave, over one and over the 64-row workgroup; plus agreement with ``masked_attention`` on the concatenated, re-padded keys
    within the same gate."""
    from npf_gwwaveform_amd import functional as FN

    pre, tail = _counts(S, T)
    case = _random_case(S, T, d, seed=7 * d + T + S)
    ops, clean, q_counts = _check(f"S={S} d={d} T={T} nq={with_nq}", case, pre, tail, T, d, with_nq)
    Q, Kp, Vp, Kt, Vt = case
    n = S * P
    Kc, Vc = torch.zeros(n, C_PAD + M_TAIL, d), torch.zeros(n, C_PAD + M_TAIL, d)
    for j in range(n):
        n_p, n_t = pre[j % P], tail[j]
        Kc[j, :n_p + n_t] = torch.cat([Kp[j % P, :n_p], Kt[j, :n_t]])
        Vc[j, :n_p + n_t] = torch.cat([Vp[j % P, :n_p], Vt[j, :n_t]])
    total = [pre[j % P] + tail[j] for j in range(n)]
    one = FN.masked_attention(ops[0], _pt(Kc), _pt(Vc), _i32(total), n, C_PAD + M_TAIL, T, d, 1.0 / math.sqrt(d),
                              n_q_valid=None if q_counts is None else _i32(q_counts))
    r64, r32 = (_reference(*case, pre, tail, q_counts, d, dt) for dt in (torch.float64, torch.float32))
    assert_gated_per_task(FN.unpack_pt(one, T, d), r64, r32, 1e-5, "masked_attention on the concatenation")


@gpu
@pytest.mark.parametrize("with_nq", (False, True))
@pytest.mark.parametrize("d", (16, 20, 32, 128, 256))
def test_empty_tails_give_the_bits_of_masked_attention(d, with_nq):
    """S = 1 and every tail count 0: the block sequence is that of ``npf_masked_attn_fwd`` on the prefix, so are the bits."""
    from npf_gwwaveform_amd import functional as FN

    T = 65
    pre = [33, 70, 0]
    Q, Kp, Vp, Kt, Vt = _random_case(1, T, d, seed=31 + d)
    ops = [_pt(x) for x in (Q, Kp, Vp, Kt, Vt)]
    q_counts = _query_counts(P, T) if with_nq else None
    nq = None if q_counts is None else _i32(q_counts)
    got = _launch(ops, pre, [0] * P, q_counts, T, d)
    want = FN.masked_attention(ops[0], ops[1], ops[2], _i32(pre), P, C_PAD, T, d, 1.0 / math.sqrt(d), n_q_valid=nq)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


def _regime_case(kind, S, T, d):
    """``ascending``: the scores of ``masked_cases`` rise over the prefix AND on across the tail (one ascending row of n_p + n_t keys
    cut at the boundary; a task of a later sample continues the shared prefix with a steeper or equal row), so the running maximum
    moves at the switch of segments.  ``one_key``: one key 30 above the rest sits in
    the first tail row."""
    KB = MC.key_block(d)
    n = S * P
    pre, tail = [33, 70, 32], [17, 40, 32, 16, 15, 1][:n]
    g = torch.Generator().manual_seed(5 + d)
    total = [pre[j % P] + tail[j] for j in range(n)]
    regime = "ascending" if kind == "ascending" else "one_key@edge"
    # (built per task over the concatenated keys; every task of ``masked_cases.build`` shares the direction u and the query scale)
    if kind == "ascending":
        Q, K, V = MC.build(regime, total, C_PAD + M_TAIL, T, d, KB, g)
    else:
        Q, K, V = MC.build("one_key@first", total, C_PAD + M_TAIL, T, d, KB, g)
        for j in range(n):  # move the dominant key from row 0 to the first tail row
            n_p = pre[j % P]
            K[j, [0, n_p]] = K[j, [n_p, 0]]
    for j in range(P, n):  # the samples s > 0 read the prefix of task j % P: their own rows continue THAT prefix
        K[j, :pre[j % P]], V[j, :pre[j % P]] = K[j % P, :pre[j % P]], V[j % P, :pre[j % P]]
    (V,) = MC.scale_per_task(V)
    Kp, Vp = torch.zeros(P, C_PAD, d), torch.zeros(P, C_PAD, d)
    Kt, Vt = torch.zeros(n, M_TAIL, d), torch.zeros(n, M_TAIL, d)
    for j in range(n):
        n_p, n_t = pre[j % P], tail[j]
        if j < P:
            Kp[j, :n_p], Vp[j, :n_p] = K[j, :n_p], V[j, :n_p]
        Kt[j, :n_t], Vt[j, :n_t] = K[j, n_p:n_p + n_t], V[j, n_p:n_p + n_t]
    return (Q, Kp, Vp, Kt, Vt), pre, tail


@gpu
@pytest.mark.parametrize("d", (32, 128, 256))
@pytest.mark.parametrize("kind", ("ascending", "one_key_in_first_tail_row"))
def test_online_rescale_across_the_switch_of_segments(kind, d):
    S, T = 2, 17
    case, pre, tail = _regime_case(kind, S, T, d)
    Q, Kp, Vp, Kt, Vt = case
    for j in range(S * P):  # the regime holds what it claims, in float64, for EVERY task (shared prefix, own tail)
        n_p, n_t = pre[j % P], tail[j]
        s_pre = Q[j].double() @ Kp[j % P, :n_p].double().T / math.sqrt(d)
        s_tail = Q[j].double() @ Kt[j, :n_t].double().T / math.sqrt(d)
        if kind == "ascending":  # every tail score lies above every prefix score: the running maximum moves at the switch
            assert float((s_tail.min(-1).values - s_pre.max(-1).values).min()) > 0, j
        else:
            rest = torch.cat([s_pre, s_tail[:, 1:]], -1).max(-1).values
            assert float((s_tail[:, 0] - rest).min()) > 27, j
    _check(f"{kind} d={d}", case, pre, tail, T, d, with_nq=True)


@gpu
def test_refusals():
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    z = lambda n, r, d: torch.zeros(pt_shape(n, r, d), device=DEV)  # noqa: E731

    def call(d=32, n=6, p=3, grad=None):
        ops = [z(n, 5, d), z(p, C_PAD, d), z(p, C_PAD, d), z(n, M_TAIL, d), z(n, M_TAIL, d)]
        if grad is not None:
            ops[grad].requires_grad_(True)
        return FN.masked_attention_prefix(ops[0], ops[1], ops[2], _i32([1] * p), ops[3], ops[4], _i32([1] * n), n, p, C_PAD, M_TAIL, 5, d, 1.0)

    assert call().shape == pt_shape(6, 5, 32)
    for i in range(5):
        with pytest.raises(RuntimeError, match="inference only"):
            call(grad=i)
    for d in (18, 260):
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            call(d=d)
    with pytest.raises(ValueError, match="multiple of n_prefix_tasks"):
        call(n=7, p=3)
