"""The masked attention kernels (csrc/masked_kernels.hip: ``npf_masked_attn_fwd`` / ``_bwd`` and the ``_nq`` pair) where the online
softmax, the four tile-width instances and the query / key blocks can go wrong: score regimes placed relative to the counts and
the key blocks (tests/masked_cases.py), widths between two instances, counts on the wave and workgroup edges, NaN in everything
the kernels promise not to read, and two launches that must give the same bits.

The reference is ``_attention_and_grads`` of tests/test_hip_masked.py in float64; the gate is the project's fp32 gate (1e-5 of the
output, 1e-4 of a gradient, or 4 x the error of the same formula evaluated in fp32) taken PER TASK (``assert_gated_per_task``), and
every case gives its tasks magnitudes between 1e-2 and 1e2, so a task cannot hide behind a larger neighbour."""
import math

import pytest
import torch

import masked_cases as MC
from helpers import launch_witness
from test_hip_masked import _attention_and_grads

gpu = pytest.mark.gpu
DEV = "cuda:0"
TENSORS = (("output", 1e-5), ("dQ", 1e-4), ("dK", 1e-4), ("dV", 1e-4))
EXPORTS = ("npf_masked_attn_fwd", "npf_masked_attn_bwd", "npf_masked_attn_fwd_nq", "npf_masked_attn_bwd_nq")


# ---- 0. the per-task gate ------------------------------------------------------------------------------------------------------
def assert_gated_per_task(got, ref64, ref32, tol, what):
    """For every task b: max|got_b - ref_b| <= max(tol * max(max|ref_b|, 1e-3 max|ref|), 4 * max|fp32 evaluation_b - ref_b|).  The
    1e-3 floor only serves tasks whose float64 reference cancels to about 0 (count 1; dQ / dK of one dominant key).  The zeros the
    kernels owe exactly (an empty task, rows beyond a count) are asserted by the caller.  Returns the worst err / gate."""
    got, ref, r32 = (t.detach().cpu().double() for t in (got, ref64, ref32))
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    whole, worst = float(ref.abs().max()), 0.0
    assert whole > 0, what
    for b in range(ref.shape[0]):
        err = float((got[b] - ref[b]).abs().max())
        gate = max(tol * max(float(ref[b].abs().max()), 1e-3 * whole), 4 * float((r32[b] - ref[b]).abs().max()))
        assert err <= gate, f"{what} task {b}: max|d|={err:.3e} > gate {gate:.3e} (max|ref_b|={float(ref[b].abs().max()):.3e})"
        worst = max(worst, err / gate)
    return worst


# ---- launching on PT32 tensors -------------------------------------------------------------------------------------------------
def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


def _i32(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _launch(q_pt, k_pt, v_pt, g_pt, counts, q_counts, C_pad, T, d):
    """One forward and one backward call on PT32 operands -> PT32 (O, dQ, dK, dV).  The witness must show the export pair the call
    meant to run, once each, and none of the other pair."""
    from npf_gwwaveform_amd import functional as FN

    leaves = [x.detach().requires_grad_(True) for x in (q_pt, k_pt, v_pt)]
    with launch_witness() as wit:
        o_pt = FN.masked_attention(*leaves, _i32(counts), len(counts), C_pad, T, d, 1.0 / math.sqrt(d),
                                   n_q_valid=None if q_counts is None else _i32(q_counts))
        o_pt.backward(g_pt)
        torch.cuda.synchronize()
    ran = EXPORTS[:2] if q_counts is None else EXPORTS[2:]
    assert all(wit[k] == (1 if k in ran else 0) for k in EXPORTS), wit
    return (o_pt.detach(),) + tuple(x.grad for x in leaves)


def _rows(pts, T, C_pad, d):
    from npf_gwwaveform_amd import functional as FN

    return [FN.unpack_pt(t, n, d) for t, n in zip(pts, (T, T, C_pad, C_pad))]


def _references(Q, K, V, dO, counts, q_counts, d):
    """(r64, r32) of the batch; with query counts dO carries nothing beyond them and the rows of O / dQ there are zeros."""
    if q_counts is not None:
        dO = dO.clone()
        for b, n in enumerate(q_counts):
            dO[b, n:] = 0
    refs = [_attention_and_grads(Q, K, V, dO, counts, 1.0 / math.sqrt(d), dt) for dt in (torch.float64, torch.float32)]
    if q_counts is not None:
        for r in refs:
            for b, n in enumerate(q_counts):
                r[0][b, n:] = 0
                r[1][b, n:] = 0
    return refs


def _check(tag, Q, K, V, dO, counts, q_counts, C_pad, T, d):
    """Both exports on the case against float64 with the per-task gate and the exact zeros beyond the counts.  The ``_nq`` call gets
    the FULL dO: what lies beyond a query count must not matter.  Returns the PT32 operands and results of both calls."""
    ops = [_pt(x) for x in (Q, K, V, dO)]
    res = {}
    for name, qc in (("plain", None), ("nq", q_counts)):
        res[name] = _launch(*ops, counts, qc, C_pad, T, d)
        got = _rows(res[name], T, C_pad, d)
        r64, r32 = _references(Q, K, V, dO, counts, qc, d)
        worst = [assert_gated_per_task(got[i], r64[i], r32[i], tol, f"{tag} {name} {what}") for i, (what, tol) in enumerate(TENSORS)]
        print(f"{tag} {name}: worst err/gate " + " ".join(f"{what}={w:.3f}" for (what, _), w in zip(TENSORS, worst)))
        o, dq, dk, dv = got
        for b, n in enumerate(counts):
            assert not dk[b, n:].any() and not dv[b, n:].any(), f"{tag} {name} task {b}: d_k / d_v beyond the count {n}"
            if n == 0:
                assert not o[b].any() and not dq[b].any(), f"{tag} {name} task {b}: empty context"
        if qc is not None:
            for b, n in enumerate(qc):
                assert not o[b, n:].any() and not dq[b, n:].any(), f"{tag} nq task {b}: rows beyond the query count {n}"
                if n == 0:
                    assert not dk[b].any() and not dv[b].any(), f"{tag} nq task {b}: d_k / d_v of a task without queries"
    return ops, res


def _random_case(B, C_pad, T, d, seed):
    """Random inputs as tests/test_hip_masked.py draws them, V and dO with the per-task factors."""
    g = torch.Generator().manual_seed(seed)
    Q, K, V = (torch.randn(B, n, d, generator=g) * a for n, a in ((T, 1.5), (C_pad, 1.5), (C_pad, 1.0)))
    V, dO = MC.scale_per_task(V, torch.randn(B, T, d, generator=g))
    return Q, K, V, dO


# ---- 1. score regimes ----------------------------------------------------------------------------------------------------------
REGIME_SHAPES = ((32, 100), (128, 100), (256, 70))  # (d, C_pad): both key-block sizes, at least 3 blocks each
REGIME_T = 70
REGIME_Q_COUNTS = [70, 0, 65, 1, 64, 17, 33, 69]


def _regime_case(regime, d, C_pad):
    KB = MC.key_block(d)
    counts = MC.key_counts(C_pad, KB)
    g = torch.Generator().manual_seed(REGIME_SHAPES.index((d, C_pad)) + 10 * MC.REGIMES.index(regime))
    Q, K, V = MC.build(regime, counts, C_pad, REGIME_T, d, KB, g)
    V, dO = MC.scale_per_task(V, torch.randn(len(counts), REGIME_T, d, generator=g))
    return Q, K, V, dO, counts, KB


@pytest.mark.parametrize("d,C_pad", REGIME_SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_regimes_hold_what_they_claim(regime, d, C_pad):
    """The builder on the CPU in float64, per task over the valid keys (tasks with fewer than two keep what the builder gives): the
    score range or gap of the regime, a finite float64 reference, and for the two ``huge`` regimes that a softmax without the
    running maximum could not pass.  ``huge_neg``: every exp(score) is an fp32 denormal (exp(-99) = 1e-43), so the naive sum has
    lost the normaliser whether the hardware keeps denormals or not; with denormals flushed, as the check is meant, it is 0."""
    Q, K, V, dO, counts, KB = _regime_case(regime, d, C_pad)
    assert sorted(counts)[:2] == [0, 1] and {KB, KB + 1, C_pad - 1, C_pad} <= set(counts) and len(counts) == 8
    for b, n in enumerate(counts):
        if n < 2:
            continue
        S = MC.scores64(Q, K, b, n, d)
        what = f"{regime} d={d} task {b} count {n}"
        if regime in ("ascending", "descending"):
            first, last = (S[:, 0], S[:, -1]) if regime == "ascending" else (S[:, -1], S[:, 0])
            assert float((first + 40).abs().max()) < 1 and float((last - 40).abs().max()) < 1, what
            bmax = torch.stack([S[:, k:k + KB].max(-1).values for k in range(0, n, KB)], -1)
            if regime == "ascending":  # the running maximum moves at every block
                assert (bmax[:, 1:] > bmax[:, :-1]).all(), what
                if n >= 2 * KB:  # (a full block further on: the rescale factor is tiny)
                    assert float((bmax[:, 0] - bmax[:, 1]).max()) < -10, what
            else:  # block 0 holds it, every later block lies below
                assert (bmax[:, 1:] < bmax[:, :1]).all(), what
        elif regime == "huge_pos":
            top = S.max(-1).values
            assert float(top.min()) > 99 and float(top.max()) < 101, what
            assert torch.isinf(torch.exp(S.float())).any(-1).all(), what
        elif regime == "huge_neg":
            assert float(S.min()) >= -101 and float(S.max()) <= -99, what
            naive = torch.exp(S.float())
            assert float(naive.max()) < torch.finfo(torch.float32).tiny, what
            had = torch.set_flush_denormal(True)
            try:
                if had:
                    assert (torch.exp(S.float()).sum(-1) == 0).all(), what
            finally:
                torch.set_flush_denormal(False)
        elif regime.startswith("one_key@"):
            j = MC.one_key_index(regime, n, KB)
            assert j == {"first": 0, "last": n - 1, "edge": max(k for k in range(0, n, KB))}[regime.split("@")[1]]
            rest = torch.cat([S[:, :j], S[:, j + 1:]], -1).max(-1).values
            gap = S[:, j] - rest
            assert float(gap.min()) > 27 and float(gap.max()) < 33, f"{what}: gap {float(gap.min()):.2f} ... {float(gap.max()):.2f}"
        else:  # identical wherever a query is not 0: every score of a query is the same number, the weights are 1 / count
            free = d - MC.EQUAL_FREE
            assert torch.equal(K[b, :n, :free], K[b, :1, :free].expand(n, free)) and not Q[b, :, free:].any(), what
            assert (S == S[:, :1]).all(), what
            P = torch.softmax(S, -1)
            assert float((P - 1.0 / n).abs().max()) < 1e-12, what
    r64 = _attention_and_grads(Q, K, V, dO, counts, 1.0 / math.sqrt(d), torch.float64)
    assert all(torch.isfinite(r).all() for r in r64)
    assert all(float(r.abs().max()) > 0 for r in (r64[0], r64[3]))
    if regime == "equal":  # dQ is a number, not the rounding of a zero (MC.build): fp32 evaluates it to well within the gate
        dq32 = _attention_and_grads(Q, K, V, dO, counts, 1.0 / math.sqrt(d), torch.float32)[1].double()
        for b, n in enumerate(counts):
            if n >= 2:
                assert 4 * float((dq32[b] - r64[1][b]).abs().max()) < 1e-4 * float(r64[1][b].abs().max()), f"equal d={d} task {b}"


@gpu
@pytest.mark.parametrize("d,C_pad", REGIME_SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_score_regimes_match_float64_per_task(regime, d, C_pad):
    Q, K, V, dO, counts, _ = _regime_case(regime, d, C_pad)
    _check(f"{regime} d={d} C_pad={C_pad}", Q, K, V, dO, counts, REGIME_Q_COUNTS, C_pad, REGIME_T, d)


# ---- 2. widths between the instances -------------------------------------------------------------------------------------------
def _feature_padding(pt, d):
    """[B, tiles, 32, pad32(d) - d]: the padding features of a PT32 tensor [B, tiles, Fp / 4, 32, 4]."""
    B, tiles, F4 = pt.shape[:3]
    return pt.permute(0, 1, 3, 2, 4).reshape(B, tiles, 32, 4 * F4)[..., d:]


def _poison_feature_padding(pt, d):
    out = pt.clone()
    feature = 4 * torch.arange(out.shape[2], device=out.device).view(1, 1, -1, 1, 1) + torch.arange(4, device=out.device)
    out.masked_fill_(feature >= d, float("nan"))
    return out


@gpu
@pytest.mark.parametrize("d", (4, 8, 20, 36, 60, 68, 100, 132, 200, 252))
def test_widths_between_the_instances(d):
    """``d`` below its tile width (and pad32(d) below it: 68 -> 96 on the 128 instance, 132 -> 160 and 200 -> 224 on the 256 one):
    float64 per task, the padding features of every PT32 result exact zeros, and NaN in the padding features of the PT32
    operands changing no bit (the ``4 * kc < d`` / ``f < d`` guards)."""
    C_pad, T = 49, 17
    counts, q_counts = [33, 1, 49, 16, 0, 17, 48, 15], [17, 0, 16, 1, 15, 9, 17, 5]
    Q, K, V, dO = _random_case(8, C_pad, T, d, seed=77 + d)
    ops, res = _check(f"width d={d}", Q, K, V, dO, counts, q_counts, C_pad, T, d)
    poisoned = [_poison_feature_padding(x, d) for x in ops]
    assert all(torch.isnan(_feature_padding(x, d)).all() and x.isnan().sum() == _feature_padding(x, d).numel() for x in poisoned)
    for name, qc in (("plain", None), ("nq", q_counts)):
        again = _launch(*poisoned, counts, qc, C_pad, T, d)
        for (what, _), clean, got in zip(TENSORS, res[name], again):
            assert not _feature_padding(clean, d).any(), f"d={d} {name} {what}: padding features of the result"
            assert torch.equal(got, clean), f"d={d} {name} {what}: NaN in the padding features of the operands changed the result"


# ---- 3. block edges of queries and keys ----------------------------------------------------------------------------------------
EDGE_KEY_COUNTS = [33, 1, 49, 16, 0, 17, 47, 15, 32, 48, 31]


@gpu
@pytest.mark.parametrize("d", (32, 256))
@pytest.mark.parametrize("T", (15, 16, 17, 63, 64, 65, 129))
def test_query_and_key_block_edges(T, d):
    """Query sizes and counts inside a 16-query wave, on its edge and on the 64-query workgroup edge; key counts either side of the
    16-key blocks of the d_k / d_v kernel.  On top of the float64 gate, the relation between the two exports bit for bit: the rows
    below the query count are equal, and d_k / d_v are equal when dO is zero beyond it."""
    C_pad = 49
    q_counts = [min(n, T) for n in (T, 0, 65, 1, 64, 17, 63, T - 1, 16, 15, T // 2)]
    Q, K, V, dO = _random_case(11, C_pad, T, d, seed=1000 * d + T)
    ops, res = _check(f"edges T={T} d={d}", Q, K, V, dO, EDGE_KEY_COUNTS, q_counts, C_pad, T, d)
    dO0 = dO.clone()
    for b, n in enumerate(q_counts):
        dO0[b, n:] = 0
    cut = _launch(*ops[:3], _pt(dO0), EDGE_KEY_COUNTS, None, C_pad, T, d)
    o0, dq0 = _rows(res["plain"], T, C_pad, d)[:2]
    o1, dq1 = _rows(res["nq"], T, C_pad, d)[:2]
    for b, n in enumerate(q_counts):
        assert torch.equal(o1[b, :n], o0[b, :n]) and torch.equal(dq1[b, :n], dq0[b, :n]), f"task {b}: rows below the query count {n}"
    assert torch.equal(res["nq"][2], cut[2]) and torch.equal(res["nq"][3], cut[3])
    assert float(cut[2].abs().max()) > 0 and float(cut[3].abs().max()) > 0  # (not two tensors of zeros)


# ---- 4. NaN in the padding rows; two launches, the same bits -------------------------------------------------------------------
def _poison_rows(pt, counts):
    """A copy of a PT32 tensor [B, tiles, F / 4, 32, 4] with NaN in every row at and beyond the task's count, tile padding included."""
    out, tiles = pt.clone(), pt.shape[1]
    row = torch.arange(32 * tiles, device=pt.device).view(1, tiles, 1, 32, 1)
    out.masked_fill_(row >= _i32(counts).view(-1, 1, 1, 1, 1), float("nan"))
    return out


@gpu
@pytest.mark.parametrize("d,C_pad,T", ((64, 49, 70), (256, 49, 17)))
def test_padding_rows_hold_nan_and_two_launches_agree(d, C_pad, T):
    """K / V rows at and beyond the key count (the tile rows beyond ``C_pad`` too), Q / dO tile rows beyond ``T`` and, with query
    counts, beyond the query count hold NaN: O, dQ, dK and dV keep every bit, on both exports.  And the clean call run a second
    time gives the same bits (no atomics: the result does not depend on the launch)."""
    counts = [33, 1, 49, 16, 0, 17, 48, 15]
    q_counts = [min(n, T) for n in (T, 0, 65, 1, 64, 17, 33, T - 1)]
    ops = [_pt(x) for x in _random_case(8, C_pad, T, d, seed=4 * d + T)]
    for name, qc in (("plain", None), ("nq", q_counts)):
        clean = _launch(*ops, counts, qc, C_pad, T, d)
        assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in clean)
        again = _launch(*ops, counts, qc, C_pad, T, d)
        q_rows = [T] * len(counts) if qc is None else qc
        bad = [_poison_rows(x, n) for x, n in zip(ops, (q_rows, counts, counts, q_rows))]
        assert all(x.isnan().any() for x in bad)
        poisoned = _launch(*bad, counts, qc, C_pad, T, d)
        for (what, _), a, b, c in zip(TENSORS, clean, again, poisoned):
            assert torch.equal(b, a), f"d={d} {name} {what}: a second launch gave other bits"
            assert torch.equal(c, a), f"d={d} {name} {what}: NaN beyond the counts changed the result"
