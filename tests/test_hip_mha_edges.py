"""The fused multihead attention kernel (csrc/mha_kernel.hip: ``npf_mha_fwd`` / ``npf_mha_bwd``) where its softmax, its 16-key
blocks, its backward instances (NBLK = 4, 8, 16: 64 / 65 and 128 / 129 keys) and its query walk (16 per wave, 64 per round, 256 per
forward workgroup) can go wrong: random inputs on every block edge, score regimes placed relative to the key blocks
(tests/mha_cases.py), NaN in everything the kernel promises not to read, NaN in one head that must not reach another, NaN in every
output element the kernel does not own, the log-sum-exp it saves, and two launches that must give the same bits.

The reference is ``attention_and_grads`` of tests/test_hip_mha.py in float64; the gate is the project's fp32 gate (1e-5 of the output,
1e-4 of a gradient, or 4 x the error of the same formula evaluated in fp32) taken PER (TASK, HEAD) (``assert_gated_per_task`` of
tests/test_hip_masked_edges.py on the tensors split to [B * H, n, D]), and V / dO of neighbouring heads differ by up to 1e4, so a
head cannot hide behind a larger neighbour.

Recorded on an MI355X (worst err / gate over the (task, head)s and the shapes, as the tests print it):

    case           D    output      dQ      dK      dV     lse
    random C=1     16    0.000   0.000   0.000   0.002           (dQ / dK: residue / ``single_key_bounds``; the residue is 0)
    random         16    0.088   0.019   0.015   0.008
    random C=1     32    0.000   0.000   0.000   0.001
    random         32    0.106   0.016   0.015   0.010
    ascending      16    0.278   0.050   0.031   0.047   0.018
    ascending      32    0.320   0.215   0.139   0.033   0.021
    descending     16    0.289   0.086   0.057   0.046   0.019
    descending     32    0.265   0.219   0.087   0.034   0.025
    huge_pos       16    0.288   0.102   0.101   0.190   0.010
    huge_pos       32    0.286   0.243   0.226   0.148   0.012
    huge_neg       16    0.278   0.068   0.113   0.169   0.006
    huge_neg       32    0.275   0.251   0.125   0.161   0.008
    one_key@first  16    0.000   0.000   0.000   0.002   0.018
    one_key@first  32    0.000   0.000   0.000   0.009   0.030
    one_key@last   16    0.000   0.000   0.000   0.002   0.018
    one_key@last   32    0.000   0.000   0.000   0.008   0.026
    one_key@edge   16    0.000   0.000   0.000   0.002   0.022
    one_key@edge   32    0.000   0.000   0.000   0.009   0.031
    equal          16    0.054   0.007   0.005   0.007   0.012
    equal          32    0.047   0.010   0.003   0.004   0.015

What ``one_key@*`` showed.  With one dominant key the weights are one-hot to exp(-30) = 1e-13 and the float64 dQ / dK cancel to 1e-10,
so the gate is its fp32 branch alone: 4 x the rounding residue of dO.V - dO.O that the fp32 torch formula keeps.  The kernel as it
was summed dO.V on the matrix unit and D = dO.O in an FMA chain with two lane exchanges, kept a residue of its own there (1e-08 of
the terms before they cancel) and missed the gate on dK of task 1 head 1 in two cases: ``one_key@first-16-129`` with max|d| =
7.995e-07 against 7.787e-07 and ``one_key@edge-16-256`` with 1.715e-06 against 1.532e-06; over the other 25 ``one_key`` cases the
dK ratio lay between 0.26 and 0.80 and the dQ ratio between 0.25 and 0.5.  ``mha_bwd_kernel`` now takes D from the same
instruction sequence as dO.V (the diagonal of O dO^T), the two sides round alike, and where O is one key's V their difference is
exactly 0: the zeros in the table."""
import pytest
import torch

import masked_cases as MC
import mha_cases as HC
from helpers import launch_witness
from test_hip_masked_edges import _feature_padding, _poison_feature_padding, _poison_rows, assert_gated_per_task

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


# ---- launching on PT32 tensors -------------------------------------------------------------------------------------------------
def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


def _launch(q_pt, k_pt, v_pt, g_pt, C, T, H, D):
    """One forward and one backward through ``functional.mha`` on PT32 operands -> PT32 (O, dQ, dK, dV); one call of each export
    and of nothing else."""
    from npf_gwwaveform_amd import functional as FN

    leaves = [x.detach().requires_grad_(True) for x in (q_pt, k_pt, v_pt)]
    with launch_witness() as wit:
        o_pt = FN.mha(*leaves, q_pt.shape[0], C, T, H, D)
        o_pt.backward(g_pt)
        torch.cuda.synchronize()
    assert wit["npf_mha_fwd"] == 1 and wit["npf_mha_bwd"] == 1 and sum(wit.calls.values()) == 2, wit
    return (o_pt.detach(),) + tuple(x.grad for x in leaves)


def _rows(pts, C, T, F):
    from npf_gwwaveform_amd import functional as FN

    return [FN.unpack_pt(t, n, F) for t, n in zip(pts, (T, T, C, C))]


def _row_padding(pt, n):
    """[B, 32 tiles - n, Fp]: the tile rows of a PT32 tensor [B, tiles, Fp / 4, 32, 4] beyond its ``n`` points."""
    B, tiles, F4 = pt.shape[:3]
    return pt.permute(0, 1, 3, 2, 4).reshape(B, 32 * tiles, 4 * F4)[:, n:]


def _owned(pt, n, F):
    """bool, the shape of ``pt``: the elements of a real point (row < n) and a real feature (< F)."""
    tiles, F4 = pt.shape[1:3]
    row = 32 * torch.arange(tiles, device=pt.device).view(1, tiles, 1, 1, 1) + torch.arange(32, device=pt.device).view(1, 1, 1, 32, 1)
    feature = 4 * torch.arange(F4, device=pt.device).view(1, 1, F4, 1, 1) + torch.arange(4, device=pt.device)
    return ((row < n) & (feature < F)).expand_as(pt)


def _check(tag, Q, K, V, dO, H):
    """``functional.mha`` on the case against float64 under the per-(task, head) gate (C == 1: dQ / dK under
    ``mha_cases.single_key_bounds``), and exact zeros in the padding of every PT32 result.  Returns the PT32 operands and results."""
    (B, T, F), C, D = Q.shape, K.shape[1], Q.shape[2] // H
    ops = [_pt(x) for x in (Q, K, V, dO)]
    res = _launch(*ops, C, T, H, D)
    got = _rows(res, C, T, F)
    r64, r32 = HC.references(Q, K, V, dO, H)
    worst = []
    for i, (what, tol) in enumerate(HC.TENSORS):
        if C == 1 and what in ("dQ", "dK"):
            bound = HC.single_key_bounds(Q, K, V, dO, H)[i - 1]
            assert torch.isfinite(got[i]).all(), f"{tag} {what}"
            err = HC.split_heads(got[i].cpu().double(), H).abs().amax((-1, -2))
            assert (err <= bound).all(), f"{tag} {what}: residue {err.tolist()} > {bound.tolist()}"
            worst.append(float((err / bound).max()))
        else:
            worst.append(assert_gated_per_task(HC.split_heads(got[i].cpu(), H), HC.split_heads(r64[i], H), HC.split_heads(r32[i], H),
                                               tol, f"{tag} {what}"))
    print(f"{tag}: worst err/gate " + " ".join(f"{what}={w:.3f}" for (what, _), w in zip(HC.TENSORS, worst)))
    for (what, _), pt, n in zip(HC.TENSORS, res, (T, T, C, C)):
        assert not _feature_padding(pt, F).any(), f"{tag} {what}: padding features of the result"
        assert not _row_padding(pt, n).any(), f"{tag} {what}: tile rows beyond {n}"
    return ops, res, worst


# ---- a. block edges, random inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,C,T", HC.RANDOM_CASES)
def test_block_edges_match_float64_per_head(D, H, C, T):
    """Key counts either side of the 16-key blocks and of the backward instances, query counts either side of the wave, the round
    and the forward workgroup, 1 to 8 heads (F = 16: half a feature chunk of a tile) and both allocation paths of ``_MhaFn``
    ((C, T) = (64, 64) with F % 32 == 0: ``torch.empty``, everything is written by the kernel)."""
    from npf_gwwaveform_amd import functional as FN

    assert FN.mha_usable(D, D, C)
    Q, K, V, dO = HC.random_case(D, H, C, T)
    _check(f"random D={D} H={H} C={C} T={T}", Q, K, V, dO, H)


# ---- b. score regimes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,C", HC.REGIME_SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_score_regimes_match_float64_per_head(regime, D, C):
    """What each regime holds is asserted on the CPU by tests/test_mha_cases_host.py.  ``one_key@first-16-129`` and
    ``one_key@edge-16-256`` are the cases that missed the gate on dK before D = rowsum(dO O) was summed in the order of dO V^T
    (the module docstring)."""
    Q, K, V, dO = HC.regime_case(regime, D, C)
    _check(f"{regime} D={D} C={C}", Q, K, V, dO, HC.REGIME_H)


# ---- c. NaN where the kernel must not read; two launches -----------------------------------------------------------------------
@pytest.mark.parametrize("D,H,C,T", ((16, 3, 37, 70), (32, 3, 17, 33), (16, 1, 129, 17)))
def test_padding_holds_nan_and_two_launches_agree(D, H, C, T):
    """The tile rows beyond T of Q / dO and beyond C of K / V and the padding features of all four hold NaN (the ``key < C``,
    ``live`` and ``lj`` guards, the head's feature slice): O, dQ, dK, dV keep every bit.  And the clean call a second time gives the
    same bits (no atomics: the reduction over the four waves has a fixed order)."""
    B, F = HC.RANDOM_B, D * H
    ops = [_pt(x) for x in HC.random_case(D, H, C, T)]
    clean = _launch(*ops, C, T, H, D)
    assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in clean)
    again = _launch(*ops, C, T, H, D)
    bad = [_poison_feature_padding(_poison_rows(x, [n] * B), F) for x, n in zip(ops, (T, C, C, T))]
    for x, n in zip(bad, (T, C, C, T)):
        owned = _owned(x, n, F)
        assert x.isnan().any() and x[~owned].isnan().all() and torch.isfinite(x[owned]).all()
        assert int(x.isnan().sum()) == x.numel() - B * n * F
    poisoned = _launch(*bad, C, T, H, D)
    for (what, _), a, b, c in zip(HC.TENSORS, clean, again, poisoned):
        assert torch.equal(b, a), f"{what}: a second launch gave other bits"
        assert torch.isfinite(c).all() and torch.equal(c, a), f"{what}: NaN in the padding of the operands changed the result"


# ---- d. heads and tasks do not leak --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,C,T", ((16, 3, 37, 70), (32, 3, 65, 17)))
def test_a_poisoned_head_stays_alone(D, H, C, T):
    """NaN in every feature of head 1 of task 0 (Q, K, V and dO): every other (task, head) of O, dQ, dK, dV keeps its bits (a head's
    LDS rows are D + 1 floats apart, the workgroup reuses ``Ks`` as its reduction buffer), and the head's own output is NaN."""
    F = D * H
    case = HC.random_case(D, H, C, T)
    clean = _rows(_launch(*[_pt(x) for x in case], C, T, H, D), C, T, F)
    bad = [x.clone() for x in case]
    for x in bad:
        x[0, :, D:2 * D] = NAN
    got = _rows(_launch(*[_pt(x) for x in bad], C, T, H, D), C, T, F)
    for (what, _), a, b in zip(HC.TENSORS, clean, got):
        a, b = HC.split_heads(a, H), HC.split_heads(b, H)
        for bh in range(a.shape[0]):
            if bh != 1:
                assert torch.equal(b[bh], a[bh]), f"{what}: NaN in head 1 of task 0 reached task {bh // H} head {bh % H}"
    assert HC.split_heads(got[0], H)[1].isnan().all()  # (the poison was where the kernel reads)


# ---- e, f. the C ABI: exact writes, the log-sum-exp ----------------------------------------------------------------------------
def _direct(ops, C, T, H, D):
    """``npf_mha_fwd`` with an ``lse`` buffer, then ``npf_mha_bwd``, into buffers full of NaN -> (out, d_q, d_k, d_v, lse)."""
    from npf_gwwaveform_amd import _lib as L

    q, k, v, g = (x.contiguous() for x in ops)
    B, F = q.shape[0], D * H
    out, d_q, d_k, d_v = (torch.full_like(x, NAN) for x in (q, q, k, v))
    lse = torch.full((B, H, T), NAN, dtype=torch.float32, device=q.device)
    lib = L.load()
    assert lib.npf_mha_fwd(L.ptr(q), L.ptr(k), L.ptr(v), B, H, C, T, F, L.ptr(out), L.ptr(lse), L.stream_ptr()) == 0
    assert lib.npf_mha_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(g), L.ptr(lse), B, H, C, T, F, L.ptr(d_q), L.ptr(d_k),
                           L.ptr(d_v), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    return out, d_q, d_k, d_v, lse


@pytest.mark.parametrize("D,H,C,T", ((16, 3, 37, 70), (16, 8, 64, 64), (32, 1, 17, 33)))
def test_the_kernel_writes_exactly_its_own_elements(D, H, C, T):
    """What ``_MhaFn`` rests its choice between ``torch.zeros`` and ``torch.empty`` on: into buffers full of NaN the kernel writes
    every element of a live row and a real feature -- the bits ``functional.mha`` returns -- and no other element."""
    F = D * H
    ops = [_pt(x) for x in HC.random_case(D, H, C, T)]
    want = _launch(*ops, C, T, H, D)
    *got, lse = _direct(ops, C, T, H, D)
    assert torch.isfinite(lse).all()
    for (what, _), w, x, n in zip(HC.TENSORS, want, got, (T, T, C, C)):
        owned = _owned(x, n, F)
        assert int(owned.sum()) == x.shape[0] * n * F
        assert torch.isfinite(x[owned]).all() and torch.equal(x[owned], w[owned]), f"{what}: the elements the kernel owns"
        assert x[~owned].isnan().all(), f"{what}: {int((~x[~owned].isnan()).sum())} elements written outside the live rows / features"


@pytest.mark.parametrize("D,C", HC.REGIME_SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_lse_matches_float64_per_head(regime, D, C):
    """Per (task, head): max|lse - ref| <= max(1e-5 max(1, max|ref|), 4 max|fp32 logsumexp - ref|) -- the project's gate; the
    max(1, .) because a logarithm passes through 0."""
    H = HC.REGIME_H
    Q, K, V, dO = HC.regime_case(regime, D, C)
    lse = _direct([_pt(x) for x in (Q, K, V, dO)], C, HC.REGIME_T, H, D)[-1].cpu().double()
    l64, l32 = HC.lse_references(Q, K, H)
    assert lse.shape == l64.shape and torch.isfinite(lse).all()
    err, e32, top = ((x.abs().amax(-1)) for x in (lse - l64, l32.double() - l64, l64))  # [B, H]
    gate = torch.maximum(1e-5 * top.clamp(min=1.0), 4 * e32)
    print(f"{regime} D={D} C={C}: lse worst err/gate {float((err / gate).max()):.3f} (max|ref| {float(top.max()):.1f})")
    assert (err <= gate).all(), f"lse: err {err.tolist()} > gate {gate.tolist()}"
