"""The weighted and the prefix rule of the masked attention kernels (csrc/masked_kernels.hip: ``MkWeighted`` / ``MkPrefix`` of
``masked_attn_fwd_kernel`` and the ``WGT`` instances of the d_q and d_k / d_v kernels, behind ``npf_masked_attn_fwd_weighted`` / ``_ex``,
``npf_masked_attn_bwd_weighted`` and ``npf_masked_attn_fwd_prefix``) and the weighted mean (csrc/layout_kernels.hip) where an online
softmax with a weight per key goes wrong: the cases of tests/weighted_cases.py (tests/test_weighted_cases_host.py checks them on the
CPU) -- scores and weights that cancel over e^+-56, weights over 2^+-100, the top key removed by every value that removes a key,
staged blocks and whole walks that hold nothing, NaN in every row and weight the kernels promise not to read.

The reference is ``keyweight_reference.weighted_attention_and_grads`` in float64; the gate is ``assert_gated_per_task`` of
tests/test_hip_masked_edges.py (1e-5 of the output, 1e-4 of a gradient, per task, or 4 x the error of the same formula in fp32), also
on ``w * d_w`` (the gradient with respect to log w, formed in float64 from the returned d_w and from both references alike).  The
weighted mean is gated per task at 1e-6 of max|ref_b| (tests/test_hip_keyweight.py's tolerance for this double-precision kernel).
Every case prints ``WE <case> <tensor> err/gate``.

Worst err / gate per tensor and pattern on an MI355X (training pair, with and without query counts, the three shapes):

    pattern    output  dQ     dK     dV     dW     w*dW
    drop_top   0.535   0.132  0.136  0.125  0.190  0.190
    counter    0.456   0.057  0.068  0.093  0.407  0.071
    wide       0.317   0.135  0.087  0.106  0.100  0.242
    holes      0.709   0.250  0.250  0.032  0.280  0.280
    replicates (output): ones 0.339, drop_top 0.375, counter 0.401;  prefix rule (output): 0.532
    weighted mean: wide out 0.045, dR 0.053, dW 0.054;  holes out 0.056, dR 0.048, dW 0.053

Two findings of this suite, both fixed with it:

* With the score contraction of the 256-wide instance as ONE fp32 chain of 64 MFMA steps, four cases of the training pair at d = 256
  missed the gate (drop_top-huge_pos with query counts, output of the task with one query row: max|d| = 3.646e-06 against a gate of
  2.555e-06; counter-descending dW 8.653e+16 / 8.512e+16; holes(a)- and holes(f)-ascending output 3.058e-03 / 2.931e-03 and
  3.510e-03 / 3.267e-03): the running sum of such a chain reaches 16 |s| and every step rounds at that size.  Every rule and both
  backward kernels now add the scores in segments of 64 features (csrc/masked_kernels.hip, MK_SEG); the same four cases are at
  0.213, 0.155, 0.255 and 0.369 of their gates.
* d_w of the weighted mean with the forward pass's fp32 result as the mean missed its gate in 10 of the 16 ``offset`` cases, by up to
  1.4e-2 of max|ref_b| (holes(a), F = 256: max|d| = 4.1e-5 at max|ref_b| = 2.8e-3); the backward kernel sums the mean in double."""
import math

import pytest
import torch

import keyweight_reference as KR
import masked_cases as MC
import weighted_cases as WC
from helpers import launch_witness
from test_hip_masked_edges import assert_gated_per_task

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TENSORS = (("output", 1e-5), ("dQ", 1e-4), ("dK", 1e-4), ("dV", 1e-4), ("dW", 1e-4))
CASE_PARAMS = [pytest.param(c, id=WC.case_id(c)) for c in WC.CASES]


def _i32(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


def _poison_queries(X, q_counts):
    """A copy with NaN in the rows at and beyond the query count (none: the tensor itself)."""
    if q_counts is None:
        return X
    X = X.clone()
    for b, n in enumerate(q_counts):
        X[b, n:] = math.nan
    return X


def _train_pair(Q, K, V, W, dO, counts, q_counts, C_pad, T, d):
    """One ``key_weighted_attention`` forward and backward -> rows (O, dQ, dK, dV, dW) on the device and the PT32 output.  The
    witness must show the training forward and the weighted backward once each and no plain or inference export."""
    from npf_gwwaveform_amd import functional as FN

    leaves = [_pt(x).requires_grad_(True) for x in (Q, K, V)]
    Wd = W.to(DEV).requires_grad_(True)
    with launch_witness() as wit:
        o_pt = FN.key_weighted_attention(*leaves, Wd, _i32(counts), len(counts), C_pad, T, d, 1.0 / math.sqrt(d),
                                         n_q_valid=None if q_counts is None else _i32(q_counts))
        o_pt.backward(_pt(dO))
        torch.cuda.synchronize()
    assert wit["npf_masked_attn_fwd_weighted_ex"] == 1 and wit["npf_masked_attn_bwd_weighted"] == 1, wit
    assert all(wit[k] == 0 for k in ("npf_masked_attn_fwd_weighted", "npf_masked_attn_fwd", "npf_masked_attn_bwd",
                                     "npf_masked_attn_fwd_nq", "npf_masked_attn_bwd_nq")), wit
    pts = (o_pt.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)
    rows = [FN.unpack_pt(t, n, d) for t, n in zip(pts, (T, T, C_pad, C_pad))]
    return rows + [Wd.grad], pts


# ---- a. the training pair ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_training_pair_matches_float64_per_task(case, d, C_pad):
    cs = WC.make(case, d, C_pad)
    Kp, Vp = cs.poisoned()
    scale, T = 1.0 / math.sqrt(d), cs.T
    w64 = cs.finite_weights().double()
    for q_counts in (None, WC.Q_COUNTS):
        tag = f"{WC.case_id(case)} d={d}{'' if q_counts is None else ' nq'}"
        r64, r32 = (KR.weighted_attention_and_grads(cs.Q, cs.K, cs.V, cs.W, cs.dO, cs.counts, scale, dt, q_counts)
                    for dt in (torch.float64, torch.float32))
        got, _ = _train_pair(_poison_queries(cs.Q, q_counts), Kp, Vp, cs.W, _poison_queries(cs.dO, q_counts), cs.counts, q_counts,
                             C_pad, T, d)
        got = [g.detach().cpu() for g in got]
        assert all(torch.isfinite(g).all() for g in got), f"{tag}: NaN / Inf"
        worst = {}
        for i, (what, tol) in enumerate(TENSORS):
            if float(r64[i].abs().max()) == 0:  # (holes (e): no admissible key anywhere -- zeros, asserted below)
                assert not got[i].any(), f"{tag} {what}"
                continue
            worst[what] = assert_gated_per_task(got[i], r64[i], r32[i], tol, f"{tag} {what}")
        if float(r64[4].abs().max()) > 0:
            worst["w*dW"] = assert_gated_per_task(w64 * got[4].double(), w64 * r64[4], w64 * r32[4].double(), 1e-4, f"{tag} w*dW")
        print(f"WE {tag}: err/gate " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        o, dq, dk, dv, dw = got
        assert not dk[~cs.adm].any() and not dv[~cs.adm].any() and not dw[~cs.adm].any(), f"{tag}: inadmissible keys"
        for b in range(len(cs.counts)):
            n_q = T if q_counts is None else q_counts[b]
            assert not o[b, n_q:].any() and not dq[b, n_q:].any(), f"{tag} task {b}: queries beyond the count {n_q}"
            if not cs.adm[b].any():
                assert not o[b].any() and not dq[b].any(), f"{tag} task {b}: no admissible key"
    if case[0] == "drop_top":  # (the emptied task of count 1 was among them)
        assert any(n == 1 and not cs.adm[b].any() for b, n in enumerate(cs.counts))


# ---- b. the same bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_same_bits_across_exports_launches_and_what_is_not_read(case, d, C_pad):
    """O of the training forward is that of ``masked_attention_weighted`` at one replicate; a second forward and backward give the
    same bits (no atomics); finite values in the place of the NaN of the inadmissible rows and of every weight that is not
    admissible (0.0 there) change no bit of any result."""
    from npf_gwwaveform_amd import functional as FN

    cs = WC.make(case, d, C_pad)
    Kp, Vp = cs.poisoned()
    T, B, scale = cs.T, len(cs.counts), 1.0 / math.sqrt(d)
    for q_counts in (None, WC.Q_COUNTS):
        tag = f"{WC.case_id(case)} d={d}{'' if q_counts is None else ' nq'}"
        Q, dO = _poison_queries(cs.Q, q_counts), _poison_queries(cs.dO, q_counts)
        first, pts = _train_pair(Q, Kp, Vp, cs.W, dO, cs.counts, q_counts, C_pad, T, d)
        with launch_witness() as wit:
            plain = FN.masked_attention_weighted(_pt(Q), _pt(Kp), _pt(Vp), cs.W.to(DEV), _i32(cs.counts), B, B, C_pad, T, d, scale,
                                                 n_q_valid=None if q_counts is None else _i32(q_counts))
        assert wit["npf_masked_attn_fwd_weighted"] == 1 and wit["npf_masked_attn_fwd_weighted_ex"] == 0, wit
        assert torch.equal(plain, pts[0]), f"{tag}: O of the training forward is not that of the inference export"
        again, _ = _train_pair(Q, Kp, Vp, cs.W, dO, cs.counts, q_counts, C_pad, T, d)
        clean, _ = _train_pair(Q, cs.K, cs.V, cs.finite_weights(), dO, cs.counts, q_counts, C_pad, T, d)
        for (what, _), a, b, c in zip(TENSORS, first, again, clean):
            assert torch.equal(b, a), f"{tag} {what}: a second launch gave other bits"
            assert torch.equal(c, a), f"{tag} {what}: finite values in the rows and weights that are not read changed the result"


# ---- c. replicates of one stored context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("regime", WC.REPLICATE_REGIMES)
def test_replicates_of_one_context_match_float64(regime, d, C_pad):
    """S = 3 replicates (all ones, ``drop_top``, ``counter``) of B = 4 context tasks in one ``masked_attention_weighted`` call: every
    replicate against float64 per task, and the all-ones replicate bit for bit ``masked_attention`` with the query counts."""
    from npf_gwwaveform_amd import functional as FN

    cs, W = WC.make_replicates(regime, d, C_pad)
    S, B, T, scale = W.shape[0], len(cs.counts), cs.T, 1.0 / math.sqrt(d)
    q_counts = WC.REPLICATE_Q_COUNTS
    K, V = cs.K.clone(), cs.V.clone()
    for b, n in enumerate(cs.counts):  # (the stored context is shared: NaN only in the rows no replicate reads)
        K[b, n:], V[b, n:] = math.nan, math.nan
    q, k, v = _pt(_poison_queries(cs.Q, q_counts)), _pt(K), _pt(V)
    with launch_witness() as wit:
        out = FN.masked_attention_weighted(q, k, v, W.to(DEV), _i32(cs.counts), S * B, B, C_pad, T, d, scale, n_q_valid=_i32(q_counts))
    assert wit["npf_masked_attn_fwd_weighted"] == 1, wit
    rows = FN.unpack_pt(out, T, d).cpu()
    assert torch.isfinite(rows).all()
    zero = torch.zeros_like(cs.dO)
    for s, pattern in enumerate(WC.REPLICATE_PATTERNS):
        r64, r32 = (KR.weighted_attention_and_grads(cs.Q, cs.K, cs.V, W[s], zero, cs.counts, scale, dt, q_counts)[0]
                    for dt in (torch.float64, torch.float32))
        got = rows[s * B:(s + 1) * B]
        worst = assert_gated_per_task(got, r64, r32, 1e-5, f"{regime} d={d} replicate {pattern}")
        print(f"WE replicate {pattern}-{regime} d={d}: err/gate output={worst:.3f}")
        adm = KR.admissible(W[s], cs.counts)
        for b in range(B):
            assert not got[b, q_counts[b]:].any()
            if not adm[b].any():
                assert not got[b].any(), f"replicate {pattern} task {b}: no admissible key"
    ones = FN.masked_attention(q, k, v, _i32(cs.counts), B, C_pad, T, d, scale, n_q_valid=_i32(q_counts))
    assert torch.equal(out[:B], ones), "the all-ones replicate is not masked_attention bit for bit"


# ---- d. the prefix rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C_pad", WC.SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_prefix_and_tail_match_float64_plain_attention(regime, d, C_pad):
    """Every plain regime cut into a shared prefix and an own tail at a point that rotates over the block edges, the ends and the
    top key; two samples per prefix, the second with its tail reversed; both against float64 attention over the task's valid keys
    at the output tolerance, with and without query counts."""
    from npf_gwwaveform_amd import functional as FN

    p = WC.make_prefix(regime, d, C_pad)
    B, T, scale, counts = 8, WC.T, 1.0 / math.sqrt(d), p["counts"]
    Q2 = torch.cat([p["Q"], p["Q"]])
    ones = torch.ones(B, C_pad)
    zero = torch.zeros(B, T, d)
    ops = [_pt(x) for x in (p["k_pre"], p["v_pre"], p["k_tail"], p["v_tail"])]
    for q_counts in (None, WC.Q_COUNTS):
        qc2 = None if q_counts is None else q_counts + q_counts
        r64 = KR.weighted_attention_and_grads(p["Q"], p["K"], p["V"], ones, zero, counts, scale, torch.float64, q_counts)[0]
        with launch_witness() as wit:
            out = FN.masked_attention_prefix(_pt(_poison_queries(Q2, qc2)), ops[0], ops[1], _i32(p["n_prefix"]), ops[2], ops[3],
                                             _i32(p["n_tail"]), 2 * B, B, C_pad, C_pad, T, d, scale,
                                             n_q_valid=None if qc2 is None else _i32(qc2))
        assert wit["npf_masked_attn_fwd_prefix"] == 1, wit
        rows = FN.unpack_pt(out, T, d).cpu()
        assert torch.isfinite(rows).all()
        for s in range(2):
            K32, V32 = p["K"].clone(), p["V"].clone()  # (the fp32 term: the same formula over the keys in the order of the walk)
            for b, n in enumerate(counts):
                K32[b, :n], V32[b, :n] = p["K"][b, p["order"][B * s + b]], p["V"][b, p["order"][B * s + b]]
            r32 = KR.weighted_attention_and_grads(p["Q"], K32, V32, ones, zero, counts, scale, torch.float32, q_counts)[0]
            got = rows[B * s:B * (s + 1)]
            worst = assert_gated_per_task(got, r64, r32, 1e-5, f"prefix {regime} d={d} sample {s}")
            print(f"WE prefix-{regime} d={d}{'' if q_counts is None else ' nq'} sample {s}: err/gate output={worst:.3f}")
            for b, n in enumerate(counts):
                if n == 0:
                    assert p["n_prefix"][b] == 0 and p["n_tail"][B * s + b] == 0 and not got[b].any(), f"task {b}: no key"
                if q_counts is not None:
                    assert not got[b, q_counts[b]:].any()


# ---- e. the weighted mean ------------------------------------------------------------------------------------------------------
def _gated_mean(got, ref, what):
    """Per task: max|got_b - ref_b| <= 1e-6 max|ref_b|, exact zeros where the reference of a task is zero.  Returns the worst ratio."""
    got, worst = got.detach().cpu().double(), 0.0
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    for b in range(ref.shape[0]):
        err, m = float((got[b] - ref[b]).abs().max()), float(ref[b].abs().max())
        if m == 0:
            assert err == 0, f"{what} task {b}: {err:.3e} where the reference is zero"
            continue
        assert err <= 1e-6 * m, f"{what} task {b}: max|d|={err:.3e} > 1e-6 * max|ref_b|={m:.3e}"
        worst = max(worst, err / (1e-6 * m))
    return worst


@pytest.mark.parametrize("F", WC.MEAN_WIDTHS)
@pytest.mark.parametrize("case", [pytest.param(c, id="-".join(x for x in c if x)) for c in WC.MEAN_CASES])
def test_weighted_mean_and_gradients_match_float64_per_task(case, F):
    """``key_weighted_mean`` forward and backward.  The ``offset`` values (1e3 + 1e-3 randn) are where d_w = <d_out, r - out> / W
    needs the task's mean in double: with the forward pass's fp32 result in its place d_w missed this gate by four orders of
    magnitude (tests/test_weighted_cases_host.py has the arithmetic); the backward kernel sums the mean again since."""
    from npf_gwwaveform_amd import functional as FN

    R, W, dOut, counts, adm, dead = WC.make_mean(case, F)
    Rp = R.clone()
    Rp[dead] = math.nan
    for b, n in enumerate(counts):
        Rp[b, n:] = math.nan
    r64 = KR.weighted_mean_and_grads(R, W, dOut, counts, torch.float64)
    Rd, Wd = Rp.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    with launch_witness() as wit:
        out = FN.key_weighted_mean(FN.pack_pt(Rd), Wd, _i32(counts), len(counts), WC.MEAN_PTS, F)[:, :F]
        (out * dOut.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    assert wit["npf_weighted_mean"] == 1 and wit["npf_weighted_mean_bwd"] == 1, wit
    tag = "-".join(x for x in case if x) + f" F={F}"
    worst = {name: _gated_mean(got, ref, f"mean {tag} {name}") for name, got, ref in (("out", out, r64[0]), ("dR", Rd.grad, r64[1]),
                                                                                      ("dW", Wd.grad, r64[2]))}
    print(f"WE mean {tag}: err/gate " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not Rd.grad.cpu()[~adm].any() and not Wd.grad.cpu()[~adm].any(), f"{tag}: inadmissible points"
