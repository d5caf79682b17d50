"""The two kernels behind ``model.loo`` / ``Conditioned.loo`` where they can go wrong: ``npf_masked_attn_fwd_loo``
(csrc/masked_kernels.hip) with the excluded key the one that would have dominated its row and the own row at every place relative
to the wave, the 16-row sub-block, the key block and the 64-query workgroup; ``npf_loo_mean`` (csrc/layout_kernels.hip) with a
row that dwarfs its task.  Inputs and references: tests/loo_cases.py, checked on the CPU by tests/test_loo_cases_host.py.

Gates.  Attention: ``assert_gated_per_task`` of tests/test_hip_masked_edges.py at 1e-5 (1e-5 of the task's max|ref| or 4 x the error
of the float64 formula evaluated in fp32 torch); the special row of a regime (the query whose own key dominates its row) by itself
with ``assert_gated`` of tests/test_hip_mha.py, so that it cannot hide under the task's maximum.  ``loo_mean``, per row i:
max_f |got - ref| <= max(1e-6 max_f |ref[i]|, 4 max_f |direct fp32[i] - ref[i]|) -- the project's 1e-6 of tests/test_hip_loo.py taken
per row; the direct fp32 evaluation (sum over the others, one division) errs by a few 1e-7 of the row.  With the fp32 sum the kernel
had, the ``outlier`` cases miss this gate by factors of 10 (x 1e3) to 1e5 (x 1e7) on the outlying row (emulated on the CPU in
tests/test_loo_cases_host.py); the kernel holds the sum in double now.  Every test prints its worst error / gate."""
import math

import pytest
import torch

import loo_cases as LC
from helpers import assert_close, launch_witness
from test_hip_masked_edges import _poison_feature_padding, _poison_rows, assert_gated_per_task
from test_hip_mha import assert_gated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
_REFS = {}


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


def _loo(q_pt, k_pt, v_pt, counts, q_counts, C_pad, d):
    """One launch of the leave-one-out kernel (and of no other attention kernel) -> PT32."""
    from npf_gwwaveform_amd import functional as FN

    with launch_witness() as w:
        o = FN.masked_attention_loo(q_pt, k_pt, v_pt, _i32(counts), len(counts), C_pad, C_pad, d, 1.0 / math.sqrt(d),
                                    n_q_valid=None if q_counts is None else _i32(q_counts))
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_loo"] == 1 and w["npf_masked_attn_fwd"] == 0 and w["npf_masked_attn_fwd_nq"] == 0, w
    return o


def _rows(o_pt, C_pad, d):
    from npf_gwwaveform_amd import functional as FN

    return FN.unpack_pt(o_pt, C_pad, d).cpu()


def _refs(regime, d, name):
    """(r64, r32) of a case and query-count variant, computed once."""
    key = (regime, d, name)
    if key not in _REFS:
        Q, K, V = LC.attn_case(regime, d)
        _REFS[key] = tuple(LC.loo_attention(Q, K, V, LC.COUNTS, LC.Q_COUNTS[name], 1.0 / math.sqrt(d), dt)
                           for dt in (torch.float64, torch.float32))
    return _REFS[key]


# ---- 1. the regimes against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,d", [(r, d) for r in LC.ATTN_REGIMES for d in LC.WIDTHS if LC.regime_runs(r, d)])
def test_loo_regimes_match_float64(regime, d):
    """Every regime with no query count, the key counts as query counts and crossed ones: per task and per special row against
    float64; finite everywhere with exact zeros beyond the query count; a second launch and a launch with NaN in every padding
    row and padding feature of the operands give the same bits; the rows n <= q < n_q equal ``masked_attention``'s within the gate.
    That last comparison is made on the crossed variant, where the issue of this test asks for it.  Without a query count the rows
    2 .. 199 of task 7 (two keys) are such rows too, and there it would measure ``masked_attention``, not this kernel: on ``huge_neg``
    at d = 256 that kernel's rows are 7.04e-6 from float64 on one MI355X against this test's gate of 6.41e-6 (each of the two
    scores is a 256-term fp32 chain that reaches 1600, and two weights 0.4 apart move by a quarter of the difference of two such
    chains' roundings).  The leave-one-out kernel had the same bits and the same miss; it now adds its score contraction in
    segments of 64 features (csrc/masked_kernels.hip) and is gated against float64 on those rows like on every other."""
    from npf_gwwaveform_amd import functional as FN

    C_pad, counts = LC.C_PAD, LC.COUNTS
    Q, K, V = LC.attn_case(regime, d)
    special = LC.special_rows(regime, Q, K, counts, d)
    assert len(special) == (len(counts) if regime in ("ascending", "huge_pos") or regime.startswith("one_key@") else 0)
    clean = [_pt(x) for x in (Q, K, V)]
    plain = _rows(FN.masked_attention(*clean, _i32(counts), len(counts), C_pad, C_pad, d, 1.0 / math.sqrt(d)), C_pad, d)
    for name, qc in LC.Q_COUNTS.items():
        tag = f"{regime} d={d} n_q={name}"
        nq = (C_pad,) * len(counts) if qc is None else qc
        o_pt = _loo(*clean, counts, qc, C_pad, d)
        out = _rows(o_pt, C_pad, d)
        r64, r32 = _refs(regime, d, name)
        assert torch.isfinite(o_pt).all(), f"{tag}: non-finite values"
        worst = assert_gated_per_task(out, r64, r32, TOL, tag)
        worst_row = 0.0
        for b, j in special:
            if j < nq[b]:
                assert_gated(out[b, j], r64[b, j], r32[b, j], TOL, f"{tag} task {b} special row {j}")
                worst_row = max(worst_row, float((out[b, j].double() - r64[b, j]).abs().max()) / LC.row_gate(r64[b, j], r32[b, j], TOL))
        worst_pad = 0.0
        for b, n in enumerate(counts):
            assert (out[b, nq[b]:] == 0).all(), f"{tag} task {b}: rows beyond the query count {nq[b]}"
            if name == "crossed" and nq[b] > n:  # no own key among the valid ones: the plain masked attention of the same operands
                err = float((out[b, n:nq[b]].double() - plain[b, n:nq[b]].double()).abs().max())
                gate = LC.task_gate(r64, r32, b, TOL)
                assert err <= gate, f"{tag} task {b}: rows {n} .. {nq[b] - 1} differ from masked_attention by {err:.3e} > {gate:.3e}"
                worst_pad = max(worst_pad, err / gate)
        print(f"{tag}: worst err/gate  per task {worst:.3f}  special rows {worst_row:.3f}  rows beyond the key count against masked_attention {worst_pad:.3f}")
        assert torch.equal(_loo(*clean, counts, qc, C_pad, d), o_pt), f"{tag}: a second launch gave other bits"
        bad = [_poison_feature_padding(_poison_rows(x, rows), d) for x, rows in zip(clean, (nq, counts, counts))]
        assert all(x.isnan().any() for x in bad)
        assert torch.equal(_loo(*bad, counts, qc, C_pad, d), o_pt), f"{tag}: NaN in the padding of the operands changed the result"


# ---- 2. the exclusion lands on the diagonal at every position ---------------------------------------------------------------------
@pytest.mark.parametrize("d,n", ((256, 200), (128, 128)))
def test_the_exclusion_lands_on_the_diagonal_at_every_position(d, n):
    """V[j] = e_j: the output row is the probability row.  Exact zeros on the diagonal for every valid row of both tasks (every own
    row position across every wave, sub-block, key block and workgroup), rows that sum to 1, the matrix against float64."""
    C_pad = LC.C_PAD
    Q, K, V, counts = LC.one_hot_case(d, n, C_pad, seed=d + n)
    out = _rows(_loo(*[_pt(x) for x in (Q, K, V)], counts, counts, C_pad, d), C_pad, d)
    r64, r32 = (LC.loo_attention(Q, K, V, counts, counts, 1.0 / math.sqrt(d), dt) for dt in (torch.float64, torch.float32))
    for b, m in enumerate(counts):
        diag = out[b, :m, :m].diagonal()
        assert (diag == 0).all(), f"d={d} task {b}: own weight of rows {diag.nonzero().flatten().tolist()[:8]} is not 0"
        total = float((out[b, :m].double().sum(-1) - 1).abs().max())
        assert total <= 1e-5, f"d={d} task {b}: a row's weights sum to 1 +- {total:.3e}"
        assert not out[b, :m, m:].any() and not out[b, m:].any()
    worst = assert_gated_per_task(out, r64, r32, TOL, f"one-hot d={d} n={n}")
    print(f"one-hot d={d} n={n}: worst err/gate {worst:.3f}")


# ---- 3. two points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LC.WIDTHS)
def test_two_points_swap_their_values_bit_for_bit(d):
    """Count 2: the one weight is exp(0) = 1, l = 1, and the product is an fmaf on the vector unit: out[0] == V[1], out[1] == V[0]."""
    C_pad, counts = 40, (2, 2, 2, 2)
    g = torch.Generator().manual_seed(900 + d)
    Q, K, V = (torch.randn(4, C_pad, d, generator=g) for _ in range(3))
    V[:, :2] = LC.pair_case(d, seed=d)
    assert float(V[:, :2].abs().min()) > 1e-30
    for qc in (counts, None):
        out = _rows(_loo(*[_pt(x) for x in (Q, K, V)], counts, qc, C_pad, d), C_pad, d)
        assert torch.equal(out[:, 0], V[:, 1]) and torch.equal(out[:, 1], V[:, 0]), f"d={d}: max|d| = {float((out[:, :2] - V[:, :2].flip(1)).abs().max()):.3e}"
    print(f"two points d={d}: bit for bit")


# ---- 4. ``equal`` under the exclusion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (64, 256))
def test_equal_scores_give_the_mean_of_the_other_values(d):
    Q, K, V = LC.attn_case("equal", d)
    out = _rows(_loo(*[_pt(x) for x in (Q, K, V)], LC.COUNTS, LC.COUNTS, LC.C_PAD, d), LC.C_PAD, d)
    for b, n in enumerate(LC.COUNTS[:2]):
        assert n in (200, 129)
        v = V[b, :n].double()
        want = (v.sum(0, keepdim=True) - v) / (n - 1)
        err = float((out[b, :n].double() - want).abs().max())
        print(f"equal d={d} count {n}: err / (1e-5 max|ref|) = {err / (1e-5 * float(want.abs().max())):.3f}")
        assert_close(out[b, :n], want, tol=1e-5, what=f"equal d={d} count {n}")


# ---- 5. loo_mean ------------------------------------------------------------------------------------------------------------------
def _loo_mean(R_pt, counts, pts, F):
    from npf_gwwaveform_amd import functional as FN

    with launch_witness() as w:
        o = FN.loo_mean(R_pt, _i32(counts), len(counts), pts, F)
        torch.cuda.synchronize()
    assert w["npf_loo_mean"] == 1 and w["npf_masked_mean_fwd"] == 0, w
    return o


@pytest.mark.parametrize("F", LC.MEAN_F)
@pytest.mark.parametrize("regime", LC.MEAN_REGIMES)
def test_loo_mean_rows_match_float64(regime, F):
    """Every row within its own gate; exact zeros beyond the count and for tasks of 0 or 1 points; NaN beyond the counts changes
    nothing; a second launch gives the same bits."""
    from npf_gwwaveform_amd import functional as FN

    counts, pts = LC.MEAN_COUNTS, LC.MEAN_PTS
    R = LC.mean_case(regime, F)
    ref, direct = LC.loo_mean_ref(R, counts, "float64"), LC.loo_mean_ref(R, counts, "direct32")
    R_pt = _pt(R)
    o_pt = _loo_mean(R_pt, counts, pts, F)
    out = FN.unpack_pt(o_pt, pts, F).cpu()
    assert torch.isfinite(o_pt).all()
    ratio = LC.mean_row_ratio(out, ref, direct)
    for b, n in enumerate(counts):
        share = float(((out[b].double() - ref[b]).abs().amax(-1) / ref[b].abs().amax(-1).clamp(min=1e-300)).max())
        print(f"{regime} F={F} task {b} (n={n}): worst err/gate {float(ratio[b].max()):.3f}, worst error {share:.2e} of its row")
        assert (out[b, n:] == 0).all(), f"task {b}: rows beyond the count {n}"
        if n < 2:
            assert (out[b] == 0).all(), f"task {b}: a task of {n} points has no other point"
    bad = (ratio > 1).nonzero().tolist()
    assert not bad, (f"{regime} F={F}: {len(bad)} rows beyond their gate, the first (task, row) = {bad[0]} at "
                     f"{float(ratio[bad[0][0], bad[0][1]]):.3g} x its gate")
    assert torch.equal(_loo_mean(R_pt, counts, pts, F), o_pt), "a second launch gave other bits"
    poisoned = _poison_rows(R_pt, counts)
    assert poisoned.isnan().any()
    assert torch.equal(_loo_mean(poisoned, counts, pts, F), o_pt), "NaN beyond the counts changed the result"


@pytest.mark.parametrize("F", LC.MEAN_F)
def test_loo_mean_of_two_points_swaps_them_bit_for_bit(F):
    """Entries within a factor 1e7 of each other: r0 + r1 is exact in double, so (s - r0) / 1 is r1.  An fp32 sum rounds the smaller
    one away (tests/test_loo_cases_host.py shows it on these inputs): this test is meant to fail on a kernel that sums in fp32."""
    from npf_gwwaveform_amd import functional as FN

    R = torch.randn(4, LC.MEAN_PTS, F, generator=torch.Generator().manual_seed(F))
    R[:, :2] = LC.pair_case(F, seed=F)
    out = FN.unpack_pt(_loo_mean(_pt(R), (2, 2, 2, 2), LC.MEAN_PTS, F), LC.MEAN_PTS, F).cpu()
    assert torch.equal(out[:, 0], R[:, 1]) and torch.equal(out[:, 1], R[:, 0]), f"F={F}: {int((out[:, :2] != R[:, :2].flip(1)).sum())} entries differ"
    assert not out[:, 2:].any()
    print(f"loo_mean two points F={F}: bit for bit")
