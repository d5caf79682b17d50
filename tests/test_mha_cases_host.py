"""The inputs of tests/test_hip_mha_edges.py on the CPU: every regime of tests/mha_cases.py holds per (task, head) what it claims
(float64, relative to the 16-key blocks of csrc/mha_kernel.hip), the references are finite and not zeros, and the random cases are
well conditioned: on them the tolerance branch of the per-(task, head) gate governs, so passing means 1e-5 / 1e-4 of the head."""
import pytest
import torch

import masked_cases as MC
import mha_cases as HC


def test_heads_split_and_merge():
    x = torch.arange(2 * 5 * 12, dtype=torch.float32).view(2, 5, 12)
    s = HC.split_heads(x, 3)
    assert s.shape == (6, 5, 4) and torch.equal(HC.merge_heads(s, 3), x)
    for b in range(2):
        for h in range(3):
            assert torch.equal(s[b * 3 + h], x[b, :, 4 * h:4 * h + 4])


def test_the_shape_families_cross_every_edge():
    """Both sides of every 16-key block edge the backward instances switch at (64 / 65 and 128 / 129 keys; NBLK = 4, 8, 16), of the
    16-query wave, the 64-query round and the 256-query workgroup, one key and one query, and both allocation paths of ``_MhaFn``."""
    for D, top in ((16, 256), (32, 128)):
        keys = {C for d, H, C, T in HC.RANDOM_CASES if d == D and T == 17}
        assert {1, 15, 16, 17, 64, 65, top - 1, top} <= keys and max(keys) == top
        assert {T for d, H, C, T in HC.RANDOM_CASES if d == D and C == 65} >= {1, 15, 16, 17, 63, 64, 65, 255, 256, 257}
    assert {128, 129} <= {C for d, H, C, T in HC.RANDOM_CASES if d == 16}
    whole = [(D, H, C, T) for D, H, C, T in HC.RANDOM_CASES if (D * H) % 32 == 0 and C % 32 == 0 and T % 32 == 0]
    assert {(16, 2, 64, 64), (16, 8, 64, 64), (32, 1, 64, 64), (32, 4, 64, 64)} == set(whole)
    assert (16, 1, 64, 64) in HC.RANDOM_CASES and len(set(HC.RANDOM_CASES)) == len(HC.RANDOM_CASES)
    assert all(C <= (256 if D == 16 else 128) and T <= 257 and H <= 8 for D, H, C, T in HC.RANDOM_CASES)
    assert HC.REGIME_B * HC.REGIME_H > len(MC.FACTORS)  # (every factor occurs, neighbouring heads 1e4 apart)


@pytest.mark.parametrize("D,C", HC.REGIME_SHAPES)
@pytest.mark.parametrize("regime", MC.REGIMES)
def test_regimes_hold_what_they_claim_per_head(regime, D, C):
    B, H, T = HC.REGIME_B, HC.REGIME_H, HC.REGIME_T
    Q, K, V, dO = HC.regime_case(regime, D, C)
    assert Q.shape == dO.shape == (B, T, H * D) and K.shape == V.shape == (B, C, H * D) and Q.dtype == torch.float32
    S_all = HC.scores(Q, K, H)
    S_order = HC.scores_in_order(Q, K, H) if regime == "equal" else None
    for bh in range(B * H):
        S = S_all[bh]
        what = f"{regime} D={D} C={C} task {bh // H} head {bh % H}"
        bmax = torch.stack([S[:, k:k + HC.KB].max(-1).values for k in range(0, C, HC.KB)], -1)
        if regime == "ascending":  # the running maximum moves at every block
            assert (bmax[:, 1:] > bmax[:, :-1]).all(), what
            assert float((S[:, 0] + 40).abs().max()) < 1 and float((S[:, -1] - 40).abs().max()) < 1, what
        elif regime == "descending":  # block 0 holds it, every later block lies below
            assert (bmax[:, 1:] < bmax[:, :1]).all(), what
            assert float((S[:, 0] - 40).abs().max()) < 1 and float((S[:, -1] + 40).abs().max()) < 1, what
        elif regime == "huge_pos":
            top = S.max(-1).values
            assert float(top.min()) > 99 and float(top.max()) < 101, what
            assert torch.isinf(torch.exp(S.float())).any(-1).all(), what
        elif regime == "huge_neg":
            assert float(S.min()) >= -101 and float(S.max()) <= -99, what
        elif regime.startswith("one_key@"):
            j = MC.one_key_index(regime, C, HC.KB)
            assert j == {"first": 0, "last": C - 1, "edge": (C - 1) // 16 * 16}[regime.split("@")[1]]
            gap = S[:, j] - torch.cat([S[:, :j], S[:, j + 1:]], -1).max(-1).values
            assert float(gap.min()) > 27 and float(gap.max()) < 33, f"{what}: gap {float(gap.min()):.2f} ... {float(gap.max()):.2f}"
        else:  # identical wherever a query is not 0: the weights are 1 / C
            free = D - MC.EQUAL_FREE
            k, q = HC.split_heads(K, H)[bh], HC.split_heads(Q, H)[bh]
            assert torch.equal(k[:, :free], k[:1, :free].expand(C, free)) and not q[:, free:].any(), what
            assert (S_order[bh] == S_order[bh, :, :1]).all(), what
            assert float((torch.softmax(S_all[bh], -1) - 1.0 / C).abs().max()) < 1e-12, what
    r64, r32 = HC.references(Q, K, V, dO, H)
    l64, l32 = HC.lse_references(Q, K, H)
    assert all(torch.isfinite(r).all() for r in r64) and torch.isfinite(l64).all() and l64.shape == (B, H, T)
    for bh in range(B * H):  # O and dV of every head are numbers
        assert all(float(HC.split_heads(r, H)[bh].abs().max()) > 0 for r in (r64[0], r64[3]))
    # the heads of one task carry magnitudes 1e4 apart
    top = HC.split_heads(r64[0], H).abs().amax((-1, -2))
    assert float(top.max() / top.min()) > 1e3


@pytest.mark.parametrize("D", (16, 32))
def test_which_branch_governs_per_regime(D):
    """For the record (printed; the table in the docstring of tests/mha_cases.py): the regime cases may be ill-conditioned in the
    rounding of the inputs, as tests/test_hip_masked_edges.py accepts -- there the fp32 branch of the gate governs."""
    for regime in MC.REGIMES:
        worst = [0.0] * 4
        for d, C in HC.REGIME_SHAPES:
            if d != D:
                continue
            Q, K, V, dO = HC.regime_case(regime, D, C)
            r64, r32 = HC.references(Q, K, V, dO, HC.REGIME_H)
            for i, (_, tol) in enumerate(HC.TENSORS):
                worst[i] = max(worst[i], float(HC.branch_ratio(r64[i], r32[i], tol, HC.REGIME_H).max()))
        print(f"    {regime:<14} {D:<3} " + " ".join(f"{w:7.3g}" for w in worst))


@pytest.mark.parametrize("D,H,C,T", HC.RANDOM_CASES)
def test_random_cases_are_not_ill_conditioned(D, H, C, T):
    """On the references alone the tolerance branch of the gate governs every (task, head) of every tensor: 4 max|fp32 - f64| <
    tol max(max|ref_b|, 1e-3 max|ref|).  dQ / dK at C == 1 are exact zeros in float64 and have the bound of
    ``single_key_bounds`` instead, which the fp32 formula has to meet with the 4 x to spare."""
    Q, K, V, dO = HC.random_case(D, H, C, T)
    assert Q.shape == dO.shape == (HC.RANDOM_B, T, H * D) and K.shape == V.shape == (HC.RANDOM_B, C, H * D)
    r64, r32 = HC.references(Q, K, V, dO, H)
    assert all(torch.isfinite(r).all() for r in r64)
    worst = {}
    for i, (what, tol) in enumerate(HC.TENSORS):
        if C == 1 and what in ("dQ", "dK"):
            bound = HC.single_key_bounds(Q, K, V, dO, H)[i - 1]
            zero = HC.split_heads(r64[i], H).abs().amax((-1, -2))  # (the float64 formula leaves its own residue of 0: 1e-12)
            assert (bound > 0).all() and (zero < 1e-9 * bound).all(), what
            err = HC.split_heads(r32[i].double(), H).abs().amax((-1, -2))
            assert (4 * err < bound).all(), f"{what}: fp32 residue {err.tolist()} against {bound.tolist()}"
            worst[what] = float((4 * err / bound).max())
            continue
        ratio = HC.branch_ratio(r64[i], r32[i], tol, H)
        assert float(ratio.max()) < 1, f"{what}: the fp32 branch governs, ratios {ratio.tolist()}"
        worst[what] = float(ratio.max())
    print(f"D={D} H={H} C={C} T={T}: fp32 branch / tolerance branch " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
