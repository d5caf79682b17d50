"""CPU checks of tests/wgrad_cases.py: every builder holds the claim the GPU tests (tests/test_hip_wgrad_edges.py) lean on, and
the gates of those tests are met by a plain float32 evaluation in an order no kernel uses -- printed, so that the room is shown."""
import pytest
import torch

import wgrad_cases as WC

SHAPES = ((2, 45, 100, 36), (3, 70, 64, 33), (5, 31, 40, 130), (1, 1, 1, 3), (2, 45, 1, 255))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("shape", SHAPES + ((9, 288, 32, 32), (57, 288, 32, 32)))
def test_int_operands_are_small_integers_with_distinct_fingerprints(shape):
    n_tasks, pts, N, K = shape
    dz, a = WC.int_operands(n_tasks, pts, N, K, _gen(1))
    for t in (dz, a):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= WC.FP_RANGE
        assert torch.equal(WC.bf16_round(t), t)  # exact in bf16, so the three x6 terms are (x, 0, 0)
    feat, val = WC.fingerprints(n_tasks, pts, N)
    flat = dz.view(-1, N)
    idx = torch.arange(n_tasks * pts)
    assert torch.equal(flat[idx, feat], val.float())
    assert bool((a.view(-1, K)[idx, (idx // WC.FP_RANGE) % K] == 1).all())
    # (feature, value) is distinct over any 255 * N consecutive points
    span = min(n_tasks * pts, WC.FP_RANGE * N)
    for i0 in {0, n_tasks * pts - span}:
        keys = feat[i0:i0 + span] * 1000 + val[i0:i0 + span]
        assert keys.unique().numel() == span
    # everything outside the fingerprints stays inside [-8, 8]
    rest = flat.clone()
    rest[idx, feat] = 0
    assert float(rest.abs().max()) <= 8
    # the exactness bounds the builder asserts
    assert float(WC.mag_shared(dz, a).max()) < WC.EXACT_LIMIT and float(WC.mag_db(dz).max()) < WC.EXACT_LIMIT


@pytest.mark.parametrize("shape", SHAPES)
def test_int_contraction_is_exact_in_float32_in_any_order(shape):
    n_tasks, pts, N, K = shape
    dz, a = WC.int_operands(n_tasks, pts, N, K, _gen(2))
    ref, ref_b = WC.ref_shared(dz, a), WC.ref_db(dz)
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    for seed, chunk in ((3, 5), (4, 1), (5, 32)):
        dW, db = WC.contract_f32_shuffled(dz, a, _gen(seed), chunk)
        assert torch.equal(dW, ref.float()) and torch.equal(db, ref_b.float())
    # and with the operands rounded to bf16 first (the bf16 variants): nothing is lost
    dW, db = WC.contract_f32_shuffled(WC.bf16_round(dz), WC.bf16_round(a), _gen(6))
    assert torch.equal(dW, ref.float()) and torch.equal(db, ref_b.float())
    per = WC.ref_per_task(dz, a)
    assert torch.equal(per.sum(0), ref) and per.shape == (n_tasks, N, K)


def test_a_dropped_or_repeated_tile_changes_an_integer():
    """Inside a block of 255 points the fingerprints of a tile sum to a value that grows with the tile: dropping tile t, or reading
    tile t' in its place, changes db (and dW at the fingerprint's column)."""
    n_tasks, pts, N, K = 2, 96, 32, 32
    dz, a = WC.int_operands(n_tasks, pts, N, K, _gen(7))
    tiles = dz.reshape(-1, 32, N)  # [tile, point, feature]
    ref_b = WC.ref_db(dz)
    for t in range(tiles.shape[0]):
        for t2 in range(tiles.shape[0]):
            if t == t2:
                continue
            swapped = tiles.clone()
            swapped[t] = tiles[t2]
            assert not torch.equal(swapped.double().sum((0, 1)), ref_b), (t, t2)


@pytest.mark.parametrize("regime", WC.REGIMES)
def test_regimes_hold_their_claims_and_fp32_meets_the_gate(regime, capsys):
    worst_w = worst_b = 0.0
    for j, (n_tasks, pts, N, K) in enumerate(((3, 70, 256, 256), (2, 45, 100, 36), (5, 31, 200, 130))):
        dz, a = WC.regime_operands(regime, n_tasks, pts, N, K, _gen(100 + j))
        assert dz.dtype == a.dtype == torch.float32 and dz.shape == (n_tasks, pts, N) and a.shape == (n_tasks, pts, K)
        WC.check_regime(dz, a)
        ref, mag, ref_b, mag_b = WC.ref_shared(dz, a), WC.mag_shared(dz, a), WC.ref_db(dz), WC.mag_db(dz)
        assert float(mag.min()) > 0 and float(mag_b.min()) > 0
        if regime == "paired_scales":
            assert 2.0 ** 30 < float(dz.abs().median()) < 2.0 ** 42 and 2.0 ** -50 < float(a.abs().median()) < 2.0 ** -38
        elif regime == "tiny":
            assert float(dz.abs().max()) < 2.0 ** -46 and float(a.abs().max()) < 2.0 ** -46
        elif regime == "six_decades":
            assert float(dz.abs().max()) / float(dz.abs().median()) > 1e3
        elif regime == "cancel":
            assert float(ref.abs().max()) == 0.0 and float(ref_b.abs().max()) == 0.0 and float(mag.min()) > 1e-3
        elif regime == "one_point":
            nz = (dz.abs().sum(-1) > 0)
            assert nz.sum(1).tolist() == [1] * n_tasks
            assert [int(r.nonzero()[0]) for r in nz] == WC.one_point_positions(n_tasks, pts)
            assert torch.equal((a.abs().sum(-1) > 0), nz)
        elif regime == "one_feature_hot":
            assert float(dz[..., N // 3].abs().median()) > 3e3 * float(dz[..., 0].abs().median())
            assert float(a[..., 2 * K // 3].abs().median()) > 3e3 * float(a[..., 0].abs().median())
        # the gate of the GPU tests, on a float32 contraction in a shuffled order
        dW, db = WC.contract_f32_shuffled(dz, a, _gen(200 + j))
        rw = float(((dW.double() - ref).abs() / mag).max()) / 2e-6
        rb = float(((db.double() - ref_b).abs() / mag_b).max()) / 2e-6
        assert rw <= 0.5 and rb <= 0.5, (regime, N, K, rw, rb)
        worst_w, worst_b = max(worst_w, rw), max(worst_b, rb)
        # the bf16 gate: bf16-rounded operands, same evaluation
        zr, ar = WC.bf16_round(dz), WC.bf16_round(a)
        WC.check_regime(zr, ar)
        dW16, _ = WC.contract_f32_shuffled(zr, ar, _gen(300 + j))
        r16 = float(((dW16.double() - WC.ref_shared(zr, ar)).abs() / WC.mag_shared(zr, ar)).max()) / 2e-6
        assert r16 <= 0.5, (regime, N, K, r16)
        worst_w = max(worst_w, r16)
    with capsys.disabled():
        print(f"\n[wgrad regimes, shuffled fp32 on the CPU] {regime:16s} worst err / gate: dW {worst_w:.3f}  db {worst_b:.3f}")


def test_tile_layouts_round_trip():
    g = _gen(9)
    for B, P, F in ((2, 45, 36), (1, 64, 256), (3, 1, 5)):
        rows = WC.bf16_round(torch.randn(B, P, F, generator=g))
        p32 = WC.pack_pt32(rows)
        assert p32.shape == (B, WC.tiles_of(P), WC.pad32(F) // 4, 32, 4)
        assert torch.equal(WC.unpack_pt32(p32, P, F), rows)
        full = WC.unpack_pt32(p32, WC.tiles_of(P) * 32, WC.pad32(F))
        assert float(full[:, P:].abs().sum()) == 0 and float(full[:, :, F:].abs().sum()) == 0
        p16 = WC.pack_pt16(rows)
        assert p16.shape == (B, WC.tiles_of(P), WC.pad32(F) // 8, 32, 8) and p16.dtype == torch.bfloat16
        assert torch.equal(WC.unpack_pt16(p16, P, F), rows)
    # feature f = 32 s + 16 h + 4 g + i sits in row 4 s + g, element 4 h + i
    rows = torch.arange(64.0).view(1, 1, 64)
    p16 = WC.pack_pt16(rows).float()
    for f in range(64):
        s, h, gq, i = f // 32, (f // 16) & 1, (f // 4) & 3, f & 3
        assert float(p16[0, 0, 4 * s + gq, 0, 4 * h + i]) == f


def test_plan_splits_agrees_with_the_library():
    from npf_gwwaveform_amd import _lib

    lib = _lib.load()
    # a job alone: the byte count gives its workgroups exactly -- never more than tiles, never more than 256
    for T in (1, 2, 3, 5, 255, 256, 257, 513):
        for flags in (0, WC.F_X6 | WC.F_NO_H16, WC.F_BF16, WC.F_BF16 | WC.F_DZ16 | WC.F_A16):
            (sp,) = WC.plan_splits(lib, [(32, 32)], flags, 1, T)
            assert sp == min(T, 256)
            assert (_lib_total(lib, [(32, 32)], flags, 1, T) - 16) // (4 * WC.slab_floats(32, 32)) == sp
    # 16 identical jobs: 16 workgroups each, or one per tile where there are fewer tiles
    for T, n_tasks, tiles in ((1, 1, 1), (15, 3, 5), (16, 2, 8), (17, 17, 1), (81, 9, 9)):
        for flags in (0, WC.F_X6 | WC.F_NO_H16, WC.F_X6, WC.F_BF16 | WC.F_DZ16 | WC.F_A16):
            for N, K in ((32, 32), (256, 256), (32, 256)):
                assert WC.plan_splits(lib, [(N, K)] * 16, flags, n_tasks, tiles) == [min(16, T)] * 16
    # the mixes of test_wgrad_job_split_fills_one_round_of_workgroups
    assert sum(WC.plan_splits(lib, [(256, 256)] * 7, 0, 64, 32)) == 256
    sk = WC.plan_splits(lib, [(256, 256), (4, 256)], WC.F_BF16, 64, 32)
    assert 85 <= sk[1] <= 100 and sum(sk) == 256
    sk = WC.plan_splits(lib, [(256, 256), (4, 256)], 0, 64, 32)
    assert 55 <= sk[1] <= 75 and sum(sk) == 256
    # per-task jobs: one workgroup per task, no partials
    assert WC.plan_splits(lib, [(64, 64, True), (64, 64)], 0, 5, 3) == [5, 15]
    assert WC.tiles_per_workgroup(17, 16) == [2] + [1] * 15 and WC.tiles_per_workgroup(3, 3) == [1, 1, 1]


def _lib_total(lib, shapes, flags, n_tasks, tiles):
    from npf_gwwaveform_amd import _lib

    sh, fl = WC._norm(shapes, flags)
    return WC._lib_bytes(lib, _lib.NpfWgradJob, sh, fl, n_tasks, tiles)
