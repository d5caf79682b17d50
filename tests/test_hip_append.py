"""``npf_append_points`` on the GPU, bit for bit: rows of a PT32 tensor placed behind the rows each task of a padded PT32 tensor holds,
the offsets being device data.  The reference is row-major indexing between ``unpack_pt`` and ``pack_pt`` over WHOLE tiles and all
``pad32(F)`` features, so ``torch.equal`` on the packed tensors covers the appended rows, every other row (those at and beyond the new
count and the tile padding beyond the capacity included) and the feature padding at once."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 70
START = [0, 31, 32, 33, 64]  # offsets on both sides of the 32-row tile boundary
B = len(START)


def _pt_random(n_rows, F, seed):
    """A PT32 tensor [B, n_rows, F] with random values everywhere, tile and feature padding included."""
    from npf_gwwaveform_amd.chain import pt_shape

    g = torch.Generator().manual_seed(seed)
    return torch.randn(pt_shape(B, n_rows, F), generator=g).to(DEV)


def _sentinel(n_rows, F):
    """A finite pattern no source row holds: negative integers below -1000."""
    from npf_gwwaveform_amd.chain import pt_shape

    shape = pt_shape(B, n_rows, F)
    n = 1
    for s in shape:
        n *= s
    return (-(torch.arange(n, dtype=torch.float32) % 4093) - 1000.0).view(shape).to(DEV)


def _ragged(N):
    return [0, N, -3, N + 5, min(2, N)]  # nothing, all, a negative value, more than there is, a part


def _reference(src, dst0, start, n_new, N, F):
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pad32, tiles_of

    Fp = pad32(F)
    s = FN.unpack_pt(src, 32 * tiles_of(N), Fp)
    d = FN.unpack_pt(dst0, 32 * tiles_of(M), Fp).clone()
    counts = []
    for b in range(B):
        have = min(max(start[b], 0), M)
        add = N if n_new is None else min(max(n_new[b], 0), N)
        for j in range(add):
            if have + j < M:
                d[b, have + j] = s[b, j]
        counts.append(min(have + add, M))
    return FN.pack_pt(d), counts


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("ragged", (False, True), ids=("all_rows", "ragged"))
@pytest.mark.parametrize("N", (1, 5, 33))
@pytest.mark.parametrize("F", (20, 128, 256))
def test_append_places_the_rows_and_nothing_else(F, N, ragged):
    from npf_gwwaveform_amd import functional as FN

    src, dst0 = _pt_random(N, F, seed=100 * F + N), _sentinel(M, F)
    n_new = _ragged(N) if ragged else None
    want, want_counts = _reference(src, dst0, START, n_new, N, F)
    dst, counts = dst0.clone(), _i32(START)
    n_new_d = _i32(n_new) if ragged else None
    FN.append_points([(src, dst, F)], counts, n_new_d, B, N, M)
    torch.cuda.synchronize()
    assert counts.tolist() == want_counts
    assert torch.equal(dst, want)
    assert not torch.equal(dst, dst0)  # (something was appended)
    if ragged:
        assert n_new_d.tolist() == n_new  # (read only)


def test_rows_beyond_the_capacity_are_dropped_and_nothing_outside_the_tensor_is_written():
    """Counts [0, 31, 32, 33, 64] + 33 rows at a capacity of 70: 33, 64, 65, 66 and 97 -> 70, the last task saturates after 6 of its
    33 rows.  dst and the counts are views into larger sentinel-filled buffers: the guard bands on both sides stay as they were."""
    from npf_gwwaveform_amd import functional as FN

    F, N, guard = 128, 33, 4096
    src, dst0 = _pt_random(N, F, seed=7), _sentinel(M, F)
    want, want_counts = _reference(src, dst0, START, None, N, F)
    assert want_counts == [33, 64, 65, 66, 70]
    big = torch.full((guard + dst0.numel() + guard,), -7.0, device=DEV)
    dst = big[guard:guard + dst0.numel()].view(dst0.shape)
    dst.copy_(dst0)
    cbig = torch.full((64 + B + 64,), -7, dtype=torch.int32, device=DEV)
    counts = cbig[64:64 + B]
    counts.copy_(_i32(START))
    FN.append_points([(src, dst, F)], counts, None, B, N, M)
    torch.cuda.synchronize()
    assert counts.tolist() == want_counts
    assert torch.equal(dst, want)
    assert (big[:guard] == -7.0).all() and (big[guard + dst0.numel():] == -7.0).all()
    assert (cbig[:64] == -7).all() and (cbig[64 + B:] == -7).all()
    # a saturated tensor takes nothing more
    before = dst.clone()
    full = _i32([M] * B)
    FN.append_points([(src, dst, F)], full, None, B, N, M)
    torch.cuda.synchronize()
    assert full.tolist() == [M] * B and torch.equal(dst, before)


@pytest.mark.parametrize("ragged", (False, True), ids=("all_rows", "ragged"))
def test_two_pairs_in_one_launch_equal_two_launches(ragged):
    from helpers import launch_witness
    from npf_gwwaveform_amd import functional as FN

    N, Fa, Fb = 33, 20, 256
    src_a, src_b = _pt_random(N, Fa, seed=1), _pt_random(N, Fb, seed=2)
    n_new = _i32(_ragged(N)) if ragged else None
    one_a, one_b, c_a, c_b = _sentinel(M, Fa), _sentinel(M, Fb), _i32(START), _i32(START)
    FN.append_points([(src_a, one_a, Fa)], c_a, n_new, B, N, M)
    FN.append_points([(src_b, one_b, Fb)], c_b, n_new, B, N, M)
    two_a, two_b, c = _sentinel(M, Fa), _sentinel(M, Fb), _i32(START)
    with launch_witness() as w:
        FN.append_points([(src_a, two_a, Fa), (src_b, two_b, Fb)], c, n_new, B, N, M)
    torch.cuda.synchronize()
    assert w.calls == {"npf_append_points": 1}
    assert torch.equal(two_a, one_a) and torch.equal(two_b, one_b)
    assert torch.equal(c, c_a) and torch.equal(c, c_b)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from npf_gwwaveform_amd import functional as FN

    src, dst, c = _pt_random(5, 128, seed=3), _sentinel(M, 128), _i32(START)
    with pytest.raises(ValueError, match="pairs"):
        FN.append_points([], c, None, B, 5, M)
    with pytest.raises(ValueError, match="pairs"):
        FN.append_points([(src, dst, 128)] * 4, c, None, B, 5, M)
    with pytest.raises(ValueError, match="pair 0"):
        FN.append_points([(src, dst, 128)], c, None, B, 33, M)  # (src holds one tile of rows)
    with pytest.raises(ValueError, match="pair 0"):
        FN.append_points([(src, dst, 128)], c, None, B, 5, M + 32)
    with pytest.raises(ValueError, match="n_valid"):
        FN.append_points([(src, dst, 128)], c.long(), None, B, 5, M)
    with pytest.raises(ValueError, match="n_new"):
        FN.append_points([(src, dst, 128)], c, c[:3], B, 5, M)
    with pytest.raises(ValueError, match="device"):
        FN.append_points([(src, dst, 128)], c.cpu(), None, B, 5, M)
    assert c.tolist() == START and torch.equal(dst, _sentinel(M, 128))
