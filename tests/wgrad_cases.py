"""Inputs, references and launch helpers of the weight-gradient edge tests (tests/test_hip_wgrad_edges.py; the builders are checked
on the CPU by tests/test_wgrad_cases_host.py).  The kernels are those of csrc/wgrad_kernel.hip: ``wgrad_kernel<false>`` (native fp32
MFMA), ``wgrad_kernel<true>`` (bf16 products; operands as fp32 tiles or PT16 tiles), ``wgrad_x6_kernel`` and ``wgrad_h16_kernel``
(fp32 as six bf16 products), ``wgrad_reduce_kernel`` and the host-side plan.  Pure torch on the CPU, seeded; only ``run_jobs``
touches the package (and a GPU).

The contraction:  dW[n][k] = sum over (task, point) of dz[task][point][n] a[task][point][k]  (shared weights),  one such sum per
task (per-task jobs: attention keys / values),  db[n] = sum dz[task][point][n].

Integer operands.  ``int_operands`` fills both operands with integers of [-8, 8] and gives every (task, point) a fingerprint: with
idx = task * pts + point, ``dz[idx][(idx // 255) % N] = 1 + idx % 255`` and ``a[idx][(idx // 255) % K] = 1``.  255 is the largest
integer range that a bf16 holds exactly (8 significant bits), so the fingerprint is exact in every variant; the pair (feature,
value) is distinct over any 255 * N consecutive points, and inside one block of 255 points the fingerprints of a tile sum into
dW[f][f'] and db[f] to a value that grows with the tile's position: a tile that is dropped, read twice or swapped for another one
changes an integer, it cannot cancel.  The builder asserts max sum |dz| |a| < 2^24 and max sum |dz| < 2^24: every partial sum of
every summation order is then an integer below 2^24, i.e. exact in fp32, the three x6 terms of an operand are (x, 0, 0), and every
kernel variant must reproduce the float64 contraction bit for bit.

Value regimes (``regime_operands``; float operands, every non-zero magnitude inside [2^-100, 2^100] so that the three bf16 terms
of an operand stay normal numbers, every |product| sum finite in fp32 -- asserted by ``check_regime`` on the float64 reference):

    paired_scales     dz ~ 2^40, a ~ 2^-40
    tiny              both ~ 2^-50
    six_decades       randn * 10^U(-3, 3), the spread of test_wgrad_split_bf16_products_equal_fp32
    cancel            six_decades with the points in (+x, -x) pairs on the dz side and equal pairs on the a side: dW = db = 0 exactly,
                      sum |dz| |a| large (an odd last point is zero)
    one_point         one non-zero point per task, at point 0, 31, 32, pts - 1 (rotating over the tasks, clipped to the task)
    one_feature_hot   randn with one feature of dz and one of a at 1e4 x its neighbours

The plan.  ``npf_wgrad_partials_bytes`` runs the launcher's host-side plan and returns ONE number per launch, 16 + 4 * sum_j
splits_j * slab_j: a single job's workgroup count follows from it exactly, the counts of several jobs do not.  ``plan_splits``
therefore restates the plan's arithmetic (``_plan_model``: the same double-precision operations in the same order) and accepts its
answer only if the byte count it implies equals the library's for the whole launch AND for every launch with one job left out -- the
one-job differences of test_wgrad_job_split_fills_one_round_of_workgroups, taken for every job.  A plan that changes makes
``plan_splits`` raise instead of letting a test run on a tile pattern it did not ask for."""
import ctypes

import torch

F_ACCUMULATE, F_BF16, F_DZ16, F_A16, F_X6, F_NO_H16 = 1, 2, 4, 8, 16, 32
EXACT_LIMIT = float(2 ** 24)
MAG_LO, MAG_HI = 2.0 ** -100, 2.0 ** 100
FP_RANGE = 255  # fingerprints are 1 .. 255: exact in bf16
REGIMES = ("paired_scales", "tiny", "six_decades", "cancel", "one_point", "one_feature_hot")


def pad32(n):
    return (n + 31) // 32 * 32


def tiles_of(pts):
    return (pts + 31) // 32


# ---- operands --------------------------------------------------------------------------------------------------------------------
def int_operands(n_tasks, pts, N, K, gen):
    """Integer-valued fp32 (dz [n_tasks, pts, N], a [n_tasks, pts, K]) with the per-point fingerprint of the module docstring."""
    dz = torch.randint(-8, 9, (n_tasks, pts, N), generator=gen).float()
    a = torch.randint(-8, 9, (n_tasks, pts, K), generator=gen).float()
    idx = torch.arange(n_tasks * pts)
    dz.view(-1, N)[idx, (idx // FP_RANGE) % N] = (1 + idx % FP_RANGE).float()
    a.view(-1, K)[idx, (idx // FP_RANGE) % K] = 1.0
    assert float(mag_shared(dz, a).max()) < EXACT_LIMIT and float(mag_db(dz).max()) < EXACT_LIMIT, (n_tasks, pts, N, K)
    return dz, a


def fingerprints(n_tasks, pts, N):
    """(feature, value) of the dz-side fingerprint of every (task, point), in idx order."""
    idx = torch.arange(n_tasks * pts)
    return (idx // FP_RANGE) % N, 1 + idx % FP_RANGE


def _spread(gen, *shape):
    return torch.randn(*shape, generator=gen) * 10.0 ** (6 * torch.rand(*shape, generator=gen) - 3)


def one_point_positions(n_tasks, pts):
    return [min((0, 31, 32, pts - 1)[b % 4], pts - 1) for b in range(n_tasks)]


def regime_operands(regime, n_tasks, pts, N, K, gen):
    """fp32 (dz, a) of one value regime; ``check_regime`` holds on the result."""
    zs, as_ = (n_tasks, pts, N), (n_tasks, pts, K)
    if regime == "paired_scales":
        dz, a = torch.randn(*zs, generator=gen) * 2.0 ** 40, torch.randn(*as_, generator=gen) * 2.0 ** -40
    elif regime == "tiny":
        dz, a = torch.randn(*zs, generator=gen) * 2.0 ** -50, torch.randn(*as_, generator=gen) * 2.0 ** -50
    elif regime == "six_decades":
        dz, a = _spread(gen, *zs), _spread(gen, *as_)
    elif regime == "cancel":
        half = pts // 2
        hz, ha = _spread(gen, n_tasks, half, N), _spread(gen, n_tasks, half, K)
        dz, a = torch.zeros(*zs), torch.zeros(*as_)
        dz[:, 0:2 * half:2], dz[:, 1:2 * half:2] = hz, -hz
        a[:, 0:2 * half:2], a[:, 1:2 * half:2] = ha, ha
    elif regime == "one_point":
        dz, a = torch.zeros(*zs), torch.zeros(*as_)
        for b, p in enumerate(one_point_positions(n_tasks, pts)):
            dz[b, p], a[b, p] = _spread(gen, N), _spread(gen, K)
    elif regime == "one_feature_hot":
        dz, a = torch.randn(*zs, generator=gen), torch.randn(*as_, generator=gen)
        dz[..., N // 3] *= 1e4
        a[..., (2 * K) // 3] *= 1e4
    else:
        raise ValueError(regime)
    check_regime(dz, a)
    return dz, a


def check_regime(dz, a):
    """The claim of every value regime: non-zero magnitudes inside [2^-100, 2^100], and the float64 reference, its |.| sum and
    the bias sums finite in fp32."""
    fmax = torch.finfo(torch.float32).max
    for t in (dz, a):
        nz = t.double().abs()
        nz = nz[nz > 0]
        assert nz.numel() > 0 and float(nz.min()) >= MAG_LO and float(nz.max()) <= MAG_HI, (float(nz.min()), float(nz.max()))
    for t in (ref_shared(dz, a), mag_shared(dz, a), mag_per_task(dz, a), mag_db(dz)):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) < fmax


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def ref_shared(dz, a):
    return torch.einsum("bpn,bpk->nk", dz.double(), a.double())


def ref_per_task(dz, a):
    return torch.einsum("bpn,bpk->bnk", dz.double(), a.double())


def ref_db(dz):
    return dz.double().sum((0, 1))


def mag_shared(dz, a):
    return torch.einsum("bpn,bpk->nk", dz.double().abs(), a.double().abs())


def mag_per_task(dz, a):
    return torch.einsum("bpn,bpk->bnk", dz.double().abs(), a.double().abs())


def mag_db(dz):
    return dz.double().abs().sum((0, 1))


def contract_f32_shuffled(dz, a, gen, chunk=5):
    """The shared contraction and the bias sums in float32, over the points in a random order, ``chunk`` points per partial
    product: an fp32 evaluation in an order no kernel uses."""
    N, K = dz.shape[-1], a.shape[-1]
    z, x = dz.reshape(-1, N).float(), a.reshape(-1, K).float()
    perm = torch.randperm(z.shape[0], generator=gen)
    z, x = z[perm], x[perm]
    dW, db = torch.zeros(N, K), torch.zeros(N)
    for p0 in range(0, z.shape[0], chunk):
        dW += z[p0:p0 + chunk].t() @ x[p0:p0 + chunk]
        db += z[p0:p0 + chunk].sum(0)
    return dW, db


# ---- tile layouts (pure index statements of include/npf_hip.h) --------------------------------------------------------------------
def pack_pt32(rows):
    """Row-major [B, P, F] -> PT32 [B, tiles, Fp / 4, 32, 4], zero padded."""
    B, P, F = rows.shape
    tiles, Fp = tiles_of(P), pad32(F)
    buf = torch.zeros(B, tiles * 32, Fp, dtype=rows.dtype)
    buf[:, :P, :F] = rows
    return buf.view(B, tiles, 32, Fp // 4, 4).permute(0, 1, 3, 2, 4).contiguous()


def unpack_pt32(pt, P, F):
    """PT32 -> row-major [B, P, F] (P, F up to the padded sizes: the padding can be read back too)."""
    B, tiles, q, _, _ = pt.shape
    return pt.permute(0, 1, 3, 2, 4).reshape(B, tiles * 32, q * 4)[:, :P, :F].contiguous()


def pack_pt16(rows):
    """Row-major [B, P, F] -> PT16 [B, tiles, Fp / 8, 32, 8] bfloat16: row 4 s + g holds the features {32 s + 4 g + i} and
    {32 s + 16 + 4 g + i}, i < 4."""
    B, P, F = rows.shape
    tiles, Fp = tiles_of(P), pad32(F)
    buf = torch.zeros(B, tiles * 32, Fp)
    buf[:, :P, :F] = rows
    v = buf.view(B, tiles, 32, Fp // 32, 2, 4, 4).permute(0, 1, 3, 5, 2, 4, 6).contiguous()
    return v.view(B, tiles, Fp // 8, 32, 8).to(torch.bfloat16)


def unpack_pt16(t, P, F):
    B, tiles, rows, _, _ = t.shape
    Fp = rows * 8
    v = t.float().view(B, tiles, Fp // 32, 4, 32, 2, 4).permute(0, 1, 4, 2, 5, 3, 6).contiguous()
    return v.view(B, tiles * 32, Fp)[:, :P, :F]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def slab_floats(N, K):
    return pad32(N) * pad32(K) + pad32(N)


def _norm(shapes, flags):
    shapes = [(s[0], s[1], bool(s[2]) if len(s) > 2 else False) for s in shapes]
    flags = [flags] * len(shapes) if isinstance(flags, int) else list(flags)
    assert len(flags) == len(shapes)
    return shapes, flags


def _plan_model(shapes, flags, n_tasks, tiles):
    """csrc/wgrad_kernel.hip ``plan``, restated: workgroups per job."""
    total = n_tasks * tiles
    bf16 = all(f & F_BF16 for f in flags)
    x6 = all((f & (F_X6 | F_BF16)) == F_X6 for f in flags)
    cost = []
    for (N, K, per_task), f in zip(shapes, flags):
        Np, Kp = pad32(N), pad32(K)
        ar, ac = (Np + 63) // 64, (Kp + 63) // 64
        nbytes = 32.0 * (Np * (2.0 if f & F_DZ16 else 4.0) + Kp * (2.0 if f & F_A16 else 4.0))
        if per_task:
            c = 0.0
        elif bf16:
            c = max(nbytes, 18432.0)
        elif x6:
            waves = ar * ((ac + 1) // 2)
            c = max(3072.0 * 1.6 * ((waves + 3) // 4) + 2500.0, nbytes / 6.5)
        else:
            c = max(4096.0 * min(ar, ac), nbytes / 6.5)
        cost.append(c)
    cost_sum = 0.0
    for c in cost:
        cost_sum += c
    n_shared = sum(not s[2] for s in shapes)
    splits, used = [], 0
    for (N, K, per_task), c in zip(shapes, cost):
        if per_task:
            splits.append(0)
            continue
        sp = min(max(int(256.0 * c / cost_sum), 1), total)
        splits.append(sp)
        used += sp
    for j, ((N, K, per_task), c) in enumerate(zip(shapes, cost)):
        if used >= 256:
            break
        if not per_task and c * n_shared >= cost_sum and splits[j] < total:
            splits[j] += 1
            used += 1
    return [n_tasks if s[2] else sp for s, sp in zip(shapes, splits)]


def _lib_bytes(lib, job_struct, shapes, flags, n_tasks, tiles):
    arr = (job_struct * len(shapes))()
    for j, ((N, K, per_task), f) in enumerate(zip(shapes, flags)):
        arr[j].dZ = arr[j].A = arr[j].dW = 4096  # (never dereferenced by the plan)
        arr[j].N, arr[j].K, arr[j].ldw, arr[j].per_task, arr[j].accumulate = N, K, K, int(per_task), f
    return lib.npf_wgrad_partials_bytes(arr, len(shapes), n_tasks, tiles)


def plan_splits(lib, shapes, flags, n_tasks, tiles):
    """Workgroups per job of one launch: ``shapes`` = (N, K) or (N, K, per_task) per job, ``flags`` = the jobs' ``accumulate``
    field(s).  A per-task job has one workgroup per task.  See the module docstring for what the library's byte count pins."""
    from npf_gwwaveform_amd import _lib

    shapes, flags = _norm(shapes, flags)

    def agree(sh, fl):
        model = _plan_model(sh, fl, n_tasks, tiles)
        want = 16 + 4 * sum(sp * slab_floats(N, K) for (N, K, per_task), sp in zip(sh, model) if not per_task)
        got = _lib_bytes(lib, _lib.NpfWgradJob, sh, fl, n_tasks, tiles)
        if got != want:
            raise AssertionError(f"the weight-gradient plan changed: {sh} flags {fl} over {n_tasks} x {tiles} tiles needs {got} bytes, "
                                 f"the restated plan {model} implies {want}")
        return model

    splits = agree(shapes, flags)
    if len(shapes) > 1:
        for j in range(len(shapes)):
            agree(shapes[:j] + shapes[j + 1:], flags[:j] + flags[j + 1:])
    return splits


def tiles_per_workgroup(total_tiles, n_split):
    """Tiles of each workgroup of a shared-weight job (tile split + n * n_split)."""
    return [len(range(s, total_tiles, n_split)) for s in range(n_split)]


# ---- C-ABI runner -----------------------------------------------------------------------------------------------------------------
def run_jobs(jobs, n_tasks, pts, poison_partials=True):
    """One ``npf_wgrad_run`` on device tensors, with a workspace of its own (``chain.run_wgrad`` hides it): NaN-filled before the
    launch unless told otherwise -- the product hands over ``torch.empty``.  jobs: dicts(dZ, A, N, K, dW, db=None, ldw=K,
    per_task=False, flags=0 (the whole ``accumulate`` field), ldz / lda / ldo = 0, dW_off = 0 (floats)).  Returns the workspace."""
    from npf_gwwaveform_amd import _lib as L

    lib = L.load()
    arr = (L.NpfWgradJob * len(jobs))()
    for j, jb in enumerate(jobs):
        z16, a16 = bool(jb.get("flags", 0) & F_DZ16), bool(jb.get("flags", 0) & F_A16)
        assert (jb["dZ"].dtype == torch.bfloat16) == z16 and (jb["A"].dtype == torch.bfloat16) == a16
        for t in (jb["dZ"], jb["A"], jb["dW"]):
            assert t.is_cuda and t.is_contiguous()
        arr[j].dZ, arr[j].A = jb["dZ"].data_ptr(), jb["A"].data_ptr()
        arr[j].dW = jb["dW"].data_ptr() + 4 * jb.get("dW_off", 0)
        arr[j].db = jb["db"].data_ptr() if jb.get("db") is not None else None
        arr[j].ldw = jb.get("ldw") or jb["K"]
        arr[j].N, arr[j].K = jb["N"], jb["K"]
        arr[j].per_task = int(jb.get("per_task", False))
        arr[j].accumulate = jb.get("flags", 0)
        arr[j].ldz, arr[j].lda, arr[j].ldo = jb.get("ldz", 0), jb.get("lda", 0), jb.get("ldo", 0)
    tiles = tiles_of(pts)
    nbytes = lib.npf_wgrad_partials_bytes(arr, len(jobs), n_tasks, tiles)
    assert nbytes > 0, "npf_wgrad_partials_bytes refused the jobs"
    ws = torch.full(((nbytes + 3) // 4,), float("nan") if poison_partials else 0.0, dtype=torch.float32, device=jobs[0]["dW"].device)
    rc = lib.npf_wgrad_run(arr, len(jobs), n_tasks, tiles, ctypes.c_void_p(ws.data_ptr()), nbytes, L.stream_ptr())
    assert rc == 0, f"npf_wgrad_run returned {rc}"
    return ws
