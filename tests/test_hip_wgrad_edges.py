"""The weight-gradient kernels (csrc/wgrad_kernel.hip: ``wgrad_kernel<false>``, ``wgrad_kernel<true>``, ``wgrad_x6_kernel``,
``wgrad_h16_kernel``, ``wgrad_reduce_kernel`` and the host-side plan) and their Python callers (``chain.run_wgrad``) where they can
go wrong without a random-operand test at one tolerance noticing: tiles dealt unevenly to the workgroups of a job, the four-slot
pipeline of the bf16 kernel with both operands PT16 (1, 2, 3, 4, 5+ tiles per workgroup; waves that own 0, 1 or 2 DMA pieces), the
wave-activity rules at the 32- and 64-feature edges, the reduce kernel's ``n_split % 4`` tail and row guard, the launch chunks and
block jobs of the wrapper, and the memory contracts (overwrite mode reads nothing, the reduce reads only what was written, a
per-task PT32 output is written whole with zero padding).

Most tests are EXACT: ``wgrad_cases.int_operands`` builds small-integer operands whose contraction is exact in bf16, in the three
x6 terms and in fp32 accumulation in any order, so every variant has to reproduce the float64 reference bit for bit
(``torch.equal``); every (task, point) carries a fingerprint, so a dropped, repeated or early-read tile changes an integer.  All
launches but those of test 5 go through the C ABI (``wgrad_cases.run_jobs``) with the flags set by hand -- ``chain.run_wgrad``
would send narrow jobs of an x6 launch to the native kernel -- and with a NaN-filled workspace.

Variants: ``native`` (fp32 MFMA), ``x6`` (NPF_WGRAD_F32X6 | NPF_WGRAD_NO_H16), ``h16`` (NPF_WGRAD_F32X6 at 256 x 256 only),
``bf16`` (fp32 tiles), ``bf16_z16`` / ``bf16_a16`` / ``bf16_dual`` (PT16 tiles on dZ, on A, on both).

What the plan does not allow: a shared-weight job never gets more workgroups than there are tiles (``plan``: ``sp > total_tiles``),
so with 16 jobs over 1 or 15 tiles every job has 1 or 15 workgroups of one tile each and no workgroup is without a tile;
test 3 asserts that count instead of 16.

Test 8 (value regimes) gates ``|got - ref| <= 2e-6 * sum |dz| |a|`` and ``2e-6 * sum |dz|`` for db.  The bf16 variants are gated
against the float64 contraction of the bf16-rounded operands; their db against the dz the kernel was handed, which for a PT16
dZ is the rounded tensor (the unrounded one does not exist on that path) and otherwise the unrounded one.

Recorded on an MI355X (worst err / gate over the three shapes, dW / db, as test 8 prints it; a float32 contraction in a shuffled
order on the CPU gives 0.06 ... 0.26, tests/test_wgrad_cases_host.py):

    variant      paired_scales          tiny   six_decades        cancel     one_point  one_feature_hot
    native       0.062 / 0.013  0.048 / 0.013  0.197 / 0.053  0.014 / 0.000  0.090 / 0.058  0.052 / 0.016
    x6           0.025 / 0.014  0.026 / 0.016  0.127 / 0.033  0.000 / 0.000  0.111 / 0.058  0.025 / 0.015
    h16          0.027 / 0.013  0.031 / 0.010  0.142 / 0.033  0.000 / 0.000  0.094 / 0.043  0.027 / 0.014
    bf16         0.029 / 0.014  0.024 / 0.016  0.133 / 0.033  0.000 / 0.000  0.078 / 0.058  0.022 / 0.015
    bf16_z16     0.029 / 0.003  0.024 / 0.004  0.133 / 0.037  0.000 / 0.000  0.078 / 0.032  0.022 / 0.005
    bf16_a16     0.029 / 0.014  0.024 / 0.016  0.133 / 0.033  0.000 / 0.000  0.078 / 0.058  0.022 / 0.015
    bf16_dual    0.029 / 0.003  0.024 / 0.004  0.133 / 0.037  0.000 / 0.000  0.078 / 0.032  0.022 / 0.005

Mutated copies of the kernel file, and how many of the 286 cases here fail on each (of the four older wgrad tests of
tests/test_hip_kernels.py): the shared-job loop of split 0 stopping one tile early 41 (1); the reduce without its tail loop 64 (4);
the dual-PT16 wait always ``vmcnt(4)`` 35 (1) -- at 32 x 32 the two 1 KiB pieces land before the barrier lets anyone read, the
wider shapes catch it; the reduce guard ``k + e < Kp`` 165 (not run: it writes past the end of their exactly-sized dW);
``_launch_wgrad`` chunking at 15 jobs 4 (0).  The x6 step rule with ``<=`` for ``<`` (``64 (2 cp + 1) <= Kp``) fails nothing and
cannot: at Kp = 64 / 192 it only adds four steps on quad rows of the LDS image that no DMA writes (zeros), and the write-out drops
those columns (``col0 >= Kp``) -- same values, more work.  The rule moved the other way (``64 (2 cp + 1) + 32 < Kp``, which skips a
column block that has data) fails 6 (1)."""
import math

import pytest
import torch

import wgrad_cases as WC
from helpers import launch_witness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -12345.0

VARIANTS = {
    "native": 0,
    "x6": WC.F_X6 | WC.F_NO_H16,
    "h16": WC.F_X6,
    "bf16": WC.F_BF16,
    "bf16_z16": WC.F_BF16 | WC.F_DZ16,
    "bf16_a16": WC.F_BF16 | WC.F_A16,
    "bf16_dual": WC.F_BF16 | WC.F_DZ16 | WC.F_A16,
}
GENERAL = tuple(v for v in VARIANTS if v != "h16")  # every shape
ALL = tuple(VARIANTS)


def variants_for(N, K):
    return ALL if (N, K) == (256, 256) else GENERAL


def _z16(v):
    return bool(VARIANTS[v] & WC.F_DZ16)


def _a16(v):
    return bool(VARIANTS[v] & WC.F_A16)


def _lib():
    from npf_gwwaveform_amd import _lib

    return _lib.load()


# ---- cases: operands, references (computed once, never modified) and packed copies ------------------------------------------------
class Case:
    def __init__(self, dz, a):
        self.dz, self.a = dz, a
        self.n_tasks, self.pts, self.N = dz.shape
        self.K = a.shape[-1]
        self._memo = {}

    def _get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    ref = property(lambda s: s._get("ref", lambda: WC.ref_shared(s.dz, s.a)))
    per = property(lambda s: s._get("per", lambda: WC.ref_per_task(s.dz, s.a)))
    db = property(lambda s: s._get("db", lambda: WC.ref_db(s.dz)))
    mag = property(lambda s: s._get("mag", lambda: WC.mag_shared(s.dz, s.a)))
    mag_db = property(lambda s: s._get("mag_db", lambda: WC.mag_db(s.dz)))
    rounded = property(lambda s: s._get("rounded", lambda: Case(WC.bf16_round(s.dz), WC.bf16_round(s.a))))

    def op(self, which, fmt16):
        rows = self.dz if which == "dz" else self.a
        return self._get((which, fmt16), lambda: (WC.pack_pt16 if fmt16 else WC.pack_pt32)(rows)).to(DEV)


_INT_CASES = {}


def int_case(n_tasks, pts, N, K, seed=0):
    key = (n_tasks, pts, N, K, seed)
    if key not in _INT_CASES:
        g = torch.Generator().manual_seed(((seed * 131 + n_tasks) * 1009 + pts) * 66003 + N * 257 + K)
        _INT_CASES[key] = Case(*WC.int_operands(n_tasks, pts, N, K, g))
    return _INT_CASES[key]


def assert_same(got, want, what):
    """``torch.equal`` with NaN equal to NaN, and a message that says where."""
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got != want))
    if bool(bad.any()):
        at = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: "
                             f"got {float(got[at])}, want {float(want[at])}")


def _int_base(shape, seed):
    return torch.randint(-99, 100, shape, generator=torch.Generator().manual_seed(seed)).float()


# ---- jobs -------------------------------------------------------------------------------------------------------------------------
def shared_job(case, v, db=True, acc=False, fill=SENT, guard=5):
    """A shared-weight job into a dW of N + 8 rows and ``ldw = K + guard`` columns and a db of N + 3 entries, all ``fill``
    (accumulate: an integer base in the N x K / N part): ``want_w`` / ``want_b`` are what has to be there afterwards."""
    N, K = case.N, case.K
    dW, dbt = torch.full((N + 8, K + guard), fill), torch.full((N + 3,), fill)
    want_w, want_b = dW.clone(), dbt.clone()
    want_w[:N, :K], want_b[:N] = case.ref.float(), case.db.float()
    if acc:
        dW[:N, :K], dbt[:N] = _int_base((N, K), 11), _int_base((N,), 12)
        want_w[:N, :K] += dW[:N, :K]
        want_b[:N] += dbt[:N]
    return dict(dZ=case.op("dz", _z16(v)), A=case.op("a", _a16(v)), N=N, K=K, dW=dW.to(DEV), db=dbt.to(DEV) if db else None,
                ldw=K + guard, flags=VARIANTS[v] | int(acc), want_w=want_w, want_b=want_b if db else None)


def per_task_job(case, v, acc=False, fill=NAN, k_extra=0, k_off=0):
    """A per-task job into a PT32 tensor of ``pad32(K) + k_extra`` features, all ``fill`` (accumulate: an integer base with zero
    padding), the job's block starting at feature ``k_off``: ``want`` is the whole tensor afterwards as rows
    [task, pad32(N), features] -- the job's rows and features exact, its padding 0.0, everything else untouched."""
    N, K, B = case.N, case.K, case.n_tasks
    Np, Kp = WC.pad32(N), WC.pad32(K)
    Ko = Kp + k_extra
    rows = torch.full((B, Np, Ko), fill)
    want = rows.clone()
    want[:, :, k_off:k_off + Kp] = 0.0
    want[:, :N, k_off:k_off + K] = case.per.float()
    if acc:
        assert k_extra == 0
        rows.zero_()
        rows[:, :N, :K] = _int_base((B, N, K), 13)
        want += rows
    return dict(dZ=case.op("dz", _z16(v)), A=case.op("a", _a16(v)), N=N, K=K, dW=WC.pack_pt32(rows).to(DEV), per_task=True,
                flags=VARIANTS[v] | int(acc), ldo=Ko if k_extra else 0, dW_off=k_off * 32, want=want)


def launch(jobs, n_tasks, pts):
    WC.run_jobs(jobs, n_tasks, pts)
    torch.cuda.synchronize()


def check(jobs, what):
    for j, jb in enumerate(jobs):
        if jb.get("per_task"):
            Np, Ko = jb["want"].shape[1:]
            assert_same(WC.unpack_pt32(jb["dW"].cpu(), Np, Ko), jb["want"], f"{what} job {j} per-task output")
        else:
            assert_same(jb["dW"], jb["want_w"], f"{what} job {j} dW")
            if jb["want_b"] is not None:
                assert_same(jb["db"], jb["want_b"], f"{what} job {j} db")


# ---- 1. feature edges -------------------------------------------------------------------------------------------------------------
FEATURE_PAIRS = ((1, 1), (3, 5), (5, 3), (4, 256), (256, 4), (1, 255), (255, 1), (31, 33), (33, 31), (32, 32), (5, 64), (64, 5),
                 (63, 65), (65, 63), (64, 64), (3, 128), (128, 3), (31, 129), (129, 31), (127, 128), (33, 192), (192, 33),
                 (191, 193), (193, 191), (65, 256), (256, 65), (255, 256), (256, 256))


def _shape_variants(shapes):
    return [(N, K, v) for N, K in shapes for v in variants_for(N, K)]


@pytest.mark.parametrize("N,K,variant", _shape_variants(FEATURE_PAIRS))
def test_feature_edges_exact(N, K, variant):
    """Every 32- / 64-feature edge of the wave-activity rules, both orientations of every skinny pair, K on both sides of the x6
    step rule: dW and db equal the float64 reference bit for bit; the guard columns of dW (ldw = K + 5), its rows beyond N and the
    db entries beyond N keep their sentinel."""
    case = int_case(2, 45, N, K)
    jobs = [shared_job(case, variant)]
    launch(jobs, 2, 45)
    check(jobs, f"{variant} {N}x{K}")


# ---- 2. point and tile edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,variant", _shape_variants(((32, 32), (100, 36), (256, 256))))
def test_point_and_tile_edges_exact(N, K, variant):
    """1 ... 65 points per task (a lone point, a full tile, one point into the next tile) for 1, 2, 3 tasks: shared-weight and
    per-task jobs, the per-task output NaN-filled before."""
    for pts in (1, 31, 32, 33, 63, 64, 65):
        for n_tasks in (1, 2, 3):
            case = int_case(n_tasks, pts, N, K)
            for jobs in ([shared_job(case, variant)], [per_task_job(case, variant)]):
                launch(jobs, n_tasks, pts)
                check(jobs, f"{variant} {N}x{K} {n_tasks} tasks of {pts} points")


# ---- 3. tiles per workgroup -------------------------------------------------------------------------------------------------------
TILE_COUNTS = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (17, 1), 31: (31, 1), 33: (3, 11), 47: (47, 1), 48: (3, 16), 49: (7, 7),
               64: (2, 32), 65: (5, 13), 81: (9, 9)}  # total tiles -> (tasks, tiles per task)


def _sixteen_jobs(variant, N, K):
    lib = _lib()
    for total, (n_tasks, tiles) in TILE_COUNTS.items():
        pts = tiles * 32 - 7
        splits = WC.plan_splits(lib, [(N, K)] * 16, VARIANTS[variant], n_tasks, tiles)
        assert splits == [min(16, total)] * 16, (total, splits)
        per_wg = WC.tiles_per_workgroup(total, splits[0])
        assert sum(per_wg) == total and set(per_wg) == {total // splits[0], -(-total // splits[0])}, per_wg
        cases = [int_case(n_tasks, pts, N, K, seed) for seed in range(4)]
        jobs = [shared_job(cases[j % 4], variant) for j in range(16)]
        launch(jobs, n_tasks, pts)
        check(jobs, f"{variant} 16 jobs of {N}x{K} over {total} tiles ({per_wg} per workgroup)")


@pytest.mark.parametrize("variant", ALL)
def test_tiles_per_workgroup_sixteen_jobs_exact(variant):
    """16 identical jobs in one launch have 16 workgroups each (one per tile below 16 tiles): over 1 ... 81 tiles a workgroup gets
    1, 1 or 2, 2, 2 or 3, 3, 3 or 4, 4, 4 or 5, 5 or 6 tiles -- prologue, steady state and drain of every pipeline."""
    N, K = (256, 256) if variant == "h16" else (32, 32)
    _sixteen_jobs(variant, N, K)


@pytest.mark.parametrize("N,K", ((32, 256), (256, 32), (256, 256)))
def test_tiles_per_workgroup_dual_pt16_piece_counts_exact(N, K):
    """The four-slot pipeline of the bf16 kernel with both operands PT16 counts its ``s_waitcnt vmcnt`` from the DMA pieces a wave
    issues per tile: 16 dZ + 16 A pieces at 256 x 256 (2 per wave), 2 + 16 and 16 + 2 at 32 x 256 and 256 x 32 (0, 1 or 2 per
    wave), 2 + 2 at 32 x 32 (test above).  Same tile counts."""
    _sixteen_jobs("bf16_dual", N, K)


@pytest.mark.parametrize("variant", GENERAL)
def test_tiles_per_workgroup_one_job_exact(variant):
    """One 32 x 32 job alone: 255 and 256 tiles give one tile per workgroup, 257 / 511 / 513 give 256 workgroups of 1 or 2, 1 or 2,
    2 or 3 tiles."""
    lib = _lib()
    for total, (n_tasks, tiles) in {255: (15, 17), 256: (16, 16), 257: (257, 1), 511: (73, 7), 513: (27, 19)}.items():
        pts = tiles * 32 - 7
        (split,) = WC.plan_splits(lib, [(32, 32)], VARIANTS[variant], n_tasks, tiles)
        assert split == min(total, 256)
        case = int_case(n_tasks, pts, 32, 32)
        jobs = [shared_job(case, variant)]
        launch(jobs, n_tasks, pts)
        check(jobs, f"{variant} one job over {total} tiles, {split} workgroups")


@pytest.mark.parametrize("variant", ALL)
def test_tiles_per_task_per_task_jobs_exact(variant):
    """Per-task jobs: one workgroup per task walks the task's 1, 2, 3, 4, 5, 7 tiles."""
    N, K = (256, 256) if variant == "h16" else (100, 36)
    for tiles in (1, 2, 3, 4, 5, 7):
        pts = tiles * 32 - 7
        case = int_case(3, pts, N, K)
        jobs = [per_task_job(case, variant)]
        launch(jobs, 3, pts)
        check(jobs, f"{variant} per-task {N}x{K}, {tiles} tiles per task")


# ---- 4. reduce tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", GENERAL)
def test_reduce_tail_exact(variant):
    """The reduce kernel sums the partials of a job four at a time with a tail loop: job mixes whose workgroup counts are 0, 1,
    2 and 3 mod 4 (a count of 1 among them), with and without db, overwriting and accumulating."""
    lib = _lib()
    shapes = [(32, 32), (100, 36), (256, 256)]
    seen = set()
    for n_tasks, tiles in ((1, 1), (1, 2), (3, 1), (2, 2), (5, 1), (3, 2), (7, 1), (2, 4), (8, 30)):
        pts = tiles * 32 - 7
        splits = WC.plan_splits(lib, shapes, VARIANTS[variant], n_tasks, tiles)
        seen.update(splits)
        cases = [int_case(n_tasks, pts, N, K) for N, K in shapes]
        for db in (True, False):
            for acc in (False, True):
                jobs = [shared_job(c, variant, db=db, acc=acc) for c in cases]
                launch(jobs, n_tasks, pts)
                check(jobs, f"{variant} splits {splits} db={db} accumulate={acc}")
    assert 1 in seen and {s % 4 for s in seen} == {0, 1, 2, 3}, sorted(seen)
    assert any(s > 8 for s in seen), sorted(seen)  # and one mix the tile count does not cap


# ---- 5. launch composition through chain.run_wgrad -------------------------------------------------------------------------------
def _mode(monkeypatch, mode, narrow_native=True):
    from npf_gwwaveform_amd import chain as CH

    monkeypatch.setattr(CH, "WGRAD_X6", mode == "x6")
    monkeypatch.setattr(CH, "WGRAD_H16", True)
    monkeypatch.setattr(CH, "X6_NARROW_NATIVE", narrow_native)
    monkeypatch.setattr(CH, "COMPUTE_DTYPE", "bf16" if mode.startswith("bf16") else "fp32")
    return CH


def _chain_shared(case, mode, db=True, acc=False):
    N, K = case.N, case.K
    p16 = mode == "bf16_pt16"
    dW, dbt = torch.zeros(N, K), torch.zeros(N)
    if acc:
        dW, dbt = _int_base((N, K), 21), _int_base((N,), 22)
    return dict(dZ=case.op("dz", p16), A=case.op("a", p16), N=N, K=K, dW=dW.to(DEV), db=dbt.to(DEV) if db else None, accumulate=acc,
                want_w=case.ref.float() + (dW if acc else 0), want_b=(case.db.float() + (dbt if acc else 0)) if db else None)


def _chain_per_task(case, mode):
    N, K, B = case.N, case.K, case.n_tasks
    p16 = mode == "bf16_pt16"
    want = torch.zeros(B, WC.pad32(N), WC.pad32(K))
    want[:, :N, :K] = case.per.float()
    out = torch.full((B, WC.tiles_of(N), WC.pad32(K) // 4, 32, 4), NAN, device=DEV)
    return dict(dZ=case.op("dz", p16), A=case.op("a", p16), N=N, K=K, dW=out, per_task=True, want=want)


def _chain_run(CH, jobs, n_tasks, pts):
    keys = ("dZ", "A", "N", "K", "dW", "db", "per_task", "accumulate")
    with launch_witness() as wit:
        CH.run_wgrad([{k: jb[k] for k in keys if k in jb} for jb in jobs], n_tasks, pts, DEV)
        torch.cuda.synchronize()
    return wit


CHAIN_MODES = ("native", "x6", "bf16", "bf16_pt16")


@pytest.mark.parametrize("mode", CHAIN_MODES)
def test_chain_launch_chunks_exact(mode, monkeypatch):
    """1, 15, 16, 17 and 33 jobs in one ``run_wgrad``: one ``npf_wgrad_run`` per 16 jobs, no more, every job exact."""
    CH = _mode(monkeypatch, mode)
    for n_jobs in (1, 15, 16, 17, 33):
        jobs = [_chain_shared(int_case(2, 45, 40, 64, seed), mode, acc=seed % 2 == 1) for seed in range(n_jobs)]
        wit = _chain_run(CH, jobs, 2, 45)
        assert wit["npf_wgrad_run"] == math.ceil(n_jobs / 16) == wit["npf_wgrad_partials_bytes"], (n_jobs, wit)
        check(jobs, f"{mode} {n_jobs} jobs")


@pytest.mark.parametrize("narrow_native", (True, False))
def test_chain_narrow_and_wide_jobs_exact(narrow_native, monkeypatch):
    """An fp32 launch with narrow (a side <= 32) and wide jobs: the narrow ones go to the native kernel in a launch of their own
    (``X6_NARROW_NATIVE``) or stay on the x6 kernel; exact both ways."""
    CH = _mode(monkeypatch, "x6", narrow_native)
    shapes = ((256, 4), (64, 64), (4, 256), (100, 36), (32, 2), (33, 33), (256, 256))
    jobs = [_chain_shared(int_case(3, 70, N, K), "x6") for N, K in shapes]
    wit = _chain_run(CH, jobs, 3, 70)
    assert wit["npf_wgrad_run"] == (2 if narrow_native else 1), wit
    check(jobs, f"narrow_native={narrow_native}")
    # narrow jobs alone: one launch either way
    jobs = [_chain_shared(int_case(3, 70, N, K), "x6") for N, K in shapes[:1] + shapes[2:3]]
    assert _chain_run(CH, jobs, 3, 70)["npf_wgrad_run"] == 1
    check(jobs, f"narrow only, narrow_native={narrow_native}")


@pytest.mark.parametrize("mode", CHAIN_MODES)
def test_chain_shared_and_per_task_jobs_in_one_launch_exact(mode, monkeypatch):
    CH = _mode(monkeypatch, mode)
    n_tasks, pts = 3, 70
    shapes = ((64, 64), (100, 36), (256, 256), (37, 96))
    jobs = []
    for j, (N, K) in enumerate(shapes):
        case = int_case(n_tasks, pts, N, K)
        jobs += [_chain_shared(case, mode), _chain_per_task(case, mode)] if j % 2 == 0 else [_chain_per_task(case, mode), _chain_shared(case, mode)]
    assert _chain_run(CH, jobs, n_tasks, pts)["npf_wgrad_run"] == 1
    check(jobs, f"{mode} mixed shared / per-task")


def test_chain_one_odd_job_leaves_h16_and_stays_exact(monkeypatch):
    """256 x 256 jobs run on wgrad_h16_kernel; one 256 x 255 job in the launch sends all of them to wgrad_x6_kernel."""
    CH = _mode(monkeypatch, "x6")
    n_tasks, pts = 3, 70
    square = [_chain_shared(int_case(n_tasks, pts, 256, 256, seed), "x6") for seed in range(2)]
    assert _chain_run(CH, square, n_tasks, pts)["npf_wgrad_run"] == 1
    check(square, "two 256x256 jobs")
    jobs = [_chain_shared(int_case(n_tasks, pts, 256, 256, seed), "x6") for seed in range(2)]
    jobs.insert(1, _chain_shared(int_case(n_tasks, pts, 256, 255), "x6"))
    assert _chain_run(CH, jobs, n_tasks, pts)["npf_wgrad_run"] == 1
    check(jobs, "256x256 jobs + one 256x255")


@pytest.mark.parametrize("mode", CHAIN_MODES)
def test_chain_block_jobs_exact(mode, monkeypatch):
    """Sides wider than 256 become block jobs (``_block_jobs``: ``dW_off``, db with the first column block only, ``ldz`` / ``lda``
    strides): with db, accumulating; and a per-task K = 288 whose blocks share one PT32 output (``ldo``)."""
    CH = _mode(monkeypatch, mode)
    n_tasks, pts = 2, 45
    jobs = [_chain_shared(int_case(n_tasks, pts, N, K), mode, acc=True) for N, K in ((257, 33), (300, 257), (512, 512), (33, 288))]
    jobs.append(_chain_per_task(int_case(n_tasks, pts, 64, 288), mode))
    wit = _chain_run(CH, jobs, n_tasks, pts)
    # 2 + 4 + 4 + 2 + 2 = 14 block jobs; an fp32 launch sends the narrow blocks (1 x 33, 44 x 1, 33 x 32 ...) to the native kernel
    assert wit["npf_wgrad_run"] == (2 if mode == "x6" else 1), wit
    check(jobs, f"{mode} block jobs")


def test_chain_per_task_job_over_256_rows_is_refused(monkeypatch):
    CH = _mode(monkeypatch, "native")
    case = int_case(1, 33, 257, 32)
    with pytest.raises(NotImplementedError):
        _chain_run(CH, [_chain_per_task(case, "native")], 1, 33)


# ---- 6. exact writes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ALL)
def test_overwrite_reads_neither_outputs_nor_unwritten_partials(variant):
    """Overwrite mode into NaN-filled dW and db, from a NaN-filled workspace, at every shape of test 1: finite and exact where the
    job writes, NaN left where it does not."""
    for N, K in FEATURE_PAIRS:
        if variant in variants_for(N, K):
            jobs = [shared_job(int_case(2, 45, N, K), variant, fill=NAN)]
            launch(jobs, 2, 45)
            check(jobs, f"{variant} {N}x{K} into NaN")


PT_PAIRS = ((1, 1), (5, 3), (33, 31), (64, 5), (5, 64), (31, 129), (100, 36), (256, 65), (65, 256), (256, 256))


@pytest.mark.parametrize("variant", ALL)
def test_per_task_output_is_written_whole(variant):
    """A NaN-filled per-task PT32 output: the N x K part exact, the padding rows and features exactly 0.0 (later kernels read the
    tensor as PT32).  As a block of a wider tensor (``ldo`` > pad32(K), block at feature 32): only the block's features change."""
    for N, K in PT_PAIRS:
        if variant in variants_for(N, K):
            case = int_case(3, 45, N, K)
            jobs = [per_task_job(case, variant), per_task_job(case, variant, fill=SENT, k_extra=96, k_off=32)]
            launch(jobs, 3, 45)
            check(jobs, f"{variant} per-task {N}x{K}")


@pytest.mark.parametrize("variant", ALL)
def test_accumulate_adds_exactly_once(variant):
    for N, K in ((256, 256), (100, 36), (33, 129)):
        if variant in variants_for(N, K):
            case = int_case(3, 70, N, K)
            jobs = [shared_job(case, variant, acc=True), per_task_job(case, variant, acc=True), shared_job(case, variant, db=False, acc=True)]
            launch(jobs, 3, 70)
            check(jobs, f"{variant} accumulate {N}x{K}")


# ---- 7. non-finite confinement ----------------------------------------------------------------------------------------------------
def _float_outputs(variant, dz, a):
    case = Case(dz, a)
    n_tasks, pts, N = dz.shape
    K = a.shape[-1]
    shared = dict(dZ=case.op("dz", _z16(variant)), A=case.op("a", _a16(variant)), N=N, K=K, dW=torch.empty(N, K, device=DEV),
                  db=torch.empty(N, device=DEV), flags=VARIANTS[variant])
    per = dict(shared, dW=torch.empty(n_tasks, WC.tiles_of(N), WC.pad32(K) // 4, 32, 4, device=DEV), db=None, per_task=True)
    launch([shared, per], n_tasks, pts)
    return shared["dW"].cpu(), shared["db"].cpu(), WC.unpack_pt32(per["dW"].cpu(), N, K)


@pytest.mark.parametrize("variant", ALL)
def test_nonfinite_stays_in_its_row_or_column(variant):
    """One NaN, then one +inf, in one (task, point, feature) of dz: every other row of dW, every other db entry and every other row
    of the per-task outputs equal the clean run bit for bit; the same for one feature of a, on the columns (db untouched)."""
    n_tasks, pts, N, K = (3, 70, 256, 256) if variant == "h16" else (2, 45, 100, 36)
    dz, a = WC.regime_operands("six_decades", n_tasks, pts, N, K, torch.Generator().manual_seed(71))
    clean = _float_outputs(variant, dz, a)
    b0, p0, n0, k0 = 1, 33, 37, 33
    rows = torch.arange(N) != n0
    cols = torch.arange(K) != k0
    for bad in (NAN, float("inf")):
        z2 = dz.clone()
        z2[b0, p0, n0] = bad
        dW, db, per = _float_outputs(variant, z2, a)
        assert_same(dW[rows], clean[0][rows], f"{variant} {bad} in dz: other rows of dW")
        assert_same(db[rows], clean[1][rows], f"{variant} {bad} in dz: other db entries")
        assert_same(per[:, rows], clean[2][:, rows], f"{variant} {bad} in dz: other rows of the per-task outputs")
        a2 = a.clone()
        a2[b0, p0, k0] = bad
        dW, db, per = _float_outputs(variant, dz, a2)
        assert_same(dW[:, cols], clean[0][:, cols], f"{variant} {bad} in a: other columns of dW")
        assert_same(db, clean[1], f"{variant} {bad} in a: db")
        assert_same(per[:, :, cols], clean[2][:, :, cols], f"{variant} {bad} in a: other columns of the per-task outputs")


# ---- 8. value regimes against float64 ---------------------------------------------------------------------------------------------
def _ratio(got, ref, mag):
    err = (got.double() - ref).abs()
    assert bool((err[mag == 0] == 0).all())
    return float((err / mag.clamp_min(1e-300)).max())


@pytest.mark.parametrize("shape", ((3, 70, 256, 256), (2, 45, 100, 36), (5, 31, 200, 130)))
@pytest.mark.parametrize("regime", WC.REGIMES)
def test_value_regimes_against_float64(regime, shape):
    n_tasks, pts, N, K = shape
    g = torch.Generator().manual_seed(1000 * WC.REGIMES.index(regime) + N)
    base = Case(*WC.regime_operands(regime, n_tasks, pts, N, K, g))
    ratios, failures = {}, []
    for variant in variants_for(N, K):
        bf16 = bool(VARIANTS[variant] & WC.F_BF16)
        ref_case = base.rounded if bf16 else base
        db_case = base.rounded if _z16(variant) else base
        job = dict(dZ=base.op("dz", _z16(variant)), A=base.op("a", _a16(variant)), N=N, K=K, dW=torch.full((N, K), NAN, device=DEV),
                   db=torch.full((N,), NAN, device=DEV), flags=VARIANTS[variant])
        launch([job], n_tasks, pts)
        rw = _ratio(job["dW"].cpu(), ref_case.ref, ref_case.mag)
        rb = _ratio(job["db"].cpu(), db_case.db, db_case.mag_db)
        ratios[variant] = rw
        print(f"WGRAD8|{regime}|{N}x{K}|{variant}|{rw / 2e-6:.4f}|{rb / 2e-6:.4f}")
        if not (rw <= 2e-6 and rb <= 2e-6):
            failures.append((variant, rw, rb))
    for variant in ("x6", "h16"):
        if variant in ratios and regime in ("cancel", "one_point") and not ratios[variant] <= 4 * ratios["native"] + 2e-7:
            failures.append((variant, "vs native", ratios[variant], ratios["native"]))
    assert not failures, (regime, shape, failures)


# ---- 9. bit-identical repeats -----------------------------------------------------------------------------------------------------
def _float_jobs(variant, cases):
    return [dict(dZ=c.op("dz", _z16(variant)), A=c.op("a", _a16(variant)), N=c.N, K=c.K, dW=torch.full((c.N, c.K), NAN, device=DEV),
                 db=torch.full((c.N,), NAN, device=DEV), flags=VARIANTS[variant]) for c in cases]


@pytest.mark.parametrize("variant", ALL)
def test_repeats_and_job_order_give_the_same_bits(variant):
    """"Deterministic, no atomics": the same launch twice gives the same bits, and so does a launch with its jobs in another
    order, for every job whose workgroup count the plan leaves unchanged."""
    lib = _lib()
    n_tasks, pts = 3, 200
    shapes = [(256, 256)] * 16 if variant == "h16" else [(32, 32)] * 13 + [(100, 36), (64, 64), (32, 256)]
    g = torch.Generator().manual_seed(91)
    cases = [Case(*WC.regime_operands("six_decades", n_tasks, pts, N, K, g)) for N, K in dict.fromkeys(shapes)]
    by_shape = dict(zip(dict.fromkeys(shapes), cases))
    order = list(range(16))
    first = _float_jobs(variant, [by_shape[shapes[j]] for j in order])
    launch(first, n_tasks, pts)
    again = _float_jobs(variant, [by_shape[shapes[j]] for j in order])
    launch(again, n_tasks, pts)
    for j in order:
        assert bool(torch.isfinite(first[j]["dW"]).all())
        assert torch.equal(first[j]["dW"], again[j]["dW"]) and torch.equal(first[j]["db"], again[j]["db"]), (variant, j)
    perm = [15 - j for j in order[:8]] + order[:8]  # the second half reversed in front of the first
    s0 = WC.plan_splits(lib, [shapes[j] for j in order], VARIANTS[variant], n_tasks, WC.tiles_of(pts))
    s1 = WC.plan_splits(lib, [shapes[j] for j in perm], VARIANTS[variant], n_tasks, WC.tiles_of(pts))
    moved = _float_jobs(variant, [by_shape[shapes[j]] for j in perm])
    launch(moved, n_tasks, pts)
    compared = 0
    for pos, j in enumerate(perm):
        if s1[pos] == s0[j]:
            compared += 1
            assert torch.equal(first[j]["dW"], moved[pos]["dW"]) and torch.equal(first[j]["db"], moved[pos]["db"]), (variant, j, pos)
    assert compared >= 12, (s0, s1)
