"""Bank match on the GPU: ``npf_waveform_match_bank`` against the float64 reference of tests/match_bank_reference.py (checked on the
CPU by tests/test_match_bank_host.py) at every tile, k-step and chunk boundary, the exact fragment layout of the double-precision
matrix instruction on integer data, removed points against cut ones bit for bit, NaN containment, degenerate pairs, the diagonal
against ``HeadDistribution.match``, ``want`` subsets, bit-identical repeats, a captured ``query`` + ``match_bank``, and
``HeadDistribution.match_bank`` of a deterministic and a latent model.

Gates (match_bank_reference.ratios, the project's own of match_reference.ratios): match, mismatch and best_match |d| <= 1e-9 +
2^-23 |ref|; hh, gg |d| <= 2^-23 |ref|; phase: the difference mod 2 pi <= 1e-6 where the reference match is >= 1e-3; dot: |d| <= 1e-9
sqrt(hh gg); tau_index and best_index exact.  The derivation carries over: double sums of at most 200 terms after at most JC rotation
steps err near 1e-13 on the normalised quantities.  Every test prints its worst error / gate ratio per quantity."""
import math

import pytest
import torch

import match_bank_reference as RB
import match_reference as M
from test_hip_predict import ROUTES, _counts, _model_and_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEEPS = {"rows": lambda f: f["n_bank"] == 3 and f["pts"] == 37 and f["n_tau"] == 5,
          "bank": lambda f: f["n_rows"] == 3 and f["pts"] == 37 and f["n_tau"] == 5,
          "points": lambda f: f["n_rows"] == 3 and f["n_bank"] in (1, 3) and f["n_tau"] in (0, 5),
          "shifts": lambda f: f["n_rows"] == 3 and f["n_bank"] == 5 and f["pts"] == 37,
          "all": lambda f: f["n_rows"] == 33 and f["n_bank"] == 40}


@pytest.fixture(scope="module")
def all_cases():
    return [(tag, fac, case, RB.reference(**RB.call_args(case))) for tag, fac, case in RB.cases()]


def _dev(args):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}


def _check(got, ref, what, worst=None):
    r = RB.ratios(got, ref)
    print(f"BANK {what}: error / gate " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, f"{what}: {r}"
    for k, v in r.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)


def _same_bits(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            same = torch.equal(x, y) if not x.is_floating_point() else torch.equal(x.view(torch.int64 if x.dtype == torch.float64
                                                                                         else torch.int32),
                                                                                  y.view(torch.int64 if y.dtype == torch.float64
                                                                                         else torch.int32))
            assert same, f"{what}: {name} differs"


# ---- the kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", list(SWEEPS))
def test_match_bank_meets_the_float64_reference_at_every_boundary(sweep, all_cases):
    from npf_gwwaveform_amd import functional as FN

    worst, n = {}, 0
    for tag, fac, case, ref in all_cases:
        if not SWEEPS[sweep](fac):
            continue
        n += 1
        args = _dev(RB.call_args(case))
        got = FN.waveform_match_bank(**args, dot=True)
        _same_bits(got, FN.waveform_match_bank(**args, dot=True), f"{tag}: two calls")
        got = {k: v.cpu() for k, v in got._asdict().items()}
        assert all(torch.isfinite(v).all() for v in got.values()), f"{tag}: a non-finite result"
        R_, G_ = fac["n_rows"], fac["n_bank"]
        assert got["match"].shape == (R_, G_) and got["dot"].shape == (R_, G_, 2) and got["dot"].dtype == torch.float64, tag
        assert got["hh"].shape == (R_,) and got["gg"].shape == (G_,) and got["best_index"].shape == (R_,), tag
        assert got["tau_index"].dtype == torch.int32 and got["best_index"].dtype == torch.int32, tag
        _check(got, ref, tag, worst)
    assert n >= 1
    print(f"BANK worst over the {n} cases of sweep {sweep}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_the_f64_fragment_layout_is_exact_on_integer_data():
    """Phases 0, weights 1, no grid, small integer amplitudes: dot[..., 0] is the integer product matrix bit for bit (every partial
    sum is an integer below 2^53) and dot[..., 1] is exactly 0.  The products differ from pair to pair, so one row or column of a
    C/D fragment in the wrong place shows."""
    from npf_gwwaveform_amd import functional as FN

    R_, G_, T = 33, 40, 37
    r, g, t = torch.arange(R_).view(R_, 1), torch.arange(G_).view(G_, 1), torch.arange(T).view(1, T)
    a, b = 1 + (7 * r + t) % 5, 1 + (3 * g + t) % 7  # int64 [R, T], [G, T]
    h = torch.stack([a.float(), torch.zeros(R_, T)], -1)
    bank = torch.stack([b.float(), torch.zeros(G_, T)], -1)
    want = a @ b.t()  # int64
    # what the data can tell apart: neighbouring rows and columns, a transposed tile, and the row map of the f32 instruction,
    # (lane >> 4) * 4 + reg, in the place of the f64 one, (lane >> 4) + 4 * reg (12 of the 16 rows of a tile would change)
    assert (want[:-1] != want[1:]).any(1).all() and (want[:, :-1] != want[:, 1:]).any(0).all()
    assert not torch.equal(want[:16, :16], want[:16, :16].t())
    i = torch.arange(16)
    misplaced = want[:16].clone()
    misplaced[4 * (i % 4) + i // 4] = want[:16]
    assert int((misplaced != want[:16]).any(1).sum()) == 12
    got = FN.waveform_match_bank(h.to(DEV), bank.to(DEV), weights=torch.ones(T, device=DEV), dot=True)
    dot = got.dot.cpu()
    assert torch.equal(dot[..., 0], want.double()), "Re dot is not the integer product matrix"
    assert (dot[..., 1] == 0).all(), "Im dot is not exactly zero"
    assert torch.equal(got.hh.cpu(), (a * a).sum(1).float()) and torch.equal(got.gg.cpu(), (b * b).sum(1).float())
    assert (got.tau_index == 0).all() and (got.phase == 0).all()
    ref = want.double() / ((a * a).sum(1).double().view(R_, 1) * (b * b).sum(1).double().view(1, G_)).sqrt()
    assert ((got.match.cpu().double() - ref).abs() <= 2.0 ** -23 * ref).all()


# ---- removed points, NaN, degenerate pairs --------------------------------------------------------------------------------------------
def _removed_case():
    case = RB.build(17, 18, 45, 17, seed=91, h_ld=4)
    t = torch.arange(45)
    kill = (t % 3 == 0) | (t == 44)  # the first and the last point among them; t % 4 below meets every kind of weight
    kinds = torch.tensor([0.0, -1.0, math.nan, math.inf])[t % 4]
    cut = dict(h=case["h"][:, ~kill], bank=case["bank"][:, ~kill], weights=case["weights"][~kill], freqs=case["freqs"][~kill],
               taus=case["taus"])
    removed = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    removed["weights"][kill] = kinds[kill]
    removed["h"][:, kill] = math.nan
    removed["bank"][:, kill] = math.nan
    removed["freqs"][kill] = math.nan
    return case, removed, cut, kill


def test_removed_points_equal_cut_points_bit_for_bit():
    from npf_gwwaveform_amd import functional as FN

    _, removed, cut, kill = _removed_case()
    a = FN.waveform_match_bank(**_dev(removed), dot=True)
    b = FN.waveform_match_bank(**_dev(cut), dot=True)
    _same_bits(a, b, f"{int(kill.sum())} of 45 points removed against the same points cut")
    assert all(torch.isfinite(v).all() for v in a)
    ref = RB.reference(**cut)
    _check({k: v.cpu() for k, v in a._asdict().items()}, ref, "removed points against the reference of the cut call")
    # without a grid the frequencies are not read at all
    nog = FN.waveform_match_bank(**_dev(dict(removed, taus=None, freqs=torch.full((45,), math.nan))), dot=True)
    _same_bits(nog, FN.waveform_match_bank(**_dev(dict(cut, taus=None, freqs=None)), dot=True), "no grid")


def test_a_nan_at_a_live_point_stays_in_its_row_or_column_and_never_wins():
    from npf_gwwaveform_amd import functional as FN

    case = RB.build(17, 18, 45, 17, seed=92)
    clean = FN.waveform_match_bank(**_dev(case), dot=True)
    r_bad, g_bad = 16, int(clean.best_index[3])  # (a row of the second tile; the template that row 3 falls on)
    bad = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    bad["h"][r_bad, 11, 0] = math.nan
    bad["bank"][g_bad, 30, 0] = math.nan
    got = FN.waveform_match_bank(**_dev(bad), dot=True)
    hit = torch.zeros(17, 18, dtype=torch.bool)
    hit[r_bad], hit[:, g_bad] = True, True
    for name in ("match", "mismatch", "phase", "dot"):
        x, c = getattr(got, name).cpu(), getattr(clean, name).cpu()
        assert torch.isnan(x[hit]).all(), name
        assert torch.equal(x[~hit], c[~hit]), f"{name}: a NaN reached another row or column"
    assert torch.equal(got.tau_index.cpu()[~hit], clean.tau_index.cpu()[~hit])
    assert torch.isnan(got.hh[r_bad]) and torch.isnan(got.gg[g_bad])
    keep = torch.arange(17) != r_bad
    assert torch.equal(got.hh.cpu()[keep], clean.hh.cpu()[keep]) and torch.equal(got.gg.cpu()[torch.arange(18) != g_bad],
                                                                                  clean.gg.cpu()[torch.arange(18) != g_bad])
    bi, bm = got.best_index.cpu(), got.best_match.cpu()
    assert (bi[keep] != g_bad).all() and torch.isfinite(bm[keep]).all(), "a NaN template won best_index"
    ref = RB.reference(**bad)
    assert torch.equal(bi.long(), ref["best_index"]), "best_index over the pairs whose match is not NaN"
    assert bi[3] != clean.best_index.cpu()[3]  # (row 3 lost its template to the NaN and took the runner-up)
    assert bi[r_bad] == 0 and torch.isnan(bm[r_bad])  # every match of the row is NaN


def test_degenerate_pairs_get_the_stated_constants():
    from npf_gwwaveform_amd import functional as FN

    case = RB.build(17, 18, 45, 17, seed=93)
    case["h"][2, :, 0] = 0.0      # a zero row
    case["h"][16, :, 0] = 0.0     # ... and one in the second tile
    case["bank"][5, :, 0] = 0.0   # a zero template
    case["bank"][0, :, 0] = 0.0
    got = FN.waveform_match_bank(**_dev(case), dot=True)
    ref = RB.reference(**case)
    deg = ref["degenerate"]
    assert deg[2].all() and deg[16].all() and deg[:, 5].all() and deg[:, 0].all() and int(deg.sum()) == 2 * 18 + 2 * 17 - 4
    for name, value in (("match", 0.0), ("mismatch", 1.0), ("tau_index", 0), ("phase", 0.0)):
        assert (getattr(got, name).cpu()[deg] == value).all(), name
    assert (got.dot.cpu()[deg] == 0).all()
    assert got.best_index[2] == 0 and got.best_match[2] == 0 and got.best_index[16] == 0 and got.best_match[16] == 0
    _check({k: v.cpu() for k, v in got._asdict().items()}, ref, "degenerate rows and templates")
    # every point removed: every pair is degenerate
    gone = FN.waveform_match_bank(**_dev(dict(case, weights=torch.zeros(45))), dot=True)
    assert (gone.match == 0).all() and (gone.mismatch == 1).all() and (gone.tau_index == 0).all() and (gone.dot == 0).all()
    assert (gone.best_index == 0).all() and (gone.best_match == 0).all() and (gone.hh == 0).all() and (gone.gg == 0).all()


# ---- want, repeats -------------------------------------------------------------------------------------------------------------------
def test_want_subsets_return_none_for_the_rest_and_the_same_bits():
    from npf_gwwaveform_amd import functional as FN

    args = _dev(RB.call_args(RB.build(17, 18, 45, 17, seed=94, h_ld=4)))
    full = FN.waveform_match_bank(**args, dot=True)
    assert all(t is not None for t in full)
    for want, dot in ((("mismatch",), False), (("hh", "gg"), False), (["tau_index", "phase"], True), ((), True), (("best_index",), False),
                      (("best_match", "match"), False), (("best_match", "best_index", "hh"), False)):
        m = FN.waveform_match_bank(**args, want=want, dot=dot)
        for name in m._fields:
            if name in want or (name == "dot" and dot):
                x, y = getattr(m, name), getattr(full, name)
                assert torch.equal(x, y), (want, name)
            else:
                assert getattr(m, name) is None, (want, name)
    with pytest.raises(ValueError, match="want"):
        FN.waveform_match_bank(**args, want=())


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _bank_inputs(T, G, seed):
    """(bank [G, T, 2] with a positive amplitude, weights [T], freqs [T], taus) for a model case."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(seed)
    bank = torch.stack([0.5 + torch.rand(G, T, generator=g), 3.0 * torch.randn(G, T, generator=g)], -1)
    return bank.to(DEV), (0.5 + torch.rand(T, generator=g)).to(DEV), torch.linspace(20.0, 512.0, T).to(DEV), M.grid(FN.MATCH_JC + 1)


def _clear_maxima(ref, what):
    top = ref["mag"].topk(2, dim=2).values
    assert float((top[..., 0] - top[..., 1]).min()) >= 1e-6, f"{what}: the inputs leave tau_index ill posed"
    top = ref["match"].topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-6, f"{what}: the inputs leave best_index ill posed"


@pytest.mark.parametrize("name,latent", [("cnp_r256_c33", False), ("attnlnp_r256_c200_nz8", True)])
def test_models_match_bank_equals_the_reference_on_their_own_loc_and_mean(name, latent):
    import npf_gwwaveform_amd as A

    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z, G = case["B"], case["T"], case.get("n_z", 1), 19
    bank, w, f, taus = _bank_inputs(T, G, 43)
    torch.manual_seed(9)
    if latent:
        p = model.condition(Xc, Yc).query(Xt)
    else:
        with torch.no_grad():
            p = model(Xc, Yc, Xt)[0]
    m = p.match_bank(bank, weights=w, freqs=f, taus=taus, dot=True)
    plain = p.match_bank(bank)
    mean = p.match_bank(bank, weights=w, freqs=f, taus=taus, of="mean")
    assert p._base is None and isinstance(m, A.BankMatch)
    assert all(getattr(m, k).shape == (n_z, Bn, G) for k in ("match", "mismatch", "tau", "tau_index", "phase"))
    assert m.best_index.shape == (n_z, Bn) and m.best_match.shape == (n_z, Bn) and m.dot.shape == (n_z, Bn, G, 2)
    assert m.tau.dtype == torch.float64 and m.tau_index.dtype == torch.int32 and m.best_index.dtype == torch.int32
    assert plain.tau is None and plain.tau_index is None and plain.dot is None and plain.match.shape == (n_z, Bn, G)
    assert mean.match.shape == (1, Bn, G) and mean.best_index.shape == (1, Bn) and mean.dot is None

    def flat(bm):
        d = {k: (v.reshape(-1, *v.shape[2:]) if v is not None else None) for k, v in bm._asdict().items()}
        return d

    loc = p.base_dist.loc.double().reshape(n_z * Bn, T, 2)
    ref = RB.reference(loc, bank, w, f, taus)
    _clear_maxima(ref, name)
    _check(flat(m), ref, f"{name} of=samples against base_dist.loc")
    assert torch.equal(m.tau.cpu().reshape(-1, G), ref["tau"]), name
    _check(flat(plain), RB.reference(loc, bank), f"{name} without weights and grid")
    ref_mean = RB.reference(p.summary().mean, bank, w, f, taus)
    _clear_maxima(ref_mean, name)
    _check(flat(mean), ref_mean, f"{name} of=mean against summary().mean")
    with pytest.raises(ValueError, match="one shared grid"):
        model.condition(Xc, Yc).query(Xt, n_trgt=_counts(Bn, T, 6, T // 2)).match_bank(bank)


def test_the_diagonal_of_match_bank_meets_match_with_equal_tau_index():
    """G = B: pair (b, b) of ``match_bank(bank)`` is row b of ``match(bank)``."""
    case = ROUTES["attnlnp_r256_c200_nz8"]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z = case["B"], case["T"], case.get("n_z", 1)
    bank, w, f, taus = _bank_inputs(T, Bn, 47)
    torch.manual_seed(9)
    p = model.condition(Xc, Yc).query(Xt)
    one = p.match(bank, weights=w, freqs=f, taus=taus)
    many = p.match_bank(bank, weights=w, freqs=f, taus=taus)
    ref = RB.reference(p.base_dist.loc.double().reshape(n_z * Bn, T, 2), bank, w, f, taus)
    _clear_maxima(ref, "diagonal")
    diag = lambda x: x.diagonal(dim1=1, dim2=2)  # noqa: E731
    assert torch.equal(diag(many.tau_index), one.tau_index) and torch.equal(diag(many.tau), one.tau)
    for name in ("match", "mismatch"):
        x, r = diag(getattr(many, name)).double(), getattr(one, name).double()
        q = float(((x - r).abs() / (1e-9 + 2.0 ** -23 * r.abs())).max())
        print(f"BANK diagonal against p.match: {name} error / gate {q:.3g}")
        assert q <= 1.0, (name, q)


# ---- one captured query + match_bank -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnp_r256_c33", "attnlnp_r256_c200_nz8"])
def test_query_and_match_bank_replay_from_one_graph_after_the_bank_is_overwritten(name):
    case = ROUTES[name]
    model, Xc, Yc, Xt = _model_and_inputs(case)
    Bn, T, n_z, G = case["B"], case["T"], case.get("n_z", 1), 19
    torch.manual_seed(23)
    post = model.condition(Xc, Yc)
    bank_s, w_s, f, taus = _bank_inputs(T, G, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            post.query(Xt).match_bank(bank_s, weights=w_s, freqs=f, taus=taus, dot=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p_g = post.query(Xt)
        m_g = p_g.match_bank(bank_s, weights=w_s, freqs=f, taus=taus, dot=True)
        loc_g = p_g.base_dist.loc
    for step in range(2):
        bank_new, w_new, _, _ = _bank_inputs(T, G, 100 + step)
        w_new[step::5] = 0.0  # (and some points removed)
        bank_s.copy_(bank_new)
        w_s.copy_(w_new)
        graph.replay()
        torch.cuda.synchronize()
        ref = RB.reference(loc_g.double().reshape(n_z * Bn, T, 2), bank_new, w_new, f, taus)
        _clear_maxima(ref, name)
        _check({k: v.reshape(-1, *v.shape[2:]) for k, v in m_g._asdict().items()}, ref, f"{name} replay {step}")
        eager = post.query(Xt).match_bank(bank_new, weights=w_new, freqs=f, taus=taus, dot=True)
        for a, b in zip(m_g, eager):
            assert torch.equal(a, b), (name, step)
