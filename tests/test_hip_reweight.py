"""Reweighted contexts on the GPU: ``npf_masked_attn_fwd_weighted`` and ``npf_weighted_mean`` against float64 (the formulas of
tests/reweight_cases.py), and ``Conditioned.reweighted`` / ``kfold`` / ``bootstrap`` against the oracle run in float64 on the context
with its rows PHYSICALLY repeated by the integer weights (``expand_context``) or cut to the other folds.

Gates.  Attention kernel: the expression ``tests/test_hip_masked.py`` applies to ``npf_masked_attn_fwd`` (``assert_gated`` with 1e-5),
per (replicate, task).  ``weighted_mean``: ``assert_gated`` with 1e-6 per task, ``loo_mean``'s gate at this row count, the fp32
evaluation being the same formula in fp32 torch.  Models: the project's fp32 gate on loc and scale, max|d| <= 1e-5 max|ref|; the
per-point k-fold log densities to 2e-5 of their largest (a relative error of 1e-5 in sigma moves the z^2 / 2 term by 2e-5 of itself:
the bound and the reasoning of tests/test_hip_loo.py).  Model inputs: the first seed for which no ReLU pre-activation of the float64
reference lies within 2e-7 of zero (the ``_well_posed_inputs`` rule; it reads the reference alone).  The transformer case has r = 128,
the width at which the default 8 heads are 16 features wide."""
import math

import pytest
import torch

import reweight_cases as RC
import specs
from helpers import EpsIndependent, assert_close, build_model, launch_witness
from oracle import npf_oracle as O
from test_hip_dispatch import _c
from test_hip_masked_edges import _poison_feature_padding, _poison_rows
from test_hip_mha import assert_gated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RELU_TIE = 2e-7
ATTN_ENTRIES = ("npf_masked_attn_fwd", "npf_masked_attn_fwd_nq", "npf_masked_attn_fwd_loo", "npf_masked_attn_fwd_prefix", "npf_mha_fwd")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _pt(rows):
    from npf_gwwaveform_amd import functional as FN

    return FN.pack_pt(rows.to(DEV)).detach()


# ---- 1. the attention kernel against float64 -------------------------------------------------------------------------------
K_B, K_CPAD, K_COUNTS, K_QCOUNTS, K_S = 4, 80, (80, 33, 1, 0), (80, 17, 64, 5), 4
ZERO_REPLICATE_TASK = (1, 1)


def _kernel_weights(g):
    """[S, B, C_pad]: all ones; integers in 0 .. 3; log-uniform in [1e-3, 1e3]; a 0 / 1 mask in which a whole 32-key block of task 0
    is zero and the only admissible key of its first block is the block's last row.  One (replicate, task) is all zero."""
    W = torch.ones(K_S, K_B, K_CPAD)
    W[1] = torch.randint(0, 4, (K_B, K_CPAD), generator=g).float()
    W[2] = torch.exp((torch.rand(K_B, K_CPAD, generator=g) * 2 - 1) * math.log(1e3))
    W[3] = torch.randint(0, 2, (K_B, K_CPAD), generator=g).float()
    W[3, 0, :31], W[3, 0, 31], W[3, 0, 32:64] = 0, 1, 0
    W[ZERO_REPLICATE_TASK] = 0
    return W


def _nan_beyond(W, counts):
    W = W.clone()
    for b, n in enumerate(counts):
        W[:, b, n:] = math.nan
    return W


def _weighted_launch(q_pt, k_pt, v_pt, W, counts, q_counts, C_pad, T, d):
    from npf_gwwaveform_amd import functional as FN

    B, S = len(counts), W.shape[0]
    with launch_witness() as w:
        o = FN.masked_attention_weighted(q_pt, k_pt, v_pt, W.to(DEV), _i32(counts), S * B, B, C_pad, T, d, 1.0 / math.sqrt(d),
                                         n_q_valid=None if q_counts is None else _i32(q_counts))
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_weighted"] == 1 and all(w[e] == 0 for e in ATTN_ENTRIES), w
    return o


@pytest.mark.parametrize("d", (4, 24, 64, 100, 256))
def test_weighted_attention_matches_float64(d):
    """Counts across the 16- / 32-key block edges, query counts across the 16- / 64-query edges, four kinds of weight rows and an
    all-zero one; NaN in every padding row and padding feature of the operands and in the weights beyond the counts; exact zeros
    where no key is admissible and beyond the query counts; a second launch gives the same bits.  K / V are shared by the replicates,
    so the K rows (NaN) and V rows (+Inf) of zero-weight keys are poisoned per replicate in one-replicate launches, which must
    reproduce the bits of the clean launch."""
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(900 + d)
    Q, K, V = (torch.randn(K_B, K_CPAD, d, generator=g) * a for a in (1.5, 1.5, 1.0))  # (as tests/test_hip_masked.py)
    W = _kernel_weights(g)
    scale = 1.0 / math.sqrt(d)
    q_pt = _poison_feature_padding(_poison_rows(_pt(Q), K_QCOUNTS), d)
    k_pt, v_pt = (_poison_feature_padding(_poison_rows(_pt(x), K_COUNTS), d) for x in (K, V))
    assert all(x.isnan().any() for x in (q_pt, k_pt, v_pt))
    Wn = _nan_beyond(W, K_COUNTS)
    o_pt = _weighted_launch(q_pt, k_pt, v_pt, Wn, K_COUNTS, K_QCOUNTS, K_CPAD, K_CPAD, d)
    out = FN.unpack_pt(o_pt, K_CPAD, d).view(K_S, K_B, K_CPAD, d)
    Wf = W.view(K_S * K_B, K_CPAD)
    r64, r32 = (RC.weighted_attention(Q, K, V, Wf, K_COUNTS, K_QCOUNTS, scale, dt).view(K_S, K_B, K_CPAD, d)
                for dt in (torch.float64, torch.float32))
    for s in range(K_S):
        for b, (n, nq) in enumerate(zip(K_COUNTS, K_QCOUNTS)):
            err = float((out[s, b].cpu().double() - r64[s, b]).abs().max())
            print(f"d={d} replicate {s} task {b} (n={n}, nq={nq}): max|d|={err:.3e} max|ref|={float(r64[s, b].abs().max()):.3e}")
            assert_gated(out[s, b], r64[s, b], r32[s, b], 1e-5, f"d={d} replicate {s} task {b}")
            assert (out[s, b, nq:] == 0).all(), f"replicate {s} task {b}: rows beyond the query count {nq}"
            if not RC.admissible(W[s, b], n).any():
                assert (out[s, b] == 0).all(), f"replicate {s} task {b}: no admissible key"
    assert (out[ZERO_REPLICATE_TASK] == 0).all() and float(r64[ZERO_REPLICATE_TASK[0], 0].abs().max()) > 0
    assert torch.isfinite(o_pt).all(), "NaN from the padding of the operands or the weights reached the result"
    assert torch.equal(_weighted_launch(q_pt, k_pt, v_pt, Wn, K_COUNTS, K_QCOUNTS, K_CPAD, K_CPAD, d), o_pt), "a second launch gave other bits"
    for s in (1, 3):  # (the replicates with zero weights)
        Kb, Vb = K.clone(), V.clone()
        Kb[W[s] == 0], Vb[W[s] == 0] = math.nan, math.inf
        kb, vb = (_poison_feature_padding(_poison_rows(_pt(x), K_COUNTS), d) for x in (Kb, Vb))
        one = _weighted_launch(q_pt, kb, vb, Wn[s:s + 1], K_COUNTS, K_QCOUNTS, K_CPAD, K_CPAD, d)
        assert torch.equal(one, o_pt[s * K_B:(s + 1) * K_B]), f"replicate {s}: a K / V row of a zero-weight key reached the result"
    # without a query count every row is a query: the rows below the counts keep their bits
    o_all = FN.unpack_pt(_weighted_launch(_pt(Q), k_pt, v_pt, Wn, K_COUNTS, None, K_CPAD, K_CPAD, d), K_CPAD, d).view(K_S, K_B, K_CPAD, d)
    for b, nq in enumerate(K_QCOUNTS):
        assert torch.equal(o_all[:, b, :nq], out[:, b, :nq]), f"task {b}: rows below the query count without n_q_valid"


# ---- 2. all-ones weights: the bits of the masked entry --------------------------------------------------------------------------
@pytest.mark.parametrize("d", (4, 24, 64, 100, 256))
def test_unit_weights_give_the_bits_of_masked_attention(d):
    from npf_gwwaveform_amd import functional as FN

    g = torch.Generator().manual_seed(1900 + d)
    Q, K, V = (_pt(torch.randn(K_B, K_CPAD, d, generator=g) * a) for a in (1.5, 1.5, 1.0))
    ones = torch.ones(1, K_B, K_CPAD)
    n, scale = _i32(K_COUNTS), 1.0 / math.sqrt(d)
    got = _weighted_launch(Q, K, V, ones, K_COUNTS, K_QCOUNTS, K_CPAD, K_CPAD, d)
    with launch_witness() as w:
        want = FN.masked_attention(Q, K, V, n, K_B, K_CPAD, K_CPAD, d, scale, n_q_valid=_i32(K_QCOUNTS))
        plain = FN.masked_attention(Q, K, V, n, K_B, K_CPAD, K_CPAD, d, scale)
    assert w["npf_masked_attn_fwd_nq"] == 1 and w["npf_masked_attn_fwd"] == 1, w
    assert torch.equal(got, want), f"d={d}: all-ones weights differ from npf_masked_attn_fwd_nq"
    assert torch.equal(_weighted_launch(Q, K, V, ones, K_COUNTS, None, K_CPAD, K_CPAD, d), plain)


# ---- 3. a maximum that a replicate does not own -----------------------------------------------------------------------------------
def test_a_zero_weight_key_does_not_set_the_running_maximum():
    """Key 7 outscores every other key of every query by more than 200 (checked in float64): the replicate that gives it weight 0
    must still match float64 -- exp(s - the maximum it never reaches) would underflow every one of its terms."""
    from npf_gwwaveform_amd import functional as FN

    d, n, C_pad, T = 64, 50, 64, 20
    g = torch.Generator().manual_seed(77)
    u = torch.ones(d) / math.sqrt(d)
    Q = torch.randn(1, T, d, generator=g) + 4.0 * u
    K, V = torch.randn(1, C_pad, d, generator=g), torch.randn(1, C_pad, d, generator=g)
    K[0, 7] = 4000.0 * u
    scale = 1.0 / math.sqrt(d)
    S64 = Q[0].double() @ K[0, :n].double().T * scale
    others = torch.cat([S64[:, :7], S64[:, 8:]], dim=1)
    gap = float((S64[:, 7:8] - others).min())
    print(f"smallest gap between key 7 and any other key: {gap:.1f}")
    assert gap > 200
    W = torch.ones(2, 1, C_pad)
    W[1, 0, 7] = 0
    out = FN.unpack_pt(_weighted_launch(_pt(Q), _pt(K), _pt(V), W, (n,), None, C_pad, T, d), T, d)
    r64, r32 = (RC.weighted_attention(Q, K, V, W.view(2, C_pad), (n,), None, scale, dt) for dt in (torch.float64, torch.float32))
    for s in range(2):
        assert_gated(out[s], r64[s], r32[s], 1e-5, f"replicate {s}")
    assert float(r64[1].abs().max()) > 0.05 and float((r64[1] - r64[0]).abs().max()) > 0.05


# ---- 4. weighted_mean against float64 ---------------------------------------------------------------------------------------------
M_COUNTS, M_PTS, M_S = (40, 33, 32, 1, 0), 40, 3


@pytest.mark.parametrize("F", (32, 96, 256))
def test_weighted_mean_matches_float64(F):
    """Positive, integer (0 .. 3) and all-zero weight rows; NaN in the rows and weights beyond the counts (tiles beyond are not
    read); the rows of zero weight hold NaN in a one-replicate launch that must reproduce the bits (R is shared by the replicates)."""
    from npf_gwwaveform_amd import functional as FN

    B = len(M_COUNTS)
    g = torch.Generator().manual_seed(40 + F)
    R = torch.randn(B, M_PTS, F, generator=g)
    W = torch.rand(M_S, B, M_PTS, generator=g) * 3.75 + 0.25
    W[1] = torch.randint(0, 4, (B, M_PTS), generator=g).float()
    W[2, 0] = 0
    Wn = _nan_beyond(W, M_COUNTS).to(DEV)
    R_pt = _poison_rows(_pt(R), M_COUNTS)

    def launch(r_pt, w):
        with launch_witness() as wit:
            o = FN.weighted_mean(r_pt, w, _i32(M_COUNTS), w.shape[0] * B, B, M_PTS, F)
            torch.cuda.synchronize()
        assert wit["npf_weighted_mean"] == 1 and wit["npf_masked_mean_fwd"] == 0 and wit["npf_loo_mean"] == 0, wit
        return o

    out = launch(R_pt, Wn)
    assert out.shape == (M_S * B, F) and torch.isfinite(out).all()
    r64, r32 = (RC.weighted_mean_ref(R, W.view(M_S * B, M_PTS), M_COUNTS, dt) for dt in (torch.float64, torch.float32))
    for j in range(M_S * B):
        s, b = divmod(j, B)
        err = float((out[j].cpu().double() - r64[j]).abs().max())
        print(f"F={F} replicate {s} task {b} (n={M_COUNTS[b]}): max|d|={err:.3e} max|ref|={float(r64[j].abs().max()):.3e}")
        assert_gated(out[j], r64[j], r32[j], 1e-6, f"F={F} replicate {s} task {b}")
        if not RC.admissible(W[s, b], M_COUNTS[b]).any():
            assert (out[j] == 0).all(), f"replicate {s} task {b}: the weights sum to 0"
    assert (out[2 * B] == 0).all() and (out[4::B] == 0).all()
    assert torch.equal(launch(R_pt, Wn), out), "a second launch gave other bits"
    Rb = R.clone()
    Rb[W[1] == 0] = math.nan
    assert torch.equal(launch(_poison_rows(_pt(Rb), M_COUNTS), Wn[1:2]), out[B:2 * B]), "a row of zero weight reached the result"


# ---- 5. models against the oracle ---------------------------------------------------------------------------------------------------
B, C, T, DY, S, CAPACITY = 3, 20, 12, 2, 3, 32
COUNTS = (20, 9, 1)
KW = dict(B=B, T=T)
CASES = {
    "cnp_r128": _c("CNP", 128, C, **KW),
    "attncnp_r64": _c("AttnCNP", 64, C, **KW),
    "attncnp_transformer_r128": _c("AttnCNP", 128, C, attention="transformer", **KW),
    "lnp_r128": _c("LNP", 128, C, encoded_path="latent", n_z=1, **KW),
    "attnlnp_r128_nz2": _c("AttnLNP", 128, C, n_z=2, **KW),
}
_CACHE = {}


def _model_weights():
    """Integer multiplicities [S, B, C] in 0 .. 3 with one (replicate, task) all zero."""
    W = torch.randint(0, 4, (S, B, C), generator=torch.Generator().manual_seed(8)).float()
    W[2, 0] = 0
    W[0, 2, 0] = 2  # (the one-point task: its point twice in replicate 0)
    return W


def _oracle_on(case, params64, Xc, Yc, Xt, eps, margins=False):
    """The oracle's float64 forward on one task: context [n, .] rows (n may be 0), targets [t, .]."""
    cfg = specs.cfg_of(case)
    n_z = case.get("n_z", 1)
    return O.forward(cfg, params64, Xc.double().unsqueeze(0), Yc.double().unsqueeze(0), Xt.double().unsqueeze(0), None,
                     eps=None if eps is None else eps.double(), n_z=n_z, training=False)


def _float64(fn):
    """Run ``fn`` with float64 as the default dtype (the zero representations the oracle makes for an empty context follow it)."""
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.set_default_dtype(default)


def _oracle_reweighted(case, params64, X, Y, Xt, W, eps, margins=False):
    """float64 (loc, scale) [n_z, S B, T, dy]: for every (s, b) the oracle on task b's context physically expanded by ``W[s, b]``
    (cut to the count first).  ``margins``: -> the smallest |ReLU pre-activation| instead."""
    n_z = case.get("n_z", 1)
    loc, scale = (torch.zeros(n_z, S * B, T, DY, dtype=torch.float64) for _ in range(2))
    O.RELU_MARGINS = [] if margins else None
    try:
        def run():
            for s in range(S):
                for b, n in enumerate(COUNTS):
                    Xe, Ye = RC.expand_context(X[b, :n], Y[b, :n], W[s, b, :n])
                    o = _oracle_on(case, params64, Xe, Ye, Xt[b], None if eps is None else eps[:, b:b + 1])
                    loc[:, s * B + b], scale[:, s * B + b] = o["loc"][:, 0], o["scale"][:, 0]
        _float64(run)
        return min(O.RELU_MARGINS) if margins else (loc, scale)
    finally:
        O.RELU_MARGINS = None


def _setup(name):
    if name in _CACHE:
        return _CACHE[name]
    case = CASES[name]
    params = specs.make_params(case, seed=11)
    params64 = {k: v.double() for k, v in params.items()}
    W = _model_weights()
    latent = case["kind"] in ("LNP", "AttnLNP")
    for seed in range(4321, 4321 + 200):
        inp = specs.make_inputs(case, seed=seed)
        X, Y, Xt, eps = inp["X_cntxt"], inp["Y_cntxt"], inp["X_trgt"], inp.get("eps") if latent else None
        if _oracle_reweighted(case, params64, X, Y, Xt, W, eps, margins=True) >= RELU_TIE:
            break
    else:
        raise AssertionError("no well-posed inputs in 200 seeds")
    model = build_model(case, DEV, params=params).eval()
    out = dict(case=case, model=model, seed=seed, X=X.to(DEV), Y=Y.to(DEV), Xt=Xt.to(DEV), W=W, eps=eps,
               ref=_oracle_reweighted(case, params64, X, Y, Xt, W, eps))
    _CACHE[name] = out
    return out


def _condition(s, how):
    """The state of test 5: with a capacity of 32 rows, or ``condition(n_cntxt=...)``; the latent draw is the setup's ``eps``."""
    m, n = s["model"], _i32(COUNTS)
    if how == "capacity":
        post = m.condition_with_capacity(s["X"], s["Y"], CAPACITY, n_cntxt=n)
        if s["eps"] is not None:
            post.eps.copy_(s["eps"].to(DEV))  # (the replicates draw z = loc + scale * eps from the state's eps)
        W = torch.full((S, B, CAPACITY), math.nan)  # (the rows beyond the counts, the stored capacity included, carry no weight)
        W[:, :, :C] = s["W"]
        return post, W.to(DEV)
    if s["eps"] is not None:
        EpsIndependent.eps = s["eps"].to(DEV)
    try:
        return m.condition(s["X"], s["Y"], n_cntxt=n), s["W"].to(DEV)
    finally:
        EpsIndependent.eps = None


@pytest.mark.parametrize("how", ("capacity", "n_cntxt"))
@pytest.mark.parametrize("name", list(CASES))
def test_reweighted_matches_the_oracle_on_the_expanded_contexts(name, how):
    s = _setup(name)
    post, W = _condition(s, how)
    attentive = s["case"]["kind"].startswith("Attn")
    pooled = not attentive or s["case"]["kind"] == "AttnLNP"
    n_z = s["case"].get("n_z", 1)
    with launch_witness() as w:
        p = post.reweighted(W).query(s["Xt"])
        d = p.base_dist
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_weighted"] == int(attentive) and w["npf_weighted_mean"] == int(pooled), w
    assert all(w[e] == 0 for e in ATTN_ENTRIES) and w["npf_masked_mean_fwd"] == 0, w
    assert tuple(p.batch_shape) == (n_z, S * B, T) and tuple(p.event_shape) == (DY,)
    for what, got, want in (("loc", d.loc, s["ref"][0]), ("scale", d.scale, s["ref"][1])):
        err = float((got.cpu().double() - want).abs().max())
        print(f"{name} [{how}] (input seed {s['seed']}) {what}: max|d|={err:.3e} max|ref|={float(want.abs().max()):.3e}")
        assert_close(got, want, what=f"{name} [{how}] {what}")
    # the summary and the score work on the result as on any other
    q = p.summary((0.5,))
    assert q.mean.shape == (S * B, T, DY) and torch.isfinite(q.mean).all() and torch.isfinite(q.std).all()
    if n_z == 1:
        assert_close(q.mean, d.loc[0].cpu(), tol=1e-6, what="summary mean")
    sc = p.score(s["Y"][:, :T].repeat(S, 1, 1).contiguous(), want=("log_density",))
    assert sc.log_density.shape == (S * B, T, DY) and torch.isfinite(sc.log_density).all()


def test_target_counts_are_repeated_per_replicate():
    s = _setup("attncnp_r64")
    post, W = _condition(s, "capacity")
    nt = (12, 5, 0)
    full = post.reweighted(W).query(s["Xt"]).base_dist
    cut = post.reweighted(W).query(s["Xt"], n_trgt=_i32(nt)).base_dist
    for j in range(S * B):
        t = nt[j % B]
        if t > 0:
            assert_close(cut.loc[0, j, :t], full.loc[0, j, :t].cpu(), what=f"task {j} below its target count")
        assert (cut.loc[0, j, t:] == 0).all() and (cut.scale[0, j, t:] == 1).all()


# ---- 6. k-fold ----------------------------------------------------------------------------------------------------------------------
F_B, F_C, F_K = 2, 24, 4
F_COUNTS = (24, 10)
F_CASES = {"cnp_r128": _c("CNP", 128, F_C, B=F_B, T=1), "attncnp_r64": _c("AttnCNP", 64, F_C, B=F_B, T=1)}
# contiguous bands; in task 1 (10 points) fold 1 holds a single point and fold 2 none (the rows beyond the count carry any id)
FOLDS = torch.tensor([[0] * 6 + [1] * 6 + [2] * 6 + [3] * 6, [0] * 5 + [1] + [3] * 4 + [2] * 14])
_F_CACHE = {}


def _oracle_kfold(case, params64, X, Y, margins=False):
    """float64 (loc, scale) [B, C, dy] (0 / 1 beyond the counts): for every task and valid ``i`` the oracle on the task's points of
    the other folds with ``x_i`` as the only target."""
    loc, scale = torch.zeros(F_B, F_C, DY, dtype=torch.float64), torch.ones(F_B, F_C, DY, dtype=torch.float64)
    O.RELU_MARGINS = [] if margins else None
    try:
        def run():
            for b, n in enumerate(F_COUNTS):
                for i in range(n):
                    keep = [j for j in range(n) if int(FOLDS[b, j]) != int(FOLDS[b, i])]
                    o = _oracle_on(case, params64, X[b, keep], Y[b, keep], X[b, i:i + 1], None)
                    loc[b, i], scale[b, i] = o["loc"][0, 0, 0], o["scale"][0, 0, 0]
        _float64(run)
        return min(O.RELU_MARGINS) if margins else (loc, scale)
    finally:
        O.RELU_MARGINS = None


def _f_setup(name):
    if name in _F_CACHE:
        return _F_CACHE[name]
    case = F_CASES[name]
    params = specs.make_params(case, seed=11)
    params64 = {k: v.double() for k, v in params.items()}
    for seed in range(4321, 4321 + 200):
        inp = specs.make_inputs(case, seed=seed)
        X, Y = inp["X_cntxt"], inp["Y_cntxt"]
        if _oracle_kfold(case, params64, X, Y, margins=True) >= RELU_TIE:
            break
    else:
        raise AssertionError("no well-posed inputs in 200 seeds")
    out = dict(case=case, model=build_model(case, DEV, params=params).eval(), seed=seed, X=X.to(DEV), Y=Y.to(DEV),
               ref=_oracle_kfold(case, params64, X, Y))
    _F_CACHE[name] = out
    return out


@pytest.mark.parametrize("name", list(F_CASES))
def test_kfold_matches_the_oracle_on_the_other_folds(name):
    s = _f_setup(name)
    m, n, folds = s["model"], _i32(F_COUNTS), FOLDS.to(DEV)
    attentive = s["case"]["kind"].startswith("Attn")
    with launch_witness() as w:
        p = m.kfold(s["X"], s["Y"], folds, F_K, n_cntxt=n)
        d = p.base_dist
        torch.cuda.synchronize()
    assert w["npf_masked_attn_fwd_weighted"] == int(attentive) and w["npf_weighted_mean"] == int(not attentive), w
    assert all(w[e] == 0 for e in ATTN_ENTRIES) and w["npf_loo_mean"] == 0, w
    assert tuple(p.batch_shape) == (1, F_B, F_C)
    loc, scale = s["ref"]
    for what, got, want in (("loc", d.loc[0], loc), ("scale", d.scale[0], scale)):
        err = float((got.cpu().double() - want).abs().max())
        print(f"{name} kfold (input seed {s['seed']}) {what}: max|d|={err:.3e} max|ref|={float(want.abs().max()):.3e}")
        assert_close(got, want, what=f"{name} kfold {what}")
    for b, nb in enumerate(F_COUNTS):
        assert (d.loc[0, b, nb:] == 0).all() and (d.scale[0, b, nb:] == 1).all(), f"task {b}: rows beyond the count {nb}"
    # k-fold scores from one encode: the per-point log density against the oracle's
    Yc = s["Y"].cpu().double()
    want = -0.5 * ((Yc - loc) / scale) ** 2 - scale.log() - 0.5 * math.log(2 * math.pi)
    for b, nb in enumerate(F_COUNTS):
        want[b, nb:] = 0
    assert_close(p.score(s["Y"], want=("log_density",)).log_density, want, tol=2e-5, what=f"{name} k-fold log density")
    # the stored state gives the same predictions, with a capacity or with counts
    for post in (m.condition_with_capacity(s["X"], s["Y"], F_C, n_cntxt=n), m.condition(s["X"], s["Y"], n_cntxt=n)):
        e = post.kfold(folds, F_K).base_dist
        assert_close(e.loc, d.loc.cpu(), what=f"{name}: Conditioned.kfold loc")
        assert_close(e.scale, d.scale.cpu(), what=f"{name}: Conditioned.kfold scale")


@pytest.mark.parametrize("name", list(F_CASES))
def test_kfold_with_one_point_per_fold_is_loo(name):
    s = _f_setup(name)
    m, n = s["model"], _i32(F_COUNTS)
    own = torch.arange(F_C, device=DEV).repeat(F_B, 1)
    a, b = m.kfold(s["X"], s["Y"], own, F_C, n_cntxt=n).base_dist, m.loo(s["X"], s["Y"], n_cntxt=n).base_dist
    assert_close(a.loc, b.loc.cpu(), what=f"{name}: kfold(k = C) against loo, loc")
    assert_close(a.scale, b.scale.cpu(), what=f"{name}: kfold(k = C) against loo, scale")


# ---- 7. bootstrap and capture -------------------------------------------------------------------------------------------------------
def test_bootstrap_weights_on_the_device():
    import npf_gwwaveform_amd as A

    n = _i32((20, 9, 1, 0))
    W = A.bootstrap_weights(n, 16, CAPACITY, generator=torch.Generator(device=DEV).manual_seed(1))
    assert W.shape == (16, 4, CAPACITY) and W.is_cuda and W.dtype == torch.float32
    assert torch.equal(W.sum(-1), n.float().expand(16, 4)) and torch.equal(W, W.round()) and (W >= 0).all()
    for b, nb in enumerate((20, 9, 1, 0)):
        assert (W[:, b, nb:] == 0).all()


@pytest.mark.parametrize("name", ("cnp_r128", "attncnp_r64", "attnlnp_r128_nz2"))
def test_bootstrap_is_reweighted_with_bootstrap_weights(name):
    import npf_gwwaveform_amd as A

    s = _setup(name)
    post, _ = _condition(s, "capacity")
    g = torch.Generator(device=DEV).manual_seed(3)
    a = post.bootstrap(s["Xt"], 4, generator=g).base_dist
    g.manual_seed(3)
    W = A.bootstrap_weights(post.n_cntxt, 4, CAPACITY, generator=g, device=DEV)
    b = post.reweighted(W).query(s["Xt"]).base_dist
    assert a.loc.shape[1] == 4 * B and torch.equal(a.loc, b.loc) and torch.equal(a.scale, b.scale)
    assert float((a.loc[0, :B] - a.loc[0, B:2 * B]).abs().max()) > 0  # (the replicates differ)


@pytest.mark.parametrize("name", ("cnp_r128", "attncnp_r64", "attncnp_transformer_r128"))
def test_a_captured_query_sees_new_weights_at_replay(name):
    """``reweighted(W).query(X).summary()`` captured once and replayed after ``W`` was overwritten in place equals the eager call
    with the new weights bit for bit; a host read of the weights or the counts inside the capture would make it fail."""
    import npf_gwwaveform_amd as A

    s = _setup(name)
    post, W = _condition(s, "capacity")
    W = torch.nan_to_num(W, nan=0.0).contiguous()
    rw = post.reweighted(W)
    assert rw.W.data_ptr() == W.data_ptr()  # (used as given)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            rw.query(s["Xt"]).summary()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = rw.query(s["Xt"]).summary()
    g = torch.Generator(device=DEV).manual_seed(5)
    for trial in range(2):
        W2 = A.bootstrap_weights(post.n_cntxt, S, CAPACITY, generator=g, device=DEV)
        if trial == 1:
            W2[1] = 0  # (a whole replicate without context)
        W.copy_(W2)
        graph.replay()
        torch.cuda.synchronize()
        want = post.reweighted(W2.clone()).query(s["Xt"]).summary()
        for what in ("mean", "std", "quantiles"):
            assert torch.equal(getattr(got, what), getattr(want, what)), (name, trial, what)
            assert torch.isfinite(getattr(got, what)).all()


# ---- 8. the state is only read ----------------------------------------------------------------------------------------------------
def _state_tensors(post):
    out = dict(n_cntxt=post.n_cntxt, R_pts=post._R_pts.t, R=post._R if torch.is_tensor(post._R) else post._R.t, Xc=post._Xc_pt.t)
    if post.z_samples is not None:
        out.update(z=post.z_samples, eps=post.eps, q_loc=post.q_zCc.base_dist.loc, q_scale=post.q_zCc.base_dist.scale)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_state_is_left_untouched(name):
    s = _setup(name)
    post, W = _condition(s, "capacity")
    before = {k: (t.data_ptr(), t.clone()) for k, t in _state_tensors(post).items()}
    d0 = post.query(s["Xt"]).base_dist
    post.reweighted(W).query(s["Xt"]).base_dist
    post.bootstrap(s["Xt"], 2).base_dist
    if s["case"]["kind"] in ("CNP", "AttnCNP"):
        post.kfold(torch.randint(0, 3, (B, CAPACITY), device=DEV), 3).base_dist
    torch.cuda.synchronize()
    d1 = post.query(s["Xt"]).base_dist
    assert torch.equal(d0.loc, d1.loc) and torch.equal(d0.scale, d1.scale)
    for k, t in _state_tensors(post).items():
        assert t.data_ptr() == before[k][0] and torch.equal(t, before[k][1]), k
    assert post.n_rows_bound == C and post.n_cntxt.tolist() == list(COUNTS)
