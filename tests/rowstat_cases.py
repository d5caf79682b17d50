"""Inputs of the row-statistic edge tests (tests/test_hip_rowstat_edges.py, checked on the CPU by tests/test_rowstat_cases_host.py):
value regimes for the kernels that reduce over a row -- the two LayerNorms (csrc/chain_kernel.hip NPF_OP_LAYERNORM / _BWD,
csrc/ln_kernel.hip), the Gaussian head and the Monte-Carlo objectives (csrc/head_kernels.hip) and the mean
(csrc/layout_kernels.hip).  Pure torch on the CPU, seeded; every builder returns fp32 inputs and a one-line claim that the host
test verifies in float64."""
import torch

# ---- LayerNorm rows ------------------------------------------------------------------------------------------------------------
LN_REGIMES = ("plain", "offset", "offset_big", "tiny", "constant", "outlier", "large", "mixed")
LN_MIXED = LN_REGIMES[:-1]  # point p of a task takes LN_MIXED[p % 7]: the 32 lanes of a tile hold every scale
LN_EPS = 1e-5
OUTLIER = 1e4

LN_CLAIMS = {
    "plain": "0.5 + 2 randn: |mean| / std about 0.25, the conditioning of the older tests",
    "offset": "30 + 0.1 randn: |mean| / std about 300, E[x^2] - E[x]^2 and a padded-sum correction cancel",
    "offset_big": "1000 + randn: |mean| / std about 1000",
    "tiny": "1e-4 randn: var about 1e-8, eps = 1e-5 dominates the root",
    "constant": "one value per row, a multiple of 1/8 up to 8: every fp32 partial sum is exact in any order, var = 0",
    "outlier": "one feature at 1e4, the rest randn",
    "large": "1e15 randn: squares and a sum of 256 of them stay finite in fp32",
    "mixed": "point p of every task takes regime p % 7 of the seven above",
}


def _ln_plain_rows(regime, n, F, gen):
    r = torch.randn(n, F, generator=gen, dtype=torch.float64)
    if regime == "plain":
        return 0.5 + 2.0 * r
    if regime == "offset":
        return 30.0 + 0.1 * r
    if regime == "offset_big":
        return 1000.0 + r
    if regime == "tiny":
        return 1e-4 * r
    if regime == "constant":
        v = torch.randint(1, 65, (n, 1), generator=gen).double() / 8.0
        sign = torch.randint(0, 2, (n, 1), generator=gen).double() * 2.0 - 1.0
        return (sign * v).expand(n, F).clone()
    if regime == "outlier":
        at = torch.randint(F, (n,), generator=gen)
        r[torch.arange(n), at] = OUTLIER
        return r
    if regime == "large":
        return 1e15 * r
    raise ValueError(regime)


def ln_row_regimes(regime, B, pts):
    """The regime of every row of a [B, pts, F] input, as a list of lists of names."""
    return [[LN_MIXED[p % len(LN_MIXED)] if regime == "mixed" else regime for p in range(pts)] for _ in range(B)]


def ln_rows(regime, B, pts, F, seed):
    """(x fp32 [B, pts, F], claim)."""
    gen = torch.Generator().manual_seed(seed)
    if regime != "mixed":
        return _ln_plain_rows(regime, B * pts, F, gen).view(B, pts, F).float(), LN_CLAIMS[regime]
    x = torch.empty(B, pts, F, dtype=torch.float64)
    for p in range(pts):
        x[:, p] = _ln_plain_rows(LN_MIXED[p % len(LN_MIXED)], B, F, gen)
    return x.float(), LN_CLAIMS[regime]


def ln_params(F, seed):
    """gamma in [0.5, 1.5], beta in [-0.5, 0.5] (fp32 [F] each), as the older LayerNorm tests draw them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(F, generator=gen) + 0.5, torch.rand(F, generator=gen) - 0.5


def split_exact(x):
    """(a, b) fp32 with a + b == x exactly in fp32 and in float64: b = 0.75 x rounded to 8 significant bits lies between x / 2 and
    2 x, so a = x - b is exact (Sterbenz) and so is a + b.  LayerNorm(a + b) then sees exactly the rows of the regime."""
    b = (0.75 * x).to(torch.bfloat16).float()
    return x - b, b


def cancelling_pair(B, pts, F, seed):
    """(a, b, claim): a = 100 randn, b = -(a + k ulp(a)) rounded to fp32, k in -3 .. 3: the sum cancels to a few ulps of a before
    any statistic is taken (where a + k ulp(a) crosses a power of two the rounding leaves half-ulp steps).  a + b is exact in fp32
    (Sterbenz), about 1e-5 in size, so eps dominates its variance."""
    gen = torch.Generator().manual_seed(seed)
    a = (100.0 * torch.randn(B, pts, F, generator=gen)).float()
    k = torch.randint(-3, 4, (B, pts, F), generator=gen).double()
    ulp = torch.ldexp(torch.ones_like(a, dtype=torch.float64), torch.frexp(a.double())[1] - 24)
    b = -(a.double() + k * ulp).float()
    return a, b, "a = -b up to a few ulps: the sum cancels before the statistics"


# ---- Gaussian head -------------------------------------------------------------------------------------------------------------
HEAD_REGIMES = ("plain", "threshold", "floor_far", "wide", "wide_overflow")
THRESHOLD_CYCLE = (-100.0, -20.0, 0.0, 19.9, 20.0, 20.1, 25.0, 80.0)
HEAD_CLAIMS = {
    "plain": "raw scale inputs randn",
    "threshold": "raw scale inputs cycle through -100, -20, 0, 19.9, 20, 20.1, 25, 80: both softplus branches and the branch point;"
                 " loc and Y are constant inside every group of 8 consecutive elements",
    "floor_far": "raw = -100 everywhere: scale = 0.01 exactly, |Y - loc| up to 50 (5000 standard deviations)",
    "wide": "raw = 80: the x > 20 branch everywhere (expf(80) is still finite in fp32)",
    "wide_overflow": "raw = 100: expf(raw) overflows fp32, only the x > 20 branch gives a number",
}


def per_group(t, group=len(THRESHOLD_CYCLE)):
    """[rows, pts, dy] with every group of ``group`` consecutive elements of a row (in the order e = t * dy + d the head walks)
    holding the value of its first element."""
    rows = t.shape[0]
    flat = t.reshape(rows, -1)
    first = (torch.arange(flat.shape[1]) // group) * group
    return flat[:, first].reshape(t.shape).contiguous()


def head_inputs(regime, rows, B, pts, dy, seed):
    """(suff fp32 [rows, pts, 2 dy], Y fp32 [B, pts, dy], claim): the raw decoder output (loc | raw scale) and the targets."""
    gen = torch.Generator().manual_seed(seed)
    loc = torch.randn(rows, pts, dy, generator=gen)
    Y = torch.randn(B, pts, dy, generator=gen)
    if regime == "plain":
        raw = torch.randn(rows, pts, dy, generator=gen)
    elif regime == "threshold":
        cyc = torch.tensor(THRESHOLD_CYCLE)
        raw = cyc[torch.arange(pts * dy) % len(cyc)].view(1, pts, dy).expand(rows, pts, dy).clone()
        loc, Y = per_group(loc), per_group(Y)
    elif regime == "floor_far":
        raw = torch.full((rows, pts, dy), -100.0)
        Y = 92.0 * torch.rand(B, pts, dy, generator=gen) - 46.0
        Y.view(-1)[0] = 46.0
    elif regime == "wide":
        raw = torch.full((rows, pts, dy), 80.0)
    elif regime == "wide_overflow":
        raw = torch.full((rows, pts, dy), 100.0)
    else:
        raise ValueError(regime)
    return torch.cat([loc, raw], -1).contiguous(), Y.contiguous(), HEAD_CLAIMS[regime]


# ---- Monte-Carlo objectives ----------------------------------------------------------------------------------------------------
MC_REGIMES = ("plain", "spread", "late_jump", "equal", "neg_inf_first", "neg_inf_some")
SPREAD = 1e4
JUMP = 200.0
MC_CLAIMS = {
    "plain": "8 randn - 100: log-likelihood sized values",
    "spread": "one sample per task 1e4 above the rest, first / middle / last by task: exp without the running maximum overflows",
    "late_jump": "non-decreasing in k with a step of 200 at n_z // 2: the running maximum moves at every sample",
    "equal": "the samples of a task are identical",
    "neg_inf_first": "log_w[0] = -inf, the rest finite",
    "neg_inf_some": "-inf at scattered k > 0, sample 0 finite",
}


def spread_index(b, n_z):
    return (0, n_z // 2, n_z - 1)[b % 3]


def neg_inf_some_mask(n_z, B):
    k, b = torch.arange(n_z).view(-1, 1), torch.arange(B).view(1, -1)
    return ((7 * k + 3 * b) % 5 == 1) & (k > 0)


def mc_log_w(regime, n_z, B, seed):
    """(log_w fp32 [n_z, B], claim)."""
    gen = torch.Generator().manual_seed(seed)
    lw = 8.0 * torch.randn(n_z, B, generator=gen) - 100.0
    if regime == "spread":
        for b in range(B):
            k = spread_index(b, n_z)
            rest = torch.cat([lw[:k, b], lw[k + 1:, b]])
            lw[k, b] = (float(rest.max()) if n_z > 1 else -100.0) + SPREAD
    elif regime == "late_jump":
        lw = -100.0 + torch.cumsum(0.1 * torch.randn(n_z, B, generator=gen).abs(), 0)
        lw[n_z // 2:] += JUMP
    elif regime == "equal":
        lw = (-100.0 + 0.125 * (torch.arange(B) % 64).float()).view(1, B).expand(n_z, B).clone()
    elif regime == "neg_inf_first":
        lw[0] = float("-inf")
    elif regime == "neg_inf_some":
        lw[neg_inf_some_mask(n_z, B)] = float("-inf")
    elif regime != "plain":
        raise ValueError(regime)
    return lw.contiguous(), MC_CLAIMS[regime]


# ---- mean ----------------------------------------------------------------------------------------------------------------------
def mean_rows(B, pts, F, seed):
    """(x fp32 [B, pts, F], claim)."""
    gen = torch.Generator().manual_seed(seed)
    return 1e4 + torch.randn(B, pts, F, generator=gen), "1e4 + randn: the partial sums grow to pts * 1e4 while the terms differ by 1"
