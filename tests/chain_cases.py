"""Programs, float64 reference and case tables of the chain-interpreter edge tests (tests/test_hip_chain_edges.py, checked on the
CPU by tests/test_chain_cases_host.py).  Not a test module.

A *program* is a list of ``(kind, attrs)`` steps that mirrors the builders of ``npf_gwwaveform_amd.chain.Chain``; its operands are
named entries of a dict of row-major CPU tensors (points ``[n_tasks, pts, F]``, weights ``[N, K]``, keys / values
``[n_tasks, C, F]``, per-task vectors ``[rows, F]``).  ``reference`` evaluates it in plain torch: float64 is the reference, float32
the plain evaluation the host test uses to prove that an input is fair (its own error stays within half the gate).

``slab_class`` and ``expected_instance`` restate, in Python, two decisions of csrc/chain_kernel.hip: the stream class of a LINEAR's
weight slabs (``make_slab_op`` / ``slab_fast_setup``) and the kernel instance ``npf_chain_run`` launches.  They exist to prove that
the tables below inhabit every class, and to be compared with ``npf_chain_instance`` on the GPU.

Gates (u = 2**-24):
  * one linear layer, y and dX, per element: |d| <= (K + 2) u (sum_k |W_ik| |x_k| + |b_i|), the worst-case bound of a length-K dot
    product in any summation order (one rounding per product, K - 1 additions, the bias addition, one spare); for dX the
    contraction runs over the N outputs.  Every element also meets the project gate 1e-5 max|ref|;
  * dW, db, multi-layer programs, attention chains: max|d| <= 1e-5 max|ref| per tensor;
  * the softmax op on crafted rows: |p - p_ref| <= u (2 |a_c| + n + SOFTMAX_C) p_ref with a_c = (s_c - max) scale, see
    ``softmax_gate``.
"""
import math

import torch

U = 2.0 ** -24
TOL = 1e-5
N_TASKS = 3

W_ROWMAJOR, W_PT_ROWS, W_PT_COLS = range(3)
BF16, EXTRA, WIDE, PAIRED, N128, DEFAULT = range(1, 7)   # npf_chain_instance (include/npf_hip.h)
INSTANCE_NAMES = {BF16: "bf16", EXTRA: "extra", WIDE: "wide", PAIRED: "paired", N128: "n128", DEFAULT: "default", -1: "EINVAL"}


def pad32(n):
    return (n + 31) // 32 * 32


# ---- PT32 layout, stated by index (include/npf_hip.h): element [task, tile, f // 4, p, f % 4] = rows[task, 32 tile + p, f] ----------
def to_pt_ref(rows, fill=0.0):
    """Row-major [n_tasks, pts, F] -> PT32; padding points and features hold ``fill``."""
    n_tasks, pts, F = rows.shape
    tiles, Fp = (pts + 31) // 32, pad32(F)
    buf = torch.full((n_tasks, tiles * 32, Fp), fill, dtype=rows.dtype)
    buf[:, :pts, :F] = rows
    return buf.view(n_tasks, tiles, 32, Fp // 4, 4).permute(0, 1, 3, 2, 4).contiguous()


def from_pt_ref(pt, pts, F):
    """PT32 -> row-major [n_tasks, pts, F] (F may reach into the feature padding)."""
    n_tasks, tiles, f4, _, _ = pt.shape
    return pt.permute(0, 1, 3, 2, 4).reshape(n_tasks, tiles * 32, f4 * 4)[:, :pts, :F].contiguous()


# ---- programs ------------------------------------------------------------------------------------------------------------------------
def step(kind, **a):
    return (kind, a)


def reference(program, tensors, dtype=torch.float64, grads=(), cotangents=None):
    """Outputs of ``program`` (taps and final outputs, in order) on ``tensors`` cast to ``dtype``; with ``grads`` (operand names)
    also d(sum_j <out_j, cotangent_j>) / d(operand) by autograd, returned as a dict."""
    T = {k: v.detach().to(dtype).clone().requires_grad_(k in grads) for k, v in tensors.items()}
    cur, outs = None, []
    for kind, a in program:
        if kind in ("input_pt", "input_rows", "input_rm"):
            cur = T[a["x"]]
        elif kind == "linear":
            W = T[a["W"]]
            z = cur @ W.t()
            if a.get("b") is not None:
                b = T[a["b"]]
                z = z + (b[:, None, :] if a.get("bias_per_task") else b)
            if a.get("addend") is not None:
                z = z + T[a["addend"]]
            if a.get("relu"):
                z = z * (z > 0)  # (relu with relu'(0) = 0, torch.relu's convention; torch.clamp passes the gradient at 0)
            cur = z + cur if a.get("residual") else z
        elif kind == "add_pt":
            cur = cur + T[a["x"]]
            if a.get("relu"):
                cur = cur * (cur > 0)
        elif kind == "add_taskvec":
            v = T[a["v"]]
            idx = torch.arange(cur.shape[0]) % (a.get("modulus") or cur.shape[0])
            cur = cur + v[idx][:, None, :]
            if a.get("relu"):
                cur = cur * (cur > 0)
        elif kind == "attn_scores":
            cur = cur @ T[a["k"]].transpose(1, 2)
        elif kind == "softmax":
            z = cur * a["scale"]
            e = torch.exp(z - z.max(-1, keepdim=True).values)
            cur = e / e.sum(-1, keepdim=True)
        elif kind == "attn_values":
            cur = cur @ T[a["v"]]
        elif kind == "layernorm":
            mu = cur.mean(-1, keepdim=True)
            var = ((cur - mu) ** 2).mean(-1, keepdim=True)
            cur = (cur - mu) / torch.sqrt(var + a["eps"]) * T[a["g"]] + T[a["b"]]
        elif kind in ("output_pt", "output_rows", "tap"):
            outs.append(cur)
        else:
            raise AssertionError(kind)
    if not grads:
        return [o.detach() for o in outs], {}
    total = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cotangents))
    g = torch.autograd.grad(total, [T[k] for k in grads], allow_unused=True)
    return [o.detach() for o in outs], {k: (gi if gi is not None else torch.zeros_like(T[k])) for k, gi in zip(grads, g)}


def cotangents_for(program, tensors, seed=7):
    """One fixed cotangent per output, shaped like the float64 outputs."""
    outs, _ = reference(program, tensors)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


def linear_ops(program):
    """(K, N) of every LINEAR the forward program of ``program`` holds, from the operand shapes implied by the steps."""
    return [(a["K"], a["N"]) for kind, a in program if kind in ("linear", "attn_scores", "attn_values")]


# ---- the kernel's slab stream classes ----------------------------------------------------------------------------------------------
def slab_class(K, N, ldw, s0, ptr_aligned, mode):
    """``make_slab_op`` + ``slab_fast_setup`` of csrc/chain_kernel.hip (fp32 instances) for one LINEAR op."""
    Kp = pad32(K)
    cpr = Kp // 4
    swz = 7 if cpr & 15 else 15
    lcpr = -1 if cpr & (cpr - 1) else cpr.bit_length() - 1
    if mode == W_ROWMAJOR:
        vec16 = ldw % 4 == 0 and K % 4 == 0 and s0 % 4 == 0 and bool(ptr_aligned)
    else:
        vec16 = mode == W_PT_ROWS
    fast = vec16 and lcpr >= 0 and K == Kp and mode != W_PT_COLS
    return dict(K=K, mode=mode, Kp=Kp, cpr=cpr, swz=swz, lcpr=lcpr, vec16=vec16, fast=fast, n_slabs=(N + 31) // 32, partial_last=N % 32 != 0)


# ---- the launcher's instance choice ------------------------------------------------------------------------------------------------
FEATURE_OPS = ("load_pt", "store_pt", "add_pt", "mask_pos", "rowdot_pt", "softmax_bwd", "add_taskvec", "softmax", "store_tr", "load_rm")


def expected_instance_ops(ops, force_wg, bf16=False):
    """The rule of ``npf_chain_run`` on op triples ``(name, i0, i1)``: name in lower case without the NPF_OP_ prefix."""
    wide = any((n == "linear" and (i0 > 256 or i1 > 256)) or (n in FEATURE_OPS and i0 > 256) for n, i0, i1 in ops)
    extra = any(n in ("layernorm", "layernorm_bwd") for n, _, _ in ops)
    n256 = sum(n == "linear" and i0 == 256 and i1 == 256 for n, i0, i1 in ops)
    n128 = sum(n == "linear" and i0 == 128 and i1 == 128 for n, i0, i1 in ops)
    if extra and wide:
        return -1
    if bf16:
        return -1 if extra or wide else BF16
    if extra:
        return EXTRA
    if wide:
        return WIDE
    if force_wg == 2:
        return PAIRED
    return N128 if n128 > n256 else DEFAULT


def forward_ops(program):
    """Op triples of the forward launch ``Chain`` assembles for ``program`` (inference: no saved activations; those are STORE_PT ops
    of a width the program already has, so they never change the instance)."""
    ops, F = [], 0
    for kind, a in program:
        if kind == "input_pt":
            F = a["F"]
            ops.append(("load_pt", pad32(F), 0))
        elif kind == "input_rm":
            F = a["F"]
            ops.append(("load_rm", F, 0))
        elif kind == "input_rows":
            F = a["F"]
            ops.append(("load_rows", F, 0))
        elif kind in ("linear", "attn_scores", "attn_values"):
            if a.get("residual"):
                ops.append(("store_pt", pad32(a["K"]), 0))
            ops.append(("linear", a["K"], a["N"]))
            if a.get("residual"):
                ops.append(("add_pt", pad32(a["N"]), 0))
            F = a["N"]
        elif kind in ("add_pt", "add_taskvec"):
            ops.append((kind, pad32(F), 0))
        elif kind == "softmax":
            ops.append(("softmax", F, 0))
        elif kind == "layernorm":
            ops.append(("layernorm", F, 0))
        elif kind in ("output_pt", "tap"):
            ops.append(("store_pt", pad32(F), 0))
        elif kind == "output_rows":
            ops.append(("store_rows", F, 0))
    return ops


def expected_instance(program, force_wg):
    return expected_instance_ops(forward_ops(program), force_wg)


# ---- weight variants ---------------------------------------------------------------------------------------------------------------
# "c": contiguous [N, K]; "s16": columns 4 .. 4 + K of a [N, roundup(K, 4) + 8] matrix (16-byte aligned rows whenever K % 4 == 0);
# "s4": columns 1 .. 1 + K of a [N, K + 5] matrix: the first element is 4 bytes past a 16-byte boundary, and at K % 4 == 0 the row
# stride is odd as well -- 4-byte pieces although K % 4 == 0.
def weight_layout(K, variant):
    """(row stride, first column) of the matrix a weight variant is a column slice of."""
    if variant == "c":
        return K, 0
    if variant == "s16":
        return (K + 3) // 4 * 4 + 8, 4
    if variant == "s4":
        return K + 5, 1
    raise AssertionError(variant)


def weight_class(K, N, variant):
    ldw, off = weight_layout(K, variant)
    return slab_class(K, N, ldw, 0, off % 4 == 0, W_ROWMAJOR)


# (K, N, weight variant, bias: None / "shared" / "task")
LINEAR_CASES = (
    (1, 32, "c", None), (2, 17, "c", "shared"), (3, 4, "c", "shared"), (4, 1, "c", None), (4, 33, "s4", "shared"),
    (20, 31, "c", "shared"), (20, 64, "s16", "task"), (32, 32, "c", "shared"), (32, 65, "s4", None), (33, 64, "c", "shared"),
    (64, 256, "c", "shared"), (64, 17, "s16", "task"), (96, 33, "c", "shared"), (100, 64, "c", "task"), (100, 255, "s4", "shared"),
    (128, 128, "c", "shared"), (128, 31, "s16", None), (160, 64, "c", "shared"), (192, 32, "c", None), (224, 65, "c", "shared"),
    (255, 256, "c", "shared"), (256, 256, "c", "shared"), (256, 255, "s16", "shared"), (256, 4, "s4", None), (256, 17, "c", "task"),
    (257, 32, "c", "shared"), (320, 288, "c", "shared"), (384, 512, "c", "shared"), (512, 512, "c", None), (512, 33, "s16", "shared"),
    (64, 512, "c", "shared"), (512, 64, "s4", None),
)
LINEAR_PTS = (70, 17)
# one fast row, one generic 16-byte row, one 4-byte row: the representatives of the geometry, zero and point tests
REPRESENTATIVES = ((256, 256, "c", "shared"), (96, 33, "c", "shared"), (32, 65, "s4", None))

POINT_CASES = tuple((pts, wg) for pts in (1, 15, 16, 17, 32, 33, 70) for wg in (False, True))


def linear_program(K, N, variant, bias, inp="input_pt", out="output_pt", relu=False):
    return [step(inp, x="x", F=K), step("linear", W="W", b="b" if bias else None, K=K, N=N, variant=variant, relu=relu,
                                        bias_per_task=bias == "task"), step(out)]


def linear_tensors(K, N, bias, pts, seed=None, n_tasks=N_TASKS):
    g = torch.Generator().manual_seed(1000 * K + N if seed is None else seed)
    t = {"x": torch.randn(n_tasks, pts, K, generator=g), "W": torch.randn(N, K, generator=g) / math.sqrt(K)}
    if bias == "shared":
        t["b"] = torch.randn(N, generator=g) * 0.5
    elif bias == "task":
        t["b"] = torch.randn(n_tasks, N, generator=g) * 0.5
    return t


def dot_bound(A, B, bias=None):
    """(k + 2) u (|A| |B|^T + |bias|) for the contraction A [.., k] B [n, k] in float64."""
    k = A.shape[-1]
    mag = A.double().abs() @ B.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()
    return (k + 2) * U * mag


# ---- multi-layer sequences ---------------------------------------------------------------------------------------------------------
def _mlp(dims, g, pts, relu_last=False, variants=None, residual=(), n_tasks=N_TASKS):
    """x -> Linear(dims[0] -> dims[1]) -> relu -> ... ; weight j named W{j}, bias b{j}."""
    prog, t = [step("input_pt", x="x", F=dims[0])], {"x": torch.randn(n_tasks, pts, dims[0], generator=g)}
    for j, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
        t[f"W{j}"] = torch.randn(N, K, generator=g) / math.sqrt(K)
        t[f"b{j}"] = torch.randn(N, generator=g) * 0.1
        prog.append(step("linear", W=f"W{j}", b=f"b{j}", K=K, N=N, variant=(variants or {}).get(j, "c"),
                         relu=relu_last or j < len(dims) - 2, residual=j in residual))
    return prog, t


def _insert(prog, pos, st):
    return prog[:pos] + [st] + prog[pos:]


def make_sequence(name, pts, n_tasks=N_TASKS):
    """(program, tensors) of one SEQUENCES entry."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    kind, _, w = name.partition("@")
    w = int(w) if w else 0
    if kind == "one":
        prog, t = _mlp([w, w], g, pts)
    elif kind == "three":
        prog, t = _mlp([w, w, w, w], g, pts)
    elif kind == "gen_fast_gen":
        prog, t = _mlp([40, w, w, 17], g, pts)
    elif kind in ("fast_addpt_fast", "fast_taskvec_fast"):
        prog, t = _mlp([w, w, w], g, pts)
        prog[1][1]["relu"] = False
        if kind == "fast_addpt_fast":
            t["a"] = torch.randn(n_tasks, pts, w, generator=g)
            prog = _insert(prog, 2, step("add_pt", x="a", relu=True))
        else:
            t["v"] = torch.randn(n_tasks, w, generator=g)
            prog = _insert(prog, 2, step("add_taskvec", v="v", relu=True, modulus=0))
    elif kind == "fast_slice_fast":
        prog, t = _mlp([w, w, w, w], g, pts, variants={1: "s4"})
    elif kind == "mix_gt":      # n128 = 2 > n256 = 1
        prog, t = _mlp([128, 128, 128, 256, 256], g, pts)
    elif kind == "mix_eq":      # n128 = n256 = 1
        prog, t = _mlp([128, 128, 256, 256], g, pts)
    elif kind == "mix_lt":      # n128 = 1 < n256 = 2
        prog, t = _mlp([128, 128, 256, 256, 256], g, pts)
    elif kind == "residual":
        prog, t = _mlp([32, 128, 128, 128, 4], g, pts, residual=(1, 2))
    elif kind == "layernorm":
        prog, t = _mlp([64, 100, 64], g, pts)
        t["ln_g"] = torch.rand(100, generator=g) + 0.5
        t["ln_b"] = torch.randn(100, generator=g) * 0.1
        prog = _insert(prog, 2, step("layernorm", g="ln_g", b="ln_b", eps=1e-5))
    else:
        raise AssertionError(name)
    return prog + [step("output_pt")], t


SEQUENCES = ("one@256", "three@256", "gen_fast_gen@256", "fast_addpt_fast@256", "fast_taskvec_fast@256", "fast_slice_fast@256",
             "one@128", "three@128", "gen_fast_gen@128", "fast_addpt_fast@128", "fast_taskvec_fast@128", "fast_slice_fast@128",
             "mix_gt", "mix_eq", "mix_lt", "residual", "layernorm")
SEQUENCE_PTS = 70
WIDE_SEQUENCES = ((384, 512, 512, 2), (257, 320, 33))


def make_wide(dims, pts):
    g = torch.Generator().manual_seed(sum(dims))
    prog, t = _mlp(list(dims), g, pts)
    return prog + [step("output_pt")], t


def grad_names(program, tensors):
    """Every operand of ``program`` that carries a gradient: all but row-major inputs."""
    skip = {a["x"] for kind, a in program if kind in ("input_rows", "input_rm")}
    return [k for k in tensors if k not in skip]


# ---- attention chains --------------------------------------------------------------------------------------------------------------
# (C keys, d key width, r value width, T queries)
ATTN_CASES = ((1, 2, 32, 1), (2, 32, 100, 33), (31, 100, 256, 70), (32, 256, 32, 33), (33, 2, 100, 70), (64, 32, 256, 1),
              (255, 100, 32, 33), (256, 256, 256, 70), (256, 2, 100, 33), (33, 256, 32, 70), (64, 100, 100, 1), (255, 32, 256, 70))


def attn_program(C, d, r):
    return [step("input_pt", x="q", F=d), step("attn_scores", k="k", K=d, N=C), step("softmax", scale=1.0 / math.sqrt(d)),
            step("attn_values", v="v", K=C, N=r), step("output_pt")]


def attn_tensors(C, d, r, T, n_tasks=N_TASKS):
    g = torch.Generator().manual_seed(((C * 1000 + d) * 1000 + r) * 100 + T)
    return {"q": torch.randn(n_tasks, T, d, generator=g), "k": torch.randn(n_tasks, C, d, generator=g),
            "v": torch.randn(n_tasks, C, r, generator=g)}


def attn_slab_classes(C, d, r, T, store_tr):
    """Stream classes of the four LINEAR ops of one attention chain (forward scores / values, backward dP / dQ)."""
    ld = 32 * ((C + 31) // 32)
    vals = slab_class(C, r, ld, r * ld, True, W_ROWMAJOR) if store_tr else slab_class(C, r, 0, 0, True, W_PT_COLS)
    dq = slab_class(C, d, ld, d * ld, True, W_ROWMAJOR) if store_tr else slab_class(C, d, 0, 0, True, W_PT_COLS)
    return {"scores": slab_class(d, C, 0, 0, True, W_PT_ROWS), "values": vals, "dP": slab_class(r, C, 0, 0, True, W_PT_ROWS), "dQ": dq}


# ---- crafted softmax rows ----------------------------------------------------------------------------------------------------------
SOFTMAX_N = (1, 2, 31, 32, 33, 255, 256)
SOFTMAX_SCALE = 0.125
GARBAGE = 1e30
# The gate's constant: 8 covers expf, the reciprocal and the product.  float32 torch on the CPU stays within half the gate with it
# on every crafted row (tests/test_chain_cases_host.py prints the largest ratio), so it is not widened.
SOFTMAX_C = 8.0
SOFTMAX_KINDS = ("random", "equal", "dominant", "tie", "offset", "negative", "wide", "max_last")


def SOFTMAX_ROWS(n_valid, seed=0):
    """fp32 score rows [len(SOFTMAX_KINDS), n_valid], one per kind, in the order of SOFTMAX_KINDS."""
    g = torch.Generator().manual_seed(100 * n_valid + seed)
    n = n_valid
    rnd = lambda s=1.0: torch.randn(n, generator=g) * s  # noqa: E731
    rows = {"random": rnd(8.0), "equal": torch.full((n,), 3.25)}
    dom = rnd(4.0)
    dom[n // 2] = 400.0
    rows["dominant"] = dom
    tie = rnd(8.0)
    tie[0] = tie[n - 1] = tie.max() + 1.0
    rows["tie"] = tie
    rows["offset"] = 1e4 + rnd(8.0)
    rows["negative"] = -50.0 - rnd(8.0).abs()
    # (spread: arguments (s - max) scale below -104 underflow expf to zero -- all but a few lanes next to the maximum)
    wide = -torch.rand(n, generator=g) * 1e5 - 2000.0
    wide[:min(n, 3)] = torch.tensor([0.0, -1.5, -700.0])[:min(n, 3)]
    rows["wide"] = wide
    last = rnd(8.0)
    last[n - 1] = last.max() + 2.0
    rows["max_last"] = last
    return torch.stack([rows[k] for k in SOFTMAX_KINDS]).float()


def softmax_reference(rows, scale, m=None, total=None):
    """float64 softmax of exact fp32 rows: (p, a, max, sum) with a = (s - max) scale; ``m`` / ``total``: statistics supplied from
    outside (mode 2), taken as exact."""
    s = rows.double()
    mx = s.max(-1, keepdim=True).values if m is None else m.double().reshape(-1, 1)
    a = (s - mx) * float(torch.tensor(scale, dtype=torch.float32))
    e = torch.exp(a)
    tot = e.sum(-1, keepdim=True) if total is None else total.double().reshape(-1, 1)
    return e / tot, a, mx.reshape(-1), tot.reshape(-1)


def softmax_gate(p_ref, a, n):
    """u (2 |a| + n + SOFTMAX_C) p_ref: 2 |a| for the two roundings of the argument (the subtraction and the product with the
    scale, each a relative u of an argument whose exp has derivative exp), n for the sum of n positive terms, SOFTMAX_C for
    expf, the reciprocal and the product."""
    return U * (2 * a.abs() + n + SOFTMAX_C) * p_ref


def softmax_check(p, p_ref, a, n):
    """Largest |p - p_ref| / gate over the elements with p_ref >= 1e-36, and whether the others lie in [0, 2e-36]."""
    big = p_ref >= 1e-36
    ratio = ((p.double() - p_ref).abs() / softmax_gate(p_ref, a, n).clamp_min(1e-300))[big].max().item() if big.any() else 0.0
    tiny_ok = bool(((p[~big] >= 0) & (p[~big] <= 2e-36)).all())
    return ratio, tiny_ok
