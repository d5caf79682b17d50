"""The chain interpreter (csrc/chain_kernel.hip) at its slab, instance, cursor and value edges, against the float64 reference of
tests/chain_cases.py (whose tables, gates and fairness tests/test_chain_cases_host.py proves on the CPU).  Inputs are packed and
outputs unpacked with the index statements of chain_cases (not with ``pack_pt``); every launch's kernel instance
(``npf_chain_instance``) is compared with ``chain_cases.expected_instance_ops``.  Each test prints its worst error / gate ratio."""
import pytest
import torch

import chain_cases as CC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mods():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd import chain as CH
    return CH, L


@pytest.fixture(autouse=True)
def launched(monkeypatch):
    CH, _ = _mods()
    rec = []
    monkeypatch.setattr(CH, "LAUNCHED", rec)
    return rec


def check_instances(rec, force_wg=0):
    """Every launch recorded so far ran on the instance the restated rule expects; returns the instances."""
    _, L = _mods()
    names = {v: k[3:].lower() for k, v in vars(L).items() if k.startswith("OP_")}
    got = []
    for prog, inst in rec:
        ops = [(names[o.op], o.i0, o.i1) for o in prog.ops]
        assert inst == CC.expected_instance_ops(ops, force_wg, prog.bf16), (CC.INSTANCE_NAMES.get(inst, inst), ops, force_wg)
        got.append(inst)
    return got


# ---- running a chain_cases program on the device ---------------------------------------------------------------------------------
class Run:
    """One execution of a program: ``outs`` (row-major CPU tensors of the valid points), ``raw`` (the device outputs as returned),
    ``grads`` (name -> CPU tensor shaped like the reference operand)."""


def _pad_cols(t, width):
    out = torch.zeros(*t.shape[:-1], width)
    out[..., :t.shape[-1]] = t
    return out


def run_program(program, tensors, pts, wg_per_task, cots=None, pt_fill=0.0, store_tr=False, overrides=None):
    CH, _ = _mods()
    n_tasks = next(iter(tensors[a["x"]] for k, a in program if k.startswith("input"))).shape[0]
    want_grad = cots is not None
    leaf, view, unpack = {}, {}, {}
    T = dict(tensors, **(overrides or {}))

    def point(name, fill=0.0):  # a PT32 operand; the PT tensor itself is the autograd leaf
        if name not in leaf:
            t = T[name]
            leaf[name] = CC.to_pt_ref(t, fill).to(DEV).requires_grad_(want_grad)
            view[name] = leaf[name]
            unpack[name] = lambda g, s=t.shape: CC.from_pt_ref(g.cpu(), s[1], s[2])
        return view[name]

    def plain(name, width=None):
        if name not in leaf:
            t = T[name]
            n = t.shape[-1]
            leaf[name] = (t if width is None else _pad_cols(t, width)).to(DEV).requires_grad_(want_grad)
            view[name] = leaf[name]
            unpack[name] = lambda g, n=n: g.cpu()[..., :n]
        return view[name]

    def weight(name, variant):
        if name not in leaf:
            W = T[name]
            N, K = W.shape
            ldw, off = CC.weight_layout(K, variant)
            big = torch.full((N, ldw), float("nan"))  # (a slab piece that reads a column outside the slice poisons the result)
            big[:, off:off + K] = W
            leaf[name] = big.to(DEV).requires_grad_(want_grad)
            view[name] = leaf[name][:, off:off + K]
            assert view[name].stride(0) == ldw and (view[name].data_ptr() % 16 == 0) == (off % 4 == 0)
            unpack[name] = lambda g, off=off, K=K: g.cpu()[:, off:off + K]
        return view[name]

    def feature_major(t):  # [n_tasks, C, F] -> [n_tasks, F, 32 tiles], zero padded (what Chain.store_tr produces)
        C = t.shape[1]
        out = torch.zeros(t.shape[0], t.shape[2], CC.pad32(C))
        out[:, :, :C] = t.transpose(1, 2)
        return out.to(DEV)

    ch = CH.Chain(n_tasks, pts, DEV, wg_per_task=wg_per_task)
    kinds = []
    for kind, a in program:
        if kind == "input_pt":
            ch.input_pt(point(a["x"], pt_fill), a["F"])
        elif kind == "input_rows":
            ch.input_rows(T[a["x"]].to(DEV), a["F"])
        elif kind == "linear":
            b = None
            if a.get("b") is not None:
                b = plain(a["b"], CC.pad32(a["N"])) if a.get("bias_per_task") else plain(a["b"])
            ch.linear(weight(a["W"], a.get("variant", "c")), b, relu=bool(a.get("relu")),
                      addend=point(a["addend"]) if a.get("addend") else None, bias_per_task=bool(a.get("bias_per_task")),
                      residual=bool(a.get("residual")))
        elif kind == "add_pt":
            ch.add_pt(point(a["x"]), relu=bool(a.get("relu")))
        elif kind == "add_taskvec":
            ch.add_taskvec(plain(a["v"], CC.pad32(T[a["v"]].shape[-1])), relu=bool(a.get("relu")), modulus=a.get("modulus", 0))
        elif kind == "attn_scores":
            ch.attn_scores(point(a["k"]), a["N"], keys_tr=feature_major(T[a["k"]]) if store_tr else None)
        elif kind == "softmax":
            ch.softmax(a["scale"])
        elif kind == "attn_values":
            ch.attn_values(point(a["v"]), a["N"], values_tr=feature_major(T[a["v"]]) if store_tr else None)
        elif kind == "layernorm":
            ch.layernorm(plain(a["g"]), plain(a["b"]), a["eps"])
        elif kind in ("output_pt", "output_rows", "tap"):
            getattr(ch, kind)()
            kinds.append((kind, ch.F))
        else:
            raise AssertionError(kind)
    r = Run()
    with torch.set_grad_enabled(want_grad):
        r.raw = ch.run()
    r.outs = [CC.from_pt_ref(o.detach().cpu(), pts, F) if k != "output_rows" else o.detach().cpu() for o, (k, F) in zip(r.raw, kinds)]
    r.full = [CC.from_pt_ref(o.detach().cpu(), pts, CC.pad32(F)) if k != "output_rows" else None for o, (k, F) in zip(r.raw, kinds)]
    r.grads = {}
    if want_grad:
        total = 0
        for o, c, (k, F) in zip(r.raw, cots, kinds):
            total = total + (o * (c.to(DEV) if k == "output_rows" else CC.to_pt_ref(c).to(DEV))).sum()
        total.backward()
        torch.cuda.synchronize()
        r.grads = {n: unpack[n](leaf[n].grad) for n in leaf if leaf[n].grad is not None}
    return r


def tensor_ratio(got, ref, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    return (got.double() - ref).abs().max().item() / (CC.TOL * max(ref.abs().max().item(), 1e-30))


def check_program(program, tensors, pts, wg, what, store_tr=False):
    """Forward result and every gradient of a program against float64 at the project gate; returns (worst ratio, Run)."""
    names = CC.grad_names(program, tensors)
    cots = CC.cotangents_for(program, tensors)
    outs, grads = CC.reference(program, tensors, torch.float64, names, cots)
    r = run_program(program, tensors, pts, wg, cots=cots, store_tr=store_tr)
    ratios = {f"out{j}": tensor_ratio(o, ref, f"{what} out{j}") for j, (o, ref) in enumerate(zip(r.outs, outs))}
    for n in names:
        assert n in r.grads, f"{what}: no gradient for {n}"
        ratios[f"d{n}"] = tensor_ratio(r.grads[n], grads[n], f"{what} d{n}")
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{what}: {worst} misses the gate 1e-5 max|ref| by a factor {ratios[worst]:.3g}; all: {ratios}"
    return ratios[worst], r


# ---- a single layer at every slab class ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", CC.LINEAR_PTS)
@pytest.mark.parametrize("case", CC.LINEAR_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}")
def test_single_layer_at_every_slab_class(case, pts, launched):
    K, N, variant, bias = case
    wg = bias == "task"
    prog = CC.linear_program(K, N, variant, bias)
    t = CC.linear_tensors(K, N, bias, pts)
    names = CC.grad_names(prog, t)
    cots = CC.cotangents_for(prog, t)
    (y64,), g64 = CC.reference(prog, t, torch.float64, names, cots)
    r = run_program(prog, t, pts, wg, cots=cots)
    b = t.get("b")
    by = CC.dot_bound(t["x"], t["W"], None if b is None else (b[:, None, :] if bias == "task" else b))
    bx = CC.dot_bound(cots[0], t["W"].t())
    el_y = ((r.outs[0].double() - y64).abs() / by).max().item()
    el_x = ((r.grads["x"].double() - g64["x"]).abs() / bx).max().item()
    ten = {"y": tensor_ratio(r.outs[0], y64, "y")}
    ten.update({f"d{n}": tensor_ratio(r.grads[n], g64[n], f"d{n}") for n in names})
    print(f"linear {K}->{N} {variant} bias={bias} pts={pts} {CC.weight_class(K, N, variant)}: element ratio y {el_y:.3f} dX {el_x:.3f}, "
          f"tensor ratios {({k: round(v, 3) for k, v in ten.items()})}")
    assert el_y <= 1.0, f"y misses (K + 2) u (|W||x| + |b|) by a factor {el_y:.3g}"
    assert el_x <= 1.0, f"dX misses (N + 2) u |dY||W| by a factor {el_x:.3g}"
    assert max(ten.values()) <= 1.0, ten
    assert torch.count_nonzero(r.full[0][..., N:]) == 0, "feature padding of the PT output is not zero"
    if K <= 32:  # row-major input, and row-major output where it fits
        out_kind = "output_rows" if N <= 32 else "output_pt"
        r2 = run_program(CC.linear_program(K, N, variant, bias, inp="input_rows", out=out_kind), t, pts, wg)
        el2 = ((r2.outs[0].double() - y64).abs() / by).max().item()
        assert el2 <= 1.0 and tensor_ratio(r2.outs[0], y64, "rows y") <= 1.0, f"input_rows / {out_kind}: {el2:.3g}"
        assert torch.equal(r2.outs[0], r.outs[0]), "row-major and PT input disagree"
    insts = check_instances(launched)
    assert insts[0] == CC.expected_instance(prog, 0) == (CC.WIDE if max(K, N) > 256 else CC.DEFAULT if (K, N) != (128, 128) else CC.N128)


# ---- point geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", sorted({p for p, _ in CC.POINT_CASES}))
@pytest.mark.parametrize("case", CC.REPRESENTATIVES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_point_geometry(case, pts, launched):
    K, N, variant, bias = case
    prog = CC.linear_program(K, N, variant, bias, relu=True)
    t = CC.linear_tensors(K, N, bias, pts)
    worst, raws = 0.0, {}
    for p, wg in CC.POINT_CASES:
        if p != pts:
            continue
        ratio, r = check_program(prog, t, pts, wg, f"{case} pts={pts} wg_per_task={wg}")
        assert torch.count_nonzero(r.full[0][..., N:]) == 0
        worst, raws[wg] = max(worst, ratio), r
    same = torch.equal(raws[False].outs[0], raws[True].outs[0]) and all(
        torch.equal(raws[False].grads[n], raws[True].grads[n]) for n in ("x",))
    print(f"point geometry {case} pts={pts}: worst ratio {worst:.3f}; wg_per_task on/off bit-identical (y, dX): {same}")
    assert same, "valid outputs differ between wg_per_task on and off"
    check_instances(launched)


# ---- instances and the prefetch cursor -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_wg", (0, 1, 2))
@pytest.mark.parametrize("name", CC.SEQUENCES)
def test_sequences_on_every_instance(name, force_wg, launched, monkeypatch):
    CH, _ = _mods()
    prog, t = CC.make_sequence(name, CC.SEQUENCE_PTS)
    monkeypatch.setattr(CH, "FORCE_WG", force_wg)
    ratio, r = check_program(prog, t, CC.SEQUENCE_PTS, False, f"{name} FORCE_WG={force_wg}")
    insts = check_instances(launched, force_wg)
    want = CC.expected_instance(prog, force_wg)
    assert insts[0] == want and len(insts) == 2 and insts[1] == want, (insts, want)  # (forward, dgrad: the same layer shapes)
    note = ""
    if force_wg == 2:
        monkeypatch.setattr(CH, "FORCE_WG", 0)
        _, r0 = check_program(prog, t, CC.SEQUENCE_PTS, False, f"{name} default")
        same = torch.equal(r.outs[0], r0.outs[0]) and all(torch.equal(r.grads[n], r0.grads[n]) for n in r.grads)
        note = f"; paired and default bit-identical: {same}"
    print(f"{name} FORCE_WG={force_wg} on {CC.INSTANCE_NAMES[want]}: worst ratio {ratio:.3f}{note}")


@pytest.mark.parametrize("dims", CC.WIDE_SEQUENCES, ids=lambda d: "-".join(map(str, d)))
def test_wide_programs(dims, launched):
    prog, t = CC.make_wide(dims, CC.SEQUENCE_PTS)
    ratio, _ = check_program(prog, t, CC.SEQUENCE_PTS, False, f"wide {dims}")
    assert check_instances(launched) == [CC.WIDE, CC.WIDE]
    print(f"wide {dims}: worst ratio {ratio:.3f}")


# ---- attention chains ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store_tr", (False, True))
@pytest.mark.parametrize("case", CC.ATTN_CASES, ids=lambda c: "C{}-d{}-r{}-T{}".format(*c))
def test_attention_chains(case, store_tr, launched):
    C, d, r, T = case
    ratio, _ = check_program(CC.attn_program(C, d, r), CC.attn_tensors(*case), T, True, f"attention {case} store_tr={store_tr}",
                             store_tr=store_tr)
    assert check_instances(launched) == [CC.DEFAULT, CC.DEFAULT]
    print(f"attention {case} store_tr={store_tr} {CC.attn_slab_classes(*case, store_tr)['values']}: worst ratio {ratio:.3f}")


# ---- the softmax op alone --------------------------------------------------------------------------------------------------------
def _softmax_launch(x_pt, n, pts, n_tasks, mode, stats):
    CH, _ = _mods()
    out = torch.full(CH.pt_shape(n_tasks, pts, n), 7.0, dtype=torch.float32, device=DEV)
    prog = CH.Program(n_tasks, pts, False)
    prog.load_pt(x_pt, n)
    prog.softmax(n, CC.SOFTMAX_SCALE, mode=mode, stats=stats)
    prog.store_pt(out, n)
    prog.launch()
    torch.cuda.synchronize()
    return CC.from_pt_ref(out.cpu(), pts, CC.pad32(n))


@pytest.mark.parametrize("n", CC.SOFTMAX_N)
def test_softmax_op_on_crafted_rows(n, launched):
    rows = CC.SOFTMAX_ROWS(n)
    pts = rows.shape[0]
    x = torch.stack([rows, rows.flip(0)])                       # two tasks, the second with the kinds in reverse order
    n_tasks = 2
    x_pt = CC.to_pt_ref(x, fill=CC.GARBAGE).to(DEV)             # lanes >= n and padding points hold finite garbage
    p_ref, a, m_ref, s_ref = CC.softmax_reference(x.view(-1, n), CC.SOFTMAX_SCALE)
    worst = {}

    def check(p_full, p_ref, a, mode):
        p = p_full.view(-1, p_full.shape[-1])
        assert torch.isfinite(p).all()
        assert torch.count_nonzero(p[:, n:]) == 0, f"mode {mode}: lanes >= n_valid are not exactly zero"
        ratio, tiny_ok = CC.softmax_check(p[:, :n], p_ref, a, n)
        worst[mode] = ratio
        assert tiny_ok, f"mode {mode}: an element with p_ref < 1e-36 lies outside [0, 2e-36]"
        assert ratio <= 1.0, f"mode {mode}: misses u (2|a| + n + {CC.SOFTMAX_C}) p_ref by a factor {ratio:.3g}"

    # mode 0
    p0 = _softmax_launch(x_pt, n, pts, n_tasks, 0, None)
    check(p0, p_ref, a, 0)
    sum_ratio = ((p0[..., :n].double().sum(-1) - 1).abs().max() / ((n + CC.SOFTMAX_C) * CC.U)).item()
    assert sum_ratio <= 1.0, f"row sums miss 1 by {sum_ratio:.3g} (n + {CC.SOFTMAX_C}) u"
    # mode 1: the same values, and (max, sum) stored for the valid points only
    stats = torch.full((n_tasks + 1, pts, 2), -3.0, device=DEV)
    p1 = _softmax_launch(x_pt, n, pts, n_tasks, 1, stats)
    check(p1, p_ref, a, 1)
    st = stats.cpu()
    assert torch.equal(st[n_tasks], torch.full((pts, 2), -3.0)), "statistics written for points beyond pts"
    assert torch.equal(st[:n_tasks, :, 0].reshape(-1).double(), m_ref), "stored maximum differs from the row maximum"
    e_sum = torch.exp(a).sum(-1)
    stat_ratio = ((st[:n_tasks, :, 1].reshape(-1).double() - e_sum).abs() / ((n + CC.SOFTMAX_C) * CC.U * e_sum)).max().item()
    assert stat_ratio <= 1.0, f"stored sums miss by {stat_ratio:.3g} (n + {CC.SOFTMAX_C}) u"
    # mode 2: statistics of a longer row (these scores followed by a second block), supplied as fp32
    longer = torch.cat([x.view(-1, n), CC.SOFTMAX_ROWS(n, seed=1).repeat(2, 1)], dim=1)
    _, a_l, m_l, s_l = CC.softmax_reference(longer, CC.SOFTMAX_SCALE)
    stats2 = torch.stack([m_l.float(), s_l.float()], dim=-1).view(n_tasks, pts, 2).contiguous()
    p_ref2, a2, _, _ = CC.softmax_reference(x.view(-1, n), CC.SOFTMAX_SCALE, m=stats2[..., 0].reshape(-1), total=stats2[..., 1].reshape(-1))
    p2 = _softmax_launch(x_pt, n, pts, n_tasks, 2, stats2.to(DEV))
    check(p2, p_ref2, a2, 2)
    assert check_instances(launched) == [CC.DEFAULT] * 3
    print(f"softmax n_valid={n}: worst element ratio by mode {({k: round(v, 3) for k, v in worst.items()})}, row-sum ratio "
          f"{sum_ratio:.3f}, stored-sum ratio {stat_ratio:.3f}")


# ---- independence of points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("mlp", "attention"))
def test_points_are_independent(which, launched):
    pts = 70
    if which == "mlp":
        prog, t = CC.make_sequence("three@256", pts)
        src, wg = "x", False
    else:
        prog, t = CC.attn_program(33, 100, 32), CC.attn_tensors(33, 100, 32, pts)
        src, wg = "q", True
    clean = run_program(prog, t, pts, wg).outs[0]
    assert torch.isfinite(clean).all()
    # NaN in one valid point: every other point is untouched (the waves of its tile, its workgroup and its task included)
    for task, p in ((0, 0), (1, 37), (2, pts - 1)):
        bad = t[src].clone()
        bad[task, p, 1] = float("nan")
        got = run_program(prog, t, pts, wg, overrides={src: bad}).outs[0]
        keep = torch.ones(got.shape[:2], dtype=torch.bool)
        keep[task, p] = False
        assert torch.equal(got[keep], clean[keep]), f"{which}: NaN in point {(task, p)} changed another point"
        # (the poisoned point itself is not looked at: the kernel's ReLU is fmaxf(v, 0), which turns NaN into 0)
    # finite garbage in the tile-padding rows (and padding features) of the point-side input
    got = run_program(prog, t, pts, wg, pt_fill=1e30 if which == "attention" else 3.0e4).outs[0]
    if CC.pad32(t[src].shape[-1]) == t[src].shape[-1]:
        assert torch.equal(got, clean), f"{which}: garbage in the padding rows changed a valid point"
    else:  # (the fill also reaches the feature padding of valid points, which the contraction reads: fill only the rows)
        x_pt = CC.to_pt_ref(t[src])
        rows = CC.from_pt_ref(x_pt, CC.pad32(pts), x_pt.shape[2] * 4)
        rows[:, pts:, :] = 1e30
        CH, _ = _mods()
        ch = CH.Chain(CC.N_TASKS, pts, DEV, wg_per_task=True)
        ch.input_pt(CC.to_pt_ref(rows)[:, :x_pt.shape[1]].contiguous().to(DEV), 100).attn_scores(CC.to_pt_ref(t["k"]).to(DEV), 33)
        ch.softmax(prog[2][1]["scale"]).attn_values(CC.to_pt_ref(t["v"]).to(DEV), 32).output_pt()
        with torch.no_grad():
            got = CC.from_pt_ref(ch.run()[0].cpu(), pts, 32)
        assert torch.equal(got, clean), f"{which}: garbage in the padding rows changed a valid point"
    check_instances(launched)


# ---- exact values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(64, 48), (256, 256), (128, 128)])
def test_relu_at_exactly_zero(K, N, launched):
    """Integer-valued W, x, b: every product and sum is exact in fp32, so the forward result equals float64 exactly, pre-activations
    that are exactly 0 included; dX and dW follow relu'(0) = 0 exactly."""
    g = torch.Generator().manual_seed(K + N)
    pts = 33
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    W, x = ri(-2, 2, N, K), ri(-3, 3, CC.N_TASKS, pts, K)
    x[1, 5] = x[0, 0]
    x[2, 32] = x[0, 0]
    b = -(W @ x[0, 0])                      # pre-activations of those three points are exactly 0 in every feature
    t = {"x": x, "W": W, "b": b}
    prog = CC.linear_program(K, N, "c", "shared", relu=True)
    cots = [ri(-3, 3, CC.N_TASKS, pts, N)]
    z = x.double() @ W.double().t() + b.double()
    assert (z == 0).sum() >= 3 * N and (z > 0).any() and (z < 0).any()
    (y64,), g64 = CC.reference(prog, t, torch.float64, ["x", "W", "b"], cots)
    assert torch.count_nonzero(g64["x"][0, 0]) == 0   # torch's convention: no gradient through relu at 0
    r = run_program(prog, t, pts, False, cots=cots)
    assert torch.equal(r.outs[0].double(), y64), "forward result is not exact"
    for n in ("x", "W", "b"):
        assert torch.equal(r.grads[n].double(), g64[n]), f"d{n} is not exact (relu'(0) must be 0)"
    check_instances(launched)
    print(f"relu at zero {K}->{N}: {(z == 0).sum().item()} pre-activations exactly 0; y, dX, dW, db exact")


@pytest.mark.parametrize("case", CC.REPRESENTATIVES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_exact_zeros(case, launched):
    """Zero weights or zero inputs give exactly the bias."""
    K, N, variant, bias = case
    pts = 33
    t = CC.linear_tensors(K, N, bias, pts)
    prog = CC.linear_program(K, N, variant, bias)
    want = (t["b"] if bias else torch.zeros(N)).expand(CC.N_TASKS, pts, N)
    for name, zeroed in (("W", torch.zeros_like(t["W"])), ("x", torch.zeros_like(t["x"]))):
        r = run_program(prog, t, pts, False, overrides={name: zeroed})
        assert torch.equal(r.outs[0], want), f"{case}: zero {name} does not give exactly the bias"
        assert torch.count_nonzero(r.full[0][..., N:]) == 0
    check_instances(launched)
