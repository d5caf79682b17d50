"""CPU checks of tests/chain_cases.py: the float64 reference against an independent statement in torch.nn.functional, every case
fair (float32 torch within half its gate), every slab stream class and every kernel instance inhabited by the tables, the PT32
index statements, and ``expected_instance`` against ``npf_chain_instance`` (host code, needs no GPU)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import chain_cases as CC

FAIR = 0.5


# ---- PT32 by index ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 70, 100), (3, 17, 1), (3, 1, 33), (2, 33, 512), (3, 32, 257)])
def test_pt_layout_index_statement(shape):
    n_tasks, pts, Fv = shape
    rows = torch.arange(n_tasks * pts * Fv, dtype=torch.float32).view(shape) + 1
    pt = CC.to_pt_ref(rows, fill=-7.0)
    tiles, Fp = (pts + 31) // 32, CC.pad32(Fv)
    assert tuple(pt.shape) == (n_tasks, tiles, Fp // 4, 32, 4)
    g = torch.Generator().manual_seed(0)
    for _ in range(300):
        t, p, f = (int(torch.randint(0, n, (1,), generator=g)) for n in (n_tasks, tiles * 32, Fp))
        want = rows[t, p, f].item() if p < pts and f < Fv else -7.0
        assert pt[t, p // 32, f // 4, p % 32, f % 4].item() == want
    assert torch.equal(CC.from_pt_ref(pt, pts, Fv), rows)
    assert torch.equal(CC.from_pt_ref(pt, pts, Fp)[..., Fv:], torch.full((n_tasks, pts, Fp - Fv), -7.0))


# ---- the reference against torch.nn.functional -----------------------------------------------------------------------------------
def _functional(program, tensors, grads, cots):
    T = {k: v.double().clone().requires_grad_(k in grads) for k, v in tensors.items()}
    cur, outs = None, []
    for kind, a in program:
        if kind.startswith("input"):
            cur = T[a["x"]]
        elif kind == "linear":
            x = cur
            if a.get("bias_per_task"):
                z = F.linear(x, T[a["W"]]) + T[a["b"]].unsqueeze(1)
            else:
                z = F.linear(x, T[a["W"]], T[a["b"]] if a.get("b") else None)
            if a.get("addend"):
                z = z + T[a["addend"]]
            z = F.relu(z) if a.get("relu") else z
            cur = z + x if a.get("residual") else z
        elif kind == "add_pt":
            cur = cur + T[a["x"]]
            cur = F.relu(cur) if a.get("relu") else cur
        elif kind == "add_taskvec":
            cur = cur + T[a["v"]].unsqueeze(1)
            cur = F.relu(cur) if a.get("relu") else cur
        elif kind == "attn_scores":
            cur = torch.bmm(cur, T[a["k"]].transpose(1, 2))
        elif kind == "softmax":
            cur = torch.softmax(cur * a["scale"], dim=-1)
        elif kind == "attn_values":
            cur = torch.bmm(cur, T[a["v"]])
        elif kind == "layernorm":
            cur = F.layer_norm(cur, (cur.shape[-1],), T[a["g"]], T[a["b"]], a["eps"])
        else:
            outs.append(cur)
    g = torch.autograd.grad(sum((o * c.double()).sum() for o, c in zip(outs, cots)), [T[k] for k in grads])
    return outs, dict(zip(grads, g))


def _all_programs():
    yield "linear relu task-bias", CC.linear_program(100, 64, "c", "task", relu=True), CC.linear_tensors(100, 64, "task", 17)
    for name in CC.SEQUENCES:
        yield (name,) + CC.make_sequence(name, 17)
    yield ("wide",) + CC.make_wide(CC.WIDE_SEQUENCES[1], 17)
    yield "attn", CC.attn_program(33, 100, 32), CC.attn_tensors(33, 100, 32, 17)


def test_reference_agrees_with_torch_functional():
    worst = 0.0
    for name, prog, t in _all_programs():
        names = CC.grad_names(prog, t)
        cots = CC.cotangents_for(prog, t)
        outs, grads = CC.reference(prog, t, torch.float64, names, cots)
        outs2, grads2 = _functional(prog, t, names, cots)
        for what, a, b in [("out", o, o2) for o, o2 in zip(outs, outs2)] + [(k, grads[k], grads2[k]) for k in names]:
            r = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
            worst = max(worst, r)
            assert r <= 1e-13, (name, what, r)
    print(f"reference vs torch.nn.functional: worst relative difference {worst:.2e}")


# ---- fairness ----------------------------------------------------------------------------------------------------------------------
def _tensor_ratio(got, ref):
    return (got.double() - ref).abs().max().item() / (CC.TOL * max(ref.abs().max().item(), 1e-30))


def _linear_ratios(K, N, bias, pts):
    """float32 torch against float64 for one LINEAR_CASES row: (y, dX) element ratios against the dot bound, and the tensor
    ratios of y, dX, dW, db against the project gate."""
    prog = CC.linear_program(K, N, "c", bias)
    t = CC.linear_tensors(K, N, bias, pts)
    names = CC.grad_names(prog, t)
    cots = CC.cotangents_for(prog, t)
    (y64,), g64 = CC.reference(prog, t, torch.float64, names, cots)
    (y32,), g32 = CC.reference(prog, t, torch.float32, names, cots)
    b = t.get("b")
    by = CC.dot_bound(t["x"], t["W"], None if b is None else (b[:, None, :] if bias == "task" else b))
    bx = CC.dot_bound(cots[0], t["W"].t())
    el = {"y": ((y32.double() - y64).abs() / by).max().item(), "dX": ((g32["x"].double() - g64["x"]).abs() / bx).max().item()}
    ten = {"y": _tensor_ratio(y32, y64)}
    ten.update({f"d{k}": _tensor_ratio(g32[k], g64[k]) for k in names})
    return el, ten


@pytest.mark.parametrize("pts", CC.LINEAR_PTS)
def test_linear_cases_are_fair(pts):
    worst_el, worst_t = 0.0, 0.0
    for K, N, variant, bias in CC.LINEAR_CASES:
        el, ten = _linear_ratios(K, N, bias, pts)
        assert max(el.values()) <= FAIR, (K, N, bias, el)
        assert max(ten.values()) <= FAIR, (K, N, bias, ten)
        worst_el, worst_t = max(worst_el, *el.values()), max(worst_t, *ten.values())
    print(f"linear cases, pts={pts}: float32 worst element ratio {worst_el:.3f}, worst tensor ratio {worst_t:.3f}")


def _program_fair(name, prog, t):
    names = CC.grad_names(prog, t)
    cots = CC.cotangents_for(prog, t)
    o64, g64 = CC.reference(prog, t, torch.float64, names, cots)
    o32, g32 = CC.reference(prog, t, torch.float32, names, cots)
    r = {"out": max(_tensor_ratio(a, b) for a, b in zip(o32, o64))}
    r.update({k: _tensor_ratio(g32[k], g64[k]) for k in names})
    assert max(r.values()) <= FAIR, (name, r)
    return max(r.values())


def test_sequences_are_fair():
    worst = max(_program_fair(n, *CC.make_sequence(n, CC.SEQUENCE_PTS)) for n in CC.SEQUENCES)
    worst = max([worst] + [_program_fair(d, *CC.make_wide(d, CC.SEQUENCE_PTS)) for d in CC.WIDE_SEQUENCES])
    print(f"sequences: float32 worst tensor ratio {worst:.3f}")


def test_attention_cases_are_fair():
    worst = max(_program_fair(c, CC.attn_program(*c[:3]), CC.attn_tensors(*c)) for c in CC.ATTN_CASES)
    print(f"attention cases: float32 worst tensor ratio {worst:.3f}")


def test_softmax_rows_are_fair():
    worst, worst_sum = 0.0, 0.0
    for n in CC.SOFTMAX_N:
        rows = CC.SOFTMAX_ROWS(n)
        assert rows.shape == (len(CC.SOFTMAX_KINDS), n) and rows.dtype == torch.float32 and torch.isfinite(rows).all()
        p_ref, a, _, _ = CC.softmax_reference(rows, CC.SOFTMAX_SCALE)
        sc = torch.tensor(CC.SOFTMAX_SCALE, dtype=torch.float32)
        e = torch.exp((rows - rows.max(-1, keepdim=True).values) * sc)
        p32 = e * (1.0 / e.sum(-1, keepdim=True))
        for i, kind in enumerate(CC.SOFTMAX_KINDS):
            ratio, tiny_ok = CC.softmax_check(p32[i], p_ref[i], a[i], n)
            s = abs(p32[i].double().sum().item() - 1.0) / ((n + CC.SOFTMAX_C) * CC.U)
            assert ratio <= FAIR and tiny_ok and s <= FAIR, (n, kind, ratio, tiny_ok, s)
            worst, worst_sum = max(worst, ratio), max(worst_sum, s)
        # what the rows are for
        k = {name: i for i, name in enumerate(CC.SOFTMAX_KINDS)}
        assert (rows[k["equal"]] == rows[k["equal"]][0]).all()
        assert rows[k["max_last"]].argmax() == n - 1 and rows[k["negative"]].max() < 0 and rows[k["offset"]].min() > 9e3
        assert (rows[k["tie"]] == rows[k["tie"]].max()).sum() == min(n, 2)
        if n > 3:
            assert (a[k["wide"]] < -104).sum() >= n - 3 and p_ref[k["dominant"]].max() > 1 - 1e-12
    print(f"softmax rows: float32 worst element ratio {worst:.3f}, worst row-sum ratio {worst_sum:.3f} (SOFTMAX_C = {CC.SOFTMAX_C})")


# ---- the tables inhabit every slab class -----------------------------------------------------------------------------------------
def _all_linear_classes():
    """(label, class) of every LINEAR the GPU tests stream: forward and dgrad (W^T, contiguous) of every table row."""
    out = []
    for K, N, v, _ in CC.LINEAR_CASES:
        out.append((f"linear {K}->{N} {v}", CC.weight_class(K, N, v)))
        out.append((f"dgrad of {K}->{N}", CC.weight_class(N, K, "c")))
    for name in CC.SEQUENCES:
        prog, _ = CC.make_sequence(name, 17)
        out += [(f"{name} {a['K']}->{a['N']} {a['variant']}", CC.weight_class(a["K"], a["N"], a["variant"])) for k, a in prog if k == "linear"]
    for c in CC.ATTN_CASES:
        for tr in (False, True):
            out += [(f"attn {c} tr={int(tr)} {k}", cl) for k, cl in CC.attn_slab_classes(*c, tr).items()]
    return out


SLAB_CLASSES = {
    "vec16 on": lambda c: c["vec16"], "vec16 off": lambda c: not c["vec16"],
    "16-byte pieces, row a power of two": lambda c: c["vec16"] and c["lcpr"] >= 0,
    "16-byte pieces, row not a power of two": lambda c: c["vec16"] and c["lcpr"] < 0,
    "swz 7": lambda c: c["swz"] == 7, "swz 15": lambda c: c["swz"] == 15,
    "swz 15, row not a power of two": lambda c: c["swz"] == 15 and c["lcpr"] < 0,
    "fast on": lambda c: c["fast"], "fast off": lambda c: not c["fast"],
    "16-byte pieces with zero-filled columns (K < Kp)": lambda c: c["vec16"] and c["K"] < c["Kp"] and c["mode"] == CC.W_ROWMAJOR,
    "4-byte pieces at K % 4 == 0": lambda c: not c["vec16"] and c["K"] % 4 == 0 and c["mode"] == CC.W_ROWMAJOR,
    "cpr == 128, fast": lambda c: c["cpr"] == 128 and c["fast"],
    "n_slabs == 1": lambda c: c["n_slabs"] == 1,
    "partial last slab": lambda c: c["partial_last"], "partial last slab, fast": lambda c: c["partial_last"] and c["fast"],
    "full slabs only": lambda c: not c["partial_last"],
}


@pytest.mark.parametrize("name", sorted(SLAB_CLASSES))
def test_tables_inhabit_slab_class(name):
    classes = _all_linear_classes()
    hits = [label for label, c in classes if SLAB_CLASSES[name](c)]
    print(f"{name}: {len(hits)} cases, e.g. {hits[:6]}")
    assert hits, f"no case of the tables is in the slab class '{name}'"


def test_weight_modes_and_required_sizes():
    Ks, Ns = {r[0] for r in CC.LINEAR_CASES}, {r[1] for r in CC.LINEAR_CASES}
    assert Ks >= {1, 2, 3, 4, 20, 32, 33, 64, 96, 100, 128, 160, 192, 224, 255, 256, 257, 320, 384, 512}
    assert Ns >= {1, 4, 17, 31, 32, 33, 64, 65, 255, 256, 288, 512}
    assert {r[2] for r in CC.LINEAR_CASES} == {"c", "s16", "s4"} and {r[3] for r in CC.LINEAR_CASES} == {None, "shared", "task"}
    assert all(r in CC.LINEAR_CASES for r in CC.REPRESENTATIVES)
    fast, gen16, four = (CC.weight_class(*r[:3]) for r in CC.REPRESENTATIVES)
    assert fast["fast"] and gen16["vec16"] and not gen16["fast"] and not four["vec16"]
    # s16 keeps 16-byte pieces whenever K % 4 == 0, s4 never does
    for K, N, v, _ in CC.LINEAR_CASES:
        ldw, off = CC.weight_layout(K, v)
        assert ldw >= K + off
        assert CC.weight_class(K, N, v)["vec16"] == (K % 4 == 0 and v != "s4")
    assert {c[0] for c in CC.ATTN_CASES} == {1, 2, 31, 32, 33, 64, 255, 256} and {c[1] for c in CC.ATTN_CASES} == {2, 32, 100, 256}
    assert {c[2] for c in CC.ATTN_CASES} == {32, 100, 256} and {c[3] for c in CC.ATTN_CASES} == {1, 33, 70}
    assert {p for p, _ in CC.POINT_CASES} == {1, 15, 16, 17, 32, 33, 70} and {w for _, w in CC.POINT_CASES} == {False, True}
    assert any((CC.N_TASKS * ((p + 31) // 32)) % 2 == 1 and not w for p, w in CC.POINT_CASES)  # a wave without a tile


# ---- the tables inhabit every instance -------------------------------------------------------------------------------------------
def _instance_cases():
    out = []
    for name in CC.SEQUENCES:
        prog, _ = CC.make_sequence(name, 17)
        out += [(f"{name} FORCE_WG={f}", prog, f) for f in (0, 1, 2)]
    for d in CC.WIDE_SEQUENCES:
        out += [(f"wide {d} FORCE_WG={f}", CC.make_wide(d, 17)[0], f) for f in (0, 2)]
    return out


def test_tables_inhabit_every_instance():
    by = {}
    for label, prog, f in _instance_cases():
        by.setdefault(CC.expected_instance(prog, f), []).append(label)
    for inst in (CC.EXTRA, CC.WIDE, CC.PAIRED, CC.N128, CC.DEFAULT):
        print(f"{CC.INSTANCE_NAMES[inst]}: {len(by.get(inst, []))} programs, e.g. {by.get(inst, [])[:4]}")
        assert by.get(inst), f"no program of the tables runs on the {CC.INSTANCE_NAMES[inst]} instance"
    # the three mixes sit on both sides of n128 > n256, and on the boundary
    assert [CC.expected_instance(CC.make_sequence(n, 17)[0], 0) for n in ("mix_gt", "mix_eq", "mix_lt")] == [CC.N128, CC.DEFAULT, CC.DEFAULT]
    assert CC.expected_instance(CC.make_sequence("layernorm", 17)[0], 2) == CC.EXTRA      # LayerNorm wins over the paired request
    assert CC.expected_instance(CC.make_wide(CC.WIDE_SEQUENCES[0], 17)[0], 2) == CC.WIDE  # and so does a wide layer


def test_expected_instance_is_the_librarys():
    """``npf_chain_instance`` is host code: it is asked here, with dummy operand addresses, about the forward program of every
    sequence (and about programs it must reject)."""
    from npf_gwwaveform_amd import _lib as L

    assert (L.CHAIN_BF16, L.CHAIN_EXTRA, L.CHAIN_WIDE, L.CHAIN_PAIRED, L.CHAIN_N128, L.CHAIN_DEFAULT) == \
        (CC.BF16, CC.EXTRA, CC.WIDE, CC.PAIRED, CC.N128, CC.DEFAULT)
    lib = L.load()
    opcode = {k[3:].lower(): v for k, v in vars(L).items() if k.startswith("OP_")}

    def ask(ops, force_wg, bf16=0, pts=17):
        prog = L.NpfProgram()
        prog.n_ops, prog.n_tasks, prog.pts_per_task, prog.tiles_per_task = len(ops), 3, pts, (pts + 31) // 32
        prog.reserved[1], prog.reserved[2] = force_wg, bf16
        for i, (name, i0, i1) in enumerate(ops):
            o = prog.ops[i]
            o.op, o.i0, o.i1, o.p0, o.p1 = opcode[name], i0, i1, 0x10000, 0x20000
            o.i3 = i0  # (row stride of a row-major weight)
            o.f0 = 1e-5
        return lib.npf_chain_instance(C.byref(prog))

    for label, prog, f in _instance_cases():
        ops = CC.forward_ops(prog)
        assert ask(ops, f) == CC.expected_instance(prog, f) == CC.expected_instance_ops(ops, f), label
    lin = [("load_pt", 256, 0), ("linear", 256, 256), ("store_pt", 256, 0)]
    assert ask(lin, 0, bf16=1) == CC.expected_instance_ops(lin, 0, bf16=True) == CC.BF16
    bad = [("load_pt", 512, 0), ("layernorm", 100, 0)]
    assert ask(bad, 0) == CC.expected_instance_ops(bad, 0) == -1
    assert ask([("linear", 513, 4)], 0) == -1 and ask(lin, 0, pts=0) == -1
    assert lib.npf_chain_instance(None) == -1
