"""CPU-side tests: the C-ABI library loads and exports every symbol of include/npf_hip.h,
host-side module logic mirrors the reference's constructors, and the product refuses to run
without device tensors (no CPU fallback).  No kernel is launched here."""
import ctypes
import os
import re
import warnings
from functools import partial

import pytest
import torch

import specs
from oracle import npf_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(npf_[a-z_0-9]+)\s*\(", txt)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from npf_gwwaveform_amd import _build, _lib

    path = _build.build()
    assert os.path.exists(path)
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 10
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/npf_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(declared)
    assert lib.npf_version() >= 1


def test_abi_struct_sizes_match_header():
    from npf_gwwaveform_amd import _lib

    assert ctypes.sizeof(_lib.NpfOp) == 80
    assert ctypes.sizeof(_lib.NpfProgram) == 32 + 80 * 40
    assert ctypes.sizeof(_lib.NpfWgradJob) == 72
    hdr = open(os.path.join(ROOT, "include", "npf_hip.h")).read()
    assert f"#define NPF_MAX_OPS {_lib.NPF_MAX_OPS}" in hdr
    assert f"#define NPF_MAX_FEATURES {_lib.NPF_MAX_FEATURES}" in hdr


def test_invalid_programs_are_rejected_without_launching():
    from npf_gwwaveform_amd import _lib

    lib = _lib.load()
    prog = _lib.NpfProgram()
    prog.n_ops, prog.n_tasks, prog.pts_per_task, prog.tiles_per_task = 1, 1, 40, 1  # tiles must be 2
    assert lib.npf_chain_run(ctypes.byref(prog), None) == -1
    prog.tiles_per_task = 2
    prog.ops[0].op, prog.ops[0].i0, prog.ops[0].i1 = _lib.OP_LINEAR, 300, 8  # K > 256, no weights
    assert lib.npf_chain_run(ctypes.byref(prog), None) == -1
    prog.ops[0].op = 99
    assert lib.npf_chain_run(ctypes.byref(prog), None) == -1
    assert lib.npf_pack_pt(None, 1, 1, 1, None, None) == -1
    assert lib.npf_gauss_head_fwd(None, 1, 1, 1, 0, None, 0, None, None, None, None) == -1


def test_wgrad_job_split_fills_one_round_of_workgroups():
    """npf_wgrad_partials_bytes runs the launcher's host-side plan: the shared-weight jobs of a launch share
    256 workgroups (one per CU) in proportion to a per-tile cost, every job gets at least one, and a skinny
    job of the bf16 variant is priced by its bytes (not by its MFMAs: it would become the critical path)."""
    from npf_gwwaveform_amd import _lib

    lib = _lib.load()

    def splits(shapes, flags=0, n_tasks=64, tiles=32):
        """workgroups per job, recovered from the partial-slab bytes of one-job-at-a-time differences"""
        arr = (_lib.NpfWgradJob * len(shapes))()
        for j, (N, K) in enumerate(shapes):
            arr[j].dZ = arr[j].A = arr[j].dW = 4096  # (never dereferenced by the plan)
            arr[j].N, arr[j].K, arr[j].ldw, arr[j].accumulate = N, K, K, flags
        total = lib.npf_wgrad_partials_bytes(arr, len(shapes), n_tasks, tiles)
        assert total > 0
        return total

    pad = lambda v: (v + 31) // 32 * 32  # noqa: E731
    slab = lambda N, K: 4 * (pad(N) * pad(K) + pad(N))  # noqa: E731
    # identical jobs: all 256 workgroups are handed out
    assert (splits([(256, 256)] * 7) - 16) == 256 * slab(256, 256)
    assert (splits([(256, 256)] * 6, flags=2) - 16) == 256 * slab(256, 256)
    # one job alone never gets more workgroups than tiles
    assert (splits([(64, 64)], n_tasks=2, tiles=3) - 16) == 6 * slab(64, 64)
    # bf16 variant, 256x256 + skinny 4x256: the skinny job's share follows its tile bytes, 36 KiB of 64 + 36 KiB
    b = splits([(256, 256), (4, 256)], flags=2) - 16
    n_skinny = (256 * slab(256, 256) - b) // (slab(256, 256) - slab(4, 256))
    assert 85 <= n_skinny <= 100, n_skinny
    # fp32 variant: priced by MFMA time (1 of 4 wave rows busy) or bytes, whichever is larger: fewer workgroups
    f = splits([(256, 256), (4, 256)], flags=0) - 16
    n_skinny32 = (256 * slab(256, 256) - f) // (slab(256, 256) - slab(4, 256))
    assert 55 <= n_skinny32 <= 75, n_skinny32
    # invalid jobs are refused
    bad = (_lib.NpfWgradJob * 1)()
    bad[0].N, bad[0].K = 300, 8
    assert lib.npf_wgrad_partials_bytes(bad, 1, 4, 4) < 0


def _model(kind, **kw):
    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(A, kind)(1, 2, **kw)


@pytest.mark.parametrize("name", ["g1_cnp_c1", "g2_lnp_both_c1", "g2_lnp_latent_c1", "g3_attncnp_c2", "g4_attnlnp_c2"])
def test_state_dict_contract(name):
    from helpers import build_model

    case = specs.CASES[name]
    m = build_model(case, device="cpu")
    want = {f"{n}.weight": (o, i) for n, o, i in O.model_shapes(specs.cfg_of(case), case["L_xy"], case["L_dec"])}
    sd = m.state_dict()
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
        assert tuple(sd[k.replace(".weight", ".bias")].shape) == (shp[0],)
    assert len(sd) == 2 * len(want)


def test_mlp_hidden_clamp_and_init_follow_reference():
    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = A.MLP(128, 128)  # default hidden 32 -> clamped up (mlp.py:72-79)
        assert m.hidden_size == 128
        m = A.MLP(64, 64, hidden_size=256, is_force_hid_smaller=True)
        assert m.hidden_size == 64
    m = A.MLP(2, 64, hidden_size=32)
    assert m.hidden_size == 32 and len(m.linears) == 0
    m = A.MLP(256, 4, hidden_size=256, n_hidden_layers=4)
    assert [tuple(l.weight.shape) for l in m.layers()] == [(256, 256)] * 4 + [(4, 256)]
    # effective init: biases zero; hidden |w| <= 1/sqrt(fan_in); out |w| <= sqrt(6/fan_in)
    assert all(float(l.bias.detach().abs().max()) == 0 for l in m.layers())
    assert float(m.to_hidden.weight.detach().abs().max()) <= 1 / 16 + 1e-6
    assert 1 / 16 < float(m.out.weight.detach().abs().max()) <= (6 / 256) ** 0.5 + 1e-6


def test_default_architecture_matches_reference_defaults():
    m = _model("AttnLNP", r_dim=64)
    assert m.encoded_path == "both" and m.z_dim == 64 and m.n_z_samples_train == 32
    assert len(m.decoder.flat_module.linears) == 3 and len(m.xy_encoder.flat_module.linears) == 1
    assert m.decoder.resizer.hidden_size == 64 and m.xy_encoder.resizer.hidden_size == 32
    assert tuple(m.r_z_merger.weight.shape) == (64, 128)
    assert not hasattr(m, "reshaper_z")
    import npf_gwwaveform_amd as A

    xy = A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, is_force_hid_smaller=True, hidden_size=64), is_sum_merge=True)
    lnp = _model("LNP", r_dim=64, z_dim=32, XYEncoder=xy)
    assert tuple(lnp.reshaper_z.weight.shape) == (64, 32)
    # reference quirk kept on purpose: LNP's MRO resolves dflt_Modules to the latent family's
    # dict, which has no "XYEncoder" -> the reference raises KeyError('XYEncoder') for LNP(x, y)
    # without an explicit XYEncoder (np.py:62-63 with base.py:462-473); so does this package.
    with pytest.raises(KeyError, match="XYEncoder"):
        _model("LNP", r_dim=64)


def test_unsupported_configurations_fail_loudly():
    import npf_gwwaveform_amd as A

    with pytest.raises(ValueError, match="Unknown encoded_path"):
        A.CNP(1, 1, encoded_path="nope")
    with pytest.raises(ValueError, match="Unknown encoded_path"):
        A.LNP(1, 1, encoded_path="deterministic")
    with pytest.raises(NotImplementedError):
        A.AttnCNP(1, 1, attention="additive")
    with pytest.raises(ValueError, match="Unknown attention"):
        A.AttnCNP(1, 1, attention="nope")
    with pytest.raises(NotImplementedError):
        A.AttnCNP(1, 1, attention="transformer", attention_kwargs=dict(dropout=0.1))
    with pytest.raises(NotImplementedError):
        A.AttnCNP(1, 1, is_self_attn=True, self_attention_kwargs=dict(positional="absolute", position_dim=1))
    with pytest.raises(NotImplementedError):
        A.MLP(4, 4, activation=torch.nn.GELU())
    assert isinstance(A.MLP(4, 4, dropout=0.1).dropout, torch.nn.Dropout) and A.MLP(4, 4).dropout_p == 0.0
    with pytest.raises(ValueError):
        A.MLP(4, 4, dropout=1.0)
    cat = A.merge_flat_input(A.MLP, is_sum_merge=False)(8, 2, 8)   # concatenating merge: one MLP over x1 | x2
    assert not hasattr(cat, "resizer") and cat.flat_module.to_hidden.in_features == 10
    res = A.MLP(8, 8, hidden_size=8, n_hidden_layers=3, is_res=True)
    assert res.is_res and len(res.linears) == 2
    m = A.AttnCNP(1, 2, r_dim=64, x_transf_dim=32)                  # base.py:126-131
    assert m.x_encoder.out.out_features == 32 and m.decoder.resizer.out.out_features == 32
    assert m.xy_encoder.flat_module.to_hidden.in_features == 32 and m.attender.kq_size == 32
    with pytest.raises(NotImplementedError):
        A.CNP(1, 1, p_y_scale_transformer=lambda s: s)


def test_cpu_tensors_are_refused_no_fallback():
    m = _model("CNP", r_dim=32)
    x = torch.zeros(2, 4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, torch.zeros(2, 4, 2), x)
    import npf_gwwaveform_amd as A

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.MLP(4, 4)(torch.zeros(3, 4))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from npf_gwwaveform_amd import _build, _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_build, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="missing"):
        _lib.load()


def test_chain_description_and_flop_count():
    from npf_gwwaveform_amd import _lib as L
    from npf_gwwaveform_amd.chain import Chain, Program, pad32, pt_shape

    assert pad32(1) == 32 and pad32(256) == 256 and pt_shape(3, 70, 40) == (3, 3, 16, 32, 4)
    W1, W2 = torch.zeros(64, 2), torch.zeros(4, 64)
    ch = Chain(3, 70, "cpu")
    ch.input_rows(torch.zeros(3, 70, 2), 2).linear(W1, None, relu=True).linear(W2, None).output_rows()
    assert [s.kind for s in ch.steps] == ["input_rows", "linear", "linear", "output_rows"] and ch.F == 4
    with pytest.raises(ValueError):
        ch.linear(torch.zeros(8, 5), None)  # wrong fan-in
    with pytest.raises(NotImplementedError):
        Chain(1, 8, "cpu").input_pt(torch.zeros(1), 256).linear(torch.zeros(1024, 256), None)
    with pytest.raises(ValueError):
        Chain(1, 8, "cpu").input_pt(torch.zeros(1), 8).attn_scores(torch.zeros(1), 4)  # needs wg_per_task
    p = Program(3, 70, False)
    p.keep = []
    o = L.NpfOp()
    o.op, o.i0, o.i1 = L.OP_LINEAR, 2, 64
    p.ops.append(o)
    assert p.flops() == 2 * 2 * 64 * 3 * 70


def test_synthetic_batch_contract():
    from npf_gwwaveform_amd.train import synthetic_waveform_batch

    b = synthetic_waveform_batch(4, 16, 48, 7, "cpu")
    assert tuple(b["X_cntxt"].shape) == (4, 16, 1) and tuple(b["Y_trgt"].shape) == (4, 48, 2)
    for k in ("X_cntxt", "X_trgt"):
        assert float(b[k].min()) >= -1 and float(b[k].max()) <= 1  # base.py:244 contract
    assert torch.isfinite(b["Y_cntxt"]).all() and torch.isfinite(b["Y_trgt"]).all()
    b2 = synthetic_waveform_batch(4, 16, 48, 7, "cpu")
    assert torch.equal(b["Y_trgt"], b2["Y_trgt"])


def test_transformer_attention_state_dict_matches_shipped_checkpoints():
    """The shipped Attn* checkpoints' attender keys (results/pretrained/*/AttnCNP/run_0/params.pt:
    key/query/value transforms, two LayerNorms, the residual MLP) load with strict=True."""
    import warnings

    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = A.AttnCNP(1, 1, r_dim=128, attention="transformer")
    keys = {k for k in m.state_dict() if k.startswith("attender.")}
    assert keys == {"attender.key_transform.weight", "attender.query_transform.weight", "attender.query_transform.bias",
                    "attender.value_transform.weight", "attender.layer_norm1.weight", "attender.layer_norm1.bias",
                    "attender.layer_norm2.weight", "attender.layer_norm2.bias", "attender.mlp.to_hidden.weight",
                    "attender.mlp.to_hidden.bias", "attender.mlp.out.weight", "attender.mlp.out.bias"}
    assert m.attender.n_heads == 8 and m.attender.kq_head_size == 16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mh = A.AttnCNP(1, 1, r_dim=64, attention="multihead")
    assert "attender.post_processor.weight" in mh.state_dict()


def test_hot_kernel_instances_do_not_spill():
    """A source change that makes hipcc spill inside the MFMA loops fails no parity test -- it only shows
    up as a slowdown -- so the register budget of the hot instances is pinned here (compile to
    assembly, read the kernel descriptors): main chain instance, the wgrad kernels and -- what BASELINE configs 2 / 4 / 5 run on --
    the x6 program kernel's default instances (a handful of spilled registers OUTSIDE the slab loops at most: a scratch access
    inside them is a vector-memory instruction issued between the matrix instructions) and the split-once weight
    gradient kernel."""
    import subprocess
    import tempfile

    from npf_gwwaveform_amd import _build

    with tempfile.TemporaryDirectory() as tmp:
        spills = {}
        for src in ("chain_kernel.hip", "wgrad_kernel.hip", "x6_kernel.hip", "b16_kernel.hip"):
            out = os.path.join(tmp, src + ".s")
            subprocess.run([_build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                            "-I", _build.CSRC, "--cuda-device-only", "-S", os.path.join(_build.CSRC, src), "-o", out],
                           check=True, stderr=subprocess.DEVNULL)
            txt = open(out).read()
            names = re.findall(r"^\s+\.name:\s+(\S+)", txt, flags=re.M)
            counts = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", txt, flags=re.M)
            spills.update(dict(zip(names, map(int, counts))))
    main = [k for k in spills if "chain_kernelILi16ELi4ELb0ELi16ELi8" in k]
    assert len(main) == 1, spills
    assert spills[main[0]] <= 32, f"main chain_kernel instance spills {spills[main[0]]} VGPRs"
    wg = [k for k in spills if "wgrad_kernelILb" in k]
    assert len(wg) == 2 and all(spills[k] <= (16 if "ILb1E" in k else 0) for k in wg), spills
    one = lambda frag: [k for k in spills if frag in k]  # noqa: E731
    assert len(one("wgrad_h16_kernel")) == 1 and spills[one("wgrad_h16_kernel")[0]] == 0, spills
    assert len(one("wgrad_x6_kernel")) == 1 and spills[one("wgrad_x6_kernel")[0]] == 0, spills
    assert len(one("x6_wide512_kernel")) == 1 and spills[one("x6_wide512_kernel")[0]] == 0, spills
    for inst, most in (("x6_program_kernelILi256ELi1ELi8ELi2E", 8), ("x6_program_kernelILi256ELi1ELi4ELi2E", 8),
                       ("x6_program_kernelILi128ELi1ELi4ELi2E", 0), ("x6_program_kernelILi256ELi2ELi4ELi2E", 0),
                       ("x6_program_kernelILi512ELi1ELi4ELi2E", 0)):
        assert len(one(inst)) == 1 and spills[one(inst)[0]] <= most, (inst, spills)
    # the b16 program kernel (BASELINE config 3): the instances the library launches by default
    for inst, most in (("b16_program_kernelILi256ELi1ELi4ELi8ELi3E", 8), ("b16_program_kernelILi128ELi1ELi4ELi8ELi3E", 0)):
        assert len(one(inst)) == 1 and spills[one(inst)[0]] <= most, (inst, spills)


def test_index_getters_follow_reference_contract():
    """GetRandomIndcs / GetRangeIndcs / get_all_indcs (npf/utils/datasplit.py:30-145): shapes, ranges,
    per-row subsets without repetition, shared rows with is_batch_share (CPU tensors: no kernel)."""
    import npf_gwwaveform_amd as A

    assert A.get_all_indcs(3, 7).shape == (3, 7)
    assert torch.equal(A.GetRangeIndcs((2, 6))(4, 100), torch.arange(2, 6).expand(4, 4))
    g = A.GetRandomIndcs(a=0.25, b=0.5)
    for _ in range(5):
        idx = g(6, 40)
        assert idx.shape[0] == 6 and 10 <= idx.shape[1] <= 20
        assert int(idx.min()) >= 0 and int(idx.max()) < 40
        assert all(len(set(r.tolist())) == idx.shape[1] for r in idx)
    assert not torch.equal(idx[0].sort().values, idx[1].sort().values) or idx.shape[1] == 40
    shared = A.GetRandomIndcs(a=5, b=5, is_batch_share=True)(4, 30)
    assert shared.shape == (4, 5) and all(torch.equal(shared[0], r) for r in shared)
    ranged = A.GetRandomIndcs(a=3, b=3, range_indcs=(10, 20))(2, 100)
    assert ranged.shape == (2, 3) and int(ranged.min()) >= 10 and int(ranged.max()) < 20
    assert A.GetRandomIndcs(a=0, b=0, is_ensure_one=True)(2, 10).shape == (2, 1)
    with pytest.raises(ValueError):
        A.GetRandomIndcs(a=-1, b=2)(2, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.CntxtTrgtGetter()(torch.zeros(2, 10, 1), torch.zeros(2, 10, 2))


def test_trainer_checkpoint_and_lr_schedule_glue(tmp_path):
    """Checkpoint files in skorch's layout (params.pt with the reference's keys, optimizer.pt,
    history.json) and the exponential LR decay of utils/helpers.py:35-46 (CPU: no step taken)."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer, get_exponential_decay_gamma

    assert abs(get_exponential_decay_gamma(10, 100) ** 100 - 0.1) < 1e-12
    m1, m2 = _model("CNP", r_dim=32), _model("CNP", r_dim=32)
    t1, t2 = Trainer(m1, A.CNPFLoss(), lr=1e-3, world=1), Trainer(m2, A.CNPFLoss(), lr=5e-4, world=1)
    t1.set_lr_decay(10, 4)
    lrs = [t1.end_epoch() for _ in range(4)]
    assert abs(lrs[-1] - 1e-4) < 1e-12 and lrs[0] > lrs[1] > lrs[2] > lrs[3]
    t1.save_checkpoint(str(tmp_path / "ck"), history=[{"epoch": 1, "train_loss": 3.5}])
    assert sorted(os.listdir(tmp_path / "ck")) == ["history.json", "optimizer.pt", "params.pt"]
    sd = torch.load(tmp_path / "ck" / "params.pt", weights_only=True)
    assert set(sd) == set(m1.state_dict())
    assert not torch.equal(m1.decoder.flat_module.out.weight, m2.decoder.flat_module.out.weight)
    hist = t2.load_checkpoint(str(tmp_path / "ck"))
    assert hist[0]["train_loss"] == 3.5
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert t2.flat.params[0].data_ptr() == t2.flat.flat.data_ptr()  # still views of the flat buffer
    assert abs(t2.opt.param_groups[0]["lr"] - 1e-4) < 1e-12


def _cnp_like_the_shipped_checkpoint():
    import warnings
    from functools import partial

    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return A.CNP(1, 1, r_dim=128,
                     XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=256), is_sum_merge=True))


def test_optimizer_state_is_interchangeable_with_per_parameter_adam():
    """``optimizer.pt`` in skorch's layout (utils/train.py:203-221): the flat Adam state exported per parameter loads
    into a plain ``torch.optim.Adam(model.parameters())`` and both then take the same step; and back."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer

    torch.manual_seed(1)
    m1, m2 = _cnp_like_the_shipped_checkpoint(), _cnp_like_the_shipped_checkpoint()
    m2.load_state_dict(m1.state_dict())
    t1 = Trainer(m1, A.CNPFLoss(), lr=1e-3, world=1)
    ref_opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    for step in range(3):  # same synthetic gradients on both sides
        grads = [torch.randn(p.shape, generator=g) for p in m2.parameters()]
        for p, gr in zip(m2.parameters(), grads):
            p.grad = gr.clone()
        ref_opt.step()
        t1.flat.flat.grad = torch.cat([gr.reshape(-1) for gr in grads])
        t1.opt.step()
        if step == 1:  # hand the state over in both directions mid-run
            exported = t1.optimizer_state_dict()
            assert sorted(exported["state"]) == list(range(len(t1.flat.params)))
            fresh = torch.optim.Adam(m2.parameters(), lr=1e-3)
            fresh.load_state_dict(exported)          # a per-parameter Adam accepts it
            t1.load_optimizer_state_dict(ref_opt.state_dict())  # and the Trainer accepts the per-parameter one
            ref_opt = fresh
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7, msg=k)


def _write_skorch_checkpoint(dirname):
    """``params.pt`` / ``optimizer.pt`` in the layout skorch's Checkpoint wrote next to the reference's pretrained CNP
    (results/pretrained/RBF_Kernel/CNP/run_0): the model's state_dict, and the state_dict of a per-parameter Adam after a
    few steps as torch < 1.12 saved it -- state and param group keyed by ``id()`` of the parameters, ``step`` a plain int."""
    g = torch.Generator().manual_seed(7)
    model = _cnp_like_the_shipped_checkpoint()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(3):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    sd = opt.state_dict()
    ids = [id(p) for p in model.parameters()]
    sd["state"] = {ids[i]: {"step": int(s["step"]), "exp_avg": s["exp_avg"], "exp_avg_sq": s["exp_avg_sq"]}
                   for i, s in sd["state"].items()}
    sd["param_groups"][0]["params"] = ids
    torch.save(model.state_dict(), os.path.join(dirname, "params.pt"))
    torch.save(sd, os.path.join(dirname, "optimizer.pt"))
    return model


def test_shipped_skorch_optimizer_state_loads(tmp_path):
    """An ``optimizer.pt`` in the layout the reference ships next to its pretrained CNP (written by skorch's Checkpoint)
    loads into the Trainer: every parameter's moments land in its slice of the flat buffers."""
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd.train import Trainer

    saved = _write_skorch_checkpoint(str(tmp_path))
    t = Trainer(_cnp_like_the_shipped_checkpoint(), A.CNPFLoss(), lr=1e-3, world=1)
    t.load_checkpoint(str(tmp_path))
    for (k, a), (_, b) in zip(saved.state_dict().items(), t.model.state_dict().items()):
        assert torch.equal(a, b), k
    sd = torch.load(tmp_path / "optimizer.pt", map_location="cpu", weights_only=True)
    st = t.opt.state[t.flat.flat]
    for pid, p, o, n in zip(sd["param_groups"][0]["params"], t.flat.params, t.flat.offsets, t.flat.sizes):
        assert torch.equal(st["exp_avg"][o:o + n].view_as(p), sd["state"][pid]["exp_avg"])
        assert torch.equal(st["exp_avg_sq"][o:o + n].view_as(p), sd["state"][pid]["exp_avg_sq"])
    assert float(st["step"]) == float(sd["state"][sd["param_groups"][0]["params"][0]]["step"]) > 0
    assert abs(t.opt.param_groups[0]["lr"] - sd["param_groups"][0]["lr"]) < 1e-12
    back = t.optimizer_state_dict()  # (re-keyed 0 .. n-1 as current torch writes it; the shipped file is keyed by id())
    for i, pid in enumerate(sd["param_groups"][0]["params"]):
        assert torch.equal(back["state"][i]["exp_avg"], sd["state"][pid]["exp_avg"])
        assert float(back["state"][i]["step"]) == float(sd["state"][pid]["step"])
