"""Whole models on both sides of every dispatch boundary (tests/test_dispatch_rules.py states the rules), against the CPU oracle,
with the path each case took recorded by the launch witness of tests/helpers.py.

Per case: one train step (forward, loss, backward) at the gates of tests/test_hip_sweep.py -- loc / scale 1e-5 of max|ref|, the
loss to rtol 2e-5, EVERY gradient tensor in full at 1e-4 of max|ref|, the latent samples and both latent distributions where the
model has them --, an evaluation-mode forward without targets (no_grad: the inference branches of the fused programs), and at the
widths of the decode-rows program (128 / 256) the stage API ``decode`` (inference: merge + decoder + output layer as one program
from row-major tensors; ``forward`` never takes that path, training or not).

The expected path of each case is derived from the rules here (``_expected``), not from what a run printed: which side functions
of x6.py / functional.py / attention_long.py run and how often, and from that the entry points of the library -- every x6 program
function is one ``npf_x6_run_ex`` launch forward and one for its dgrad, a fully fused AttnCNP step runs no chain launch, the split
kernel (``npf_mlp_x6_run*``) serves the 256-wide decoder whenever the target side is not fused."""
import gc

import numpy as np
import pytest
import torch

import specs
from helpers import EpsIndependent, assert_close, build_loss, build_model, launch_witness
from oracle import npf_oracle as O
from test_hip_sweep import _oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SPY = ("x6.target_side", "x6.context_side", "x6.decoder_side", "x6.xenc_proj", "x6.pair_linear", "x6.mlp_pt", "x6.decode_rows",
       "functional.mha", "attention_long.long_scaledot_attention")
X6_FUNCS = ("x6.target_side", "x6.context_side", "x6.decoder_side", "x6.xenc_proj", "x6.pair_linear", "x6.mlp_pt")


def _c(kind, r, C, **kw):
    return dict(dict(kind=kind, r=r, C=C, B=2, dx=1, dy=2, L_xy=2, L_dec=2, T=70), **kw)


CASES = {}
for _C in (1, 128, 129, 256, 257):
    CASES[f"attncnp_r256_c{_C}"] = _c("AttnCNP", 256, _C)
CASES["attncnp_r256_c129_t1"] = _c("AttnCNP", 256, 129, T=1)
CASES["attncnp_r256_c129_t257"] = _c("AttnCNP", 256, 129, T=257)
for _C in (0, 1, 128, 129):
    CASES[f"attncnp_r128_c{_C}"] = _c("AttnCNP", 128, _C)
for _C in (128, 129, 256, 257):
    CASES[f"attnlnp_r256_c{_C}"] = _c("AttnLNP", 256, _C, is_q_zCct=True, n_z=1)
CASES["attnlnp_r256_c200_nz8"] = _c("AttnLNP", 256, 200, is_q_zCct=True, n_z=8)
CASES["attnlnp_r256_c200_nz32_t33"] = _c("AttnLNP", 256, 200, is_q_zCct=True, n_z=32, T=33)
CASES["attnlnp_r256_c200_noq"] = _c("AttnLNP", 256, 200, is_q_zCct=False, n_z=1)
for _C in (1, 128, 129):
    CASES[f"attnlnp_r128_c{_C}"] = _c("AttnLNP", 128, _C, is_q_zCct=True, n_z=1)
for _C in (1, 37, 128, 129):  # 32-feature heads
    CASES[f"attncnp_r256_transformer_c{_C}"] = _c("AttnCNP", 256, _C, attention="transformer")
CASES["attnlnp_r256_transformer_c128"] = _c("AttnLNP", 256, 128, attention="transformer", is_q_zCct=True, n_z=1)
CASES["attnlnp_r256_transformer_c128_nz4"] = _c("AttnLNP", 256, 128, attention="transformer", is_q_zCct=True, n_z=4)
CASES["attnlnp_r128_transformer_c33"] = _c("AttnLNP", 128, 33, attention="transformer", is_q_zCct=True, n_z=1)  # decoder side + zb
for _C in (256, 257):  # 16-feature heads
    CASES[f"attncnp_r128_transformer_c{_C}"] = _c("AttnCNP", 128, _C, attention="transformer")
CASES["attncnp_r256_multihead_c128"] = _c("AttnCNP", 256, 128, attention="multihead")
CASES["attncnp_r256_multihead_c129"] = _c("AttnCNP", 256, 129, attention="multihead")
CASES["attncnp_r128_multihead_c256"] = _c("AttnCNP", 128, 256, attention="multihead")
for _C in (1, 32, 33, 257):
    CASES[f"cnp_r256_c{_C}"] = _c("CNP", 256, _C)
CASES["lnp_latent_r256_c33_nz4"] = _c("LNP", 256, 33, encoded_path="latent", is_q_zCct=True, n_z=4)


def _expected(case, training=True):
    """The side functions a forward of ``case`` runs, from the dispatch rules (tests/test_dispatch_rules.py)."""
    kind, r, C, T = case["kind"], case["r"], case["C"], case["T"]
    n_z, att = case.get("n_z", 1), case.get("attention", "scaledot")
    latent, attentive = kind in ("LNP", "AttnLNP"), kind in ("AttnCNP", "AttnLNP")
    wide = r in (128, 256)
    heads = att != "scaledot"
    head = r // 8
    mha = heads and 0 < C <= {16: 256, 32: 128}.get(head, 0)
    fused_t = (attentive and not heads and (n_z == 1 or kind == "AttnCNP")
               and ((r == 256 and 128 < C <= 256) or (r == 128 and 1 <= C <= 128)))
    q_zcct = latent and case.get("is_q_zCct", False) and training  # (the evaluation forward passes no targets)
    e = dict.fromkeys(SPY, 0)
    e["x6.target_side"] = int(fused_t)
    # the context points; with the target side fused, the target-side latent encode is the context program over the targets
    e["x6.context_side"] = int(wide and C >= 1) + int(wide and fused_t and q_zcct)
    e["functional.mha"] = int(mha)
    e["x6.xenc_proj"] = e["x6.pair_linear"] = int(mha and wide)
    e["x6.mlp_pt"] = int(att == "transformer" and C > 0 and wide)
    e["x6.decoder_side"] = int(heads and C > 0 and r == 128 and n_z == 1)
    e["attention_long.long_scaledot_attention"] = int(attentive and not mha and C > 256)
    return e


def _check_path(w, case, training=True):
    e = _expected(case, training)
    got = {k: w[k] for k in SPY}
    assert got == e, f"path: got {got}\nexpected {e}\n{w}"
    n_x6 = sum(e[k] for k in X6_FUNCS) * (2 if training else 1)  # (one launch forward, one for the dgrad)
    assert w["npf_x6_run_ex"] == n_x6, w
    assert w["npf_mha_fwd"] == e["functional.mha"] and w["npf_mha_bwd"] == (e["functional.mha"] if training else 0), w
    assert w["npf_b16_run"] == 0 and w["npf_x6_run"] == 0, w
    if e["functional.mha"] == 0 and case.get("attention", "scaledot") != "scaledot" and case["C"] > 0:
        assert w["npf_split_heads"] > 0 and w["npf_merge_heads"] > 0, w  # (heads as extra tasks of the chain kernel)
    else:
        assert w["npf_split_heads"] == 0 and w["npf_merge_heads"] == 0, w
    n_split = w["npf_mlp_x6_run"] + w["npf_mlp_x6_run_rows"]
    assert (n_split > 0) == (case["r"] == 256 and not e["x6.target_side"]), w
    # no chain launch at all: AttnCNP with the fused target side, or with transformer attention on the multihead / LayerNorm kernels
    # in front of the decoder-side program; every other step has chain launches (latent path, attention, decoder, x-encoder)
    no_chain = case["kind"] == "AttnCNP" and (e["x6.target_side"] or (case.get("attention") == "transformer"
                                                                       and e["functional.mha"] and e["x6.decoder_side"]))
    assert (w["npf_chain_run"] == 0) == bool(no_chain), w


def _train_step(case, params, inp, w_spy=SPY):
    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    if "eps" in dinp:
        EpsIndependent.eps = dinp["eps"]
    crit = build_loss(case)
    model.train()
    crit.train()
    with launch_witness(spy=w_spy) as w:
        out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
        loss = crit(out, dinp["Y_trgt"])
        loss.backward()
        torch.cuda.synchronize()
    return model, out, loss, w


def _compare_outputs(out, ref, what=""):
    assert_close(out[0].base_dist.loc, ref["loc"], what=f"loc {what}")
    assert_close(out[0].base_dist.scale, ref["scale"], what=f"scale {what}")
    np.testing.assert_allclose(out[0].base_dist.scale.detach().cpu().numpy(), ref["scale"].detach().numpy(), rtol=1e-5)
    if out[1] is not None or ref["z_samples"] is not None:
        assert_close(out[1], ref["z_samples"], what=f"z_samples {what}")
    for i, key in ((2, "q_zCc"), (3, "q_zCct")):
        assert (out[i] is None) == (ref[key] is None), key
        if out[i] is not None:
            assert_close(out[i].base_dist.loc, ref[key][0], what=f"{key}.loc {what}")
            assert_close(out[i].base_dist.scale, ref[key][1], what=f"{key}.scale {what}")


def _compare_grads(model, ref_p, what=""):
    refs = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in ref_p.items()}
    for k, p in model.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        if float(refs[k].abs().max()) == 0.0:
            # an exactly zero gradient (one context point: its attention weight is 1 whatever the key projection, so that
            # projection's gradient vanishes): the relative gate has no scale, take that of the module's other gradients
            scale = max(float(v.abs().max()) for j, v in refs.items() if j.split(".")[0] == k.split(".")[0])
            err = float(got.detach().abs().max())
            assert err <= 1e-4 * scale, f"grad {k} {what}: max|d|={err:.3e} > 1e-04 * {scale:.3e} (module scale, zero reference)"
        else:
            assert_close(got, refs[k], tol=1e-4, what=f"grad {k} {what}")


@pytest.mark.parametrize("name", list(CASES))
def test_dispatch_boundary_matches_oracle(name):
    case = CASES[name]
    params = specs.make_params(case, seed=11)
    inp = specs.make_inputs(case, seed=4321)
    n_z = case.get("n_z", 1)

    # train step
    ref_p, ref_out, ref_loss = _oracle(case, inp, params)
    model, out, loss, w = _train_step(case, params, inp)
    _compare_outputs(out, ref_out)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=2e-5)
    _compare_grads(model, ref_p)
    _check_path(w, case, training=True)

    # evaluation-mode forward, no targets
    model.eval()
    with torch.no_grad(), launch_witness(spy=SPY) as we:
        out_e = model(*(inp[k].to(DEV) for k in ("X_cntxt", "Y_cntxt", "X_trgt")))
        torch.cuda.synchronize()
    ref_e = O.forward(specs.cfg_of(case), params, inp["X_cntxt"], inp["Y_cntxt"], inp["X_trgt"], None, eps=inp.get("eps"), n_z=n_z,
                      training=False)
    _compare_outputs(out_e, ref_e, what="(eval)")
    _check_path(we, case, training=False)

    # the decode stage at inference (decode-rows program) where its width is covered
    if n_z == 1 and case["r"] in (128, 256):
        with torch.no_grad(), launch_witness(spy=SPY) as wd:
            p = model.decode(ref_e["Xt_enc"].to(DEV), ref_e["R_trgt"].to(DEV))
            torch.cuda.synchronize()
        loc, scale = O.decode(specs.cfg_of(case), params, ref_e["Xt_enc"], ref_e["R_trgt"])
        assert_close(p.base_dist.loc, loc, what="decode loc")
        assert_close(p.base_dist.scale, scale, what="decode scale")
        assert wd["x6.decode_rows"] == 1 and wd["npf_x6_run_ex"] == 1 and wd["npf_chain_run"] == 0, wd


@pytest.mark.parametrize("r,c_lo,c_hi", [(256, 128, 129), (128, 128, 129), (256, 256, 257)])
def test_launch_counts_change_at_the_target_side_switch(r, c_lo, c_hi):
    """AttnCNP one context point apart on both sides of a switch of the fused target side: the fused side adds exactly its two
    program launches (forward, dgrad) and takes every chain launch of the target side away; the context side is a program on
    both sides."""
    ws = {}
    for C in (c_lo, c_hi):
        case = _c("AttnCNP", r, C)
        ws[C] = _train_step(case, specs.make_params(case, seed=11), specs.make_inputs(case, seed=4321))[3]
    fused = {C: (r == 256 and 128 < C <= 256) or (r == 128 and 1 <= C <= 128) for C in (c_lo, c_hi)}
    assert fused[c_lo] != fused[c_hi]
    on, off = (c_lo, c_hi) if fused[c_lo] else (c_hi, c_lo)
    assert ws[on]["npf_x6_run_ex"] == ws[off]["npf_x6_run_ex"] + 2, ws
    assert ws[on]["npf_chain_run"] == 0 < ws[off]["npf_chain_run"], ws


# ---- BASELINE configurations at batch 2 (bench.py's shapes): which kernels the flagship steps run
def test_config2_step_runs_no_chain_launch():
    case = specs.CASES["g3_attncnp_c2"]
    w = _train_step(case, specs.make_params(case), specs.make_inputs(case))[3]
    assert w["npf_chain_run"] == 0 and w["x6.target_side"] == 1 and w["x6.context_side"] == 1, w
    assert w["npf_x6_run_ex"] == 4, w


def test_config3_bf16_step_runs_b16_programs_and_no_chain_launch():
    from npf_gwwaveform_amd import chain as CH

    case = specs.CASES["g3_attncnp_c2"]
    CH.set_compute_dtype("bf16")
    try:
        w = _train_step(case, specs.make_params(case), specs.make_inputs(case))[3]
    finally:
        CH.set_compute_dtype("fp32")
    assert w["npf_b16_run"] > 0 and w["npf_chain_run"] == 0 and w["npf_x6_run_ex"] == 0, w
    assert w["x6.target_side"] == 1 and w["x6.context_side"] == 1, w


def test_config5_decode_is_one_program():
    case = dict(kind="CNP", r=specs.DECODE_CASE["r"], L_xy=2, L_dec=specs.DECODE_CASE["L_dec"], dx=1, dy=2, B=2, C=1, T=1)
    params = specs.make_params(case, seed=5)
    model = build_model(case, DEV, params=params).eval()
    inp = specs.make_decode_inputs()
    with torch.no_grad(), launch_witness(spy=SPY) as w:
        p = model.decode(inp["X_trgt_enc"].to(DEV), inp["R_trgt"].to(DEV))
        torch.cuda.synchronize()
    loc, scale = O.decode(specs.cfg_of(case), params, inp["X_trgt_enc"], inp["R_trgt"])
    assert_close(p.base_dist.loc, loc, what="decode loc")
    assert_close(p.base_dist.scale, scale, what="decode scale")
    assert w["npf_x6_run_ex"] >= 1 and w["x6.decode_rows"] == 1, w
    assert w["npf_chain_run"] == 0 and w["npf_mlp_x6_run"] == 0 and w["npf_mlp_x6_run_rows"] == 0, w


# AttnLNP at config-2 sizes: the target side is one fused program, but the latent path (z half of merge_r_z, latent encoder over
# the pooled context and target representations, their backward) still runs as chain launches.  Pinned, so that folding it into
# the programs changes this number on purpose.
ATTNLNP_C2_CHAIN_LAUNCHES = 14


def test_attnlnp_config2_latent_path_chain_launches_are_pinned():
    case = specs.CASES["g4_attnlnp_c2"]
    w = _train_step(case, specs.make_params(case), specs.make_inputs(case))[3]
    assert w["x6.target_side"] == 1 and w["x6.context_side"] == 2 and w["npf_x6_run_ex"] == 6, w
    assert w["npf_chain_run"] == ATTNLNP_C2_CHAIN_LAUNCHES, w


# ---- several steps crossing the boundaries: nothing a path caches (zero blocks, task images, per-shape buffers) leaks into the next
STEPS = {
    "attnlnp_r256": (_c("AttnLNP", 256, 1, is_q_zCct=True, n_z=1),
                     [(1, 70), (64, 33), (128, 100), (129, 70), (200, 45), (256, 64), (257, 70), (300, 31), (129, 257),
                      (128, 70), (1, 1), (256, 96)]),
    "attncnp_r128": (_c("AttnCNP", 128, 1),
                     [(1, 70), (50, 33), (128, 100), (129, 70), (0, 45), (128, 64), (1, 1), (129, 257), (64, 70), (0, 31),
                      (128, 96), (1, 70)]),
}


@pytest.mark.parametrize("name", list(STEPS))
def test_steps_across_the_boundaries_track_the_oracle(name):
    """Adam steps with a new (C, T) every step, across the fused / chain / blocked switches, garbage collection and allocator
    churn in between: forward outputs, the loss and every gradient against the oracle on the model's current parameters."""
    base, plan = STEPS[name]
    model = build_model(base, DEV, params=specs.make_params(base, seed=21))
    crit = build_loss(base)
    model.train()
    crit.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    rng = np.random.Generator(np.random.Philox(7))
    seen = set()
    for step, (C, T) in enumerate(plan):
        case = dict(base, C=C, T=T)
        inp = specs.make_inputs(case, seed=700 + step)
        params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        ref_p, ref_out, ref_loss = _oracle(case, inp, params)
        dinp = {k: v.to(DEV) for k, v in inp.items()}
        if "eps" in dinp:
            EpsIndependent.eps = dinp["eps"]
        opt.zero_grad(set_to_none=True)
        with launch_witness(spy=SPY) as w:
            out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
            loss = crit(out, dinp["Y_trgt"])
            loss.backward()
        what = f"step {step} (C={C}, T={T})"
        _compare_outputs(out, ref_out, what=what)
        np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=2e-5, err_msg=what)
        _compare_grads(model, ref_p, what=what)
        _check_path(w, case, training=True)
        seen.add((w["x6.target_side"], w["attention_long.long_scaledot_attention"]))
        opt.step()
        del out, loss
        gc.collect()
        junk = [torch.empty(int(rng.integers(1, 64)) * 1024, device=DEV) for _ in range(8)]  # allocator churn
        del junk
    assert (1, 0) in seen and (0, 0) in seen  # both sides of the fused target side's switch
    if base["r"] == 256:
        assert (0, 1) in seen  # and the blocked softmax
