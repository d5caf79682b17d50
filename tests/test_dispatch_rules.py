"""The run-time dispatch rules as a table (CPU, no kernel launched).  Which kernels a train step runs depends on the model's
width r, the number of context points C, the number of target points T, the number of latent samples, the attention kind and the
compute dtype; these predicates decide it:

  fused target side   x6.target_side_usable: r = 256 -> 128 < C <= 256; r = 128 -> 1 <= C <= 128 (AttnLNP: one latent sample)
  fused context side  x6.context_side_usable: C >= 1 (padded to whole 32-point tiles), r in (128, 256)
  decoder side        x6.decoder_side_usable: r = 128 only
  decode rows         x6.decode_rows_usable: inference, F in (128, 256, 512)
  multihead kernel    functional.mha_usable: 16-feature heads C <= 256, 32-feature heads C <= 128
  one score row       DotAttender.fits_fused: C <= 256 (else the blocked softmax of attention_long.py)
  LayerNorm kernel,   functional.add_layernorm_usable, x6.mlp_pt_usable, MergeFlatInputs._x6_stack: F <= 256 / F in (128, 256) /
  MLP stacks          F = 256, fp32 only

The expected values below are the rules written out, not read back from the predicates: a change to a rule has to change this
table on purpose.  tests/test_hip_dispatch.py checks on the GPU that the launches of whole models follow the same rules."""
import pytest
import torch

from helpers import build_model

R_VALUES = (128, 256)
C_VALUES = (0, 1, 128, 129, 256, 257)
T_VALUES = (1, 70)


def _case(kind, r, **kw):
    return dict(dict(kind=kind, r=r, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=1, T=1), **kw)


_MODELS = {}


def _model(kind, r, **kw):
    """A CPU model of the test's usual shape (built once per configuration; the predicates only read its modules)."""
    key = (kind, r, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = build_model(_case(kind, r, **kw), device="cpu")
    m = _MODELS[key]
    m.train()
    return m


def _target_rule(r, C, T):
    return T > 0 and ((r == 256 and 128 < C <= 256) or (r == 128 and 1 <= C <= 128))


def _mha_rule(head, C):
    return 0 < C <= {16: 256, 32: 128}[head]


@pytest.fixture
def bf16_mode():
    from npf_gwwaveform_amd import chain as CH

    CH.set_compute_dtype("bf16")
    try:
        yield
    finally:
        CH.set_compute_dtype("fp32")


@pytest.mark.parametrize("r", R_VALUES)
def test_scaledot_attncnp_rules(r):
    from npf_gwwaveform_amd import x6

    m = _model("AttnCNP", r)
    for C in C_VALUES:
        for T in T_VALUES:
            assert m._fused_target_side(C, T) == _target_rule(r, C, T), (r, C, T)
            assert x6.target_side_usable(m, C, T) == _target_rule(r, C, T), (r, C, T)
            assert x6.decoder_side_usable(m, T) == (r == 128), (r, T)
        assert m._fused_context_side(C) == (C >= 1), (r, C)
        assert not m._xenc_with_query_projection(C, 70)
        if C > 0:
            assert m.attender.fits_fused(C) == (C <= 256), C
    # the decoder's 256 -> 256 layers (and the resizer, with the encoded targets as its addend) on the split kernel: r = 256 only
    assert (m.decoder._x6_stack() is not None) == (r == 256)
    assert m.decoder.x6_resizer_ok() == (r == 256)
    assert x6.decoder_side_usable(m, 0) is False


@pytest.mark.parametrize("r", R_VALUES)
@pytest.mark.parametrize("n_z", (1, 8))
@pytest.mark.parametrize("q_zcct", (True, False))
def test_scaledot_attnlnp_rules(r, n_z, q_zcct):
    """AttnLNP's fused target side (the latent merge inside the program) takes one latent sample only."""
    from npf_gwwaveform_amd import x6

    m = _model("AttnLNP", r, is_q_zCct=q_zcct, n_z=n_z)
    m.n_z_samples = n_z  # (set by forward from n_z_samples_train / _test)
    for C in C_VALUES:
        for T in T_VALUES:
            assert m._fused_target_side(C, T) == (n_z == 1 and _target_rule(r, C, T)), (r, n_z, C, T)
            assert x6.target_side_usable(m, C, T, latent_merge=True) == _target_rule(r, C, T), (r, C, T)
        # the target-side latent encode of is_q_zCct runs the context-side program over the target points
        assert m._fused_context_side(C) == (C >= 1)


@pytest.mark.parametrize("r", R_VALUES + (512, 64))
def test_cnp_and_lnp_rules(r):
    from npf_gwwaveform_amd import x6

    for kind, kw in (("CNP", {}), ("LNP", dict(encoded_path="latent", n_z=4)), ("LNP", dict(encoded_path="both", n_z=1))):
        m = _model(kind, r, **kw)
        for C in C_VALUES:
            assert not m._fused_target_side(C, 70)
            assert m._fused_context_side(C) == (r in R_VALUES and C >= 1), (kind, r, C)
        assert x6.decoder_side_usable(m, 70) == (r == 128)


@pytest.mark.parametrize("attention", ("transformer", "multihead"))
@pytest.mark.parametrize("head", (16, 32))
def test_multihead_rules(attention, head):
    """8 heads of 16 (r = 128) or 32 (r = 256) features: the fused multihead kernel and the query projection fused into the
    target x-encoder while the kernel takes the context; the scaled-dot target side never (learned projections)."""
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd import x6

    r = 8 * head
    m = _model("AttnCNP", r, attention=attention)
    att = m.attender
    assert (att.n_heads, att.kq_head_size, att.value_head_size) == (8, head, head)
    for C in (1, 37, 128, 129, 255, 256, 257):
        assert FN.mha_usable(head, head, C) == _mha_rule(head, C), (head, C)
        assert m._xenc_with_query_projection(C, 70) == _mha_rule(head, C), (head, C)
        assert m._xenc_with_query_projection(C, 0) is False
        assert not m._fused_target_side(C, 70)
        assert m._fused_context_side(C)
        assert att.dot.fits_fused(C) == (C <= 256)
    assert not FN.mha_usable(head, head, 0)
    assert x6.pair_linear_usable(att.key_transform, att.value_transform)
    assert x6.decoder_side_usable(m, 70) == (r == 128)
    if attention == "transformer":
        assert FN.add_layernorm_usable(r)
        assert x6.mlp_pt_usable(att.mlp)
    else:
        assert att.post_processor is not None
    assert not FN.mha_usable(64, 64, 100) and not FN.mha_usable(8, 8, 100) and not FN.mha_usable(16, 32, 100)
    assert not FN.add_layernorm_usable(320) and not FN.add_layernorm_usable(30)


@pytest.mark.parametrize("F", (64, 96, 128, 256, 512))
@pytest.mark.parametrize("T", (0, 1, 70))
def test_decode_rows_rule(F, T):
    from npf_gwwaveform_amd import x6

    m = _model("CNP", F)
    x1, x2 = torch.empty(2, T, F), torch.empty(2, T, F)
    assert x6.decode_rows_usable(m.decoder, x1, x2) == (F in (128, 256, 512) and T > 0), (F, T)
    assert not x6.decode_rows_usable(m.decoder, x1, torch.empty(2, T, F // 2))


@pytest.mark.parametrize("r,C", ((256, 200), (128, 64)))
@pytest.mark.parametrize("variant", (dict(is_res=True), dict(dropout=0.25), dict(x_transf_dim=64)))
def test_variants_leave_the_fused_sides(r, C, variant):
    """Residual layers, active dropout and x_transf_dim != r are off every fused side; dropout only while it is active."""
    from npf_gwwaveform_amd import x6

    base = _model("AttnCNP", r)
    assert base._fused_target_side(C, 70) and base._fused_context_side(C)
    for kind in ("AttnCNP", "AttnLNP"):
        m = _model(kind, r, **variant)
        m.n_z_samples = 1
        assert not m._fused_target_side(C, 70), (kind, variant)
        assert not m._fused_context_side(C), (kind, variant)
        assert not x6.decoder_side_usable(m, 70), (kind, variant)
        assert m.decoder._x6_stack() is None or r != 256 or "x_transf_dim" in variant
        if "dropout" in variant:
            m.eval()
            assert m._fused_target_side(C, 70) and m._fused_context_side(C)
            assert x6.decoder_side_usable(m, 70) == (r == 128)
            m.train()


def test_bf16_mode_rules(bf16_mode):
    """The bf16 compute mode: the fused sides as b16 programs wherever the fp32 mode has them (x6._mode_ok); no multihead
    kernel, no LayerNorm kernel, no MLP-block / decoder-side / decode-rows program, no split-kernel stack."""
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd import x6

    assert x6._mode_ok()
    for r in R_VALUES:
        m = _model("AttnCNP", r)
        lnp = _model("AttnLNP", r, is_q_zCct=True, n_z=1)
        lnp.n_z_samples = 1
        for C in C_VALUES:
            for T in T_VALUES:
                assert m._fused_target_side(C, T) == _target_rule(r, C, T), (r, C, T)
                assert lnp._fused_target_side(C, T) == _target_rule(r, C, T), (r, C, T)
                assert not x6.decoder_side_usable(m, T)
            assert m._fused_context_side(C) == (C >= 1)
        assert m.decoder._x6_stack() is None and not m.decoder.x6_resizer_ok()
        assert not x6.decode_rows_usable(m.decoder, torch.empty(2, 70, r), torch.empty(2, 70, r))
        for head in (16, 32):
            for C in (1, 128, 129, 256, 257):
                assert not FN.mha_usable(head, head, C)
        assert not FN.add_layernorm_usable(r)
        t = _model("AttnCNP", r, attention="transformer")
        assert not x6.mlp_pt_usable(t.attender.mlp)
        assert not x6.pair_linear_usable(t.attender.key_transform, t.attender.value_transform)
        assert not t._xenc_with_query_projection(100, 70)


def test_bf16_fixture_restores_fp32():
    from npf_gwwaveform_amd import chain as CH

    assert CH.COMPUTE_DTYPE == "fp32"


def test_launch_witness_counts_and_restores():
    """The witness of tests/helpers.py (no kernel runs: calls the library refuses before launching)."""
    import ctypes

    from helpers import launch_witness
    from npf_gwwaveform_amd import _build
    from npf_gwwaveform_amd import _lib as L

    _build.build()  # (a no-op when the library is up to date)
    real = L.load()
    with launch_witness() as w:
        assert L.load().npf_version() >= 1
        prog = L.NpfProgram()
        prog.n_ops, prog.n_tasks, prog.pts_per_task, prog.tiles_per_task = 1, 1, 40, 1
        assert L.load().npf_chain_run(ctypes.byref(prog), None) == -1
        assert L.load().npf_chain_run(ctypes.byref(prog), None) == -1
    assert L._lib is real
    assert w["npf_version"] == 1 and w["npf_chain_run"] == 2 and w["npf_x6_run_ex"] == 0
    with pytest.raises(RuntimeError):
        with launch_witness(spy=("attention_long.long_scaledot_attention",)):
            raise RuntimeError("boom")
    from npf_gwwaveform_amd import attention_long

    assert L._lib is real and attention_long.long_scaledot_attention.__name__ == "long_scaledot_attention"
