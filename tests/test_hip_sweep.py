"""GPU parity sweep over shapes the golden vectors do not cover: the HIP models against the CPU
oracle (oracle/npf_oracle.py, itself pinned bit-exactly to the reference by tests/test_oracle.py)
on the same seeded weights and inputs.  Feature widths that are not multiples of 32 or of 4,
wider x / y, ragged context / target counts, several latent samples, homoskedastic heads.
Tolerances as in tests/test_hip_models.py (fp32)."""
import numpy as np
import pytest
import torch

import specs
from helpers import EpsIndependent, assert_close, build_loss, build_model
from oracle import npf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = {"cnpf": O.cnpf_loss, "elbo": O.elbo_loss, "nll": O.nll_loss, "sumo": O.sumo_loss}

SWEEP = {
    "cnp_r48": dict(kind="CNP", r=48, L_xy=2, L_dec=3, dx=1, dy=2, B=5, C=17, T=45),
    "cnp_r100_dx3_dy1": dict(kind="CNP", r=100, L_xy=1, L_dec=2, dx=3, dy=1, B=3, C=33, T=65),
    "cnp_r200_L1": dict(kind="CNP", r=200, L_xy=1, L_dec=1, dx=2, dy=2, B=2, C=70, T=130),
    "cnp_r36_homosk": dict(kind="CNP", r=36, L_xy=2, L_dec=2, dx=1, dy=4, B=4, C=12, T=31, is_heteroskedastic=False),
    "lnp_latent_nz3_r40": dict(kind="LNP", r=40, L_xy=2, L_dec=2, dx=1, dy=2, B=3, C=20, T=50, encoded_path="latent",
                               is_q_zCct=True, n_z=3),
    "lnp_both_nz2_r72": dict(kind="LNP", r=72, L_xy=2, L_dec=2, dx=2, dy=3, B=2, C=31, T=33, encoded_path="both",
                             is_q_zCct=False, n_z=2),
    "attncnp_r96": dict(kind="AttnCNP", r=96, L_xy=2, L_dec=2, dx=1, dy=2, B=3, C=37, T=70),
    "attncnp_r160_c255": dict(kind="AttnCNP", r=160, L_xy=2, L_dec=2, dx=2, dy=2, B=2, C=255, T=129),
    "attncnp_r256_c256_t100": dict(kind="AttnCNP", r=256, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=256, T=100),
    # BASELINE config 2's model and point counts at batch 2: EVERY gradient tensor in full (the golden vectors
    # g3 / g4 of this size only store norms and 64-entry heads)
    "attncnp_c2_full": dict(kind="AttnCNP", r=256, L_xy=4, L_dec=4, dx=1, dy=2, B=2, C=256, T=1024),
    "attnlnp_c2_full": dict(kind="AttnLNP", r=256, L_xy=4, L_dec=4, dx=1, dy=2, B=2, C=256, T=1024, is_q_zCct=True, n_z=1),
    # wider than 256 features: 32-block chain instance, weight gradients in 256 x 256 blocks (full gradients vs the oracle)
    "cnp_r512": dict(kind="CNP", r=512, L_xy=1, L_dec=2, dx=1, dy=2, B=2, C=33, T=70),
    "cnp_r384_L2": dict(kind="CNP", r=384, L_xy=2, L_dec=2, dx=2, dy=1, B=2, C=20, T=45),
    "attncnp_r512": dict(kind="AttnCNP", r=512, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=37, T=50),
    "attnlnp_r320_nz2": dict(kind="AttnLNP", r=320, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=21, T=40, is_q_zCct=True, n_z=2),
    "attncnp_r44": dict(kind="AttnCNP", r=44, L_xy=2, L_dec=2, dx=1, dy=1, B=2, C=3, T=9),
    "attnlnp_nz3_r64": dict(kind="AttnLNP", r=64, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=40, T=48, is_q_zCct=True, n_z=3),
    # more context points than one fused score row holds: blocked softmax (attention_long.py)
    "attncnp_c300_r64": dict(kind="AttnCNP", r=64, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=300, T=70),
    "attncnp_c513_r96": dict(kind="AttnCNP", r=96, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=513, T=33),
    "attncnp_c1030_r256": dict(kind="AttnCNP", r=256, L_xy=1, L_dec=1, dx=1, dy=2, B=1, C=1030, T=64),
    "attnlnp_c400_nz2_r64": dict(kind="AttnLNP", r=64, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=400, T=40, is_q_zCct=True,
                                 n_z=2),
    "attnlnp_c260_nz1_r32": dict(kind="AttnLNP", r=32, L_xy=1, L_dec=1, dx=1, dy=1, B=3, C=260, T=50, is_q_zCct=False,
                                 n_z=1),
    # the reference's other MLP / merge options (G14 pins them on reference outputs) at the widths of the pipelined layers,
    # of the 32-block instance, with the blocked attention and with unaligned weight-column slices
    "attncnp_r256_res": dict(kind="AttnCNP", r=256, L_xy=3, L_dec=3, dx=1, dy=2, B=2, C=100, T=130, is_res=True),
    "cnp_r512_res": dict(kind="CNP", r=512, L_xy=2, L_dec=3, dx=1, dy=2, B=2, C=33, T=70, is_res=True),
    "attncnp_xt128_r256": dict(kind="AttnCNP", r=256, L_xy=2, L_dec=2, dx=1, dy=2, B=2, C=100, T=130, x_transf_dim=128),
    "attncnp_xt64_r96_c300": dict(kind="AttnCNP", r=96, L_xy=1, L_dec=1, dx=1, dy=2, B=2, C=300, T=70, x_transf_dim=64),
    "attncnp_cat_xt72_r96": dict(kind="AttnCNP", r=96, L_xy=2, L_dec=2, dx=1, dy=2, B=3, C=37, T=70, x_transf_dim=72,
                                 is_sum_merge=False),
    "attnlnp_cat_res_xt_r128": dict(kind="AttnLNP", r=128, L_xy=3, L_dec=3, dx=2, dy=3, B=2, C=40, T=48, is_q_zCct=True, n_z=2,
                                    x_transf_dim=64, is_sum_merge=False, is_res=True),
    "lnp_cat_nz2_r72": dict(kind="LNP", r=72, L_xy=2, L_dec=2, dx=2, dy=3, B=2, C=31, T=33, encoded_path="both",
                            is_q_zCct=True, n_z=2, is_sum_merge=False),
    "attnlnp_nz2_r104_noq": dict(kind="AttnLNP", r=104, L_xy=1, L_dec=2, dx=1, dy=2, B=2, C=19, T=35, is_q_zCct=False,
                                 n_z=2),
}


def _oracle(case, inp, params, mode="fp32"):
    """The oracle's train step; ``mode="bf16"``: its emulation of the bf16 compute mode."""
    cfg = specs.cfg_of(case)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    with O.matmul_mode(mode):
        out = O.forward(cfg, p, inp["X_cntxt"], inp["Y_cntxt"], inp["X_trgt"], inp["Y_trgt"], eps=inp.get("eps"),
                        n_z=case.get("n_z", 1), training=True)
        loss = LOSSES[specs.loss_name(case)](out, inp["Y_trgt"])
        loss.backward()
    return p, out, loss


@pytest.mark.parametrize("name", list(SWEEP))
def test_hip_matches_oracle_on_odd_shapes(name):
    case = SWEEP[name]
    params = specs.make_params(case, seed=11)
    inp = specs.make_inputs(case, seed=4321)
    ref_p, ref_out, ref_loss = _oracle(case, inp, params)

    model = build_model(case, DEV, params=params)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    if "eps" in dinp:
        EpsIndependent.eps = dinp["eps"]
    crit = build_loss(case)
    model.train()
    crit.train()
    out = model(dinp["X_cntxt"], dinp["Y_cntxt"], dinp["X_trgt"], dinp["Y_trgt"])
    loss = crit(out, dinp["Y_trgt"])
    loss.backward()

    assert_close(out[0].base_dist.loc, ref_out["loc"], what="loc")
    assert_close(out[0].base_dist.scale, ref_out["scale"], what="scale")
    np.testing.assert_allclose(out[0].base_dist.scale.detach().cpu().numpy(), ref_out["scale"].detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=2e-5)
    if out[1] is not None:
        assert_close(out[1], ref_out["z_samples"], what="z_samples")
    for k, p in model.named_parameters():
        ref = ref_p[k].grad if ref_p[k].grad is not None else torch.zeros_like(ref_p[k])
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        assert_close(got, ref, tol=1e-4, what=f"grad {k}")


def test_dot_attender_long_context_matches_torch():
    """DotAttender.forward (attention.py:129-164,204-220) with 1000 keys: forward and all three
    gradients against a float64 torch evaluation of softmax(Q K^T / sqrt(d)) V."""
    import npf_gwwaveform_amd as A

    g = torch.Generator().manual_seed(3)
    B, C, T, d = 2, 1000, 77, 128
    K, Q, V = (torch.randn(B, n, d, generator=g) * s for n, s in ((C, 1.5), (T, 1.5), (C, 1.0)))
    dO = torch.randn(B, T, d, generator=g)
    ref_in = [t.double().requires_grad_(True) for t in (K, Q, V)]
    ref = torch.softmax(ref_in[1] @ ref_in[0].transpose(1, 2) / d ** 0.5, dim=-1) @ ref_in[2]
    ref.backward(dO.double())
    att = A.get_attender("scaledot", d, d, d)
    dev_in = [t.to(DEV).requires_grad_(True) for t in (K, Q, V)]
    out = att(*dev_in)
    out.backward(dO.to(DEV))
    assert_close(out, ref, what="context vectors")
    for name, a, b in zip(("dK", "dQ", "dV"), dev_in, ref_in):
        assert_close(a.grad, b.grad, tol=2e-5, what=name)


@pytest.mark.parametrize("regime", ["large", "one_key", "equal"])
@pytest.mark.parametrize("C", [128, 129, 256, 257])
def test_dot_attender_score_regimes(regime, C):
    """DotAttender.forward at d = 256 on both sides of the one-score-row limit (chain path up to 256 keys, blocked softmax of
    attention_long.py beyond) with large scores (max q.k / sqrt(d) about 40), one key that dominates every query, and all keys
    equal -- forward and the three gradients against float64.  Those float64 results are ill-conditioned in the inputs' rounding,
    so the gate is max(the long-context test's gate, 4 x the error of the same formula evaluated in fp32 torch)
    (test_hip_mha.assert_gated)."""
    import npf_gwwaveform_amd as A
    from test_hip_mha import _regime, assert_gated, attention_and_grads

    B, T, d = 2, 70, 256
    g = torch.Generator().manual_seed(C)
    Q, K, V = _regime(regime, B, C, T, d, 1, g)
    dO = torch.randn(B, T, d, generator=g)
    r64, r32 = (attention_and_grads(Q, K, V, dO, 1, dt) for dt in (torch.float64, torch.float32))
    att = A.get_attender("scaledot", d, d, d)
    dev_in = [t.to(DEV).requires_grad_(True) for t in (K, Q, V)]
    out = att(*dev_in)
    out.backward(dO.to(DEV))
    for i, (name, got, tol) in enumerate((("context vectors", out, 1e-5), ("dQ", dev_in[1].grad, 2e-5), ("dK", dev_in[0].grad, 2e-5),
                                          ("dV", dev_in[2].grad, 2e-5))):
        assert_gated(got, r64[i], r32[i], tol, f"{regime} {name}")
