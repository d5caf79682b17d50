"""Measurements of profiles/waveform_loglike_sky.md (one MI355X, one process, the variants alternating):

  python tools/loglike_sky_bench.py [--reps 3] [--steps 3]   functional.waveform_loglike_sky at n_z x B = 8 x 8 = 64 rows, D = 3,
                                                             pts = 1024, n_tau = 64, P = 768 pixels against P calls of
                                                             functional.waveform_loglike_network, one pixel's response and delays
                                                             broadcast over the tasks each

The loop is what the library offered before the sky call (``waveform_loglike_network`` is unchanged by it); the broadcast operands
are made once, outside the clock, and stacking the loop's results and the torch ``logsumexp`` over the pixels are not timed either.
The method is that of tools/predict_bench.py: a host clock around work that ends in a device synchronise, 5 warm-up calls per
variant, ``--reps`` repetitions of ``--steps`` calls of each variant in turn; min ... max over the repetitions are printed as one
JSON line per variant, with the agreement of the two results in units of the suite's gates and the double-precision rate of the
contraction, 8 R n_tau P D pts real operations, over the time of the whole call (three launches, the R P n_tau evaluations of ln I0
included), so a lower bound of the kernel's own rate."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import DEV, alternate  # noqa: E402


def main(args):
    from npf_gwwaveform_amd import functional as FN

    n_z, B, D, T, n_tau, P = args.n_z, args.tasks, args.det, args.pts, args.n_tau, args.pix
    R = n_z * B
    g = torch.Generator(device=DEV).manual_seed(1)
    rand = lambda *s: torch.rand(*s, device=DEV, generator=g)  # noqa: E731
    h = torch.stack([0.05 * (0.5 + rand(R, T)), 3.0 * torch.randn(R, T, device=DEV, generator=g)], -1)
    data = torch.randn(B, D, T, 2, device=DEV, generator=g)
    w = 0.5 + rand(D, T)
    f = torch.linspace(20.0, 512.0, T, device=DEV)
    taus = (-(n_tau // 2) / 2048.0, 1.0 / 2048.0, n_tau)
    mod, arg = 0.4 + rand(P, D).double(), 2.0 * math.pi * rand(P, D).double()
    resp = torch.stack([mod * torch.cos(arg), mod * torch.sin(arg)], -1)
    delays = (2.0 * rand(P, D).double() - 1.0) * 0.01
    mass = 0.2 + rand(P).double()
    log_prior = torch.log(mass / mass.sum())
    resp_b = [resp[p].expand(B, D, 2).contiguous() for p in range(P)]
    delays_b = [delays[p].expand(B, D).contiguous() for p in range(P)]
    want = ("hh", "dd", "lnl_marg")

    def sky_call():
        return FN.waveform_loglike_sky(h, data, resp, delays, log_prior, w, f, taus, want=("lnl_sky",), posterior=True)

    def loop():
        return [FN.waveform_loglike_network(h, data, resp_b[p], delays_b[p], w, f, taus, want=want) for p in range(P)]

    got, parts = sky_call(), loop()
    u = torch.stack([m.lnl_marg for m in parts], 1) + log_prior.view(1, P)
    hh, dd = torch.stack([m.hh for m in parts], 1), parts[0].dd.repeat(n_z).view(R, 1)
    gate = 1e-10 * ((hh * dd).sqrt() + 0.5 * hh).max(1).values + 1e-12
    lnl = torch.logsumexp(u, 1)
    ratio_lnl = float(((got.lnl_sky - lnl).abs() / gate).max())
    ratio_post = float((((got.post - (u - lnl.view(R, 1))).abs()) / (2.0 * gate.view(R, 1))).max())
    flops = 8.0 * R * max(n_tau, 1) * P * D * T
    name = f"{P} calls of waveform_loglike_network"
    ms = alternate({"waveform_loglike_sky": sky_call, name: loop}, args.reps, args.steps)
    for k, v in ms.items():
        row = {"table": "loglike_sky", "rows": R, "n_z": n_z, "D": D, "pts": T, "n_tau": n_tau, "P": P, "variant": k,
               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "lnl_sky_diff_over_gate": ratio_lnl,
               "post_diff_over_gate": ratio_post}
        if k == "waveform_loglike_sky":
            row["f64_tflops_at_ms_min"] = round(flops / (min(v) * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)
    a, b = min(ms["waveform_loglike_sky"]), min(ms[name])
    print(json.dumps({"table": "loglike_sky", "loop_over_sky_call": round(b / a, 2), "agree_within_gates": ratio_lnl <= 1 and ratio_post <= 1}),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-z", type=int, default=8)
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--det", type=int, default=3)
    ap.add_argument("--pts", type=int, default=1024)
    ap.add_argument("--n-tau", type=int, default=64)
    ap.add_argument("--pix", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a)
