"""Measurements of profiles/waveform_loglike_sky_distance.md (one MI355X, one process, the variants alternating):

  python tools/loglike_sky_distance_bench.py [--reps 3] [--steps 3]
      functional.waveform_loglike_sky_distance at n_z x B = 8 x 8 = 64 rows, D = 3, pts = 1024, n_tau = 64, P = 768 pixels and
      n_a = 32 scales against (a) P calls of functional.waveform_loglike_network_distance, one pixel's response and delays
      broadcast over the tasks each, and (b) functional.waveform_loglike_sky at the same size: the price of the scale axis

The loop is what the library offered before the joint call (``waveform_loglike_network_distance`` is unchanged by it); the broadcast
operands are made once, outside the clock, and the torch glue that turns the loop's results into the joint marginal (stacking,
adding the pixel prior, ``logsumexp``) is not timed either.  The method is that of tools/loglike_sky_bench.py and
tools/predict_bench.py: a host clock around work that ends in a device synchronise, 5 warm-up calls per variant, ``--reps``
repetitions of ``--steps`` calls of each variant in turn; min ... max over the repetitions are printed as one JSON line per variant,
with the agreement of the call and the loop in units of the suite's gates and the rate of ln I0 evaluations, R P n n_a over the time
of the whole call (four launches, the correlation included), so a lower bound of the scale-marginal launch's own rate."""
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

    n_z, B, D, T, n_tau, P, n_a = args.n_z, args.tasks, args.det, args.pts, args.n_tau, args.pix, args.scales
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
    scales, lps = FN.distance_prior(torch.linspace(0.25, 4.0, n_a, dtype=torch.float64, device=DEV), 1.0)
    resp_b = [resp[p].expand(B, D, 2).contiguous() for p in range(P)]
    delays_b = [delays[p].expand(B, D).contiguous() for p in range(P)]
    want = ("hh", "dd", "lnl_dist")

    def joint_call():
        return FN.waveform_loglike_sky_distance(h, data, resp, delays, scales, lps, log_prior, w, f, taus, want=("lnl_vol",),
                                                posterior=True, moments=True)

    def loop():
        return [FN.waveform_loglike_network_distance(h, data, resp_b[p], delays_b[p], scales, lps, w, f, taus, want=want, posterior=True)
                for p in range(P)]

    def sky_call():
        return FN.waveform_loglike_sky(h, data, resp, delays, log_prior, w, f, taus, want=("lnl_sky",), posterior=True)

    got, parts = joint_call(), loop()
    wpi = torch.stack([m.post + m.lnl_dist.view(R, 1) for m in parts], 1) + log_prior.view(1, P, 1)  # [R, P, n_a]
    hh, dd = torch.stack([m.base.hh for m in parts], 1), parts[0].base.dd.repeat(n_z).view(R, 1)
    S = (scales.view(1, 1, -1) * (hh * dd).sqrt().unsqueeze(2) + 0.5 * (scales ** 2).view(1, 1, -1) * hh.unsqueeze(2)
         + lps.abs().view(1, 1, -1)).amax((1, 2))
    gate = 1e-10 * S + 1e-12
    vol = torch.logsumexp(wpi.reshape(R, -1), 1)
    ratios = {"lnl_vol": float(((got.lnl_vol - vol).abs() / gate).max()),
              "post_sky": float(((got.post_sky - (torch.logsumexp(wpi, 2) - vol.view(R, 1))).abs() / (2.0 * gate.view(R, 1))).max()),
              "post_dist": float(((got.post_dist - (torch.logsumexp(wpi, 1) - vol.view(R, 1))).abs() / (2.0 * gate.view(R, 1))).max())}
    evals = float(R) * P * max(n_tau, 1) * n_a
    name = f"{P} calls of waveform_loglike_network_distance"
    ms = alternate({"waveform_loglike_sky_distance": joint_call, name: loop, "waveform_loglike_sky": sky_call}, args.reps, args.steps)
    for k, v in ms.items():
        row = {"table": "loglike_sky_distance", "rows": R, "n_z": n_z, "D": D, "pts": T, "n_tau": n_tau, "P": P, "n_a": n_a, "variant": k,
               "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
        if k == "waveform_loglike_sky_distance":
            row.update({f"{q}_diff_over_gate": r for q, r in ratios.items()})
            row["log_i0_gevals_per_s_at_ms_min"] = round(evals / (min(v) * 1e-3) / 1e9, 2)
        print(json.dumps(row), flush=True)
    a, b, c = min(ms["waveform_loglike_sky_distance"]), min(ms[name]), min(ms["waveform_loglike_sky"])
    print(json.dumps({"table": "loglike_sky_distance", "loop_over_joint_call": round(b / a, 2), "joint_call_over_sky_call": round(a / c, 2),
                      "agree_within_gates": max(ratios.values()) <= 1}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-z", type=int, default=8)
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--det", type=int, default=3)
    ap.add_argument("--pts", type=int, default=1024)
    ap.add_argument("--n-tau", type=int, default=64)
    ap.add_argument("--pix", type=int, default=768)
    ap.add_argument("--scales", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a)
