"""Measurements of profiles/waveform_loglike_distance.md (one MI355X, one process, the variants alternating):

  python tools/loglike_dist_bench.py [--windows 15] [--calls 10]   HeadDistribution.loglike_distance and
                                                                   HeadDistribution.loglike_network_distance (D = 3) with n_a in
                                                                   {32, 128, 512} scales and the posterior, against the plain
                                                                   HeadDistribution.loglike / loglike_network call, at n_z B =
                                                                   8 x 256 rows, T = 1024, n_tau = 257 on a random raw decoder output

The plain calls do NOT compute the new quantity: they are the existing cost the two scale launches are added to.  Method: three
warm-up windows, then ``--windows`` windows of ``--calls`` calls per variant, the variants in turn, HIP events around each window;
ms per call as median, min and max over the windows, the increment over the yardstick per n_a and per (row, j, i) evaluation of
ln I0.  One JSON line with every figure is printed at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npf_gwwaveform_amd as A  # noqa: E402

DEV = "cuda:0"
N_Z, B, T, N_TAU, D = 8, 256, 1024, 257, 3
N_AS = (32, 128, 512)
TAUS = (-128.0 / 2048.0, 1.0 / 2048.0, N_TAU)


def inputs():
    g = torch.Generator().manual_seed(0)
    suff = torch.randn(N_Z * B, T, 4, generator=g)
    suff[..., 0] = suff[..., 0].abs() + 0.1
    suff[..., 1] *= 30.0
    data = torch.randn(B, D, T, 2, generator=g)
    w = 0.5 + torch.rand(B, D, T, generator=g)
    resp = torch.randn(B, D, 2, generator=g, dtype=torch.float64)
    delays = 0.02 * (2.0 * torch.rand(B, D, generator=g, dtype=torch.float64) - 1.0)
    return suff.to(DEV), data.to(DEV), w.to(DEV), resp.to(DEV), delays.to(DEV), torch.linspace(20.0, 512.0, T).to(DEV)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglike_dist_bench needs a GPU: there is nothing to measure without one")
    suff, data, w, resp, delays, f = inputs()
    d0, w0 = data[:, 0].contiguous(), w[:, 0].contiguous()
    p = A.HeadDistribution(suff, 2, False, N_Z, B, T)
    variants = {"single": lambda: p.loglike(d0, weights=w0, freqs=f, taus=TAUS),
                "network": lambda: p.loglike_network(data, resp, delays, weights=w, freqs=f, taus=TAUS)}
    for n_a in N_AS:
        s, lp = A.functional.distance_prior(torch.logspace(1.0, 3.0, n_a, dtype=torch.float64, device=DEV), 100.0)
        variants[f"single_na{n_a}"] = lambda s=s, lp=lp: p.loglike_distance(d0, s, lp, weights=w0, freqs=f, taus=TAUS, posterior=True)
        variants[f"network_na{n_a}"] = lambda s=s, lp=lp: p.loglike_network_distance(data, resp, delays, s, lp, weights=w, freqs=f,
                                                                                    taus=TAUS, posterior=True)
    windows = {k: (lambda fn=fn: [fn() for _ in range(args.calls)]) for k, fn in variants.items()}
    for _ in range(3):
        for win in windows.values():
            win()
    torch.cuda.synchronize()
    times = {k: [] for k in windows}
    for _ in range(args.windows):
        for k, win in windows.items():
            times[k].append(timed(win) / args.calls)
    res = dict(rows=N_Z * B, T=T, n_tau=N_TAU, D=D, windows=args.windows, calls=args.calls)
    for k, t in times.items():
        res[f"{k}_ms"], res[f"{k}_ms_min"], res[f"{k}_ms_max"] = statistics.median(t), min(t), max(t)
    for kind in ("single", "network"):
        for n_a in N_AS:
            inc = res[f"{kind}_na{n_a}_ms"] - res[f"{kind}_ms"]
            res[f"{kind}_na{n_a}_increment_ms"] = inc
            res[f"{kind}_na{n_a}_ns_per_evaluation"] = inc * 1e6 / (N_Z * B * N_TAU * n_a)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
