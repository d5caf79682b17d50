"""Measurements of profiles/waveform_loglike_network.md (one MI355X, one process, the variants alternating):

  python tools/loglike_net_bench.py [--windows 15] [--calls 10]   HeadDistribution.loglike_network with D = 3 detectors against D
                                                                  successive HeadDistribution.loglike calls (one per detector's data
                                                                  and weights) at n_z B = 8 x 256 rows, T = 1024, n_tau = 257 on a
                                                                  random raw decoder output, with the peak extra memory of both
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/loglike_net_bench.py --trace
                                                                  10 calls of each and nothing else: the kernel times of the profile

The D calls do NOT compute the network quantity (they maximise per detector and know no delay): they are the yardstick for time
only.  Method: three warm-up windows, then ``--windows`` windows of ``--calls`` calls per variant, the two variants in turn, HIP
events around each window; ms per call as median, min and max over the windows.  One JSON line with every figure is printed at
the end."""
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
TAUS = (-128.0 / 2048.0, 1.0 / 2048.0, N_TAU)


def inputs():
    g = torch.Generator().manual_seed(0)
    suff = torch.randn(N_Z * B, T, 4, generator=g)
    suff[..., 0] = suff[..., 0].abs() + 0.1
    suff[..., 1] *= 30.0
    data = torch.randn(B, D, T, 2, generator=g)
    w = 0.5 + torch.rand(B, D, T, generator=g)
    resp = torch.randn(B, D, 2, generator=g, dtype=torch.float64)
    delays = 0.02 * (2.0 * torch.rand(B, D, generator=g, dtype=torch.float64) - 1.0)  # +- 20 ms: the light travel time across the Earth
    return suff.to(DEV), data.to(DEV), w.to(DEV), resp.to(DEV), delays.to(DEV), torch.linspace(20.0, 512.0, T).to(DEV)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak_extra(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="10 calls of each variant and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglike_net_bench needs a GPU: there is nothing to measure without one")
    suff, data, w, resp, delays, f = inputs()
    per_det = [(data[:, k].contiguous(), w[:, k].contiguous()) for k in range(D)]
    p = A.HeadDistribution(suff, 2, False, N_Z, B, T)
    net = lambda: p.loglike_network(data, resp, delays, weights=w, freqs=f, taus=TAUS)  # noqa: E731
    calls = lambda: [p.loglike(d_k, weights=w_k, freqs=f, taus=TAUS) for d_k, w_k in per_det]  # noqa: E731
    if args.trace:
        for _ in range(10):
            net(), calls()
        torch.cuda.synchronize()
        return
    net_window = lambda: [net() for _ in range(args.calls)]  # noqa: E731
    calls_window = lambda: [calls() for _ in range(args.calls)]  # noqa: E731
    for _ in range(3):
        net_window(), calls_window()
    torch.cuda.synchronize()
    t_net, t_calls = [], []
    for _ in range(args.windows):
        t_net.append(timed(net_window) / args.calls)
        t_calls.append(timed(calls_window) / args.calls)
    res = dict(rows=N_Z * B, T=T, n_tau=N_TAU, D=D, windows=args.windows, calls=args.calls,
               network_ms=statistics.median(t_net), network_ms_min=min(t_net), network_ms_max=max(t_net),
               d_calls_ms=statistics.median(t_calls), d_calls_ms_min=min(t_calls), d_calls_ms_max=max(t_calls),
               network_peak_extra_bytes=peak_extra(net), d_calls_peak_extra_bytes=peak_extra(calls))
    res["network_over_d_calls"] = res["network_ms"] / res["d_calls_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
