"""Measurements of profiles/waveform_loglike_grad.md (one MI355X, one process, the variants alternating):

  python tools/loglike_grad_bench.py [--windows 15] [--calls 10] [--regime noise|loud] [--det 0|3]
        forward + backward of HeadDistribution.lnl (or lnl_network with D = --det detectors) against the forward alone
        (HeadDistribution.loglike / loglike_network) at n_z B = 8 x 256 rows, T = 1024, n_tau = 257 on a random raw decoder output.
        ``noise``: Gaussian data; ``loud``: the data hold the template itself, so p_j is 0 on most of the grid.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/loglike_grad_bench.py --trace
        10 forward + backward calls and nothing else: the kernel times of the profile (waveform_loglike_bwd_kernel against
        waveform_filter_kernel)

Method: three warm-up windows, then ``--windows`` windows of ``--calls`` calls per variant, the two variants in turn, HIP events
around each window; ms per call as median, min and max over the windows.  One JSON line with every figure is printed at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npf_gwwaveform_amd as A  # noqa: E402

DEV = "cuda:0"
N_Z, B, T, N_TAU = 8, 256, 1024, 257
TAUS = (-128.0 / 2048.0, 1.0 / 2048.0, N_TAU)


def inputs(regime, D):
    g = torch.Generator().manual_seed(0)
    suff = torch.randn(N_Z * B, T, 4, generator=g)
    suff[..., 0] = suff[..., 0].abs() + 0.1
    suff[..., 1] *= 30.0
    shape = (B, T, 2) if D == 0 else (B, D, T, 2)
    if regime == "loud":  # d = 3 A e^{i phi} of latent sample 0: a sharp peak at tau = 0
        a, p = 3.0 * suff[:B, :, 0].double(), suff[:B, :, 1].double()
        data = torch.stack([a * torch.cos(p), a * torch.sin(p)], -1).float()
        data = data if D == 0 else data.unsqueeze(1).expand(shape).contiguous()
    else:
        data = torch.randn(shape, generator=g)
    w = 0.5 + torch.rand(shape[:-1], generator=g)
    resp = torch.ones(B, max(D, 1), 2, dtype=torch.float64)
    resp[..., 1] = 0.0
    return suff.to(DEV), data.to(DEV), w.to(DEV), resp.to(DEV), torch.linspace(20.0, 512.0, T).to(DEV)


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
    ap.add_argument("--regime", choices=("noise", "loud"), default="noise")
    ap.add_argument("--det", type=int, default=0, help="0: the single stream; D >= 1: the network of D detectors")
    ap.add_argument("--trace", action="store_true", help="10 forward + backward calls and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglike_grad_bench needs a GPU: there is nothing to measure without one")
    suff, data, w, resp, f = inputs(args.regime, args.det)
    suff.requires_grad_()
    p = A.HeadDistribution(suff, 2, False, N_Z, B, T)
    if args.det:
        fwd = lambda: p.loglike_network(data, resp, None, weights=w, freqs=f, taus=TAUS)  # noqa: E731
        lnl = lambda: p.lnl_network(data, resp, None, weights=w, freqs=f, taus=TAUS)  # noqa: E731
    else:
        fwd = lambda: p.loglike(data, weights=w, freqs=f, taus=TAUS)  # noqa: E731
        lnl = lambda: p.lnl(data, weights=w, freqs=f, taus=TAUS)  # noqa: E731

    def both():
        suff.grad = None
        lnl().lnl.sum().backward()

    if args.trace:
        for _ in range(10):
            both()
        torch.cuda.synchronize()
        return
    both_window = lambda: [both() for _ in range(args.calls)]  # noqa: E731
    fwd_window = lambda: [fwd() for _ in range(args.calls)]  # noqa: E731
    for _ in range(3):
        both_window(), fwd_window()
    torch.cuda.synchronize()
    t_both, t_fwd = [], []
    for _ in range(args.windows):
        t_both.append(timed(both_window) / args.calls)
        t_fwd.append(timed(fwd_window) / args.calls)
    res = dict(rows=N_Z * B, T=T, n_tau=N_TAU, D=args.det, regime=args.regime, windows=args.windows, calls=args.calls,
               fwd_bwd_ms=statistics.median(t_both), fwd_bwd_ms_min=min(t_both), fwd_bwd_ms_max=max(t_both),
               fwd_ms=statistics.median(t_fwd), fwd_ms_min=min(t_fwd), fwd_ms_max=max(t_fwd))
    res["fwd_bwd_over_fwd"] = res["fwd_bwd_ms"] / res["fwd_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
