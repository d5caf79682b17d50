"""Measurements of profiles/waveform_loglike.md (one MI355X, one process, the variants alternating):

  python tools/loglike_bench.py [--windows 15] [--calls 20]   HeadDistribution.loglike against HeadDistribution.match at
                                                              n_z B = 8 x 256 rows, T = 1024, n_tau = 257 on a random raw decoder
                                                              output, then the same quantities in eager PyTorch with peak memory
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/loglike_bench.py --trace
                                                              20 calls of each and nothing else: the kernel times of the profile

Method: three warm-up windows, then ``--windows`` windows of ``--calls`` calls per variant, the two variants in turn, HIP events
around each window; ms per call as median, min and max over the windows.  The eager composition is the reference, not the code under
test: ``exp(1j (phi + 2 pi f tau_j))`` over a [rows, T, n_tau] complex128 temporary, ``torch.special.i0e``, ``logsumexp``.  One JSON
line with every figure is printed at the end."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import npf_gwwaveform_amd as A  # noqa: E402

DEV = "cuda:0"
N_Z, B, T, N_TAU = 8, 256, 1024, 257
TAUS = (-128.0 / 2048.0, 1.0 / 2048.0, N_TAU)


def inputs():
    g = torch.Generator().manual_seed(0)
    suff = torch.randn(N_Z * B, T, 4, generator=g)
    suff[..., 0] = suff[..., 0].abs() + 0.1
    suff[..., 1] *= 30.0
    data = torch.randn(B, T, 2, generator=g)
    Y_ref = torch.stack([0.5 + torch.rand(B, T, generator=g), 30.0 * torch.randn(B, T, generator=g)], -1)
    w = 0.5 + torch.rand(B, T, generator=g)
    return suff.to(DEV), data.to(DEV), Y_ref.to(DEV), w.to(DEV), torch.linspace(20.0, 512.0, T).to(DEV)


def eager(suff, data, w, f):
    """(lnl [B], lnl_marg [R], lnl_max [R]) in eager PyTorch."""
    h = suff.double()
    amp, phi = h[..., 0], h[..., 1]
    d = torch.complex(data[..., 0].double(), data[..., 1].double()).repeat(N_Z, 1)
    wd = w.double().repeat(N_Z, 1)
    tau = TAUS[0] + torch.arange(N_TAU, dtype=torch.float64, device=DEV) * TAUS[1]
    c = wd * amp * d.conj()
    kappa = (c.unsqueeze(2) * torch.exp(1j * (phi.unsqueeze(2) + 2 * math.pi * f.double().view(1, T, 1) * tau.view(1, 1, -1)))).sum(1)
    hh = (wd * amp * amp).sum(1)
    x = kappa.abs()
    L = x + torch.log(torch.special.i0e(x)) - 0.5 * hh.unsqueeze(1)
    lnl_marg = torch.logsumexp(L, 1) - math.log(N_TAU)
    return torch.logsumexp(lnl_marg.view(N_Z, B), 0) - math.log(N_Z), lnl_marg, x.max(1).values - 0.5 * hh


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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="20 calls of each variant and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglike_bench needs a GPU: there is nothing to measure without one")
    suff, data, Y_ref, w, f = inputs()
    p = A.HeadDistribution(suff, 2, False, N_Z, B, T)
    ll = lambda: p.loglike(data, weights=w, freqs=f, taus=TAUS)  # noqa: E731
    ma = lambda: p.match(Y_ref, weights=w, freqs=f, taus=TAUS)  # noqa: E731
    if args.trace:
        for _ in range(20):
            ll(), ma()
        torch.cuda.synchronize()
        return
    ll_window = lambda: [ll() for _ in range(args.calls)]  # noqa: E731
    ma_window = lambda: [ma() for _ in range(args.calls)]  # noqa: E731
    for _ in range(3):
        ll_window(), ma_window()
    torch.cuda.synchronize()
    t_ll, t_ma = [], []
    for _ in range(args.windows):
        t_ll.append(timed(ll_window) / args.calls)
        t_ma.append(timed(ma_window) / args.calls)
    res = dict(rows=N_Z * B, T=T, n_tau=N_TAU, windows=args.windows, calls=args.calls,
               loglike_ms=statistics.median(t_ll), loglike_ms_min=min(t_ll), loglike_ms_max=max(t_ll),
               match_ms=statistics.median(t_ma), match_ms_min=min(t_ma), match_ms_max=max(t_ma))
    m = ll()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ll()
    torch.cuda.synchronize()
    res["loglike_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e_mix, e_marg, _ = eager(suff, data, w, f)  # (the warm-up call)
    torch.cuda.synchronize()
    res["eager_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
    t_e = [timed(lambda: eager(suff, data, w, f)) for _ in range(5)]
    res.update(eager_ms=statistics.median(t_e), eager_ms_min=min(t_e), eager_ms_max=max(t_e),
               eager_vs_kernel_lnl=float((e_mix - m.lnl).abs().max()),
               eager_vs_kernel_lnl_marg=float((e_marg.view(N_Z, B) - m.lnl_marg).abs().max()),
               lnl_marg_abs_max=float(m.lnl_marg.abs().max()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
