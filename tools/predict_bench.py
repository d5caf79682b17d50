"""Measurements of profiles/predictive_summary.md (one MI355X, one process, the variants alternating):

  python tools/predict_bench.py summary [--iters-lib LIB]   npf_mixture_summary at n_z = 32, B = 256, T = 1024, dy = 2: moments only,
                                                            with three quantiles, and the eager route (base_dist, mean, variance);
                                                            LIB: a build of csrc/predict_kernels.hip with -DNPF_MIXTURE_COUNT_ITERS
                                                            (tools/fastbuild.sh), whose counter gives the solver steps per element
  python tools/predict_bench.py grids                       condition once + 8 queries of 1024 targets against 8 eval-mode forwards
                                                            (AttnCNP config-2 sizes; transformer attention at r = 128)

Every timing: a host clock around work that ends in a device synchronise, every shape warmed up, ``--reps`` repetitions of each
variant in turn; min ... max over the repetitions are printed as one JSON line per table row."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def alternate(variants, reps, n):
    for fn in variants.values():
        for _ in range(5):
            fn()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn, n))
    return ms


def summary(args):
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import functional as FN

    n_z, B, T, dy = 32, 256, 1024, 2
    suff = torch.randn(n_z * B, T, 2 * dy, device=DEV)
    probs = (0.025, 0.5, 0.975)

    def eager():
        p = A.HeadDistribution(suff, dy, False, n_z, B, T)
        loc, scale = p.base_dist.loc, p.base_dist.scale
        mean = loc.mean(0)
        return mean, (scale.pow(2) + (loc - mean).pow(2)).mean(0).sqrt()

    ms = alternate({"moments": lambda: FN.mixture_summary(suff, n_z, dy, False),
                    "moments+3 quantiles": lambda: FN.mixture_summary(suff, n_z, dy, False, probs=probs),
                    "eager moments (base_dist, mean, variance)": eager}, args.reps, args.steps)
    nbytes = suff.numel() * 4
    for k, v in ms.items():
        print(json.dumps({"table": "summary", "variant": k, "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                          "suff_bytes": nbytes, "suff_GB_per_s_best": round(nbytes / min(v) / 1e6, 1)}))
    if args.iters_lib:
        lib = C.CDLL(args.iters_lib)
        z_p, p_dev = FN._z_p_device(probs, suff.device)
        mean = torch.empty(B, T, dy, device=DEV)
        std, quant = torch.empty_like(mean), torch.empty(3, B, T, dy, device=DEV)
        vp = C.c_void_p
        lib.npf_debug_mixture_iters(None, 1)
        rc = lib.npf_mixture_summary(vp(suff.data_ptr()), None, n_z, B, T, dy, 0, vp(z_p.data_ptr()), 3, vp(p_dev.data_ptr()),
                                     vp(mean.data_ptr()), vp(std.data_ptr()), vp(quant.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        out = (C.c_ulonglong * 2)()
        lib.npf_debug_mixture_iters(out, 0)
        assert rc == 0 and out[1] == 3 * B * T * dy
        print(json.dumps({"table": "summary", "variant": "solver", "cdf_evaluations_per_quantile": round(out[0] / out[1], 3),
                          "per_element_3_quantiles": round(3 * out[0] / out[1], 3)}))


def grids(args):
    import bench

    for tag, kw, C_ in (("attncnp scaledot r=256 C=256 B=256", dict(r=256, attention="scaledot"), 256),
                        ("attncnp transformer r=128 C=128 B=256", dict(r=128, attention="transformer"), 128)):
        model = bench.build_model("attncnp", kw["r"], 4, DEV, attention=kw["attention"])[0].eval()
        B, T, G = 256, 1024, 8
        g = torch.Generator().manual_seed(1)
        Xc, Yc = (torch.rand(B, C_, 1, generator=g) * 2 - 1).to(DEV), torch.randn(B, C_, 2, generator=g).to(DEV)
        Xts = [(torch.rand(B, T, 1, generator=g) * 2 - 1).to(DEV) for _ in range(G)]

        def forwards():
            with torch.no_grad():
                return [model(Xc, Yc, Xt)[0] for Xt in Xts]

        def conditioned():
            post = model.condition(Xc, Yc)
            return [post.query(Xt) for Xt in Xts]

        ms = alternate({"8 eval forwards": forwards, "condition + 8 queries": conditioned}, args.reps, args.steps)
        for k, v in ms.items():
            print(json.dumps({"table": "grids", "model": tag, "variant": k, "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}))
        print(json.dumps({"table": "grids", "model": tag, "forwards_over_conditioned_best": round(min(ms["8 eval forwards"]) / min(ms["condition + 8 queries"]), 4)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("summary", "grids"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"summary": summary, "grids": grids}[a.what](a)
