"""Measurements of profiles/predictive_scores.md (one MI355X, one process, the variants alternating):

  python tools/score_bench.py [--nz 1 8 32 128]   npf_mixture_score at B = 256, T = 1024, dy = 2 (heteroskedastic) per n_z: all three
                                                  scores, the log density alone, and the eager torch composition over base_dist
                                                  (logsumexp of the component log densities, cdf().mean(0), the pairwise CRPS)

The method is that of tools/predict_bench.py: a host clock around work that ends in a device synchronise, every shape warmed up,
``--reps`` repetitions of each variant in turn; min ... max over the repetitions are printed as one JSON line per table row.  The
eager pairwise CRPS makes [n_z, n_z, B, T, dy] temporaries: it is chunked over the first axis to stay below ``--eager-bytes``."""
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


def _A(m, s):
    return 2.0 * s * torch.exp(-0.5 * (m / s) ** 2) / math.sqrt(2.0 * math.pi) + m * torch.erf(m / (s * math.sqrt(2.0)))


def main(args):
    import npf_gwwaveform_amd as A
    from npf_gwwaveform_amd import functional as FN

    B, T, dy = 256, 1024, 2
    for n_z in args.nz:
        suff = torch.randn(n_z * B, T, 2 * dy, device=DEV)
        Y = torch.randn(B, T, dy, device=DEV)
        rows = max(1, min(n_z, args.eager_bytes // (n_z * B * T * dy * 4 * 4)))  # (about four temporaries of a chunk alive at once)

        def eager():
            p = A.HeadDistribution(suff, dy, False, n_z, B, T)
            base = p.base_dist
            loc, scale = base.loc, base.scale
            ld = torch.logsumexp(base.log_prob(Y), 0) - math.log(n_z)
            pit = base.cdf(Y).mean(0)
            pair = torch.zeros_like(Y)
            for i in range(0, n_z, rows):
                pair += _A(loc[i:i + rows].unsqueeze(1) - loc.unsqueeze(0),
                           (scale[i:i + rows].unsqueeze(1) ** 2 + scale.unsqueeze(0) ** 2).sqrt()).sum((0, 1))
            return ld, pit, _A(Y - loc, scale).mean(0) - pair / (2.0 * n_z * n_z)

        def eager_ld():
            p = A.HeadDistribution(suff, dy, False, n_z, B, T)
            return torch.logsumexp(p.base_dist.log_prob(Y), 0) - math.log(n_z)

        ms = alternate({"all three scores": lambda: FN.mixture_score(suff, Y, n_z, dy, False),
                        "log_density only": lambda: FN.mixture_score(suff, Y, n_z, dy, False, want=("log_density",)),
                        "eager torch, all three": eager, "eager torch, log_density only": eager_ld},
                       args.reps, args.steps if n_z < 128 else max(1, args.steps // 10))
        for k, v in ms.items():
            print(json.dumps({"table": "score", "n_z": n_z, "variant": k, "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                              "pairs_per_element": n_z * (n_z - 1) // 2}), flush=True)
        del suff, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--eager-bytes", type=int, default=8 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a)
