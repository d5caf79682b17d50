"""Measurements of profiles/loo.md (one MI355X): ms per ``model.loo`` call at B = 64, C = 256 for AttnCNP scaled-dot r = 256,
AttnCNP transformer r = 128 and CNP r = 256, full counts and counts drawn per task, beside ``forward`` in evaluation mode on the
same context with the context points as targets (the same number of decoded points; it answers another question and is only a
yardstick for the launch overheads).

  timeout -k 10 120 python tools/loo_bench.py [--reps 7] [--calls 20]

Every timing: warmed up, ``--reps`` repetitions of ``--calls`` calls each between two device synchronisations, the variants in
turn; ms per call, min ... max over the repetitions, one JSON line per model."""
import argparse
import json
import os
import sys
import time
import warnings
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
B, C = 64, 256


def _model(kind, r, **kw):
    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(kw, r_dim=r, XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=r), is_sum_merge=True),
                  Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=4, hidden_size=r), is_sum_merge=True))
        return getattr(A, kind)(1, 2, **kw).to(DEV).eval()


def _ms_per_call(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def row(args, name, kind, r, **kw):
    model = _model(kind, r, **kw)
    g = torch.Generator().manual_seed(1)
    Xc, Yc = (torch.rand(B, C, 1, generator=g) * 2 - 1).to(DEV), torch.randn(B, C, 2, generator=g).to(DEV)
    full = torch.full((B,), C, dtype=torch.int32, device=DEV)
    mixed = torch.randint(1, C + 1, (B,), generator=g).to(torch.int32).to(DEV)
    variants = {
        "loo_full_counts": lambda: model.loo(Xc, Yc, n_cntxt=full).base_dist,
        "loo_mixed_counts": lambda: model.loo(Xc, Yc, n_cntxt=mixed).base_dist,
        "forward_context_as_targets": lambda: model(Xc, Yc, Xc)[0].base_dist,
    }
    for fn in variants.values():
        _ms_per_call(fn, 10)
    ms = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            ms[k].append(_ms_per_call(fn, args.calls))
    print(json.dumps(dict(model=name, B=B, C=C, reps=args.reps, calls=args.calls,
                          ms_per_call={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()})), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    with torch.no_grad():
        row(args, "AttnCNP scaled-dot r = 256", "AttnCNP", 256)
        row(args, "AttnCNP transformer r = 128", "AttnCNP", 128, attention="transformer")
        row(args, "CNP r = 256", "CNP", 256)
