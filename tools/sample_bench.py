"""Measurements of profiles/function_samples.md (one MI355X, one process per table, the variants alternating):

  python tools/sample_bench.py scaledot      AttnCNP scaled-dot r = 256, B = 64, C = 256, T = 64, S in {1, 4, 16}, chunk in {1, 8}
  python tools/sample_bench.py transformer   AttnCNP transformer attention r = 128, the same sizes
  python tools/sample_bench.py cnp           CNP r = 256, the same sizes

Each row: ``Conditioned.sample_functions(X_trgt, S)`` on one conditioned context against ``Conditioned.rollout`` on the batch tiled S
times (conditioned anew for every call, outside the timed region, since a rollout uses its state up), with the same noise.  Run each
table as a command of its own under a time limit (``timeout -k 10 300 python tools/sample_bench.py scaledot``).  Every timing: every
shape warmed up, ``--reps`` repetitions of each variant in turn, min ... max over the repetitions as one JSON line per row; the bytes
of conditioned state each route holds are printed beside it (4 bytes x PT32 rows x padded features, keys + values)."""
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
B, C, T = 64, 256, 64


def _model(kind, r, **kw):
    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(kw, r_dim=r, XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=r), is_sum_merge=True),
                  Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=4, hidden_size=r), is_sum_merge=True))
        return getattr(A, kind)(1, 2, **kw).to(DEV).eval()


def _ms(fn, prepare):
    """Wall time of ``fn(prepare())`` in ms, the preparation outside the timed region."""
    state = prepare()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(state)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def state_bytes(model, S, tiled):
    """Bytes of conditioned keys + values (attentive) or per-point representations (CNP) held while drawing: the prefix once plus
    S B tails of pad32(T) rows, or S B copies at capacity C + T."""
    pad = lambda n: (n + 31) // 32 * 32  # noqa: E731
    feats = pad(model.r_dim) + (pad(model.x_transf_dim) if model._attentive else 0)
    if tiled:
        return 4 * S * B * pad(C + T) * feats
    return 4 * (B * pad(C) + S * B * pad(T)) * feats


def table(args, kind, r, **kw):
    model = _model(kind, r, **kw)
    g = torch.Generator().manual_seed(1)
    Xc, Yc = (torch.rand(B, C, 1, generator=g) * 2 - 1).to(DEV), torch.randn(B, C, 2, generator=g).to(DEV)
    Xt = (torch.rand(B, T, 1, generator=g) * 2 - 1).to(DEV)
    for S in (1, 4, 16):
        eps = torch.randn(S, B, T, 2, generator=g).to(DEV)
        Xc_t, Yc_t, Xt_t, eps_t = Xc.repeat(S, 1, 1), Yc.repeat(S, 1, 1), Xt.repeat(S, 1, 1), eps.reshape(S * B, T, 2)
        shared = model.condition_with_capacity(Xc, Yc, C)
        for chunk in (1, 8):
            variants = {
                "sample_functions": (lambda post, S=S, eps=eps, chunk=chunk: post.sample_functions(Xt, S, eps=eps, chunk=chunk), lambda: shared),
                "tiled_rollout": (lambda post, chunk=chunk: post.rollout(Xt_t, eps=eps_t, chunk=chunk),
                                  lambda: model.condition_with_capacity(Xc_t, Yc_t, C + T)),
            }
            for fn, prep in variants.values():
                for _ in range(2):
                    _ms(fn, prep)
            ms = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, (fn, prep) in variants.items():
                    ms[k].append(_ms(fn, prep))
            print(json.dumps(dict(table=args.table, kind=kind, r=r, B=B, C=C, T=T, S=S, chunk=chunk,
                                  ms={k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                                  state_bytes={"sample_functions": state_bytes(model, S, False), "tiled_rollout": state_bytes(model, S, True)})),
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("table", choices=("scaledot", "transformer", "cnp"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    with torch.no_grad():
        if args.table == "scaledot":
            table(args, "AttnCNP", 256)
        elif args.table == "transformer":
            table(args, "AttnCNP", 128, attention="transformer")
        else:
            table(args, "CNP", 256)
