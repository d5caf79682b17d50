"""Measurements of profiles/incremental_context.md (one MI355X, one process per table, the variants alternating):

  python tools/extend_bench.py append     npf_append_points at B = 256, F = 256, capacity 1024, N in {1, 32, 256}: GB/s of the rows moved
                                          (read + written), device time from HIP events around batches of launches
  python tools/extend_bench.py extend     Conditioned.extend(N = 1) at 64 / 256 / 1024 stored rows against condition(..., n_cntxt=...) on
                                          C + 1 points (the route a frozen Conditioned leaves), AttnCNP and CNP at r = 256, B = 256
  python tools/extend_bench.py rollout    one rollout step (query at 1 point + draw + extend), eager and as one replayed graph

Run each table as a command of its own under a time limit (``timeout -k 10 300 python tools/extend_bench.py append``).  Every timing:
every shape warmed up, ``--reps`` repetitions of each variant in turn, min ... max over the repetitions as one JSON line per row."""
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


def _model(kind, r=256):
    import npf_gwwaveform_amd as A

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(r_dim=r, XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=r), is_sum_merge=True),
                  Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=4, hidden_size=r), is_sum_merge=True))
        return getattr(A, kind)(1, 2, **kw).to(DEV).eval()


def append(args):
    from npf_gwwaveform_amd import functional as FN
    from npf_gwwaveform_amd.chain import pt_shape

    B, F, M = 256, 256, 1024
    dst = torch.zeros(pt_shape(B, M, F), device=DEV)
    zero, counts = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    for N in (1, 32, 256):
        src = torch.randn(pt_shape(B, N, F), device=DEV)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for rep in range(args.reps + 1):
            counts.copy_(zero + 17)  # (an offset inside a tile: two destination runs per source tile)
            e0.record()
            for _ in range(3):  # 17 + 3 N <= 1024: every row is written
                FN.append_points([(src, dst, F)], counts, None, B, N, M)
            e1.record()
            torch.cuda.synchronize()
            if rep:  # (the first batch warms up)
                us.append(e0.elapsed_time(e1) / 3 * 1e3)
        moved = 2 * B * N * F * 4
        print(json.dumps({"table": "append", "N": N, "us_min": round(min(us), 2), "us_max": round(max(us), 2), "bytes_moved": moved,
                          "GB_per_s_best": round(moved / min(us) / 1e3, 1), "note": "two launches (rows, counts) per call"}))


def extend(args):
    B = 256
    for kind in ("AttnCNP", "CNP"):
        model = _model(kind)
        for C in (64, 256, 1024):
            X, Y = torch.rand(B, C + 1, 1, device=DEV) * 2 - 1, torch.randn(B, C + 1, 2, device=DEV)
            x1, y1 = X[:, C:].contiguous(), Y[:, C:].contiguous()
            n_all = torch.full((B,), C + 1, dtype=torch.int32, device=DEV)
            post = model.condition_with_capacity(X[:, :C].contiguous(), Y[:, :C].contiguous(), C + 32)
            zero = torch.zeros(B, dtype=torch.int32, device=DEV)

            def ext():
                post.n_rows_bound = C  # (the same stored size every time: the row appended is not counted, n_new = 0 below ...
                post.extend(x1, y1, n_new=zero)  # ... keeps the device counts at C; the launches are those of a real extension)

            ms = alternate({"extend(N=1)": ext, "condition(C+1, n_cntxt)": lambda: model.condition(X, Y, n_cntxt=n_all)},
                           args.reps, args.steps)
            for k, v in ms.items():
                print(json.dumps({"table": "extend", "model": kind, "stored_rows": C, "variant": k, "ms_min": round(min(v), 4),
                                  "ms_max": round(max(v), 4)}))


def rollout(args):
    B, C = 256, 128
    for kind in ("AttnCNP", "CNP"):
        model = _model(kind)
        X, Y = torch.rand(B, C, 1, device=DEV) * 2 - 1, torch.randn(B, C, 2, device=DEV)
        x_s, eps_s = torch.rand(B, 1, 1, device=DEV) * 2 - 1, torch.randn(B, 1, 2, device=DEV)
        zero = torch.zeros(B, dtype=torch.int32, device=DEV)

        def step(post):
            d = post.query(x_s).base_dist
            post.n_rows_bound = C
            return post.extend(x_s, d.loc[0] + d.scale[0] * eps_s, n_new=zero)  # (n_new = 0: the stored size stays C, same launches)

        eager, captured = (model.condition_with_capacity(X, Y, C + 32) for _ in range(2))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step(captured)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(captured)
        ms = alternate({"eager": lambda: step(eager), "one replayed graph": graph.replay}, args.reps, args.steps)
        for k, v in ms.items():
            print(json.dumps({"table": "rollout step", "model": kind, "stored_rows": C, "variant": k, "ms_min": round(min(v), 4),
                              "ms_max": round(max(v), 4)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["append", "extend", "rollout"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    {"append": append, "extend": extend, "rollout": rollout}[a.what](a)
