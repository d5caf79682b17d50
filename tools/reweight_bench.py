"""``python -m tools.reweight_bench``: S = 32 bootstrap replicates of AttnCNP r = 256 at B = 16, C = 256, T = 1024: Conditioned.reweighted against the parent-commit way
(condition + query on a batch tiled 32 times with the rows physically resampled).  Device events around synchronised work; the two
ways alternate inside one process; the medians and the spread over the rounds are printed."""
import json
import statistics
import sys
import warnings

import torch

import npf_gwwaveform_amd as A

DEV = "cuda:0"
B, C, T, S, R = 16, 256, 1024, 32, 256
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    m = A.AttnCNP(1, 2, r_dim=R).to(DEV).eval()
Xc = torch.rand(B, C, 1, device=DEV) * 2 - 1
Yc = torch.randn(B, C, 2, device=DEV)
Xt = (torch.rand(B, T, 1, device=DEV) * 2 - 1)
n = torch.full((B,), C, dtype=torch.int32, device=DEV)
W = A.bootstrap_weights(n, S, C, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
# the parent-commit batch: task s * B + b holds task b's rows repeated by W[s, b] (sum = C rows each)
idx = torch.repeat_interleave(torch.arange(C, device=DEV).repeat(S * B), W.reshape(-1).long()).view(S * B, C)
X_big = Xc.repeat(S, 1, 1).gather(1, idx.unsqueeze(-1).expand(S * B, C, 1)).contiguous()
Y_big = Yc.repeat(S, 1, 1).gather(1, idx.unsqueeze(-1).expand(S * B, C, 2)).contiguous()
Xt_big = Xt.repeat(S, 1, 1).contiguous()
n_big = n.repeat(S)
post = m.condition(Xc, Yc, n_cntxt=n)


def new_way():
    d = post.reweighted(W).query(Xt).base_dist
    return d.loc, d.scale


def new_way_with_encode():
    d = m.condition(Xc, Yc, n_cntxt=n).reweighted(W).query(Xt).base_dist
    return d.loc, d.scale


def parent_way():
    d = m.condition(X_big, Y_big, n_cntxt=n_big).query(Xt_big).base_dist
    return d.loc, d.scale


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


ways = {"reweighted (state stored)": new_way, "reweighted incl. condition": new_way_with_encode, "parent: tiled condition + query": parent_way}
a, b = new_way(), parent_way()
torch.cuda.synchronize()
diff = {k: float((x - y).abs().max()) for k, x, y in (("loc", a[0], b[0]), ("scale", a[1], b[1]))}
top = {"loc": float(b[0].abs().max()), "scale": float(b[1].abs().max())}
mem = {}
for name, fn in ways.items():
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    mem[name] = (torch.cuda.max_memory_allocated() - base) / 2**20
times = {k: [] for k in ways}
for rnd in range(7):
    for name, fn in ways.items():
        times[name].append(timed(fn, 20))
out = dict(shape=dict(B=B, C=C, T=T, S=S, r=R), max_abs_diff=diff, max_abs_ref=top, peak_extra_MiB=mem,
           ms_per_call={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()})
print(json.dumps(out, indent=1))
sys.stdout.flush()
