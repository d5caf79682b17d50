"""``python -m tools.keyweight_bench``: the Trainer step of AttnCNP r = 128 (scaled-dot attention), 128 context / 256 target points,
B = 256, with ``n_cntxt`` = 128 everywhere against the same step with ``w_cntxt`` (log-uniform in [1/e, e]) on top -- eager and
HIP-graph replay.  Two trainers per mode, 5 alternating rounds of 30 steps each, device events around a round; the ms per step of
every round are printed sorted, as one JSON line (``profiles/weighted_training.md``)."""
import json
import warnings

import torch

import npf_gwwaveform_amd as A
from npf_gwwaveform_amd.train import Trainer, synthetic_waveform_batch

DEV = "cuda:0"
B, C, T = 256, 128, 256


def batch(i, weighted):
    b = synthetic_waveform_batch(B, C, T, 100 + i, DEV)
    b["n_cntxt"] = torch.full((B,), C, dtype=torch.int32, device=DEV)
    if weighted:
        g = torch.Generator().manual_seed(i)
        b["w_cntxt"] = torch.exp(torch.rand(B, C, generator=g) * 2 - 1).to(DEV)
    return b


def make(weighted, graph):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = A.AttnCNP(1, 2, r_dim=128).to(DEV)
    tr = Trainer(m, A.CNPFLoss(), lr=1e-3, world=1, use_graph=graph, defer_input_check=True)
    bs = [batch(i, weighted) for i in range(4)]
    for i in range(8):
        tr.step(bs[i % 4])
    torch.cuda.synchronize()
    return tr, bs


def timed(tr, bs, steps=30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(steps):
        tr.step(bs[i % 4])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


res = {}
for graph in (False, True):
    runs = {w: make(w, graph) for w in (False, True)}
    times = {False: [], True: []}
    for rnd in range(5):
        for w in (False, True):
            times[w].append(timed(*runs[w]))
    for w in (False, True):
        res[f"{'graph' if graph else 'eager'}_{'w_cntxt' if w else 'n_cntxt'}_ms"] = sorted(times[w])
print(json.dumps(res))
