"""Measurements of profiles/waveform_match.md (one MI355X, one process, the variants alternating):

  python tools/match_bench.py [--reps 3] [--steps 10]   HeadDistribution.match at B = 256, T = 1024, n_tau = 512 of an AttnCNP
                                                        prediction (one row per task) and of an AttnLNP prediction at n_z = 32,
                                                        against the eager complex128 torch composition on the same device

The eager composition is the reference, not the code under test: ``loc`` materialised, ``exp(1j * (theta + 2 pi f tau_j))`` over a
[rows, T, n_tau] complex128 temporary (chunked over the rows to stay below ``--eager-bytes``), sums, abs, max.  The method is that of
tools/predict_bench.py: a host clock around work that ends in a device synchronise, every shape warmed up, ``--reps`` repetitions
of each variant in turn; min ... max over the repetitions are printed as one JSON line per table row, with the largest difference
between the two results."""
import argparse
import json
import math
import os
import sys
import warnings
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import DEV, alternate  # noqa: E402


def model_of(kind, r, n_z):
    import npf_gwwaveform_amd as A

    kw = dict(r_dim=r, XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=r), is_sum_merge=True),
              Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=4, hidden_size=r), is_sum_merge=True))
    if kind == "AttnLNP":
        kw.update(n_z_samples_train=n_z, n_z_samples_test=n_z)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(A, kind)(1, 2, **kw).to(DEV).eval()


def eager_match(p, Y, w, f, taus, chunk_bytes):
    """(overlap, match, mismatch, tau_index, phase) [n_z, B] by complex128 torch ops on base_dist.loc."""
    n_z, B, T = p.batch_shape
    loc = p.base_dist.loc.double()
    A_, ph = loc[..., 0], loc[..., 1]
    Ag, phg = Y[..., 0].double(), Y[..., 1].double()
    wd, fd = w.double(), f.double()
    tau = taus[0] + torch.arange(taus[2], dtype=torch.float64, device=Y.device) * taus[1]
    a, theta = wd * A_ * Ag, ph - phg
    nrm = ((wd * A_ * A_).sum(-1) * (wd * Ag * Ag).sum(-1)).sqrt()
    c0 = (a * torch.exp(1j * theta)).sum(-1)
    rot = 2.0 * math.pi * fd.view(1, T, 1) * tau.view(1, 1, -1)  # [1, T, n_tau], shared by the rows
    a, theta = a.reshape(n_z * B, T), theta.reshape(n_z * B, T)
    rows = max(1, chunk_bytes // (T * taus[2] * 16 * 3))  # (about three complex128 temporaries of a chunk alive at once)
    c = torch.cat([(a[i:i + rows].unsqueeze(2) * torch.exp(1j * (theta[i:i + rows].unsqueeze(2) + rot))).sum(1)
                   for i in range(0, n_z * B, rows)]).view(n_z, B, -1)
    best, idx = c.abs().max(-1)
    cb = c.gather(-1, idx.unsqueeze(-1))[..., 0]
    return c0.real / nrm, best / nrm, 1.0 - best / nrm, idx, torch.atan2(cb.imag, cb.real)


def main(args):
    B, T, C, n_tau = 256, 1024, 128, 512
    g = torch.Generator(device=DEV).manual_seed(1)
    Xc = torch.rand(B, C, 1, device=DEV, generator=g) * 2 - 1
    Yc = torch.randn(B, C, 2, device=DEV, generator=g)
    Xt = torch.linspace(-1, 1, T, device=DEV).view(1, T, 1).expand(B, T, 1).contiguous()
    Y = torch.stack([0.5 + torch.rand(B, T, device=DEV, generator=g), 3.0 * torch.randn(B, T, device=DEV, generator=g)], -1)
    f = torch.linspace(20.0, 512.0, T, device=DEV)
    w = 0.5 + torch.rand(T, device=DEV, generator=g)
    taus = (-256.0 / 2048.0, 1.0 / 2048.0, n_tau)
    for kind, n_z in (("AttnCNP", 1), ("AttnLNP", 32)):
        torch.manual_seed(7)
        model = model_of(kind, args.r, n_z)
        p = model.condition(Xc, Yc).query(Xt)
        assert tuple(p.batch_shape) == (n_z, B, T)
        p.base_dist  # (materialised once: the eager variant is not charged for the head)
        got, ref = p.match(Y, weights=w, freqs=f, taus=taus), eager_match(p, Y, w, f, taus, args.eager_bytes)
        diff = {k: float((getattr(got, k).double() - r).abs().max()) for k, r in zip(("overlap", "match", "mismatch"), ref)}
        same_index = bool((got.tau_index.long() == ref[3]).all())
        ms = alternate({"HeadDistribution.match": lambda: p.match(Y, weights=w, freqs=f, taus=taus),
                        "match, of='mean'": lambda: p.match(Y, weights=w, freqs=f, taus=taus, of="mean"),
                        "eager complex128 torch": lambda: eager_match(p, Y, w, f, taus, args.eager_bytes)}, args.reps, args.steps)
        for k, v in ms.items():
            print(json.dumps({"table": "match", "model": kind, "n_z": n_z, "B": B, "T": T, "n_tau": n_tau, "variant": k,
                              "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "max_abs_diff_vs_eager": diff,
                              "tau_index_equal": same_index}), flush=True)
        del model, p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--r", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--eager-bytes", type=int, default=4 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a)
