"""Measurements of profiles/waveform_match_bank.md (one MI355X, one process, the variants alternating):

  python tools/match_bank_bench.py [--reps 3] [--steps 3]   functional.waveform_match_bank at 256 rows, G = 1024 templates,
                                                            pts = 1024, n_tau = 64 against the same result from G calls of
                                                            functional.waveform_match, one template broadcast over the rows each

The loop is what the library offered before the bank call (``waveform_match`` is unchanged by it).  The method is that of
tools/predict_bench.py: a host clock around work that ends in a device synchronise, every shape warmed up, ``--reps`` repetitions of
each variant in turn; min ... max over the repetitions are printed as one JSON line per variant, with the largest difference between
the two results and the double-precision rate of the contraction: 8 R G pts real operations per shift (a complex multiply-add per
(row, template, point)), n_tau shifts, over the time of the whole call (three launches), so a lower bound of the kernel's own rate."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import DEV, alternate  # noqa: E402


def main(args):
    from npf_gwwaveform_amd import functional as FN

    R, G, T, n_tau = args.rows, args.bank, args.pts, args.n_tau
    g = torch.Generator(device=DEV).manual_seed(1)
    h = torch.stack([0.5 + torch.rand(R, T, device=DEV, generator=g), 3.0 * torch.randn(R, T, device=DEV, generator=g)], -1)
    bank = torch.stack([0.5 + torch.rand(G, T, device=DEV, generator=g), 3.0 * torch.randn(G, T, device=DEV, generator=g)], -1)
    f = torch.linspace(20.0, 512.0, T, device=DEV)
    w = 0.5 + torch.rand(T, device=DEV, generator=g)
    taus = (-(n_tau // 2) / 2048.0, 1.0 / 2048.0, n_tau)
    want = ("match", "tau_index", "phase")

    def bank_call():
        return FN.waveform_match_bank(h, bank, w, f, taus, want=want)

    def loop():
        out = [FN.waveform_match(h, bank[k:k + 1], w, f, taus, want=want) for k in range(G)]
        return tuple(torch.stack([getattr(m, name) for m in out], 1) for name in want)

    got, ref = bank_call(), loop()
    diff = float((got.match.double() - ref[0].double()).abs().max())
    same_index = float((got.tau_index == ref[1]).double().mean())
    flops = 8.0 * R * G * T * max(n_tau, 1)
    ms = alternate({"waveform_match_bank": bank_call, f"{G} calls of waveform_match": loop}, args.reps, args.steps)
    for k, v in ms.items():
        row = {"table": "match_bank", "rows": R, "G": G, "pts": T, "n_tau": n_tau, "variant": k, "ms_min": round(min(v), 4),
               "ms_max": round(max(v), 4), "max_abs_match_diff": diff, "tau_index_equal_share": same_index}
        if k == "waveform_match_bank":
            row["f64_tflops_at_ms_min"] = round(flops / (min(v) * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)
    a, b = min(ms["waveform_match_bank"]), min(ms[f"{G} calls of waveform_match"])
    print(json.dumps({"table": "match_bank", "loop_over_bank_call": round(b / a, 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--bank", type=int, default=1024)
    ap.add_argument("--pts", type=int, default=1024)
    ap.add_argument("--n-tau", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a)
