#!/usr/bin/env python3
"""The reference's 1-D workflow on the MI355X path, end to end: synthetic waveform-like functions,
random context / target split on the device, AttnCNP with transformer attention (what the
reference's notebooks and shipped checkpoints use), Adam, checkpoint in skorch's layout.

    python examples/train_attncnp_1d.py [--steps 200] [--dtype bf16] [--per-task-contexts | --ragged] [--predict] [--rollout] [--loo] [--score] [--match]

Only the import line differs from a script written against the reference:
    from npf import AttnCNP, CNPFLoss                      # reference
    from npf_gwwaveform_amd import AttnCNP, CNPFLoss       # this package
"""
import argparse
import os
import sys
import time
import warnings
from functools import partial

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import npf_gwwaveform_amd as A  # noqa: E402
from npf_gwwaveform_amd.train import Trainer  # noqa: E402


def functions(n_tasks, n_points, device, seed):
    """Smooth random 1-D functions on sorted random inputs in [-1, 1] (amplitude / phase like)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x, _ = torch.sort(torch.rand(n_tasks, n_points, 1, generator=g, device=device) * 2 - 1, dim=1)
    th = torch.rand(n_tasks, 1, 4, generator=g, device=device)
    y = torch.cat([(1.5 + x / 2).pow(-7 / 6) * (1 + th[..., :1]), torch.sin(6 * th[..., 1:2] * x + 6 * th[..., 2:3])], dim=-1)
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tasks", type=int, default=64)
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--r", type=int, default=128)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--graph", action="store_true", help="replay the step from a captured HIP graph (fixed batch shapes)")
    ap.add_argument("--per-task-contexts", action="store_true",
                    help="every task draws its own context size; the batch comes padded with the sizes as n_cntxt and the "
                         "step is replayed from ONE captured graph (implies --graph)")
    ap.add_argument("--ragged", action="store_true",
                    help="waveforms of different lengths: every task has its own number of samples (between a quarter of --points "
                         "and --points), the data set comes padded with the lengths as n_points, the batch carries n_cntxt and "
                         "n_trgt, and ONE captured graph serves every mix (implies --per-task-contexts)")
    ap.add_argument("--predict", action="store_true",
                    help="after training: condition the model on 16 points of one new function and print the predicted mean and "
                         "95 %% band on a refined grid (model.predict)")
    ap.add_argument("--rollout", action="store_true",
                    help="after training (fp32): condition on 16 points of one new function with room to grow and draw ONE "
                         "autoregressive sample on a 32-point grid (Conditioned.rollout: query, draw, feed the draw back)")
    ap.add_argument("--loo", action="store_true",
                    help="after training (fp32): the leave-one-out check of a 16-point context of one new function, one of whose "
                         "observations is a glitch -- every point predicted from the other 15 out of one encode (model.loo)")
    ap.add_argument("--score", action="store_true",
                    help="after training: score held-out targets of 64 new functions under the predictive distribution "
                         "(HeadDistribution.score): mean log density, mean CRPS and the PIT decile counts")
    ap.add_argument("--match", action="store_true",
                    help="after training: the mismatch of the predicted waveforms A e^{i phi} of 64 new functions against the true "
                         "ones, maximised over a constant phase and a grid of time shifts (HeadDistribution.match)")
    ap.add_argument("--out", default="/tmp/npf_example_ckpt")
    args = ap.parse_args()
    dev = "cuda:0"
    if args.ragged:
        args.per_task_contexts = True
    if args.per_task_contexts:
        args.graph = True
    A.set_compute_dtype(args.dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = A.AttnCNP(1, 2, r_dim=args.r, attention="transformer",
                          XYEncoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=2, hidden_size=args.r), is_sum_merge=True),
                          Decoder=A.merge_flat_input(partial(A.MLP, n_hidden_layers=4, hidden_size=args.r), is_sum_merge=True)).to(dev)
    trainer = Trainer(model, A.CNPFLoss(), lr=1e-3, world=1, use_graph=args.graph)
    trainer.set_lr_decay(10, max(args.steps // 50, 1))
    # (a captured graph needs fixed shapes: a fixed number of context points per batch in that mode)
    n_ctx = dict(a=32, b=32) if args.graph else dict(a=0.1, b=0.5)
    if args.per_task_contexts:  # (sizes as data: the context tensors keep the shape of the largest size)
        n_ctx = dict(a=0.1, b=0.5, is_per_task=True)
    split = A.CntxtTrgtGetter(contexts_getter=A.GetRandomIndcs(**n_ctx), targets_getter=A.get_all_indcs)
    t0 = time.perf_counter()
    for step in range(args.steps):
        X, Y = functions(args.tasks, args.points, dev, seed=step)
        if args.ragged:  # (lengths drawn on the device; the samples beyond a task's length are padding the getter never picks)
            n = torch.randint(args.points // 4, args.points + 1, (args.tasks,), device=dev,
                              generator=torch.Generator(device=dev).manual_seed(10 ** 6 + step))
            loss = trainer.step(split.batch(X, Y, n_points=n))
        else:
            loss = trainer.step(split.batch(X, Y))
        if (step + 1) % 50 == 0:
            print(f"step {step + 1:5d}  loss/task {loss.item():9.3f}  lr {trainer.end_epoch():.2e}  "
                  f"{(step + 1) * args.tasks * args.points / (time.perf_counter() - t0):,.0f} target-points/s")
    trainer.save_checkpoint(args.out, history=[{"steps": args.steps, "loss": float(loss)}])
    print("checkpoint:", sorted(os.listdir(args.out)))
    if args.predict:
        if args.dtype == "fp32":
            model.eval()
        X, Y = functions(1, args.points, dev, seed=10 ** 7)
        ctx = torch.linspace(0, args.points - 1, 16, device=dev).long()
        grid = torch.linspace(-1, 1, 4 * args.points, device=dev).view(1, -1, 1)  # (finer than anything the model was trained on)
        pred = model.predict(X[:, ctx], Y[:, ctx], grid)  # Prediction(mean, std, quantiles [3, 1, T, 2], probs)
        print("   x      mean(y0)  2.5 %    97.5 %   mean(y1)  2.5 %    97.5 %")
        for t in range(0, grid.shape[1], grid.shape[1] // 16):
            row = [grid[0, t, 0]] + [v for d in (0, 1) for v in (pred.mean[0, t, d], pred.quantiles[0, 0, t, d], pred.quantiles[2, 0, t, d])]
            print("  ".join(f"{float(v):7.3f}" for v in row))
    if args.rollout and args.dtype == "fp32":  # (a growing context runs the masked route: fp32 only)
        model.eval()
        X, Y = functions(1, args.points, dev, seed=10 ** 7)
        ctx = torch.linspace(0, args.points - 1, 16, device=dev).long()
        grid = torch.linspace(-1, 1, 32, device=dev).view(1, -1, 1)
        post = model.condition_with_capacity(X[:, ctx], Y[:, ctx], capacity=16 + 32)
        sample = post.rollout(grid)  # [1, 32, 2]; ``post`` is now conditioned on the 16 points and the 32 draws
        print("autoregressive sample   x      y0       y1")
        for t in range(0, 32, 4):
            print(f"                     {float(grid[0, t, 0]):7.3f}  {float(sample[0, t, 0]):7.3f}  {float(sample[0, t, 1]):7.3f}")
    if args.loo and args.dtype == "fp32":  # (the masked route: fp32 only)
        model.eval()
        X, Y = functions(1, args.points, dev, seed=10 ** 7)
        ctx = torch.linspace(0, args.points - 1, 16, device=dev).long()
        Xc, Yc = X[:, ctx].contiguous(), Y[:, ctx].clone()
        Yc[0, 7, 1] += 1.0  # (the glitch)
        p = model.loo(Xc, Yc)  # HeadDistribution [1, 1, 16] x [2]: point i given the other 15
        log_density = p.log_prob(Yc.unsqueeze(0))[0, 0]
        resid = ((Yc - p.base_dist.loc[0]) / p.base_dist.scale[0])[0]
        print("leave-one-out   x     log p(y_i | others)   residual / sigma (y0, y1)")
        for i in range(16):
            print(f"             {float(Xc[0, i, 0]):7.3f}  {float(log_density[i]):12.3f}          {float(resid[i, 0]):7.2f} {float(resid[i, 1]):7.2f}"
                  + ("   <- glitch" if i == 7 else ""))
    if args.score:
        if args.dtype == "fp32":
            model.eval()
        X, Y = functions(64, args.points, dev, seed=10 ** 7 + 1)
        ctx = torch.linspace(0, args.points - 1, 16, device=dev).long()
        held = torch.ones(args.points, dtype=torch.bool, device=dev)
        held[ctx] = False
        Xt, Yt = X[:, held].contiguous(), Y[:, held].contiguous()
        with torch.no_grad():
            s = model(X[:, ctx].contiguous(), Y[:, ctx].contiguous(), Xt)[0].score(Yt)  # Score(log_density, pit, crps), [64, T, 2] each
        print(f"held-out targets: mean log density {float(s.log_density.mean()):.3f}, mean CRPS {float(s.crps.mean()):.4f} (per output dim)")
        # (no padded rows here; with n_trgt the histogram must be masked by the counts: rows beyond them hold pit = 0.5)
        print("PIT decile counts (flat for a calibrated model):", torch.histc(s.pit, bins=10, min=0.0, max=1.0).long().tolist())
    if args.match:
        if args.dtype == "fp32":
            model.eval()
        X, Y = functions(64, args.points, dev, seed=10 ** 7 + 2)
        ctx = torch.linspace(0, args.points - 1, 16, device=dev).long()
        Xt = torch.linspace(-1, 1, args.points, device=dev).view(1, -1, 1).expand(64, -1, -1).contiguous()  # (a uniform frequency grid)
        th = torch.rand(64, 1, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        Yt = torch.cat([(1.5 + Xt / 2).pow(-7 / 6) * (1 + th[..., :1]), torch.sin(6 * th[..., 1:2] * Xt + 6 * th[..., 2:3])], dim=-1)
        freqs = 20.0 + (Xt[0, :, 0] + 1) * 246.0                   # x in [-1, 1] stands for 20 .. 512 Hz
        weights = 4.0 * (freqs[1] - freqs[0]) * (freqs / 100.0).pow(-2)  # 4 df / S_n(f) of a toy noise curve
        with torch.no_grad():
            m = model(Xt[:, ctx].contiguous(), Yt[:, ctx].contiguous(), Xt)[0].match(Yt, weights=weights, freqs=freqs,
                                                                                      taus=(-16 / 2048, 1 / 2048, 33))
        print(f"mismatch over 64 new waveforms: median {float(m.mismatch.median()):.3e}, worst {float(m.mismatch.max()):.3e}; "
              f"overlap without phase / time maximisation: median {float(m.overlap.median()):.4f}; "
              f"time shifts found: {float(m.tau.min()) * 1e3:.2f} .. {float(m.tau.max()) * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
