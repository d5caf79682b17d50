"""bench.py's options: a plain run times the steps and prints the headline only (``--full`` adds the eager comparison, the
roofline pass and the CPU baseline); ``--dump-outputs DIR`` writes what the last timed step computed, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_plain_run_is_the_default_and_full_is_an_option():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.full, args.dump_outputs, args.steps, args.warmup, args.config) == (False, None, 7, 2, "c2")
    args = bench.parse_args(["--full", "--dump-outputs", "out", "--config", "c5"])
    assert (args.full, args.dump_outputs, args.workload) == (True, "out", "decode")


def test_dump_outputs_writes_float_arrays_and_samples_within_the_budget(tmp_path):
    g = torch.Generator().manual_seed(0)
    small = {"loss": torch.tensor([1.25]), "params": torch.randn(1000, generator=g), "d": torch.randn(3, dtype=torch.float64)}
    info = bench.dump_outputs(str(tmp_path / "small"), small)
    for name, t in small.items():
        a = np.load(tmp_path / "small" / f"{name}.npy")
        assert a.dtype == (np.float64 if name == "d" else np.float32) and info["arrays"][name]["sampled"] is None
        assert np.array_equal(a, t.numpy())
    # 2 x 48 MB of float32: each array keeps its share of the budget, the same elements every time
    big = {"loc": torch.arange(12 << 20, dtype=torch.float32), "scale": -torch.arange(12 << 20, dtype=torch.float32)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20
    for name in big:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b) and a.dtype == np.float32 and 0 < a.size < big[name].numel()
        idx = np.abs(a).astype(np.int64)  # (the values are their own flat indices)
        assert np.all(np.diff(idx) > 0) and np.array_equal(a, big[name].numpy()[idx])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    n_params = sum(p.numel() for p in bench.build_model("attncnp", 256, 4, "cpu")[0].parameters())
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "16", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - 16 * 1024 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and "eager" not in line
    loss, params, grad = (np.load(out / f"{n}.npy") for n in ("loss", "params", "grad"))
    assert loss.shape == (1,) and abs(float(loss[0]) - line["config"]["final_loss"]) <= 1e-6 * abs(float(loss[0]))
    assert params.shape == grad.shape == (n_params,) and params.dtype == grad.dtype == np.float32
    assert np.isfinite(params).all() and np.isfinite(grad).all() and np.abs(grad).max() > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_decode_line_names_the_kernel_it_runs(tmp_path):
    """The decode line's dtype names the x6 program kernel from the launches of the run itself, not from the --full pass."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c5", "--batch", "8", "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k != "NPF_NO_X6_FUSED"}
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=250)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["roofline"] is None and line["cpu_baseline"] is None
    assert line["dtype"].startswith("f32 (fp32 operands as three exact bf16 terms"), line["dtype"]
    loc, scale = np.load(tmp_path / "loc.npy"), np.load(tmp_path / "scale.npy")
    assert loc.shape == scale.shape == (1, 8, 4096, 2) and (scale > 0).all()
    assert abs(float(loc.astype(np.float64).sum()) - line["config"]["checksum_loc"]) <= 1e-6 * np.abs(loc).sum()
