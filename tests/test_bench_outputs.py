"""bench.py's plain run and --dump-outputs: exactly --steps timed steps, the headline keys only, and the arrays of the last
timed step written as .npy (float32, 64 MB at most, a seeded sample of what does not fit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_limit_and_seeded_sample(tmp_path):
    g = torch.Generator().manual_seed(5)
    arrays = {"outputs": torch.randn(8, 2, 64, 64, generator=g), "loss": torch.tensor(0.25),
              "params": torch.randn(20_000_000, generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == ["loss", "outputs", "params"]
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in a) <= bench.DUMP_LIMIT_BYTES
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["outputs"], arrays["outputs"].numpy()) and float(a["loss"]) == 0.25       # small arrays: whole
    assert 0 < a["params"].size < 20_000_000 and np.array_equal(a["params"], b["params"])                # large: the same sample
    assert np.isin(a["params"][:100], arrays["params"].float().numpy()).all()


def test_cpu_baseline_b32_needs_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-b32"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--full" in p.stderr


def _plain(args, out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", "--size", "64", "--dump-outputs", str(out)] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), _files(out)


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    rec, a = _plain(["--steps", "3", "--warmup", "2"], tmp_path / "a")
    assert all(k in rec for k in HEADLINE) and rec["steps"] == 3 and rec["timed_regions"]["repeats"] == 1
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    assert not any(k in rec for k in ("roofline", "cpu_baseline", "ms_per_step_with_loss_readback", "fwd_ms_per_tile"))
    assert a["outputs"].shape == (2, 2, 64, 64) and np.isfinite(a["outputs"]).all()
    assert float(a["loss"]) == np.float32(rec["final_loss"]) and np.isfinite(a["params"]).all()
    # same arguments, same inputs: a second run computes what the first did
    rec2, b = _plain(["--steps", "3", "--warmup", "2"], tmp_path / "b")
    assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape for k in a)
    for k in a:
        err = float(np.abs(a[k].astype(np.float64) - b[k]).max() / max(1e-30, np.abs(a[k]).max()))
        assert err < 1e-3, (k, err)
    rec, c = _plain(["--infer", "--steps", "2", "--warmup", "1"], tmp_path / "c")
    assert sorted(c) == ["outputs"] and c["outputs"].shape == (2, 2, 64, 64) and rec["metric"].startswith("inference")
