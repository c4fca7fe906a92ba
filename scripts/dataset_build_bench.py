#!/usr/bin/env python3
"""Timing of the dataset build's kernel (mau_amd.dataset_build.raw_tile_process, mau_raw_tile_process), one process, one device, at
B = 64 of 250 x 250 in its three modes:
  rows    30 bytes per pixel read (two uint8 class maps, seven fp32 planes), one fp64 row per sample written;
  planes  28 bytes per pixel read (the class maps are not needed), 28 written (cont (B,5,H,W) and targets (B,2,H,W));
  both    30 read, 28 written.
Regions of 20 back-to-back calls between device events, median of 30 regions; bytes / s of what the mode reads plus what it writes.
mau_tile_stats (30 bytes per pixel read, nine moment rows of 8) is timed next to it in the same process, as the nearest comparable
kernel.
Usage: python scripts/dataset_build_bench.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = W = 250
B = 64
NORM = [0.4471, 0.4012, 0.3577, 0.2113, 0.1987, 0.2054, 301.337, 4.2971]


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 20 * 1e3)
    return times


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    import mau_amd  # noqa: F401
    from mau_amd import dataset_build as DB, dataset_metrics as D
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    a, b = (torch.from_numpy(rng.integers(0, 9, (B, H, W)).astype(np.uint8)).to(dev) for _ in range(2))
    rgb = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).to(dev)
    n1, n2 = (torch.from_numpy(np.tanh(rng.standard_normal((B, H, W))).astype(np.float32)).to(dev) for _ in range(2))
    t1, t2 = (torch.from_numpy((300 + 4 * rng.standard_normal((B, H, W))).astype(np.float32)).to(dev) for _ in range(2))
    norm = torch.tensor(NORM, dtype=torch.float64, device=dev)
    cont = torch.from_numpy(rng.standard_normal((B, 5, H, W)).astype(np.float32)).to(dev)
    tgt = torch.from_numpy(rng.standard_normal((B, 2, H, W)).astype(np.float32)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W]}
    modes = {"rows": (True, False, 30, 0), "planes": (False, True, 28, 28), "both": (True, True, 30, 28)}
    for name, (rows, planes, rd, wr) in modes.items():
        times = timed(lambda: DB.raw_tile_process(a, b, rgb, n1, n2, t1, t2, norm=norm, rows=rows, planes=planes))
        med = statistics.median(times)
        nbytes = B * H * W * (rd + wr)
        res[f"raw_tile_{name}_us"] = {"median": med, "min": min(times), "max": max(times), "bytes_per_pixel_read": rd,
                                      "bytes_per_pixel_written": wr, "gb_per_s": nbytes / med / 1e3}
        print(f"raw_tile_process[{name}]: {med:.1f} us per call (min {min(times):.1f}, max {max(times):.1f}); {nbytes / med / 1e3:.0f} GB/s "
              f"({rd} B/pixel read + {wr} written)", flush=True)
    times = timed(lambda: D.tile_stats(a, b, cont, tgt))
    med = statistics.median(times)
    res["tile_stats_us"] = {"median": med, "min": min(times), "max": max(times), "gb_per_s": B * H * W * 30 / med / 1e3}
    print(f"tile_stats: {med:.1f} us per call (min {min(times):.1f}, max {max(times):.1f}); {B * H * W * 30 / med / 1e3:.0f} GB/s of input", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
