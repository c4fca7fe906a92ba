#!/usr/bin/env python3
"""Timing of the dataset survey (mau_amd.dataset_metrics), one process, one device:
  1. tile_stats (mau_tile_stats) at B = 64 of 250 x 250 (30 bytes per pixel read): regions of 20 back-to-back calls between device
     events, median of 30 regions;
  2. one extract pass over a synthetic directory of tiles (23 x 250 x 250 input, 2 x 250 x 250 target, compressed .npz, written by
     16 processes) against the loader alone (every batch read, compacted and dropped) -- host clock around a synchronised pass --
     and the device time of the pass's launches (device events around every tile_stats call of an identical pass).
Usage: python scripts/dataset_metrics_bench.py [out.json] [tiles]"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METRICS = {"temp_mean": 296.4173, "temp_std": 11.0291, "temp_series_mean": 295.75, "temp_series_std": 9.125,
           "meta_mean": [17.25, 9.5, 1250000.5, 2.125], "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
H = W = 250
BYTES_PER_PIXEL = 2 + 4 * 5 + 4 * 2


def write_tile(args):
    folder, i = args
    rng = np.random.default_rng(1000 + i)
    eye = np.eye(9, dtype=np.float32)
    a, b = rng.integers(0, 9, (H, W)), rng.integers(0, 9, (H, W))
    x = np.vstack([eye[a].transpose(2, 0, 1), rng.standard_normal((5, H, W)).astype(np.float32), eye[b].transpose(2, 0, 1)])
    tgt = np.stack([np.tanh(rng.standard_normal((H, W))), rng.standard_normal((H, W))]).astype(np.float32)
    np.savez_compressed(os.path.join(folder, f"City_{i}_41.8990_12.4690_2019_08_to_2021_08.npz"), input=x, target=tgt,
                        metadata=rng.standard_normal(4).astype(np.float32), temperature_serie=rng.standard_normal(24).astype(np.float32))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    tiles = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    tmp = tempfile.TemporaryDirectory()
    root = tmp.name
    if tiles > 0:                                                     # the writer processes start before this process touches the device
        import multiprocessing as mp
        os.makedirs(os.path.join(root, "test"))
        with open(os.path.join(root, "normalization_metrics.json"), "w") as f:
            json.dump(METRICS, f)
        t0 = time.perf_counter()
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(write_tile, [(os.path.join(root, "test"), i) for i in range(tiles)], chunksize=8)
        print(f"wrote {tiles} tiles in {time.perf_counter() - t0:.1f} s", flush=True)
    import mau_amd
    from mau_amd import dataset_metrics as D
    from mau_amd.data import FuturePredictionDataset
    from torch.utils.data import DataLoader
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "shape": [64, H, W], "bytes_per_pixel": BYTES_PER_PIXEL}

    # 1. the launch
    rng = np.random.default_rng(0)
    B = 64
    a, b = (torch.from_numpy(rng.integers(0, 9, (B, H, W)).astype(np.uint8)).to(dev) for _ in range(2))
    cont = torch.from_numpy(rng.standard_normal((B, 5, H, W)).astype(np.float32)).to(dev)
    tgt = torch.from_numpy(rng.standard_normal((B, 2, H, W)).astype(np.float32)).to(dev)
    for _ in range(5):
        D.tile_stats(a, b, cont, tgt)
    torch.cuda.synchronize()
    times = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            D.tile_stats(a, b, cont, tgt)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 20 * 1e3)
    nbytes = B * H * W * BYTES_PER_PIXEL
    med = statistics.median(times)
    res["tile_stats_us"] = {"median": med, "min": min(times), "max": max(times), "input_gb_per_s": nbytes / med / 1e3}
    print(f"tile_stats: {med:.1f} us per call (min {min(times):.1f}, max {max(times):.1f}); {nbytes / med / 1e3:.0f} GB/s of input", flush=True)

    # 2. a pass over a directory
    if tiles > 0:
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r

        def loader_only():
            ds = FuturePredictionDataset("test", processed_dir=root, compact=True, skip_errors=True)
            return sum(len(files) for _, files in DataLoader(ds, batch_size=64, shuffle=False, collate_fn=D._collate))

        device_ms = []
        real = D.tile_stats

        def timed_stats(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rows = real(*args)
            e1.record()
            device_ms.append((e0, e1))
            return rows

        d_extract, df = timed(lambda: D.extract(root, batch_size=64))
        d_loader, n = timed(loader_only)
        assert n == tiles == len(df)
        D.tile_stats = timed_stats
        try:
            d_extract2, _ = timed(lambda: D.extract(root, batch_size=64))
        finally:
            D.tile_stats = real
        dev_s = sum(e0.elapsed_time(e1) for e0, e1 in device_ms) / 1e3
        res["pass"] = {"tiles": tiles, "batch_size": 64, "num_workers": 0, "extract_s": [d_extract, d_extract2], "loader_only_s": d_loader,
                       "device_s_between_events": dev_s}
        print("pass:", res["pass"], flush=True)
    tmp.cleanup()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
