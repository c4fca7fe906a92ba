#!/usr/bin/env python3
"""Timing of the ground-truth sensitivity path (mau_amd.ground_truth), one process, one device:
  1. BinStats.update (mau_plane_moments + mau_bin_moments) and plane_moments alone at (256, 2, 250, 250): alternating regions of 20
     back-to-back calls between device events, median of 30 regions;
  2. one pass over a synthetic split of 512 tiles (23 x 250 x 250 input, 2 x 250 x 250 target, compressed .npz, written by 16
     processes): ground_truth_sensitivity against a host pass that restates the reference script in float32 numpy on the same
     files and the same loader, and against the loader alone (every batch read and dropped) -- host clock around a synchronised pass.
Usage: python scripts/ground_truth_bench.py [out.json] [tiles]"""
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
METRICS = {"temp_mean": 29.4173, "temp_std": 11.0291, "meta_mean": [17.25, 9.5, 1250000.5, 2.125], "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
CHANNELS = ("after_ndvi", "after_temp")
H = W = 250


def write_tile(args):
    folder, i = args
    rng = np.random.default_rng(1000 + i)
    eye = np.eye(9, dtype=np.float32)
    a, b = rng.integers(0, 9, (H, W)), rng.integers(0, 9, (H, W))
    x = np.vstack([eye[a].transpose(2, 0, 1), rng.standard_normal((5, H, W)).astype(np.float32), eye[b].transpose(2, 0, 1)])
    tgt = np.stack([np.tanh(rng.standard_normal((H, W))), rng.standard_normal((H, W))]).astype(np.float32)
    meta = rng.standard_normal(4).astype(np.float32)                 # latitude 17 +- 22, longitude 10 +- 68: mostly in range
    np.savez_compressed(os.path.join(folder, f"City_{i}_41.8990_12.4690_2019_08_to_2021_08.npz"), input=x, target=tgt, metadata=meta,
                        temperature_serie=rng.standard_normal(24).astype(np.float32))


def host_pass(G, data, root, batch_size):
    """The reference script (generate_ground_truth_sensitivity.py:59-149) on the same loader: float32 per-pixel un-normalisation,
    every target kept, float32 np.mean / np.std per bin."""
    loader = data.create_dataloader("test", batch_size, False, processed_dir=root, device=None)
    meta_mean, meta_std = np.array(METRICS["meta_mean"]), np.array(METRICS["meta_std"])
    lats_all, lons_all, targets_all = [], [], []
    for batch in loader:
        md = batch.metadatas
        lats_all.append(md[:, 0].numpy() * meta_std[0] + meta_mean[0])
        lons_all.append(md[:, 1].numpy() * meta_std[1] + meta_mean[1])
        targets_np = batch.targets.numpy()
        un = np.zeros_like(targets_np)
        for i, ch in enumerate(CHANNELS):
            un[:, i] = targets_np[:, i] * METRICS["temp_std"] + METRICS["temp_mean"] if "temp" in ch else targets_np[:, i]
        targets_all.append(un)
    lats_all, lons_all, targets_all = np.concatenate(lats_all), np.concatenate(lons_all), np.concatenate(targets_all, axis=0)
    out = {}
    for name, x, centers in (("latitude", lats_all, G.LAT_RANGE), ("longitude", lons_all, G.LON_RANGE)):
        idx = np.digitize(x, G.bin_edges(centers))
        out[name] = {}
        for c, ch in enumerate(CHANNELS):
            y = targets_all[:, c]
            means = [float(np.mean(y[idx == i])) if np.any(idx == i) else float("nan") for i in range(1, 51)]
            stds = [float(np.std(y[idx == i])) if np.any(idx == i) else float("nan") for i in range(1, 51)]
            out[name][ch] = {"mean": means, "std": stds}
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    tiles = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    # the tiles first: the writer processes start before this process has touched the device
    tmp = tempfile.TemporaryDirectory()
    root = tmp.name
    split = {}
    if tiles > 0:
        import multiprocessing as mp
        os.makedirs(os.path.join(root, "test"))
        with open(os.path.join(root, "normalization_metrics.json"), "w") as f:
            json.dump(METRICS, f)
        t0 = time.perf_counter()
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(write_tile, [(os.path.join(root, "test"), i) for i in range(tiles)], chunksize=8)
        files = os.listdir(os.path.join(root, "test"))
        mb = sum(os.path.getsize(os.path.join(root, "test", f)) for f in files) / 1e6
        print(f"wrote {len(files)} tiles, {mb:.0f} MB, in {time.perf_counter() - t0:.1f} s", flush=True)
        split = {"tiles": len(files), "file_mb": mb, "batch_size": 256, "num_workers": 0}
    import mau_amd
    from mau_amd import data, ground_truth as G
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "shape": [256, 2, H, W]}

    # 1. the two launches
    rng = np.random.default_rng(0)
    t = torch.from_numpy(rng.standard_normal((256, 2, H, W)).astype(np.float32)).to(dev)
    md = torch.from_numpy(rng.standard_normal((256, 4)).astype(np.float32)).to(dev)
    st = G.BinStats([G.Axis("latitude", 0, G.LAT_RANGE, METRICS["meta_std"][0], METRICS["meta_mean"][0]),
                     G.Axis("longitude", 1, G.LON_RANGE, METRICS["meta_std"][1], METRICS["meta_mean"][1])], 2, dev)
    fns = {"update": lambda: st.update(t, md), "plane_moments": lambda: G.plane_moments(t)}
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(30):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / 20 * 1e3)
    nbytes = t.numel() * 4
    for k, v in times.items():
        med = statistics.median(v)
        res[k + "_us"] = {"median": med, "min": min(v), "max": max(v), "input_gb_per_s": nbytes / med / 1e3}
        print(f"{k}: {med:.1f} us per call (min {min(v):.1f}, max {max(v):.1f}); {nbytes / med / 1e3:.0f} GB/s of input")

    # 2. a pass over a split
    if tiles > 0:
        res["split"] = split

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r

        def loader_only():
            n = 0
            for b in data.create_dataloader("test", 256, False, processed_dir=root, device=None):
                n += len(b.targets)
            return n

        passes = {"device": [], "loader_only": [], "host_float32": []}
        d1, dev_res = timed(lambda: G.ground_truth_sensitivity(root, "test", 256))
        passes["device"].append(d1)
        d, n = timed(loader_only)
        passes["loader_only"].append(d)
        assert n == tiles
        d, host_res = timed(lambda: host_pass(G, data, root, 256))
        passes["host_float32"].append(d)
        worst = 0.0
        for axis in ("latitude", "longitude"):
            for ch in CHANNELS:
                for k in ("mean", "std"):
                    a, b = np.array(dev_res["sweeps"][axis]["channels"][ch][k]), np.array(host_res[axis][ch][k])
                    assert np.array_equal(np.isnan(a), np.isnan(b))
                    scale = max(1.0, float(np.nanmax(np.abs(a))))
                    worst = max(worst, float(np.nanmax(np.abs(a - b))) / scale)
        res["split"]["pass_seconds"] = passes
        res["split"]["device_vs_host_float32_worst_abs_over_scale"] = worst
        print("passes, s:", passes, "worst device / host-float32 deviation:", worst)
    tmp.cleanup()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
