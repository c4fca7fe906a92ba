#!/usr/bin/env python3
"""Timing of the climate stage's three launches (mau_amd.climate, csrc/climate.hip) at the sizes of the global 0.5 degree grid, one
process, one device, on synthetic data generated on the device (degrees Celsius, 30 % of the cells NaN in every month: the ocean):
  baseline   600 x 259 200 fp32 read twice (two passes), 259 200 rows of 4 fp64 written;
  normalise  828 x 259 200 fp32 read and written once, the rows read;
  series     4 096 queries of 828 months (random cells, random cuts) against the raw 828 x 259 200 grid.
Regions of 10 back-to-back calls between device events, median of 20 regions; bytes / s of what the launch must read plus write
(for the series: the 4 bytes of every value it gathers, not the memory lines they sit in).  The float64 numpy twins are timed next
to them on the same machine (one call each; series_host over the first 256 queries, scaled), after checking that the device's
results are the twins' on a sample of cells.
Usage: python scripts/climate_bench.py [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAT, LON = 360, 720
G = LAT * LON
T_BASE, T_OUT, N_QUERIES = 600, 828, 4096


def timed(fn, calls=10, regions=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / calls * 1e3)
    return times


def grid(T, gen, ocean):
    x = torch.empty((T, G), dtype=torch.float32, device="cuda")
    mean = torch.empty((1, G), dtype=torch.float32, device="cuda").uniform_(-25, 28, generator=gen)
    for t0 in range(0, T, 64):
        part = x[t0:t0 + 64]
        part.normal_(0.0, 3.0, generator=gen)
        part += mean
        part[:, ocean] = float("nan")
    return x


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    import mau_amd  # noqa: F401
    from mau_amd import climate as CL
    gen = torch.Generator(device="cuda").manual_seed(0)
    ocean = torch.rand(G, device="cuda", generator=gen) < 0.3
    base, raw = grid(T_BASE, gen, ocean), grid(T_OUT, gen, ocean)
    cell = torch.randint(0, G, (N_QUERIES,), device="cuda", generator=gen, dtype=torch.int32)
    keep = torch.randint(0, T_OUT + 1, (N_QUERIES,), device="cuda", generator=gen, dtype=torch.int32)
    rows = CL.baseline(base)
    res = {"device": torch.cuda.get_device_name(0), "grid": [LAT, LON], "months": [T_BASE, T_OUT], "queries": N_QUERIES}

    def report(name, times, nbytes):
        med = statistics.median(times)
        res[name] = {"median_us": med, "min_us": min(times), "max_us": max(times), "bytes": nbytes, "gb_per_s": nbytes / med / 1e3}
        print(f"{name}: {med:.1f} us per call (min {min(times):.1f}, max {max(times):.1f}); {nbytes / med / 1e3:.0f} GB/s", flush=True)

    report("baseline", timed(lambda: CL.baseline(base)), 2 * T_BASE * G * 4 + G * 32)
    report("normalise", timed(lambda: CL.normalise(raw, rows)), 2 * T_OUT * G * 4 + G * 32)
    kept = int(keep.sum())
    report("series", timed(lambda: CL.series(raw, rows, cell, keep)), 4 * kept + 4 * N_QUERIES * T_OUT + N_QUERIES * 72)

    # the twins on the same machine, and that the device computes what they compute
    base_h, raw_h, rows_h = base.cpu().numpy(), raw.cpu().numpy(), rows.cpu().numpy()
    same = lambda a, b: bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))     # noqa: E731
    t0 = time.perf_counter()
    twin_rows = CL.baseline_host(base_h)
    res["baseline_host_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    twin_norm = CL.normalise_host(raw_h, rows_h)
    res["normalise_host_s"] = time.perf_counter() - t0
    nq = 256
    t0 = time.perf_counter()
    twin_series, _ = CL.series_host(raw_h, rows_h, cell[:nq].cpu().numpy(), keep[:nq].cpu().numpy())
    res["series_host_s"] = (time.perf_counter() - t0) * N_QUERIES / nq
    res["same_as_twins"] = {"baseline": same(rows_h, twin_rows), "normalise": same(CL.normalise(raw, rows).cpu().numpy(), twin_norm),
                            "series": same(CL.series(raw, rows, cell[:nq], keep[:nq])[0].cpu().numpy(), twin_series)}
    print(f"twins: baseline_host {res['baseline_host_s']:.2f} s, normalise_host {res['normalise_host_s']:.2f} s, series_host "
          f"{res['series_host_s']:.2f} s (scaled from {nq} queries); device results equal to the twins': {res['same_as_twins']}", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
