"""A/B of one sample's metadata sensitivity sweeps (latitude sweep + longitude sweep, 50 rows each; the reference's
test/metadata_sensitivity.py:289-366) for both model types at the production tile: 250 x 250 x 23, 8 metadata features,
base_filters 64, bf16, B = 50, one process, the two routes timed alternately:

    A = what the library offered before ``mau_amd.sensitivity``:
          "unet++": the eval forward on the tile repeated 50 times, ``.cpu().numpy()``, ``np.mean`` per sample and channel;
          "unet":   ``forward_metadata_sweep`` followed by the same host reduction;
    B = ``sensitivity.sweep_means`` over the 100 rows in chunks of 50 (encoder once per sample, head + fp64 mean in one launch,
        a (100, 2) table read back).

Every round times A once, then B once, the device synchronised before every clock read; the figure of a route is the median
of its rounds, its spread their (max - min).  Also: peak device memory of each route (``torch.cuda.max_memory_allocated``)
and the largest difference between the two routes' curves.  One JSON line on stdout (and in ``--out``) with the library's sha256.

    python scripts/sensitivity_ab.py --rounds 5 --out profiles/r8/sensitivity_ab.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MAU_QUIET", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mau_amd  # noqa: E402
from mau_amd import _lib  # noqa: E402
from mau_amd import sensitivity as S  # noqa: E402

TEMP_MEAN, TEMP_STD = 14.5, 8.25          # un-normalisation of the temperature channel (channel 1)


def host_means(out: torch.Tensor) -> np.ndarray:
    """The reference's reduction: the maps to the host, temperature un-normalised, np.mean over (H, W)."""
    o = out.cpu().numpy()
    o[:, 1] = o[:, 1] * TEMP_STD + TEMP_MEAN
    return np.mean(o, axis=(2, 3))


def route_a(net, model_type, x, ts, rows):
    res = []
    with torch.no_grad():
        for md in rows:
            B = md.shape[0]
            if model_type == "unet":
                out = net.forward_metadata_sweep(x, ts, md)
            else:
                out = net(x.repeat(B, 1, 1, 1), ts.repeat(B, 1), md)
            res.append(host_means(out))
    return np.concatenate(res)


def route_b(net, x, ts, rows):
    return S.sweep_means(net, x, ts, torch.cat(rows), scale=[1.0, TEMP_STD], shift=[0.0, TEMP_MEAN]).cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=250)
    ap.add_argument("--rows", type=int, default=50)
    ap.add_argument("--base-filters", type=int, default=64)
    ap.add_argument("--seq-len", type=int, default=828)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rec = {"workload": f"{args.size}x{args.size}x23, 8 metadata features, base_filters {args.base_filters}, bf16, latitude + longitude sweep of "
                       f"{args.rows} rows each, series of {args.seq_len}",
           "lib_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "models": {}}
    for model_type in ("unet", "unet++"):
        torch.manual_seed(0)
        net = mau_amd.UrbanPredictor(model_type, 23, args.seq_len, 16, 8, 8, 32, 2, base_filters=args.base_filters).cuda().set_precision("bf16").eval()
        g = torch.Generator().manual_seed(1)
        x, ts = torch.randn(1, 23, args.size, args.size, generator=g).cuda(), torch.randn(1, args.seq_len, generator=g).cuda()
        md, t1, t2 = torch.randn(1, 4, generator=g).cuda(), torch.randn(1, 2, generator=g).cuda(), torch.randn(1, 2, generator=g).cuda()
        mean, std = [20.0, 10.0, 0.0, 0.0], [25.0, 70.0, 1.0, 1.0]
        rows = [S.metadata_rows(md, t1, t2, 0, np.linspace(-60, 70, args.rows), mean, std, 8),
                S.metadata_rows(md, t1, t2, 1, np.linspace(-180, 180, args.rows), mean, std, 8)]
        fa = lambda: route_a(net, model_type, x, ts, rows)          # noqa: E731
        fb = lambda: route_b(net, x, ts, rows)                       # noqa: E731
        ra, rb = fa(), fb()                                          # warm-up of both routes (allocator, weight packs)
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(fa)[0])
            tb.append(timed(fb)[0])
        m = {"A_ms": ta, "B_ms": tb, "A_median_ms": statistics.median(ta), "B_median_ms": statistics.median(tb),
             "A_spread_ms": max(ta) - min(ta), "B_spread_ms": max(tb) - min(tb),
             "A_peak_MiB": peak_mib(fa), "B_peak_MiB": peak_mib(fb),
             "max_abs_curve_difference": float(np.abs(ra.astype(np.float64) - rb).max())}
        m["speedup"] = m["A_median_ms"] / m["B_median_ms"]
        m["B_not_slower_beyond_spread"] = m["B_median_ms"] <= m["A_median_ms"] + max(m["A_spread_ms"], m["B_spread_ms"])
        rec["models"][model_type] = m
        del net
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(m["B_not_slower_beyond_spread"] for m in rec["models"].values()) else 1


if __name__ == "__main__":
    raise SystemExit(main())
