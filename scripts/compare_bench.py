#!/usr/bin/env python3
"""Time one model comparison of a 250 x 250 tile, M = 3 (two base-64 U-Nets with 4 and 8 metadata features, one base-64 U-Net++), fp16,
828-step temperature series, two ways:

  session  ``ComparisonSession``: one hipGraph replay (pack -> three networks -> ``mau_compare_result``) and ONE read-back, the
           (6, 40) fp64 rows;
  eager    the same three frozen models run eagerly on the packed tile, then the page's un-normalise, subtract, min and max in torch
           operators over the tile and its four quadrants, every number read back as the page's numpy calls would (90 read-backs).

Five alternating pairs of windows of 40 calls, a host clock around each window that ends in a device synchronise.  Also counts the
library calls of both spellings (an entry point is one launch but for a few two-launch ones).

    timeout -k 10 300 python scripts/compare_bench.py [--json out.json]

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MAU_QUIET", "1")
import mau_amd  # noqa: E402
from mau_amd import compare as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
args = ap.parse_args()
H = W = 250
T = 828
METRICS = {"rgb_mean": [0.4312, 0.5127, 0.3989], "rgb_std": [0.2213, 0.1907, 0.2571], "temp_mean": 29.4173, "temp_std": 11.0291}
rng = np.random.default_rng(0)
g = torch.Generator().manual_seed(0)
sample = {"cls_a": torch.from_numpy(rng.integers(0, 9, (H, W)).astype(np.uint8)), "cls_b": torch.from_numpy(rng.integers(0, 9, (H, W)).astype(np.uint8)),
          "cont": torch.randn(5, H, W, generator=g), "metadata": torch.randn(4, generator=g), "temp_series": torch.randn(T, generator=g),
          "t1_date": torch.tensor([2019.0, 3.0]), "t2_date": torch.tensor([2022.0, 9.0]), "target": torch.randn(2, H, W, generator=g)}
palette = rng.integers(0, 256, (9, 3)).astype(np.uint8)
torch.manual_seed(1)
models = [("unet4", mau_amd.UrbanPredictor("unet", 23, T, 64, 4, 64, 96, 2).cuda().eval()),
          ("unet8", mau_amd.UrbanPredictor("unet", 23, T, 64, 8, 64, 96, 2).cuda().eval()),
          ("unetpp8", mau_amd.UrbanPredictor("unet++", 23, T, 64, 8, 64, 96, 2).cuda().eval())]
sess = C.ComparisonSession(models, sample, metrics=METRICS, palette=palette, precision="fp16", clone_output=False)


def session_once():
    r = sess()
    return r.stats.rows.cpu()                       # the one read-back of the numbers; the maps stay on the device until drawn


b = sess._buf
mean, std = METRICS["temp_mean"], METRICS["temp_std"]


def eager_once():
    """The page's loop on the device: pack once, each model, then un-normalise, subtract, and the ranges of the whole tile and
    the four quadrants per model and channel, each number read back as the page's np.min / np.max calls would."""
    with torch.no_grad():
        x = mau_amd.data.pack_tiles(b["cls_a"], b["cls_b"], b["cont"], None, torch.float16)
        outs = [m(x, b["ts"], b["md8"] if n == 8 else b["md4"])[0] for (_, m), n in zip(models, sess._n_meta)]
        tgt = b["target"].clone()
        tgt[1] = tgt[1] * std + mean
        numbers = []
        for o in outs:
            p = o.clone()
            p[1] = p[1] * std + mean
            e = p - tgt
            for c in range(2):
                for y1, y2, x1, x2 in ((0, H, 0, W),) + C.quadrants(H, W):
                    gq, pq, eq = tgt[c, y1:y2, x1:x2], p[c, y1:y2, x1:x2], e[c, y1:y2, x1:x2]
                    numbers.append((float(torch.minimum(gq.min(), pq.min())), float(torch.maximum(gq.max(), pq.max())), float(eq.abs().max())))
        return numbers


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for _ in range(5):
    session_once(), eager_once()
N = 40
rows = {"session_ms": [], "eager_ms": []}
for _ in range(5):
    rows["session_ms"].append(window(session_once, N))
    rows["eager_ms"].append(window(eager_once, N))
# library calls of the chain (one launch each but for a few two-launch entry points), counted on the eager spelling of the chain
from mau_amd import _lib  # noqa: E402
calls = []
real_check = _lib.check
_lib.check = lambda status, what="": (calls.append(what), real_check(status, what))[1]
with torch.no_grad():
    sess._run()
chain_calls = len(calls)
calls.clear()
eager_once()
eager_calls = len(calls)
_lib.check = real_check
res = {"shape": [3, H, W], "precision": "fp16", **{k: [round(v, 4) for v in vs] for k, vs in rows.items()},
       "session_ms_median": round(float(np.median(rows["session_ms"])), 4), "eager_ms_median": round(float(np.median(rows["eager_ms"])), 4),
       "eager_readbacks": 3 * 2 * 5 * 3, "session_readbacks": 1,
       "session_library_calls": chain_calls, "session_copy_nodes": 3, "eager_library_calls": eager_calls,
       # torch operators of eager_once, counted from its text: 4 for the target, per model 5 and 8 per (channel, region)
       "eager_torch_ops": 4 + 3 * (5 + 2 * 5 * 8)}
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f)
