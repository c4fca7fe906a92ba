"""What placement screening costs and how well it ranks (EXPERIMENTS.md, "Placement screening"), at the app's shape: 512 x 512, 23
channels, base-64 networks with random weights, a 32 x 32 stamp at stride 16, two classes (1922 candidates), the objective
"temperature over the tile" and "temperature over a roi".  Per model type and precision, in one process:

* the time of building one ``ScreeningSession`` (seed, pack, one forward, one data-gradient-only backward), wall clock, synchronised;
* the time of one ``__call__`` on the whole grid (one launch, one read-back), wall clock, and of the launch alone by device events;
* non-finite gradient values (entry 3) at ``seed_scale`` 1, and at 2^8 and 2^-8 where a scale is needed;
* the exact ``PlacementSession`` sweep of the same grid (batch 8, the captured graph), wall clock, and the Spearman rank correlation
  of the predicted change with the exact ``mean_dt`` / ``mean_dt_roi`` over the full grid.

The weights are random: the agreement says little about a trained network.  Prints one JSON line; ``python
scripts/screening_bench.py [OUT.json] [unet|unet++ ...]`` also writes it."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mau_amd  # noqa: E402
from mau_amd import screening as SC  # noqa: E402

METRICS = {"rgb_mean": [0.4312, 0.5127, 0.3989], "rgb_std": [0.2213, 0.1907, 0.2571], "temp_mean": 29.4173, "temp_std": 11.0291}
S, NCLS, PATCH, STRIDE, CLASSES, BATCH = 512, 9, 32, 16, [1, 6], 8
FLAGS = {"unet": dict(temporal_embeddings=False, metadata_embeddings=True), "unet++": {}}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3       # ms


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".json") else None
    types = [a for a in sys.argv[1:] if a in FLAGS] or ["unet", "unet++"]
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    dw = dev(rng.integers(0, NCLS, (S, S)).astype(np.uint8))
    rgb = dev(rng.uniform(0, 255, (3, S, S)).astype(np.float32))
    ndvi = dev(rng.uniform(-1, 1, (S, S)).astype(np.float32))
    temp = dev(rng.uniform(5, 55, (S, S)).astype(np.float32))
    roi = torch.zeros((S, S), dtype=torch.uint8, device="cuda")
    roi[128:320, 192:448] = 1
    g = torch.Generator().manual_seed(1)
    ts, md = torch.randn(1, 10, generator=g).cuda(), torch.randn(1, 4, generator=g).cuda()
    summary = {"shape": f"{S}x{S}x23, base_filters=64, random weights, patch {PATCH}, stride {STRIDE}, classes {CLASSES}", "runs": {}}
    for mt in types:
        torch.manual_seed(0)
        net = mau_amd.UrbanPredictor(mt, 23, 10, 64, 4, 64, 96, 2, base_filters=64, **FLAGS[mt]).cuda().eval()
        for prec in ("fp16", "bf16"):
            net.set_precision(prec)
            kw = dict(metrics=METRICS, ncls=NCLS, patch=PATCH, objectives=(("temp", None), ("temp", roi)))
            mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, **kw)                        # warm: packs, allocator, kernel attributes
            sess, build_ms = wall(lambda: mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, **kw))
            sess(CLASSES, stride=STRIDE)
            r, call_ms = wall(lambda: sess(CLASSES, stride=STRIDE))
            e = dev(r.edits)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                SC._rows(sess.gradient, sess.gradient.stride(2), sess._dw_t2, e, sess.counts, sess._objs, sess._std, 1.0, sess.patch, NCLS)
            b.record()
            torch.cuda.synchronize()
            run = {"candidates": int(r.edits.shape[0]), "session_build_ms": round(build_ms, 3), "call_ms": round(call_ms, 3),
                   "rows_launch_us": round(a.elapsed_time(b) / 20 * 1e3, 2), "non_finite_scale_1": int(r.rows[..., 3].sum()),
                   "gradient_absmax": float(sess.gradient.float().abs().max()),
                   "gradient_absmin_nonzero": float(sess.gradient.float().abs()[sess.gradient != 0].min())}
            for scale in (2.0 ** 8, 2.0 ** -8):
                rs = mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, seed_scale=scale, **kw)(CLASSES, stride=STRIDE)
                run[f"non_finite_scale_{scale:g}"] = int(rs.rows[..., 3].sum())
                run[f"spearman_scale_{scale:g}_vs_scale_1"] = SC.spearman(rs.rows[0, :, 2], r.rows[0, :, 2])
            place = mau_amd.PlacementSession(net, dw, rgb, ndvi, temp, md, ts, metrics=METRICS, ncls=NCLS, patch=PATCH, batch=BATCH, roi=roi)
            place(CLASSES, stride=PATCH * 4)
            exact, sweep_ms = wall(lambda: place(CLASSES, stride=STRIDE))
            run.update({"exact_sweep_ms": round(sweep_ms, 3), "exact_over_call": round(sweep_ms / call_ms, 1),
                        "spearman_tile": SC.spearman(r.rows[0, :, 2], exact.rows[:, 1]), "spearman_roi": SC.spearman(r.rows[1, :, 2], exact.rows[:, 7])})
            for n in (8, 32):                                              # how many of the exact best n per class the screening's top 4n holds
                hits = [len(set(r.top_index(4 * n, 0, c).tolist()) & set(np.flatnonzero(exact.edits[:, 2] == c)[np.argsort(exact.rows[exact.edits[:, 2] == c, 1], kind="stable")[:n]].tolist()))
                        for c in CLASSES]
                run[f"exact_best_{n}_in_screened_top_{4 * n}"] = hits
            summary["runs"][f"{mt}_{prec}"] = run
            del sess, place
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
