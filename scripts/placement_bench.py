"""What the two launches of a placement sweep cost (EXPERIMENTS.md, "Placement sweeps"): ``PlacementSession`` replay against
``GraphedInference`` replay and against the network alone on an already packed input, at the app's shape (512 x 512, 23 channels,
fp16, batch 8, base-64 U-Net), and ``mau_placement_pack`` / ``mau_placement_result`` alone -- all in one process, alternating, device
events around back-to-back calls.  Prints one JSON line; ``python scripts/placement_bench.py [OUT.json]`` also writes it."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mau_amd  # noqa: E402
from mau_amd import placement as P  # noqa: E402
from mau_amd._capture import warm_up_and_capture  # noqa: E402

METRICS = {"rgb_mean": [0.4312, 0.5127, 0.3989], "rgb_std": [0.2213, 0.1907, 0.2571], "temp_mean": 29.4173, "temp_std": 11.0291}
S, B, NCLS, REPS, ROUNDS = 512, 8, 9, 40, 4


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us per call


def main():
    torch.manual_seed(0)
    net = mau_amd.UrbanPredictor("unet", 23, 10, 64, 4, 64, 96, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    net = net.cuda().set_precision("fp16").eval()
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    dw = dev(rng.integers(0, NCLS, (S, S)).astype(np.uint8))
    rgb = dev(rng.uniform(0, 255, (3, S, S)).astype(np.float32))
    ndvi = dev(rng.uniform(-1, 1, (S, S)).astype(np.float32))
    temp = dev(rng.uniform(5, 55, (S, S)).astype(np.float32))
    roi = dev((rng.random((S, S)) < 0.3).astype(np.uint8))
    g = torch.Generator().manual_seed(1)
    ts, md = torch.randn(1, 10, generator=g).cuda(), torch.randn(1, 4, generator=g).cuda()
    sess = mau_amd.PlacementSession(net, dw, rgb, ndvi, temp, md, ts, metrics=METRICS, ncls=NCLS, patch=32, batch=B, roi=roi)
    edits = P.edits_table(P.stamp_grid(S, 32, 16)[:2], P.stamp_grid(S, 32, 16)[:4], [1])
    sess._edits.copy_(dev(edits))
    x = torch.randn(B, 23, S, S, generator=g).cuda()
    gi = mau_amd.GraphedInference(net, x, ts.expand(B, -1).contiguous(), md.expand(B, -1).contiguous(), clone_output=False)
    # the network alone on an already packed input (no layout pass of a dense tensor): the cleanest difference
    act = P.pack(dw, None, rgb, ndvi, temp, dev(edits), 32, NCLS, METRICS, torch.float16)
    tsb, mdb = ts.expand(B, -1).contiguous(), md.expand(B, -1).contiguous()
    gnet, _ = warm_up_and_capture(lambda: net(act, tsb, mdb), dw.device, 2)
    out = sess.output
    norm = torch.from_numpy(np.array(METRICS["rgb_mean"] + METRICS["rgb_std"] + [METRICS["temp_mean"], METRICS["temp_std"]])).cuda()
    e_dev = dev(edits)

    def pack_only():
        P._pack(dw, None, rgb, ndvi, temp, e_dev, norm, 32, 32, NCLS, torch.float16, 24)

    def result_only():
        P._result(out, sess.base, e_dev, roi, METRICS["temp_mean"], METRICS["temp_std"], 32, 32, sess._tickets)

    runs = {"placement_session_replay": sess._replay, "graphed_inference_replay": gi.graph.replay, "network_on_packed_input_replay": gnet.replay,
            "placement_pack_alone": pack_only, "placement_result_alone": result_only}
    for fn in runs.values():                                          # warm every shape
        timed(fn, 5)
    res = {k: [] for k in runs}
    for _ in range(ROUNDS):                                            # alternate the variants within one call
        for k, fn in runs.items():
            res[k].append(round(timed(fn, REPS), 2))
    pack_bytes = B * S * S * 24 * 2
    result_bytes = B * 2 * S * S * 4 + 2 * S * S * 4 + S * S
    med = {k: float(np.median(v)) for k, v in res.items()}
    summary = {"shape": f"{S}x{S}x23 fp16 U-Net base_filters=64, batch {B}, patch 32", "reps_per_round": REPS, "us_per_call_rounds": res,
               "us_per_call_median": med, "pack_bytes_written": pack_bytes, "result_bytes_read": result_bytes,
               "pack_alone_TBps": round(pack_bytes / med["placement_pack_alone"] / 1e6, 3),
               "result_alone_TBps": round(result_bytes / med["placement_result_alone"] / 1e6, 3),
               "session_minus_graphed_inference_us": round(med["placement_session_replay"] - med["graphed_inference_replay"], 2),
               "session_minus_network_on_packed_us": round(med["placement_session_replay"] - med["network_on_packed_input_replay"], 2)}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
