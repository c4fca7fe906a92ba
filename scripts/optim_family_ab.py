"""A/B of the optimizer family on the flagship workload (U-Net bf16, B = 32, 6 x 256 x 256, MSE, GraphedTrainStep), one process, the two
routes resident side by side and timed alternately:

    A = torch's optimizer (the captured step starts with the multi-tensor re-pack) / torch.nn.utils.clip_grad_norm_
    B = mau_amd.SGD / mau_amd.Adam (update + re-pack in one launch) / max_grad_norm inside the fused update

for (i) SGD(momentum 0.9), (ii) Adam, (iii) AdamW with clipping at a bound that clips (a third of the first measured norm).
Every round times one region of ``--steps`` replays of A, then one of B; the figure of a route is the median of its regions, the
A/A spread the (max - min) of A's regions in the same call.  One JSON line on stdout (and in ``--out``) with the library's sha256.

    python scripts/optim_family_ab.py --rounds 6 --steps 10 --out profiles/r7/optim_family_ab.json
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

import torch  # noqa: E402

import mau_amd  # noqa: E402
from mau_amd import _lib  # noqa: E402


def make(args, route, which, clip):
    torch.manual_seed(0)
    net = mau_amd.UrbanPredictor("unet", 6, 10, 64, 4, 64, 96, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    net = net.cuda().set_precision("bf16").train()
    ps = net.parameters()
    if which == "sgd":
        opt = torch.optim.SGD(ps, lr=1e-4, momentum=0.9) if route == "A" else mau_amd.SGD(ps, lr=1e-4, momentum=0.9)
    elif which == "adam":
        opt = torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-3) if route == "A" else mau_amd.Adam(ps, lr=1e-4, weight_decay=1e-3)
    else:
        opt = mau_amd.AdamW(ps, lr=1e-4, weight_decay=1e-3)
    crit = lambda o, t: mau_amd.compute_loss_mse(o, t)          # noqa: E731
    step = mau_amd.GraphedTrainStep(net, opt, crit, warmup=3, copy_inputs=False, clip_grad_norm=clip if route == "B" else 0.0)
    if route == "A" and clip > 0:
        step.clip = clip                                         # the route of a torch optimizer: clip_grad_norm_ between backward and step
    return step


def region(step, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(1234)
    B, S = args.batch, args.size
    batch = (torch.randn(B, 6, S, S, generator=g).cuda(), torch.randn(B, 10, generator=g).cuda(), torch.randn(B, 4, generator=g).cuda(),
             torch.randn(B, 2, S, S, generator=g).cuda())
    # a bound that clips: a third of the gradient norm of the first step
    probe = mau_amd.UrbanPredictor("unet", 6, 10, 64, 4, 64, 96, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    torch.manual_seed(0)
    probe = probe.cuda().set_precision("bf16").train()
    mau_amd.compute_loss_mse(probe(*batch[:3]), batch[3])["total"].backward()
    norm0 = float(torch.nn.utils.clip_grad_norm_(probe.parameters(), 1e30))
    del probe
    torch.cuda.empty_cache()
    rec = {"workload": f"unet_bf16_b{B}_s{S}_c6_train", "rounds": args.rounds, "steps_per_region": args.steps, "first_grad_norm": norm0,
           "lib_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "device": torch.cuda.get_device_name(0), "configs": {}}
    for which in ("sgd", "adam", "adamw_clip"):
        clip = norm0 / 3 if which == "adamw_clip" else 0.0
        steps = {r: make(args, r, which, clip) for r in ("A", "B")}
        for r in ("A", "B"):
            for _ in range(3 + 1 + 3):                           # eager warm-ups, the capture, replays
                steps[r](*batch)
        ms = {"A": [], "B": []}
        for _ in range(args.rounds):
            for r in ("A", "B"):
                ms[r].append(region(steps[r], batch, args.steps))
        loss = {r: float(steps[r].loss) for r in ms}
        a, b = statistics.median(ms["A"]), statistics.median(ms["B"])
        out = {"A_ms": a, "B_ms": b, "B_minus_A_ms": b - a, "A_regions_ms": ms["A"], "B_regions_ms": ms["B"],
               "A_spread_ms": max(ms["A"]) - min(ms["A"]), "B_spread_ms": max(ms["B"]) - min(ms["B"]), "last_loss": loss}
        if clip > 0:
            out["clip"] = clip
            out["last_grad_norm_B"] = float(steps["B"].optimizer.last_grad_norm)
        rec["configs"][which] = out
        print(f"{which}: A {a:.3f} ms  B {b:.3f} ms  (B - A {b - a:+.3f} ms; A spread {out['A_spread_ms']:.3f} ms)", file=sys.stderr, flush=True)
        del steps
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
