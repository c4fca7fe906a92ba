#!/usr/bin/env python3
"""Time the SSIM gradient, in one process:

  kernel   mau_ssim_loss_grad at (32, 2, 256, 256) and at (8, 2, 512, 512) (pooled by f = 2), fp32, preallocated buffers, raw entry
           point -- beside mau_ssim_loss (the value: two launches) on the same tensors, as a yardstick of the same kind;
  step     the captured training step (production U-Net, bf16, synthetic batches of the configured size) with
           compute_loss_l1_grad_ssim_trained against the step with compute_loss_l1_grad_ssim (the SSIM term detached).

The two sides of a comparison ALTERNATE (a, b, a, b, ...): a region is CALLS back-to-back calls between two device events; the figure is
the median region divided by CALLS, with min and max.

    timeout -k 10 300 python scripts/ssim_grad_bench.py [--json out.json]

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mau_amd  # noqa: E402
from mau_amd import functional as F_  # noqa: E402
from mau_amd._lib import call, lib  # noqa: E402

SHAPES = [(32, 2, 256, 256), (8, 2, 512, 512)]
REGIONS = 30


def region_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def summary(v, calls):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "regions": len(v), "calls_per_region": calls}


def alternate(fa, fb, calls):
    for _ in range(3):                                  # warm-up: code objects, clocks
        region_us(fa, calls)
        region_us(fb, calls)
    ta, tb = [], []
    for _ in range(REGIONS):                            # alternating regions: drift of the clock hits both alike
        ta.append(region_us(fa, calls))
        tb.append(region_us(fb, calls))
    torch.cuda.synchronize()
    return ta, tb


def kernels(B, C, H, W, calls=20):
    g = torch.Generator().manual_seed(1)
    o = torch.randn(B, C, H, W, generator=g).cuda()
    t = o + 0.3 * torch.randn(B, C, H, W, generator=g).cuda()
    st = F_._stream()
    d = torch.empty_like(o)
    ws = torch.empty(lib.mau_ssim_ws_elems(B, C, H, W), dtype=torch.float64, device=o.device)
    per_image, loss = torch.empty(B, device=o.device), torch.empty(1, device=o.device)

    def grad():
        call("mau_ssim_loss_grad", o.data_ptr(), t.data_ptr(), d.data_ptr(), 1.0, 1, B, C, H, W, st)

    def value():
        call("mau_ssim_loss", o.data_ptr(), t.data_ptr(), ws.data_ptr(), per_image.data_ptr(), loss.data_ptr(), 1, B, C, H, W, st)

    tg, tv = alternate(grad, value, calls)
    mb = 3 * o.numel() * 4 / 1e6                        # out and tgt read, dout written, once each
    return {"shape": [B, C, H, W], "ssim_loss_grad": summary(tg, calls), "ssim_loss_value": summary(tv, calls),
            "grad_over_value": statistics.median(tg) / statistics.median(tv), "operand_MB": mb,
            "grad_GBps_of_operand": mb / 1e3 / (statistics.median(tg) * 1e-6)}


def train_step(calls=5):
    from mau_amd import train
    from mau_amd.config import CONFIG
    cfg, ds = CONFIG.training, CONFIG.dataset
    gen = torch.Generator().manual_seed(3)
    x, md, ts, _l, t1, t2, tgt = train.synthetic_batch(cfg.batch_size, "cuda", gen)
    mdf = torch.cat([md, t1, t2], dim=1) if ds.nb_metadata_features >= 8 else md
    steps = {}
    for name, crit in (("trained", mau_amd.compute_loss_l1_grad_ssim_trained), ("detached", mau_amd.compute_loss_l1_grad_ssim)):
        torch.manual_seed(0)
        net = mau_amd.UrbanPredictor(model_type="unet", spatial_channels=ds.nb_input_channels, seq_len=ds.temporal_length,
                                     temporal_dim=cfg.temporal_dim, meta_features=ds.nb_metadata_features, meta_dim=cfg.meta_dim,
                                     lstm_dim=cfg.lstm_hidden, out_channels=2, temporal_embeddings=False,
                                     metadata_embeddings=True).cuda().set_precision("bf16").train()
        opt = mau_amd.AdamW(net.parameters(), lr=1e-4, weight_decay=cfg.weight_decay)
        gs = mau_amd.GraphedTrainStep(net, opt, crit, warmup=2)
        for _ in range(4):
            gs(x, ts, mdf, tgt)
        assert gs.graph is not None
        steps[name] = gs
    ta, tb = alternate(lambda: steps["trained"](x, ts, mdf, tgt), lambda: steps["detached"](x, ts, mdf, tgt), calls)
    return {"batch": [int(v) for v in tgt.shape], "trained": summary(ta, calls), "detached": summary(tb, calls),
            "trained_over_detached": statistics.median(ta) / statistics.median(tb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"kernels": [kernels(*s) for s in SHAPES], "train_step": train_step()}
    line = json.dumps(out)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
