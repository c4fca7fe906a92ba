#!/usr/bin/env python3
"""Time the loss terms of one validation batch two ways, in the same process, at (16, 2, 250, 250) and (32, 2, 256, 256) fp32:

  new    mau_loss_terms: every term of compute_all_loss in ONE launch (preallocated buffers, raw entry point);
  old    the three existing entry points back to back: mau_mse_fwd_bwd and mau_l1_gradient_loss without dout, mau_ssim_loss
         (two launches each: six launches over the same two tensors).

The two regions ALTERNATE (new, old, new, old, ...): a region is CALLS back-to-back calls between two device events; the figure
is the median region divided by CALLS, with min and max.  Also: one validation pass over a synthetic 64-tile val/ (the U-Net at the
production configuration, batches of 16) with the sums on the device (one read-back per pass, ``train.validate``) against the same pass
with one ``.item()`` per batch.

    timeout -k 10 300 python scripts/loss_terms_bench.py [--json out.json]

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mau_amd  # noqa: E402
from mau_amd import functional as F_  # noqa: E402
from mau_amd import losses as L  # noqa: E402
from mau_amd._lib import call, lib  # noqa: E402

SHAPES = [(16, 2, 250, 250), (32, 2, 256, 256)]
REGIONS, CALLS = 30, 20


def clock_mhz():
    """Best effort, read-only: the current shader clock as torch reports it."""
    try:
        return torch.cuda.clock_rate()
    except Exception:
        return None


def region_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "regions": len(v), "calls_per_region": CALLS}


def kernels(B, C, H, W):
    g = torch.Generator().manual_seed(1)
    o = torch.randn(B, C, H, W, generator=g).cuda()
    t = (o + 0.3 * torch.randn(B, C, H, W, generator=g).cuda())
    dev, n, st = o.device, o.numel(), F_._stream()
    f64 = lambda k: torch.empty(max(1, k), dtype=torch.float64, device=dev)
    f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)
    ws_new, terms, per_image, acc = f64(lib.mau_loss_terms_ws_elems(B, C, H, W)), f32(8), f32(B), torch.zeros(8, dtype=torch.float64, device=dev)
    tickets = torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device=dev)
    p_mse, p_l1, ws_ssim = f64(lib.mau_mse_blocks(n)), f64(3 * lib.mau_l1_gradient_blocks(n)), f64(lib.mau_ssim_ws_elems(B, C, H, W))
    l_mse, t_l1, pi_old, l_ssim = f32(1), f32(3), f32(B), f32(1)

    def new():
        call("mau_loss_terms", o.data_ptr(), t.data_ptr(), ws_new.data_ptr(), tickets.data_ptr(), terms.data_ptr(), per_image.data_ptr(),
             acc.data_ptr(), 0.1, 0.5, B, C, H, W, st)

    def old():
        call("mau_mse_fwd_bwd", o.data_ptr(), t.data_ptr(), p_mse.data_ptr(), l_mse.data_ptr(), None, n, st)
        call("mau_l1_gradient_loss", o.data_ptr(), t.data_ptr(), p_l1.data_ptr(), t_l1.data_ptr(), None, 1.0, 0.1, B, C, H, W, st)
        call("mau_ssim_loss", o.data_ptr(), t.data_ptr(), ws_ssim.data_ptr(), pi_old.data_ptr(), l_ssim.data_ptr(), 1, B, C, H, W, st)

    for _ in range(3):                                  # warm-up: code objects, clocks
        region_us(new)
        region_us(old)
    tn, to = [], []
    for _ in range(REGIONS):                            # alternating regions: drift of the clock hits both alike
        tn.append(region_us(new))
        to.append(region_us(old))
    torch.cuda.synchronize()
    agree = {"mse": (float(terms[0]), float(l_mse)), "pixel": (float(terms[1]), float(t_l1[0])), "ssim": (float(terms[5]), float(l_ssim))}
    return {"shape": [B, C, H, W], "new_one_launch": summary(tn), "old_three_entry_points": summary(to),
            "old_over_new": statistics.median(to) / statistics.median(tn), "values_new_old": agree}


def validation_pass(tiles=64, bs=16):
    """64 synthetic val tiles through the production U-Net in eval mode: ``train.validate`` (sums on the device, one read-back) against
    the same loop reading the batch total back with .item() -- host clock around the pass, stream synchronised at both ends."""
    from mau_amd import train
    from mau_amd.config import CONFIG
    torch.manual_seed(0)
    cfg, ds = CONFIG.training, CONFIG.dataset
    net = mau_amd.UrbanPredictor(model_type="unet", spatial_channels=ds.nb_input_channels, seq_len=ds.temporal_length, temporal_dim=cfg.temporal_dim,
                                 meta_features=ds.nb_metadata_features, meta_dim=cfg.meta_dim, lstm_dim=cfg.lstm_hidden, out_channels=2,
                                 temporal_embeddings=False, metadata_embeddings=True).cuda().set_precision("bf16")
    gen = torch.Generator().manual_seed(3)
    loader = [train.synthetic_batch(bs, "cuda", gen) for _ in range(tiles // bs)]

    def per_batch_readback():
        net.eval()
        total, num = 0.0, 0
        with torch.no_grad():
            for x, md, ts, _l, t1, t2, tgt in loader:
                out = net(x, ts, torch.cat([md, t1, t2], dim=1))
                total += L.compute_all_loss(out, tgt)["total"].item() * len(tgt)
                num += len(tgt)
        return total / num

    def on_device():
        return train.validate(net, loader, mau_amd.compute_loss_l1_grad_ssim)[0]

    res = {}
    for name, fn in (("one_readback_per_pass", on_device), ("one_readback_per_batch", per_batch_readback)):
        fn()
        v = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "passes": len(v), "value": val}
    res["tiles"], res["batch"] = tiles, bs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"clock_mhz_before": clock_mhz(), "kernels": [kernels(*s) for s in SHAPES], "validation_pass": validation_pass(),
           "clock_mhz_after": clock_mhz()}
    line = json.dumps(out)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
