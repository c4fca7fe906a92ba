#!/usr/bin/env python3
"""Time the evaluation metrics of one batch, (16, 2, 250, 250) fp32, two ways:

  kernel   mau_eval_metrics on device-resident maps (device events; windows of CALLS back-to-back launches, the median window
           divided by CALLS), raw entry point with preallocated buffers and through ``mau_amd.evaluate.eval_metrics``
           (allocations and the small coefficient copies included), plus the read-back of the (16, 2, 38) fp64 rows;
  host     what the reference's loop does per batch: copy both maps to the host, rebuild the class map from the nine dense
           planes, then float32 numpy / scipy per sample and channel -- overall MAE / RMSE, two Laplacian variances, and a mask,
           an MAE pass and an RMSE pass per class (host clock around work that starts with a synchronising copy).

    timeout -k 10 300 python scripts/eval_metrics_bench.py [--json out.json]

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mau_amd  # noqa: E402
from mau_amd import functional as F_  # noqa: E402
from mau_amd._lib import call, lib  # noqa: E402

B, C, H, W, NCLS = 16, 2, 250, 250, 9
WINDOWS, CALLS, HOST_REPS = 30, 20, 20


def clock_state():
    """Best effort, read-only: the current shader clock as the driver reports it."""
    try:
        return {"sclk_mhz_torch": torch.cuda.clock_rate()}
    except Exception:
        pass
    import glob
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            cur = [ln.strip() for ln in open(f) if "*" in ln]
            if cur:
                return {"pp_dpm_sclk": cur[0]}
        except OSError:
            pass
    return {"clock": "not available"}


def host_metrics(outputs, targets, inputs, scale, shift):
    """The reference-style host path of one batch (test/evaluate.py:188-275 in this project's words), float32."""
    from scipy.ndimage import laplace
    o, t = outputs.cpu().numpy(), targets.cpu().numpy()
    res = []
    for i in range(o.shape[0]):
        planes = inputs[i, :NCLS].cpu().numpy()
        dw = np.argmax(np.stack([planes[c] * c for c in range(NCLS)]), axis=0)
        for ch in range(o.shape[1]):
            pred, gt = o[i, ch] * scale[ch] + shift[ch], t[i, ch] * scale[ch] + shift[ch]
            row = [np.mean(np.abs(pred - gt)), np.sqrt(np.mean((pred - gt) ** 2)), np.var(laplace(pred)), np.var(laplace(gt))]
            for k in range(NCLS):
                mask = dw == k
                if np.any(mask):
                    row += [np.mean(np.abs(pred[mask] - gt[mask])), np.sqrt(np.mean((pred[mask] - gt[mask]) ** 2))]
            res.append(row)
    return res


def device_ms(fn):
    for _ in range(3 * CALLS):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / CALLS)
    return {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    g = torch.Generator().manual_seed(0)
    out = torch.randn(B, C, H, W, generator=g).cuda()
    tgt = torch.randn(B, C, H, W, generator=g).cuda()
    cls = torch.randint(0, NCLS, (B, H, W), generator=g).to(torch.uint8).cuda()
    dense = torch.nn.functional.one_hot(cls.long(), NCLS).permute(0, 3, 1, 2).float().contiguous()     # the nine planes the reference reads
    scale, shift = [1.0, 7.3], [0.0, 21.5]
    sc, sh = torch.tensor(scale, dtype=torch.float64).cuda(), torch.tensor(shift, dtype=torch.float64).cuda()
    rows = torch.empty((B, C, lib.mau_eval_metrics_row_elems(NCLS)), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.mau_eval_metrics_ws_elems(B, C, H, W, NCLS), dtype=torch.float64, device="cuda")
    tk = F_._tickets(out.device)

    def raw():
        call("mau_eval_metrics", out.data_ptr(), tgt.data_ptr(), cls.data_ptr(), sc.data_ptr(), sh.data_ptr(), rows.data_ptr(),
             ws.data_ptr(), tk.data_ptr(), B, C, H, W, NCLS, F_._stream())

    res = {"shape": [B, C, H, W], "windows": WINDOWS, "calls_per_window": CALLS, "clock_before": clock_state(),
           "workgroups": lib.mau_eval_metrics_chunks(H, W) * B * C}
    res["kernel_raw"] = device_ms(raw)
    res["kernel_wrapper"] = device_ms(lambda: mau_amd.evaluate.eval_metrics(out, tgt, cls, scale, shift, NCLS))
    res["kernel_wrapper_and_readback"] = device_ms(lambda: mau_amd.evaluate.eval_metrics(out, tgt, cls, scale, shift, NCLS).rows.cpu())
    # bytes the algorithm needs: both maps once + the class map once per channel
    res["bytes_needed"] = B * C * H * W * 9
    res["kernel_raw_gb_per_s_of_needed_bytes"] = res["bytes_needed"] / (res["kernel_raw"]["median_ms"] * 1e-3) / 1e9
    host_metrics(out, tgt, dense, scale, shift)
    ts = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = host_metrics(out, tgt, dense, scale, shift)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["host_reference_style"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": HOST_REPS}
    res["clock_after"] = clock_state()
    # the two paths compute the same quantities (float32 host against fp64 device): worst relative difference of the overall entries
    dev = mau_amd.evaluate.eval_metrics(out, tgt, cls, scale, shift, NCLS).rows.cpu().numpy().reshape(B * C, -1)
    res["max_rel_diff_overall_host_f32_vs_device"] = float(max(abs(h[j] - d[j]) / abs(d[j]) for h, d in zip(host, dev) for j in range(4)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
