#!/usr/bin/env python3
"""Time one scenario edit of the app's tile, 512 x 512, base-64 U-Net, 23 input channels, N = 1, fp16 and bf16, two ways:

  session    ``ScenarioSession``: the (512, 512, 4) canvas to the device, one hipGraph replay (pack -> network -> result), the
             (1, 5) fp64 statistics back.  Device events around windows of CALLS back-to-back edits (the median window divided
             by CALLS), and a host clock around single edits (each ends in the synchronising read-back);
  reference  what the app does per click with the model on the device: ``prepare_input_host`` (resize, palette match, float64
             normalisation, one-hot stacks), the dense (1, 23, 512, 512) fp32 tensor to the device, ``GraphedInference``, the
             output back, numpy un-normalisation, difference and mean.  Host clock (the path starts and ends on the host).

and the two kernels alone (raw entry points, preallocated buffers), the replay alone and the plain forward's replay alone.

    timeout -k 10 600 python scripts/scenario_bench.py [--json out.json]

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
from mau_amd import scenario as S  # noqa: E402
from mau_amd._lib import call, lib  # noqa: E402

H = W = HC = WC = 512
WINDOWS, CALLS, HOST_REPS = 20, 10, 10
METRICS = {"rgb_mean": [0.5045, 0.4785, 0.4885], "rgb_std": [0.2355, 0.1755, 0.1391], "temp_mean": 32.1837, "temp_std": 13.3625}


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


def device_ms(fn, calls=CALLS, windows=WINDOWS):
    for _ in range(2 * calls):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / calls)
    return {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call)}


def host_ms(fn, reps=HOST_REPS):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def painted_canvas(rng, palette):
    """A canvas as the app delivers it: transparent, with a few painted rectangles of palette colours."""
    c = np.zeros((HC, WC, 4), dtype=np.uint8)
    for _ in range(6):
        y, x = rng.integers(0, HC - 120), rng.integers(0, WC - 120)
        c[y:y + rng.integers(30, 120), x:x + rng.integers(30, 120)] = list(palette[rng.integers(0, len(palette))]) + [255]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "dw_palette.json")) as f:
        palette = S.palette_from_hex(json.load(f))
    rng = np.random.default_rng(0)
    dw = rng.integers(0, 9, (H, W)).astype(np.uint8)
    rgb = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    ndvi = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    temp = rng.uniform(5, 55, (H, W)).astype(np.float32)
    canvases = [painted_canvas(rng, palette) for _ in range(4)]
    g = torch.Generator().manual_seed(1)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    d_dw, d_rgb, d_ndvi, d_temp = (torch.from_numpy(v).cuda() for v in (dw, rgb, ndvi, temp))
    res = {"tile": [H, W], "canvas": [HC, WC], "scenarios": 1, "windows": WINDOWS, "calls_per_window": CALLS, "host_reps": HOST_REPS,
           "clock_before": clock_state(), "bytes_per_edit": {"session_h2d": HC * WC * 4, "session_d2h": 5 * 8,
                                                             "reference_h2d": 23 * H * W * 4, "reference_d2h": 2 * H * W * 4}}
    torch.manual_seed(2)
    net = mau_amd.UrbanPredictor("unet", 23, 12, 64, 8, 64, 96, 2, base_filters=64, temporal_embeddings=True, metadata_embeddings=True).cuda().eval()
    for prec, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        net.set_precision(prec)
        sess = mau_amd.ScenarioSession(net, d_dw, d_rgb, d_ndvi, d_temp, md, ts, palette=palette, metrics=METRICS, canvas_shape=(HC, WC),
                                       clone_output=False)
        k = [0]

        def edit():
            k[0] += 1
            return sess(canvases[k[0] % 4]).stats.cpu()

        r = {"session_edit_device_events": device_ms(edit), "session_edit_host_clock": host_ms(edit),
             "session_replay_only": device_ms(lambda: sess(sess.canvas))}
        # the two kernels alone
        tb = S._Tables((H, W), (HC, WC), palette, METRICS, d_dw.device)
        cv = torch.from_numpy(canvases[0][None]).cuda()
        out = torch.empty((1, H, W, 24), dtype=dtype, device="cuda")
        t2 = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        r["pack_kernel"] = device_ms(lambda: call("mau_scenario_pack", d_dw.data_ptr(), d_rgb.data_ptr(), d_ndvi.data_ptr(), d_temp.data_ptr(),
                                                  cv.data_ptr(), tb.yidx.data_ptr(), tb.xidx.data_ptr(), tb.palette.data_ptr(), tb.norm.data_ptr(),
                                                  out.data_ptr(), 24, t2.data_ptr(), F_.dtype_code(dtype), 1, H, W, HC, WC, 9, F_._stream()), calls=50)
        head = torch.randn(1, 2, H, W, device="cuda")
        o3 = [torch.empty((1, H, W), device="cuda") for _ in range(3)]
        rows = torch.empty((1, 5), dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.mau_scenario_result_ws_elems(1, H, W), dtype=torch.float64, device="cuda")
        tk = F_._tickets(head.device)
        r["result_kernel"] = device_ms(lambda: call("mau_scenario_result", head.data_ptr(), d_temp.data_ptr(), d_dw.data_ptr(), t2.data_ptr(),
                                                    METRICS["temp_mean"], METRICS["temp_std"], o3[0].data_ptr(), o3[1].data_ptr(), o3[2].data_ptr(),
                                                    rows.data_ptr(), ws.data_ptr(), tk.data_ptr(), 1, H, W, F_._stream()), calls=50)
        r["pack_bytes_needed"] = H * W * (1 + 5 * 4 + 4 + 24 * out.element_size() + 1)
        r["result_bytes_needed"] = H * W * (2 * 4 + 4 + 2 + 3 * 4)
        # the reference-style path around the same network
        gi = mau_amd.GraphedInference(net, torch.zeros(1, 23, H, W, device="cuda"), ts, md, clone_output=False)
        r["forward_replay_only"] = device_ms(lambda: gi(*gi.inputs))
        j = [0]
        host_parts = {}

        def reference_edit():
            j[0] += 1
            t0 = time.perf_counter()
            x = torch.from_numpy(S.prepare_input_host(dw, rgb, ndvi, temp, canvases[j[0] % 4], palette, METRICS))
            t1 = time.perf_counter()
            o = gi(x, ts, md).cpu().numpy()
            t2_ = time.perf_counter()
            change = o[0, 1] * METRICS["temp_std"] + METRICS["temp_mean"] - temp          # float32 numpy, as the app's arrays are
            m = float(change.mean()), float(change.min()), float(change.max())
            t3 = time.perf_counter()
            host_parts.setdefault("prepare_input_ms", []).append((t1 - t0) * 1e3)
            host_parts.setdefault("h2d_forward_d2h_ms", []).append((t2_ - t1) * 1e3)
            host_parts.setdefault("denormalise_delta_stats_ms", []).append((t3 - t2_) * 1e3)
            return m

        r["reference_edit_host_clock"] = host_ms(reference_edit)
        r["reference_edit_parts_median_ms"] = {k_: statistics.median(v[1:]) for k_, v in host_parts.items()}
        # the two paths agree: the session's mean against the reference path's float32 numpy mean of the same edit
        want = reference_edit()
        got = sess(canvases[j[0] % 4]).stats.cpu().numpy()[0]
        r["mean_delta_session_vs_reference"] = [float(got[0]), want[0]]
        res[prec] = r
    res["clock_after"] = clock_state()
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
