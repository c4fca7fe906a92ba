#!/usr/bin/env python3
"""The first layer's dz route (conv0_0.conv1, 6 -> 64, bf16): mau_bn_relu_bwd_apply + mau_conv3x3_first_wgrad against
mau_conv3x3_first_wgrad_bn, through the C ABI, one HIP-event pair per call, the two routes alternated in ONE process, median of REPS
calls per point.  The smallest size from which the fused route is never slower is functional._FIRST_DZ_FUSED_MIN_WORK.
    python scripts/first_dz_fused_bench.py [output file]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mau_amd  # noqa: F401
from mau_amd._lib import MAU_BF16, call, lib

REPS, Cin, Cout = 30, 6, 64
POINTS = [(2, 64), (8, 128), (8, 256), (32, 256)]             # (N, H = W)
st = torch.cuda.current_stream().cuda_stream
lines = [f"{'N x H x W':>14s} {'pixels':>9s} {'apply + wgrad us':>17s} {'fused us':>9s} {'fused / two':>12s} {'fused TB/s':>11s}"]
for N, S in POINTS:
    npix = N * S * S
    da = (torch.randn(npix, Cout, device="cuda") * 0.5).bfloat16()
    z = (torch.randn(npix, Cout, device="cuda") * 1.5).bfloat16()
    dz = torch.empty_like(da)
    x8 = torch.zeros(N, S, S, 8, device="cuda", dtype=torch.bfloat16)
    x8[..., :Cin] = torch.randn(N, S, S, Cin, device="cuda").bfloat16()
    coefs = [0.5 + torch.rand(Cout, device="cuda"), torch.randn(Cout, device="cuda") * 0.5, torch.randn(Cout, device="cuda") * 0.3,
             0.5 + torch.rand(Cout, device="cuda")]              # scale, shift, mean, invstd
    k = [t.data_ptr() for t in coefs]
    slab = torch.empty(lib.mau_bn_bwd_rows(npix), 2, Cout, device="cuda")
    call("mau_bn_relu_bwd_reduce", da.data_ptr(), Cout, z.data_ptr(), Cout, *k, slab.data_ptr(), Cout, MAU_BF16, npix, Cout, st)
    sums = torch.cat([slab.double().sum(0).reshape(-1), torch.tensor([float(npix)], dtype=torch.float64, device="cuda")])
    ws = torch.empty(lib.mau_conv3x3_first_wgrad_ws_elems(N, S, S, Cout), device="cuda")
    dw = [torch.empty(Cout, Cin, 3, 3, device="cuda") for _ in range(2)]

    def two():
        call("mau_bn_relu_bwd_apply", da.data_ptr(), Cout, z.data_ptr(), Cout, *k, sums.data_ptr(), float(npix), dz.data_ptr(), Cout, MAU_BF16, npix, Cout, st)
        call("mau_conv3x3_first_wgrad", x8.data_ptr(), dz.data_ptr(), Cout, dw[0].data_ptr(), ws.data_ptr(), Cin, Cout, MAU_BF16, N, S, S, st)

    def one():
        call("mau_conv3x3_first_wgrad_bn", x8.data_ptr(), da.data_ptr(), Cout, z.data_ptr(), Cout, *k, sums.data_ptr(), float(npix), dw[1].data_ptr(),
             ws.data_ptr(), Cin, Cout, MAU_BF16, N, S, S, st)

    times = {two: [], one: []}
    for rep in range(REPS + 3):
        for f in (two, one):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if rep >= 3:                                          # (three warm-up rounds)
                times[f].append(e0.elapsed_time(e1) * 1e3)
    assert torch.equal(dw[0].view(torch.int32), dw[1].view(torch.int32)), "the routes differ in bits"
    t2, t1 = statistics.median(times[two]), statistics.median(times[one])
    mb = npix * (2 * Cout * 2 + 16) / 1e6                        # da + z + x8
    lines.append(f"{N:4d} x {S:3d} x {S:3d} {npix:9d} {t2:17.1f} {t1:9.1f} {t1 / t2:12.3f} {mb / t1:11.2f}")
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
