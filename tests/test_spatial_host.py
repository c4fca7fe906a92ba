"""CPU-only checks around csrc/spatial.hip: the plain references of tests/spatial_ref.py against the recorded fixtures and against
torch's own CPU operators (an oracle that is wrong proves nothing on the GPU), the host-side resize plan query
(``mau_resize_bilinear_plan``: which kernel and how many source rows per workgroup a shape reaches), and the launchers' refusals.
No kernel is launched here; tests/test_gpu_spatial.py runs the kernels against these references."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import spatial_ref as SR
from tests._helpers import load_npz


@pytest.fixture(scope="module")
def lib():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    return _lib


def _interp64(x, H, W):
    return TF.interpolate(torch.from_numpy(np.asarray(x)).double(), size=(H, W), mode="bilinear", align_corners=True)


def _interp64_bwd(dy, h, w):
    x = torch.zeros(dy.shape[0], dy.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    y = TF.interpolate(x, size=dy.shape[2:], mode="bilinear", align_corners=True)
    y.backward(torch.from_numpy(np.asarray(dy)).double())
    return x.grad.numpy()


def _table_bwd_slack(dy, h, w):
    """What the float32 TABLES (not the accumulation) may differ by from float64 coordinates in the adjoint: each weight is off by
    at most the forward bound's coordinate part, 2^-23 * 3 * in per axis, and a destination pixel reaches at most 2 x 2 sources."""
    H, W = dy.shape[2:]
    return 2.0 ** -23 * (3 * (h + w) + 8) * np.abs(dy).sum(axis=(2, 3), keepdims=True)


def test_resize_oracle_reproduces_the_fixtures_and_float64_interpolate():
    """resize_fwd_ref / resize_bwd_ref against every up_* / resize_* fixture of g2_spatial.npz (recorded from the reference in float32)
    and against float64 ``interpolate`` at every shape the GPU tests run; bounds of the issue's section 5, derived in spatial_ref."""
    d = load_npz("g2_spatial.npz")
    worst_f, worst_b, biteq, total = 0.0, 0.0, 0, 0
    for kind in ("up", "resize"):
        for tag in ("x2", "odd", "rect", "one"):
            if f"{kind}_{tag}/x" not in d:
                continue
            x, y, dy, dx = (d[f"{kind}_{tag}/{k}"] for k in ("x", "y", "dy", "dx"))
            h, w = x.shape[2:]
            H, W = y.shape[2:]
            steps = [(h, w, 2 * h, 2 * w), (2 * h, 2 * w, H, W)] if kind == "up" and (2 * h, 2 * w) != (H, W) else [(h, w, H, W)]
            got = x
            for (_, _, Hs, Ws) in steps:
                got = SR.resize_fwd_ref(got, Hs, Ws)
            bound = sum(SR.resize_fwd_bound(a, b, float(np.abs(x).max())) for a, b, _, _ in steps)
            err = np.abs(got.astype(np.float64) - y)
            worst_f = max(worst_f, float(err.max() / bound))
            assert err.max() <= bound, (kind, tag, err.max(), bound)
            biteq += int((got.view(np.int32) == y.view(np.int32)).sum())
            total += y.size
            # (the fixture's adjoint used the same float32 weights and accumulated in float32: the bound of section 5 per step; the
            #  first step's error passes through the second adjoint, whose weights are non-negative)
            g, lim = dy.astype(np.float64), np.zeros(dy.shape)
            for (hs, ws, Hs, Ws) in reversed(steps):
                ref, S, n, _, _ = SR.resize_bwd_ref(g, hs, ws)
                lim = SR.resize_bwd_ref(lim, hs, ws)[0] + (n + 1) * 2.0 ** -24 * S
                g = ref
            err = np.abs(g - dx)
            worst_b = max(worst_b, float((err / np.maximum(lim, 1e-300)).max()))
            assert (err <= lim).all(), (kind, tag, float(err.max()))
    print(f"fixtures: forward bit-equal {biteq} of {total} elements, worst |err|/bound {worst_f:.3f}; backward worst |err|/bound {worst_b:.3f}")
    assert worst_f <= 1.0 and worst_b <= 1.0
    rng = np.random.default_rng(11)
    worst_f = worst_b = 0.0
    for (N, Cc, h, w, H, W) in SR.ROWCOL_SHAPES + SR.CELL_SHAPES + SR.DEST_SHAPES + SR.BWD_EXTRA_SHAPES:
        x = rng.standard_normal((N, Cc, h, w)).astype(np.float32)
        got = SR.resize_fwd_ref(x, H, W).astype(np.float64)
        err = np.abs(got - _interp64(x, H, W).numpy()).max()
        bound = SR.resize_fwd_bound(h, w, float(np.abs(x).max()))
        worst_f = max(worst_f, float(err / bound))
        assert err <= bound, ((N, Cc, h, w, H, W), err, bound)
        dy = rng.standard_normal((N, Cc, H, W)).astype(np.float32)
        ref, S, n, tn, ti = SR.resize_bwd_ref(dy, h, w)
        err = np.abs(ref - _interp64_bwd(dy, h, w))
        lim = np.broadcast_to(_table_bwd_slack(dy, h, w), ref.shape)
        worst_b = max(worst_b, float((err / lim).max()))
        assert (err <= lim).all(), ((N, Cc, h, w, H, W), float(err.max()))
        assert (tn <= ti).all() and (n[ti] > 0).all()
    print(f"float64 interpolate: forward worst |err|/bound {worst_f:.3f}, adjoint worst |err|/bound {worst_b:.3f}")
    # the eager-torch spelling of the oracle (the large GPU shapes use it) gives the numpy form's bits
    xb = torch.from_numpy(rng.standard_normal((2, 9, 7, 8)).astype(np.float32)).bfloat16()
    a = SR.resize_fwd_ref_torch(xb, 19, 14, torch.bfloat16).float().permute(0, 3, 1, 2).numpy()
    b = SR.resize_fwd_ref(xb.float().permute(0, 3, 1, 2).numpy(), 19, 14, torch.bfloat16)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # ... and the index_add form of the adjoint (the large GPU shapes use it) is the dense form
    dyb = torch.from_numpy(rng.standard_normal((2, 19, 14, 8)))
    d1, S1, n1 = SR.resize_bwd_ref_nhwc(dyb, 9, 7)
    d2, S2, n2, _, _ = SR.resize_bwd_ref(dyb.permute(0, 3, 1, 2).numpy(), 9, 7)
    assert np.allclose(d1.permute(0, 3, 1, 2).numpy(), d2, rtol=0, atol=1e-13) and np.allclose(S1.permute(0, 3, 1, 2).numpy(), S2, rtol=1e-13)
    assert np.array_equal(n1, n2)
    # the identity resize returns its input's bits; at an exact scale of 1/2 every weight is 0, 1/2 or 1
    x = rng.standard_normal((1, 8, 12, 10)).astype(np.float32)
    assert np.array_equal(SR.resize_fwd_ref(x, 12, 10).view(np.int32), x.view(np.int32))
    for n_in, n_out in ((9, 17), (7, 13), (5, 9)):
        _, _, l0, l1 = SR.resize_tables(n_in, n_out)
        assert set(np.unique(np.concatenate([l0, l1]))) <= {0.0, 0.5, 1.0}


def test_rounding_to_a_16_bit_type_moves_a_value_by_half_an_ulp_of_that_type():
    """The 16-bit term of the adjoint's bound is half the SPACING of the type at the result: up to 2^-8 |v| for bf16 (8 significant
    bits) and 2^-11 |v| for fp16 (11) just above a power of two -- the rounding of the reference alone reaches it, so no smaller
    constant times |v| can bound a correctly rounded result."""
    v = np.linspace(0.25, 9.0, 20001)
    for dt, rel in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        r = torch.from_numpy(v).to(dt).double().numpy()
        err = np.abs(r - v)
        assert (err <= SR.half_ulp(v, dt)).all()
        assert (SR.half_ulp(v, dt) <= rel * v).all()
        worst = float((err / v).max())
        print(f"{dt}: worst rounding error {worst / rel:.3f} of {rel:.3e} |v|")
        assert worst > 0.9 * rel


def test_maxpool_oracle_on_ties_and_fixtures():
    d = load_npz("g2_spatial.npz")
    for tag in ("even", "odd", "rect"):
        x, y, dy, dx = (d[f"pool_{tag}/{k}"] for k in ("x", "y", "dy", "dx"))
        assert np.array_equal(SR.maxpool_fwd_ref(x), y) and np.array_equal(SR.maxpool_bwd_ref(x, dy), dx)
    g = torch.Generator().manual_seed(5)
    tied = []
    for shape in SR.POOL_SHAPES:
        x = SR.pool_input(shape, sum(shape))
        assert bool((x == 0).any()) and bool(torch.signbit(x).any()) and bool(((x == 0) & ~torch.signbit(x)).any())
        xr = x.clone().requires_grad_(True)
        y = TF.max_pool2d(xr, 2, 2)
        dy = torch.randint(1, 6, y.shape, generator=g).float()
        y.backward(dy)
        assert np.array_equal(SR.maxpool_fwd_ref(x.numpy()), y.detach().numpy())
        assert np.array_equal(SR.maxpool_bwd_ref(x.numpy(), dy.numpy()), xr.grad.numpy())
        tied.append(((SR._windows(x.numpy()) == SR.maxpool_fwd_ref(x.numpy())[None]).sum(0) > 1).mean())
    print("windows with more than one maximum:", " ".join(f"{v:.2f}" for v in tied))
    assert min(tied[1:]) > 0.3                                                   # (the first shape has 8 windows)


def _plan(lib, N, h, w, H, W, Cc):
    return lib.resize_bilinear_plan(N, h, w, H, W, Cc)


def test_resize_plan_query(lib):
    assert "mau_resize_bilinear_plan" in lib.PROTOTYPES and hasattr(lib.lib, "mau_resize_bilinear_plan")
    assert lib.PROTOTYPES["mau_resize_bilinear_plan"] == (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 3)
    assert lib.lib.mau_abi_version() == 5 and SR.RESIZE_FWD_ROWCOL == lib.RESIZE_FWD_ROWCOL
    assert lib.lib.mau_resize_bilinear_plan(2, 16, 16, 32, 32, 6, None, None, None) == 0          # null out-pointers are allowed
    fk = C.c_int(-1)
    assert lib.lib.mau_resize_bilinear_plan(2, 16, 16, 32, 32, 6, C.byref(fk), None, None) == 0 and fk.value == lib.RESIZE_FWD_ROWCOL
    assert lib.lib.mau_resize_bilinear_plan(0, 16, 16, 32, 32, 6, None, None, None) != 0
    assert b"resize_bilinear_plan" in lib.lib.mau_last_error()
    for kernel, shapes in ((lib.RESIZE_FWD_ROWCOL, SR.ROWCOL_SHAPES), (lib.RESIZE_FWD_CELL, SR.CELL_SHAPES), (lib.RESIZE_FWD_DEST, SR.DEST_SHAPES)):
        for (N, Cc, h, w, H, W) in shapes:
            fwd, rows, bwd = _plan(lib, N, h, w, H, W, Cc)
            assert fwd == kernel, ((N, Cc, h, w, H, W), fwd)
            assert rows == 1                                                     # the small shapes: one source row per workgroup
            gather = h < 2 or w < 2 or h > H or w > W
            assert bwd == (lib.RESIZE_BWD_GATHER if gather else lib.RESIZE_BWD_2X2), (N, Cc, h, w, H, W)
    for (N, Cc, h, w, H, W) in SR.BWD_EXTRA_SHAPES:
        assert _plan(lib, N, h, w, H, W, Cc)[2] == lib.RESIZE_BWD_2X2
    # the three large shapes: 2, 4 and 8 source rows per workgroup, none of which divides h
    seen = {1}
    for rows, (Cc, h, w, H, W) in SR.LARGE_ROWS_SHAPES.items():
        N = SR.large_rows_batch(lambda *a: _plan(lib, *a), rows)
        assert N is not None, f"no batch size gives {rows} rows per workgroup at {(Cc, h, w, H, W)}"
        assert _plan(lib, N, h, w, H, W, Cc) == (lib.RESIZE_FWD_ROWCOL, rows, lib.RESIZE_BWD_2X2)
        assert h % rows != 0 and N * H * W * SR.pad8(Cc) <= 64 << 20
        seen.add(rows)
    assert seen == {1, 2, 4, 8}
    # what production levels run: B = 32, 128 -> 256 at 128 channels
    assert _plan(lib, 32, 128, 128, 256, 256, 128) == (lib.RESIZE_FWD_ROWCOL, 8, lib.RESIZE_BWD_2X2)
    # any downsampling, and h < 2 or w < 2: the gather adjoint
    for (N, h, w, H, W) in ((1, 16, 12, 8, 6), (1, 4, 12, 8, 6), (1, 12, 4, 6, 8), (1, 1, 5, 4, 5), (1, 6, 1, 6, 7), (1, 1, 1, 3, 3), (3, 9, 9, 8, 64)):
        assert _plan(lib, N, h, w, H, W, 8)[2] == lib.RESIZE_BWD_GATHER, (N, h, w, H, W)


def test_spatial_entry_points_refuse_bad_arguments(lib):
    """Refused on the host, before any launch (the pointers are never dereferenced), with the entry named in mau_last_error."""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    L = lib.lib

    def refused(status, name):
        assert status != 0, name
        assert name.encode() in L.mau_last_error(), (name, L.mau_last_error())

    F32 = lib.MAU_F32
    # choff % 8 != 0
    refused(L.mau_resize_bilinear_fwd(p, 8, 4, 4, p, 24, 4, F32, 1, 8, 8, 8, None), "resize_bilinear_fwd")
    refused(L.mau_resize_bilinear_bwd(p, 24, 4, 8, 8, p, 8, F32, 1, 4, 4, 8, None), "resize_bilinear_bwd")
    refused(L.mau_resize_bilinear_bn_fwd(p, 8, 4, 4, p, p, p, 24, 4, F32, 1, 8, 8, 8, None), "resize_bilinear_bn_fwd")
    # lddst < choff + C8
    refused(L.mau_resize_bilinear_fwd(p, 8, 4, 4, p, 8, 8, F32, 1, 8, 8, 5, None), "resize_bilinear_fwd")
    refused(L.mau_resize_bilinear_bwd(p, 8, 8, 8, 8, p, 8, F32, 1, 4, 4, 5, None), "resize_bilinear_bwd")
    # the BatchNorm-fused resize is an upsampling
    refused(L.mau_resize_bilinear_bn_fwd(p, 8, 9, 4, p, p, p, 8, 0, F32, 1, 8, 8, 8, None), "resize_bilinear_bn_fwd")
    # maxpool2x2_bwd_add without the skip gradient
    refused(L.mau_maxpool2x2_bwd_add(p, 8, p, 8, None, 8, p, 8, F32, 1, 4, 4, 8, None), "maxpool2x2_bwd_add")
    # bcast_fill / copy_channels zero-filling past the row
    refused(L.mau_bcast_fill(p, p, 16, 8, 24, F32, 1, 4, 8, None), "bcast_fill")
    refused(L.mau_copy_channels(p, 8, p, 16, 8, 24, F32, 4, 8, None), "copy_channels")
