"""The HBM-streaming kernels of csrc/spatial.hip through the C ABI (ctypes), each against the plain reference of tests/spatial_ref.py:
MaxPool and its adjoint on tie-heavy inputs, the bilinear-resize kernels -- every forward and backward kernel the launchers can
choose, asserted reached with ``mau_resize_bilinear_plan`` -- bit for bit against one float32 oracle, the channel copy, and the
embedding broadcast with its adjoint.

Every buffer a kernel writes is NaN-prefilled and over-allocated by a few pixels at both ends: channels outside
[choff, choff + C8) and the pixels in front of / behind the tensor must still be NaN after the call, pad lanes [C, C8) must be 0.
Source buffers carry NaN in every lane a kernel has no business reading."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import spatial_ref as SR
from tests._helpers import NAN, SLACK, Buf, _bits_equal, _call, _nbits_differ, _stream, mau  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
pad8 = SR.pad8


def _code(dt):
    from mau_amd import _lib
    return {torch.float32: _lib.MAU_F32, torch.bfloat16: _lib.MAU_BF16, torch.float16: _lib.MAU_F16}[dt]


def _plan(N, h, w, H, W, C):
    from mau_amd import _lib
    return _lib.resize_bilinear_plan(N, h, w, H, W, C)


def _randn(shape, seed, dt):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dt).float()


def _randint(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ---- resize forward ----------------------------------------------------------------------------------------------------------------
FWD_CASES = [("rowcol", s) for s in SR.ROWCOL_SHAPES] + [("cell", s) for s in SR.CELL_SHAPES] + [("dest", s) for s in SR.DEST_SHAPES]


def _ids(cases):
    return [f"{k}-" + "x".join(map(str, s)) for k, s in cases]


def _run_resize_fwd(x, H, W, dt, choff, ldsrc, lddst):
    N, C, h, w = x.shape
    src = Buf(N * h * w, ldsrc, dt).put(x).cuda()
    dst = Buf(N * H * W, lddst, dt).cuda()
    _call("mau_resize_bilinear_fwd", src.ptr, ldsrc, h, w, dst.ptr, lddst, choff, _code(dt), N, H, W, C, _stream())
    return dst.get((N, C, H, W), choff)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,shape", FWD_CASES, ids=_ids(FWD_CASES))
def test_resize_fwd_bit_exact(mau, kind, shape, dt):
    """Every forward kernel against ONE oracle, bit for bit in all three types -- which also makes the three kernels bit-identical to
    each other.  Pixel pitches wider than the channel block on both sides, the destination block at channel 0, 8 or 24."""
    from mau_amd import _lib
    N, C, h, w, H, W = shape
    want = {"rowcol": _lib.RESIZE_FWD_ROWCOL, "cell": _lib.RESIZE_FWD_CELL, "dest": _lib.RESIZE_FWD_DEST}[kind]
    assert _plan(N, h, w, H, W, C)[0] == want
    C8 = pad8(C)
    x = _randn((N, C, h, w), sum(shape), dt)
    ref = torch.from_numpy(SR.resize_fwd_ref(x.numpy(), H, W, dt))
    for choff in ((0, 8, 24) if shape in (SR.ROWCOL_SHAPES[1], SR.CELL_SHAPES[0], SR.DEST_SHAPES[0]) else ((0, 8, 24)[sum(shape) % 3],)):
        got = _run_resize_fwd(x, H, W, dt, choff, C8 + 8, choff + C8 + 8)
        assert _bits_equal(got, ref), (shape, choff, _nbits_differ(got, ref), float((got - ref).abs().max()))
        if (h, w) == (H, W):
            assert _bits_equal(got, x)                          # the identity returns its input's bits
    if shape == (1, 64, 6, 40, 12, 80):
        assert w * C8 // 8 > 256                                # two x-chunks of the source row
    got = _run_resize_fwd(x, H, W, dt, 0, C8, C8)               # and the tight layout
    assert _bits_equal(got, ref)


@pytest.mark.parametrize("rows", [2, 4, 8])
def test_resize_fwd_rows_per_workgroup(mau, rows):
    """The row-column kernel with 2, 4 and 8 source rows per workgroup where the count does not divide h: the bottom-row -> top-row
    carry, the prefetch clamp min(ys + 2, h - 1) and the last workgroup's shortened column.  bf16, channels-last throughout, the
    oracle's arithmetic spelled with eager torch float32 operations."""
    from mau_amd import _lib
    C, h, w, H, W = SR.LARGE_ROWS_SHAPES[rows]
    N = SR.large_rows_batch(_plan, rows)
    assert N is not None and _plan(N, h, w, H, W, C)[:2] == (_lib.RESIZE_FWD_ROWCOL, rows) and h % rows != 0
    dt, choff = torch.bfloat16, 8
    ldsrc, lddst = C + 8, choff + C + 8
    g = torch.Generator().manual_seed(rows)
    x = torch.randn((N, h, w, C), generator=g).to(dt)
    src = Buf(N * h * w, ldsrc, dt)
    src.body.view(N, h, w, ldsrc)[..., :C] = x
    dst = Buf(N * H * W, lddst, dt).cuda()
    _call("mau_resize_bilinear_fwd", src.cuda().ptr, ldsrc, h, w, dst.ptr, lddst, choff, _code(dt), N, H, W, C, _stream())
    ref = SR.resize_fwd_ref_torch(x, H, W, dt)
    b = dst.back().view(N, H, W, lddst)
    assert bool(torch.isnan(b[..., :choff].float()).all()) and bool(torch.isnan(b[..., choff + C:].float()).all())
    got = b[..., choff:choff + C]
    bad = got.view(torch.int16) != ref.view(torch.int16)
    rows_bad = sorted(set(torch.nonzero(bad.any(-1).any(-1).any(0)).flatten().tolist()))[:8]
    print(f"rows per workgroup {rows}: N = {N}, {(N, C, h, w)} -> {(H, W)}, {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bool(bad.any()), (int(bad.sum()), rows_bad)


# ---- BatchNorm + ReLU fused into the resize ------------------------------------------------------------------------------------------
BN_SHAPES = [(2, 5, 15, 15, 31, 31), (1, 8, 9, 7, 17, 13), (1, 24, 6, 40, 12, 80), (1, 24, 5, 4, 15, 12), (2, 5, 1, 2, 4, 9), (1, 8, 6, 1, 6, 7)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", BN_SHAPES, ids=["x".join(map(str, s)) for s in BN_SHAPES])
def test_resize_bn_fwd_equals_apply_then_resize(mau, shape, dt):
    """mau_resize_bilinear_bn_fwd against mau_bn_relu_apply into a temporary + mau_resize_bilinear_fwd, bit for bit (random data),
    and against the oracle on dyadic data, where relu(scale * y + shift) is exact in every type however it is formed."""
    from mau_amd import _lib
    N, C, h, w, H, W = shape
    C8 = pad8(C)
    assert C in (5, 8, 24) and _plan(N, h, w, H, W, C)[0] in (_lib.RESIZE_FWD_ROWCOL, _lib.RESIZE_FWD_CELL)
    code, st = _code(dt), _stream()
    choff, ldy, lddst = 8, C8 + 8, 8 + C8 + 8
    g = torch.Generator().manual_seed(sum(shape))
    for dyadic in (False, True):
        if dyadic:
            y = torch.randint(-8, 9, (N, C, h, w), generator=g).float() / 4
            scale = torch.tensor([0.5, 0.5, -1.0, 2.0, -0.5, 1.0, -2.0, 1.0])[torch.arange(C) % 8]
            shift = torch.tensor([0.25, -4.0, 0.5, -1.0, 1.25, 0.0, -0.75, 2.0])[torch.arange(C) % 8]
        else:
            y = _randn((N, C, h, w), sum(shape) + 1, dt)
            scale = torch.randn(C, generator=g)
            shift = torch.randn(C, generator=g)
            scale[0], scale[2] = -scale[0].abs() - 0.1, scale[2].abs() + 0.1
            scale[1], shift[1] = 0.25, -40.0
        a = torch.relu(scale[None, :, None, None] * y + shift[None, :, None, None])
        assert float(a[:, 1].max()) == 0.0 and bool((scale < 0).any()) and bool((scale > 0).any())      # a channel entirely below 0
        ybuf = Buf(N * h * w, ldy, dt).put(y).cuda()
        ybuf.dev[SLACK:SLACK + N * h * w, C:C8] = 1.5        # the raw conv output's pad lanes are not defined: the result's must be 0
        sc, sh = scale.cuda(), shift.cuda()
        fused = Buf(N * H * W, lddst, dt).cuda()
        _call("mau_resize_bilinear_bn_fwd", ybuf.ptr, ldy, h, w, sc.data_ptr(), sh.data_ptr(), fused.ptr, lddst, choff, code, N, H, W, C, st)
        got = fused.get((N, C, H, W), choff)
        tmp = Buf(N * h * w, C8, dt).cuda()
        _call("mau_bn_relu_apply", ybuf.ptr, ldy, sc.data_ptr(), sh.data_ptr(), tmp.ptr, C8, code, N * h * w, C, st)
        two = Buf(N * H * W, lddst, dt).cuda()
        _call("mau_resize_bilinear_fwd", tmp.ptr, C8, h, w, two.ptr, lddst, choff, code, N, H, W, C, st)
        assert _bits_equal(got, two.get((N, C, H, W), choff)), (shape, dyadic)
        if dyadic:
            assert _bits_equal(tmp.get((N, C, h, w)), a)
            assert _bits_equal(got, torch.from_numpy(SR.resize_fwd_ref(a.numpy(), H, W, dt))), shape


# ---- resize backward ---------------------------------------------------------------------------------------------------------------
BWD_SHAPES = SR.ROWCOL_SHAPES + SR.CELL_SHAPES + SR.DEST_SHAPES + [s for s in SR.BWD_EXTRA_SHAPES if s not in SR.CELL_SHAPES]


def _run_resize_bwd(dy, h, w, dt, choff, ldddst, lddsrc):
    N, C, H, W = dy.shape
    ddst = Buf(N * H * W, ldddst, dt).put(dy, choff).cuda()
    dsrc = Buf(N * h * w, lddsrc, dt).cuda()
    _call("mau_resize_bilinear_bwd", ddst.ptr, ldddst, choff, H, W, dsrc.ptr, lddsrc, _code(dt), N, h, w, C, _stream())
    return dsrc.get((N, C, h, w))


@functools.lru_cache(maxsize=None)
def _bwd_ref(shape, dt):
    N, C, h, w, H, W = shape
    dy = _randn((N, C, H, W), sum(shape) + 7, dt)
    return dy, SR.resize_bwd_ref(dy.numpy(), h, w)


_worst_bwd = {}


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=["x".join(map(str, s)) for s in BWD_SHAPES])
def test_resize_bwd_within_rounding_bound(mau, shape, dt):
    """The adjoint against the float64 sum over the same float32 tables: |got - ref| <= (n + 1) * 2^-24 * S, plus half an ulp of the
    stored 16-bit value (spatial_ref.resize_bwd_bound); the 2x2 / gather choice is the plan query's."""
    from mau_amd import _lib
    N, C, h, w, H, W = shape
    gather = h < 2 or w < 2 or h > H or w > W
    assert _plan(N, h, w, H, W, C)[2] == (_lib.RESIZE_BWD_GATHER if gather else _lib.RESIZE_BWD_2X2)
    C8 = pad8(C)
    choff = (0, 8, 24)[sum(shape) % 3]
    dy, (ref, S, n, _, _) = _bwd_ref(shape, dt)
    got = _run_resize_bwd(dy, h, w, dt, choff, choff + C8 + 8, C8 + 8).double().numpy()
    bound = SR.resize_bwd_bound(ref, S, n, dt)
    ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    key = DT_IDS[DTYPES.index(dt)]
    _worst_bwd[key] = max(_worst_bwd.get(key, 0.0), ratio)
    print(f"resize bwd {shape} {key}: worst |err| / bound {ratio:.3f} (so far {_worst_bwd[key]:.3f})")
    assert ratio <= 1.0, (shape, ratio)


@pytest.mark.parametrize("rows", [2, 4, 8])
def test_resize_bwd_at_the_large_shapes(mau, rows):
    """The adjoint of the three large row-column shapes, bf16, channels-last: source coordinates in the thousands in the 2x2 kernel's
    loose window estimates and their tightening loops, up to 2047 block rows, two x-chunks of block columns at 256 channels.  The
    same bound as the small shapes, the reference by index_add in float64."""
    from mau_amd import _lib
    C, h, w, H, W = SR.LARGE_ROWS_SHAPES[rows]
    N = SR.large_rows_batch(_plan, rows)
    assert N is not None
    N = min(N, 4)                   # (the batch size does not enter the adjoint's plan or its per-image work: 4 images keep the float64 reference quick)
    assert _plan(N, h, w, H, W, C)[2] == _lib.RESIZE_BWD_2X2
    if rows == 2:
        assert ((w + 1) // 2) * (C // 8) > 256                 # two x-chunks of 2-column blocks
    dt, choff = torch.bfloat16, 8
    ldddst, lddsrc = choff + C + 8, C + 8
    g = torch.Generator().manual_seed(10 + rows)
    dy = torch.randn((N, H, W, C), generator=g).to(dt)
    ddst = Buf(N * H * W, ldddst, dt)
    ddst.body.view(N, H, W, ldddst)[..., choff:choff + C] = dy
    dsrc = Buf(N * h * w, lddsrc, dt).cuda()
    _call("mau_resize_bilinear_bwd", ddst.cuda().ptr, ldddst, choff, H, W, dsrc.ptr, lddsrc, _code(dt), N, h, w, C, _stream())
    b = dsrc.back().view(N, h, w, lddsrc)
    assert bool(torch.isnan(b[..., C:].float()).all())
    got = b[..., :C].double().numpy()
    ref, S, n = SR.resize_bwd_ref_nhwc(dy, h, w)
    ref, S = ref.numpy(), S.numpy()
    bound = SR.resize_bwd_bound(ref, S, n[None, :, :, None], dt)
    ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"resize bwd, large shape {(N, C, h, w)} <- {(H, W)} bf16: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _bwd2_window_cols(w, W):
    """destination columns in the window of each 2-column block of the 2x2 adjoint (those whose x0 lies in [xi0 - 1, xi0 + 1])"""
    x0 = SR.resize_tables(w, W)[0]
    return [int(((x0 >= xi0 - 1) & (x0 <= xi0 + 1)).sum()) for xi0 in range(0, w, 2)]


def test_resize_bwd_extra_shapes_reach_the_wide_window_loop():
    """More than 8 destination columns per block takes the 2x2 kernel's general loop: one extra shape has such blocks next to narrow
    ones (both forms in one launch), one has only such blocks."""
    cols = {s: _bwd2_window_cols(s[3], s[5]) for s in SR.BWD_EXTRA_SHAPES}
    assert any(max(c) > 8 and min(c) <= 8 for c in cols.values()), cols
    assert any(min(c) > 8 for c in cols.values()), cols


EXACT_BWD_SHAPES = [(1, 8, 9, 7, 17, 13), (2, 5, 8, 6, 15, 11), (1, 8, 2, 2, 3, 3)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", EXACT_BWD_SHAPES, ids=["x".join(map(str, s)) for s in EXACT_BWD_SHAPES])
def test_resize_bwd_exact_at_half_scale(mau, shape, dt):
    """H = 2h - 1, W = 2w - 1: every weight is 0, 1/2 or 1, small-integer gradients sum exactly in every type; odd h and w leave the
    last 2x2 block of a row / column half outside the tensor."""
    N, C, h, w, H, W = shape
    assert (H, W) == (2 * h - 1, 2 * w - 1)
    dy = _randint((N, C, H, W), sum(shape), -4, 4)
    ref, _, _, _, _ = SR.resize_bwd_ref(dy.numpy(), h, w)
    got = _run_resize_bwd(dy, h, w, dt, 8, 8 + pad8(C) + 8, pad8(C) + 8)
    assert _bits_equal(got, torch.from_numpy(ref).float()) and _bits_equal(torch.from_numpy(ref).float().to(dt), torch.from_numpy(ref).float())


INF_SHAPES = [("fast", (1, 8, 9, 7, 17, 13)), ("wide", (1, 8, 4, 3, 16, 12)), ("gather", (1, 8, 16, 12, 8, 6))]


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind,shape", INF_SHAPES, ids=[k for k, _ in INF_SHAPES])
def test_resize_bwd_contains_a_non_finite_gradient(mau, kind, shape, dt):
    """One +Inf in the incoming gradient: the non-finite source elements contain every source pixel the destination pixel reaches
    with a non-zero weight and are contained in those it has as y0|y1 and x0|x1; every finite element keeps the bits of the run
    without the Inf."""
    from mau_amd import _lib
    N, C, h, w, H, W = shape
    assert _plan(N, h, w, H, W, C)[2] == (_lib.RESIZE_BWD_GATHER if kind == "gather" else _lib.RESIZE_BWD_2X2)
    if kind != "gather":
        cols = _bwd2_window_cols(w, W)
        assert (max(cols) <= 8) if kind == "fast" else (max(cols) > 8)
    C8 = pad8(C)
    dy = _randn((N, C, H, W), 3 + sum(shape), dt)
    base = _run_resize_bwd(dy, h, w, dt, 8, 8 + C8 + 8, C8)
    assert bool(torch.isfinite(base).all())
    ch = 2
    positions = [(1, 1) if H > 2 else (0, 1), (0, 0), (H - 1, W // 2), (H // 2, W - 1)] + ([(4, 4)] if (h, H) == (9, 17) else [])
    for (j, k) in positions:
        d2 = dy.clone()
        d2[0, ch, j, k] = float("inf")
        got = _run_resize_bwd(d2, h, w, dt, 8, 8 + C8 + 8, C8)
        tn, ti = SR.resize_touch(h, w, H, W, j, k)
        bad = ~torch.isfinite(got)
        hit = bad[0, ch].numpy()
        assert (tn <= hit).all(), (kind, (j, k), "a contributor stayed finite")
        assert (hit <= ti).all(), (kind, (j, k), "a source pixel that never read the destination pixel became non-finite")
        bad[0, ch] = False
        assert not bool(bad.any())
        fin = torch.isfinite(got)
        assert _bits_equal(got[fin], base[fin]), (kind, (j, k))


# ---- MaxPool -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SR.POOL_SHAPES, ids=["x".join(map(str, s)) for s in SR.POOL_SHAPES])
def test_maxpool_and_adjoint_on_ties(mau, shape, dt):
    """Forward, adjoint and adjoint + skip gradient on inputs where four windows in ten have several maxima: the gradient goes to the
    first one in scan order, bit for bit; an odd last row / column gets 0, or exactly the skip gradient.  Four different pitches."""
    N, C, H, W = shape
    Ho, Wo, C8 = H // 2, W // 2, pad8(C)
    code, st = _code(dt), _stream()
    ldx, lddy, lddskip, lddx = C8 + 8, C8, C8 + 16, C8 + 24
    x = SR.pool_input(shape, sum(shape))
    dy = _randint((N, C, Ho, Wo), sum(shape) + 1, 1, 5)
    dskip = _randint((N, C, H, W), sum(shape) + 2, 1, 7) * (1 - 2 * (_randint((N, C, H, W), 9, 0, 1)))      # +-1..7, never zero
    if shape == (1, 72, 6, 64):
        assert W * C8 // 8 > 256 and Wo * C8 // 8 > 256      # two x-chunks, forward and backward
    xb = Buf(N * H * W, ldx, dt).put(x).cuda()
    yb = Buf(N * Ho * Wo, ldx, dt).cuda()
    _call("mau_maxpool2x2_fwd", xb.ptr, ldx, yb.ptr, ldx, code, N, H, W, C, st)
    assert torch.equal(yb.get((N, C, Ho, Wo)), torch.from_numpy(SR.maxpool_fwd_ref(x.numpy())))      # (the sign of a zero maximum is the max's choice)
    dyb = Buf(N * Ho * Wo, lddy, dt).put(dy).cuda()
    want = torch.from_numpy(SR.maxpool_bwd_ref(x.numpy(), dy.numpy()))
    dxb = Buf(N * H * W, lddx, dt).cuda()
    _call("mau_maxpool2x2_bwd", xb.ptr, ldx, dyb.ptr, lddy, dxb.ptr, lddx, code, N, H, W, C, st)
    got = dxb.get((N, C, H, W))
    assert _bits_equal(got, want), _nbits_differ(got, want)
    assert float(got[:, :, 2 * Ho:].abs().sum()) == 0 and float(got[:, :, :, 2 * Wo:].abs().sum()) == 0
    skb = Buf(N * H * W, lddskip, dt).put(dskip).cuda()
    dxa = Buf(N * H * W, lddx, dt).cuda()
    _call("mau_maxpool2x2_bwd_add", xb.ptr, ldx, dyb.ptr, lddy, skb.ptr, lddskip, dxa.ptr, lddx, code, N, H, W, C, st)
    got = dxa.get((N, C, H, W))
    assert _bits_equal(got, want + dskip), _nbits_differ(got, want + dskip)
    assert _bits_equal(got[:, :, 2 * Ho:], dskip[:, :, 2 * Ho:]) and _bits_equal(got[:, :, :, 2 * Wo:], dskip[:, :, :, 2 * Wo:])


# ---- embedding broadcast and its adjoint ---------------------------------------------------------------------------------------------
def _run_bcast_bwd(dx, ld, choff, E, dt, ws_mode):
    from mau_amd._lib import lib
    N, HW = dx.shape[:2]
    buf = Buf(N * HW, ld, dt)
    buf.body.view(N, HW, ld)[..., choff:choff + E] = dx.to(dt)
    demb = Buf(N, E, torch.float32).cuda()
    need = lib.mau_bcast_bwd_ws_elems(N, HW, E)
    assert need == N * -(-HW // 2048) * E
    ws = None if ws_mode == "null" else torch.full((need + (4096 if ws_mode == "oversized" else 0),), NAN, dtype=torch.float32, device="cuda")
    _call("mau_bcast_bwd", buf.cuda().ptr, ld, choff, demb.ptr, None if ws is None else ws.data_ptr(), _code(dt), N, HW, E, _stream())
    out = demb.back().clone()
    if ws_mode == "oversized":
        assert bool(torch.isnan(ws[need:]).all()), "the workspace was written behind the queried size"
    return out


BCAST_BWD_CASES = [(2, 2048 + 33, 40, 16), (1, 3 * 2048, 64, 0), (3, 31, 8, 8), (2, 65, 72, 24)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", BCAST_BWD_CASES, ids=["x".join(map(str, c)) for c in BCAST_BWD_CASES])
def test_bcast_bwd_exact_sums(mau, case, dt):
    """Integer gradients: every fp32 partial sum is exact, the result equals the float64 sum bit for bit -- across several 2048-pixel
    chunks, E no multiple of 64, pixel counts that leave a tail of the 64- and the 32-pixel loops; the same from an oversized
    workspace, and from the element kernel (no workspace)."""
    N, HW, E, choff = case
    ld = pad8(choff + E) + 8
    dx = _randint((N, HW, E), sum(case), -3, 3)
    ref = torch.from_numpy(SR.bcast_bwd_ref(dx.numpy(), 0, E)).float()
    assert float(ref.abs().max()) < 2 ** 24
    got = _run_bcast_bwd(dx, ld, choff, E, dt, "exact")
    assert _bits_equal(got, ref)
    assert _bits_equal(_run_bcast_bwd(dx, ld, choff, E, dt, "oversized"), got)
    assert _bits_equal(_run_bcast_bwd(dx, ld, choff, E, dt, "null"), ref)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [(2, 133, 8, 4), (2, 133, 5, 8), (1, 70, 5, 3)], ids=["choff4", "E5", "E5-choff3"])
def test_bcast_bwd_element_path(mau, case, dt):
    """A channel offset or count that is no multiple of 8 takes the element kernel even with a workspace (which stays unwritten)."""
    N, HW, E, choff = case
    ld = pad8(choff + E) + 8
    dx = _randint((N, HW, E), sum(case), -3, 3)
    ref = torch.from_numpy(SR.bcast_bwd_ref(dx.numpy(), 0, E)).float()
    assert _bits_equal(_run_bcast_bwd(dx, ld, choff, E, dt, "oversized"), ref)
    assert _bits_equal(_run_bcast_bwd(dx, ld, choff, E, dt, "null"), ref)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("E,choff", [(5, 3), (5, 8), (8, 3), (8, 8)])
def test_bcast_fill_writes_its_channels_only(mau, E, choff, dt):
    N, HW = 2, 37
    ld = pad8(choff + E) + 8
    emb = _randn((N, E), E + choff, dt)
    for zero_to in (0, choff + E, ld):
        dst = Buf(N * HW, ld, dt).cuda()
        embd = emb.cuda()
        _call("mau_bcast_fill", embd.data_ptr(), dst.ptr, ld, choff, zero_to, _code(dt), N, HW, E, _stream())
        b = dst.back().view(N, HW, ld).float()
        end = max(zero_to, choff + E)
        assert bool(torch.isnan(b[..., :choff]).all()) and bool(torch.isnan(b[..., end:]).all())
        assert _bits_equal(b[..., choff:choff + E], emb[:, None, :].expand(N, HW, E))
        assert bool((b[..., choff + E:end] == 0).all())


# ---- channel copy ------------------------------------------------------------------------------------------------------------------
def _run_copy(src_vals, ldsrc, lddst, choff, zero_to, dt, src_advance=0, expect=None):
    """src_vals (npix, C); ``src_advance``: the source tensor starts that many channels into its buffer's pixels"""
    npix, C = src_vals.shape
    src = Buf(npix, ldsrc, dt)
    src.body[:, src_advance:src_advance + C] = src_vals.to(dt)
    dst = Buf(npix, lddst, dt).cuda()
    sptr = src.cuda().ptr + src_advance * src.dev.element_size()
    # which kernel the launcher takes hangs on these addresses: the cases say what they mean to pass
    # (``expect``: "aligned" = both pointers on 16 bytes, with channel counts that fit the vector kernel; "src_misaligned" = the same
    #  but for the source address; None = the channel counts alone select the element kernel)
    if expect is not None:
        assert dst.ptr % 16 == 0 and (sptr % 16 == 0) == (expect == "aligned"), (expect, sptr % 16, dst.ptr % 16)
    _call("mau_copy_channels", sptr, ldsrc, dst.ptr, lddst, choff, zero_to, _code(dt), npix, C, _stream())
    b = dst.back().float()
    end = max(zero_to, choff + C)
    assert bool(torch.isnan(b[:, :choff]).all()) and bool(torch.isnan(b[:, end:]).all()), "channels outside the copy were written"
    assert _bits_equal(b[:, choff:choff + C], src_vals), _nbits_differ(b[:, choff:choff + C], src_vals)
    assert bool((b[:, choff + C:end] == 0).all())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [8, 64, 2048 + 8])
def test_copy_channels_vector_path(mau, C, dt):
    """8-channel vectors: fewer and more than 256 of them per pixel, pixel counts around the four-pixel unrolled loop of a thread's
    walk (PS pixel slots per workgroup, 8 * PS pixels per workgroup) and its tail."""
    nv = C // 8
    PS = 256 // min(nv, 256)
    for i, npix in enumerate((1, 7, 8, 33, 4 * PS + 3, 4 * PS * 3 + 3)):
        vals = _randn((npix, C), C + npix, dt)
        choff = (0, 8)[i % 2]
        _run_copy(vals, C + 8, choff + C + 16, choff, 0, dt, expect="aligned")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_copy_channels_element_path(mau, dt):
    """C = 5 at channel 3: element granularity, zero fill up to ``zero_to`` when that lies above choff + C, none when below."""
    for npix in (1, 33, 1027):
        vals = _randn((npix, 5), npix, dt)
        for zero_to in (0, 8, 13, 16):
            _run_copy(vals, 8, 16, 3, zero_to, dt)
        _run_copy(vals, 5, 11, 3, 11, dt)                       # pitches that are no multiple of 8


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32, torch.float16], ids=["bf16", "fp32", "fp16"])
@pytest.mark.parametrize("advance", [4, 2, 1])
def test_copy_channels_source_not_16_byte_aligned(mau, advance, dt):
    """What ConcatUp.backward passes for a skip of 8 channels behind one of 4: a source pointer advanced by 4 channels, C = 8,
    choff = 0.  Every other argument fits the vector kernel; the address does not (8 bytes into a 16-byte vector in the 16-bit
    types), so the launcher must take the element kernel -- the result is the slice either way.  (In fp32 four channels are 16
    bytes: that case is the vector kernel on an offset pointer, and is asserted to be.)"""
    esize = torch.empty((), dtype=dt).element_size()
    expect = "src_misaligned" if (advance * esize) % 16 else "aligned"
    assert expect == "src_misaligned" or (dt, advance) == (torch.float32, 4)
    for npix in (1, 33, 2051):
        vals = _randn((npix, 8), npix + advance, dt)
        _run_copy(vals, 16, 8, 0, 8, dt, src_advance=advance, expect=expect)
        _run_copy(vals, 24, 16, 8, 0, dt, src_advance=advance, expect=expect)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_concat_up_with_a_4_channel_skip_in_front(mau, dt):
    """ConcatUp with skips of 4 and 8 channels and 8 low-resolution channels: the second skip's and the upsampled block's gradients
    start at channels 4 and 12 of the incoming gradient.  (5, 4) -> (9, 7) is a scale of exactly 1/2 and the data are small
    integers: forward and backward equal torch.cat + interpolate in float64 exactly."""
    from mau_amd import functional as F_
    N, h, w, H, W = 2, 5, 4, 9, 7
    low, s0, s1 = _randint((N, 8, h, w), 1, -4, 4), _randint((N, 4, H, W), 2, -4, 4), _randint((N, 8, H, W), 3, -4, 4)
    g = _randint((N, 20, H, W), 4, -4, 4)
    ref_in = [v.clone().double().requires_grad_(True) for v in (low, s0, s1)]
    ref = torch.cat([ref_in[1], ref_in[2], TF.interpolate(ref_in[0], size=(H, W), mode="bilinear", align_corners=True)], 1)
    ref.backward(g.double())
    dev = [F_.ToNHWC.apply(v.cuda(), dt).detach().requires_grad_(True) for v in (low, s0, s1)]
    out = F_.ConcatUp.apply(dev[0], 8, False, (4, 8), dev[1], dev[2])
    assert torch.equal(F_.to_nchw(F_.Act(out.detach(), 20)).cpu().double(), ref.detach())
    assert float(out.detach()[..., 20:].float().abs().sum()) == 0
    out.backward(F_.ToNHWC.apply(g.cuda(), dt))
    torch.cuda.synchronize()
    for t_dev, t_ref, C in zip(dev, ref_in, (8, 4, 8)):
        assert torch.equal(F_.to_nchw(F_.Act(t_dev.grad, C)).cpu().double(), t_ref.grad), C


# ---- flip --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 255, 257])
def test_flip_rows(mau, W):
    N, C, H = 3, 2, 3
    x = _randn((N, C, H, W), W, torch.float32)
    flip = torch.tensor([1, 0, 7], dtype=torch.uint8)
    src = Buf(N * C * H, W, torch.float32)
    src.body[:] = x.reshape(N * C * H, W)
    dst = Buf(N * C * H, W, torch.float32).cuda()
    fd = flip.cuda()
    _call("mau_flip_rows", src.cuda().ptr, dst.ptr, fd.data_ptr(), N, C, H, W, _stream())
    got = dst.back().view(N, C, H, W)
    want = torch.stack([torch.flip(x[n], dims=[-1]) if int(flip[n]) else x[n] for n in range(N)])
    assert _bits_equal(got, want)
    assert _bits_equal(got, torch.from_numpy(SR.flip_rows_ref(x.numpy(), flip.tolist())))
