"""The BatchNorm-backward kernels (csrc/bn.hip), their pool- and head-fused forms (csrc/bn_fused.hip) and the output head
(csrc/head.hip) through the C ABI, each against the plain float64 reference of tests/bn_head_ref.py.

The exact cases (scale / invstd powers of two, everything else small integers or dyadic fractions: tests/test_bn_head_host.py proves
every sum exact in float32 in any order) must equal the reference rounded to the tensor type BIT FOR BIT; one random case per kernel is
held to the rounding bounds of ``bn_head_ref``.  Source tensors carry NaN in every lane outside [0, C8) and in sentinel pixels at
both ends, 0 in the pad lanes [C, C8); every written buffer is NaN-prefilled, and what a kernel has no business writing must still be
NaN afterwards (``Buf``).  Pixel pitch C8 and C8 + 16 (a channel slice of a wider buffer)."""
import itertools

import numpy as np
import pytest
import torch

from tests import bn_head_ref as R
from tests._helpers import Buf, _call, _stream, mau, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

pad8 = R.pad8
# Largest distance seen between tanhf on the device and float64 tanh rounded to float32, over the exact arguments of every head case
# of this module (multiples of 1/8, most within [-12, 12]; head_fwd on both paths, head_bn_fwd, head_mean): 1 ulp.  Asserted: twice
# that.  The inputs are a fixed finite set.
TANH_ULPS = 2
_tanh_seen = {}                                               # exact argument -> bits of tanhf, whichever kernel computed it
_tanh_worst = [0]


def _code(dt):
    from mau_amd import _lib
    return {torch.float32: _lib.MAU_F32, torch.bfloat16: _lib.MAU_BF16, torch.float16: _lib.MAU_F16}[dt]


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).float()


def _src(vals, ld, dt):
    """(npix, C) values -> device buffer of pitch ld: pad lanes 0, every other lane and the sentinel pixels NaN"""
    npix, C = vals.shape
    b = Buf(npix, ld, dt)
    b.body[:, :C] = torch.from_numpy(vals).to(dt)
    b.body[:, C:pad8(C)] = 0
    return b.cuda()


def _rows(vals):
    """an fp32 source matrix (rows, n) with NaN sentinel rows at both ends (out / dout of the head as (N * Co, HW))"""
    b = Buf(vals.shape[0], vals.shape[1], torch.float32)
    b.body[:] = _f32(vals)
    return b.cuda()


def _read(buf, C):
    """(npix, C) float32 of a written buffer: lanes outside [0, C8) still NaN, pad lanes 0"""
    b = buf.back().float()
    assert bool(torch.isnan(b[:, pad8(C):]).all()), "lanes outside [0, C8) were written"
    assert bool((b[:, C:pad8(C)] == 0).all()), "pad lanes are not 0"
    return b[:, :C]


def _coefs(k):
    return {n: _f32(v).cuda() for n, v in k.items()}


def _kp(d, *names):
    return [d[n].data_ptr() for n in names]


def _bn_slab(slab, nb, C, ldslab, written):
    """(blocks, 2, C) of a BatchNorm slab; columns [C, written) hold 0, the rest is still NaN"""
    g = slab.back().view(nb, 2, ldslab)
    assert bool((g[..., C:written] == 0).all()) and bool(torch.isnan(g[..., written:]).all()), "slab columns beyond C"
    return g[..., :C]


def _sums(B):
    return torch.from_numpy(np.append(B.sums, B.count)).cuda()


def _want(x, dt):
    return _f32(R.round_t(x, dt))


# ---- bn_relu_bwd_reduce / bn_relu_bwd_apply -------------------------------------------------------------------------------------------
def _bn_bwd_exact(npix, C, dt):
    c = R.exact_bn_case(npix, C)
    B = R.BnBwd(c["da"], c["y"], c["k"], R.EXACT_COUNT)
    k, C8, nb, code, st = _coefs(c["k"]), pad8(C), -(-npix // R.BLOCK), _code(dt), _stream()
    for ld, ldslab in ((C8, C), (C8 + 16, C8 + 8)):
        dab, yb = _src(c["da"], ld, dt), _src(c["y"], ld + 8, dt)
        slab = Buf(2 * nb, ldslab, torch.float32).cuda()
        _call("mau_bn_relu_bwd_reduce", dab.ptr, ld, yb.ptr, ld + 8, *_kp(k, "scale", "shift", "mean", "invstd"), slab.ptr, ldslab, code, npix, C, st)
        assert same_bits(_bn_slab(slab, nb, C, ldslab, min(ldslab, -(-C // 64) * 64)), _f32(B.slab)), ("slab", npix, C, ld)
        sums, got = _sums(B), []
        for count in (R.EXACT_COUNT, 0.0):                    # count = 0: the count travels in sums[2 * C]
            dyb = Buf(npix, ld, dt).cuda()
            _call("mau_bn_relu_bwd_apply", dab.ptr, ld, yb.ptr, ld + 8, *_kp(k, "scale", "shift", "mean", "invstd"), sums.data_ptr(), count, dyb.ptr, ld,
                  code, npix, C, st)
            got.append(_read(dyb, C))
        assert same_bits(got[0], _want(B.dy, dt)), ("dy", npix, C, ld)
        assert same_bits(got[1], got[0]), ("dy, count in the sums", npix, C, ld)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("npix", R.BN_NPIX)
def test_bn_relu_bwd_exact(mau, npix, dt):
    """Empty pixel slots (5), the pair loop and its tail (33), a block one pixel short, full, and one pixel over (a 1-pixel block), two
    blocks and a part; C with pad lanes, an idle last thread (nv = 3), a second, partial 64-channel block with ldslab = C."""
    for C in R.BN_C:
        _bn_bwd_exact(npix, C, dt)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("npix,C", R.BN_WIDE)
def test_bn_relu_bwd_exact_wide(mau, npix, C, dt):
    """nv = 128: two pixel slots per workgroup in the apply kernel; nv = 257 > 256: its outer vector loop"""
    _bn_bwd_exact(npix, C, dt)


# ---- bn_relu_apply_pool with argidx, pool_bn_bwd_reduce / apply ------------------------------------------------------------------------
ARG_SLACK = 16


def _apply_pool(yb, ld, k, N, H, W, C, dt):
    """-> a (npix, C), pooled (nwin, C), argidx (nwin, C8 / 8) int64 and the device argidx tensor (with its sentinels)"""
    npix, nwin, nv = N * H * W, N * (H // 2) * (W // 2), pad8(C) // 8
    ab, pb = Buf(npix, ld, dt).cuda(), Buf(nwin, ld + 8, dt).cuda()
    arg = torch.full((nwin * nv + 2 * ARG_SLACK,), -1, dtype=torch.int16).cuda()
    _call("mau_bn_relu_apply_pool", yb.ptr, ld, *_kp(k, "scale", "shift"), ab.ptr, ld, pb.ptr, ld + 8, arg.data_ptr() + 2 * ARG_SLACK, _code(dt), N, H, W, C,
          _stream())
    a, pooled = _read(ab, C), _read(pb, C)
    h = arg.cpu()
    assert bool((h[:ARG_SLACK] == -1).all()) and bool((h[ARG_SLACK + nwin * nv:] == -1).all()), "argidx written outside [nwin][nv]"
    return a, pooled, (h[ARG_SLACK:ARG_SLACK + nwin * nv].view(nwin, nv).long() & 0xFFFF), arg


def _pool_bwd(yb, ld, k, arg_dev, dpl, dskip, B, N, H, W, C, dt, check_slab, check_dy):
    npix, nwin, C8, code, st = N * H * W, N * (H // 2) * (W // 2), pad8(C), _code(dt), _stream()
    nb = -(-npix // R.BLOCK)
    pb = _src(dpl, ld + 8, dt) if dpl is not None else None
    sb = _src(dskip, ld, dt) if dskip is not None else None
    grads = (pb.ptr if pb else None, ld + 8, arg_dev.data_ptr() + 2 * ARG_SLACK, sb.ptr if sb else None, ld)
    ldslab = C if ld == C8 else C8 + 8
    slab = Buf(2 * nb, ldslab, torch.float32).cuda()
    _call("mau_pool_bn_bwd_reduce", yb.ptr, ld, *grads, *_kp(k, "scale", "shift", "mean", "invstd"), slab.ptr, ldslab, code, N, H, W, C, st)
    check_slab(_bn_slab(slab, nb, C, ldslab, min(ldslab, -(-C // 64) * 64)))
    sums, got = _sums(B), []
    for count in (B.count, 0.0):
        dyb = Buf(npix, ld + 16, dt).cuda()
        _call("mau_pool_bn_bwd_apply", yb.ptr, ld, *grads, *_kp(k, "scale", "shift", "mean", "invstd"), sums.data_ptr(), count, dyb.ptr, ld + 16, code,
              N, H, W, C, st)
        got.append(_read(dyb, C))
    assert same_bits(got[1], got[0]), "dy, count in the sums"
    check_dy(got[0])


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=["x".join(map(str, s)) for s in R.POOL_SHAPES])
def test_apply_pool_argidx_and_pool_bn_bwd_exact(mau, shape, dt):
    """a, pooled and the 2-bit first-maximum index on tie-heavy activations; then the fused backward fed with THAT index, in its three
    forms.  Odd sizes: the last row / column lies outside the pooled range and gets the skip gradient only.  (3, 4, 3): an image is
    shorter than the 32-pixel stride of the reduce kernel's walk, which then wraps rows and images within one step."""
    N, H, W = shape
    for C in R.POOL_C:
        c = R.exact_pool_case(N, H, W, C)
        k, C8 = _coefs(c["k"]), pad8(C)
        a_ref = R.bn_relu_apply(c["y"], c["k"]["scale"], c["k"]["shift"], dt)
        pooled_ref, arg_ref = R.pool_first_max(a_ref, N, H, W)
        for ld in (C8, C8 + 16):
            yb = _src(c["y"], ld, dt)
            a, pooled, bits, arg_dev = _apply_pool(yb, ld, k, N, H, W, C, dt)
            assert same_bits(a, _f32(a_ref)) and same_bits(pooled, _f32(pooled_ref)), (shape, C, ld)
            assert torch.equal(bits, torch.from_numpy(R.pack_argidx(arg_ref).astype(np.int64))), (shape, C, ld, "argidx")
            for dpl, dskip in ((c["dpl"], c["dskip"]), (c["dpl"], None), (None, c["dskip"])):
                pre = R.pool_da_pre(dpl, arg_ref, dskip, N, H, W)
                if dskip is not None:                         # outside the pooled range: the skip gradient only
                    v, s = pre.reshape(N, H, W, C), dskip.reshape(N, H, W, C)
                    assert (v[:, 2 * (H // 2):] == s[:, 2 * (H // 2):]).all() and (v[:, :, 2 * (W // 2):] == s[:, :, 2 * (W // 2):]).all()
                B = R.BnBwd(R.round_t(pre, dt), c["y"], c["k"], R.EXACT_COUNT)
                what = (shape, C, ld, dpl is not None, dskip is not None)
                _pool_bwd(yb, ld, k, arg_dev, dpl, dskip, B, N, H, W, C, dt,
                          lambda g: _assert(same_bits(g, _f32(B.slab)), ("slab",) + what), lambda g: _assert(same_bits(g, _want(B.dy, dt)), ("dy",) + what))


def _assert(ok, what):
    assert ok, what


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def _check_out(got, pre, tanh0, what):
    """got (N, Co, HW) float32 against the exact pre-activation: bit for bit, but for the tanh channel: tanhf against float64 tanh
    rounded to float32 in ulps, and ONE result per argument across every kernel of this module"""
    lin = slice(1, None) if tanh0 else slice(None)
    assert same_bits(got[:, lin], _f32(pre[:, lin])), what
    if tanh0:
        t = got[:, 0].numpy().ravel()
        d = int(R.ulp_distance_f32(t, np.tanh(pre[:, 0]).astype(np.float32).ravel()).max())
        _tanh_worst[0] = max(_tanh_worst[0], d)
        print(f"tanhf {what}: {d} ulp (so far {_tanh_worst[0]})")
        assert d <= TANH_ULPS, (what, d)
        args, first = np.unique(pre[:, 0].ravel(), return_index=True)
        for x, b in zip(args.tolist(), t.view(np.int32)[first].tolist()):
            assert _tanh_seen.setdefault(x, b) == b, (what, "tanhf of one argument differs between kernels or pixels", x)
        assert (t.view(np.int32) == np.array([_tanh_seen[x] for x in pre[:, 0].ravel().tolist()], dtype=np.int32)).all(), what


def _head_operands(c):
    return _f32(c["w"]).contiguous().cuda(), _f32(c["b"]).cuda()


def _head_slab(buf, nb, Co, C):
    return buf.back().view(nb, Co, pad8(C) + 8)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("N,HW", R.HEAD_BN_SHAPES)
def test_head_bn_trio_exact(mau, N, HW, dt):
    """head_bn_fwd, head_bn_bwd_reduce, head_bn_bwd_apply: every Co (one template instantiation each), tanh0 0 and 1, an image
    boundary inside a 32-pixel step (35), inside the four-pixel iteration (300) and at a block edge (1061), images of exactly one step."""
    npix, nb, code, st = N * HW, -(-N * HW // R.BLOCK), _code(dt), _stream()
    for Co, C, tanh0 in itertools.product(R.HEAD_CO, R.HEAD_BN_C, (0, 1)):
        c = R.exact_head_case(N, HW, C, Co)
        k, C8, (w, b) = _coefs(c["k"]), pad8(C), _head_operands(c)
        a = R.bn_relu_apply(c["y"], c["k"]["scale"], c["k"]["shift"], dt)
        hb = R.HeadBwd(a, c["w"], c["out"], c["dout"], tanh0)
        B = R.BnBwd(R.round_t(hb.da_pre, dt), c["y"], c["k"], R.HEAD_EXACT_COUNT)
        outb, doutb = _rows(c["out"].reshape(N * Co, HW)), _rows(c["dout"].reshape(N * Co, HW))
        for ld, ldslab in ((C8, C), (C8 + 16, 72)):
            what = (N, HW, Co, C, tanh0, ld)
            yb = _src(c["y"], ld, dt)
            res = Buf(N * Co, HW, torch.float32).cuda()
            _call("mau_head_bn_fwd", yb.ptr, ld, *_kp(k, "scale", "shift"), w.data_ptr(), b.data_ptr(), res.ptr, tanh0, code, N, HW, C, Co, st)
            _check_out(res.back().view(N, Co, HW), R.head_pre(a, c["w"], c["b"], N, HW), tanh0, ("head_bn_fwd",) + what)
            slab, hslab = Buf(2 * nb, ldslab, torch.float32).cuda(), Buf(nb, Co * (C8 + 8), torch.float32).cuda()
            _call("mau_head_bn_bwd_reduce", yb.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), w.data_ptr(), outb.ptr, doutb.ptr, slab.ptr, ldslab,
                  hslab.ptr, tanh0, code, N, HW, C, Co, st)
            assert same_bits(_bn_slab(slab, nb, C, ldslab, min(ldslab, 64)), _f32(B.slab)), ("BatchNorm slab",) + what
            assert same_bits(_head_slab(hslab, nb, Co, C), _f32(hb.slab(C)), nan_matches_nan=True), ("dW, db",) + what
            sums, got = _sums(B), []
            for count in (B.count, 0.0):
                dyb = Buf(npix, ld + 8, dt).cuda()
                _call("mau_head_bn_bwd_apply", yb.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), sums.data_ptr(), count, w.data_ptr(), outb.ptr,
                      doutb.ptr, dyb.ptr, ld + 8, tanh0, code, N, HW, C, Co, st)
                got.append(_read(dyb, C))
            assert same_bits(got[0], _want(B.dy, dt)), ("dy",) + what
            assert same_bits(got[1], got[0]), ("dy, count in the sums",) + what


def _head_mean(ab, ld, w, b, N, HW, C, Co, tanh0, dt, scale=None, shift=None):
    from mau_amd import functional as F_
    from mau_amd._lib import lib
    n = lib.mau_head_mean_ws_elems(N, HW, Co)
    assert n == N * -(-HW // 1024) * Co
    ws = torch.full((n + 8,), float("nan"), dtype=torch.float64, device="cuda")
    means = torch.full((N * Co + 8,), float("nan"), dtype=torch.float64, device="cuda")
    tk = F_._tickets(torch.device("cuda"))
    _call("mau_head_mean", ab.ptr, ld, w.data_ptr(), b.data_ptr(), None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(),
          means.data_ptr(), ws.data_ptr(), tk.data_ptr(), tanh0, _code(dt), N, HW, C, Co, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n:]).all()) and bool(torch.isnan(means[N * Co:]).all()) and int(tk.abs().sum()) == 0
    return means[:N * Co].cpu().view(N, Co)


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("N,HW", R.HEAD_SHAPES)
def test_head_fwd_bwd_mean_exact(mau, N, HW, dt):
    """head_fwd on its fast path (C <= 64, HW >= 32) and its general one (wider heads: weights from memory; (4, 12): images shorter
    than a step), head_bwd with a second 64-channel group, head_mean against the float64 mean of the same exact map -- and, one pixel
    per sample, against head_fwd's value of every pixel."""
    npix, nb, code, st = N * HW, -(-N * HW // R.BLOCK), _code(dt), _stream()
    for Co, C, tanh0 in itertools.product(R.HEAD_CO, R.HEAD_C, (0, 1)):
        c = R.exact_head_case(N, HW, C, Co)
        C8, (w, b) = pad8(C), _head_operands(c)
        pre = R.head_pre(c["a"], c["w"], c["b"], N, HW)
        hb = R.HeadBwd(c["a"], c["w"], c["out"], c["dout"], tanh0)
        outb, doutb = _rows(c["out"].reshape(N * Co, HW)), _rows(c["dout"].reshape(N * Co, HW))
        for ld in (C8, C8 + 16):
            what = (N, HW, Co, C, tanh0, ld)
            ab = _src(c["a"], ld, dt)
            res = Buf(N * Co, HW, torch.float32).cuda()
            _call("mau_head_fwd", ab.ptr, ld, w.data_ptr(), b.data_ptr(), res.ptr, tanh0, code, N, HW, C, Co, st)
            out = res.back().view(N, Co, HW)
            _check_out(out, pre, tanh0, ("head_fwd",) + what)
            dab, hslab = Buf(npix, ld + 8, dt).cuda(), Buf(nb, Co * (C8 + 8), torch.float32).cuda()
            _call("mau_head_bwd", ab.ptr, ld, w.data_ptr(), outb.ptr, doutb.ptr, dab.ptr, ld + 8, hslab.ptr, tanh0, code, N, HW, C, Co, st)
            assert same_bits(_read(dab, C), _want(hb.da_pre, dt)), ("da",) + what
            assert same_bits(_head_slab(hslab, nb, Co, C), _f32(hb.slab(C)), nan_matches_nan=True), ("dW, db",) + what
            # the mean of the map head_fwd wrote (float32 values of one binade range: their float64 sum is exact in any order)
            got = _head_mean(ab, ld, w, b, N, HW, C, Co, tanh0, dt)
            assert torch.equal(got, out.double().sum(-1) / HW), ("head_mean",) + what
            lin = slice(1, None) if tanh0 else slice(None)
            assert torch.equal(got[:, lin], torch.from_numpy(pre[:, lin].sum(-1) / HW)), ("head_mean against float64",) + what
            if tanh0:
                assert float((got[:, 0] - torch.from_numpy(np.tanh(pre[:, 0]).mean(-1))).abs().max()) <= TANH_ULPS * 2.0 ** -24, what
            if ld == C8 and tanh0:
                sc, sh = torch.tensor([2.0, 0.5, 1.0, 4.0][:Co], dtype=torch.float64).cuda(), torch.tensor([0.5, -1.0, 0.0, 3.0][:Co], dtype=torch.float64).cuda()
                n1 = min(npix, 160)                          # one pixel per sample: head_mean's per-pixel values, bit for bit
                px = _head_mean(ab, ld, w, b, n1, 1, C, Co, tanh0, dt, sc, sh)
                assert torch.equal(px, out.permute(0, 2, 1).reshape(npix, Co)[:n1].double() * sc.cpu() + sh.cpu()), ("head_mean per pixel",) + what


# ---- one random case per kernel ---------------------------------------------------------------------------------------------------------
def _within(got, ref, bound, what, leave_out=None):
    err = np.abs(got.double().numpy() - ref)
    bad = err > bound
    if leave_out is not None:
        share = float(leave_out.mean())
        print(f"{what}: {share:.5%} of the elements left out (mask may flip)")
        assert share < 1e-3, (what, share)
        bad &= ~leave_out
    ratio = float((err / np.maximum(bound, 1e-300))[~leave_out if leave_out is not None else slice(None)].max())
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    assert not bad.any(), (what, int(bad.sum()), ratio)


def _dy_bound(B, y, k, dt, da_slack=0.0):
    """fp32: the k0 / k1 form's bound; 16-bit: one ulp of the type around the float64 value (+ ``da_slack``, see the head's case)"""
    return R.dy_bound_f32(B, y, k) if dt == torch.float32 else R.type_ulp(B.dy, dt) + da_slack


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
def test_bn_and_pool_bwd_random(mau, dt):
    """randn data, C = 70, 2112 pixels: bn_relu_bwd_reduce / apply, then bn_relu_apply_pool and pool_bn_bwd_reduce / apply (pool + skip)"""
    N, H, W = R.RANDOM_POOL
    npix, C, nb, code, st = N * H * W, R.RANDOM_C, -(-N * H * W // R.BLOCK), _code(dt), _stream()
    C8 = pad8(C)
    ld = C8 + 16
    c = R.random_case(npix, C, 0, dt, ("dskip", "dpl"))
    kk = R.random_coefs(C, 0)
    k = _coefs(kk)
    B = R.BnBwd(c["da"], c["y"], kk)
    out = R.mask_uncertain(B, c["y"], kk)
    dab, yb = _src(c["da"], ld, dt), _src(c["y"], ld, dt)
    slab = Buf(2 * nb, C, torch.float32).cuda()
    _call("mau_bn_relu_bwd_reduce", dab.ptr, ld, yb.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), slab.ptr, C, code, npix, C, st)
    assert not out.any()                                      # (the sums' bound presumes that no pixel's mask is in doubt)
    _within(_bn_slab(slab, nb, C, C, C), B.slab, np.stack([R.slab_bound(B.add1), R.slab_bound(B.add2)], 1), f"bn_relu_bwd_reduce {dt}")
    dyb = Buf(npix, ld, dt).cuda()
    _call("mau_bn_relu_bwd_apply", dab.ptr, ld, yb.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), _sums(B).data_ptr(), float(npix), dyb.ptr, ld, code,
          npix, C, st)
    _within(_read(dyb, C), B.dy, _dy_bound(B, c["y"], kk, dt), f"bn_relu_bwd_apply {dt}", out)
    # the pool: the first maximum is defined on the activations the kernel stored; those against float64 within an ulp of the type
    a, pooled, bits, arg_dev = _apply_pool(yb, ld, k, N, H, W, C, dt)
    a64 = np.maximum(kk["scale"] * c["y"] + kk["shift"], 0)
    tol = 4 * 2.0 ** -24 * (np.abs(kk["scale"] * c["y"]) + np.abs(kk["shift"])) if dt == torch.float32 else R.type_ulp(a64, dt)
    _within(a, a64, tol, f"bn_relu_apply_pool a {dt}")
    pooled_ref, arg = R.pool_first_max(a.double().numpy(), N, H, W)
    assert same_bits(pooled, _f32(pooled_ref)) and torch.equal(bits, torch.from_numpy(R.pack_argidx(arg).astype(np.int64)))
    nwin = N * (H // 2) * (W // 2)
    da = R.round_t(R.pool_da_pre(c["dpl"][:nwin], arg, c["dskip"], N, H, W), dt)
    B = R.BnBwd(da, c["y"], kk)
    out = R.mask_uncertain(B, c["y"], kk)
    assert not out.any()
    _pool_bwd(yb, ld, k, arg_dev, c["dpl"][:nwin], c["dskip"], B, N, H, W, C, dt,
              lambda g: _within(g, B.slab, np.stack([R.slab_bound(B.add1), R.slab_bound(B.add2)], 1), f"pool_bn_bwd_reduce {dt}"),
              lambda g: _within(g, B.dy, _dy_bound(B, c["y"], kk, dt), f"pool_bn_bwd_apply {dt}", out))


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
def test_head_random(mau, dt):
    """randn data, 2112 pixels: the plain head at C = 70 (general path, two channel groups in head_bwd) and the BatchNorm-fused trio at
    C = 64, Co = 2, tanh on channel 0.  The activation inside the fused kernels is the float32 FMA's value rounded to the type: the
    reference forms it the same way (float64 product and sum, rounded to float32, then to the type).  Where the float64 W^T dz lies
    within its fp32 accumulation error of a rounding boundary of the type, the kernel's da may be the neighbouring value: dy gets
    |scale| times that step as slack there, and only there."""
    N, HW = R.RANDOM_HEAD
    npix, nb, Co, code, st = N * HW, -(-N * HW // R.BLOCK), 2, _code(dt), _stream()
    for C, fused in ((R.RANDOM_C, False), (R.RANDOM_HEAD_C, True)):
        C8 = pad8(C)
        ld = C8 + 16
        r = R._rng(7, C)
        c = R.random_case(npix, C, 1, dt)
        kk = R.random_coefs(C, 1)
        k = _coefs(kk)
        f = lambda v: v.astype(np.float32).astype(np.float64)      # noqa: E731
        wv, bv, dout = f(r.standard_normal((Co, C)) / 8), f(r.standard_normal(Co)), f(r.standard_normal((N, Co, HW)))
        w, b = _f32(wv).contiguous().cuda(), _f32(bv).cuda()
        a = R.round_t(f(np.maximum(kk["scale"] * c["y"] + kk["shift"], 0)), dt) if fused else c["da"]
        pre = R.head_pre(a, wv, bv, N, HW)
        out64 = R.head_fwd(a, wv, bv, N, HW, 1)
        src = _src(c["y"] if fused else a, ld, dt)
        res = Buf(N * Co, HW, torch.float32).cuda()
        if fused:
            _call("mau_head_bn_fwd", src.ptr, ld, *_kp(k, "scale", "shift"), w.data_ptr(), b.data_ptr(), res.ptr, 1, code, N, HW, C, Co, st)
        else:
            _call("mau_head_fwd", src.ptr, ld, w.data_ptr(), b.data_ptr(), res.ptr, 1, code, N, HW, C, Co, st)
        terms = (np.abs(a) @ np.abs(wv).T + np.abs(bv)).reshape(N, HW, Co).transpose(0, 2, 1)
        bound = 2.0 ** -24 * (C + 2) * terms                       # C FMAs, the butterfly's adds, the bias
        bound[:, 0] += (TANH_ULPS + 1) * 2.0 ** -24                # tanh' <= 1; tanhf's own error and the final rounding
        _within(res.back().view(N, Co, HW), out64, bound, f"head{'_bn' if fused else ''}_fwd {dt}")
        outv = f(out64)
        hb = R.HeadBwd(a, wv, outv, dout, 1)
        outb, doutb = _rows(outv.reshape(N * Co, HW)), _rows(dout.reshape(N * Co, HW))
        e_da = 2.0 ** -24 * (Co + 3) * (np.abs(hb.dz) @ np.abs(wv))
        hslab = Buf(nb, Co * (C8 + 8), torch.float32).cuda()
        hbound = np.full((nb, Co, C8 + 8), np.inf)
        hbound[:, :, :C], hbound[:, :, C:C8], hbound[:, :, C8] = R.slab_bound(hb.addw) + 2.0 ** -22 * R.block_sums(np.abs(hb.addw)), 0.0, \
            R.slab_bound(hb.dz) + 2.0 ** -22 * R.block_sums(np.abs(hb.dz))                     # (+ dz's own roundings: 1 - t^2, the product)
        if not fused:
            dab = Buf(npix, ld, dt).cuda()
            _call("mau_head_bwd", src.ptr, ld, w.data_ptr(), outb.ptr, doutb.ptr, dab.ptr, ld, hslab.ptr, 1, code, N, HW, C, Co, st)
            _within(_read(dab, C), hb.da_pre, e_da + (0 if dt == torch.float32 else R.type_ulp(hb.da_pre, dt)), f"head_bwd da {dt}")
            got = _head_slab(hslab, nb, Co, C)
            assert bool(torch.isnan(got[:, :, C8 + 1:]).all())
            _within(got[:, :, :C8 + 1], np.nan_to_num(hb.slab(C))[:, :, :C8 + 1], hbound[:, :, :C8 + 1], f"head_bwd dW, db {dt}")
            continue
        da = R.round_t(hb.da_pre, dt)
        if dt == torch.float32:                                # da is the fp32 sum itself
            tie, step = np.zeros(da.shape, dtype=bool), e_da
        else:                                                  # da is the float64 value's rounding, or, at a boundary, its neighbour
            tie = R.round_t(hb.da_pre - e_da, dt) != R.round_t(hb.da_pre + e_da, dt)
            step = np.where(tie, R.type_ulp(da, dt), 0.0)
        B = R.BnBwd(da, c["y"], kk)
        out = R.mask_uncertain(B, c["y"], kk)
        assert not out.any()
        slab = Buf(2 * nb, C, torch.float32).cuda()
        _call("mau_head_bn_bwd_reduce", src.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), w.data_ptr(), outb.ptr, doutb.ptr, slab.ptr, C, hslab.ptr, 1,
              code, N, HW, C, Co, st)
        e1 = R.block_sums(step)
        _within(_bn_slab(slab, nb, C, C, C), B.slab, np.stack([R.slab_bound(B.add1) + e1, R.slab_bound(B.add2) + e1 * np.abs(B.xhat).max(0)], 1),
                f"head_bn_bwd_reduce BatchNorm sums {dt}")
        got = _head_slab(hslab, nb, Co, C)
        assert bool(torch.isnan(got[:, :, C8 + 1:]).all())
        _within(got[:, :, :C8 + 1], np.nan_to_num(hb.slab(C))[:, :, :C8 + 1], hbound[:, :, :C8 + 1], f"head_bn_bwd_reduce dW, db {dt}")
        dyb = Buf(npix, ld, dt).cuda()
        _call("mau_head_bn_bwd_apply", src.ptr, ld, *_kp(k, "scale", "shift", "mean", "invstd"), _sums(B).data_ptr(), float(npix), w.data_ptr(), outb.ptr,
              doutb.ptr, dyb.ptr, ld, 1, code, N, HW, C, Co, st)
        slack = np.abs(kk["scale"]) * step
        print(f"head_bn_bwd_apply {dt}: {float(tie.mean()):.5%} of da within fp32 error of a rounding boundary")
        bound = R.dy_bound_f32(B, c["y"], kk) + slack if dt == torch.float32 else R.type_ulp(B.dy, dt) + slack
        _within(_read(dyb, C), B.dy, bound, f"head_bn_bwd_apply {dt}", out)
