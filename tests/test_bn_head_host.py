"""CPU-only checks around the BatchNorm-backward and head kernels (csrc/bn.hip, csrc/bn_fused.hip, csrc/head.hip): the references of
tests/bn_head_ref.py against torch float64 autograd (an oracle that is wrong proves nothing on the GPU), the proof that every
generated "exact" case is exact in float32 -- which is what lets tests/test_gpu_bn_head.py demand equality -- the mask-flip share of
the random cases, and the launchers' refusals.  No kernel is launched here."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import bn_head_ref as R

F64 = np.float64


@pytest.fixture(scope="module")
def lib():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    return _lib


# ---- the reference against torch float64 autograd -------------------------------------------------------------------------------
def _close(got, want, what):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-12, (what, err)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


@pytest.mark.parametrize("composition", ["relu", "pool+skip", "head"])
def test_reference_against_torch_autograd(composition):
    """BatchNorm2d(train) -> ReLU, then a MaxPool2d(2, 2) reader next to a skip reader, or a 1x1 Conv2d with tanh on channel 0: dy,
    dgamma, dbeta (and dW, db) of the reference equal torch's float64 autograd to 1e-12 relative.  More than one 1024-pixel block,
    odd sizes."""
    N, Cc, H, W, Co = 2, 5, 25, 23, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cc, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    bn = torch.nn.BatchNorm2d(Cc).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Cc, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(Cc, generator=g, dtype=torch.float64))
    a = torch.relu(bn(x))
    xs = _nhwc(x)
    mean, var = xs.mean(0), xs.var(0)
    invstd = 1.0 / np.sqrt(var + bn.eps)
    scale = bn.weight.detach().numpy() * invstd
    k = {"scale": scale, "shift": bn.bias.detach().numpy() - mean * scale, "mean": mean, "invstd": invstd}
    a_ref = R.bn_relu_apply(xs, k["scale"], k["shift"], None)
    _close(a_ref, _nhwc(a), "a")
    if composition == "relu":
        ga = torch.randn(a.shape, dtype=torch.float64, generator=g)
        (a * ga).sum().backward()
        da = _nhwc(ga)
    elif composition == "pool+skip":
        p = torch.nn.functional.max_pool2d(a, 2, 2)
        gp, gs = torch.randn(p.shape, dtype=torch.float64, generator=g), torch.randn(a.shape, dtype=torch.float64, generator=g)
        ((p * gp).sum() + (a * gs).sum()).backward()
        pooled, arg = R.pool_first_max(a_ref, N, H, W)
        _close(pooled, _nhwc(p), "pooled")
        da = R.pool_da_pre(_nhwc(gp), arg, _nhwc(gs), N, H, W)
        assert (da.reshape(N, H, W, Cc)[:, 2 * (H // 2):] == _nhwc(gs).reshape(N, H, W, Cc)[:, 2 * (H // 2):]).all()
    else:
        conv = torch.nn.Conv2d(Cc, Co, 1).double()
        o = conv(a)
        o = torch.cat([torch.tanh(o[:, :1]), o[:, 1:]], 1)
        go = torch.randn(o.shape, dtype=torch.float64, generator=g)
        (o * go).sum().backward()
        w, b = conv.weight.detach().numpy().reshape(Co, Cc), conv.bias.detach().numpy()
        out = R.head_fwd(a_ref, w, b, N, H * W, 1)
        _close(out, o.detach().reshape(N, Co, H * W).numpy(), "out")
        hb = R.HeadBwd(a_ref, w, out, go.reshape(N, Co, H * W).numpy(), 1)
        assert hb.dW.shape[0] == -(-N * H * W // R.BLOCK) == 2
        _close(hb.dW.sum(0), conv.weight.grad.numpy().reshape(Co, Cc), "dW")
        _close(hb.db.sum(0), conv.bias.grad.numpy(), "db")
        s = hb.slab(Cc)
        assert np.isnan(s[:, :, R.pad8(Cc) + 1:]).all() and (s[:, :, Cc:R.pad8(Cc)] == 0).all() and (s[:, :, R.pad8(Cc)] == hb.db).all()
        da = hb.da_pre
    B = R.BnBwd(da, xs, k)
    assert B.slab.shape == (2, 2, Cc)
    _close(B.slab.sum(0), B.sums.reshape(2, Cc), "slab")
    _close(B.dy, _nhwc(x.grad), "dy")
    _close(B.sums[Cc:], bn.weight.grad.numpy(), "dgamma")
    _close(B.sums[:Cc], bn.bias.grad.numpy(), "dbeta")


def test_first_maximum_and_argidx_packing():
    """a window of equal values names position 0, a later maximum wins only when strictly greater; 2 bits per channel, channel j of a
    vector at bits [2j, 2j+2); against torch's max_pool2d with return_indices on a tie-heavy input"""
    a = np.array([[1, 1], [1, 1], [1, 2], [2, 2]], dtype=F64).reshape(1, 2, 2, 2).reshape(4, 2)         # pixels (0,0) (0,1) (1,0) (1,1)
    pooled, arg = R.pool_first_max(a, 1, 2, 2)
    assert pooled.tolist() == [[2, 2]] and arg.tolist() == [[3, 2]]
    assert R.pack_argidx(np.array([[3, 1, 0, 2, 0, 0, 0, 1, 2]])).tolist() == [[3 | 1 << 2 | 2 << 6 | 1 << 14, 2]]
    N, H, W, Cc = 2, 5, 7, 3
    x = torch.randint(0, 3, (N, Cc, H, W), generator=torch.Generator().manual_seed(1)).double()
    p, idx = torch.nn.functional.max_pool2d(x, 2, 2, return_indices=True)
    pooled, arg = R.pool_first_max(_nhwc(x), N, H, W)
    yy, xx = idx // W, idx % W
    assert (_nhwc(p) == pooled).all() and (_nhwc((yy % 2) * 2 + xx % 2) == arg).all()


# ---- every generated exact case is exact --------------------------------------------------------------------------------------
def _assert_exact_sums(addends, what):
    """The block sums of these addends in float32 equal the float64 sums in ANY order: every addend is a multiple of one power of
    two g, and sum |addend| of a block stays below 2^24 g, so every partial sum is a float32.  Checked too, as the issue words it: the
    sums evaluated in float32 in forward and in reversed pixel order equal the float64 sums bit for bit."""
    a = addends.reshape(addends.shape[0], -1)
    assert R.is_f32(a), what
    k = next(k for k in range(0, 60) if (np.ldexp(a, k) == np.round(np.ldexp(a, k))).all())
    assert np.ldexp(R.block_sums(np.abs(a)), k).max() < 2 ** 24, (what, k)
    want = R.block_sums(a)
    for b, p0 in enumerate(range(0, a.shape[0], R.BLOCK)):
        blk = a[p0:p0 + R.BLOCK].astype(np.float32)
        for order in (blk, blk[::-1]):
            s = np.cumsum(order, axis=0, dtype=np.float32)[-1]
            assert s.dtype == np.float32 and (s.astype(F64) == want[b]).all(), (what, b)


def _assert_exact_bn(da, y, k, what, count=R.EXACT_COUNT):
    """sums, means and every intermediate of dy = sc*dz - (k1*y + k0), k1 = sc*m2*is, k0 = sc*m1 - k1*mu are float32 values"""
    assert R.is_f32(k["scale"] * y + k["shift"]), what
    B = R.BnBwd(da, y, k, count)
    _assert_exact_sums(B.add1, what + " dz")
    _assert_exact_sums(B.add2, what + " dz*xhat")
    k1 = k["scale"] * B.m2 * k["invstd"]
    k1mu = k1 * k["mean"]
    k0 = k["scale"] * B.m1 - k1mu
    inner = k1 * y + k0
    for name, v in (("xhat", B.xhat), ("m1", B.m1), ("m2", B.m2), ("k1", k1), ("k1*mu", k1mu), ("k0", k0), ("k1*y+k0", inner), ("dy", B.dy)):
        assert R.is_f32(v), (what, name)
    assert (B.dy == k["scale"] * B.dz - inner).all(), what
    return B


def test_exact_bn_cases_are_exact():
    zero_act = []
    for npix, Cc in list(itertools.product(R.BN_NPIX, R.BN_C)) + R.BN_WIDE:
        c = R.exact_bn_case(npix, Cc)
        B = _assert_exact_bn(c["da"], c["y"], c["k"], f"bn {npix}x{Cc}")
        zero_act.append((B.act == 0).mean())
    assert np.mean(zero_act) > 0.03, np.mean(zero_act)          # the strict `> 0` of the mask is exercised


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
def test_exact_pool_cases_are_exact(dt):
    tied = []
    for (N, H, W), Cc in itertools.product(R.POOL_SHAPES, R.POOL_C):
        c = R.exact_pool_case(N, H, W, Cc)
        pre = np.maximum(c["k"]["scale"] * c["y"] + c["k"]["shift"], 0)
        a = R.round_t(pre, dt)
        assert R.is_f32(pre) and (a == pre).all()
        pooled, arg = R.pool_first_max(a, N, H, W)
        win = R._windows(a, N, H, W)
        tied.append(((win == win.max(0)).sum(0) > 1).mean())
        for dpl, dskip in ((c["dpl"], c["dskip"]), (c["dpl"], None), (None, c["dskip"])):
            pre = R.pool_da_pre(dpl, arg, dskip, N, H, W)
            assert R.is_f32(pre)
            _assert_exact_bn(R.round_t(pre, dt), c["y"], c["k"], f"pool {(N, H, W, Cc)}")
    assert np.mean(tied) > 0.3, np.mean(tied)                   # windows with several maxima are frequent


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
def test_exact_head_cases_are_exact(dt):
    for (N, HW), Co, tanh0 in itertools.product(R.HEAD_SHAPES, R.HEAD_CO, (0, 1)):
        for Cc in sorted(set(R.HEAD_C + R.HEAD_BN_C)):
            c = R.exact_head_case(N, HW, Cc, Co)
            what = f"head {(N, HW, Cc, Co, tanh0)}"
            inputs = [("a", c["a"])] if Cc in R.HEAD_C else []
            if Cc in R.HEAD_BN_C and (N, HW) in R.HEAD_BN_SHAPES:
                pre = np.maximum(c["k"]["scale"] * c["y"] + c["k"]["shift"], 0)
                assert R.is_f32(pre)
                inputs.append(("bn", R.round_t(pre, dt)))
            for kind, a in inputs:
                assert (R.round_t(a, dt) == a).all(), what                        # the activation is a value of the tensor type
                pre = R.head_pre(a, c["w"], c["b"], N, HW)
                terms = np.concatenate([a[:, None, :] * c["w"][None], np.broadcast_to(c["b"][None, :, None], (N * HW, Co, 1))], -1)
                kk = next(k for k in range(60) if (np.ldexp(terms, k) == np.round(np.ldexp(terms, k))).all())
                assert np.ldexp(np.abs(terms).sum(-1), kk).max() < 2 ** 24 and R.is_f32(pre), what     # the sum over channels, any order
                hb = R.HeadBwd(a, c["w"], c["out"], c["dout"], tanh0)
                assert R.is_f32(hb.dz) and R.is_f32(hb.da_pre), what
                _assert_exact_sums(hb.addw, what + " dW")
                _assert_exact_sums(hb.dz, what + " db")
                if kind == "bn":
                    _assert_exact_bn(R.round_t(hb.da_pre, dt), c["y"], c["k"], what, R.HEAD_EXACT_COUNT)


# ---- the random cases: how many elements the mask-flip rule leaves out ---------------------------------------------------------------
def test_random_cases_leave_out_fewer_than_one_in_a_thousand():
    """|scale*y+shift| within the fp32 dy bound of 0: with randn inputs and the generators' seeds, for the reference alone"""
    for dt in R.DTYPES:
        N, H, W = R.RANDOM_POOL
        npix = N * H * W
        c = R.random_case(npix, R.RANDOM_C, 0, dt)
        k = R.random_coefs(R.RANDOM_C, 0)
        B = R.BnBwd(c["da"], c["y"], k)
        share = R.mask_uncertain(B, c["y"], k).mean()
        print(f"bn/pool random case {dt}: {share:.5%} of the elements left out")
        assert share < 1e-3
        N, HW = R.RANDOM_HEAD
        c = R.random_case(N * HW, R.RANDOM_HEAD_C, 1, dt)
        k = R.random_coefs(R.RANDOM_HEAD_C, 1)
        B = R.BnBwd(c["da"], c["y"], k)
        share = R.mask_uncertain(B, c["y"], k).mean()
        print(f"head random case {dt}: {share:.5%} of the elements left out")
        assert share < 1e-3


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def _signatures(p, F32):
    """{entry point: ordered {argument: a valid value}}; C = 20 (C8 = 24), 2 x 8 x 8 pixels, HW = 64"""
    bn = dict(scale=p, shift=p, mean=p, invstd=p)
    dims = dict(dtype=F32, N=2, H=8, W=8, C=20)
    head = dict(tanh0=1, dtype=F32, N=2, HW=64, C=20, Co=2)
    return {
        "bn_relu_bwd_reduce": dict(da=p, ldda=24, y=p, ldy=24, **bn, slab=p, ldslab=20, dtype=F32, npix=128, C=20, stream=None),
        "bn_relu_bwd_apply": dict(da=p, ldda=24, y=p, ldy=24, **bn, sums=p, count=128.0, dy=p, lddy=24, dtype=F32, npix=128, C=20, stream=None),
        "bn_relu_apply_pool": dict(y=p, ldy=24, scale=p, shift=p, a=p, lda=24, pooled=p, ldp=24, argidx=p, **dims, stream=None),
        "pool_bn_bwd_reduce": dict(y=p, ldy=24, dpl=p, lddpl=24, argidx=p, dskip=p, lddskip=24, **bn, slab=p, ldslab=20, **dims, stream=None),
        "pool_bn_bwd_apply": dict(y=p, ldy=24, dpl=p, lddpl=24, argidx=p, dskip=p, lddskip=24, **bn, sums=p, count=128.0, dy=p, lddy=24, **dims, stream=None),
        "head_bn_fwd": dict(y=p, ldy=24, scale=p, shift=p, w=p, b=p, out=p, **head, stream=None),
        "head_bn_bwd_reduce": dict(y=p, ldy=24, **bn, w=p, out=p, dout=p, bn_slab=p, ldslab=20, head_slab=p, **head, stream=None),
        "head_bn_bwd_apply": dict(y=p, ldy=24, **bn, sums=p, count=128.0, w=p, out=p, dout=p, dy=p, lddy=24, **head, stream=None),
        "head_fwd": dict(a=p, lda=24, w=p, b=p, out=p, **head, stream=None),
        "head_bwd": dict(a=p, lda=24, w=p, out=p, dout=p, da=p, ldda=24, slab=p, **head, stream=None),
        "head_mean": dict(a=p, lda=24, w=p, b=p, scale=None, shift=None, means=p, ws=p, tickets=p, **head, stream=None),
    }


# pointers that may be null, per entry point (either gradient of the pool pair, but not both; the optional outputs)
_OPTIONAL = {"bn_relu_apply_pool": {"argidx"}, "pool_bn_bwd_reduce": {"dpl", "dskip"}, "pool_bn_bwd_apply": {"dpl", "dskip"},
             "head_mean": {"scale", "shift"}}


def test_bn_and_head_entry_points_refuse_bad_arguments(lib):
    """Refused on the host, before any launch (the pointers are never dereferenced), with the entry point's own message in
    mau_last_error: null pointers, ld % 8 != 0, ld < C8, ldslab < C, Co outside [1, 4], C above mau_head_bn_max_channels(), HW < 32 for
    the head_bn trio, H < 2 / W < 2 for the pool entries."""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    L = lib.lib
    sigs = _signatures(p, lib.MAU_F32)
    assert L.mau_head_bn_max_channels() == 64
    n = 0

    def refused(name, why, **changed):
        nonlocal n
        args = dict(sigs[name], **changed)
        assert len(args) == len(lib.PROTOTYPES["mau_" + name][1]), name
        status = getattr(L, "mau_" + name)(*args.values())
        msg = L.mau_last_error()
        assert status == 1 and (name + ": ").encode() in msg and b"_kernel" not in msg, (name, why, changed, status, msg)
        n += 1

    for name, sig in sigs.items():
        for arg, v in sig.items():
            if v == p and arg not in _OPTIONAL.get(name, ()):
                refused(name, "null pointer", **{arg: None})
            if arg.startswith("ld") and arg != "ldslab":
                refused(name, "ld % 8 != 0", **{arg: 28})
                refused(name, "ld < C8", **{arg: 16})
        if "ldslab" in sig:
            refused(name, "ldslab < C", ldslab=19)
        if "Co" in sig:
            refused(name, "Co = 0", Co=0)
            refused(name, "Co = 5", Co=5)
        if name.startswith("head_bn"):
            refused(name, "C > 64", C=65, **{a: 72 for a in sig if a.startswith("ld")})
            refused(name, "HW < 32", HW=31)
        if "H" in sig:
            refused(name, "H < 2", H=1)
            refused(name, "W < 2", W=1)
    for name in ("pool_bn_bwd_reduce", "pool_bn_bwd_apply"):
        refused(name, "neither gradient", dpl=None, dskip=None)
        refused(name, "pooled gradient without argidx", argidx=None)
    print(f"{n} refusals")
