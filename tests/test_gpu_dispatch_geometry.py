"""GPU tests at the layer shapes where the 16-bit convolution's statistics slab was sized for one tiling and written by another:
64 output channels, more than 192 input channels, an ODD number of 32-row tiles in the image height (the U-Net++'s full-resolution
nodes at 224 x 224, for one).  tests/test_dispatch_geometry_host.py proves on the host that the size query and the launch agree for
every layer; here the launch itself is checked at such shapes, in the default environment: exact-integer outputs and statistics
through the C ABI, a slab with sentinel rows behind the queried count (an overrun shows without leaving the allocation), and one
conv-bn-relu training step at module level against float64."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from tests._helpers import mau, rel_l2  # noqa: F401

pytestmark = pytest.mark.gpu


def _to_act(x_nchw, dt):
    from mau_amd import functional as F_
    return F_.Act(F_.ToNHWC.apply(x_nchw.cuda(), dt), x_nchw.shape[1])


def _sparse_int_case(seed, N, Cin, Cout, H, W):
    """x uniform in {-1, 0, 1}, w in {-1, 0, 1} with one entry in eight non-zero, bias in -4..4: |y| stays below 128 at K up to
    9 * 320 (asserted by the callers), so y is exact in both 16-bit types, y^2 < 2^14 and the sum of y^2 over the 1024 pixels of a
    64 x 16 tile stays below 2^24: every fp32 partial the kernel can form -- whatever the tiling -- is an exact integer."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (N, Cin, H, W), generator=g).float()
    w = (torch.randint(0, 2, (Cout, Cin, 3, 3), generator=g) * 2 - 1).float() * (torch.randint(0, 8, (Cout, Cin, 3, 3), generator=g) == 0).float()
    b = torch.randint(-4, 5, (Cout,), generator=g).float()
    return x, w, b


@functools.lru_cache(maxsize=2)
def _fwd_case(shape):
    """(inputs, float64 reference) of one forward case; shared by the bf16 and the fp16 run of the shape."""
    N, C0, C1, Cout, H, W, E = shape
    x, w, b = _sparse_int_case(sum(shape) + 5, N, C0 + C1 + E, Cout, H, W)
    if E:               # the embedding channels are constant over the image (and zero in the padding halo, like every other channel)
        x[:, C0 + C1:] = x[:, C0 + C1:, :1, :1].clone()
    ref = TF.conv2d(x.double(), w.double(), b.double(), padding=1)
    return x, w, b, ref


# (N, C0, C1, Cout, H, W, E): one tensor source through mau_conv3x3_fwd (C1 = E = 0), two sources + a broadcast embedding through
# mau_conv3x3_fwd2; with each, the variant the launch must take on the 256-CU device (tile rows, waves, cout block)
FWD_CASES = [
    ((5, 256, 0, 64, 224, 128, 0), (32, 4, 64)),        # 16 stages, even: the 16x16x32 stage-pair loop
    ((13, 208, 0, 64, 65, 128, 0), (32, 4, 64)),        # 13 stages, odd: the 32x32x16 loop and its epilogue
    ((6, 320, 0, 64, 96, 256, 0), (32, 4, 64)),         # wider K, short image
    ((5, 200, 0, 64, 224, 128, 0), (32, 4, 64)),        # Cin not a multiple of 16: the loader without buffer addressing
    ((4, 64, 128, 64, 224, 128, 32), (32, 8, 64)),      # two sources + embedding, 224 input channels; N = 4 leaves the 64-row tile
                                                        # behind <64,2,8> in the grid-fill score: the 8-wave-row slab of 32-row tiles
    ((5, 64, 128, 64, 224, 128, 32), (32, 4, 64)),      # the same layer at N = 5: the 64-row tile wins the score, the slab rule decides
]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,variant", FWD_CASES, ids=["x".join(map(str, c[0])) for c in FWD_CASES])
def test_conv3x3_stats_slab_exact_at_odd_tile_rows(mau, dt, shape, variant):
    """Forward + BatchNorm partial sums, default environment, against conv2d on the CPU in float64: the output bit for bit (after one
    rounding to the 16-bit type), sum(y) and sum(y^2) per channel EQUAL to the reference's (exact-integer data), every queried slab
    row written and every row behind them untouched (the slab is 1.5x over-allocated and NaN-filled)."""
    from mau_amd import functional as F_
    from mau_amd._lib import call, conv3x3_variant, lib
    N, C0, C1, Cout, H, W, E = shape
    Cin = C0 + C1 + E
    code = F_.dtype_code(dt)
    # this IS a layer of the kind the slab rule is about, and the launch takes the variant the rule is meant to give it
    assert Cout == 64 and Cin > 192 and (-(-H // 32)) % 2 == 1
    assert conv3x3_variant(code, N, H, W, Cout, Cin=Cin)[:3] == variant
    if variant == (32, 4, 64):
        # (32, 4, 64) is reached ONLY from the 64-row tile winning the grid-fill score (the loop itself yields 4 waves for 16-row tiles
        # alone): with Cin > 192 the K rule would take <64,4,8> here, whose 8 * ceil(H / 64) rows per tile column exceed the slab's
        assert 8 * -(-H // 64) > 4 * -(-H // 32)
        assert conv3x3_variant(code, N, H, W, Cout, Cin=0)[:3] == (32, 4, 64)
    th, nw, bn = variant
    tiles = lib.mau_conv3x3_num_pixel_tiles(code, N, H, W, Cout)
    assert tiles == (8 if (bn == 64 and nw == 8) else 4) * N * -(-H // th) * -(-W // 16)

    x, w, b, ref = _fwd_case(shape)
    assert float(ref.abs().max()) < 128                      # exactness of everything below rests on this, not on the seed
    s1, s2 = ref.sum(dim=(0, 2, 3)), (ref ** 2).sum(dim=(0, 2, 3))
    assert float(s2.max()) < 2 ** 53

    st = torch.cuda.current_stream().cuda_stream
    wf = F_.pack_conv_weights(w.cuda(), code)[0]
    bd = b.cuda()
    ldy = F_.pad8(Cout)
    y = torch.full((N, H, W, ldy), float("nan"), dtype=dt, device="cuda")
    cpad = (Cout + 63) // 64 * 64
    rows = tiles + tiles // 2 + 8                             # spare rows: an overrun lands inside the allocation, on sentinels
    slab = torch.full((rows, 2 * cpad), float("nan"), dtype=torch.float32, device="cuda")
    if C1 == 0 and E == 0:
        a = _to_act(x, dt)
        call("mau_conv3x3_fwd", a.t.data_ptr(), a.t.shape[-1], C0, None, None, 0, wf.data_ptr(), bd.data_ptr(), None, None, y.data_ptr(),
             ldy, Cout, slab.data_ptr(), code, N, H, W, st)
    else:
        a, a1 = _to_act(x[:, :C0], dt), _to_act(x[:, C0:C0 + C1], dt)
        emb = x[:, C0 + C1:, 0, 0].contiguous().cuda()
        ews = torch.empty((N, E), dtype=dt, device="cuda")
        call("mau_conv3x3_fwd2", a.t.data_ptr(), a.t.shape[-1], C0, a1.t.data_ptr(), a1.t.shape[-1], C1, emb.data_ptr(), ews.data_ptr(), E,
             wf.data_ptr(), bd.data_ptr(), None, None, y.data_ptr(), ldy, Cout, slab.data_ptr(), code, N, H, W, st)
    torch.cuda.synchronize()
    slab = slab.cpu()
    written, spare = slab[:tiles], slab[tiles:]
    assert bool(torch.isnan(spare).all()), f"rows behind the {tiles} queried ones were written: {int((~torch.isnan(spare)).any(1).sum())} of {rows - tiles}"
    assert not bool(torch.isnan(written).any()), f"{int(torch.isnan(written).any(1).sum())} of the {tiles} queried rows were not (fully) written"
    got = F_.to_nchw(F_.Act(y, Cout)).cpu()
    assert torch.equal(got, ref.to(dt).float())
    assert float(y[..., Cout:].float().abs().sum()) == 0.0    # pad channels stay zero
    s = written.double().sum(0)
    assert torch.equal(s[:Cout], s1) and torch.equal(s[cpad:cpad + Cout], s2)


def test_conv_bn_relu_training_step_at_odd_tile_rows(mau):
    """One ``functional.ConvBNReLU`` training forward + backward, 256 -> 64 channels at 5 x 224 x 128 in bf16 (what a VGGBlock half of a
    U-Net++ full-resolution node runs), on the exact-integer data: the slab is allocated by functional.py from the size query and
    reduced by ``mau_bn_stats_finalize_train``, so wrong slab rows show in the batch statistics.

    Statistics against float64 moments of the float64 convolution: the slab sums are exact here, what remains is the finalize's
    rounding -- (float) of the fp64 mean, fp32 1/sqrt -- bounded by rtol 3e-7 exactly as in
    test_bn_stats_finalize_every_length_matches_two_launch_form; the running statistics add (1 - m) * old + m * new in fp32 on top
    (old = 0 and 1: no cancellation, three more roundings of 2^-24 each), inside the same 3e-7.
    Gradients against float64 autograd of conv -> batch_norm -> relu in relative L2, at test_g1_vgg_block's bf16 bound: 2e-2 + 1.5 x
    the error of torch's own CPU bf16 autocast on the same data."""
    from mau_amd import functional as F_
    from mau_amd._lib import conv3x3_variant
    N, Cin, Cout, H, W = 5, 256, 64, 224, 128
    dt = torch.bfloat16
    code = F_.dtype_code(dt)
    assert conv3x3_variant(code, N, H, W, Cout, Cin=Cin)[:3] == (32, 4, 64) and (-(-H // 32)) % 2 == 1
    x, w, b = _sparse_int_case(99, N, Cin, Cout, H, W)
    g = torch.Generator().manual_seed(100)
    gamma = torch.rand(Cout, generator=g) + 0.5
    beta = torch.randn(Cout, generator=g)
    da = torch.randint(-2, 3, (N, Cout, H, W), generator=g).float()
    momentum, eps = 0.1, 1e-5

    def reference(dtype, autocast):
        xr, wr, br, gr, be = (v.clone().to(dtype).requires_grad_(True) for v in (x, w, b, gamma, beta))      # (fresh leaves)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            y = TF.conv2d(xr, wr, br, padding=1)
            a = torch.relu(TF.batch_norm(y, None, None, gr, be, True, momentum, eps))
        a.to(dtype).backward(da.to(dtype))
        return y.detach(), a.detach(), [v.grad for v in (xr, wr, gr, be)]

    y64, a64, grads64 = reference(torch.float64, False)
    assert float(y64.abs().max()) < 128
    _, a_bf, grads_bf = reference(torch.float32, True)
    yard = max([rel_l2(a_bf, a64)] + [rel_l2(p, q) for p, q in zip(grads_bf, grads64)])
    tol = 2e-2 + 1.5 * yard

    xd = x.cuda().requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    gd, bed = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    rmean, rvar = torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    st = F_.BNState(training=True, C0=Cin, momentum=momentum, eps=eps)
    out = F_.ConvBNReLU.apply(F_.ToNHWC.apply(xd, dt), None, None, wd, bd, gd, bed, rmean, rvar, nbt, None, None, st)
    saved = out.grad_fn.saved_tensors
    y_dev, mean, invstd = saved[4], saved[7], saved[8]
    assert torch.equal(F_.to_nchw(F_.Act(y_dev, Cout)).cpu().double(), y64)      # the raw convolution is exact
    out.backward(_to_act(da, dt).t)
    torch.cuda.synchronize()

    count = N * H * W
    m64 = y64.mean(dim=(0, 2, 3))
    var64 = (y64 ** 2).mean(dim=(0, 2, 3)) - m64 ** 2
    eps32, mom32 = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))     # the kernel receives floats
    invstd64 = 1.0 / torch.sqrt(var64 + eps32)
    stats = {"mean": (mean, m64), "invstd": (invstd, invstd64), "running_mean": (rmean, mom32 * m64),
             "running_var": (rvar, (1.0 - mom32) + mom32 * var64 * (count / (count - 1.0)))}
    for name, (got, want) in stats.items():
        err = float(((got.cpu().double() - want).abs() / want.abs()).max())
        print(f"{name}: max relative error {err:.3e}")
        assert torch.allclose(got.cpu().double(), want, rtol=3e-7, atol=1e-30 if "mean" in name else 0), (name, err)
    assert int(nbt) == 1

    got = {"activation": F_.to_nchw(F_.Act(out.detach(), Cout)).cpu(), "dx": xd.grad.cpu(), "dw": wd.grad.cpu(), "dgamma": gd.grad.cpu(), "dbeta": bed.grad.cpu()}
    want = {"activation": a64, "dx": grads64[0], "dw": grads64[1], "dgamma": grads64[2], "dbeta": grads64[3]}
    for name in got:
        err = rel_l2(got[name], want[name])
        print(f"{name}: relative L2 error {err:.3e} (bound {tol:.3e}, CPU bf16 autocast {yard:.3e})")
        assert err < tol, (name, err, tol)
    assert bd.grad is None or float(bd.grad.abs().max()) == 0.0                 # a bias in front of a training-mode BatchNorm has no gradient
