"""``mau_conv3x3_first_wgrad_bn`` (csrc/conv3x3_first.hip) at the C ABI: the first layer's weight gradient with dz formed in the kernel's
load stage, against the two launches it replaces -- ``mau_bn_relu_bwd_apply`` followed by ``mau_conv3x3_first_wgrad`` -- BIT FOR BIT
(dw as uint32 patterns).  The reference is the library's own two-call route, whose kernels are pinned elsewhere
(tests/test_gpu_bn_head.py, tests/test_gpu_ops.py); what is tested here is that the fused loader puts the same LDS image in front of the
same multiply: every shape below is one way for a loader to go wrong.

Inputs are random with non-trivial scale (both signs), shift, mean and invstd; the sums come from a real ``mau_bn_relu_bwd_reduce`` of the
same tensors.  Lanes of da / z outside [0, C8) and the whole dz buffer and workspace start as NaN."""
import pytest
import torch

from tests._helpers import _call, _stream, mau, pad8, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

# a ragged only segment whose halo rows lie above and below the image (3 x 5); W just above one segment, halo rows inside and outside
# (18 x 37); whole segments, several images (16 x 64); three segments a row, an odd row count (33 x 96)
SHAPES = [(1, 3, 5), (2, 18, 37), (3, 16, 64), (2, 33, 96)]
CINS = [1, 6, 8]
# a narrow row; exactly one co tile; a second, partial co tile; a pitch above Cout
COUT_LD = [(16, 16), (64, 64), (80, 80), (64, 72)]
DTYPES = [torch.bfloat16, torch.float16]


def _code(dt):
    from mau_amd import _lib
    return {torch.bfloat16: _lib.MAU_BF16, torch.float16: _lib.MAU_F16}[dt]


def _inputs(N, H, W, Cout, ld, dt, seed):
    """da, z as (npix, ld) with NaN outside [0, C8) and 0 in the pad lanes; the four coefficient vectors; sums (2 C + 1 fp64, the count
    appended) from mau_bn_relu_bwd_reduce"""
    from mau_amd._lib import lib
    g = torch.Generator().manual_seed(seed)
    npix, C8 = N * H * W, pad8(Cout)

    def rows(scale):
        t = torch.full((npix, ld), float("nan"), dtype=dt)
        t[:, :Cout] = (torch.randn(npix, Cout, generator=g) * scale).to(dt)
        t[:, Cout:C8] = 0
        return t.cuda()

    da, z = rows(0.5), rows(1.5)
    sign = torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
    k = dict(scale=sign * (0.5 + torch.rand(Cout, generator=g)), shift=0.5 * torch.randn(Cout, generator=g),
             mean=0.3 * torch.randn(Cout, generator=g), invstd=0.5 + 1.5 * torch.rand(Cout, generator=g))
    k = {n: v.float().cuda() for n, v in k.items()}
    kp = [k[n].data_ptr() for n in ("scale", "shift", "mean", "invstd")]
    nb = lib.mau_bn_bwd_rows(npix)
    slab = torch.full((nb, 2, Cout), float("nan"), device="cuda")
    _call("mau_bn_relu_bwd_reduce", da.data_ptr(), ld, z.data_ptr(), ld, *kp, slab.data_ptr(), Cout, _code(dt), npix, Cout, _stream())
    sums = torch.cat([slab.double().sum(0).reshape(-1), torch.tensor([float(npix)], dtype=torch.float64, device="cuda")])
    assert bool(torch.isfinite(sums).all())
    return da, z, k, kp, sums


def _x8(N, H, W, Cin, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x8 = torch.zeros(N, H, W, 8, dtype=dt)
    x8[..., :Cin] = torch.randn(N, H, W, Cin, generator=g).to(dt)
    return x8.cuda()


def _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, count, x8):
    """(dw of apply + first_wgrad, dw of first_wgrad_bn)"""
    from mau_amd._lib import lib
    code, st, npix = _code(dt), _stream(), N * H * W
    nws = lib.mau_conv3x3_first_wgrad_ws_elems(N, H, W, Cout)
    out = []
    for fused in (False, True):
        ws = torch.full((nws,), float("nan"), device="cuda")
        dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
        if fused:
            _call("mau_conv3x3_first_wgrad_bn", x8.data_ptr(), da.data_ptr(), ld, z.data_ptr(), ld, *kp, sums.data_ptr(), count, dw.data_ptr(),
                  ws.data_ptr(), Cin, Cout, code, N, H, W, st)
        else:
            dz = torch.full((npix, ld), float("nan"), dtype=dt, device="cuda")
            _call("mau_bn_relu_bwd_apply", da.data_ptr(), ld, z.data_ptr(), ld, *kp, sums.data_ptr(), count, dz.data_ptr(), ld, code, npix, Cout, st)
            _call("mau_conv3x3_first_wgrad", x8.data_ptr(), dz.data_ptr(), ld, dw.data_ptr(), ws.data_ptr(), Cin, Cout, code, N, H, W, st)
        torch.cuda.synchronize()
        out.append(dw.cpu())
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cout_ld", COUT_LD, ids=lambda c: f"co{c[0]}ld{c[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_apply_then_wgrad(mau, shape, cout_ld, dt):
    (N, H, W), (Cout, ld) = shape, cout_ld
    da, z, k, kp, sums = _inputs(N, H, W, Cout, ld, dt, seed=7 + H)
    for Cin in CINS:
        x8 = _x8(N, H, W, Cin, dt, seed=3 + Cin)
        two, one = _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, float(N * H * W), x8)
        assert bool(torch.isfinite(two).all()) and float(two.abs().max()) > 0
        assert same_bits(one, two), (shape, Cin, cout_ld, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_count_in_the_sums(mau, dt):
    """data parallel: count = 0, the all-reduced pixel count is sums[2 * C] -- here NOT the tensor's own pixel count"""
    N, H, W, Cin, Cout, ld = 2, 18, 37, 6, 80, 88
    da, z, k, kp, sums = _inputs(N, H, W, Cout, ld, dt, seed=21)
    sums[2 * Cout] = 3.0 * N * H * W
    x8 = _x8(N, H, W, Cin, dt, seed=22)
    two, one = _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, 0.0, x8)
    assert same_bits(one, two)
    explicit = _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, 3.0 * N * H * W, x8)
    assert same_bits(one, explicit[1]) and same_bits(two, explicit[0])


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_nan_and_inf_in_da(mau, dt):
    """non-finite gradients at a few pixels: whatever the two launches make of them, the fused kernel makes the same"""
    N, H, W, Cin, Cout, ld = 2, 18, 37, 6, 64, 64
    da, z, k, kp, sums = _inputs(N, H, W, Cout, ld, dt, seed=31)
    for pix, c, v in ((0, 0, float("nan")), (40, 17, float("inf")), (N * H * W - 1, 63, float("-inf")), (700, 33, float("nan"))):
        da[pix, c] = v
    da[41, :Cout] = float("inf")                               # (a whole pixel: some channel's ReLU is open there)
    da[701, :Cout:2] = float("nan")
    x8 = _x8(N, H, W, Cin, dt, seed=32)
    two, one = _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, float(N * H * W), x8)
    assert not bool(torch.isfinite(two).all())
    assert same_bits(one, two)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_every_wave_cycles_both_buffers(mau, dt):
    """The grid is at most 2 workgroups x 4 waves per compute unit, a wave's tiles are tile, tile + waves, ...: only above 2048 tiles
    (256 compute units) does a wave run its loop more than once.  3 x 50 rows x 29 segments = 4350 tiles: up to three trips a wave, so
    registers are refilled behind a tile's multiply, both LDS buffers are re-used, and the last trip takes the other branch."""
    N, H, W, Cin, Cout, ld = 3, 50, 900, 6, 80, 80
    da, z, k, kp, sums = _inputs(N, H, W, Cout, ld, dt, seed=41)
    x8 = _x8(N, H, W, Cin, dt, seed=42)
    two, one = _both_routes(N, H, W, Cin, Cout, ld, dt, da, z, kp, sums, float(N * H * W), x8)
    assert bool(torch.isfinite(two).all())
    assert same_bits(one, two)
