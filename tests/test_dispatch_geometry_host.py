"""Host-only dispatch contracts of the 16-bit 3x3 convolution (no GPU: size queries and the variant rule are plain host code).

The forward launch writes BatchNorm partial sums into a slab whose row count the caller asks ``mau_conv3x3_num_pixel_tiles`` for.
That query does not see the layer's input channels; the tile variant the launch picks does (64-channel layers with Cin > 192 may run
the 64-row, 8-wave tile <64,4,8> instead of the 32-row, 4-wave <64,4,4>).  The two must agree for EVERY layer, or the kernel stores
past the caller's allocation and the statistics are reduced over the wrong rows."""
import ctypes
import itertools

import pytest

TW = 16                                                    # pixel columns of every workgroup tile

# heights around every tile-row boundary (8 / 16 / 32 / 64), odd and even counts of 32-row tiles, and the sizes the networks run
HEIGHTS = [16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 128, 160, 224, 250, 256, 288, 299]
WIDTHS = [16, 17, 64, 128, 250, 256]
COUTS = [8, 64, 70, 128, 192, 256, 1024]
CINS = [0, 16, 64, 192, 193, 208, 256, 400, 1536]

# (N, H, W) with Cin = 256, Cout = 64: rows the caller allocated / rows the launch wrote before the rule knew about ceil(H / 32)
BROKEN = [((8, 224, 224), 3136, 3584), ((16, 160, 160), 3200, 3840), ((8, 288, 288), 5184, 5760), ((5, 224, 128), 1120, 1280),
          ((13, 65, 128), 1248, 1664), ((6, 96, 256), 1152, 1536)]


def _ceil_div(a, b):
    return -(-a // b)


def _wave_rows(nw, bn):
    """wave rows of a workgroup = slab rows per pixel tile (stated here independently of the library's tiling table, conv3x3_bf16.hip kTilings):
    <64,2,8> and <64,4,8> have 8, every other variant 4"""
    return 8 if (bn == 64 and nw == 8) else 4


def _rows_written(_lib, code, N, H, W, Cout, Cin):
    th, nw, bn, _ = _lib.conv3x3_variant(code, N, H, W, Cout, Cin=Cin)
    return _wave_rows(nw, bn) * N * _ceil_div(H, th) * _ceil_div(W, TW), (th, nw, bn)


def test_slab_query_matches_launch_geometry_sweep():
    """``mau_conv3x3_num_pixel_tiles`` (what functional.py allocates) == wave rows x pixel tiles of the variant the launch takes for
    that layer, whatever its input channels: both 16-bit types, N = 1..33, heights around every tile boundary, ragged widths."""
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    fn = _lib.lib.mau_conv3x3_variant
    th, nw, bn, kg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(th), ctypes.byref(nw), ctypes.byref(bn), ctypes.byref(kg))
    for h in (16, 31, 32, 33, 64, 65, 96, 97, 160, 224, 250, 256, 288):
        assert h in HEIGHTS
    bad, checked = [], 0
    for code in (_lib.MAU_BF16, _lib.MAU_F16):
        for N, H, W, Cout in itertools.product(range(1, 34), HEIGHTS, WIDTHS, COUTS):
            rows = _lib.lib.mau_conv3x3_num_pixel_tiles(code, N, H, W, Cout)
            for Cin in CINS:
                assert fn(code, N, H, W, Cin, Cout, *out) == 0
                want = _wave_rows(nw.value, bn.value) * N * _ceil_div(H, th.value) * _ceil_div(W, TW)
                checked += 1
                if rows != want:
                    bad.append(((code, N, Cin, Cout, H, W), rows, want, (th.value, nw.value, bn.value)))
    assert checked == 2 * 33 * len(HEIGHTS) * len(WIDTHS) * len(COUTS) * len(CINS)
    assert not bad, f"{len(bad)} of {checked} layers: (dtype, N, Cin, Cout, H, W), rows queried, rows written, variant: {bad[:12]}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape,was_allocated,was_written", BROKEN, ids=["x".join(map(str, b[0])) for b in BROKEN])
def test_slab_query_matches_launch_at_the_shapes_that_overran(shape, was_allocated, was_written, dtype):
    """The six 256 -> 64 layers named when the overrun was found (a U-Net++ full-resolution node at 224 x 224 among them): ceil(H / 32)
    is odd, so 8 * ceil(H / 64) rows per tile column are more than 4 * ceil(H / 32).  The query keeps the row count it always
    returned; the launch now writes exactly that many."""
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    code = _lib.MAU_BF16 if dtype == "bf16" else _lib.MAU_F16
    N, H, W = shape
    assert _ceil_div(H, 32) % 2 == 1
    rows = _lib.lib.mau_conv3x3_num_pixel_tiles(code, N, H, W, 64)
    assert rows == was_allocated == 4 * N * _ceil_div(H, 32) * _ceil_div(W, TW)
    assert was_written == 8 * N * _ceil_div(H, 64) * _ceil_div(W, TW)
    written, variant = _rows_written(_lib, code, N, H, W, 64, 256)
    assert written == rows, (shape, variant, f"the launch writes {written} slab rows, the caller allocates {rows}")


def test_k_rule_keeps_the_big_tile_where_the_slab_allows_it():
    """The fix must not throw the 8-wave tile away where it was measured faster and fits the slab: Cin > 192 at heights with an even
    number of 32-row tiles (256, 250: the bench's and the fixtures' sizes) stays on <64,4,8>; Cin <= 192 stays on <64,4,4>."""
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    for code in (_lib.MAU_BF16, _lib.MAU_F16):
        for H in (256, 250, 128, 64):
            assert _lib.conv3x3_variant(code, 32, H, 256, 64, Cin=208)[:3] == (64, 8, 64), H
            assert _lib.conv3x3_variant(code, 32, H, 256, 64, Cin=400)[:3] == (64, 8, 64), H
            assert _lib.conv3x3_variant(code, 32, H, 256, 64, Cin=192)[:3] == (32, 4, 64), H
        for (N, H, W), _, _ in BROKEN:                               # ... and where it does not fit, <64,4,4> whatever Cin is
            assert _lib.conv3x3_variant(code, N, H, W, 64, Cin=400)[:3] == (32, 4, 64), (N, H, W)


# the 3x3 layers of the U-Net at B = 32, 256 x 256 (model.py, nb_filter = 64..1024; conv0_0.conv1 runs the first-layer kernel):
# (Cin, Cout, H) -> (tile rows, waves, cout block, K groups) -- the code path of the bench's headline step
UNET_B32_VARIANTS = [
    (64, 64, 256, (32, 4, 64, 1)),        # conv0_0.conv2
    (64, 128, 128, (32, 8, 128, 1)),      # conv1_0.conv1
    (128, 128, 128, (32, 8, 128, 1)),     # conv1_0.conv2, conv1_1.conv2
    (128, 256, 64, (32, 8, 128, 1)),      # conv2_0.conv1
    (256, 256, 64, (32, 8, 128, 1)),      # conv2_0.conv2, conv2_1.conv2
    (256, 512, 32, (32, 8, 128, 1)),      # conv3_0.conv1
    (512, 512, 32, (32, 8, 128, 1)),      # conv3_0.conv2, conv3_1.conv2
    (576, 1024, 16, (16, 8, 128, 1)),     # conv4_0.conv1 (512 + the 64 metadata-embedding channels)
    (1024, 1024, 16, (16, 8, 128, 1)),    # conv4_0.conv2
    (1536, 512, 32, (32, 8, 128, 1)),     # conv3_1.conv1
    (768, 256, 64, (32, 8, 128, 1)),      # conv2_1.conv1
    (384, 128, 128, (32, 8, 128, 1)),     # conv1_1.conv1
    (192, 64, 256, (32, 4, 64, 1)),       # conv0_1.conv1; conv0_1.conv2 is the first row again
]


def test_unet_b32_layers_keep_their_variants():
    """``conv3x3_variant`` for the 13 U-Net layer shapes of the B = 32, 256 x 256 training step: the values the rule returned before
    the slab condition was added (none of these layers has Cin > 192 with 64 output channels), so the measured step runs the kernels it ran."""
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    assert len(UNET_B32_VARIANTS) == 13
    for Cin, Cout, H, want in UNET_B32_VARIANTS:
        for code in (_lib.MAU_BF16, _lib.MAU_F16):
            assert _lib.conv3x3_variant(code, 32, H, H, Cout, Cin=Cin) == want, (Cin, Cout, H)
            th, nw, bn, _ = want
            assert _lib.lib.mau_conv3x3_num_pixel_tiles(code, 32, H, H, Cout) == _wave_rows(nw, bn) * 32 * _ceil_div(H, th) * _ceil_div(H, TW)
