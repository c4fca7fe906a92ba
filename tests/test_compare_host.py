"""CPU-only checks of ``mau_amd.compare``: the host twins against a direct spelling of the Model Comparison page's numpy (float32
arrays, Python-float metrics), the quadrant split, the whole-tile join, the page's derived colour ranges, truncation and clipping
of the colour bytes, and the C ABI of the new entry points (header, library, binding, size helpers, refused calls) -- the library
is needed, a device is not.  The normalisation numbers are made up; the palette is the app's."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests._helpers import header_prototypes, header_symbols
from tests.test_scenario_host import METRICS, load_palette


def make_outputs(rng, M, H, W):
    """M heads' outputs and one target, normalised: NDVI in -1..1, temperature as a z-score."""
    out = rng.standard_normal((M, 2, H, W)).astype(np.float32)
    out[:, 0] = np.tanh(out[:, 0])
    tgt = rng.standard_normal((2, H, W)).astype(np.float32)
    tgt[0] = np.tanh(tgt[0])
    return out, tgt


def make_sample(rng, H, W, ncls=9):
    """A compact input sample: two class maps and the five normalised planes."""
    cls_a = rng.integers(0, ncls, (H, W)).astype(np.uint8)
    cls_b = rng.integers(0, ncls, (H, W)).astype(np.uint8)
    cont = rng.standard_normal((5, H, W)).astype(np.float32)
    cont[:3] *= 2.5                                                     # colours that leave [0, 1] on both sides
    return cls_a, cls_b, cont


def page_numbers(gt_img, pred_img):
    """What the page computes for one figure, in its own words: the error map and the three colour-range numbers."""
    error = pred_img - gt_img
    top = np.max(np.abs(error))
    return error, np.min([gt_img.min(), pred_img.min()]), np.max([gt_img.max(), pred_img.max()]), top if top > 0 else 1


@pytest.mark.parametrize("M,H,W", [(1, 7, 9), (3, 20, 18), (2, 1, 1), (2, 33, 2)])
def test_compare_host_is_the_pages_numpy(M, H, W):
    from mau_amd import compare as C
    rng = np.random.default_rng(100 + M)
    out, tgt = make_outputs(rng, M, H, W)
    pred, gt, err, rows = C.compare_host(out, tgt, METRICS)
    assert pred.dtype == gt.dtype == err.dtype == np.float32 and rows.dtype == np.float64
    assert pred.shape == err.shape == out.shape and gt.shape == tgt.shape and rows.shape == (M * 2, 40)
    # un-normalisation as the page writes it: zeros_like, then channel by channel
    want_gt, want_pred = np.zeros_like(tgt), np.zeros_like(out)
    want_gt[0], want_gt[1] = tgt[0], tgt[1] * METRICS["temp_std"] + METRICS["temp_mean"]
    for m in range(M):
        want_pred[m, 0], want_pred[m, 1] = out[m, 0], out[m, 1] * METRICS["temp_std"] + METRICS["temp_mean"]
    assert np.array_equal(gt.view(np.uint32), want_gt.view(np.uint32)) and np.array_equal(pred.view(np.uint32), want_pred.view(np.uint32))
    stats = C.ComparisonStats(torch.from_numpy(rows))
    h, w = H, W
    boxes = [(0, h, 0, w), (0, h // 2, 0, w // 2), (0, h // 2, w // 2, w), (h // 2, h, 0, w // 2), (h // 2, h, w // 2, w)]
    for m in range(M):
        for c in range(2):
            error, _, _, _ = page_numbers(want_gt[c], want_pred[m, c])
            assert np.array_equal(err[m, c].view(np.uint32), error.view(np.uint32))
            for r, (y1, y2, x1, x2) in enumerate(boxes):
                row = rows[m * 2 + c].reshape(5, 8)[r]
                assert row[0] == (y2 - y1) * (x2 - x1)
                if row[0] == 0:                                         # a one-pixel tile has empty quadrants: nothing to draw
                    assert row[1] == row[3] == np.inf and row[2] == row[4] == -np.inf and (row[5:] == 0).all()
                    continue
                g, p = want_gt[c, y1:y2, x1:x2], want_pred[m, c, y1:y2, x1:x2]
                e, vmin, vmax, top = page_numbers(g, p)
                assert (row[1], row[2], row[3], row[4], row[5]) == (g.min(), g.max(), p.min(), p.max(), np.abs(e).max())
                assert float(stats.vmin[m, c, r]) == vmin and float(stats.vmax[m, c, r]) == vmax and float(stats.err_max_abs[m, c, r]) == top
                e64 = e.astype(np.float64)
                n = e64.size
                assert abs(row[6] - np.abs(e64).sum()) <= n * 2.0 ** -52 * np.abs(e64).sum()
                assert abs(row[7] - (e64 ** 2).sum()) <= n * 2.0 ** -52 * (e64 ** 2).sum()
                assert abs(float(stats.mae[m, c, r]) - np.abs(e64).mean()) <= n * 2.0 ** -51 * np.abs(e64).mean()
                assert abs(float(stats.rmse[m, c, r]) - np.sqrt((e64 ** 2).mean())) <= n * 2.0 ** -51 * np.sqrt((e64 ** 2).mean())
    with pytest.raises(ValueError):
        C.compare_host(out[:, :1], tgt, METRICS)
    with pytest.raises(ValueError):
        C.compare_host(out, tgt, {"temp_mean": 1.0})


def test_quadrants_of_an_odd_tile_and_the_whole_tile_join():
    from mau_amd import compare as C
    assert C.quadrants(7, 9) == ((0, 3, 0, 4), (0, 3, 4, 9), (3, 7, 0, 4), (3, 7, 4, 9))
    rng = np.random.default_rng(7)
    out, tgt = make_outputs(rng, 2, 7, 9)
    _, _, _, rows = C.compare_host(out, tgt, METRICS)
    rows = rows.reshape(4, 5, 8)
    assert np.array_equal(rows[:, :, 0], np.tile(np.array([63.0, 3 * 4, 3 * 5, 4 * 4, 4 * 5]), (4, 1)))
    for row in rows:
        tl, tr, bl, br = row[1:]
        want = np.array([tl[0] + tr[0] + bl[0] + br[0], min(tl[1], tr[1], bl[1], br[1]), max(tl[2], tr[2], bl[2], br[2]),
                         min(tl[3], tr[3], bl[3], br[3]), max(tl[4], tr[4], bl[4], br[4]), max(tl[5], tr[5], bl[5], br[5]),
                         ((tl[6] + tr[6]) + bl[6]) + br[6], ((tl[7] + tr[7]) + bl[7]) + br[7]])
        assert np.array_equal(row[0].view(np.uint64), want.view(np.uint64))
        assert np.array_equal(C.join_entries(C.join_entries(C.join_entries(tl, tr), bl), br).view(np.uint64), row[0].view(np.uint64))


def test_nan_is_skipped_by_ranges_and_carried_by_sums():
    from mau_amd import compare as C
    rng = np.random.default_rng(8)
    out, tgt = make_outputs(rng, 1, 6, 6)
    out[0, 1, 0, 0] = np.nan                                            # top-left quadrant of the temperature channel
    _, _, _, rows = C.compare_host(out, tgt, METRICS)
    rows = rows.reshape(2, 5, 8)
    assert np.isfinite(rows[0]).all()                                   # the NDVI channel is untouched
    assert np.isfinite(rows[1, :, :6]).all()
    assert np.isnan(rows[1, [0, 1], 6:]).all() and np.isfinite(rows[1, 2:, 6:]).all()


def test_err_max_abs_is_one_for_a_perfect_prediction():
    from mau_amd import compare as C
    rng = np.random.default_rng(9)
    _, tgt = make_outputs(rng, 1, 8, 10)
    _, _, err, rows = C.compare_host(tgt[None], tgt, METRICS)
    stats = C.ComparisonStats(torch.from_numpy(rows))
    assert not err.any() and not stats.max_abs_err.any()
    assert (stats.err_max_abs == 1).all() and (stats.mae == 0).all() and (stats.rmse == 0).all()
    assert torch.equal(stats.vmin, stats.gt_min) and torch.equal(stats.vmax, stats.gt_max)
    assert tuple(stats.table.shape) == (1, 2, 5, 8) and tuple(stats.region("bottom_right").shape) == (1, 2, 8)
    assert torch.equal(stats.region("top_left")[..., 2], stats.gt_max[..., 1]) and torch.equal(stats.entry("count"), stats.count)
    with pytest.raises(AttributeError):
        stats.no_such_entry


def test_input_views_host_is_the_pages_numpy():
    from mau_amd import compare as C
    palette = load_palette()
    rng = np.random.default_rng(10)
    cls_a, cls_b, cont = make_sample(rng, 13, 11)
    got = C.input_views_host(cls_a, cls_b, cont, palette, METRICS)
    # the page's own lines on the planes it slices out of the dense stack
    rgb_normalized = cont[0:3]
    rgb_image = (rgb_normalized * np.array(METRICS["rgb_std"])[:, np.newaxis, np.newaxis] + np.array(METRICS["rgb_mean"])[:, np.newaxis, np.newaxis]) * 255.0
    assert rgb_image.dtype == np.float64
    rgb_image = np.clip(rgb_image.transpose(1, 2, 0), 0, 255).astype(np.uint8)
    temp_image = cont[4] * METRICS["temp_std"] + METRICS["temp_mean"]
    assert temp_image.dtype == np.float32
    assert got["rgb8"].dtype == np.uint8 and np.array_equal(got["rgb8"], rgb_image)
    assert (rgb_image == 0).mean() > 0.05 and (rgb_image == 255).mean() > 0.05      # the sample does clip on both sides
    assert np.array_equal(got["temp_c"].view(np.uint32), temp_image.view(np.uint32))
    assert np.array_equal(got["ndvi"].view(np.uint32), cont[3].view(np.uint32))
    assert np.array_equal(got["dw_t1_rgb"], palette[cls_a]) and np.array_equal(got["dw_t2_rgb"], palette[cls_b])
    assert got["dw_t1_rgb"].shape == (13, 11, 3) and got["dw_t1_rgb"].dtype == np.uint8
    cls_a[0, 0], cls_b[1, 1] = 9, 255                                   # ids the palette does not have: black
    got = C.input_views_host(cls_a, cls_b, cont, palette, METRICS)
    assert not got["dw_t1_rgb"][0, 0].any() and not got["dw_t2_rgb"][1, 1].any()
    with pytest.raises(ValueError):
        C.input_views_host(cls_a, cls_b, cont[:4], palette, METRICS)
    with pytest.raises(ValueError):
        C.input_views_host(cls_a, cls_b, cont, palette.astype(np.int32), METRICS)


def test_colour_bytes_truncate_and_clip():
    """Values placed just below and above 0, 255 and an integer boundary.  With std 1 and mean 0 the byte is
    trunc(clip(double(x) * 255)): the product of a 24-bit and an 8-bit number is exact in float64, so the expected byte is
    exact rational arithmetic."""
    from mau_amd import compare as C
    one, below_one, above_one = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0)), np.nextafter(np.float32(1.0), np.float32(2.0))
    under = np.float32(100.0 / 255.0)
    if Fraction(float(under)) * 255 >= 100:                              # the float32 neighbours of 100 / 255, one on each side
        under = np.nextafter(under, np.float32(0.0))
    over = np.nextafter(under, np.float32(1.0))
    assert Fraction(float(under)) * 255 < 100 <= Fraction(float(over)) * 255
    tiny = np.float32(1e-30)
    xs = np.array([-tiny, -0.0, 0.0, tiny, np.float32(1.0 / 255.0 - 1e-6), below_one, one, above_one, np.float32(7.5), np.float32(-3.0),
                   under, over, np.float32(0.5), np.nan, np.inf, -np.inf], dtype=np.float32)
    want = np.array([0, 0, 0, 0, 0, 254, 255, 255, 255, 0, 99, 100, 127, 0, 255, 0], dtype=np.uint8)
    for x, b in zip(xs, want):                                          # the expectation itself, exactly
        if np.isfinite(x):
            assert b == int(min(max(Fraction(float(x)) * 255, 0), 255)), x
    cont = np.zeros((5, 1, xs.size), dtype=np.float32)
    cont[:3] = xs
    metrics = dict(METRICS, rgb_mean=[0.0, 0.0, 0.0], rgb_std=[1.0, 1.0, 1.0])
    z = np.zeros((1, xs.size), dtype=np.uint8)
    got = C.input_views_host(z, z, cont, load_palette(), metrics)["rgb8"]
    assert got.shape == (1, xs.size, 3)
    for c in range(3):
        assert np.array_equal(got[0, :, c], want), got[0, :, c]


def test_header_library_and_binding_carry_the_compare_entry_points():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    want = {"mau_compare_row_elems": 0, "mau_compare_chunks": 2, "mau_compare_ws_elems": 3, "mau_compare_result": 14, "mau_compare_inputs": 14}
    syms, protos = header_symbols(), header_prototypes()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in want.items():
        assert name in syms and hasattr(so, name) and name in _lib.PROTOTYPES, name
        assert len(protos[name][1]) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert list(protos[name][1]) == list(_lib.PROTOTYPES[name][1]) and protos[name][0] is _lib.PROTOTYPES[name][0], name
    assert protos["mau_compare_result"][1][2:4] == [ctypes.c_double, ctypes.c_double]
    assert protos["mau_compare_ws_elems"][0] is ctypes.c_size_t
    assert _lib.lib.mau_abi_version() == 5                              # additive: no version bump
    assert mau_amd.compare.ComparisonSession is mau_amd.ComparisonSession and mau_amd.compare.ComparisonResult is mau_amd.ComparisonResult


def test_compare_size_helpers_and_refused_calls():
    import mau_amd  # noqa: F401
    from mau_amd._lib import lib
    assert lib.mau_compare_row_elems() == 40
    per = lib.mau_reduce_tickets_elems()
    for M, H, W in ((1, 1, 1), (1, 7, 9), (3, 67, 63), (3, 250, 250), (per, 8, 8)):
        chunks = lib.mau_compare_chunks(H, W)
        assert chunks >= 1 and (chunks - 1) * 4096 < H * W <= chunks * 4096
        assert chunks == lib.mau_scenario_result_chunks(H, W)           # the one chunking of chunk_reduce.h
        assert lib.mau_compare_ws_elems(M, H, W) == min(M * 2, per) * chunks * 28 > 0
    assert lib.mau_compare_chunks(250, 250) == 16 and lib.mau_compare_chunks(67, 63) == 2 and lib.mau_compare_chunks(7, 9) == 1
    for bad in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert lib.mau_compare_ws_elems(*bad) == 0
    assert lib.mau_compare_chunks(0, 5) == 0 and lib.mau_compare_chunks(5, -1) == 0
    # refused calls report through mau_last_error, without a device (argument validation comes first)
    some = ctypes.create_string_buffer(64)
    p = ctypes.cast(some, ctypes.c_void_p)
    ten = [p] * 8
    assert lib.mau_compare_result(None, None, 0.0, 1.0, None, None, None, None, None, None, 1, 8, 8, None) != 0
    assert b"compare_result: null pointer" in lib.mau_last_error()
    for k in range(8):                                                  # each pointer on its own
        args = list(ten)
        args[k] = None
        assert lib.mau_compare_result(args[0], args[1], 0.0, 1.0, *args[2:], 1, 8, 8, None) != 0
        assert b"compare_result: null pointer" in lib.mau_last_error()
    for M, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-2, 8, 8)):
        assert lib.mau_compare_result(p, p, 0.0, 1.0, p, p, p, p, p, p, M, H, W, None) != 0
        assert b"compare_result: non-positive dimension" in lib.mau_last_error()
    assert lib.mau_compare_inputs(*([None] * 10), 8, 8, 9, None) != 0
    assert b"compare_inputs: null pointer" in lib.mau_last_error()
    assert lib.mau_compare_inputs(*([p] * 10), 0, 8, 9, None) != 0
    assert b"compare_inputs: non-positive dimension" in lib.mau_last_error()
    for ncls in (0, lib.mau_scenario_max_classes() + 1):
        assert lib.mau_compare_inputs(*([p] * 10), 8, 8, ncls, None) != 0
        assert b"compare_inputs: ncls" in lib.mau_last_error()
