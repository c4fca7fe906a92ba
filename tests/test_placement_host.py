"""CPU-only checks of ``mau_amd.placement``: the stamp grid and the table of edits, the numpy twins against ``scenario``'s own host
path and against the order-exact twin of the reduction (tests/placement_ref.py), the NaN conventions of the rows, every
``ValueError``, and the C ABI of the new entry points (size helpers and refusals run without a device)."""
import ctypes

import numpy as np
import pytest

from tests import placement_ref as PR
from tests.test_scenario_host import METRICS, load_palette, make_tile

NCLS = 9


def P():
    from mau_amd import placement
    return placement


# --------------------------------------------------------------------------- #
# the grid and the table
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,p,stride,want", [(32, 8, 8, [0, 8, 16, 24]), (37, 5, 4, [0, 4, 8, 12, 16, 20, 24, 28, 32]),
                                             (37, 5, 3, [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 32]), (45, 7, 16, [0, 16, 32, 38]),
                                             (9, 9, 4, [0]), (10, 9, 4, [0, 1]), (512, 32, 16, list(range(0, 481, 16)))])
def test_stamp_grid(n, p, stride, want):
    g = P().stamp_grid(n, p, stride)
    assert g.dtype == np.int32 and g.tolist() == want
    assert g[0] == 0 and g[-1] == n - p and np.unique(g).size == g.size and (np.diff(g) > 0).all()      # the far edge exactly, nothing twice
    assert (np.diff(g)[:-1] == stride).all() and (np.diff(g) <= stride).all()


def test_stamp_grid_gaps_and_refusals():
    g = P().stamp_grid(45, 7, 16)                              # stride > p leaves gaps, and that is legal
    covered = np.zeros(45, dtype=bool)
    for o in g:
        covered[o:o + 7] = True
    assert not covered.all() and covered[-1] and covered[0]
    assert len(P().stamp_grid(512, 32, 16)) ** 2 == 961        # the issue's "1024 placements" is 31 x 31 whole stamps
    for bad in ((8, 9, 1), (8, 0, 1), (8, 2, 0), (8, -1, 2)):
        with pytest.raises(ValueError):
            P().stamp_grid(*bad)


def test_edits_table_is_class_major_then_rows_then_columns():
    t = P().edits_table([0, 8], [0, 5, 9], [6, 1])
    assert t.dtype == np.int32 and t.shape == (12, 3)
    assert t.tolist() == [[y, x, c] for c in (6, 1) for y in (0, 8) for x in (0, 5, 9)]
    for bad in (([], [0], [1]), ([0], [0.5], [1]), ([0], [0], [])):
        with pytest.raises(ValueError):
            P().edits_table(*bad)


# --------------------------------------------------------------------------- #
# the pack
# --------------------------------------------------------------------------- #
H, W, PH, PW = 37, 45, 5, 7
EDITS = np.array([[10, 12, 3], [-2, 20, 1], [35, 5, 2], [8, -3, 4], [15, 41, 5], [-1, -4, 6], [34, 42, 7],          # interior, four edges, two corners
                  [37, 0, 1], [-5, 10, 2], [3, 45, 2], [3, -7, 2],                                                  # wholly outside, all four sides
                  [10, 12, -1], [10, 12, 9], [10, 12, 3],                                                          # no class, no class, a duplicate
                  [-2 ** 31, 5, 1], [5, 2 ** 31 - 1, 1], [2 ** 31 - 1, -2 ** 31, 8]], dtype=np.int32)
STAMP_PIXELS = [35, 21, 14, 20, 20, 12, 9, 0, 0, 0, 0, 35, 35, 35, 0, 0, 0]            # by hand: the clipped rectangles


def test_the_two_stamp_formulations_agree_and_match_hand_counts():
    dw2 = np.random.default_rng(1).integers(0, NCLS, (H, W)).astype(np.uint8)
    want = PR.edited_maps(dw2, EDITS, PH, PW, NCLS)
    got = P().edited_maps_host(dw2, EDITS, (PH, PW), NCLS)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for b, e in enumerate(EDITS):
        m = P().stamp_mask(e, (H, W), (PH, PW))
        assert np.array_equal(m, PR.stamp(e, H, W, PH, PW)) and int(m.sum()) == STAMP_PIXELS[b], b
        edited = 0 <= e[2] < NCLS
        assert (got[b][m] == e[2]).all() if edited else np.array_equal(got[b], dw2)
        assert np.array_equal(got[b][~m], dw2[~m])
    assert (got[0][10:15, 12:19] == 3).all() and (got[1][0:3, 20:27] == 1).all() and (got[6][34:37, 42:45] == 7).all()


def test_pack_host_is_the_scenario_path_on_a_painted_canvas():
    """A canvas of the tile's own size (the nearest-neighbour tables are then the identity) painted with the palette colour on the
    stamp's rectangle: ``prepare_input_host`` builds the very input ``pack_host`` does."""
    from mau_amd import scenario as S
    palette = load_palette()
    dw, rgb, ndvi, temp = make_tile(np.random.default_rng(2), H, W)
    assert np.array_equal(S.nearest_index_table(H, H), np.arange(H))
    for e in EDITS[:7]:
        canvas = np.zeros((H, W, 4), dtype=np.uint8)
        y0, x0, c = (int(v) for v in e)
        canvas[max(y0, 0):max(y0 + PH, 0), max(x0, 0):max(x0 + PW, 0), :3] = palette[c]
        canvas[max(y0, 0):max(y0 + PH, 0), max(x0, 0):max(x0 + PW, 0), 3] = 255
        want = S.prepare_input_host(dw, rgb, ndvi, temp, canvas, palette, METRICS)
        got = P().pack_host(dw, None, rgb, ndvi, temp, e[None], (PH, PW), NCLS, METRICS)
        assert got.shape == (1, 23, H, W) and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # all rows at once, a second map of its own, against the per-pixel restatement
    dw2 = np.random.default_rng(3).integers(0, NCLS, (H, W)).astype(np.uint8)
    got = P().pack_host(dw, dw2, rgb, ndvi, temp, EDITS, (PH, PW), NCLS, METRICS)
    want = PR.pack_dense(dw, dw2, S.normalized_planes_host(rgb, ndvi, temp, METRICS), EDITS, PH, PW, NCLS)
    assert got.shape == (len(EDITS), 23, H, W) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[7, 14:], (dw2[None] == np.arange(NCLS).reshape(-1, 1, 1)).astype(np.float32))         # outside: the map as it is


# --------------------------------------------------------------------------- #
# the rows
# --------------------------------------------------------------------------- #
def make_result_case(rng, B, h, w):
    """A head output with a clear effect: the means are not sums that cancel, so a relative bound on them is meaningful."""
    base = rng.standard_normal((2, h, w)).astype(np.float32)
    out = (base[None] + 0.3 + 0.1 * rng.standard_normal((B, 2, h, w))).astype(np.float32)
    roi = (rng.random((h, w)) < 0.3).astype(np.uint8) * 7
    return out, base, roi


@pytest.mark.parametrize("h,w,vec4", [(37, 45, False), (64, 64, True), (64, 64, False), (65, 64, True), (96, 128, True)])
def test_result_host_agrees_with_the_order_exact_twin(h, w, vec4):
    rng = np.random.default_rng(h + w)
    out, base, roi = make_result_case(rng, 3, h, w)
    edits = np.array([[3, 4, 1], [-2, -3, 6], [h - 2, w - 3, 2]], dtype=np.int32)
    for r in (roi, None):
        exact = PR.placement_result(out, base, edits, r, METRICS["temp_mean"], METRICS["temp_std"], PH, PW, vec4=vec4)
        plain = P().result_host(out, base, edits, (PH, PW), METRICS["temp_mean"], METRICS["temp_std"], roi=r)
        assert exact.shape == plain.shape == (3, 12) and plain.dtype == np.float64
        finite = np.isfinite(exact)
        assert np.array_equal(finite, np.isfinite(plain)) and np.array_equal(np.isnan(exact), np.isnan(plain))
        rel = np.abs(plain[finite] - exact[finite]) / np.maximum(np.abs(exact[finite]), 1e-300)
        assert rel.max() <= 1e-12, rel.max()
        assert np.array_equal(plain[:, [0, 2, 3, 6, 11]], exact[:, [0, 2, 3, 6, 11]])      # counts, minimum, maximum: exact
        assert plain[:, 0].tolist() == [35, 12, 6] and (plain[:, 11] == 0).all()
        assert (plain[:, 6] == (0 if r is None else int((roi != 0).sum()))).all()
    if h * w % 4 == 0:                                          # the two access forms are two orders: the same values, not the same bits
        a = PR.placement_result(out, base, edits, roi, 1.5, 2.5, PH, PW, vec4=True)
        b = PR.placement_result(out, base, edits, roi, 1.5, 2.5, PH, PW, vec4=False)
        assert np.allclose(a, b, rtol=1e-12, atol=0) and np.array_equal(a[:, [0, 2, 3, 6, 11]], b[:, [0, 2, 3, 6, 11]])


def test_nan_conventions_of_the_rows():
    rng = np.random.default_rng(9)
    h, w = 12, 20
    out, base, roi = make_result_case(rng, 4, h, w)
    out[3, 1, 2, 3], out[3, 0, 5, 5], out[3, 0, 6, 6] = np.nan, np.inf, -np.inf
    edits = np.array([[2, 3, 1], [h, 0, 1], [-40, -40, 1], [2, 3, 1]], dtype=np.int32)       # a stamp, two empty ones, a sick sample
    for fn in (lambda *a, **k: P().result_host(*a, **k),
               lambda o, b, e, p, m, s, roi=None: PR.placement_result(o, b, e, roi, m, s, *p)):
        rows = fn(out, base, edits, (4, 6), 29.0, 11.0, roi=roi)
        assert rows[:, 0].tolist() == [24, 0, 0, 24] and np.isfinite(rows[0]).all()
        assert np.isnan(rows[1:3][:, [4, 9]]).all() and np.isfinite(rows[1:3][:, [1, 2, 3, 5, 7, 8, 10]]).all()    # an empty stamp: [4], [9]
        assert rows[3, 11] == 3 and np.isnan(rows[3, [1, 8]]).all() and np.isfinite(rows[3, [2, 3]]).all()          # sums carry, fmin / fmax skip
        assert np.isnan(rows[3, 4]) and np.isfinite(rows[3, 5]) and rows[3, 9] == rows[3, 9]                        # the NaN sits in the stamp
        none = fn(out, base, edits, (4, 6), 29.0, 11.0, roi=None)
        empty = fn(out, base, edits, (4, 6), 29.0, 11.0, roi=np.zeros((h, w), dtype=np.uint8))
        for r in (none, empty):                                                                                     # no roi: [6] = 0, [7], [10] NaN
            assert (r[:, 6] == 0).all() and np.isnan(r[:, [7, 10]]).all() and np.array_equal(r[:, :6], rows[:, :6], equal_nan=True)
        cover = fn(out[:2], base, np.array([[0, 0, 1], [-1, -2, 1]], dtype=np.int32), (h + 1, w + 2), 29.0, 11.0, roi=roi)
        assert (cover[:, 0] == h * w).all() and np.isnan(cover[:, 5]).all() and np.isfinite(cover[:, [1, 4, 9]]).all()   # the tile covered: [5]
        assert np.allclose(cover[:, 4], cover[:, 1], rtol=1e-12) and np.allclose(cover[:, 9], cover[:, 8], rtol=1e-12)


def test_placement_result_grid_and_best():
    pl = P()
    ys, xs, classes = pl.stamp_grid(32, 8, 8), pl.stamp_grid(40, 8, 16), np.array([6, 1], dtype=np.int32)
    edits = pl.edits_table(ys, xs, classes)
    rows = np.random.default_rng(4).standard_normal((edits.shape[0], 12))
    rows[5, 1] = np.nan
    r = pl.PlacementResult(rows, edits, classes, ys, xs, None, None)
    n = ys.size * xs.size
    assert np.array_equal(r.grid(6, 1), rows[:n, 1].reshape(ys.size, xs.size), equal_nan=True)
    assert np.array_equal(r.grid(1, 4), rows[n:, 4].reshape(ys.size, xs.size))
    for c, lo in ((6, 0), (1, n)):
        k = lo + int(np.nanargmin(rows[lo:lo + n, 1]))
        assert r.best(c) == (int(edits[k, 0]), int(edits[k, 1]), float(rows[k, 1])) and edits[k, 2] == c
    with pytest.raises(ValueError):
        r.grid(3)
    with pytest.raises(ValueError):
        r.grid(6, 12)


def test_every_value_error_of_the_host_helpers():
    pl = P()
    dw, rgb, ndvi, temp = make_tile(np.random.default_rng(5), 8, 8)
    out, base = np.zeros((2, 2, 8, 8), np.float32), np.zeros((2, 8, 8), np.float32)
    e2 = np.zeros((2, 3), dtype=np.int32)
    for bad in (np.zeros((2, 2), np.int32), np.zeros((0, 3), np.int32), np.zeros((2, 3), np.float32), np.array([[0, 0, 2 ** 31]])):
        with pytest.raises(ValueError):
            pl.pack_host(dw, None, rgb, ndvi, temp, bad, 2, NCLS, METRICS)
    for patch in (0, (2, 0), (-1, 2)):
        with pytest.raises(ValueError):
            pl.pack_host(dw, None, rgb, ndvi, temp, e2, patch, NCLS, METRICS)
        with pytest.raises(ValueError):
            pl.result_host(out, base, e2, patch, 0.0, 1.0)
    with pytest.raises(ValueError):
        pl.pack_host(dw, None, rgb, ndvi, temp, e2, 2, NCLS, {"rgb_mean": [0, 0, 0]})
    with pytest.raises(ValueError):
        pl.result_host(out[:, :1], base, e2, 2, 0.0, 1.0)
    with pytest.raises(ValueError):
        pl.result_host(out, base[:, :4], e2, 2, 0.0, 1.0)
    with pytest.raises(ValueError):
        pl.result_host(out, base, e2[:1], 2, 0.0, 1.0)
    with pytest.raises(ValueError):
        pl._int_list("1,x")
    assert list(pl._int_list("1, 6,")) == [1, 6]


# --------------------------------------------------------------------------- #
# the C ABI
# --------------------------------------------------------------------------- #
def test_size_helpers_and_refusals_without_a_device():
    import mau_amd
    from mau_amd import _lib
    lib = _lib.lib
    assert mau_amd.placement.PlacementSession is mau_amd.PlacementSession and "placement" in mau_amd.__all__
    assert lib.mau_placement_row_elems() == 12 == mau_amd.placement.ROW == len(mau_amd.placement.ROW_NAMES) == PR.ROW
    per = lib.mau_reduce_tickets_elems()
    for B, h, w in ((1, 1, 1), (5, 37, 45), (5, 64, 64), (5, 65, 64), (8, 512, 512), (per + 1, 8, 8)):
        chunks = lib.mau_placement_chunks(h, w)
        assert chunks >= 1 and (chunks - 1) * 4096 < h * w <= chunks * 4096
        assert lib.mau_placement_ws_elems(B, h, w) == min(B, per) * chunks * 12 > 0
    assert [lib.mau_placement_chunks(*s) for s in ((37, 45), (64, 64), (65, 64), (96, 128), (512, 512))] == [1, 1, 2, 3, 64]
    assert lib.mau_placement_chunks(0, 5) == 0 and lib.mau_placement_ws_elems(0, 8, 8) == 0 and lib.mau_placement_ws_elems(2, 8, -1) == 0
    assert _lib.PROTOTYPES["mau_placement_result"][1][4:6] == [ctypes.c_double, ctypes.c_double]
    assert lib.mau_abi_version() == 5
    # argument validation comes before any launch: a refused call needs no device and reads none of its pointers
    mem = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(mem) + 15) // 16 * 16

    def pack(dw_t1=p, dw_t2=p, edits=p, out=p, ldo=24, B=2, h=8, w=8, ph=2, pw=2, ncls=9):
        return lib.mau_placement_pack(dw_t1, dw_t2, p, p, p, edits, p, out, ldo, _lib.MAU_BF16, B, h, w, ph, pw, ncls, None)

    def result(out=p, base=p, edits=p, rows=p, ws=p, tickets=p, B=2, h=8, w=8, ph=2, pw=2):
        return lib.mau_placement_result(out, base, edits, None, 0.0, 1.0, rows, ws, tickets, B, h, w, ph, pw, None)

    for kw in (dict(ph=0), dict(pw=0), dict(pw=-3), dict(ncls=0), dict(ncls=lib.mau_scenario_max_classes() + 1), dict(ldo=20), dict(ldo=16),
               dict(ldo=28), dict(B=65536), dict(h=32768, w=32769), dict(dw_t1=None), dict(edits=None), dict(out=None), dict(B=0), dict(h=0)):
        assert pack(**kw) != 0, kw
        assert b"placement_pack" in lib.mau_last_error(), kw
    for kw in (dict(ph=0), dict(pw=0), dict(h=32768, w=32769), dict(out=None), dict(base=None), dict(edits=None), dict(rows=None), dict(ws=None),
               dict(tickets=None), dict(B=0), dict(w=0)):
        assert result(**kw) != 0, kw
        assert b"placement_result" in lib.mau_last_error(), kw
