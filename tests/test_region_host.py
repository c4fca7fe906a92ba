"""CPU-only checks of ``mau_amd.region``: the window grid, the blend's host twin (``stitch_host``: exact where the arithmetic says
it is), ``gather_host`` against ``scenario.prepare_input_host``, and the C ABI of the two entry points (header, library, binding,
refused calls -- argument validation comes before any launch, so no device is needed)."""
import ctypes

import numpy as np
import pytest

from tests._helpers import header_prototypes, header_symbols
from tests.test_scenario_host import METRICS, load_palette, make_tile

# (Hr, Wr, T, overlap): ragged both ways; no overlap with a moved-back last window; an exact multiple; one window; small odd sizes
SHAPES = [(70, 83, 32, 8), (70, 83, 32, 0), (64, 64, 32, 0), (32, 32, 32, 8), (41, 47, 16, 5)]


def cut(field, ys, xs, T):
    """The windows of a (C, Hr, Wr) field in window order k = iy * nx + ix."""
    return np.stack([field[:, y0:y0 + T, x0:x0 + T] for y0 in ys for x0 in xs])


def test_window_origins_sweep():
    from mau_amd import region as R
    cases = 0
    for T in (16, 17, 32, 250):
        for overlap in sorted({0, 1, T // 4, T // 2 - 1, T // 2}):
            for n in sorted({T, T + 1, T + overlap, 2 * T - overlap, 2 * T - overlap + 1, 2 * T, 3 * T - 1, 5 * T + 3, 1000}):
                o = R.window_origins(n, T, overlap)
                assert o.dtype == np.int32 and o.ndim == 1
                assert o[0] == 0 and o[-1] == n - T, (n, T, overlap, o)
                d = np.diff(o)
                assert (d >= 1).all() and (d <= T).all() and (d[:-1] == T - overlap).all(), (n, T, overlap, o)
                cover = np.zeros(n, dtype=np.int64)
                for s in o:
                    cover[s:s + T] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (n, T, overlap, o)
                assert len(o) == (1 if n == T else 1 + -(-(n - T) // (T - overlap)))       # no window more than needed
                assert np.array_equal(R._check_table(o, n, T, "t"), o)                      # ... and the stitch wrapper takes it
                cases += 1
    assert cases > 100
    assert R.window_origins(32, 32, 8).tolist() == [0] and R.window_origins(33, 32, 8).tolist() == [0, 1]
    assert R.window_origins(70, 32, 8).tolist() == [0, 24, 38] and R.window_origins(83, 32, 8).tolist() == [0, 24, 48, 51]
    for bad in ((31, 32, 0), (100, 15, 0), (5000, 4097, 0), (100, 32, 17), (100, 32, -1)):
        with pytest.raises(ValueError):
            R.window_origins(*bad)


def test_blend_weights_and_table_rules():
    from mau_amd import region as R
    assert R.blend_weights(8, 3).tolist() == [1, 2, 3, 3, 3, 3, 2, 1] and R.blend_weights(8, 3).dtype == np.int64
    assert R.blend_weights(5, 100).tolist() == [1, 2, 3, 2, 1] and R.blend_weights(4, 1).tolist() == [1, 1, 1, 1]
    assert R.default_ramp(0) == 1 and R.default_ramp(8) == 8
    with pytest.raises(ValueError):
        R.blend_weights(8, 0)
    # tables the device could not check: not from 0, not to n - T, descending, a gap, four windows over one coordinate
    for bad in ([1, 24, 38], [0, 24, 37], [0, 38, 24, 38], [0, 38], [0, 5, 10, 15, 38]):
        with pytest.raises(ValueError):
            R._check_table(np.array(bad), 70, 32, "t")
    assert R._check_table([0, 10, 20, 38], 70, 32, "t").dtype == np.int32                  # three over [20, 32): allowed


@pytest.mark.parametrize("Hr,Wr,T,overlap", SHAPES)
def test_stitch_host_returns_a_cut_field_bit_for_bit(Hr, Wr, T, overlap):
    """Integer weights: every w * v is exact in fp64 and so is every partial sum of v * (an integer < 2^26), hence num / den == v."""
    from mau_amd import region as R
    rng = np.random.default_rng(Hr * 100 + overlap)
    field = (rng.standard_normal((2, Hr, Wr)) * 300).astype(np.float32)                   # temperature-like magnitudes
    ys, xs = R.window_origins(Hr, T, overlap), R.window_origins(Wr, T, overlap)
    got = R.stitch_host(cut(field, ys, xs, T), ys, xs, (Hr, Wr), R.default_ramp(overlap))
    assert got.dtype == np.float32 and got.shape == field.shape
    assert np.array_equal(got.view(np.uint32), field.view(np.uint32))


def test_stitch_host_without_overlap_places_windows_side_by_side():
    from mau_amd import region as R
    rng = np.random.default_rng(7)
    T, ny, nx = 16, 3, 2
    win = (rng.standard_normal((ny * nx, 2, T, T)) * 300).astype(np.float32)
    ys, xs = R.window_origins(ny * T, T, 0), R.window_origins(nx * T, T, 0)
    assert ys.tolist() == [0, 16, 32] and xs.tolist() == [0, 16]
    want = win.reshape(ny, nx, 2, T, T).transpose(2, 0, 3, 1, 4).reshape(2, ny * T, nx * T)
    for ramp in (1, 4):                                                                    # one window per pixel: the weight cancels
        got = R.stitch_host(win, ys, xs, (ny * T, nx * T), ramp)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a pixel no window covers is NaN
    gap = R.stitch_host(win[:2], np.array([0]), np.array([0, 20]), (T, 40), 1)
    assert np.array_equal(np.isnan(gap[0, 0]), np.isin(np.arange(40), list(range(16, 20)) + list(range(36, 40))))
    with pytest.raises(ValueError):
        R.stitch_host(win[:5], ys, xs, (ny * T, nx * T), 1)


def test_stitch_host_is_the_weighted_mean_where_windows_overlap():
    """Restated per pixel with Python integers and fractions: the float64 quotient of the exact numerator."""
    from fractions import Fraction
    from mau_amd import region as R
    rng = np.random.default_rng(8)
    Hr, Wr, T, overlap = 41, 47, 16, 5
    ys, xs = R.window_origins(Hr, T, overlap), R.window_origins(Wr, T, overlap)
    win = (rng.standard_normal((ys.size * xs.size, 1, T, T)) * 300).astype(np.float32)
    got = R.stitch_host(win, ys, xs, (Hr, Wr), overlap)
    w1 = R.blend_weights(T, overlap)
    cover = np.zeros((Hr, Wr), dtype=int)
    for y0 in ys:
        for x0 in xs:
            cover[y0:y0 + T, x0:x0 + T] += 1
    most = tuple(int(v) for v in np.unravel_index(cover.argmax(), cover.shape))
    assert cover[most] >= 6                                                                # three windows along y, two along x
    for y, x in [(0, 0), (12, 12), (11, 30), (24, 23), (25, 31), (26, 40), (40, 46), (13, 5), (30, 11), most]:
        num, mag, den, n = Fraction(0), Fraction(0), 0, 0
        for iy, y0 in enumerate(ys):
            for ix, x0 in enumerate(xs):
                if 0 <= y - y0 < T and 0 <= x - x0 < T:
                    w = int(w1[y - y0]) * int(w1[x - x0])
                    v = Fraction(float(win[iy * xs.size + ix, 0, y - y0, x - x0]))
                    num, mag, den, n = num + w * v, mag + w * abs(v), den + w, n + 1
        exact = num / den
        # n <= 9 exact products added in float64 (n - 1 roundings of at most 2^-53 of the running magnitude), one division
        # (2^-53), one rounding to float32 (2^-24)
        bound = abs(exact) * (Fraction(1, 2 ** 24) + Fraction(1, 2 ** 52)) + Fraction(n, 2 ** 53) * mag / den
        assert n == cover[y, x] and abs(Fraction(float(got[0, y, x])) - exact) <= bound, (y, x, n)


def test_gather_host_is_prepare_input_host_on_the_cropped_planes():
    from mau_amd import region as R
    from mau_amd import scenario as S
    palette = load_palette()
    rng = np.random.default_rng(9)
    Hr, Wr, T = 37, 45, 16
    dw, rgb, ndvi, temp = make_tile(rng, Hr, Wr)
    origins = np.array([[0, 0], [Hr - T, Wr - T], [7, 13], [100, -4]])                     # the last one clamps to (Hr - T, 0)
    got = R.gather_host(dw, dw, rgb, ndvi, temp, origins, T, len(palette), METRICS)
    assert got.shape == (4, 23, T, T) and got.dtype == np.float32
    clear = np.zeros((8, 8, 4), dtype=np.uint8)                                            # all transparent: dw_t2 is dw_t1
    for k, (y0, x0) in enumerate([(0, 0), (Hr - T, Wr - T), (7, 13), (Hr - T, 0)]):
        ys, xs = slice(y0, y0 + T), slice(x0, x0 + T)
        want = S.prepare_input_host(dw[ys, xs], rgb[:, ys, xs], ndvi[ys, xs], temp[ys, xs], clear, palette, METRICS)
        assert np.array_equal(got[k].view(np.uint32), want[0].view(np.uint32)), k
    # an edited map shows in the last block only; a class id beyond the palette sets no channel
    dw2 = dw.copy()
    dw2[:8] = 200
    edited = R.gather_host(dw, dw2, rgb, ndvi, temp, origins[:1], T, len(palette), METRICS)
    assert np.array_equal(edited[0, :14], got[0, :14]) and edited[0, 14:, :8].sum() == 0 and np.array_equal(edited[0, 14:, 8:], got[0, 14:, 8:])
    with pytest.raises(ValueError):
        R.gather_host(dw, dw, rgb, ndvi, temp, origins, 40, len(palette), METRICS)


def test_header_library_and_binding_carry_the_region_entry_points():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    want = {"mau_region_gather": 16, "mau_region_stitch": 12}
    syms, protos = header_symbols(), header_prototypes()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in want.items():
        assert name in syms and hasattr(so, name) and name in _lib.PROTOTYPES, name
        assert len(protos[name][1]) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert list(protos[name][1]) == list(_lib.PROTOTYPES[name][1]) and protos[name][0] is _lib.PROTOTYPES[name][0], name
    assert _lib.lib.mau_abi_version() == 5
    assert mau_amd.region.RegionSession is not None and "region" in mau_amd.__all__


def test_entry_points_refuse_bad_arguments_without_a_device():
    import mau_amd  # noqa: F401
    from mau_amd._lib import lib
    p = ctypes.c_void_p(64)                                                                # never dereferenced: refused before any launch

    def gather(ldo=24, B=1, T=16, Hr=37, Wr=45, ncls=9, ptr=p):
        return lib.mau_region_gather(ptr, p, p, p, p, p, p, p, ldo, 1, B, T, Hr, Wr, ncls, None)

    def stitch(C=2, T=16, ramp=4, Hr=37, Wr=45, ny=3, nx=3, ptr=p):
        return lib.mau_region_stitch(ptr, p, p, p, C, T, ramp, Hr, Wr, ny, nx, None)

    for kw in (dict(T=38), dict(T=46, Hr=50), dict(ncls=0), dict(ncls=lib.mau_scenario_max_classes() + 1), dict(ldo=20), dict(ldo=16),
               dict(B=0), dict(ptr=None), dict(T=4097, Hr=5000, Wr=5000)):
        assert gather(**kw) == 1, kw
        assert b"region_gather" in lib.mau_last_error()
    for kw in (dict(T=38), dict(ramp=0), dict(C=0), dict(ny=0), dict(ptr=None), dict(Hr=70000, Wr=32)):
        assert stitch(**kw) == 1, kw
        assert b"region_stitch" in lib.mau_last_error()
