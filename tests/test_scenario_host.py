"""CPU-only checks of ``mau_amd.scenario``: the host helpers against the reference's own spelling (Pillow's nearest-neighbour
resize, scipy's ``cdist`` + ``argmin``, numpy restatements of the float64 formulas of app/processing_utils.py:134-160), and the C ABI of the two new
entry points (header, library, binding, size helpers).  The normalisation numbers are made up; the palette is the app's."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests._helpers import header_prototypes, header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METRICS = {"rgb_mean": [0.4312, 0.5127, 0.3989], "rgb_std": [0.2213, 0.1907, 0.2571], "temp_mean": 29.4173, "temp_std": 11.0291,
           "meta_mean": [17.25, 9.5, 1250000.5, 2.125], "meta_std": [21.75, 68.25, 4900000.25, 1.375],
           "temp_series_mean": 0.0917, "temp_series_std": 1.0133}


def load_palette():
    from mau_amd import scenario as S
    with open(os.path.join(ROOT, "tests", "golden", "dw_palette.json")) as f:
        return S.palette_from_hex(json.load(f))


def make_tile(rng, H, W, ncls=9):
    """A base tile with raw values: class ids, rgb 0..255, ndvi -1..1, temperature in degrees C (fp32 planes)."""
    dw = rng.integers(0, ncls, (H, W)).astype(np.uint8)
    rgb = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    ndvi = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    temp = rng.uniform(5, 55, (H, W)).astype(np.float32)
    return dw, rgb, ndvi, temp


def make_canvas(rng, Hc, Wc, palette, transparent=0.3):
    """A random RGBA canvas: `transparent` of the pixels have alpha 0; of the painted ones a third are palette colours, a third
    random colours and a third sit EXACTLY midway between two palette colours (where both coordinates sums are even: an exact
    tie of the two distances), so that the first-minimum rule is exercised."""
    n = Hc * Wc
    rgb = rng.integers(0, 256, (n, 3))
    kind = rng.integers(0, 3, n)
    pick = rng.integers(0, len(palette), (n, 2))
    rgb[kind == 0] = palette[pick[kind == 0, 0]]
    a, b = palette[pick[:, 0]].astype(int), palette[pick[:, 1]].astype(int)
    even = ((a + b) % 2 == 0).all(axis=1) & (kind == 1)
    rgb[even] = ((a + b) // 2)[even]
    alpha = np.where(rng.random(n) < transparent, 0, rng.integers(1, 256, n))
    return np.concatenate([rgb, alpha[:, None]], axis=1).reshape(Hc, Wc, 4).astype(np.uint8)


@pytest.mark.parametrize("n_in", [1, 5, 199, 200, 511, 512, 777])
def test_nearest_index_table_is_pillows_rule(n_in):
    Image = pytest.importorskip("PIL.Image")
    from mau_amd import scenario as S
    ramp = np.arange(n_in, dtype=np.int32)
    for n_out in (1, 31, 250, 251, 512):
        want = S.nearest_index_table(n_in, n_out)
        assert want.dtype == np.int32 and want.shape == (n_out,)
        along_x = np.array(Image.fromarray(np.tile(ramp[None, :], (3, 1))).resize((n_out, 3), Image.NEAREST))
        along_y = np.array(Image.fromarray(np.tile(ramp[:, None], (1, 3))).resize((3, n_out), Image.NEAREST))
        assert np.array_equal(along_x[0], want) and np.array_equal(along_x[2], want), (n_in, n_out)
        assert np.array_equal(along_y[:, 0], want) and np.array_equal(along_y[:, 2], want), (n_in, n_out)
    with pytest.raises(ValueError):
        S.nearest_index_table(0, 4)


def class_map_by_cdist(canvas, shape, palette, keep=None):
    """Independent restatement of the canvas step with the libraries the app uses: Pillow resizes the RGBA image with nearest
    neighbour, scipy's ``cdist`` measures every resized pixel against the palette, ``argmin`` picks the class, and pixels the
    user left transparent fall back to ``keep`` when a map to keep is given."""
    from PIL import Image
    from scipy.spatial.distance import cdist
    h, w = shape
    small = np.asarray(Image.fromarray(canvas, mode="RGBA").resize((w, h), resample=Image.NEAREST))
    colours = small[..., :3].reshape(h * w, 3).astype(np.float64)
    winner = cdist(colours, palette.astype(np.float64)).argmin(axis=1).reshape(h, w).astype(np.uint8)
    if keep is None:
        return winner
    painted = small[..., 3] != 0
    merged = np.array(keep, dtype=np.uint8).reshape(h, w)
    merged[painted] = winner[painted]
    return merged


@pytest.mark.parametrize("canvas_shape,target", [((53, 41), (37, 300)), ((600, 91), (37, 300)), ((64, 64), (64, 64))])
def test_canvas_to_dw_map_matches_cdist_and_pillow(canvas_shape, target):
    pytest.importorskip("PIL")
    pytest.importorskip("scipy")
    from mau_amd import scenario as S
    palette = load_palette()
    rng = np.random.default_rng(3)
    canvas = make_canvas(rng, *canvas_shape, palette)
    dw = rng.integers(0, 9, target).astype(np.uint8)
    # the canvas does hold exact ties between two palette entries
    d = ((canvas[:, :, None, :3].astype(int) - palette[None, None].astype(int)) ** 2).sum(3)
    srt = np.sort(d, axis=2)
    assert (srt[:, :, 0] == srt[:, :, 1]).sum() >= 10 and (canvas[:, :, 3] == 0).mean() > 0.2
    got = S.canvas_to_dw_map_host(canvas, target, palette, dw)
    assert got.dtype == np.uint8 and np.array_equal(got, class_map_by_cdist(canvas, target, palette, dw))
    assert np.array_equal(S.canvas_to_dw_map_host(canvas, target, palette, dw[None]), got)                  # (1, H, W) original map
    assert np.array_equal(S.canvas_to_dw_map_host(canvas, target, palette), class_map_by_cdist(canvas, target, palette))
    with pytest.raises(ValueError):
        S.canvas_to_dw_map_host(canvas[:, :, :3], target, palette)


def test_prepare_input_is_the_float64_formula_bit_for_bit():
    from mau_amd import scenario as S
    palette = load_palette()
    rng = np.random.default_rng(4)
    H, W = 37, 60
    dw, rgb, ndvi, temp = make_tile(rng, H, W)
    canvas = make_canvas(rng, 53, 41, palette)
    got = S.prepare_input_host(dw, rgb, ndvi, temp, canvas, palette, METRICS)
    assert got.shape == (1, 23, H, W) and got.dtype == np.float32
    # numpy restatement of the dense input: every plane a float64 array, one rounding to float32 at the very end
    t2 = S.canvas_to_dw_map_host(canvas, (H, W), palette, original_map=dw)
    want64 = np.zeros((1, 23, H, W), dtype=np.float64)
    for k in range(9):
        want64[0, k] = dw == k
        want64[0, 14 + k] = t2 == k
    for c in range(3):
        want64[0, 9 + c] = (rgb[c].astype(np.float64) / 255.0 - METRICS["rgb_mean"][c]) / METRICS["rgb_std"][c]
    want64[0, 12] = ndvi
    want64[0, 13] = (temp.astype(np.float64) - METRICS["temp_mean"]) / METRICS["temp_std"]
    want = want64.astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(S.normalized_planes_host(rgb, ndvi, temp, METRICS).view(np.uint32), want[0, 9:14].view(np.uint32))
    with pytest.raises(ValueError):
        S.prepare_input_host(dw, rgb, ndvi, temp, canvas, palette, {"rgb_mean": [0, 0, 0]})


def test_metadata_row_and_temperature_series():
    from mau_amd import scenario as S
    lat, lon, population, year_t1, month_t1, year_t2, month_t2 = 48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9
    got = S.metadata_row(lat, lon, population, year_t1, month_t1, year_t2, month_t2, METRICS["meta_mean"], METRICS["meta_std"])
    # restatement: the first three entries and the span in years are z-scored in float64, the four date numbers follow as they are
    years = (year_t2 + month_t2 / 12.0) - (year_t1 + month_t1 / 12.0)
    want = np.empty((1, 8), dtype=np.float64)
    for k, v in enumerate((lat, lon, population, (year_t2 - year_t1) + (month_t2 - month_t1) / 12.0)):
        want[0, k] = (v - METRICS["meta_mean"][k]) / METRICS["meta_std"][k]
    want[0, 4:] = year_t1, month_t1, year_t2, month_t2
    want = want.astype(np.float32)
    assert abs(years - 3.5) < 1e-12
    assert got.shape == (1, 8) and got.dtype == np.float32 and np.array_equal(got, want)
    ts = np.linspace(-2.0, 3.0, 17)
    got = S.normalize_temp_series(ts, METRICS)
    assert got.shape == (1, 17) and got.dtype == np.float32
    want = np.array([[(float(v) - METRICS["temp_series_mean"]) / METRICS["temp_series_std"] for v in ts]], dtype=np.float64)
    assert np.array_equal(got, want.astype(np.float32))


def test_header_library_and_binding_carry_the_scenario_entry_points():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    want = {"mau_scenario_max_classes": 0, "mau_scenario_pack": 20, "mau_scenario_result_row_elems": 0,
            "mau_scenario_result_chunks": 2, "mau_scenario_result_ws_elems": 3, "mau_scenario_result": 16}
    syms, protos = header_symbols(), header_prototypes()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in want.items():
        assert name in syms and hasattr(so, name) and name in _lib.PROTOTYPES, name
        assert len(protos[name][1]) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert list(protos[name][1]) == list(_lib.PROTOTYPES[name][1]) and protos[name][0] is _lib.PROTOTYPES[name][0], name
    assert protos["mau_scenario_result"][1][4:6] == [ctypes.c_double, ctypes.c_double]
    assert protos["mau_scenario_result_ws_elems"][0] is ctypes.c_size_t
    assert _lib.lib.mau_abi_version() == 5


def test_scenario_size_helpers():
    import mau_amd  # noqa: F401
    from mau_amd._lib import lib
    assert lib.mau_scenario_result_row_elems() == 5 and lib.mau_scenario_max_classes() >= 9
    per = lib.mau_reduce_tickets_elems()
    for N, H, W in ((1, 1, 1), (1, 37, 300), (3, 37, 300), (1, 512, 512), (per + 3, 8, 8)):
        chunks = lib.mau_scenario_result_chunks(H, W)
        assert chunks >= 1 and (chunks - 1) * 4096 < H * W <= chunks * 4096
        assert lib.mau_scenario_result_ws_elems(N, H, W) == min(N, per) * chunks * 5 > 0
    assert lib.mau_scenario_result_chunks(512, 512) == 64
    for bad in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert lib.mau_scenario_result_ws_elems(*bad) == 0
    assert lib.mau_scenario_result_chunks(0, 5) == 0
    # a refused call reports through mau_last_error, without a device (argument validation comes first)
    assert lib.mau_scenario_result(None, None, None, None, 0.0, 1.0, None, None, None, None, None, None, 1, 8, 8, None) != 0
    assert b"scenario_result" in lib.mau_last_error()
    assert lib.mau_scenario_pack(*([None] * 10), 24, None, 1, 0, 8, 8, 8, 8, 9, None) != 0
    assert b"scenario_pack" in lib.mau_last_error()
