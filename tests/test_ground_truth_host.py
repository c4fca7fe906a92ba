"""CPU-only checks of ``mau_amd.ground_truth``: the bin edges against the reference's literal expression, the float64 host twin
against pooled numpy statistics, ``np.digitize``'s corner cases, the pairwise merge, the export layout, and the refusals of the two
new entry points (called through ctypes with no device: every refusal comes before a launch)."""
import ctypes
import json
import math

import numpy as np
import pytest

METRICS = {"temp_mean": 29.4173, "temp_std": 11.0291, "meta_mean": [17.25, 9.5, 1250000.5, 2.125],
           "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
CHANNELS = ("after_ndvi", "after_temp")
MAU_ERR_ARG = 1


@pytest.fixture(scope="module")
def G():
    from mau_amd import ground_truth
    return ground_truth


def test_bin_edges_are_the_references_expression(G):
    for bin_centers in (np.linspace(-60, 70, 50), np.linspace(-180, 180, 50), np.array([0.0, 1.0, 2.0, 3.0]), np.array([1.0, 1.5, 4.0])):
        edges = np.concatenate([                                     # generate_ground_truth_sensitivity.py:107-111, verbatim
            [bin_centers[0] - (bin_centers[1] - bin_centers[0])/2],
            (bin_centers[:-1] + bin_centers[1:]) / 2,
            [bin_centers[-1] + (bin_centers[-1] - bin_centers[-2])/2]
        ])
        got = G.bin_edges(bin_centers)
        assert got.dtype == np.float64 and np.array_equal(got, edges)
    assert np.array_equal(G.LAT_RANGE, np.linspace(-60, 70, 50)) and np.array_equal(G.LON_RANGE, np.linspace(-180, 180, 50))
    assert np.array_equal(G.bin_edges([0, 1, 2, 3]), [-0.5, 0.5, 1.5, 2.5, 3.5])
    with pytest.raises(ValueError):
        G.bin_edges([1.0])


def test_bin_stats_host_against_pooled_numpy(G):
    rng = np.random.default_rng(11)
    n = 60
    coords = rng.uniform(-75, 85, n)                                 # some outside [-61.3, 71.3]
    planes = (300.0 + 7.0 * rng.standard_normal((n, 9, 7))) * rng.uniform(0.5, 1.5, (n, 1, 1))
    means, stds, counts = G.bin_stats_host(coords, planes, G.LAT_RANGE)
    edges = G.bin_edges(G.LAT_RANGE)
    idx = np.digitize(coords, edges)
    assert len(means) == len(stds) == len(counts) == 50
    assert sum(counts) == int(((idx >= 1) & (idx <= 50)).sum()) < n
    seen = 0
    for i in range(1, 51):
        mask = idx == i
        assert counts[i - 1] == int(mask.sum())
        if mask.any():
            vals = planes[mask]                                       # all pixels of all samples of the bin, float64
            rms = math.sqrt(float(np.mean(vals ** 2)))
            assert abs(means[i - 1] - float(np.mean(vals))) <= 1e-13 * rms
            assert abs(stds[i - 1] - float(np.std(vals))) <= 1e-13 * rms
            seen += 1
        else:
            assert math.isnan(means[i - 1]) and math.isnan(stds[i - 1])
    assert 10 < seen < 50


def test_digitize_corner_cases_through_the_host_twin(G):
    centers = [0.0, 1.0, 2.0, 3.0]                                   # edges -0.5, 0.5, 1.5, 2.5, 3.5: exact
    coords = np.array([-0.5, 0.5, 3.5, -0.6, np.nan, 2.5 - 1e-12])
    planes = np.arange(6, dtype=np.float64)[:, None] * np.ones((1, 4)) + 10.0
    means, stds, counts = G.bin_stats_host(coords, planes, centers)
    assert counts == [1, 1, 1, 0]                                    # first edge: bin 0; on an edge: the upper bin; the last edge, below, NaN: dropped
    assert means[:3] == [10.0, 11.0, 15.0] and math.isnan(means[3])
    assert stds[:3] == [0.0, 0.0, 0.0] and math.isnan(stds[3])
    # a NaN pixel: its bin is NaN in both, the others are untouched
    planes[1, 2] = np.nan
    means, stds, counts = G.bin_stats_host(coords, planes, centers)
    assert counts == [1, 1, 1, 0] and math.isnan(means[1]) and math.isnan(stds[1]) and means[0] == 10.0 and stds[2] == 0.0


def test_pairwise_merge_is_associative_and_matches_the_pooled_set(G):
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        sets = [rng.normal(rng.uniform(-300, 300), rng.uniform(0.01, 30), int(rng.integers(1, 400))) for _ in range(3)]
        a, b, c = [(float(len(s)), float(np.mean(s)), float(np.sum((s - np.mean(s)) ** 2))) for s in sets]
        left = G.merge_moments(G.merge_moments(a, b), c)
        right = G.merge_moments(a, G.merge_moments(b, c))
        allv = np.concatenate(sets)
        pooled = (float(len(allv)), float(np.mean(allv)), float(np.sum((allv - np.mean(allv)) ** 2)))
        rms = math.sqrt(float(np.mean(allv ** 2)))
        for x, y in ((left, right), (left, pooled)):
            assert x[0] == y[0]
            dm = abs(x[1] - y[1]) / rms
            ds = abs(math.sqrt(x[2] / x[0]) - math.sqrt(y[2] / y[0])) / rms
            worst = max(worst, dm, ds)
    print("merge: worst deviation relative to the RMS", worst)
    assert worst <= 1e-14
    assert G.merge_moments((0.0, 0.0, 0.0), (3.0, 2.5, 0.75)) == (3.0, 2.5, 0.75)      # an empty left side: the right side as it is


def _host_result(G, rng, n=40):
    lat, lon = rng.uniform(-10, 30, n), rng.uniform(-170, 170, n)
    t = rng.standard_normal((n, 2, 6, 5))
    scale, shift = G.channel_affine(CHANNELS, METRICS)
    assert scale == [1.0, METRICS["temp_std"]] and shift == [0.0, METRICS["temp_mean"]]
    res = {}
    for name, x, centers in (("latitude", lat, G.LAT_RANGE), ("longitude", lon, G.LON_RANGE)):
        per = [G.bin_stats_host(x, t[:, c] * scale[c] + shift[c], centers) for c in range(2)]
        res[name] = {"x": centers, "mean": np.array([p[0] for p in per]), "std": np.array([p[1] for p in per]), "count": np.array(per[0][2])}
    return res


def test_export_layout_and_save_roundtrip(G, tmp_path):
    res = _host_result(G, np.random.default_rng(3))
    data = G.export_dict(res, CHANNELS)
    assert set(data) == {"model_name", "model_type", "sweeps", "heatmaps"}
    assert data["model_name"] == "Ground Truth (Dataset)" and data["model_type"] == "dataset" and data["heatmaps"] == {}
    assert set(data["sweeps"]) == {"latitude", "longitude"}
    for axis, centers in (("latitude", G.LAT_RANGE), ("longitude", G.LON_RANGE)):
        sw = data["sweeps"][axis]
        assert set(sw) == {"x", "channels"} and sw["x"] == centers.tolist() and len(sw["x"]) == 50
        assert list(sw["channels"]) == list(CHANNELS)
        for ch in CHANNELS:
            assert set(sw["channels"][ch]) == {"mean", "std"}
            m, s = sw["channels"][ch]["mean"], sw["channels"][ch]["std"]
            assert len(m) == len(s) == 50 and all(type(v) is float for v in m + s)
            empty = [i for i in range(50) if res[axis]["count"][i] == 0]
            assert empty and all(math.isnan(m[i]) and math.isnan(s[i]) for i in empty)
            assert all(not math.isnan(m[i]) for i in range(50) if i not in empty)
    path = G.save(data, str(tmp_path / "reports" / "sensitivity"))
    assert path.endswith("sensitivity_data_ground_truth.json")
    text = open(path).read()
    assert "NaN" in text and text.startswith("{\n    \"model_name\"")                 # indent = 4, NaN as Python writes it
    back = json.load(open(path))
    assert set(back) == set(data) and back["sweeps"]["latitude"]["x"] == data["sweeps"]["latitude"]["x"]
    for axis in ("latitude", "longitude"):
        for ch in CHANNELS:
            for k in ("mean", "std"):
                assert np.array_equal(back["sweeps"][axis]["channels"][ch][k], data["sweeps"][axis]["channels"][ch][k], equal_nan=True)


def test_missing_metrics_file_is_an_error(G, tmp_path):
    with pytest.raises(FileNotFoundError, match="normalization_metrics.json"):
        G.ground_truth_sensitivity(str(tmp_path))
    assert G.main(["--processed-dir", str(tmp_path), "--output-dir", str(tmp_path / "out")]) == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.BinStats([G.Axis("latitude", 0, G.LAT_RANGE)], 2, "cpu")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers and non-positive sizes: MAU_ERR_ARG and a message, with no device in the process."""
    from mau_amd import _lib
    lib = _lib.lib
    assert lib.mau_moments_row_elems() == 4
    assert lib.mau_plane_moments_chunks(250 * 250) == 16 and lib.mau_plane_moments_chunks(4096) == 1 and lib.mau_plane_moments_chunks(4097) == 2
    assert lib.mau_plane_moments_chunks(1) == 1 and lib.mau_plane_moments_chunks(0) == 0 and lib.mau_plane_moments_chunks(-5) == 0
    per = lib.mau_reduce_tickets_elems()
    assert lib.mau_plane_moments_ws_elems(3, 2, 62500) == 6 * 16 * 4
    assert lib.mau_plane_moments_ws_elems(256, 2, 62500) == per * 16 * 4             # the launches of a call share the first one's partials
    assert lib.mau_plane_moments_ws_elems(0, 2, 62500) == 0 and lib.mau_plane_moments_ws_elems(2, 0, 62500) == 0
    assert lib.mau_plane_moments_ws_elems(2, 2, 0) == 0
    buf = (ctypes.c_double * 64)()                                   # host memory standing in for pointers that are never followed
    p = ctypes.addressof(buf)

    def refused(status, word):
        msg = lib.mau_last_error().decode()
        assert status == MAU_ERR_ARG and word in msg, (status, msg)

    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        refused(lib.mau_plane_moments(*args, 2, 2, 64, None), "null pointer")
    for B, C, HW in ((0, 2, 64), (2, 0, 64), (2, 2, 0), (-1, 2, 64)):
        refused(lib.mau_plane_moments(p, p, p, p, B, C, HW, None), "non-positive")
    refused(lib.mau_plane_moments(p, p, p, p, 1, 1, (1 << 30) + 1, None), "2^30")
    refused(lib.mau_plane_moments(p + 2, p, p, p, 1, 1, 64, None), "aligned")

    cols, std, mean = (ctypes.c_int * 2)(0, 1), (ctypes.c_double * 2)(1.0, 1.0), (ctypes.c_double * 2)(0.0, 0.0)
    assert lib.mau_bin_moments_max_entries() >= 2 * 50 * 2
    good = [p, p, 4, cols, std, mean, p, p, 8, 2, 2, 50]
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[k] = None
        refused(lib.mau_bin_moments(*args, None), "null pointer")
    for k in (8, 9, 11):                                             # B, C, bins
        args = list(good)
        args[k] = 0
        refused(lib.mau_bin_moments(*args, None), "non-positive")
    for axes in (0, 5):
        args = list(good)
        args[10] = axes
        refused(lib.mau_bin_moments(*args, None), "axes")
    args = list(good)
    args[11] = lib.mau_bin_moments_max_entries() // 4 + 1            # 2 axes x 2 channels x bins: one entry too many
    refused(lib.mau_bin_moments(*args, None), "entries")
    args = list(good)
    args[2] = 0
    refused(lib.mau_bin_moments(*args, None), "pitch")
    args = list(good)
    args[2] = 1                                                      # column 1 of axis 1 is outside a row of one float
    refused(lib.mau_bin_moments(*args, None), "outside")
