"""CPU-only checks of ``mau_amd.dataset_metrics``: the column order and the float64 twin against rows recorded from the reference's own
``extract_metrics`` (tests/golden/surveyfix*), the temperature-series branches, un-normalisation of the moments against per-pixel
float64 numpy, the dataset's ``skip_errors``, the command line's refusals, and the C entry point's bindings, size helpers and
refusals (called through ctypes with no device: every refusal comes before a launch).

The bound per column is ``2 * dev32[col] + 1e-10 * scale[col]``: dev32 is the reference's own float32-versus-float64 deviation on
the four fixture tiles and scale the column's largest magnitude there (tests/golden/surveyfix_deviation.json); the factor two is the
margin the project gives the reference's fp32 deviation, 1e-10 is test_gpu_ground_truth.TOL."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "surveyfix")
MAU_ERR_ARG = 1
TOL = 1e-10


@pytest.fixture(scope="module")
def D():
    from mau_amd import dataset_metrics
    return dataset_metrics


@pytest.fixture(scope="module")
def fixture():
    import pandas as pd
    expected = pd.read_csv(os.path.join(GOLDEN, "surveyfix_expected.csv"), float_precision="round_trip")
    deviation = json.load(open(os.path.join(GOLDEN, "surveyfix_deviation.json")))
    metrics = json.load(open(os.path.join(FIX, "normalization_metrics.json")))
    return expected, deviation, metrics


def assert_rows_match(got_rows, expected, deviation, what):
    """got_rows: {filepath: {column: value}} with ``split``; every numeric column within the bound of the module's docstring, NaN where
    the fixture is NaN, ``meta_*`` bit-equal.  Prints the worst column."""
    worst = (0.0, "")
    assert sorted(got_rows) == sorted(expected["filepath"])
    for _, ref in expected.iterrows():
        got = got_rows[ref["filepath"]]
        assert got["split"] == ref["split"]
        for col in expected.columns[2:]:
            r, g = float(ref[col]), float(got[col])
            if math.isnan(r) or math.isnan(g):
                assert math.isnan(r) and math.isnan(g), (what, ref["filepath"], col, r, g)
                continue
            if col.startswith("meta_"):
                assert g == r, (what, col, r, g)
            bound = 2 * deviation["dev32"][col] + TOL * deviation["scale"][col]
            assert abs(g - r) <= bound, (what, ref["filepath"], col, r, g, bound)
            if bound > 0:
                worst = max(worst, (abs(g - r) / bound, col))
    print(f"{what}: worst |difference| / bound = {worst[0]:.3g} ({worst[1]})")


def test_columns_are_the_fixture_csv_header(D):
    header = open(os.path.join(GOLDEN, "surveyfix_expected.csv")).readline().rstrip("\n").split(",")
    assert D.COLUMNS == header
    assert header[:2] == ["filepath", "split"] and len(header) == len(set(header)) == 148


def test_host_twin_against_the_reference_rows(D, fixture):
    expected, deviation, metrics = fixture
    assert deviation["source"].startswith("reference extract_metrics")
    got = {}
    for _, ref in expected.iterrows():
        z = np.load(os.path.join(FIX, ref["split"], ref["filepath"]))
        m = D.tile_metrics_host({k: z[k] for k in z.files}, metrics)
        assert list(m) == D.COLUMNS[2:]
        got[ref["filepath"]] = {"split": ref["split"], **m}
    assert sorted(len(np.load(os.path.join(FIX, r["split"], r["filepath"]))["temperature_serie"]) for _, r in expected.iterrows()) == [1, 13, 24, 24]
    assert int(expected["temp_series_autocorr_1"].isna().sum()) == 2 and int(expected["temp_series_seasonal_amplitude"].isna().sum()) == 1
    assert_rows_match(got, expected, deviation, "tile_metrics_host vs the reference's rows")


def test_temperature_series_branches(D):
    s = D.series_metrics(np.array([]))
    assert math.isnan(s["mean"]) and s["std"] == 0.0 and s["slope"] == 0.0 and math.isnan(s["autocorr_1"]) and math.isnan(s["seasonal_amplitude"])
    s = D.series_metrics(np.array([301.5]))
    assert s["mean"] == 301.5 and s["std"] == 0.0 and s["slope"] == 0.0 and math.isnan(s["autocorr_1"]) and math.isnan(s["seasonal_amplitude"])
    s = D.series_metrics(np.full(24, 299.171875))                     # constant, longer than a year
    assert s["mean"] == 299.171875 and s["std"] == 0.0 and s["slope"] == 0.0 and math.isnan(s["autocorr_1"])
    assert abs(s["seasonal_amplitude"]) < 1e-10
    s = D.series_metrics(np.full(5, 2.5))                             # constant and short
    assert s["slope"] == 0.0 and math.isnan(s["autocorr_1"]) and math.isnan(s["seasonal_amplitude"])
    x = np.array([1.0, 3.0, 2.0, 5.0, 4.0, 7.0, 6.0, 9.0, 8.0, 11.0, 10.0, 13.0])    # 12 values: no seasonal amplitude
    s = D.series_metrics(x)
    t = np.arange(12.0)
    slope = np.sum((t - t.mean()) * (x - x.mean())) / np.sum((t - t.mean()) ** 2)
    assert math.isnan(s["seasonal_amplitude"]) and abs(s["slope"] - slope) < 1e-12 and abs(s["mean"] - x.mean()) < 1e-15
    assert abs(s["std"] - x.std()) < 1e-15 and abs(s["autocorr_1"] - np.corrcoef(x[1:], x[:-1])[0, 1]) < 1e-14
    t = np.arange(36)                                                 # a pure annual wave of amplitude 3 on a trend
    x = 3.0 * np.sin(2 * np.pi * t / 12.0) + 0.5 * t + 280.0
    s = D.series_metrics(x)
    resid = x - np.polyval(np.polyfit(t, x, 1), t)                    # 36 monthly values: bin 3 of the transform is one cycle per year
    assert abs(s["seasonal_amplitude"] - 2.0 / 36 * abs(np.sum(resid * np.exp(-2j * np.pi * 3 * t / 36)))) < 1e-12
    ls = np.sum((t - t.mean()) * (x - x.mean())) / np.sum((t - t.mean()) ** 2)      # the fitted line takes a little of the wave
    assert abs(s["slope"] - ls) < 1e-12 and 0.4 < ls < 0.5 and 2.5 < s["seasonal_amplitude"] < 3.0
    s = D.series_metrics(np.array([4.0, 6.0]))                        # one pair: 0 / 0
    assert abs(s["slope"] - 2.0) < 1e-12 and math.isnan(s["autocorr_1"])


def dense_sample(rng, hw=(11, 13)):
    H, W = hw
    eye = np.eye(9, dtype=np.float32)
    a, b = rng.choice([0, 1, 3, 6, 8], (H, W)), rng.choice([1, 6, 7], (H, W))
    cont = np.concatenate([rng.uniform(0, 1, (3, H, W)), np.tanh(rng.standard_normal((1, H, W))), rng.standard_normal((1, H, W))])
    x = np.vstack([eye[a].transpose(2, 0, 1), cont.astype(np.float32), eye[b].transpose(2, 0, 1)]).astype(np.float32)
    y = np.stack([np.tanh(rng.standard_normal((H, W))), cont[4] + 0.2 * rng.standard_normal((H, W))]).astype(np.float32)
    return {"input": x, "target": y, "metadata": rng.standard_normal(4).astype(np.float32),
            "temperature_serie": rng.standard_normal(17).astype(np.float32)}


@pytest.mark.parametrize("temp_std", [11.0291, -3.5])
def test_moment_unnormalisation_against_per_pixel_float64(D, temp_std):
    """scale * mean, |scale| * std, min / max swapped for a negative scale, |scale| * sum |x|, |scale| * sqrt(M2 + n mean^2)."""
    metrics = {"temp_mean": 296.4173, "temp_std": temp_std, "temp_series_mean": 295.75, "temp_series_std": 9.125,
               "meta_mean": [17.25, 9.5, 1250000.5, 2.125], "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
    s = dense_sample(np.random.default_rng(3))
    m = D.tile_metrics_host(s, metrics)
    x, y = s["input"].astype(np.float64), s["target"].astype(np.float64)
    td = (y[1] - x[13]) * temp_std                                    # the + temp_mean of both cancels
    nd = y[0] - x[12]
    for name, v in (("temp_diff", td), ("ndvi_diff", nd)):
        rms = math.sqrt(float(np.mean(v ** 2)))
        for k, want in (("mean", v.mean()), ("std", v.std()), ("min", v.min()), ("max", v.max())):
            assert abs(m[f"{name}_{k}"] - want) <= 1e-13 * rms, (name, k)
    assert abs(m["delta_temp_l1_norm"] - np.abs(td).sum()) <= 1e-13 * np.abs(td).sum()
    assert abs(m["delta_temp_l2_norm"] - math.sqrt(np.sum(td ** 2))) <= 1e-13 * math.sqrt(np.sum(td ** 2))
    assert abs(m["delta_ndvi_l2_norm"] - math.sqrt(np.sum(nd ** 2))) <= 1e-13 * math.sqrt(np.sum(nd ** 2))
    # the one-hot planes' statistics from the counts, against the dense planes
    names = [f"dw_t1_{c}" for c in D.DW_CLASS_NAMES] + D.CONT_NAMES + [f"dw_t2_{c}" for c in D.DW_CLASS_NAMES]
    for i, name in enumerate(names):
        for k, want in (("mean", x[i].mean()), ("std", x[i].std()), ("min", x[i].min()), ("max", x[i].max())):
            assert abs(m[f"input_{name}_{k}"] - want) <= 1e-14, (name, k)
    p1, p2 = x[:9].mean(axis=(1, 2)), x[14:].mean(axis=(1, 2))
    assert abs(m["dw_t1_entropy"] - -np.sum(p1[p1 > 0] * np.log2(p1[p1 > 0]))) <= 1e-14
    assert abs(m["dw_diff_std"] - (p2 - p1).std()) <= 1e-15 and abs(m["dw_diff_max"] - (p2 - p1).max()) <= 1e-15
    assert m["meta_population"] == float(s["metadata"][2] * np.float64(4900000.25) + np.float64(1250000.5))
    assert m["pop_density_proxy"] == m["meta_population"] / (p1[6] + 1e-9)


def test_twin_rows_hold_nan_and_out_of_range_counts(D):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 9, (1, 5, 7)).astype(np.uint8)
    b = a.copy()
    b[0, 2, 3] = 9
    cont = rng.standard_normal((1, 5, 5, 7)).astype(np.float32)
    tgt = rng.standard_normal((1, 2, 5, 7)).astype(np.float32)
    cont[0, 3, 1, 1] = np.nan
    tgt[0, 1, 0, 0] = np.inf
    rows = D.tile_rows_host(a, b, cont, tgt)
    assert rows.shape == (1, D.ROW) and rows[0, D.OOR] == 0 and rows[0, D.OOR + 1] == 1
    assert rows[0, :9].sum() == 35 and rows[0, 16:25].sum() == 34 and rows[0, 9:16].sum() == 0
    planes = rows[0, D.PLANES0:].reshape(9, 8)
    assert planes[:, D.P_NAN].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0] and planes[:, D.P_BAD].tolist() == [0, 0, 0, 1, 0, 0, 1, 1, 1]
    assert math.isnan(planes[3, D.P_MEAN]) and not math.isnan(planes[3, D.P_MIN]) and planes[6, D.P_MAX] == np.inf
    with pytest.raises(ValueError, match="outside"):
        D.check_class_range(rows)
    m = D.sample_metrics(rows, np.zeros((1, 4), np.float32), np.zeros((1, 3), np.float32), [3],
                         {"temp_std": 2.0, "temp_mean": 1.0, "temp_series_std": 1.0, "temp_series_mean": 0.0, "meta_std": [1.0] * 4, "meta_mean": [0.0] * 4})[0]
    for k in ("mean", "std", "min", "max"):                           # np.min / np.max of a plane with a NaN: NaN
        assert math.isnan(m[f"input_ndvi_t1_{k}"]) and math.isnan(m[f"ndvi_diff_{k}"])
    assert math.isnan(m["delta_ndvi_l1_norm"]) and math.isnan(m["delta_ndvi_l2_norm"]) and m["temp_diff_max"] == np.inf


def test_dataset_skip_errors_leaves_existing_callers_alone(D, tmp_path, capsys):
    from mau_amd.data import FuturePredictionDataset, collate_fn
    rng = np.random.default_rng(6)
    d = tmp_path / "p" / "test"
    d.mkdir(parents=True)
    good, bad = dense_sample(rng), dense_sample(rng)
    bad["input"][0] *= 0.5                                            # not one-hot
    np.savez_compressed(d / "A_0_1.0_2.0_2019_08_to_2021_08.npz", **good)
    np.savez_compressed(d / "B_1_1.0_2.0_2019_08_to_2021_08.npz", **bad)
    (d / "C_2_1.0_2.0_2019_08_to_2021_08.npz").write_bytes(b"not a zip file")
    ds = FuturePredictionDataset("test", processed_dir=str(tmp_path / "p"))
    assert len(ds) == 3 and "filepath" not in ds[0]
    with pytest.raises(ValueError, match="one-hot"):
        ds[1]
    with pytest.raises(Exception):
        ds[2]
    ds = FuturePredictionDataset("test", processed_dir=str(tmp_path / "p"), skip_errors=True)
    samples = [ds[i] for i in range(3)]
    out = capsys.readouterr().out
    assert samples[0]["filepath"] == "A_0_1.0_2.0_2019_08_to_2021_08.npz" and samples[1] is None and samples[2] is None
    assert f"Failed to process {d / 'B_1_1.0_2.0_2019_08_to_2021_08.npz'}: compact_input" in out
    assert f"Failed to process {d / 'C_2_1.0_2.0_2019_08_to_2021_08.npz'}: " in out
    batch = collate_fn(samples)
    assert batch.cls_a.shape == (1, 11, 13) and batch.temp_series_lengths.tolist() == [17]
    files = D._collate(samples)[1]
    assert files == ["A_0_1.0_2.0_2019_08_to_2021_08.npz"] and D._collate([None, None]) == (None, [])


def test_command_line_refusals_come_before_the_device(D, tmp_path, capsys):
    import torch
    was_initialised = torch.cuda.is_initialized()                     # true only when device tests ran earlier in this process
    (tmp_path / "train").mkdir()
    assert D.main(["extract", str(tmp_path), str(tmp_path / "out.csv")]) == 1
    out = capsys.readouterr().out
    assert "Error: Normalization metrics not found at" in out and "normalization_metrics.json" in out
    assert D.main(["extract", str(tmp_path), str(tmp_path / "out.csv"), "--metrics-json", str(tmp_path / "nowhere.json")]) == 1
    assert "nowhere.json" in capsys.readouterr().out
    with pytest.raises(FileNotFoundError, match="Normalization metrics"):
        D.extract(str(tmp_path))
    assert torch.cuda.is_initialized() == was_initialised and not os.path.exists(tmp_path / "out.csv")      # nothing touched the device
    with pytest.raises(SystemExit) as e:
        D.main(["extract", str(tmp_path), str(tmp_path / "out.csv"), "--device", "cpu"])
    assert e.value.code == 2 and "no CPU fallback" in capsys.readouterr().err
    json.dump({}, open(tmp_path / "normalization_metrics.json", "w"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.extract(str(tmp_path), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):    # the wrapper: host tensors are refused, not computed
        D.tile_stats(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 5, 4, 4),
                     torch.zeros(1, 2, 4, 4))
    with pytest.raises(TypeError):
        D.tile_stats(np.zeros((1, 4, 4), np.uint8), None, None, None)
    import mau_amd
    assert mau_amd.dataset_metrics is D and "dataset_metrics" in mau_amd.__all__


def test_entry_point_bindings_sizes_and_refusals(D):
    from mau_amd import _lib
    lib = _lib.lib
    for name, nargs in (("mau_tile_stats_row_elems", 0), ("mau_tile_stats_ws_elems", 2), ("mau_tile_stats", 11)):
        assert nargs == len(_lib.PROTOTYPES[name][1]) and hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    assert _lib.PROTOTYPES["mau_tile_stats_ws_elems"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64])
    assert _lib.PROTOTYPES["mau_tile_stats"][1][7:10] == [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    assert lib.mau_abi_version() == 5
    R = lib.mau_tile_stats_row_elems()
    assert R == D.ROW == 2 * 16 + 2 + 9 * 8
    per = lib.mau_reduce_tickets_elems()
    ws = lib.mau_tile_stats_ws_elems
    assert ws(3, 62500) == 3 * 16 * R and ws(1, 4096) == R and ws(1, 4097) == 2 * R and ws(per + 5, 62500) == per * 16 * R
    assert ws(0, 64) == 0 and ws(2, 0) == 0 and ws(-1, 64) == 0 and ws(1, (1 << 30) + 1) == 0
    assert D.CHUNK_PIX * lib.mau_plane_moments_chunks(62500) >= 62500               # the chunking of mau_plane_moments

    buf = (ctypes.c_double * 64)()                                   # host memory standing in for pointers that are never followed
    p = ctypes.addressof(buf)

    def refused(status, word):
        msg = lib.mau_last_error().decode()
        assert status == MAU_ERR_ARG and "tile_stats" in msg and word in msg, (status, msg)

    for k in range(7):
        args = [p] * 7
        args[k] = None
        refused(lib.mau_tile_stats(*args, 2, 64, 9, None), "null pointer")
    for B, HW in ((0, 64), (2, 0), (-1, 64), (2, -4)):
        refused(lib.mau_tile_stats(*[p] * 7, B, HW, 9, None), "non-positive")
    refused(lib.mau_tile_stats(*[p] * 7, 1, (1 << 30) + 1, 9, None), "2^30")
    for nc in (0, 17, -1):
        refused(lib.mau_tile_stats(*[p] * 7, 1, 64, nc, None), "num_classes")
    refused(lib.mau_tile_stats(p, p, p + 2, p, p, p, p, 1, 64, 9, None), "aligned")
    refused(lib.mau_tile_stats(p, p, p, p + 1, p, p, p, 1, 64, 9, None), "aligned")
    refused(lib.mau_tile_stats(p, p, p, p, p + 4, p, p, 1, 64, 9, None), "aligned")
