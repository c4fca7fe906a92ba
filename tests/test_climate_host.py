"""``mau_amd.climate`` without a device: the float64 twins against the fixture of the reference's arithmetic
(tests/golden/make_climatefix.py -> tests/golden/climatefix, climatefix_deviation.json), ``process(device="cpu")`` end to end, the
queries, the twins' edge cases, the C entry points' bindings and refusals (called through ctypes with no device: every refusal
comes before a launch), the command line.

The fixture.  The reference (``src/data/process_temperature.py``) works through xarray, which is not available where the fixture is
made: what is recorded is its arithmetic in numpy -- float32 ``np.nanmean`` / ``np.nanstd(ddof=0)`` along time, then float32
``(tas - mean) / std`` -- which is what xarray dispatches to without bottleneck.  It is UNVERIFIED against xarray itself.

Bound per value of the baseline mean, the baseline std and the anomalies: ``2 * dev + 1e-10 * scale`` -- dev is the recorded
arithmetic's own deviation from the float64 twin on the fixture (float32 sums and float32 coefficients: up to 1e-5), the factor two
the margin the project gives it (tests/test_dataset_build_host.py), 1e-10 test_gpu_ground_truth.TOL relative to the value's scale.  NaN
positions are identical.  Query results are bit for bit the twin's grid."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

from tests._helpers import bits
from tests.test_dataset_build_host import MAU_ERR_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "climatefix")
TOL = 1e-10
BASELINE_YEARS, YEARS = (1901, 1904), (1951, 1953)


@pytest.fixture(scope="module")
def CL():
    import mau_amd
    return mau_amd.climate


def recorded_queries():
    return json.load(open(os.path.join(FIX, "queries.json")))


def make_grid(T, G, seed, nan=0.1):
    """A seeded (T, G) float32 grid in degrees (cell means -20 .. 30, |mean| >> std in many cells) with about ``nan`` of the values NaN."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-20, 30, (1, G)) + rng.uniform(0.3, 8, (1, G)) * rng.standard_normal((T, G))).astype(np.float32)
    x[rng.random((T, G)) < nan] = np.nan
    return x


@pytest.fixture(scope="module")
def twin(CL):
    """The fixture's years through the twins: baseline grid, raw grid, rows, anomalies."""
    base, lats, lons = CL.read_years(FIX, *BASELINE_YEARS)
    raw, _, _ = CL.read_years(FIX, *YEARS, (lats, lons))
    rows = CL.baseline_host(base)
    return {"base": base, "raw": raw, "lats": lats, "lons": lons, "rows": rows, "norm": CL.normalise_host(raw, rows)}


@pytest.fixture(scope="module")
def processed(CL, tmp_path_factory):
    out = tmp_path_factory.mktemp("climate") / "processed"
    return CL.process(FIX, str(out), BASELINE_YEARS, YEARS, "cpu"), str(out)


# --------------------------------------------------------------------------- #
# the twins against the recorded arithmetic
# --------------------------------------------------------------------------- #
def test_read_year_and_the_reference_file_stem(CL, twin):
    path = CL.year_path(FIX, 1951)
    assert os.path.basename(path) == "CRU_mean_temperature_mon_0.5x0.5_global_1951_v4.03.npz"
    tas, lats, lons = CL.read_year(path)
    assert tas.shape == (12, 6, 8) and tas.dtype == np.float32 and lats.shape == (6,) and lons.shape == (8,)
    assert twin["base"].shape == (48, 6, 8) and twin["raw"].shape == (36, 6, 8) and np.array_equal(bits(twin["raw"][:12]), bits(tas))
    with pytest.raises(FileNotFoundError, match="global_1950_v4.03"):
        CL.year_path(FIX, 1950)


def test_twin_within_the_recorded_deviation(CL, twin):
    deviation = json.load(open(os.path.join(GOLDEN, "climatefix_deviation.json")))
    assert deviation["source"].startswith("float32 np.nanmean / np.nanstd(ddof=0)") and "unverified against xarray" in deviation["source"]
    expected = json.load(open(os.path.join(FIX, "expected_baseline.json")))
    with np.load(os.path.join(FIX, "expected_tas_norm.npz")) as z:
        want_norm = z["data"]
        assert np.array_equal(z["lats"], twin["lats"]) and np.array_equal(z["lons"], twin["lons"]) and int(z["start_year"]) == 1951
    assert want_norm.dtype == np.float32 and twin["norm"].dtype == np.float32 and want_norm.shape == twin["norm"].shape == (36, 6, 8)
    rows = twin["rows"]
    got = {"mean": rows[:, CL.R_MEAN].reshape(6, 8), "std": CL.baseline_std(rows).reshape(6, 8), "anomaly": twin["norm"].astype(np.float64)}
    want = {"mean": np.array(expected["mean"], dtype=np.float64), "std": np.array(expected["std"], dtype=np.float64),
            "anomaly": want_norm.astype(np.float64)}
    for k in ("mean", "std", "anomaly"):
        dev, scale = np.array(deviation["dev"][k]), np.array(deviation["scale"][k])
        nan = np.isnan(want[k])
        assert np.array_equal(nan, np.isnan(got[k])), k                             # the same NaN positions
        d = np.where(nan, 0.0, np.abs(want[k] - got[k]))
        print(f"{k}: |recorded - twin| {np.max(d):.3g} (recorded deviation {np.max(dev):.3g})")
        assert d.shape == dev.shape == scale.shape and np.all(d <= 2 * dev + TOL * scale), (k, float(np.max(d)))
        assert np.all(np.abs(d - dev) <= TOL * scale), k                            # the deviation file is re-derivable
    assert 1e-8 < np.max(deviation["dev"]["anomaly"]) < 1e-4 and 1e-8 < np.max(deviation["dev"]["mean"]) < 1e-4
    assert int(np.isnan(want["mean"]).sum()) == 2 and int(np.isnan(want["anomaly"]).sum()) == 2 * 36 + 1
    assert rows[2 * 8 + 2].tolist()[0::3] == [44.0, 4.0] and np.all(rows[[0, 3 * 8 + 5], 0] == 0)     # the partly-NaN cell; the ocean


def test_queries_are_the_twins_grid_bit_for_bit(CL, twin):
    cq = CL.ClimateQuery(twin["raw"], twin["rows"], twin["lats"], twin["lons"], 1951)
    dev = np.array(json.load(open(os.path.join(GOLDEN, "climatefix_deviation.json")))["dev"]["anomaly"])
    qs = recorded_queries()
    assert len(qs) == 6 and [q["keep"] for q in qs] == [19, 36, 36, 13, 26, 1]
    for q in qs:
        got = cq.query(q["lat"], q["lon"], q["year"], q["month"])
        i, j, keep = q["lat_index"], q["lon_index"], q["keep"]
        assert isinstance(got, list) and len(got) == keep and all(isinstance(v, float) for v in got)
        assert np.array_equal(bits(np.array(got, dtype=np.float32)), bits(twin["norm"][:keep, i, j])), q
        want = np.array(q["series"], dtype=np.float64)
        assert np.array_equal(np.isnan(want), np.isnan(got))
        d = np.where(np.isnan(want), 0.0, np.abs(want - np.array(got)))
        assert np.all(d <= 2 * dev[:keep, i, j] + TOL * np.maximum(1.0, np.nan_to_num(np.abs(want)))), q
    # all six at once: the same rows, zero padding, the lengths
    out, lengths, srows = cq.query_batch(*([q[k] for q in qs] for k in ("lat", "lon", "year", "month")), Tpad=40)
    assert out.shape == (6, 40) and out.dtype == np.float32 and lengths.tolist() == [q["keep"] for q in qs] and srows.shape == (6, 4)
    for n, q in enumerate(qs):
        assert np.array_equal(bits(out[n, :q["keep"]]), bits(twin["norm"][:q["keep"], q["lat_index"], q["lon_index"]]))
        assert not out[n, q["keep"]:].any()
    assert srows[:, 0].tolist() == [19, 36, 36, 13, 26, 1] and srows[:, 3].tolist() == [0, 0, 0, 13, 1, 0]


# --------------------------------------------------------------------------- #
# process, end to end
# --------------------------------------------------------------------------- #
def test_process_on_the_cpu_end_to_end(CL, twin, processed, capsys):
    from mau_amd.dataset_build import ArrayTemperatureQuery
    res, out = processed
    assert res["skipped"] is False and sorted(os.listdir(out)) == ["baseline_metrics.json", "tas_norm.npz"]
    with np.load(res["tas_norm"]) as z:
        assert sorted(z.files) == ["data", "lats", "lons", "start_year"] and z["data"].dtype == np.float32
        assert np.array_equal(bits(z["data"]), bits(twin["norm"])) and int(z["start_year"]) == 1951
    text = open(res["baseline_metrics"]).read()
    metrics = json.loads(text)
    assert list(metrics) == ["mean", "std"] and "NaN" in text
    # json keeps every finite double exactly and a NaN as "NaN" (without its sign)
    assert np.array_equal(np.array(metrics["mean"]), twin["rows"][:, CL.R_MEAN].reshape(6, 8), equal_nan=True)
    assert np.array_equal(np.array(metrics["std"]), CL.baseline_std(twin["rows"]).reshape(6, 8), equal_nan=True)
    # the file dataset_build reads, queried by dataset_build's own class, against the resident query
    tq = ArrayTemperatureQuery.from_npz(res["tas_norm"])
    cq = CL.ClimateQuery(twin["raw"], None, twin["lats"], twin["lons"], 1951)      # rows = None: the baseline of the raw grid itself ...
    assert not np.array_equal(bits(cq.rows), bits(twin["rows"]))
    cq = CL.ClimateQuery(twin["raw"], twin["rows"], twin["lats"], twin["lons"], 1951)
    for q in recorded_queries():
        a, b = tq.query(q["lat"], q["lon"], q["year"], q["month"]), cq.query(q["lat"], q["lon"], q["year"], q["month"])
        assert len(a) == len(b) == q["keep"] and np.array_equal(bits(np.array(a, dtype=np.float64)), bits(np.array(b, dtype=np.float64))), q
    # a second call skips
    stamp = {f: os.path.getmtime(os.path.join(out, f)) for f in os.listdir(out)}
    capsys.readouterr()
    again = CL.process(FIX, out, BASELINE_YEARS, YEARS, "cpu")
    assert again["skipped"] is True and "already exist. Skipping" in capsys.readouterr().out
    assert stamp == {f: os.path.getmtime(os.path.join(out, f)) for f in os.listdir(out)}
    assert CL.process(str(os.path.join(out, "nowhere")), out, BASELINE_YEARS, YEARS, "cpu")["skipped"] is True       # as the reference: checked first


def test_process_refuses_a_missing_year_and_a_mismatched_grid(CL, tmp_path):
    raw = tmp_path / "raw"
    shutil.copytree(FIX, raw)
    os.remove(raw / "CRU_mean_temperature_mon_0.5x0.5_global_1952_v4.03.npz")
    with pytest.raises(FileNotFoundError, match="CRU_mean_temperature_mon_0.5x0.5_global_1952_v4.03"):
        CL.process(str(raw), str(tmp_path / "out"), BASELINE_YEARS, YEARS, "cuda")   # raised before the device is touched
    assert not os.path.exists(tmp_path / "out")
    with np.load(os.path.join(FIX, "CRU_mean_temperature_mon_0.5x0.5_global_1951_v4.03.npz")) as z:
        tas, lat, lon = z["tas"], z["lat"], z["lon"]
    np.savez(raw / "CRU_mean_temperature_mon_0.5x0.5_global_1952_v4.03.npz", tas=tas, lat=lat + 0.5, lon=lon)
    with pytest.raises(ValueError, match="global_1952_v4.03.npz: its grid .* differs from the first year's"):
        CL.process(str(raw), str(tmp_path / "out"), BASELINE_YEARS, YEARS, "cpu")
    np.savez(raw / "CRU_mean_temperature_mon_0.5x0.5_global_1903_v4.03.npz", tas=tas[:, :5], lat=lat[:5], lon=lon)
    with pytest.raises(ValueError, match="global_1903_v4.03.npz: its grid \\(5 x 8\\)"):
        CL.process(str(raw), str(tmp_path / "out2"), BASELINE_YEARS, YEARS, "cpu")
    with pytest.raises(FileNotFoundError, match="Raw temperature directory not found"):
        CL.process(str(tmp_path / "nowhere"), str(tmp_path / "out3"), BASELINE_YEARS, YEARS, "cpu")
    with pytest.raises(ValueError, match="first <= last"):
        CL.process(str(raw), str(tmp_path / "out3"), (1904, 1901), YEARS, "cpu")


# --------------------------------------------------------------------------- #
# moments of the series; edge cases of the twins
# --------------------------------------------------------------------------- #
def test_series_moments_against_numpy_over_the_concatenated_values(CL):
    T, G = 120, 23
    x = make_grid(T, G, 5, nan=0.0)
    rows = CL.baseline_host(x[:60])
    rng = np.random.default_rng(6)
    cell, keep = rng.integers(0, G, 40), rng.integers(0, T + 1, 40)
    keep[3] = 0
    keep[7] = T
    out, srows = CL.series_host(x, rows, cell, keep)
    values = np.concatenate([out[n, :k].astype(np.float64) for n, k in enumerate(keep)])
    mean, std = CL.series_moments(srows)
    rms = float(np.sqrt(np.mean(values ** 2)))
    assert int(srows[:, 0].sum()) == values.size == int(keep.sum()) and srows[3].tolist()[0::2] == [0.0, 0.0] and np.isnan(srows[3, 1])
    print(f"series_moments: mean {abs(mean - np.mean(values)) / rms:.3g}, std {abs(std - np.std(values)) / rms:.3g} of the RMS (bound {TOL:g})")
    assert abs(mean - np.mean(values)) <= TOL * rms and abs(std - np.std(values)) <= TOL * rms
    assert all(np.isnan(v) for v in CL.series_moments(np.array([[0.0, np.nan, 0.0, 0.0]])))
    # one NaN value makes both NaN, as np.mean / np.std of the concatenation
    x[5, cell[0]] = np.nan
    keep[0] = 10
    assert all(np.isnan(v) for v in CL.series_moments(CL.series_host(x, rows, cell, keep)[1]))


def test_twin_edge_cases(CL):
    # T = 1: n = 1, M2 = 0, std 0, the anomaly 0 / 0
    x = np.array([[3.5, np.nan, -2.0]], dtype=np.float32)
    rows = CL.baseline_host(x)
    assert rows[0].tolist() == [1.0, 3.5, 0.0, 0.0] and rows[2].tolist() == [1.0, -2.0, 0.0, 0.0]
    assert rows[1, 0] == 0 and np.isnan(rows[1, 1]) and np.isnan(rows[1, 2]) and rows[1, 3] == 1                  # an all-NaN cell
    assert np.isnan(CL.normalise_host(x, rows)).all()
    # a single non-NaN value among NaN: std 0, anomaly NaN at the value; +-inf next to it
    x = np.full((5, 4), np.nan, dtype=np.float32)
    x[2, 0] = 7.25
    x[:, 1] = [1.0, 2.0, 3.0, 4.0, 5.0]
    x[:, 2] = [1.0, np.inf, 3.0, np.nan, 5.0]
    rows = CL.baseline_host(x)
    assert rows[0].tolist() == [1.0, 7.25, 0.0, 4.0] and rows[1].tolist() == [5.0, 3.0, 10.0, 0.0]
    assert rows[2, 0] == 4 and rows[2, 1] == np.inf and np.isnan(rows[2, 2]) and rows[2, 3] == 1                  # an inf is not skipped
    assert rows[3, 0] == 0 and np.isnan(rows[3, 1:3]).all() and rows[3, 3] == 5
    norm = CL.normalise_host(x, rows)
    assert np.isnan(norm[:, 0]).all() and np.isnan(norm[:, 2:]).all()
    assert np.array_equal(norm[:, 1], ((np.arange(1, 6) - 3.0) / np.sqrt(2.0)).astype(np.float32))
    two = np.array([[1.0], [3.0]], dtype=np.float32)                                                                   # std > 0, other rows' std 0
    assert np.array_equal(CL.normalise_host(np.array([[5.0]], np.float32), np.array([[2.0, 1.0, 0.0, 0.0]])), [[np.inf]])
    assert np.array_equal(CL.normalise_host(two, CL.baseline_host(two)), [[-1.0], [1.0]])
    # keep = 0 and keep = T; beyond the ranges; a cell outside the grid
    x = make_grid(9, 5, 1, nan=0.0)
    rows = CL.baseline_host(x)
    norm = CL.normalise_host(x, rows)
    out, srows = CL.series_host(x, rows, [2, 2, 4, 4, 7, -1], [0, 9, 40, -3, 4, 4], Tpad=11)
    assert out.shape == (6, 11) and not out[0].any() and np.array_equal(bits(out[1, :9]), bits(norm[:, 2])) and not out[1, 9:].any()
    assert np.array_equal(bits(out[2, :9]), bits(norm[:, 4])) and not out[3].any()
    assert srows[:, 0].tolist() == [0, 9, 9, 0, 0, 0] and np.isnan(out[4:, :4]).all() and not out[4:, 4:].any()
    assert np.isnan(srows[[0, 3, 4, 5], 1]).all() and not srows[[0, 3, 4, 5], 2:].any()
    with pytest.raises(ValueError, match="Tpad"):
        CL.series_host(x, rows, [0], [1], Tpad=8)
    with pytest.raises(ValueError, match="float32"):
        CL.baseline_host(x.astype(np.float64))
    with pytest.raises(ValueError, match="rows must be float64"):
        CL.normalise_host(x, rows[:4])
    # an argmin tie takes the first index; the nearest point otherwise; the cut
    cq = CL.ClimateQuery(x.reshape(9, 1, 5), rows, [10.0], [0.0, 1.0, 2.0, 3.0, 4.0], 2000)
    cell, keep = cq.indices([10.0, -80.0, 0.0, 0.0], [1.5, 3.4, 9.0, -9.0], [2000, 2000, 1999, 2003], [3, 9, 12, 1])
    assert cell.tolist() == [1, 3, 4, 0] and keep.tolist() == [3, 9, 0, 9] and cell.dtype == keep.dtype == np.int32
    assert cq.query(10.0, 1.5, 2000, 3) == norm[:3, 1].tolist() and cq.query(0.0, 0.0, 1999, 12) == []
    with pytest.raises(ValueError, match="ClimateQuery: raw"):
        CL.ClimateQuery(x.reshape(9, 1, 5), rows, [10.0, 11.0], [0.0, 1.0, 2.0, 3.0, 4.0], 2000)
    with pytest.raises(ValueError, match="one length"):
        cq.indices([1.0, 2.0], [1.0], [2000], [1])


# --------------------------------------------------------------------------- #
# the C entry points
# --------------------------------------------------------------------------- #
def test_every_refusal_of_the_entry_points(CL):
    from mau_amd._lib import lib
    hdr = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    assert lib.mau_abi_version() == 5 and "#define MAU_ABI_VERSION 5" in hdr
    assert lib.mau_climate_row_elems() == CL.ROW == 4 == lib.mau_moments_row_elems()
    assert lib.mau_climate_series_max_months() == CL.MAX_MONTHS == 4096
    buf = (ctypes.c_double * 64)()                                   # host memory standing in for pointers that are never followed
    p = ctypes.addressof(buf)

    def refused(fn, prefix, good, word, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        status = getattr(lib, fn)(*args)
        msg = lib.mau_last_error().decode()
        assert status == MAU_ERR_ARG and msg.startswith(prefix + ": ") and word in msg, (fn, change, status, msg)

    good = [p, p, 12, 48, None]
    for k in range(2):
        refused("mau_climate_baseline", "climate_baseline", good, "null pointer", **{f"a{k}": None})
    for T, G in ((0, 48), (12, 0), (-1, 48), (12, -48)):
        refused("mau_climate_baseline", "climate_baseline", good, "non-positive size", a2=T, a3=G)
    refused("mau_climate_baseline", "climate_baseline", good, "at most 2^30 cells", a3=(1 << 30) + 1)
    refused("mau_climate_baseline", "climate_baseline", good, "x must be 4-byte aligned", a0=p + 2)
    refused("mau_climate_baseline", "climate_baseline", good, "rows must be 8-byte aligned", a1=p + 4)

    good = [p, p, p, 12, 48, None]
    for k in range(3):
        refused("mau_climate_normalise", "climate_normalise", good, "null pointer", **{f"a{k}": None})
    for T, G in ((0, 48), (12, 0), (-1, 48), (12, -48)):
        refused("mau_climate_normalise", "climate_normalise", good, "non-positive size", a3=T, a4=G)
    refused("mau_climate_normalise", "climate_normalise", good, "at most 2^30 cells", a4=(1 << 30) + 1)
    refused("mau_climate_normalise", "climate_normalise", good, "months", a3=65535 * 64 + 1)
    for k in (0, 2):
        refused("mau_climate_normalise", "climate_normalise", good, "4-byte aligned", **{f"a{k}": p + 2})
    refused("mau_climate_normalise", "climate_normalise", good, "rows must be 8-byte aligned", a1=p + 4)

    good = [p, p, p, p, p, p, 3, 12, 48, 12, None]
    for k in range(6):
        refused("mau_climate_series", "climate_series", good, "null pointer", **{f"a{k}": None})
    for N, T, G in ((0, 12, 48), (3, 0, 48), (3, 12, 0), (-1, 12, 48), (3, -12, 48), (3, 12, -48)):
        refused("mau_climate_series", "climate_series", good, "non-positive size", a6=N, a7=T, a8=G, a9=max(T, 12))
    refused("mau_climate_series", "climate_series", good, "at most 2^30 cells", a8=(1 << 30) + 1)
    refused("mau_climate_series", "climate_series", good, "at most 2^30 queries", a6=(1 << 30) + 1)
    refused("mau_climate_series", "climate_series", good, "at most 4096 months", a7=4097, a9=4097)
    refused("mau_climate_series", "climate_series", good, "Tpad 11 is shorter", a9=11)
    for k in (0, 2, 3, 4):
        refused("mau_climate_series", "climate_series", good, "4-byte aligned", **{f"a{k}": p + 2})
    for k in (1, 5):
        refused("mau_climate_series", "climate_series", good, "8-byte aligned", **{f"a{k}": p + 4})


# --------------------------------------------------------------------------- #
# the command line
# --------------------------------------------------------------------------- #
def test_command_line_exit_codes_and_the_one_line_error(CL, twin, tmp_path, capsys):
    import mau_amd
    assert mau_amd.climate is CL and "climate" in mau_amd.__all__ and mau_amd.ClimateQuery is CL.ClimateQuery
    out = tmp_path / "processed"
    argv = ["--raw-dir", FIX, "--output-dir", str(out), "--baseline-years", "1901", "1904", "--years", "1951", "1953", "--device", "cpu"]
    assert CL.main(argv) == 0
    capsys.readouterr()
    with np.load(out / "tas_norm.npz") as z:
        assert np.array_equal(bits(z["data"]), bits(twin["norm"]))

    def fails(args, word):
        assert CL.main(args) == 1
        lines = capsys.readouterr().out.strip().split("\n")
        assert lines[-1].startswith("Error: ") and word in lines[-1] and sum(1 for x in lines if x.startswith("Error")) == 1, lines

    fails(["--raw-dir", FIX, "--output-dir", str(tmp_path / "a"), "--device", "cpu"], "global_1905_v4.03")           # the default years
    fails(["--raw-dir", FIX, "--output-dir", str(tmp_path / "b"), "--baseline-years", "1901", "1904", "--years", "1951", "1954"], "global_1954_v4.03")
    fails(["--raw-dir", str(tmp_path / "nowhere"), "--output-dir", str(tmp_path / "c"), "--device", "cpu"], "Raw temperature directory not found")
    fails(argv[:4] + ["--baseline-years", "1904", "1901", "--device", "cpu"], "first <= last")
    assert not any(os.path.exists(tmp_path / d) for d in "abc")
    with pytest.raises(SystemExit) as e:
        CL.main(["--raw-dir", FIX])
    assert e.value.code == 2 and "--output-dir" in capsys.readouterr().err
