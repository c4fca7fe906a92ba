#!/usr/bin/env python3
"""Record the dataset-build fixture (tests/golden/buildfix, buildfix_deviation.json) FROM THE REFERENCE ITSELF.  CPU only:

    MAU_REFERENCE=<checkout of the reference> python tests/golden/make_buildfix.py

Generates raw tiles of 16 x 16 (uint8 class maps and RGB, float32 NDVI and temperature -- the reference's own cached rasters hold
uint8 / uint8 / float32 and a FLOAT64 temperature; see mau_amd/dataset_build.py on what that means), a cities CSV and a small monthly
temperature array, then imports the reference's ``src/data/processing_10m/process.py`` with stand-ins in ``sys.modules`` for
``loguru``, ``rasterio`` / ``rasterio.warp`` (a reader over the fixture's ``.npy`` rasters), ``xarray`` and ``urban_planner.config``,
and a ``TemperatureQuery`` made without its ``__init__``, and runs ``filter_and_calculate_metrics``, ``filter_subset`` and
``process_and_save_subset`` on them.  Recorded: the raw rasters (one archive, raw.npz), the reference's metrics JSON, the kept file names per split, three
processed tiles in compact form (class maps as uint8; the recorder checks that the compact form expands to the reference's dense
input bit for bit) and the deviation of each of the reference's metrics from the float64 twin.  No reference source is copied:
fixtures are data.  Every property the tests rely on is asserted here."""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MAU_REFERENCE")                 # a checkout of the reference project
FIX = os.path.join(HERE, "buildfix")
H = W = 16
MARGIN = 1e-3
START_YEAR, YEARS = 2015, 8


# --------------------------------------------------------------------------- #
# the raw tiles
# --------------------------------------------------------------------------- #
def stem(city, cid, lat, lon, year, month):
    return f"{city}_{cid}_{lat:.4f}_{lon:.4f}_0.0_0.0_{year}_{month:02d}"


def scene(rng):
    """One timestamp: class map, RGB, NDVI, temperature."""
    dw = rng.choice(np.array([0, 1, 2, 4, 6, 7], dtype=np.uint8), (H, W), p=[0.1, 0.3, 0.2, 0.1, 0.2, 0.1])
    rgb = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    ndvi = np.clip(0.3 + 0.25 * rng.standard_normal((H, W)), -0.2, 0.9).astype(np.float32)
    temp = (295.0 + rng.uniform(-8, 8) + 3.0 * rng.standard_normal((H, W))).astype(np.float32)
    return {"dw": dw, "rgb": rgb, "ndvi": ndvi, "temp": temp}


def later(rng, s, ndvi=False, temp=False, dw=False):
    """The scene some years on: every plane moves a little (mean |change| ~ 0.05, 3 % of the class map), the named ones a lot."""
    out = {"rgb": rng.integers(0, 256, (3, H, W)).astype(np.uint8)}
    out["ndvi"] = (s["ndvi"] + rng.uniform(-1, 1, (H, W)) * (0.4 if ndvi else 0.1)).astype(np.float32)
    out["temp"] = (s["temp"] + rng.uniform(-1, 1, (H, W)) * 0.1 + (0.5 if temp else 0.0)).astype(np.float32)
    d = s["dw"].copy()
    if dw:
        d[rng.random((H, W)) < 0.35] = 6
    else:
        pick = rng.random((H, W)) < 0.03
        d[pick] = rng.choice(np.array([0, 1, 2, 4, 6, 7], dtype=np.uint8), int(pick.sum()))
    out["dw"] = d
    return out


def unpack_raw(archive, raw_dir):
    """raw.npz (raster file name -> array) -> a directory of ``.npy`` rasters, as the build reads it."""
    os.makedirs(raw_dir)
    with np.load(archive) as z:
        for name in z.files:
            np.save(os.path.join(raw_dir, name), z[name])


def write_raw(raw_dir):
    rng = np.random.default_rng(20240607)
    files = {}

    def put(city, cid, lat, lon, year, month, sc, leave_out=()):
        for k, v in sc.items():
            if k not in leave_out:
                files[f"{stem(city, cid, lat, lon, year, month)}_{k}.npy"] = v

    # train (t2 <= 2023): dropped, kept by NDVI alone, by temperature alone, by land cover alone, an out-of-range class
    for city, cid, lat, lon, t1, t2, kw in (("Roma", 0, 41.899, 12.469, (2019, 8), (2021, 8), {}),
                                            ("Sao_Paulo", 1, -23.5505, -46.6333, (2018, 1), (2022, 3), {"ndvi": True}),
                                            ("Oslo", 2, 59.9139, 10.7522, (2020, 6), (2023, 6), {"temp": True}),
                                            ("Lagos", 3, 6.5244, 3.3792, (2017, 11), (2023, 2), {"dw": True}),
                                            ("Quito", 4, -0.1807, -78.4678, (2019, 5), (2022, 5), {"ndvi": True}),
                                            ("Lima", 7, -12.0464, -77.0428, (2020, 2), (2024, 2), {}),             # val, dropped
                                            ("Cairo", 6, 30.0444, 31.2357, (2022, 1), (2026, 1), {"ndvi": True})):  # t2 2026: no split
        a = scene(rng)
        b = later(rng, a, **kw)
        if city == "Quito":
            b["dw"][3, 5] = 9
        put(city, cid, lat, lon, *t1, a)
        put(city, cid, lat, lon, *t2, b)
    # three timestamps of one location: 2021 -> 2024 (val, kept), 2021 -> 2025 (test, kept), 2024 -> 2025 (test, dropped)
    a = scene(rng)
    b = later(rng, a, ndvi=True, dw=True)
    c = later(rng, b)
    for t, sc in (((2021, 3), a), ((2024, 3), b), ((2025, 9), c)):
        put("New_York", 5, 40.7128, -74.006, *t, sc)
    # a second timestamp without its temperature raster: no sample; and a name that does not parse
    a = scene(rng)
    put("Perth", 8, -31.9523, 115.8613, 2019, 1, a)
    put("Perth", 8, -31.9523, 115.8613, 2021, 1, later(rng, a, ndvi=True), leave_out=("temp",))
    files["notes_ndvi.npy"] = np.zeros((2, 2), np.float32)
    np.savez_compressed(os.path.join(FIX, "raw.npz"), **files)               # one archive: the tests unpack it (unpack_raw)
    unpack_raw(os.path.join(FIX, "raw.npz"), raw_dir)
    with open(os.path.join(FIX, "cities.csv"), "w") as f:                      # Lagos is not listed: population 0
        f.write("city,id,population\nRoma,0,2872800\nSao Paulo,1,12252023\nOslo,2,693494\nQuito,4,2011388\nNew York,5,8804190\n"
                "Cairo,6,9539673\nLima,7,9751717\nPerth,8,2059484\n")
    lats, lons = np.array([-31.75, -23.75, -12.25, -0.25, 6.75, 30.25, 40.75, 41.75, 59.75]), np.array([-78.25, -77.25, -74.25, -46.75, 3.25, 10.75, 12.25, 31.25, 115.75])
    t = np.arange(12 * YEARS)
    data = (np.sin(2 * np.pi * t / 12.0)[:, None, None] * 1.2 + 0.004 * t[:, None, None] + 0.3 * rng.standard_normal((t.size, lats.size, lons.size))).astype(np.float32)
    np.savez_compressed(os.path.join(FIX, "temperature.npz"), data=data, lats=lats, lons=lons, start_year=np.int64(START_YEAR))


# --------------------------------------------------------------------------- #
# the reference, with stand-ins for what it imports and this machine does not need
# --------------------------------------------------------------------------- #
class _Reader:
    def __init__(self, path):
        self.data = np.load(path)
        self.height, self.width = self.data.shape[-2:]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def read(self, bands, out_shape=None, resampling=None):
        out = self.data if isinstance(bands, list) else (self.data if self.data.ndim == 2 else self.data[bands - 1])
        assert tuple(out_shape) == out.shape, (out_shape, out.shape)           # the fixture needs no resampling
        return out.copy()


def import_reference():
    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("loguru", logger=_Logger())
    resampling = types.SimpleNamespace(bilinear="bilinear", nearest="nearest")
    warp = module("rasterio.warp", Resampling=resampling)
    module("rasterio", open=_Reader, warp=warp)
    module("xarray")
    config = types.SimpleNamespace(PROCESSED_TEMPERATURE_DATA_DIR=None, dataset=types.SimpleNamespace(temporal_start_year=START_YEAR, temporal_end_year=START_YEAR + YEARS - 1))
    module("urban_planner")
    module("urban_planner.config", CONFIG=config)
    sys.path.insert(0, REF)
    import src.data.processing_10m.process as process
    import src.data.processing_10m.split as split
    return process, split


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("make_buildfix: set MAU_REFERENCE to a checkout of the reference project")
    sys.path.insert(0, ROOT)
    from mau_amd import dataset_build as DB
    from mau_amd.data import compact_input, expand_input

    if os.path.isdir(FIX):
        shutil.rmtree(FIX)
    os.makedirs(FIX)
    scratch = tempfile.TemporaryDirectory()
    raw_dir = os.path.join(scratch.name, "raw")
    write_raw(raw_dir)

    process, split = import_reference()
    z = np.load(os.path.join(FIX, "temperature.npz"))
    tq = object.__new__(process.TemperatureQuery)                               # no __init__: it would read NetCDF files
    tq.start_year, tq.end_year = START_YEAR, START_YEAR + YEARS - 1
    tq.data, tq.lats, tq.lons = z["data"], z["lats"], z["lons"]
    tq.timestamps = [(y, m) for y in range(tq.start_year, tq.end_year + 1) for m in range(1, 13)]
    process.TemperatureQuery = lambda processed_dir: tq

    samples = DB.list_samples(raw_dir, os.path.join(FIX, "cities.csv"))
    assert len(set(s["city_id"] for s in samples)) < 100                        # the holdout count is 0
    assert sorted(set(s["t2_year"] for s in samples)) == [2021, 2022, 2023, 2024, 2025, 2026]
    train, val, test = quiet(split.train_test_val_split, samples)
    mine = DB.split_samples(samples)
    assert [[DB.output_filename(s) for s in part] for part in (train, val, test)] == [[DB.output_filename(s) for s in part] for part in mine]
    assert (len(train), len(val), len(test)) == (5, 2, 2) and len(samples) == 10

    shape = (H, W)
    metrics, train_kept = quiet(process.filter_and_calculate_metrics, train, shape)
    text = json.dumps(metrics, indent=4, default=float)                         # numpy 2 leaves temp_mean / temp_std as np.float32 scalars
    metrics = json.loads(text)
    val_kept = quiet(process.filter_subset, val, shape, "validation")
    test_kept = quiet(process.filter_subset, test, shape, "test")
    kept = {"train": train_kept, "val": val_kept, "test": test_kept}
    names = {k: [DB.output_filename(s) for s in v] for k, v in kept.items()}
    assert [len(v) for v in names.values()] == [3, 1, 1], names

    # the reference's own float32 numbers of every sample: margins, and which criterion keeps which sample
    own = {}
    for s in samples:
        r = DB.read_sample(s, shape)
        eye = np.eye(10)
        vals = (float(np.abs(r["ndvi_t2"] - r["ndvi_t1"]).mean()), float(np.abs(r["temp_t2"] - r["temp_t1"]).mean()),
                float(np.max(np.mean(np.abs(eye[r["dw_t2"]] - eye[r["dw_t1"]]), axis=0)[:9])))
        assert all(abs(v - 0.1) >= MARGIN for v in vals), (DB.output_filename(s), vals)
        own[DB.output_filename(s)] = [v >= 0.1 for v in vals]
    by = {tuple(v) for k, v in own.items() if k in names["train"]}
    assert by == {(True, False, False), (False, True, False), (False, False, True)}, by
    assert sum(1 for s in train if not any(own[DB.output_filename(s)])) == 1    # one training sample dropped
    oor = [s for s in samples if max(DB.read_sample(s, shape)["dw_t2"].max(), DB.read_sample(s, shape)["dw_t1"].max()) >= 9]
    assert len(oor) == 1 and oor[0] in train and oor[0] not in train_kept

    with tempfile.TemporaryDirectory() as tmp:
        for k, v in kept.items():
            quiet(process.process_and_save_subset, v, metrics, tq, os.path.join(tmp, k), shape)
            assert sorted(os.listdir(os.path.join(tmp, k))) == sorted(names[k])
        os.makedirs(os.path.join(FIX, "reference"))
        with open(os.path.join(FIX, "reference", "normalization_metrics.json"), "w") as f:
            f.write(text)
        with open(os.path.join(FIX, "reference", "kept.json"), "w") as f:
            json.dump({k: sorted(v) for k, v in names.items()}, f, indent=1)
        for k in ("train", "val", "test"):
            name = sorted(names[k])[0]
            t = np.load(os.path.join(tmp, k, name))
            assert t["input"].dtype == np.float32 and t["input"].shape == (23, H, W) and t["target"].shape == (2, H, W)
            a, b, cont = compact_input(t["input"])
            assert np.array_equal(expand_input(a, b, cont).view(np.uint32), t["input"].view(np.uint32))
            os.makedirs(os.path.join(FIX, "reference", k))
            np.savez_compressed(os.path.join(FIX, "reference", k, name), cls_a=a, cls_b=b, cont=cont, target=t["target"],
                                metadata=t["metadata"], temperature_serie=t["temperature_serie"])

    # the float64 twin, and the deviation of the reference's metrics from it
    with tempfile.TemporaryDirectory() as tmp:
        res = quiet(DB.build, raw_dir, tmp, DB.ArrayTemperatureQuery.from_npz(os.path.join(FIX, "temperature.npz")),
                    os.path.join(FIX, "cities.csv"), "cpu")
    assert {k: sorted(v) for k, v in res["kept"].items()} == {k: sorted(v) for k, v in names.items()}
    twin = res["metrics"]
    assert list(twin) == list(metrics) == DB.METRIC_KEYS
    dev = {k: np.abs(np.asarray(metrics[k], dtype=np.float64) - np.asarray(twin[k], dtype=np.float64)).tolist() for k in metrics}
    scale = {k: np.abs(np.asarray(twin[k], dtype=np.float64)).tolist() for k in metrics}
    scale["rgb_std"] = np.sqrt(np.square(twin["rgb_std"]) + np.square(twin["rgb_mean"])).tolist()        # the RMS of the plane
    scale["temp_std"] = float(np.hypot(twin["temp_std"], twin["temp_mean"]))
    scale["temp_series_std"] = float(np.hypot(twin["temp_series_std"], twin["temp_series_mean"]))
    with open(os.path.join(HERE, "buildfix_deviation.json"), "w") as f:
        json.dump({"source": "reference filter_and_calculate_metrics (sum x^2 / n - mean^2; float32 temperature sums) versus the float64 twin",
                   "dev": dev, "scale": scale}, f, indent=1)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(FIX) for f in fs)
    print(f"buildfix: {len(os.listdir(raw_dir))} rasters, {size / 1024:.1f} KiB; deviation of temp_std {dev['temp_std']:.3g}, of rgb_std {max(dev['rgb_std']):.3g}")


if __name__ == "__main__":
    main()
