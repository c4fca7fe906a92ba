"""``mau_amd.dataset_build`` without a device: file names, pairing and splits; the numpy twins against the fixture recorded from the
reference's ``process.py`` (tests/golden/make_buildfix.py -> tests/golden/buildfix, buildfix_deviation.json): keep / drop lists, tiles
bit for bit, metrics within the recorded deviation; the fixture's margins; the C entry point's bindings, size helper and refusals
(called through ctypes with no device: every refusal comes before a launch); the command line.

Metrics bound per value: ``2 * dev + 1e-10 * scale`` -- dev is the reference's own deviation from the float64 twin on the fixture (its
sum x^2 / n - mean^2 with float32 temperature sums: 1e-3 on temp_std there), the factor two the margin the project gives it
(tests/test_dataset_metrics_host.py), 1e-10 test_gpu_ground_truth.TOL relative to the plane's RMS."""
import ctypes
import json
import os
import random
import shutil

import numpy as np
import pytest

from tests._helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "buildfix")
TOL = 1e-10
MARGIN = 1e-3
MAU_ERR_ARG = 1
SPLITS = ("train", "val", "test")
TILE_KEYS = ("input", "target", "metadata", "temperature_serie")


@pytest.fixture(scope="module")
def DB():
    import mau_amd
    return mau_amd.dataset_build


def unpack_raw(raw_dir):
    """tests/golden/buildfix/raw.npz (raster file name -> array) -> a directory of ``.npy`` rasters."""
    os.makedirs(raw_dir)
    with np.load(os.path.join(FIX, "raw.npz")) as z:
        for name in z.files:
            np.save(os.path.join(raw_dir, name), z[name])
    return str(raw_dir)


def reference_kept():
    return json.load(open(os.path.join(FIX, "reference", "kept.json")))


def reference_metrics():
    return json.load(open(os.path.join(FIX, "reference", "normalization_metrics.json")))


def recorded_tiles():
    """{(split, file name): the recorded tile, dense again}"""
    from mau_amd.data import expand_input
    out = {}
    for split in SPLITS:
        for name in sorted(os.listdir(os.path.join(FIX, "reference", split))):
            z = np.load(os.path.join(FIX, "reference", split, name))
            out[(split, name)] = {"input": expand_input(z["cls_a"], z["cls_b"], z["cont"]), "target": z["target"], "metadata": z["metadata"],
                                  "temperature_serie": z["temperature_serie"]}
    return out


def assert_tiles_are_the_recorded_ones(processed_dir, what):
    tiles = recorded_tiles()
    assert len(tiles) == 3
    for (split, name), want in tiles.items():
        got = np.load(os.path.join(processed_dir, split, name))
        assert sorted(got.files) == sorted(TILE_KEYS)
        for k in TILE_KEYS:
            assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, name, k)
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, name, k, float(np.max(np.abs(got[k] - want[k]))))


def assert_kept_is_the_references(result, processed_dir):
    want = reference_kept()
    assert {k: sorted(v) for k, v in result["kept"].items()} == want
    for split in SPLITS:
        assert sorted(os.listdir(os.path.join(processed_dir, split))) == want[split]


def run_build(DB, raw_dir, out_dir, device, with_reference_metrics, **kw):
    os.makedirs(out_dir, exist_ok=True)
    if with_reference_metrics:
        shutil.copy(os.path.join(FIX, "reference", "normalization_metrics.json"), out_dir)
    tq = DB.ArrayTemperatureQuery.from_npz(os.path.join(FIX, "temperature.npz"))
    return DB.build(raw_dir, str(out_dir), tq, os.path.join(FIX, "cities.csv"), device, **kw)


@pytest.fixture(scope="module")
def raw_dir(tmp_path_factory):
    return unpack_raw(tmp_path_factory.mktemp("buildfix") / "raw")


@pytest.fixture(scope="module")
def twin_build(DB, raw_dir, tmp_path_factory):
    """build(device='cpu') without a metrics file: (result, processed dir)"""
    out = tmp_path_factory.mktemp("twin") / "processed"
    return run_build(DB, raw_dir, out, "cpu", False, batch_size=3), str(out)


def make_raw(B, H, W, seed):
    """A raw batch: class maps in which classes 2, 4, 5 and 7 never occur, integer RGB in 0..255, a temperature plane with |mean| a
    thousand times its std (tests/test_gpu_dataset_metrics.make_batch)."""
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0, 1, 3, 6, 8], dtype=np.uint8), (B, H, W))
    b = a.copy()
    flip = rng.random((B, H, W)) < 0.25
    b[flip] = rng.choice(np.array([0, 1, 3, 6, 8], dtype=np.uint8), int(flip.sum()))
    rgb = rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)
    n1 = np.tanh(0.6 * rng.standard_normal((B, H, W)) + rng.uniform(-0.5, 0.5, (B, 1, 1))).astype(np.float32)
    n2 = np.clip(n1 + 0.1 * rng.standard_normal((B, H, W)), -1, 1).astype(np.float32)
    t1 = (300.0 + rng.uniform(-20, 20, (B, 1, 1)) + 0.3 * rng.standard_normal((B, H, W))).astype(np.float32)
    t2 = (t1 + 0.05 * rng.standard_normal((B, H, W)) + 0.12).astype(np.float32)
    return a, b, rgb, n1, n2, t1, t2


NORM = [0.4471, 0.4012, 0.3577, 0.2113, 0.1987, 0.2054, 301.337, 0.2971]


# --------------------------------------------------------------------------- #
# names, pairs, splits
# --------------------------------------------------------------------------- #
def test_file_names_and_sample_pairs(DB, raw_dir, capsys):
    p = DB.parse_filename("/x/New_York_5_40.7128_-74.0060_0.0_0.0_2021_03_ndvi.npy")
    assert (p["city_name"], p["city_id"], p["lat"], p["lon"], p["offset_x"], p["year"], p["month"], p["type"]) == \
        ("New_York", 5, 40.7128, -74.006, 0.0, 2021, 3, "ndvi")
    assert DB.parse_filename("Roma_0_41.8990_12.4690_0.0_0.0_2019_08_rgb.tif")["type"] == "rgb"
    assert DB.parse_filename("notes_ndvi.npy") is None and DB.parse_filename("a_b_c_d_e_f_g_h_i.tif") is None
    groups = DB.group_files(raw_dir)
    assert "Could not parse filename: notes_ndvi.npy" in capsys.readouterr().out
    assert len(groups) == 9 and sorted(groups[(5, 40.7128, -74.006)]["timestamps"]) == [(2021, 3), (2024, 3), (2025, 9)]
    assert sorted(groups[(8, -31.9523, 115.8613)]["timestamps"][(2021, 1)]) == ["dw", "ndvi", "rgb"]
    samples = DB.list_samples(raw_dir, os.path.join(FIX, "cities.csv"))
    assert len(samples) == 10 and not any(s["city_name"] == "Perth" for s in samples)            # no temperature raster at t2: no sample
    ny = [s for s in samples if s["city_id"] == 5]
    assert [(s["t1_year"], s["t2_year"]) for s in ny] == [(2021, 2024), (2021, 2025), (2024, 2025)]
    assert ny[1]["delta_time_years"] == (2025 - 2021) + (9 - 3) / 12.0 and ny[0]["population"] == 8804190.0
    assert sorted(ny[0]["files"]) == ["dw", "dw_t2", "ndvi", "ndvi_t2", "rgb", "temp", "temp_t2"]
    assert ny[0]["files"]["temp_t2"].endswith("2024_03_temp.npy") and ny[0]["files"]["temp"].endswith("2021_03_temp.npy")
    lagos = [s for s in samples if s["city_name"] == "Lagos"][0]
    assert lagos["population"] == 0 and DB.list_samples(raw_dir)[0]["population"] == 0          # absent from the CSV / no CSV
    assert DB.output_filename(lagos) == "Lagos_3_6.5244_3.3792_2017_11_to_2023_02.npz"


def test_split_by_year_and_seeded_holdout(DB, raw_dir):
    samples = DB.list_samples(raw_dir, os.path.join(FIX, "cities.csv"))
    train, val, test = DB.split_samples(samples)
    assert [len(x) for x in (train, val, test)] == [5, 2, 2]                       # fewer than 100 cities: no holdout city
    assert all(s["t2_year"] <= 2023 for s in train) and all(s["t2_year"] == 2024 for s in val) and all(s["t2_year"] == 2025 for s in test)
    assert not any(s["city_name"] == "Cairo" for s in train + val + test)          # t2 in 2026: in no split
    many = [{"city_id": c, "t2_year": y} for c in range(250) for y in (2022, 2024, 2025, 2027)]
    a = DB.split_samples(many, 0.01, random.Random(7))
    b = DB.split_samples(many, 0.01, random.Random(7))
    assert a == b
    held = {s["city_id"] for s in a[2] if s["t2_year"] != 2025}
    assert len(held) == 2 and sum(1 for s in a[2] if s["city_id"] in held) == 8   # int(250 * 0.01) cities, whole, the 2027 pair too
    assert not any(s["city_id"] in held for s in a[0] + a[1])
    assert [len(x) for x in a] == [248, 248, 248 + 8]
    other = {s["city_id"] for s in DB.split_samples(many, 0.01, random.Random(8))[2] if s["t2_year"] != 2025}
    assert other != held
    assert len({s["city_id"] for s in DB.split_samples(many, 0.1, random.Random(7))[2] if s["t2_year"] != 2025}) == 25


def test_temperature_query(DB):
    z = np.load(os.path.join(FIX, "temperature.npz"))
    tq = DB.ArrayTemperatureQuery.from_npz(os.path.join(FIX, "temperature.npz"))
    i, j = int(np.abs(z["lats"] - 40.7128).argmin()), int(np.abs(z["lons"] + 74.006).argmin())
    s = tq.query(40.7128, -74.006, 2021, 3)
    assert isinstance(s, list) and len(s) == 6 * 12 + 3 and s == z["data"][:75, i, j].tolist()   # up to and including 2021-03
    assert len(tq.query(0.0, 0.0, 2015, 1)) == 1 and tq.query(0.0, 0.0, 2014, 12) == [] and len(tq.query(0.0, 0.0, 2040, 1)) == 96
    with pytest.raises(ValueError, match="ArrayTemperatureQuery"):
        DB.ArrayTemperatureQuery(np.zeros((4, 2, 3)), np.zeros(3), np.zeros(3), 2000)


# --------------------------------------------------------------------------- #
# the twins against the reference fixture
# --------------------------------------------------------------------------- #
def test_twin_tiles_are_the_references_bit_for_bit(DB, raw_dir, tmp_path, capsys):
    out = tmp_path / "processed"
    res = run_build(DB, raw_dir, out, "cpu", True, batch_size=4)
    log = capsys.readouterr().out
    assert "Loading existing normalization metrics" in log and "Saved new" not in log
    assert res["metrics"] == reference_metrics()
    assert_kept_is_the_references(res, out)
    assert_tiles_are_the_recorded_ones(out, "build(cpu) with the reference's metrics")
    assert "Failed during filtering for sample Quito_4: 1 class values outside [0, 9)" in log
    assert log.count("due to negligible changes") == 3                              # Roma, Lima, New York 2024 -> 2025
    # a second run writes nothing: existing outputs are skipped
    stamp = {f: os.path.getmtime(out / "train" / f) for f in os.listdir(out / "train")}
    again = run_build(DB, raw_dir, out, "cpu", False)
    assert again["written"] == {"train": [], "val": [], "test": []} and again["kept"] == res["kept"]
    assert stamp == {f: os.path.getmtime(out / "train" / f) for f in os.listdir(out / "train")}


def test_twin_metrics_within_the_recorded_deviation(DB, twin_build):
    res, out = twin_build
    deviation = json.load(open(os.path.join(GOLDEN, "buildfix_deviation.json")))
    assert deviation["source"].startswith("reference filter_and_calculate_metrics")
    text = open(os.path.join(out, "normalization_metrics.json")).read()
    twin, ref = json.loads(text), reference_metrics()
    assert twin == res["metrics"] and list(twin) == list(ref) == DB.METRIC_KEYS and text == json.dumps(twin, indent=4)
    assert_kept_is_the_references(res, out)
    for k in DB.METRIC_KEYS:
        d = np.abs(np.asarray(ref[k], dtype=np.float64) - np.asarray(twin[k], dtype=np.float64))
        dev, scale = np.asarray(deviation["dev"][k]), np.asarray(deviation["scale"][k])
        print(f"{k}: |reference - twin| {np.max(d):.3g} (recorded {np.max(dev):.3g})")
        assert d.shape == dev.shape and np.all(d <= 2 * dev + TOL * scale), (k, d, dev)
        assert np.all(np.abs(d - dev) <= TOL * scale), (k, d, dev)                  # the deviation file is re-derivable
    assert deviation["dev"]["meta_mean"] == [0.0] * 4 and 1e-4 < deviation["dev"]["temp_std"] < 1e-2
    # with its own metrics the twin's tiles differ from the recorded ones only through temp_mean / temp_std
    for (split, name), want in recorded_tiles().items():
        got = np.load(os.path.join(out, split, name))
        assert np.array_equal(bits(got["input"][:9]), bits(want["input"][:9])) and np.array_equal(bits(got["input"][12]), bits(want["input"][12]))
        assert np.array_equal(bits(got["target"][0]), bits(want["target"][0])) and np.array_equal(bits(got["metadata"]), bits(want["metadata"]))
        assert np.max(np.abs(got["input"][13] - want["input"][13])) < 5e-3


def test_every_fixture_sample_is_a_margin_away_from_every_threshold(DB, raw_dir):
    samples = DB.list_samples(raw_dir)
    shape = DB.raster_shape(samples[0]["files"]["ndvi"])
    assert shape == (16, 16)
    raws = [DB.read_sample(s, shape) for s in samples]
    assert raws[0]["rgb"].dtype == np.float32 and raws[0]["dw_t1"].dtype == np.uint8 and raws[0]["temp_t2"].dtype == np.float32
    rows = DB.raw_rows_host(*(np.stack([r[k] for r in raws]) for k in DB.RAW_KEYS))
    why = {}
    for s, r in zip(samples, rows):
        vals = DB.filter_values(r)
        assert all(abs(v - 0.1) >= MARGIN for v in vals), (DB.output_filename(s), vals)
        why[DB.output_filename(s)] = tuple(v >= 0.1 for v in vals)
    kept = reference_kept()
    assert {why[n] for n in kept["train"]} == {(True, False, False), (False, True, False), (False, False, True)}
    assert sum(1 for v in why.values() if not any(v)) == 3 and int(rows[:, DB.OOR:DB.OOR + 2].sum()) == 1


def test_twins_on_bad_values_and_the_decision(DB):
    a, b, rgb, n1, n2, t1, t2 = make_raw(3, 9, 11, 3)
    clean = DB.raw_rows_host(a, b, rgb, n1, n2, t1, t2)
    assert clean.shape == (3, DB.ROW) and np.all(clean[:, DB.MOM0::4] == 99) and np.all(clean[:, [2, 4, 5, 7]] == 0)
    assert all(DB.row_decision(r) == (True, None) for r in clean)                   # temperature change 0.12
    i = 0
    want = ((a[i] == 3) != (b[i] == 3)).sum()
    assert clean[i, 3] == want and clean[i, DB.NDVI_L1] == np.abs(n2[i].astype(np.float64) - n1[i]).sum()
    n1[1, 4, 4] = np.nan
    b[2, 0, 0] = 12
    rows = DB.raw_rows_host(a, b, rgb, n1, n2, t1, t2)
    assert np.array_equal(rows[0], clean[0]) and rows[1, DB.NDVI_BAD] == 1 and rows[1, DB.TEMP_BAD] == 0 and np.isnan(rows[1, DB.NDVI_L1])
    assert rows[2, DB.OOR + 1] == 1 and rows[2, DB.OOR] == 0
    assert DB.row_decision(rows[1]) == (False, "1 non-finite values (the reference would carry NaN into the metrics file and every tile)")
    assert DB.row_decision(rows[2])[1] == "1 class values outside [0, 9)"
    quiet = clean[0].copy()
    quiet[:9] = 9
    quiet[DB.NDVI_L1] = quiet[DB.TEMP_L1] = 0.0999 * 99
    assert DB.row_decision(quiet) == (False, None)
    for at, v in ((DB.NDVI_L1, 0.1 * 99), (DB.TEMP_L1, 0.1 * 99), (4, 10.0)):       # one value at its threshold keeps the sample: '<'
        r = quiet.copy()
        r[at] = v
        assert DB.row_decision(r) == (True, None), at
    cont, tgt = DB.normalise_host(rgb, n1, n2, t1, t2, NORM)
    assert cont.shape == (3, 5, 9, 11) and tgt.shape == (3, 2, 9, 11) and cont.dtype == tgt.dtype == np.float32
    assert np.array_equal(bits(cont[:, 3]), bits(n1)) and np.array_equal(bits(tgt[:, 0]), bits(n2))
    assert np.array_equal(cont[:, 0], ((rgb[:, 0].astype(np.float64) / 255.0 - NORM[0]) / NORM[3]).astype(np.float32))
    assert np.array_equal(tgt[:, 1], (t2 - np.float32(NORM[6])) / np.float32(NORM[7]))


def test_a_sample_that_cannot_be_read_is_skipped(DB, raw_dir, tmp_path, capsys):
    raw = tmp_path / "raw"
    shutil.copytree(raw_dir, raw)
    np.save(raw / "Oslo_2_59.9139_10.7522_0.0_0.0_2023_06_temp.npy", np.zeros((16, 15), np.float32))     # not the target shape
    nan = np.load(raw / "Lagos_3_6.5244_3.3792_0.0_0.0_2017_11_temp.npy")
    nan[2, 2] = np.nan
    np.save(raw / "Lagos_3_6.5244_3.3792_0.0_0.0_2017_11_temp.npy", nan)
    res = run_build(DB, str(raw), tmp_path / "processed", "cpu", True)
    log = capsys.readouterr().out
    assert "Failed during filtering for sample Oslo_2: Oslo_2_59.9139_10.7522_0.0_0.0_2023_06_temp.npy: shape (16, 15), expected (16, 16). Skipping." in log
    assert "Failed during filtering for sample Lagos_3: 2 non-finite values" in log          # temp_t1 and the temperature difference
    assert res["kept"]["train"] == ["Sao_Paulo_1_-23.5505_-46.6333_2018_01_to_2022_03.npz"]
    with pytest.raises(ValueError, match="expected \\(3, 16, 16\\)"):
        DB.read_raster(str(raw / "Oslo_2_59.9139_10.7522_0.0_0.0_2023_06_ndvi.npy"), (16, 16), "rgb")
    np.save(raw / "c.npy", np.array([[0, 8, 300], [-1, 255, 9]], dtype=np.int16))
    assert DB.read_raster(str(raw / "c.npy"), (2, 3), "classes").tolist() == [[0, 8, 255], [255, 255, 9]]


# --------------------------------------------------------------------------- #
# the C entry point
# --------------------------------------------------------------------------- #
def test_workspace_arithmetic(DB):
    from mau_amd._lib import lib
    assert lib.mau_abi_version() == 5
    assert lib.mau_raw_tile_row_elems() == DB.ROW == 16 + 2 + 4 + 4 * 4
    R, per, ws = lib.mau_raw_tile_row_elems(), lib.mau_reduce_tickets_elems(), lib.mau_raw_tile_ws_elems
    assert ws(3, 62500) == 3 * 16 * R and ws(1, 4096) == R and ws(1, 4097) == 2 * R and ws(per + 5, 62500) == per * 16 * R
    assert ws(0, 64) == 0 and ws(2, 0) == 0 and ws(-1, 64) == 0 and ws(1, (1 << 30) + 1) == 0 and ws(1, 1 << 30) == (1 << 18) * R


def test_every_refusal_of_the_entry_point(DB):
    from mau_amd._lib import lib
    buf = (ctypes.c_double * 64)()                                   # host memory standing in for pointers that are never followed
    p = ctypes.addressof(buf)
    good = [p] * 13 + [2, 64, 9, None]

    def refused(word, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        status = lib.mau_raw_tile_process(*args)
        msg = lib.mau_last_error().decode()
        assert status == MAU_ERR_ARG and msg.startswith("raw_tile_process: ") and word in msg, (change, status, msg)

    for k in range(7):
        refused("null pointer (an input)", **{f"a{k}": None})
    refused("nothing asked for", a8=None, a9=None, a10=None)
    refused("cont and targets come together", a9=None)
    refused("cont and targets come together", a10=None)
    refused("need norm", a7=None)
    refused("rows need ws and tickets", a11=None)
    refused("rows need ws and tickets", a12=None)
    for B, HW in ((0, 64), (2, 0), (-1, 64), (2, -4)):
        refused("non-positive size", a13=B, a14=HW)
    refused("at most 2^30 pixels", a14=(1 << 30) + 1)
    refused("at most 2^24 samples", a13=(1 << 24) + 1)
    for nc in (0, 17, -1):
        refused("num_classes must be in [1,16]", a15=nc)
    for k in (2, 3, 4, 5, 6, 9, 10):
        refused("fp32 planes must be 4-byte aligned", **{f"a{k}": p + 2})
    for k in (7, 8, 11):
        refused("8-byte aligned", **{f"a{k}": p + 4})
    refused("tickets must be 4-byte aligned", a12=p + 2)


# --------------------------------------------------------------------------- #
# the command line
# --------------------------------------------------------------------------- #
def test_command_line_exit_codes_and_the_one_line_error(DB, raw_dir, tmp_path, capsys):
    import mau_amd
    assert mau_amd.dataset_build is DB and "dataset_build" in mau_amd.__all__
    temperature = os.path.join(FIX, "temperature.npz")
    out = tmp_path / "processed"
    shutil.copytree(os.path.join(FIX, "reference"), out, ignore=shutil.ignore_patterns("*.npz", "kept.json"))
    argv = ["--raw-dir", raw_dir, "--processed-dir", str(out), "--temperature", temperature, "--cities-csv", os.path.join(FIX, "cities.csv"),
            "--device", "cpu", "--batch-size", "2"]
    assert DB.main(argv) == 0
    capsys.readouterr()
    assert_tiles_are_the_recorded_ones(out, "command line, --device cpu")

    def fails(args, word):
        assert DB.main(args) == 1
        lines = capsys.readouterr().out.strip().split("\n")
        assert lines[-1].startswith("Error: ") and word in lines[-1] and sum(1 for x in lines if x.startswith("Error")) == 1, lines

    fails(["--raw-dir", str(tmp_path / "nowhere"), "--processed-dir", str(out), "--temperature", temperature, "--device", "cpu"], "Raw tile directory not found")
    fails(argv[:4] + ["--temperature", str(tmp_path / "none.npz"), "--device", "cpu"], "none.npz")
    (tmp_path / "empty").mkdir()
    fails(["--raw-dir", str(tmp_path / "empty"), "--processed-dir", str(out), "--temperature", temperature, "--device", "cpu"], "No (t1, t2) samples")
    fails(argv[:-1] + ["0"], "batch size must be positive")
    with pytest.raises(SystemExit) as e:
        DB.main(["--raw-dir", raw_dir])
    assert e.value.code == 2 and "--processed-dir" in capsys.readouterr().err
