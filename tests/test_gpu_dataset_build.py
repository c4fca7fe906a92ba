"""``mau_amd.dataset_build`` on the device: the rows of ``mau_raw_tile_process`` against the float64 twin and its normalised planes bit
for bit against ``normalise_host`` at every load path and chunk count, the three modes, bitwise repeatability and batch independence,
one NaN pixel, an out-of-range class, the refusals of the C entry point, and the fixture recorded from the reference
(tests/golden/buildfix*) through ``build`` end to end.  Tiles of at most 66 x 66 (one run of two 250 x 250 tiles), batches of at most 8.

Bounds.  Counts and n: exact.  Means, sqrt(M2 / n) and the two sums (as means): 1e-10 of the plane's RMS -- test_gpu_ground_truth.TOL
and its derivation (n * 2^-53 ~ 7e-12 at n = 62 500, x 10); for the |difference| sums the RMS is that of the difference plane.  The
planes: bit for bit (numpy's own float32 / float64 operations, each correctly rounded, nothing contracted)."""
import json
import os

import numpy as np
import pytest
import torch

from tests._helpers import bits, mau  # noqa: F401
from tests.test_dataset_build_host import raw_dir  # noqa: F401
from tests.test_dataset_build_host import (FIX, NORM, assert_kept_is_the_references, assert_tiles_are_the_recorded_ones, make_raw,
                                           reference_kept, run_build)

pytestmark = pytest.mark.gpu

TOL = 1e-10
SHAPES = [(3, 24, 24), (2, 64, 64), (3, 66, 66), (2, 65, 63), (2, 250, 250)]
IDS = ["24x24-one-partial-chunk", "64x64-one-full-chunk", "66x66-two-chunks-vec4", "65x63-scalar", "250x250-16-chunks"]


@pytest.fixture(scope="module")
def DB(mau):
    return mau.dataset_build


def on_device(DB, raw, norm=None, rows=True, planes=False):
    out = DB.raw_tile_process(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in raw), norm=norm, rows=rows, planes=planes)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def assert_rows_close(DB, got, want, raw, what):
    assert got.shape == want.shape and got.dtype == np.float64
    exact = list(range(DB.OOR + 2)) + [DB.NDVI_BAD, DB.TEMP_BAD] + [DB.MOM0 + 4 * p + k for p in range(DB.N_MOM) for k in (DB.M_N, DB.M_BAD)]
    assert np.array_equal(got[:, exact], want[:, exact]), what
    n = want[:, DB.MOM0]
    worst = 0.0
    for p in range(DB.N_MOM):
        g, w = got[:, DB.MOM0 + 4 * p:][:, :4], want[:, DB.MOM0 + 4 * p:][:, :4]
        rms = np.sqrt(w[:, DB.M_M2] / n + w[:, DB.M_MEAN] ** 2)
        worst = max(worst, float(np.max(np.abs(g[:, DB.M_MEAN] - w[:, DB.M_MEAN]) / rms)),
                    float(np.max(np.abs(np.sqrt(g[:, DB.M_M2] / n) - np.sqrt(w[:, DB.M_M2] / n)) / rms)))
    for at, (x1, x2) in ((DB.NDVI_L1, (raw[3], raw[4])), (DB.TEMP_L1, (raw[5], raw[6]))):
        d = x2.astype(np.float64) - x1.astype(np.float64)
        rms = np.sqrt(np.mean(d.reshape(d.shape[0], -1) ** 2, axis=1))
        worst = max(worst, float(np.max(np.abs(got[:, at] - want[:, at]) / n / rms)))
    print(f"{what}: worst |difference| / plane RMS = {worst:.3g} (bound {TOL:g})")
    assert worst <= TOL, (what, worst)


# --------------------------------------------------------------------------- #
# the kernel against the twins
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def cases(DB):
    """Per shape: the raw batch, the twin's rows and planes (computed once) and the device's results in the three modes."""
    out = {}
    for (B, H, W) in SHAPES:
        raw = make_raw(B, H, W, 100 + H + W)
        out[(B, H, W)] = {"raw": raw, "rows": DB.raw_rows_host(*raw), "planes": DB.normalise_host(*raw[2:], NORM),
                          "both": on_device(DB, raw, NORM, True, True), "rows_only": on_device(DB, raw, None, True, False),
                          "planes_only": on_device(DB, raw, NORM, False, True)}
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_against_the_float64_twin(DB, cases, shape):
    c = cases[shape]
    B, H, W = shape
    want = c["rows"]
    t1 = want[:, DB.MOM0 + 12:][:, :4]
    assert np.all(np.abs(t1[:, DB.M_MEAN]) >= 900 * np.sqrt(t1[:, DB.M_M2] / (H * W)))           # |mean| ~ 1000 std
    assert np.all(want[:, [2, 4, 5, 7]] == 0) and np.all(want[:, [0, 1, 3, 6, 8]] > 0) and np.all(want[:, 9:18] == 0)
    rows = c["rows_only"][0]
    assert rows.shape == (B, DB.ROW) and c["rows_only"][1] is None and c["rows_only"][2] is None
    assert_rows_close(DB, rows, want, c["raw"], f"raw_tile_process rows {B}x{H}x{W}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_normalised_planes_bit_for_bit(DB, cases, shape):
    c = cases[shape]
    raw, (cont, tgt) = c["raw"], c["planes"]
    _, gc, gt = c["planes_only"]
    assert gc.shape == cont.shape and gt.shape == tgt.shape and gc.dtype == gt.dtype == np.float32
    for p in range(5):
        assert np.array_equal(bits(gc[:, p]), bits(cont[:, p])), (shape, "cont", p, int((bits(gc[:, p]) != bits(cont[:, p])).sum()))
    for p in range(2):
        assert np.array_equal(bits(gt[:, p]), bits(tgt[:, p])), (shape, "targets", p, int((bits(gt[:, p]) != bits(tgt[:, p])).sum()))
    assert np.array_equal(bits(gc[:, 3]), bits(raw[3])) and np.array_equal(bits(gt[:, 0]), bits(raw[4]))      # NDVI passes through


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_three_modes_give_the_same_bits(DB, cases, shape):
    c = cases[shape]
    rows, cont, tgt = c["both"]
    assert np.array_equal(bits(rows), bits(c["rows_only"][0]))
    assert np.array_equal(bits(cont), bits(c["planes_only"][1])) and np.array_equal(bits(tgt), bits(c["planes_only"][2]))


def test_division_is_correctly_rounded_on_awkward_quotients(DB):
    """Every fp32 quotient (t - m) / s and every fp64 one of the RGB planes against numpy, with divisors and values chosen freely:
    subnormal and huge results, a negative std."""
    rng = np.random.default_rng(9)
    a, b, rgb, n1, n2, t1, t2 = make_raw(2, 64, 64, 77)
    t1 = (rng.standard_normal(t1.shape) * 10.0 ** rng.integers(-30, 30, t1.shape)).astype(np.float32)
    t2 = np.ldexp(rng.uniform(1, 2, t2.shape), rng.integers(-149, 100, t2.shape)).astype(np.float32)
    rgb = rng.uniform(0, 255, rgb.shape).astype(np.float32)
    for norm in ([0.3, 0.5, 0.7, 0.29, 1e-3, 3.0, 0.0, 3.0], [0.1, 0.2, 0.3, -0.7, 123.0, 1.0 / 3.0, 1e-3, -7.0e5], [0, 0, 0, 1, 1, 1, 2.5e-40, 1.17e-38]):
        want_c, want_t = DB.normalise_host(rgb, n1, n2, t1, t2, norm)
        _, cont, tgt = on_device(DB, (a, b, rgb, n1, n2, t1, t2), norm, False, True)
        assert np.array_equal(bits(cont), bits(want_c)), (norm, [int((bits(cont[:, p]) != bits(want_c[:, p])).sum()) for p in range(5)])
        assert np.array_equal(bits(tgt), bits(want_t)), (norm, int((bits(tgt) != bits(want_t)).sum()))


# --------------------------------------------------------------------------- #
# repeatability and independence
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("hw", [(66, 66), (65, 63)], ids=["vec4", "scalar"])
def test_results_repeat_and_do_not_depend_on_the_batch(DB, hw):
    raw = make_raw(8, *hw, 8)
    first = on_device(DB, raw, NORM, True, True)

    def same(got, sel=slice(None)):
        return all(np.array_equal(bits(g), bits(f[sel])) for g, f in zip(got, first))

    assert same(on_device(DB, raw, NORM, True, True))
    lo, hi = on_device(DB, tuple(x[:3] for x in raw), NORM, True, True), on_device(DB, tuple(x[3:] for x in raw), NORM, True, True)
    assert same(lo, slice(0, 3)) and same(hi, slice(3, 8))
    assert same(on_device(DB, tuple(x[::-1] for x in raw), NORM, True, True), slice(None, None, -1))
    # a base misaligned by 4 bytes is cloned: the load path, and with it the bits, stay a function of H * W alone
    dev = [torch.from_numpy(x).cuda() for x in raw]
    flat = torch.zeros(raw[5].size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = dev[5].reshape(-1)
    shifted = flat[1:].view(raw[5].shape)
    assert shifted.data_ptr() % 16 == 4
    dev[5] = shifted
    assert same(tuple(t.cpu().numpy() for t in DB.raw_tile_process(*dev, norm=NORM, rows=True, planes=True)))


def test_more_samples_than_tickets(DB):
    from mau_amd._lib import lib
    per = lib.mau_reduce_tickets_elems()
    raw = make_raw(2, 24, 24, 5)
    one = on_device(DB, raw, NORM, True, True)
    idx = np.arange(per + 3) % 2
    many = on_device(DB, tuple(x[idx] for x in raw), NORM, True, True)                 # two launches share one workspace
    assert all(np.array_equal(bits(m), bits(o[idx])) for m, o in zip(many, one))


# --------------------------------------------------------------------------- #
# bad values
# --------------------------------------------------------------------------- #
def test_one_nan_pixel_stays_in_its_sample(DB):
    raw = list(make_raw(3, 66, 66, 21))
    clean = on_device(DB, raw, NORM, True, True)
    raw[3] = raw[3].copy()
    raw[3][1, 63, 10] = np.nan                                                         # ndvi_t1, pixel 4168: the second chunk
    rows, cont, tgt = on_device(DB, raw, NORM, True, True)
    assert np.array_equal(bits(rows[[0, 2]]), bits(clean[0][[0, 2]]))                  # bit-identical: the other samples ...
    touched = np.zeros(DB.ROW, dtype=bool)
    touched[[DB.NDVI_L1, DB.NDVI_BAD]] = True
    assert np.array_equal(bits(rows[1, ~touched]), bits(clean[0][1, ~touched]))         # ... and every entry that does not read the plane
    assert rows[1, DB.NDVI_BAD] == 1 and np.isnan(rows[1, DB.NDVI_L1]) and rows[1, DB.TEMP_BAD] == 0
    want = clean[1].copy()
    want[1, 3, 63, 10] = np.nan
    assert np.array_equal(bits(cont), bits(want)) and np.array_equal(bits(tgt), bits(clean[2]))
    assert DB.row_decision(rows[1]) == (False, "1 non-finite values (the reference would carry NaN into the metrics file and every tile)")
    assert DB.row_decision(rows[0]) == (True, None)


def test_out_of_range_class_is_counted(DB):
    raw = list(make_raw(2, 24, 24, 33))
    clean = on_device(DB, raw)[0]
    raw[1] = raw[1].copy()
    was_a, was_b = int(raw[0][1, 5, 7]), int(raw[1][1, 5, 7])
    raw[1][1, 5, 7] = 9
    rows = on_device(DB, raw)[0]
    assert rows[1, DB.OOR + 1] == 1 and rows[1, DB.OOR] == 0 and rows[0, DB.OOR:DB.OOR + 2].tolist() == [0, 0]
    want = clean.copy()
    want[1, DB.OOR + 1] = 1
    if was_a == was_b:
        want[1, was_a] += 1                                                            # dw_t1 is of that class there, dw_t2 no longer
    else:
        want[1, was_b] -= 1
    assert np.array_equal(rows, want)
    assert DB.row_decision(rows[1]) == (False, "1 class values outside [0, 9)")


# --------------------------------------------------------------------------- #
# the fixture directory, end to end on the device
# --------------------------------------------------------------------------- #
def test_build_with_the_references_metrics_gives_its_tiles_bit_for_bit(DB, raw_dir, tmp_path, capsys):
    out = tmp_path / "processed"
    res = run_build(DB, raw_dir, out, "cuda", True, batch_size=3)
    log = capsys.readouterr().out
    assert "Loading existing normalization metrics" in log
    assert "Failed during filtering for sample Quito_4: 1 class values outside [0, 9)" in log and log.count("due to negligible changes") == 3
    assert_kept_is_the_references(res, out)
    assert_tiles_are_the_recorded_ones(out, "build(cuda) with the reference's metrics")
    # a NaN pixel: the sample is dropped with a message
    import shutil
    raw2 = tmp_path / "raw"
    shutil.copytree(raw_dir, raw2)
    name = "Lagos_3_6.5244_3.3792_0.0_0.0_2023_02_ndvi.npy"
    x = np.load(raw2 / name)
    x[7, 7] = np.nan
    np.save(raw2 / name, x)
    res2 = run_build(DB, str(raw2), tmp_path / "processed2", "cuda", True)
    assert "Failed during filtering for sample Lagos_3: 1 non-finite values" in capsys.readouterr().out
    assert sorted(res2["kept"]["train"]) == [n for n in reference_kept()["train"] if not n.startswith("Lagos")]


def test_build_from_nothing_and_the_tools_downstream(DB, raw_dir, tmp_path, capsys):
    out = tmp_path / "processed"
    res = run_build(DB, raw_dir, out, "cuda", False, batch_size=2)
    assert "Saved new normalization metrics" in capsys.readouterr().out
    assert_kept_is_the_references(res, out)
    text = open(out / "normalization_metrics.json").read()
    got = json.loads(text)
    assert got == res["metrics"] and list(got) == DB.METRIC_KEYS and text == json.dumps(got, indent=4)
    twin = run_build(DB, raw_dir, tmp_path / "twin", "cpu", False)["metrics"]
    for k in ("meta_mean", "meta_std", "temp_series_mean", "temp_series_std"):
        assert got[k] == twin[k], k                                                    # host arithmetic on both sides
    rms_rgb = np.hypot(twin["rgb_mean"], twin["rgb_std"])
    rms_t = float(np.hypot(twin["temp_mean"], twin["temp_std"]))
    worst = max(float(np.max(np.abs(np.subtract(got["rgb_mean"], twin["rgb_mean"])) / rms_rgb)),
                float(np.max(np.abs(np.subtract(got["rgb_std"], twin["rgb_std"])) / rms_rgb)),
                abs(got["temp_mean"] - twin["temp_mean"]) / rms_t, abs(got["temp_std"] - twin["temp_std"]) / rms_t)
    print(f"build(cuda) metrics vs the twin: worst |difference| / plane RMS = {worst:.3g} (bound {TOL:g})")
    assert worst <= TOL
    # the directory is a processed dataset: the loader and the survey read it
    import mau_amd
    from mau_amd.data import FuturePredictionDataset, collate_fn
    ds = FuturePredictionDataset("train", processed_dir=str(out), compact=True)
    assert len(ds) == 3
    batch = collate_fn([ds[i] for i in range(3)])
    assert batch.cls_a.shape == (3, 16, 16) and batch.cont.shape == (3, 5, 16, 16) and batch.targets.shape == (3, 2, 16, 16)
    df = mau_amd.dataset_metrics.extract(str(out), batch_size=2)
    assert len(df) == 5 and df["split"].tolist() == ["test", "train", "train", "train", "val"]
    assert bool(np.isfinite(df["input_temp_t1_mean"]).all()) and abs(float(df[df["split"] == "train"]["input_temp_t1_mean"].mean())) < 1e-3


# --------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------- #
def test_a_refused_call_leaves_the_next_one_working(DB):
    from mau_amd import _lib
    lib = _lib.lib
    raw = make_raw(2, 8, 12, 1)
    dev = [torch.from_numpy(x).cuda() for x in raw]
    for args, err in (((dev[0].int(),) + tuple(dev[1:]), TypeError), ((dev[0][0],) + tuple(dev[1:]), ValueError),
                      (tuple(dev[:2]) + (dev[2][:, :2],) + tuple(dev[3:]), ValueError), (tuple(dev[:6]) + (dev[6].cpu(),), RuntimeError)):
        with pytest.raises(err):
            DB.raw_tile_process(*args)
    with pytest.raises(ValueError, match="need norm"):
        DB.raw_tile_process(*dev, planes=True)
    with pytest.raises(ValueError, match="nothing asked for"):
        DB.raw_tile_process(*dev, rows=False)
    rows = torch.full((2, DB.ROW), -7.0, dtype=torch.float64, device="cuda")
    cont = torch.full((2, 5, 8, 12), -7.0, device="cuda")
    tgt = torch.full((2, 2, 8, 12), -7.0, device="cuda")
    norm = torch.tensor(NORM, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.mau_raw_tile_ws_elems(2, 96), dtype=torch.float64, device="cuda")
    tick = torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device="cuda")
    good = [t.data_ptr() for t in dev] + [norm.data_ptr(), rows.data_ptr(), cont.data_ptr(), tgt.data_ptr(), ws.data_ptr(), tick.data_ptr(), 2, 96, 9, None]
    cases = [(k, None, "null pointer") for k in range(7)] + [(7, None, "need norm"), (9, None, "come together"), (11, None, "rows need ws"),
                                                              (13, 0, "non-positive"), (14, 0, "non-positive"), (14, (1 << 30) + 1, "2^30"),
                                                              (15, 0, "num_classes"), (15, 17, "num_classes"), (2, dev[2].data_ptr() + 2, "aligned"),
                                                              (10, tgt.data_ptr() + 1, "aligned"), (8, rows.data_ptr() + 4, "aligned")]
    for k, v, word in cases:
        args = list(good)
        args[k] = v
        assert lib.mau_raw_tile_process(*args) == 1 and word in lib.mau_last_error().decode(), (k, v)
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((cont == -7.0).all()) and bool((tgt == -7.0).all()) and int(tick.abs().sum()) == 0
    assert lib.mau_raw_tile_process(*good) == 0                                        # ... and the same arguments, unchanged, run
    torch.cuda.synchronize()
    want = DB.raw_tile_process(*dev, norm=norm, rows=True, planes=True)
    assert torch.equal(rows, want[0]) and torch.equal(cont, want[1]) and torch.equal(tgt, want[2]) and int(tick.abs().sum()) == 0
