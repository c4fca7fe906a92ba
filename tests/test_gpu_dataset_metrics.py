"""``mau_amd.dataset_metrics`` on the device: ``mau_tile_stats`` against its float64 numpy twin at every load path and chunk count,
bitwise repeatability and batch independence, one NaN pixel, an out-of-range class, the refusals of the wrapper and of the C entry
point, and the fixture directory recorded from the reference (tests/golden/surveyfix*) through ``extract`` and the command line.
Tiles of at most 66 x 66 (one run of two 250 x 250 tiles), batches of at most 8; made-up normalisation numbers."""
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import mau  # noqa: F401
from tests.test_dataset_metrics_host import FIX, GOLDEN, assert_rows_match

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = {"temp_mean": 296.4173, "temp_std": 11.0291, "temp_series_mean": 295.75, "temp_series_std": 9.125,
           "meta_mean": [17.25, 9.5, 1250000.5, 2.125], "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
TOL = 1e-10        # relative to the RMS of the plane: test_gpu_ground_truth.TOL and its derivation (n * 2^-53 ~ 7e-12 at n = 62 500, x 10)


@pytest.fixture(scope="module")
def D(mau):
    return mau.dataset_metrics


def make_batch(B, H, W, seed):
    """Class maps in which classes 2, 4, 5 and 7 never occur; a temperature plane with |mean| a thousand times its std."""
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0, 1, 3, 6, 8], dtype=np.uint8), (B, H, W))
    b = a.copy()
    flip = rng.random((B, H, W)) < 0.25
    b[flip] = rng.choice(np.array([0, 1, 3, 6, 8], dtype=np.uint8), int(flip.sum()))
    rgb = rng.uniform(0, 1, (B, 3, H, W))
    ndvi1 = np.tanh(0.6 * rng.standard_normal((B, 1, H, W)) + rng.uniform(-0.5, 0.5, (B, 1, 1, 1)))
    t1 = 50.0 * rng.choice([-1.0, 1.0], (B, 1, 1, 1)) + 0.05 * rng.standard_normal((B, 1, H, W))
    cont = np.concatenate([rgb, ndvi1, t1], axis=1).astype(np.float32)
    tgt = np.concatenate([np.clip(ndvi1 + 0.1 * rng.standard_normal((B, 1, H, W)), -1, 1),
                          t1 + 0.01 * rng.standard_normal((B, 1, H, W)) + 0.02], axis=1).astype(np.float32)
    return a, b, cont, tgt


def on_device(D, a, b, cont, tgt):
    return D.tile_stats(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, b, cont, tgt)))


def assert_rows_close(D, got, want, what):
    """Counts, n, min, max and both bad-value counts exact; mean, sqrt(M2 / n) and sum |x| / n within TOL of the plane's RMS."""
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got[:, :D.PLANES0], want[:, :D.PLANES0])
    g, w = got[:, D.PLANES0:].reshape(-1, D.N_PLANES, D.PLANE_ROW), want[:, D.PLANES0:].reshape(-1, D.N_PLANES, D.PLANE_ROW)
    for k in (D.P_N, D.P_MIN, D.P_MAX, D.P_NAN, D.P_BAD):
        assert np.array_equal(g[..., k], w[..., k]), (what, k)
    n = w[..., D.P_N]
    rms = np.sqrt(w[..., D.P_M2] / n + w[..., D.P_MEAN] ** 2)
    worst = max(float(np.max(np.abs(g[..., D.P_MEAN] - w[..., D.P_MEAN]) / rms)),
                float(np.max(np.abs(np.sqrt(g[..., D.P_M2] / n) - np.sqrt(w[..., D.P_M2] / n)) / rms)),
                float(np.max(np.abs(g[..., D.P_L1] - w[..., D.P_L1]) / n / rms)))
    print(f"{what}: worst |difference| / plane RMS = {worst:.3g} (bound {TOL:g})")
    assert worst <= TOL, (what, worst)


# --------------------------------------------------------------------------- #
# the kernel against the twin
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,H,W", [(3, 24, 24), (2, 64, 64), (3, 66, 66), (2, 65, 63), (2, 250, 250)],
                         ids=["24x24-one-partial-chunk", "64x64-one-full-chunk", "66x66-two-chunks-vec4", "65x63-scalar", "250x250-16-chunks"])
def test_tile_stats_against_the_float64_twin(D, B, H, W):
    a, b, cont, tgt = make_batch(B, H, W, 100 + H + W)
    want = D.tile_rows_host(a, b, cont, tgt)
    planes = want[:, D.PLANES0:].reshape(B, D.N_PLANES, D.PLANE_ROW)
    assert np.all(np.abs(planes[:, 4, D.P_MEAN]) >= 900 * np.sqrt(planes[:, 4, D.P_M2] / (H * W)))     # |mean| ~ 1000 std
    assert np.all(want[:, [2, 4, 5, 7]] == 0) and np.all(want[:, [0, 1, 3, 6, 8]] > 0) and np.all(want[:, 9:16] == 0)
    rows = on_device(D, a, b, cont, tgt)
    assert rows.shape == (B, D.ROW) and rows.dtype == torch.float64 and rows.is_cuda
    assert_rows_close(D, rows.cpu().numpy(), want, f"tile_stats {B}x{H}x{W}")


@pytest.mark.parametrize("hw", [(66, 66), (65, 63)], ids=["vec4", "scalar"])
def test_rows_repeat_bit_for_bit_and_do_not_depend_on_the_batch(D, hw):
    a, b, cont, tgt = make_batch(8, *hw, 8)
    rows = on_device(D, a, b, cont, tgt)
    assert torch.equal(rows, on_device(D, a, b, cont, tgt))
    parts = torch.cat([on_device(D, a[:3], b[:3], cont[:3], tgt[:3]), on_device(D, a[3:], b[3:], cont[3:], tgt[3:])])
    assert torch.equal(parts, rows)
    rev = on_device(D, a[::-1], b[::-1], cont[::-1], tgt[::-1])
    assert torch.equal(rev.flip(0), rows)
    # a misaligned base is cloned: the load path, and with it the bits, stay a function of H * W alone
    flat = torch.zeros(cont.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(cont).cuda().reshape(-1)
    shifted = flat[1:].view(cont.shape)
    assert shifted.data_ptr() % 16 == 4
    ta, tb, tt = (torch.from_numpy(x).cuda() for x in (a, b, tgt))
    assert torch.equal(D.tile_stats(ta, tb, shifted, tt), rows)


def test_more_samples_than_tickets(D):
    from mau_amd._lib import lib
    per = lib.mau_reduce_tickets_elems()
    a, b, cont, tgt = make_batch(2, 24, 24, 5)
    one = on_device(D, a, b, cont, tgt)
    idx = np.arange(per + 3) % 2
    many = on_device(D, a[idx], b[idx], cont[idx], tgt[idx])                           # two launches share one workspace
    assert torch.equal(many, one[torch.from_numpy(idx).cuda()])


# --------------------------------------------------------------------------- #
# bad values
# --------------------------------------------------------------------------- #
def test_one_nan_pixel(D):
    a, b, cont, tgt = make_batch(3, 66, 66, 21)
    clean = on_device(D, a, b, cont, tgt).cpu().numpy()
    cont[1, 3, 63, 10] = np.nan                                                        # ndvi_t1, pixel 4168: the second chunk
    rows = on_device(D, a, b, cont, tgt).cpu().numpy()
    reads = np.zeros(D.ROW, dtype=bool)
    for p in (3, D.PLANE_NDVI_DIFF):
        reads[D.PLANES0 + p * D.PLANE_ROW:D.PLANES0 + (p + 1) * D.PLANE_ROW] = True
    assert np.array_equal(rows[[0, 2]], clean[[0, 2]])                                 # bit-identical: the other samples ...
    assert np.array_equal(rows[1, ~reads], clean[1, ~reads])                           # ... and every entry that does not read the plane
    for p in (3, D.PLANE_NDVI_DIFF):
        pr = rows[1, D.PLANES0 + p * D.PLANE_ROW:][:D.PLANE_ROW]
        assert pr[D.P_N] == 66 * 66 and pr[D.P_NAN] == 1 and pr[D.P_BAD] == 1
        assert math.isnan(pr[D.P_MEAN]) and math.isnan(pr[D.P_M2]) and math.isnan(pr[D.P_L1])
        cp = clean[1, D.PLANES0 + p * D.PLANE_ROW:][:D.PLANE_ROW]
        assert pr[D.P_MIN] <= pr[D.P_MAX] and pr[D.P_MIN] >= cp[D.P_MIN] and pr[D.P_MAX] <= cp[D.P_MAX]     # of the other 4355 values
    md, ts = np.zeros((3, 4), np.float32), np.zeros((3, 14), np.float32)
    m, c = D.sample_metrics(rows, md, ts, [14] * 3, METRICS), D.sample_metrics(clean, md, ts, [14] * 3, METRICS)
    nan_cols = [f"{n}_{k}" for n in ("input_ndvi_t1", "ndvi_diff") for k in ("mean", "std", "min", "max")] + ["delta_ndvi_l1_norm", "delta_ndvi_l2_norm"]
    for col in D.COLUMNS[2:]:
        if col in nan_cols:
            assert math.isnan(m[1][col]) and not math.isnan(c[1][col]), col
        else:
            assert m[1][col] == c[1][col] or (math.isnan(m[1][col]) and math.isnan(c[1][col])), col
    assert all(m[i][col] == c[i][col] or math.isnan(c[i][col]) for i in (0, 2) for col in D.COLUMNS[2:])


def test_out_of_range_class_is_counted_and_refused_by_the_driver(D):
    a, b, cont, tgt = make_batch(2, 24, 24, 33)
    clean = on_device(D, a, b, cont, tgt).cpu().numpy()
    D.check_class_range(clean)
    was = int(b[1, 5, 7])
    b[1, 5, 7] = 9
    rows = on_device(D, a, b, cont, tgt).cpu().numpy()                                 # a direct call still returns
    assert rows[1, D.OOR + 1] == 1 and rows[1, D.OOR] == 0 and rows[0, D.OOR:D.OOR + 2].tolist() == [0, 0]
    assert rows[1, 16 + was] == clean[1, 16 + was] - 1 and rows[1, 16:32].sum() == 24 * 24 - 1
    keep = np.ones(D.ROW, dtype=bool)
    keep[[16 + was, D.OOR + 1]] = False
    assert np.array_equal(rows[:, keep], clean[:, keep])
    with pytest.raises(ValueError, match="sample 1 .* 1 class values outside"):
        D.check_class_range(rows)


def test_refusals_of_the_wrapper_and_of_the_entry_point(D):
    from mau_amd import _lib
    a, b, cont, tgt = (torch.from_numpy(x).cuda() for x in make_batch(2, 8, 12, 1))
    for args in ((a.int(), b, cont, tgt), (a, b.float(), cont, tgt), (a, b, cont.double(), tgt), (a, b, cont, tgt.half()), (a.cpu().numpy(), b, cont, tgt)):
        with pytest.raises(TypeError):
            D.tile_stats(*args)
    for args in ((a[0], b, cont, tgt), (a, b[:1], cont, tgt), (a, b, cont[:, :4], tgt), (a, b, cont, tgt[:, :1]), (a, b, cont[..., :8], tgt),
                 (a[:0], b[:0], cont[:0], tgt[:0]), (a, b, cont, torch.cat([tgt, tgt], 1))):
        with pytest.raises(ValueError):
            D.tile_stats(*args)
    for args in ((a.cpu(), b, cont, tgt), (a, b, cont, tgt.cpu())):
        with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
            D.tile_stats(*args)
    # the C entry point: MAU_ERR_ARG and a message; the rows it was handed stay as they were (no launch)
    lib = _lib.lib
    rows = torch.full((2, D.ROW), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.mau_tile_stats_ws_elems(2, 96), dtype=torch.float64, device="cuda")
    tick = torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device="cuda")
    good = [a.data_ptr(), b.data_ptr(), cont.data_ptr(), tgt.data_ptr(), rows.data_ptr(), ws.data_ptr(), tick.data_ptr(), 2, 96, 9, None]
    cases = [(k, None, "null pointer") for k in range(7)] + [(7, 0, "non-positive"), (8, 0, "non-positive"), (8, (1 << 30) + 1, "2^30"),
                                                              (9, 0, "num_classes"), (9, 17, "num_classes"), (2, cont.data_ptr() + 2, "aligned"),
                                                              (3, tgt.data_ptr() + 1, "aligned")]
    for k, v, word in cases:
        args = list(good)
        args[k] = v
        assert lib.mau_tile_stats(*args) == 1 and word in lib.mau_last_error().decode(), (k, v)
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and int(tick.abs().sum()) == 0
    assert lib.mau_tile_stats(*good) == 0                                              # ... and the same arguments, unchanged, run
    torch.cuda.synchronize()
    assert torch.equal(rows, D.tile_stats(a, b, cont, tgt)) and int(tick.abs().sum()) == 0


# --------------------------------------------------------------------------- #
# the fixture directory, and the command line
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def survey_dir(tmp_path_factory):
    """The four fixture tiles and a fifth whose class planes are not one-hot."""
    root = tmp_path_factory.mktemp("survey") / "processed"
    shutil.copytree(FIX, root)
    z = np.load(root / "train" / "Roma_0_41.8990_12.4690_2019_08_to_2021_08.npz")
    arrays = {k: z[k].copy() for k in z.files}
    arrays["input"][0] *= 0.5
    np.savez_compressed(root / "train" / "Quito_9_-0.1807_-78.4678_2019_08_to_2021_08.npz", **arrays)
    return root


def test_fixture_directory_through_extract(D, survey_dir, capsys):
    import pandas as pd
    expected = pd.read_csv(os.path.join(GOLDEN, "surveyfix_expected.csv"), float_precision="round_trip")
    deviation = json.load(open(os.path.join(GOLDEN, "surveyfix_deviation.json")))
    df = D.extract(str(survey_dir), batch_size=3)
    out = capsys.readouterr().out
    assert f"Failed to process {survey_dir / 'train' / 'Quito_9_-0.1807_-78.4678_2019_08_to_2021_08.npz'}: compact_input" in out
    assert list(df.columns) == D.COLUMNS and len(df) == 4
    assert df["split"].tolist() == ["train", "train", "val", "val"] and df["filepath"].tolist() == sorted(df["filepath"][:2]) + sorted(df["filepath"][2:])
    got = {r["filepath"]: r for r in df.to_dict("records")}
    assert_rows_match(got, expected, deviation, "extract vs the reference's rows")
    one = D.extract(str(survey_dir / "val"), metrics_path=str(survey_dir / "normalization_metrics.json"))      # no split folders
    assert one["split"].tolist() == ["unknown", "unknown"]
    pd.testing.assert_frame_equal(one.drop(columns="split"), df[df["split"] == "val"].reset_index(drop=True).drop(columns="split"), check_exact=True)


def test_command_line_in_a_fresh_process(D, survey_dir, tmp_path):
    import pandas as pd
    df = D.extract(str(survey_dir), batch_size=64)
    csv = tmp_path / "reports" / "dataset_processed_metrics.csv"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.dataset_metrics", "extract", str(survey_dir), str(csv), "--batch-size", "2"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert f"Metrics for all splits saved to {csv}" in p.stdout and "Failed to process" in p.stdout
    back = pd.read_csv(csv, float_precision="round_trip")
    pd.testing.assert_frame_equal(back, df, check_exact=True)                          # batches of 2 instead of 64: the same bits
