"""``mau_amd.climate`` on the device: the three kernels of csrc/climate.hip against their float64 numpy twins -- baseline rows and
anomalies bit for bit at every seam of the launch geometry (one partial workgroup, a workgroup boundary, the last partial group of
the unrolled time loop, the 16-byte and the two 4-byte paths), the batched query against the normalised grid's columns, its moment
rows, batch independence and repeatability -- and ``process`` / ``ClimateQuery`` on the fixture (tests/golden/climatefix; it records
the reference's arithmetic in numpy, float32 np.nanmean / np.nanstd and float32 (tas - mean) / std, which is what xarray dispatches to
without bottleneck and is unverified against xarray itself: see tests/test_climate_host.py) against ``device="cpu"``.

Seeded grids of at most 4096 x 37 and 828 x 1028 values, about 10 % NaN.

Bounds.  Baseline rows, anomalies and series values: bit for bit (every operation is an IEEE fp64 operation in a fixed order, nothing
contracted); a NaN must be a NaN at the same place -- its sign and payload are not compared (0 / 0 is -NaN on the host, +NaN on the
device).  srows: n and the non-finite count exact, mean and sqrt(M2 / n) within 1e-10 of the series RMS -- test_gpu_dataset_build's
rule (the twin adds in numpy's order; n * 2^-53 ~ 5e-13 at n = 4096, x 10, with room)."""
import json
import os

import numpy as np
import pytest
import torch

from tests._helpers import bits, dev, mau  # noqa: F401
from tests.test_climate_host import BASELINE_YEARS, FIX, YEARS, make_grid, recorded_queries

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def CL(mau):
    return mau.climate


def assert_same_bits(got, want, what):
    """The same bits wherever the twin is not NaN, a NaN wherever it is."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions", int((np.isnan(got) != nan).sum()))
    differ = (bits(got) != bits(want)) & ~nan
    assert not differ.any(), (what, int(differ.sum()), got[differ][:4], want[differ][:4])


# --------------------------------------------------------------------------- #
# baseline
# --------------------------------------------------------------------------- #
def edge_column(kind, T):
    col = np.full(T, np.nan, dtype=np.float32)
    if kind == "single-value":                               # std 0
        col[T // 2] = 17.25
    elif kind == "inf":
        col[:] = np.linspace(-3, 9, T, dtype=np.float32)
        col[T - 1] = np.inf
    return col                                               # "all-nan" otherwise


@pytest.mark.parametrize("G", [1, 63, 256, 257, 1028])
@pytest.mark.parametrize("T", [1, 2, 7, 48, 600])
def test_baseline_rows_bit_for_bit(CL, T, G):
    x = make_grid(T, G, 1000 * T + G)
    for kind in ("seeded", "all-nan", "single-value", "inf"):
        if kind != "seeded":
            x[:, G - 1] = edge_column(kind, T)
        want = CL.baseline_host(x)
        got = CL.baseline(dev(x)).cpu().numpy()
        assert_same_bits(got, want, f"baseline {T}x{G} {kind}")
        last = got[G - 1]
        if kind == "all-nan":
            assert last[0] == 0 and np.isnan(last[1]) and np.isnan(last[2]) and last[3] == T
        elif kind == "single-value":
            assert last.tolist() == [1.0, 17.25, 0.0, T - 1.0]
        elif kind == "inf":
            assert last[0] == T and last[3] == 0 and last[1] == np.inf and np.isnan(last[2])
    assert np.all(want[:, 0] + want[:, 3] == T)
    if T >= 48 and G >= 63:
        assert 0.05 * T * G < want[:-1, 3].sum() < 0.15 * T * G                       # about 10 % NaN, skipped and counted


def test_baseline_takes_the_lat_lon_grid_and_repeats(CL):
    x = make_grid(48, 6 * 8, 3).reshape(48, 6, 8)
    a, b = CL.baseline(dev(x)), CL.baseline(dev(x))
    assert a.shape == (48, 4) and a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))
    # a cell's bits depend on its own column only: the same cells inside a wider grid
    wide = np.concatenate([make_grid(48, 300, 4), x.reshape(48, 48)], axis=1)
    assert torch.equal(CL.baseline(dev(wide))[300:].view(torch.int64), a.view(torch.int64))
    for bad in (x.astype(np.float64), x[0, 0], x[:0]):
        with pytest.raises(ValueError, match="baseline: x must be"):
            CL.baseline(dev(bad))
    with pytest.raises(ValueError, match="torch tensor"):
        CL.baseline(x)


# --------------------------------------------------------------------------- #
# normalise
# --------------------------------------------------------------------------- #
def rows_with_edges(CL, G, seed):
    """Baseline rows of another seeded grid, with a cell of zero variance and an empty cell among them."""
    rows = CL.baseline_host(make_grid(24, G, seed))
    rows[G // 2] = [1.0, 4.5, 0.0, 23.0]
    rows[G - 1] = [0.0, np.nan, np.nan, 24.0]
    return rows


@pytest.mark.parametrize("path", ["vec4", "scalar-by-size", "scalar-by-alignment"])
@pytest.mark.parametrize("T", [1, 36, 828])
def test_normalise_bit_for_bit(CL, T, path):
    G = 257 if path == "scalar-by-size" else 1028
    x = make_grid(T, G, 7 * T + G)
    x[0, G // 2] = 4.5                                        # 0 / 0 at the cell of zero variance, +-inf around it
    rows = rows_with_edges(CL, G, T + 1)
    want = CL.normalise_host(x, rows)
    if path == "scalar-by-alignment":
        buf = torch.empty(T * G + 1, dtype=torch.float32, device="cuda")
        xd = buf[1:].view(T, G)
        xd.copy_(torch.from_numpy(x))
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    else:
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
    got = CL.normalise(xd, dev(rows))
    assert got.shape == (T, G) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert_same_bits(got, want, f"normalise {T}x{G} {path}")
    assert np.isnan(got[:, G - 1]).all() and np.isnan(got[0, G // 2]) and (T == 1 or np.isinf(got[1:, G // 2][~np.isnan(x[1:, G // 2])]).all())
    assert np.isfinite(got).sum() > 0.8 * T * G


def test_normalise_keeps_the_shape_and_refuses_bad_arguments(CL):
    x = make_grid(12, 48, 9).reshape(12, 6, 8)
    rows = CL.baseline(dev(x))
    out = CL.normalise(dev(x), rows)
    assert out.shape == (12, 6, 8)
    assert_same_bits(out.cpu().numpy(), CL.normalise_host(x, rows.cpu().numpy()), "normalise (12, 6, 8)")
    with pytest.raises(ValueError, match="rows must be a float64"):
        CL.normalise(dev(x), rows[:40])
    with pytest.raises(ValueError, match="rows must be a float64"):
        CL.normalise(dev(x), rows.float())
    with pytest.raises(ValueError, match="x must be"):
        CL.normalise(dev(x).double(), rows)


# --------------------------------------------------------------------------- #
# series
# --------------------------------------------------------------------------- #
G_SERIES = 37


def series_case(CL, T):
    """The raw grid (NaN in every third cell only, so that most moment rows are finite), its rows, the twin's anomalies and 300
    queries: every keep of {0, 1, T - 1, T} first, cells repeated, two cells outside the grid."""
    rng = np.random.default_rng(50 + T)
    x = make_grid(T, G_SERIES, 40 + T, nan=0.0)
    holes = rng.random((T, G_SERIES)) < 0.1
    holes[:, np.arange(G_SERIES) % 3 != 0] = False
    x[holes] = np.nan
    rows = CL.baseline_host(make_grid(24, G_SERIES, 41 + T))
    cell = rng.integers(0, G_SERIES, 300).astype(np.int32)
    keep = rng.integers(0, T + 1, 300).astype(np.int32)
    keep[:8] = [0, 1, T - 1, T, 0, 1, T - 1, T]
    cell[4:8] = [0, 0, 3, 3]                                  # the same keeps on cells with NaN months
    cell[20], cell[21] = -1, G_SERIES
    cell[30:40] = 5                                           # repeated cells
    return x, rows, CL.normalise_host(x, rows), cell, keep


def check_series(T, Tpad, norm, cell, keep, out, srows, what):
    assert out.shape == (cell.size, Tpad) and out.dtype == np.float32 and srows.shape == (cell.size, 4) and srows.dtype == np.float64
    worst = 0.0
    for n, (c, k) in enumerate(zip(cell.tolist(), keep.tolist())):
        assert not bits(out[n, k:]).any(), (what, n, "padding")
        if not 0 <= c < G_SERIES:
            assert np.isnan(out[n, :k]).all() and srows[n, 0] == 0 and np.isnan(srows[n, 1]) and srows[n, 2] == 0 and srows[n, 3] == 0, (what, n)
            continue
        assert_same_bits(out[n, :k], norm[:k, c], f"{what} query {n} (cell {c}, keep {k})")
        v = out[n, :k].astype(np.float64)
        bad = int((~np.isfinite(v)).sum())
        assert srows[n, 0] == k and srows[n, 3] == bad, (what, n, srows[n])
        if k == 0:
            assert np.isnan(srows[n, 1]) and srows[n, 2] == 0
        elif bad:
            assert np.isnan(srows[n, 1]) and np.isnan(srows[n, 2])
        else:
            rms = np.sqrt(np.mean(v ** 2))
            worst = max(worst, abs(srows[n, 1] - v.mean()) / rms, abs(np.sqrt(srows[n, 2] / k) - v.std()) / rms)
    print(f"{what}: worst |difference| / series RMS = {worst:.3g} (bound {TOL:g})")
    assert worst <= TOL, (what, worst)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 828, 4096])
def test_series_values_padding_and_moment_rows(CL, T, pad):
    x, rows, norm, cell, keep = series_case(CL, T)
    Tpad = T + pad
    xd, rd = dev(x), dev(rows)
    run = lambda idx: tuple(t.cpu().numpy() for t in CL.series(xd, rd, dev(cell[idx]), dev(keep[idx]), Tpad))     # noqa: E731
    everything = np.arange(300)
    out, srows = run(everything)
    check_series(T, Tpad, norm, cell, keep, out, srows, f"series T {T} Tpad {Tpad} N 300")
    # the twin's rows: counts exact, the same empty and NaN rows
    _, twin_rows = CL.series_host(x, rows, cell, keep, Tpad)
    assert np.array_equal(srows[:, [0, 3]], twin_rows[:, [0, 3]]) and np.array_equal(np.isnan(srows), np.isnan(twin_rows))
    # run twice: the same bits; N = 1 and N = 3, and the queries permuted: a query's bits do not depend on the batch
    again = run(everything)
    same = lambda a, b: np.array_equal(bits(a), bits(b))     # noqa: E731
    assert same(again[0], out) and same(again[1], srows)
    for idx in (np.array([3]), np.array([2, 6, 30])):
        o, s = run(idx)
        assert o.shape == (idx.size, Tpad) and same(o, out[idx]) and same(s, srows[idx]), idx
    perm = np.random.default_rng(T).permutation(300)
    o, s = run(perm)
    assert same(o, out[perm]) and same(s, srows[perm])


def test_series_refuses_bad_arguments_before_any_launch(CL):
    x, rows, _, cell, keep = series_case(CL, 36)
    xd, rd, cd, kd = dev(x), dev(rows), dev(cell), dev(keep)
    with pytest.raises(ValueError, match="Tpad 35 is shorter"):
        CL.series(xd, rd, cd, kd, 35)
    with pytest.raises(ValueError, match="cell must be a non-empty int32"):
        CL.series(xd, rd, cd.long(), kd)
    with pytest.raises(ValueError, match="keep must be a non-empty int32"):
        CL.series(xd, rd, cd, kd[:0])
    with pytest.raises(ValueError, match="300 cells for 299 lengths"):
        CL.series(xd, rd, cd, kd[:299])
    with pytest.raises(ValueError, match="rows must be a float64"):
        CL.series(xd, rd[:30], cd, kd)
    with pytest.raises(ValueError, match="at most 4096 months"):
        CL.series(torch.zeros((4097, 2), device="cuda"), torch.zeros((2, 4), dtype=torch.float64, device="cuda"), cd, kd)
    with pytest.raises(RuntimeError, match="tensor is on 'cpu'"):
        CL.series(torch.from_numpy(x), rd, cd, kd)


# --------------------------------------------------------------------------- #
# the fixture, end to end
# --------------------------------------------------------------------------- #
def test_process_on_the_device_writes_what_the_twins_write(CL, tmp_path):
    cpu = CL.process(FIX, str(tmp_path / "cpu"), BASELINE_YEARS, YEARS, "cpu")
    gpu = CL.process(FIX, str(tmp_path / "gpu"), BASELINE_YEARS, YEARS, "cuda")
    assert cpu["skipped"] is False and gpu["skipped"] is False
    with np.load(cpu["tas_norm"]) as a, np.load(gpu["tas_norm"]) as b:
        assert sorted(a.files) == sorted(b.files) == ["data", "lats", "lons", "start_year"]
        assert_same_bits(b["data"], a["data"], "tas_norm.npz data")
        assert int(np.isnan(a["data"]).sum()) == 2 * 36 + 1
        for k in ("lats", "lons", "start_year"):
            assert np.array_equal(a[k], b[k])
    want, got = json.load(open(cpu["baseline_metrics"])), json.load(open(gpu["baseline_metrics"]))
    assert list(got) == ["mean", "std"]
    for k in ("mean", "std"):
        assert_same_bits(np.array(got[k]), np.array(want[k]), f"baseline_metrics.json {k}")
    assert CL.process(FIX, str(tmp_path / "gpu"), BASELINE_YEARS, YEARS, "gpu")["skipped"] is True


def test_query_batch_against_six_query_calls(CL):
    from mau_amd.dataset_build import ArrayTemperatureQuery
    base, lats, lons = CL.read_years(FIX, *BASELINE_YEARS)
    raw, _, _ = CL.read_years(FIX, *YEARS, (lats, lons))
    rows = CL.baseline(dev(base))
    cq = CL.ClimateQuery(dev(raw), rows, lats, lons, YEARS[0])
    host = CL.ClimateQuery(raw, CL.baseline_host(base), lats, lons, YEARS[0])
    tq = ArrayTemperatureQuery(CL.normalise_host(raw, host.rows), lats, lons, YEARS[0])
    qs = recorded_queries()
    args = [[q[k] for q in qs] for k in ("lat", "lon", "year", "month")]
    out, lengths, srows = cq.query_batch(*args)
    assert out.is_cuda and srows.is_cuda and out.shape == (6, 36) and lengths.tolist() == [q["keep"] for q in qs]
    out = out.cpu().numpy()
    singles = []
    for n, q in enumerate(qs):
        one = cq.query(q["lat"], q["lon"], q["year"], q["month"])
        assert isinstance(one, list) and len(one) == q["keep"]
        assert_same_bits(np.array(one, dtype=np.float32), out[n, :q["keep"]], f"query {n}")
        assert_same_bits(np.array(one), np.array(tq.query(q["lat"], q["lon"], q["year"], q["month"]), dtype=np.float64), f"query {n} against the file's")
        assert not bits(out[n, q["keep"]:]).any()
        singles.append(one)
    assert srows.cpu().numpy()[:, 0].tolist() == [19, 36, 36, 13, 26, 1] and srows.cpu().numpy()[:, 3].tolist() == [0, 0, 0, 13, 1, 0]
    # the moments over the finite queries: dataset_build's temp_series_mean / temp_series_std
    pick = [0, 1, 2, 5]
    values = np.concatenate([np.array(singles[n]) for n in pick])
    mean, std = CL.series_moments(srows[pick])
    rms = np.sqrt(np.mean(values ** 2))
    assert abs(mean - values.mean()) <= TOL * rms and abs(std - values.std()) <= TOL * rms
    assert_same_bits(cq.rows.cpu().numpy(), host.rows, "the resident baseline")
