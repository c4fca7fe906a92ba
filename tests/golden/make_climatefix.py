#!/usr/bin/env python3
"""Record the climate-stage fixture (tests/golden/climatefix, climatefix_deviation.json).  CPU only:

    python tests/golden/make_climatefix.py

The reference's ``src/data/process_temperature.py`` does its arithmetic through xarray, which is not available where this fixture is
made, so the reference program itself is NOT run.  What is recorded is its arithmetic written in numpy: float32 ``np.nanmean`` and
``np.nanstd(ddof=0)`` along time over the baseline years, then the float32 ``(tas - mean) / std`` of the output years.  That is what
xarray's ``mean(dim='time', skipna=True)`` / ``std(dim='time', skipna=True)`` dispatch to for a float32 variable when bottleneck is
not installed -- UNVERIFIED against xarray itself (parity unpinned, like the SSIM term of mau_amd/losses.py).  No reference source
is copied: fixtures are data.

Written: year files ``CRU_mean_temperature_mon_0.5x0.5_global_{year}_v4.03.npz`` (``tas (12, 6, 8) float32, lat, lon``) of 4 baseline
and 3 output years in degrees Celsius, ``expected_baseline.json`` (``mean``, ``std``), ``expected_tas_norm.npz`` (``data, lats, lons,
start_year``), ``queries.json`` (six recorded ``query`` results of the reference's ``TemperatureQuery`` over the expected grid) and,
next to the directory, ``climatefix_deviation.json``: per value the recorded arithmetic's own deviation from the float64 twin
(mau_amd.climate.baseline_host / normalise_host), 0 where both are NaN.  Every property the tests rely on is asserted here."""
import json
import os
import shutil
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIX = os.path.join(HERE, "climatefix")
STEM = "CRU_mean_temperature_mon_0.5x0.5_global_{year}_v4.03"
BASELINE_YEARS, YEARS = (1901, 1904), (1951, 1953)
LATS = np.array([-37.25, -12.25, 0.25, 23.75, 48.25, 61.75])
LONS = np.array([-120.25, -77.75, -46.25, -3.75, 10.75, 31.25, 77.25, 139.75])
OCEAN = [(0, 0), (3, 5)]                                     # NaN in every month of every year
PARTLY = (2, 2)                                              # NaN in some baseline months only
GAP = (4, 1)                                                 # NaN in one output month
QUERIES = [(-12.0464, -77.0428, 1952, 7),                    # cut mid-year
           (48.8566, 2.3522, 1953, 12),                      # the whole series
           (59.9139, 10.7522, 2021, 3),                      # past the last year: the whole series
           (-37.0, -121.0, 1952, 1),                         # an ocean cell: NaN
           (47.9, -77.7, 1953, 2),                           # the cell with a NaN output month
           (0.1, -46.0, 1951, 1)]                            # one month; NaN baseline months only


def year_grids():
    """year -> tas (12, 6, 8) float32: a climatology per cell (mean -20 .. 28 degrees, seasonal amplitude 0.4 .. 14), a slow
    warming and weather noise."""
    rng = np.random.default_rng(19010101)
    mean = 28.0 - 0.011 * LATS[:, None] ** 2 + rng.uniform(-2, 2, (LATS.size, LONS.size))
    amp = 0.4 + 0.22 * np.abs(LATS)[:, None] + rng.uniform(0, 0.5, (LATS.size, LONS.size))
    phase = np.where(LATS[:, None] < 0, np.pi, 0.0)
    out = {}
    for year in list(range(BASELINE_YEARS[0], BASELINE_YEARS[1] + 1)) + list(range(YEARS[0], YEARS[1] + 1)):
        m = np.arange(12)[:, None, None]
        tas = mean - amp * np.cos(2 * np.pi * (m - 0.5) / 12 + phase) + 0.008 * (year - 1901) + 0.6 * rng.standard_normal((12, LATS.size, LONS.size))
        tas = tas.astype(np.float32)
        for cell in OCEAN:
            tas[(slice(None),) + cell] = np.nan
        out[year] = tas
    out[1901][(slice(2, 5),) + PARTLY] = np.nan
    out[1903][(7,) + PARTLY] = np.nan
    out[1952][(9,) + GAP] = np.nan
    return out


def recorded_arithmetic(base, raw):
    """The reference's arithmetic in numpy (see the module docstring): float32 throughout."""
    assert base.dtype == raw.dtype == np.float32
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)     # all-NaN cells
        mean, std = np.nanmean(base, axis=0), np.nanstd(base, axis=0, ddof=0)
        norm = (raw - mean) / std
    assert mean.dtype == std.dtype == norm.dtype == np.float32
    return mean, std, norm


def deviation(recorded, twin):
    """|recorded - twin| in float64, 0 where both are NaN (their positions must agree)."""
    a, b = np.asarray(recorded, dtype=np.float64), np.asarray(twin, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.isfinite(a) | np.isnan(a))
    return np.where(np.isnan(a), 0.0, np.abs(a - b))


def scales(mean, std, norm):
    """What 1e-10 is relative to: |mean|; the RMS of the cell, hypot(std, mean); max(1, |anomaly|) (a normalised series has RMS 1).
    1 where the value is NaN."""
    f = lambda x: np.where(np.isnan(x), 1.0, x)                # noqa: E731
    return {"mean": f(np.abs(mean)), "std": f(np.hypot(std, mean)), "anomaly": f(np.maximum(1.0, np.abs(norm.astype(np.float64))))}


def main():
    sys.path.insert(0, ROOT)
    from mau_amd import climate as CL

    if os.path.isdir(FIX):
        shutil.rmtree(FIX)
    os.makedirs(FIX)
    grids = year_grids()
    for year, tas in grids.items():
        np.savez_compressed(os.path.join(FIX, STEM.format(year=year) + ".npz"), tas=tas, lat=LATS, lon=LONS)
    base = np.concatenate([grids[y] for y in range(BASELINE_YEARS[0], BASELINE_YEARS[1] + 1)])
    raw = np.concatenate([grids[y] for y in range(YEARS[0], YEARS[1] + 1)])
    assert base.shape == (48, 6, 8) and raw.shape == (36, 6, 8)

    mean, std, norm = recorded_arithmetic(base, raw)
    nan_cells = np.isnan(mean)
    assert sorted(zip(*np.nonzero(nan_cells))) == sorted(OCEAN) and np.array_equal(np.isnan(std), nan_cells)
    assert np.all(std[~nan_cells] > 0.2)                                             # no finite cell with zero variance
    assert np.sum(np.abs(mean[~nan_cells]) > 20 * std[~nan_cells]) >= 6              # |mean| >> std in some cells
    assert np.isnan(base[(slice(None),) + PARTLY]).sum() == 4 and not np.isnan(raw[(slice(None),) + PARTLY]).any()
    assert np.isnan(norm).sum() == 2 * 36 + 1 and np.isnan(norm[(21,) + GAP])

    with open(os.path.join(FIX, "expected_baseline.json"), "w") as f:
        json.dump({"mean": mean.tolist(), "std": std.tolist()}, f)                   # NaN as Python's json writes it, as the reference
    np.savez_compressed(os.path.join(FIX, "expected_tas_norm.npz"), data=norm, lats=LATS, lons=LONS, start_year=np.int64(YEARS[0]))

    # the six queries, by the reference's TemperatureQuery.query over the expected grid: nearest grid point (first minimum), the
    # months up to and including (year, month)
    stamps = [(y, m) for y in range(YEARS[0], YEARS[1] + 1) for m in range(1, 13)]
    queries = []
    for lat, lon, year, month in QUERIES:
        i, j = int(np.abs(LATS - lat).argmin()), int(np.abs(LONS - lon).argmin())
        keep = sum(1 for (y, m) in stamps if not (y > year or (y == year and m > month)))
        queries.append({"lat": lat, "lon": lon, "year": year, "month": month, "lat_index": i, "lon_index": j, "keep": keep,
                        "series": norm[:keep, i, j].tolist()})
    assert [q["keep"] for q in queries] == [19, 36, 36, 13, 26, 1]
    assert (queries[3]["lat_index"], queries[3]["lon_index"]) == OCEAN[0] and (queries[4]["lat_index"], queries[4]["lon_index"]) == GAP
    assert (queries[5]["lat_index"], queries[5]["lon_index"]) == PARTLY
    assert all(np.isnan(v) for v in queries[3]["series"]) and sum(np.isnan(v) for v in queries[4]["series"]) == 1
    with open(os.path.join(FIX, "queries.json"), "w") as f:
        json.dump(queries, f, indent=1)

    # the float64 twin and the recorded arithmetic's deviation from it
    rows = CL.baseline_host(base)
    twin_mean, twin_std = rows[:, CL.R_MEAN].reshape(mean.shape), CL.baseline_std(rows).reshape(mean.shape)
    twin_norm = CL.normalise_host(raw, rows)
    dev = {"mean": deviation(mean, twin_mean), "std": deviation(std, twin_std), "anomaly": deviation(norm, twin_norm)}
    scale = scales(twin_mean, twin_std, twin_norm)
    with open(os.path.join(HERE, "climatefix_deviation.json"), "w") as f:
        json.dump({"source": "float32 np.nanmean / np.nanstd(ddof=0) and float32 (tas - mean) / std (what xarray dispatches to without "
                             "bottleneck; unverified against xarray itself) versus the float64 twin",
                   "dev": {k: v.tolist() for k, v in dev.items()}, "scale": {k: v.tolist() for k, v in scale.items()}}, f)
    size = sum(os.path.getsize(os.path.join(FIX, f)) for f in os.listdir(FIX))
    print(f"climatefix: {len(grids)} year files, {size / 1024:.1f} KiB; deviation of the mean {dev['mean'].max():.3g}, of the std "
          f"{dev['std'].max():.3g}, of the anomalies {dev['anomaly'].max():.3g}")


if __name__ == "__main__":
    main()
