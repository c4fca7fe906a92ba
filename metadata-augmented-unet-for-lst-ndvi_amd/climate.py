"""Climate stage (the reference's ``src/data/process_temperature.py``): CRU monthly temperature -> per-grid-point baseline mean and
standard deviation over 1901-1950 -> the normalised anomalies ``(tas - mean) / std`` of 1951-2019 -> the nearest-grid-point series
cut at (year, month) that feeds the LSTM branch of every sample.  ``process`` writes the ``.npz`` that
``python -m mau_amd.dataset_build --temperature`` reads.

The grid is the reference's concatenation of the year files: ``x`` (T, G) float32, time-major, G = lat * lon.  Three launches
(``csrc/climate.hip``, include/mau_hip.h):

* ``baseline`` (``mau_climate_baseline``): per cell the fp64 row (n, mean, M2 = sum (x - mean)^2, NaN months) of its non-NaN months,
  two passes in time order;
* ``normalise`` (``mau_climate_normalise``): ``(float)(((double)x - mean) / sqrt(M2 / n))``, rounded once;
* ``series`` (``mau_climate_series``): the batched query -- per (cell, keep) the first ``keep`` anomalies of the cell straight from
  the RAW grid (the bits of ``normalise``), zero padding after them, and the moment row of the kept values.  ``ClimateQuery`` keeps
  the raw grid and its baseline on the device and answers ``query`` (the reference's ``TemperatureQuery.query``) and ``query_batch``.
* ``baseline_host`` / ``normalise_host`` / ``series_host`` are the float64 numpy twins: ``device="cpu"`` and the tests.

Departures from the reference, all three on purpose:

* the baseline is fp64 two-pass moments; the reference takes float32 ``nanmean`` / ``nanstd`` (through xarray);
* the anomaly is formed in float64 from the float64 coefficients and rounded once to float32; the reference does float32
  arithmetic on float32 coefficients (tests/golden/climatefix_deviation.json records the difference on the fixture);
* the outputs are one ``tas_norm.npz`` (``data, lats, lons, start_year``) and ``baseline_metrics.json``, not one netCDF file per year.

Year files carry the reference's stem, ``CRU_mean_temperature_mon_0.5x0.5_global_{year}_v4.03``: ``.npz`` (keys ``tas, lat, lon``) is
read natively; ``.nc`` goes through ``xarray``, imported lazily (that branch is exercised by no test: xarray is not a dependency of
the test suite).

    python -m mau_amd.climate --raw-dir R --output-dir O [--baseline-years 1901 1950] [--years 1951 2019] [--device gpu|cpu]
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

FILE_STEM = "CRU_mean_temperature_mon_0.5x0.5_global_{year}_v4.03"
YEAR_SUFFIXES = (".nc", ".npz")
ROW = 4                                                    # the row of mau_climate_baseline / mau_climate_series
R_N, R_MEAN, R_M2, R_BAD = range(ROW)                      # [3]: NaN months (baseline), non-finite values (series)
MAX_MONTHS = 4096                                          # mau_climate_series_max_months(): a series is one chunk
BASELINE_JSON, NORM_NPZ = "baseline_metrics.json", "tas_norm.npz"


# --------------------------------------------------------------------------- #
# year files
# --------------------------------------------------------------------------- #
def year_path(raw_dir: str, year: int) -> str:
    """The year's file in ``raw_dir`` (``.nc`` before ``.npz``); ``FileNotFoundError`` naming it when there is none."""
    stem = os.path.join(raw_dir, FILE_STEM.format(year=int(year)))
    for suffix in YEAR_SUFFIXES:
        if os.path.exists(stem + suffix):
            return stem + suffix
    raise FileNotFoundError(f"Temperature file not found: {stem}.nc (or .npz)")


def read_year(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One year file -> ``(tas (12, lat, lon) float32, lats, lons)``.  ``.npz`` holds ``tas, lat, lon``; ``.nc`` is opened with
    xarray as the reference does (imported here; no test exercises that branch: xarray is not a dependency of the test suite)."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            tas, lats, lons = z["tas"], z["lat"], z["lon"]
    else:
        import xarray as xr
        with xr.open_dataset(path) as ds:
            tas, lats, lons = ds["tas"].values, ds["lat"].values, ds["lon"].values
    tas = np.ascontiguousarray(tas, dtype=np.float32)
    lats, lons = np.asarray(lats), np.asarray(lons)
    if tas.ndim != 3 or tas.shape[1:] != (lats.size, lons.size):
        raise ValueError(f"{os.path.basename(path)}: tas {tas.shape} for {lats.size} lats and {lons.size} lons")
    return tas, lats, lons


def read_years(raw_dir: str, first: int, last: int, grid=None):
    """The years first..last concatenated along time: ``(x (T, lat, lon) float32, lats, lons)``.  ``grid``: the (lats, lons) every
    year must have (None: those of the first year read); another grid is a ``ValueError``."""
    parts = []
    for year in range(int(first), int(last) + 1):
        path = year_path(raw_dir, year)
        tas, lats, lons = read_year(path)
        if grid is None:
            grid = (lats, lons)
        if lats.shape != grid[0].shape or lons.shape != grid[1].shape or not (np.array_equal(lats, grid[0]) and np.array_equal(lons, grid[1])):
            raise ValueError(f"{os.path.basename(path)}: its grid ({lats.size} x {lons.size}) differs from the first year's "
                             f"({grid[0].size} x {grid[1].size})")
        parts.append(tas)
    return np.concatenate(parts, axis=0), grid[0], grid[1]


# --------------------------------------------------------------------------- #
# the numpy twins
# --------------------------------------------------------------------------- #
def _grid_host(x, what: str) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2 or x.size == 0:
        raise ValueError(f"{what}: x must be a non-empty float32 (T, G) or (T, lat, lon) array, got {x.shape} {x.dtype}")
    return x.reshape(x.shape[0], -1)


def _rows_host(rows, G: int, what: str) -> np.ndarray:
    rows = np.asarray(rows)
    if rows.dtype != np.float64 or rows.shape != (G, ROW):
        raise ValueError(f"{what}: rows must be float64 ({G}, {ROW}), got {rows.shape} {rows.dtype}")
    return rows


def baseline_host(x) -> np.ndarray:
    """float64 numpy twin of :func:`baseline`, operation for operation: x (T, G) float32 -> (G, 4) rows.  An explicit loop over
    time with the kernel's two passes (np.nanmean's summation order is numpy's business)."""
    x = _grid_host(x, "baseline_host")
    T, G = x.shape
    s, n = np.zeros(G), np.zeros(G)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            v = x[t].astype(np.float64)
            ok = ~np.isnan(v)
            s = np.where(ok, s + v, s)
            n = n + ok
        mean = s / n                                        # no month: 0 / 0 = NaN
        m2 = np.zeros(G)
        for t in range(T):
            v = x[t].astype(np.float64)
            ok = ~np.isnan(v)
            d = v - mean
            m2 = np.where(ok, m2 + d * d, m2)
    m2 = np.where(n == 0, np.nan, m2)
    return np.stack([n, mean, m2, T - n], axis=1)


def baseline_std(rows) -> np.ndarray:
    """sqrt(M2 / n) of baseline rows: the population standard deviation the anomalies divide by."""
    rows = np.asarray(rows, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(rows[..., R_M2] / rows[..., R_N])


def normalise_host(x, rows) -> np.ndarray:
    """float64 numpy twin of :func:`normalise`: ``((x - mean) / sqrt(M2 / n))`` in float64, rounded once to float32; the shape of x."""
    shape = np.asarray(x).shape
    x = _grid_host(x, "normalise_host")
    rows = _rows_host(rows, x.shape[1], "normalise_host")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return ((x.astype(np.float64) - rows[None, :, R_MEAN]) / baseline_std(rows)[None, :]).astype(np.float32).reshape(shape)


def _queries_host(cell, keep, what: str):
    cell, keep = np.asarray(cell), np.asarray(keep)
    if cell.ndim != 1 or cell.size == 0 or keep.shape != cell.shape or cell.dtype.kind not in "iu" or keep.dtype.kind not in "iu":
        raise ValueError(f"{what}: cell and keep must be non-empty integer (N,) arrays, got {cell.shape} {cell.dtype} and {keep.shape} {keep.dtype}")
    return cell.astype(np.int64), keep.astype(np.int64)


def series_host(x, rows, cell, keep, Tpad: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """numpy twin of :func:`series`: ``(series (N, Tpad) float32, srows (N, 4) float64)``.  The values are :func:`normalise_host`'s
    (bit for bit the kernel's); the moment rows use np.mean / np.sum instead of the kernel's fixed order: equal to it within the
    rounding of the sums, not bit for bit.  ``keep`` is clamped to [0, T]; a cell outside [0, G) gives NaN values and the empty row."""
    x = _grid_host(x, "series_host")
    T, G = x.shape
    rows = _rows_host(rows, G, "series_host")
    cell, keep = _queries_host(cell, keep, "series_host")
    Tpad = T if Tpad is None else int(Tpad)
    if T > MAX_MONTHS or Tpad < T:
        raise ValueError(f"series_host: T {T} must be at most {MAX_MONTHS} and Tpad {Tpad} at least T")
    out = np.zeros((cell.size, Tpad), dtype=np.float32)
    srows = np.zeros((cell.size, ROW), dtype=np.float64)
    for i, (c, k) in enumerate(zip(cell.tolist(), np.clip(keep, 0, T).tolist())):
        if not 0 <= c < G:
            out[i, :k] = np.nan
            srows[i] = [0.0, np.nan, 0.0, 0.0]
            continue
        v = normalise_host(x[:k, c:c + 1], rows[c:c + 1])[:, 0] if k else np.zeros(0, np.float32)
        out[i, :k] = v
        v = v.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            mean = v.mean() if k else np.nan
            srows[i] = [k, mean, np.sum((v - mean) ** 2) if k else 0.0, (~np.isfinite(v)).sum()]
    return out, srows


# --------------------------------------------------------------------------- #
# the kernels
# --------------------------------------------------------------------------- #
def _grid_dev(x, what: str):
    import torch
    from . import functional as F_
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}: x must be a torch tensor on the device, got {type(x).__name__}")
    F_._require_cuda(x, what)
    if x.dtype != torch.float32 or x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{what}: x must be a non-empty float32 (T, G) or (T, lat, lon) tensor, got {tuple(x.shape)} {x.dtype}")
    x = x.detach().contiguous()
    x2 = x.view(x.shape[0], -1)
    if x2.shape[1] > (1 << 30) or x2.shape[0] >= (1 << 31):
        raise ValueError(f"{what}: a grid of at most 2^30 cells and 2^31 - 1 months, got {tuple(x2.shape)}")
    return x2


def _rows_dev(rows, G: int, dev, what: str):
    import torch
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or tuple(rows.shape) != (G, ROW):
        got = f"{tuple(rows.shape)} {rows.dtype}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"{what}: rows must be a float64 ({G}, {ROW}) tensor, got {got}")
    if rows.device != dev:
        raise RuntimeError(f"{what}: all tensors must be on the same device")
    return rows.detach().contiguous()


def baseline(x):
    """x (T, G) or (T, lat, lon) fp32 on the device -> (G, 4) fp64 device rows (n, mean, M2, NaN months), one launch, no
    synchronisation.  A cell's row depends on its own column only; repeated calls agree bit for bit."""
    import torch
    from . import functional as F_
    from .functional import call
    x = _grid_dev(x, "baseline")
    T, G = x.shape
    rows = torch.empty((G, ROW), dtype=torch.float64, device=x.device)
    call("mau_climate_baseline", x.data_ptr(), rows.data_ptr(), T, G, F_._stream())
    return rows


def normalise(x, rows):
    """x fp32 and its (G, 4) baseline rows on the device -> the anomalies, fp32, the shape of x; one launch."""
    import torch
    from . import functional as F_
    from .functional import call
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else None
    x = _grid_dev(x, "normalise")
    T, G = x.shape
    rows = _rows_dev(rows, G, x.device, "normalise")
    out = torch.empty((T, G), dtype=torch.float32, device=x.device)
    call("mau_climate_normalise", x.data_ptr(), rows.data_ptr(), out.data_ptr(), T, G, F_._stream())
    return out.view(shape)


def series(x, rows, cell, keep, Tpad: Optional[int] = None):
    """The batched query: x the RAW grid, rows its baseline, ``cell`` and ``keep`` int32 (N,) device tensors ->
    ``(series (N, Tpad) fp32, srows (N, 4) fp64)`` on the device, one launch, no synchronisation, no host work per query.
    ``Tpad`` defaults to T.  Values outside their ranges are not refused here (that would need a read-back; ``ClimateQuery`` checks
    them before the upload): ``keep`` is clamped to [0, T], a cell outside [0, G) gives NaN values and the row (0, NaN, 0, 0)."""
    import torch
    from . import functional as F_
    from .functional import call
    x = _grid_dev(x, "series")
    T, G = x.shape
    rows = _rows_dev(rows, G, x.device, "series")
    for name, t in (("cell", cell), ("keep", keep)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() == 0:
            got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"series: {name} must be a non-empty int32 (N,) tensor, got {got}")
        if t.device != x.device:
            raise RuntimeError("series: all tensors must be on the same device")
    if cell.shape != keep.shape:
        raise ValueError(f"series: {cell.numel()} cells for {keep.numel()} lengths")
    Tpad = T if Tpad is None else int(Tpad)
    if T > MAX_MONTHS:
        raise ValueError(f"series: a grid of at most {MAX_MONTHS} months, got {T}")
    if Tpad < T:
        raise ValueError(f"series: Tpad {Tpad} is shorter than the {T} months of the grid")
    N = cell.numel()
    if N > (1 << 30):
        raise ValueError(f"series: at most 2^30 queries, got {N}")
    out = torch.empty((N, Tpad), dtype=torch.float32, device=x.device)
    srows = torch.empty((N, ROW), dtype=torch.float64, device=x.device)
    call("mau_climate_series", x.data_ptr(), rows.data_ptr(), cell.contiguous().data_ptr(), keep.contiguous().data_ptr(), out.data_ptr(),
         srows.data_ptr(), N, T, G, Tpad, F_._stream())
    return out, srows


# --------------------------------------------------------------------------- #
# queries
# --------------------------------------------------------------------------- #
def series_moments(srows) -> Tuple[float, float]:
    """(mean, sqrt(M2 / n)) over all kept values of all queries: the rows merged in query order with ``ground_truth.merge_moments``
    (an empty query is passed over) -- the ``temp_series_mean`` / ``temp_series_std`` of ``dataset_build.metrics_from_rows``."""
    from .ground_truth import merge_moments
    rows = srows if isinstance(srows, np.ndarray) else srows.cpu().numpy()
    acc = (0.0, 0.0, 0.0)
    for r in rows.reshape(-1, ROW):
        if r[R_N] > 0:
            acc = merge_moments(acc, (float(r[R_N]), float(r[R_MEAN]), float(r[R_M2])))
    if acc[0] == 0.0:
        return float("nan"), float("nan")
    return acc[1], math.sqrt(acc[2] / acc[0])


class ClimateQuery:
    """The reference's ``TemperatureQuery`` without a normalised grid in memory: ``raw`` (T, lat, lon) fp32 monthly values from
    January of ``start_year`` and ``rows`` (lat * lon, 4) their baseline (None: the baseline of ``raw`` itself), both device tensors
    (resident; every query is one launch) or both numpy arrays (the twins).  ``lats``, ``lons``: the grid."""

    def __init__(self, raw, rows, lats, lons, start_year: int):
        self.lats, self.lons = np.asarray(lats), np.asarray(lons)
        self.start_year = int(start_year)
        self.on_device = not isinstance(raw, np.ndarray)
        if len(raw.shape) != 3 or tuple(raw.shape[1:]) != (self.lats.size, self.lons.size):
            raise ValueError(f"ClimateQuery: raw {tuple(raw.shape)} for {self.lats.size} lats and {self.lons.size} lons")
        if self.on_device:
            self.raw = _grid_dev(raw, "ClimateQuery")
            self.rows = baseline(self.raw) if rows is None else _rows_dev(rows, self.raw.shape[1], self.raw.device, "ClimateQuery")
        else:
            self.raw = _grid_host(raw, "ClimateQuery")
            self.rows = baseline_host(self.raw) if rows is None else _rows_host(rows, self.raw.shape[1], "ClimateQuery")
        self.T, self.G = (int(v) for v in self.raw.shape)
        if self.T > MAX_MONTHS:
            raise ValueError(f"ClimateQuery: at most {MAX_MONTHS} months, got {self.T}")

    def indices(self, lats, lons, years, months) -> Tuple[np.ndarray, np.ndarray]:
        """(cell, keep) of the queries, on the host: the reference's nearest grid point (``np.abs(grid - v).argmin()``, the first
        minimum) and the months up to and including (year, month), clamped to [0, T]."""
        lats, lons = np.atleast_1d(np.asarray(lats, dtype=np.float64)), np.atleast_1d(np.asarray(lons, dtype=np.float64))
        years, months = np.atleast_1d(np.asarray(years)), np.atleast_1d(np.asarray(months))
        if not (lats.ndim == 1 and lats.size and lats.shape == lons.shape == years.shape == months.shape):
            raise ValueError(f"ClimateQuery: lats, lons, years and months must be non-empty and of one length, got {lats.shape}, "
                             f"{lons.shape}, {years.shape}, {months.shape}")
        cell = np.array([int(np.abs(self.lats - la).argmin()) * self.lons.size + int(np.abs(self.lons - lo).argmin())
                         for la, lo in zip(lats.tolist(), lons.tolist())], dtype=np.int64)
        keep = np.clip((years.astype(np.int64) - self.start_year) * 12 + months.astype(np.int64), 0, self.T)
        assert np.all((cell >= 0) & (cell < self.G))         # checked before the upload: the device cannot refuse them
        return cell.astype(np.int32), keep.astype(np.int32)

    def query_batch(self, lats, lons, years, months, Tpad: Optional[int] = None):
        """All queries in one launch: ``(series (N, Tpad) fp32, lengths (N,) numpy, srows (N, 4) fp64)``; series and srows are device
        tensors (numpy arrays over numpy data).  Row n holds ``lengths[n]`` values, then zeros."""
        cell, keep = self.indices(lats, lons, years, months)
        if not self.on_device:
            out, srows = series_host(self.raw, self.rows, cell, keep, Tpad)
            return out, keep.astype(np.int64), srows
        import torch
        both = torch.from_numpy(np.stack([cell, keep])).to(self.raw.device)
        out, srows = series(self.raw, self.rows, both[0], both[1], Tpad)
        return out, keep.astype(np.int64), srows

    def query(self, lat: float, lon: float, max_year: int, max_month: int) -> List[float]:
        """``ArrayTemperatureQuery.query`` over the normalised grid, value for value: the series of the nearest grid point up to and
        including (max_year, max_month)."""
        out, lengths, _ = self.query_batch([lat], [lon], [int(max_year)], [int(max_month)])
        row = out[0, :int(lengths[0])]
        return (row if isinstance(row, np.ndarray) else row.cpu().numpy()).tolist()


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def process(raw_dir: str, output_dir: str, baseline_years: Sequence[int] = (1901, 1950), years: Sequence[int] = (1951, 2019),
            device="cuda") -> dict:
    """The reference's ``process_temperature``: ``baseline_metrics.json`` (``mean`` and ``std`` per grid point as nested lists, NaN
    as Python's json writes it) and ``tas_norm.npz`` (``data (T, lat, lon), lats, lons, start_year``) in ``output_dir``.  Nothing is
    done when both exist.  ``device`` 'cpu' runs the numpy twins."""
    b0, b1 = (int(v) for v in baseline_years)
    y0, y1 = (int(v) for v in years)
    if b1 < b0 or y1 < y0:
        raise ValueError(f"climate: year ranges must be (first, last) with first <= last, got {(b0, b1)} and {(y0, y1)}")
    metrics_path, norm_path = os.path.join(output_dir, BASELINE_JSON), os.path.join(output_dir, NORM_NPZ)
    result = {"baseline_metrics": metrics_path, "tas_norm": norm_path}
    if os.path.exists(metrics_path) and os.path.exists(norm_path):
        print("Processed temperature files already exist. Skipping processing.")
        return {**result, "skipped": True}
    if not os.path.isdir(raw_dir):
        raise FileNotFoundError(f"Raw temperature directory not found at {raw_dir}")
    for year in list(range(b0, b1 + 1)) + list(range(y0, y1 + 1)):           # every file, before the device is touched
        year_path(raw_dir, year)
    dev = None
    if str(device).lower() != "cpu":
        import torch
        dev = torch.device("cuda:0" if str(device).lower() == "gpu" else device)
        if dev.type != "cuda":
            raise RuntimeError(f"climate: device {device!r}: 'cpu' (the numpy twins) or a 'cuda' (ROCm) device")
    os.makedirs(output_dir, exist_ok=True)

    print("Loading baseline years...")
    base, lats, lons = read_years(raw_dir, b0, b1)
    if dev is None:
        rows_dev = None
        rows = baseline_host(base)
    else:
        import torch
        rows_dev = baseline(torch.from_numpy(base).to(dev))
        rows = rows_dev.cpu().numpy()
    del base
    grid = (lats.size, lons.size)
    with open(metrics_path, "w") as f:
        json.dump({"mean": rows[:, R_MEAN].reshape(grid).tolist(), "std": baseline_std(rows).reshape(grid).tolist()}, f)
    print(f"Baseline metrics saved to {metrics_path}")

    raw, _, _ = read_years(raw_dir, y0, y1, (lats, lons))
    if dev is None:
        data = normalise_host(raw, rows)
    else:
        import torch
        data = normalise(torch.from_numpy(raw).to(dev), rows_dev).cpu().numpy()
    np.savez_compressed(norm_path, data=data, lats=lats, lons=lons, start_year=np.int64(y0))
    print(f"{data.shape[0]} months of {grid[0]} x {grid[1]} normalised anomalies saved to {norm_path}")
    return {**result, "skipped": False}


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.climate", description=__doc__.split("\n\n")[0])
    p.add_argument("--raw-dir", required=True, help="directory of " + FILE_STEM.format(year="<year>") + ".nc|.npz")
    p.add_argument("--output-dir", required=True, help="where baseline_metrics.json and tas_norm.npz are written")
    p.add_argument("--baseline-years", type=int, nargs=2, default=(1901, 1950), metavar=("FIRST", "LAST"))
    p.add_argument("--years", type=int, nargs=2, default=(1951, 2019), metavar=("FIRST", "LAST"))
    p.add_argument("--device", default="gpu", help="'gpu', a torch device name, or 'cpu' (the numpy twins)")
    a = p.parse_args(argv)
    try:
        process(a.raw_dir, a.output_dir, a.baseline_years, a.years, a.device)
    except (OSError, ValueError, KeyError, RuntimeError) as err:
        print(f"Error: {' '.join(str(err).split())}")
        return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
