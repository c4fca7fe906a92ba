"""Dataset build (the reference's ``src/data/processing_10m/process.py process_future_data``): raw tiles -> (t1, t2) samples ->
train / val / test -> samples with negligible change filtered out -> normalisation statistics over the kept training samples ->
``normalization_metrics.json`` and the normalised ``.npz`` tiles every other tool of the package reads.

The reference reads each raster two or three times and does its pixel arithmetic in numpy.  Here

* ``raw_tile_process`` is ONE launch (``mau_raw_tile_process``) per batch of raw samples, every byte read once: per sample an fp64
  row with what the filter needs (per-class changed-pixel counts, out-of-range class counts, sum |ndvi_t2 - ndvi_t1|,
  sum |temp_t2 - temp_t1|) and what the statistics need (two-pass moment rows of r / 255, g / 255, b / 255 and temp_t1), and / or
  the normalised planes in the compact layout (``cont`` (B,5,H,W), ``targets`` (B,2,H,W));
* ``build`` makes one pass of rows over the train split (rows stay on the device, one read-back), decides keep / drop on the host
  with the reference's comparison, merges the kept samples' moment rows in sample order (``ground_truth.merge_moments``) and writes
  the metrics file; then one pass per split filters and normalises in one launch per batch and writes the tiles;
* ``raw_rows_host`` / ``normalise_host`` are the numpy twins (float64 / the dtypes numpy itself uses): ``--device cpu`` and the tests.

Raster dtypes.  The kernel's arithmetic is numpy's for uint8 RGB (``rgb / 255.0`` is float64 there, cast to float32 at the end) and
float32 NDVI / temperature rasters (a float32 array combined with Python floats stays float32): with such rasters the tiles are the
reference's bit for bit.  Of the reference's own cached rasters (``app/cache/*.tif``) the class map and RGB are uint8 and NDVI is
float32, but the temperature raster is FLOAT64: the reader here converts every plane to float32 on read, so for float64 temperature
rasters the normalised temperature agrees with the reference's to float32 rounding, not bit for bit.

Departures from the reference, both stated in the log: a sample with a non-finite pixel in a plane the row covers is dropped (the
reference would write NaN into the metrics file and every tile), and the statistics are two-pass moments in float64 (the reference
takes sum x^2 / n - mean^2, for the temperature with float32 sums).

``.npy`` rasters with the reference's file stems are read natively; ``.tif`` goes through ``rasterio``, imported lazily, with the
reference's resampling arguments (that branch is exercised by no test: rasterio is not a dependency of the test suite).

    python -m mau_amd.dataset_build --raw-dir R --processed-dir P --temperature series.npz [--cities-csv C] [--device gpu|cpu]
                                    [--batch-size 64] [--holdout-ratio 0.01] [--seed 0]
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import random
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

NUM_CLASSES, N_CONT, N_TGT = 9, 5, 2
NDVI_CHANGE_THRESHOLD = 0.1
TEMP_CHANGE_THRESHOLD = 0.1
DW_CHANGE_THRESHOLD = 0.1                                  # largest proportion of pixels changed in any single class
METRIC_KEYS = ["rgb_mean", "rgb_std", "temp_mean", "temp_std", "meta_mean", "meta_std", "temp_series_mean", "temp_series_std"]
REQUIRED_T1, REQUIRED_T2 = ("dw", "rgb", "ndvi", "temp"), ("ndvi", "temp", "dw")
RASTER_SUFFIXES = (".tif", ".npy")

# the row of mau_raw_tile_process (include/mau_hip.h)
MAX_CLASSES = 16
OOR = MAX_CLASSES                                          # [16], [17]: class values >= num_classes of dw_t1, dw_t2
NDVI_L1, NDVI_BAD, TEMP_L1, TEMP_BAD = OOR + 2, OOR + 3, OOR + 4, OOR + 5
MOM0 = OOR + 6                                             # four moment rows (n, mean, M2, non-finite): r/255, g/255, b/255, temp_t1
M_N, M_MEAN, M_M2, M_BAD = range(4)
N_MOM = 4
ROW = MOM0 + 4 * N_MOM
NORM = 8                                                   # rgb_mean[3], rgb_std[3], temp_mean, temp_std


# --------------------------------------------------------------------------- #
# file names, samples, splits
# --------------------------------------------------------------------------- #
def parse_filename(filename: str) -> Optional[dict]:
    """``<city>_<id>_<lat>_<lon>_<offx>_<offy>_<year>_<month>_<type>.<ext>`` -> its fields (the city may itself hold underscores),
    ``None`` for a name that does not follow the convention."""
    parts = os.path.basename(filename).split("_")
    try:
        return {"city_name": "_".join(parts[:-8]), "city_id": int(parts[-8]), "lat": float(parts[-7]), "lon": float(parts[-6]),
                "offset_x": float(parts[-5]), "offset_y": float(parts[-4]), "year": int(parts[-3]), "month": int(parts[-2]),
                "type": parts[-1].split(".")[0], "filepath": filename}
    except (IndexError, ValueError):
        return None


def group_files(image_dir: str) -> Dict[tuple, dict]:
    """(city_id, lat, lon) -> {city_name, ..., timestamps: {(year, month): {type: path}}} over the rasters of ``image_dir`` in sorted
    order (the reference walks ``os.listdir`` as it comes)."""
    locations: Dict[tuple, dict] = {}
    for filename in sorted(os.listdir(image_dir)):
        if not filename.endswith(RASTER_SUFFIXES):
            continue
        md = parse_filename(filename)
        if md is None:
            print(f"Could not parse filename: {filename}")
            continue
        loc = locations.setdefault((md["city_id"], md["lat"], md["lon"]),
                                   {"lat": md["lat"], "lon": md["lon"], "city_id": md["city_id"], "city_name": md["city_name"], "timestamps": {}})
        loc["timestamps"].setdefault((md["year"], md["month"]), {})[md["type"]] = os.path.join(image_dir, filename)
    return locations


def read_population(cities_csv: Optional[str]) -> Dict[int, float]:
    """``id`` -> ``population`` of the cities CSV (empty without one)."""
    if not cities_csv:
        return {}
    with open(cities_csv, newline="") as f:
        return {int(float(r["id"])): float(r["population"]) for r in csv.DictReader(f) if r.get("population") not in (None, "")}


def list_samples(raw_dir: str, cities_csv: Optional[str] = None) -> List[dict]:
    """Every pair t1 < t2 of a location that has ``dw, rgb, ndvi, temp`` at t1 and ``ndvi, temp, dw`` at t2, as the reference's sample
    dictionaries (population 0 for a city the CSV does not list)."""
    population = read_population(cities_csv)
    samples = []
    for (city_id, lat, lon), loc in group_files(raw_dir).items():
        stamps = sorted(loc["timestamps"])
        for i, t1 in enumerate(stamps):
            for t2 in stamps[i + 1:]:
                f1, f2 = loc["timestamps"][t1], loc["timestamps"][t2]
                if not (all(k in f1 for k in REQUIRED_T1) and all(k in f2 for k in REQUIRED_T2)):
                    continue
                samples.append({"city_id": city_id, "lat": lat, "lon": lon, "city_name": loc["city_name"],
                                "population": population.get(city_id, 0), "t1_year": t1[0], "t1_month": t1[1], "t2_year": t2[0],
                                "t2_month": t2[1], "delta_time_years": (t2[0] - t1[0]) + (t2[1] - t1[1]) / 12.0,
                                "files": {**f1, "ndvi_t2": f2["ndvi"], "temp_t2": f2["temp"], "dw_t2": f2["dw"]}})
    return samples


def split_samples(samples: Sequence[dict], holdout_ratio: float = 0.01, rng: Optional[random.Random] = None):
    """(train, val, test): ``int(cities * holdout_ratio)`` cities drawn by a shuffle of the sorted city ids go to test whole; of the
    rest t2_year 2025 -> test, 2024 -> val, <= 2023 -> train, anything else is dropped.  The reference shuffles with the unseeded
    global generator; here the generator is explicit (``random.Random(0)`` by default)."""
    rng = rng if rng is not None else random.Random(0)
    cities = sorted(set(s["city_id"] for s in samples))
    rng.shuffle(cities)
    holdout = set(cities[:int(len(cities) * holdout_ratio)])
    train, val, test = [], [], []
    for s in samples:
        if s["city_id"] in holdout or s["t2_year"] == 2025:
            test.append(s)
        elif s["t2_year"] == 2024:
            val.append(s)
        elif s["t2_year"] <= 2023:
            train.append(s)
    return train, val, test


def output_filename(s: Mapping) -> str:
    return (f"{s['city_name']}_{s['city_id']}_{s['lat']:.4f}_{s['lon']:.4f}_{s['t1_year']}_{s['t1_month']:02d}_to_"
            f"{s['t2_year']}_{s['t2_month']:02d}.npz")


# --------------------------------------------------------------------------- #
# rasters and the temperature series
# --------------------------------------------------------------------------- #
def read_raster(path: str, target_shape: Tuple[int, int], kind: str) -> np.ndarray:
    """One raster at ``target_shape``: ``kind`` 'plane' -> (H,W) float32, 'rgb' -> (3,H,W) float32 (raw 0..255), 'classes' -> (H,W)
    uint8 (a value outside [0,255] becomes 255: out of range for any layout).  ``.npy`` must have the target shape already;
    ``.tif`` is resampled by rasterio as the reference does (bilinear, nearest for the class map)."""
    want = ((3,) if kind == "rgb" else ()) + tuple(target_shape)
    if path.endswith(".npy"):
        data = np.load(path)
        if data.shape != want:
            raise ValueError(f"{os.path.basename(path)}: shape {data.shape}, expected {want}")
    else:
        import rasterio
        from rasterio.warp import Resampling
        with rasterio.open(path) as src:
            data = src.read([1, 2, 3] if kind == "rgb" else 1, out_shape=want,
                            resampling=Resampling.nearest if kind == "classes" else Resampling.bilinear)
    if kind != "classes":
        return np.ascontiguousarray(data, dtype=np.float32)
    if data.dtype == np.uint8:
        return np.ascontiguousarray(data)
    with np.errstate(invalid="ignore"):
        return np.where((data >= 0) & (data <= 255), data, 255).astype(np.uint8)


def raster_shape(path: str) -> Tuple[int, int]:
    if path.endswith(".npy"):
        return tuple(np.load(path, mmap_mode="r").shape[-2:])
    import rasterio
    with rasterio.open(path) as src:
        return (src.height, src.width)


RAW_KEYS = ("dw_t1", "dw_t2", "rgb", "ndvi_t1", "ndvi_t2", "temp_t1", "temp_t2")


def read_sample(sample: Mapping, target_shape: Tuple[int, int]) -> Dict[str, np.ndarray]:
    """The seven rasters of a sample, each read once."""
    f = sample["files"]
    return {"dw_t1": read_raster(f["dw"], target_shape, "classes"), "dw_t2": read_raster(f["dw_t2"], target_shape, "classes"),
            "rgb": read_raster(f["rgb"], target_shape, "rgb"), "ndvi_t1": read_raster(f["ndvi"], target_shape, "plane"),
            "ndvi_t2": read_raster(f["ndvi_t2"], target_shape, "plane"), "temp_t1": read_raster(f["temp"], target_shape, "plane"),
            "temp_t2": read_raster(f["temp_t2"], target_shape, "plane")}


class ArrayTemperatureQuery:
    """The reference's ``TemperatureQuery`` over arrays: ``data`` (T, lat, lon) monthly values from January of ``start_year``,
    ``lats``, ``lons`` the grid.  ``query`` returns the series of the nearest grid point up to and including (year, month)."""

    def __init__(self, data, lats, lons, start_year: int):
        self.data, self.lats, self.lons = np.asarray(data), np.asarray(lats), np.asarray(lons)
        if self.data.ndim != 3 or self.data.shape[1:] != (self.lats.size, self.lons.size):
            raise ValueError(f"ArrayTemperatureQuery: data {self.data.shape} for {self.lats.size} lats and {self.lons.size} lons")
        self.start_year = int(start_year)

    @classmethod
    def from_npz(cls, path: str) -> "ArrayTemperatureQuery":
        with np.load(path) as z:
            return cls(z["data"], z["lats"], z["lons"], int(z["start_year"]))

    def query(self, lat: float, lon: float, max_year: int, max_month: int) -> List[float]:
        ts = self.data[:, np.abs(self.lats - lat).argmin(), np.abs(self.lons - lon).argmin()]
        keep = (int(max_year) - self.start_year) * 12 + int(max_month)          # months up to and including (max_year, max_month)
        return ts[:max(0, keep)].tolist()


# --------------------------------------------------------------------------- #
# the numpy twins
# --------------------------------------------------------------------------- #
def raw_rows_host(dw_t1, dw_t2, rgb, ndvi_t1, ndvi_t2, temp_t1, temp_t2, num_classes: int = NUM_CLASSES) -> np.ndarray:
    """float64 numpy twin of the rows of :func:`raw_tile_process`: (B,H,W) uint8 x 2, (B,3,H,W), (B,H,W) x 4 -> (B, ROW).  np.mean /
    np.sum instead of the kernel's chunked order: equal to it within the rounding of the sums, not bit for bit."""
    a, b = np.asarray(dw_t1), np.asarray(dw_t2)
    f64 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)          # noqa: E731
    rgb, n1, n2, t1, t2 = f64(rgb), f64(ndvi_t1), f64(ndvi_t2), f64(temp_t1), f64(temp_t2)
    B = a.shape[0]
    rows = np.zeros((B, ROW), dtype=np.float64)
    for i in range(B):
        for c in range(num_classes):
            rows[i, c] = int(((a[i] == c) != (b[i] == c)).sum())
        rows[i, OOR], rows[i, OOR + 1] = int((a[i] >= num_classes).sum()), int((b[i] >= num_classes).sum())
        with np.errstate(invalid="ignore", over="ignore"):
            for at, d in ((NDVI_L1, n2[i] - n1[i]), (TEMP_L1, t2[i] - t1[i])):
                rows[i, at], rows[i, at + 1] = np.abs(d).sum(), (~np.isfinite(d)).sum()
            for p, v in enumerate([rgb[i, 0] / 255.0, rgb[i, 1] / 255.0, rgb[i, 2] / 255.0, t1[i]]):
                mean = v.mean()
                rows[i, MOM0 + 4 * p:MOM0 + 4 * p + 4] = [v.size, mean, np.sum((v - mean) ** 2), (~np.isfinite(v)).sum()]
    return rows


def normalise_host(rgb, ndvi_t1, ndvi_t2, temp_t1, temp_t2, norm) -> Tuple[np.ndarray, np.ndarray]:
    """numpy twin of the planes of :func:`raw_tile_process`, in the dtypes numpy uses for uint8 RGB and float32 planes: cont (B,5,H,W),
    targets (B,2,H,W) float32.  ``norm``: rgb_mean[3], rgb_std[3], temp_mean, temp_std."""
    norm = np.asarray(norm, dtype=np.float64).reshape(NORM)
    rgb = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    n1, n2, t1, t2 = (np.asarray(x, dtype=np.float32) for x in (ndvi_t1, ndvi_t2, temp_t1, temp_t2))
    mean32, std32 = np.float32(norm[6]), np.float32(norm[7])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = ((rgb / 255.0 - norm[0:3][None, :, None, None]) / norm[3:6][None, :, None, None]).astype(np.float32)
        cont = np.concatenate([c, n1[:, None], ((t1 - mean32) / std32)[:, None]], axis=1)
        targets = np.stack([n2, (t2 - mean32) / std32], axis=1)
    assert cont.dtype == np.float32 and targets.dtype == np.float32
    return cont, targets


# --------------------------------------------------------------------------- #
# the kernel
# --------------------------------------------------------------------------- #
def raw_tile_process(dw_t1, dw_t2, rgb, ndvi_t1, ndvi_t2, temp_t1, temp_t2, norm=None, rows: bool = True, planes: bool = False):
    """(B,H,W) uint8 x 2, (B,3,H,W) fp32, (B,H,W) fp32 x 4 on the device -> ``(rows, cont, targets)``: the (B, ROW) fp64 rows of
    ``mau_raw_tile_process`` (include/mau_hip.h) when ``rows``, the normalised (B,5,H,W) / (B,2,H,W) fp32 planes when ``planes`` (they
    need ``norm``: 8 values, or an fp64 device tensor of 8), ``None`` for what was not asked for.  One launch per 64 samples, no
    synchronisation.  A sample's results depend on its own bytes only: not on B, not on its position, not on what else was asked
    for; repeated calls agree bit for bit."""
    import torch
    from . import functional as F_
    from .functional import call, lib
    what = "raw_tile_process"
    a = F_._device_planes(dw_t1, what, "dw_t1", torch.uint8, 3, "(B, H, W)")
    b = F_._device_planes(dw_t2, what, "dw_t2", torch.uint8, 3, "(B, H, W)")
    c = F_._device_planes(rgb, what, "rgb", torch.float32, 4, "(B, 3, H, W)")
    pl = [F_._device_planes(t, what, name, torch.float32, 3, "(B, H, W)")
          for t, name in ((ndvi_t1, "ndvi_t1"), (ndvi_t2, "ndvi_t2"), (temp_t1, "temp_t1"), (temp_t2, "temp_t2"))]
    B, H, W = a.shape
    if b.shape != a.shape or c.shape != (B, 3, H, W) or any(t.shape != a.shape for t in pl):
        raise ValueError(f"{what}: dw_t1 {tuple(a.shape)}, dw_t2 {tuple(b.shape)}, rgb {tuple(c.shape)}, planes "
                         f"{[tuple(t.shape) for t in pl]}: expected (B,H,W) x 2, (B,3,H,W), (B,H,W) x 4")
    dev = a.device
    if any(t.device != dev for t in [b, c] + pl):
        raise RuntimeError(f"{what}: all tensors must be on the same device")
    if not rows and not planes:
        raise ValueError(f"{what}: nothing asked for (rows and planes are both false)")
    nrm = None
    if planes:
        if norm is None:
            raise ValueError(f"{what}: the normalised planes need norm (rgb_mean[3], rgb_std[3], temp_mean, temp_std)")
        nrm = norm if isinstance(norm, torch.Tensor) else torch.tensor([float(x) for x in norm], dtype=torch.float64)
        if nrm.dtype != torch.float64 or nrm.numel() != NORM:
            raise ValueError(f"{what}: norm must be {NORM} float64 values, got {tuple(nrm.shape)} {nrm.dtype}")
        nrm = nrm.to(dev).contiguous()
    out_rows = torch.empty((B, ROW), dtype=torch.float64, device=dev) if rows else None
    ws = torch.empty(lib.mau_raw_tile_ws_elems(B, H * W), dtype=torch.float64, device=dev) if rows else None
    cont = torch.empty((B, N_CONT, H, W), dtype=torch.float32, device=dev) if planes else None
    tgt = torch.empty((B, N_TGT, H, W), dtype=torch.float32, device=dev) if planes else None
    ptr = lambda t: t.data_ptr() if t is not None else None                      # noqa: E731
    call("mau_raw_tile_process", a.data_ptr(), b.data_ptr(), c.data_ptr(), *(t.data_ptr() for t in pl), ptr(nrm), ptr(out_rows),
         ptr(cont), ptr(tgt), ptr(ws), F_._tickets(dev).data_ptr() if rows else None, B, H * W, NUM_CLASSES, F_._stream())
    return out_rows, cont, tgt


# --------------------------------------------------------------------------- #
# rows -> decisions and statistics (host)
# --------------------------------------------------------------------------- #
def filter_values(row: np.ndarray, num_classes: int = NUM_CLASSES) -> Tuple[float, float, float]:
    """(ndvi_diff, temp_diff, dw_diff) of the reference's filter check from a row: mean |ndvi_t2 - ndvi_t1|, mean |temp_t2 - temp_t1|,
    the largest per-class proportion of changed pixels."""
    n = row[MOM0 + M_N]
    return float(row[NDVI_L1] / n), float(row[TEMP_L1] / n), float(np.max(row[:num_classes]) / n)


def row_decision(row: np.ndarray) -> Tuple[bool, Optional[str]]:
    """(keep, message): ``message`` is set when the sample fails (an out-of-range class, as ``np.eye(9)[img]`` raises in the
    reference) or is dropped for a non-finite pixel; a sample with negligible change is dropped as in the reference: iff all three
    of ndvi_diff, temp_diff and dw_diff are below their thresholds."""
    oor = int(row[OOR] + row[OOR + 1])
    if oor:
        return False, f"{oor} class values outside [0, {NUM_CLASSES})"
    bad = int(row[NDVI_BAD] + row[TEMP_BAD] + sum(row[MOM0 + 4 * p + M_BAD] for p in range(N_MOM)))
    if bad:
        return False, f"{bad} non-finite values (the reference would carry NaN into the metrics file and every tile)"
    ndvi_diff, temp_diff, dw_diff = filter_values(row)
    if ndvi_diff < NDVI_CHANGE_THRESHOLD and temp_diff < TEMP_CHANGE_THRESHOLD and dw_diff < DW_CHANGE_THRESHOLD:
        return False, None
    return True, None


def metrics_from_rows(rows: Sequence[np.ndarray], samples: Sequence[Mapping], temp_query) -> dict:
    """The reference's metrics dictionary from the rows of the KEPT training samples: their moment rows merged in sample order
    (std = sqrt(M2 / n)), np.mean / np.std of the metadata, mean / std of all values of all temperature series."""
    from .ground_truth import merge_moments
    if not len(rows):
        raise ValueError("dataset_build: no training sample was kept: there is nothing to take normalisation statistics from")
    acc = [(0.0, 0.0, 0.0)] * N_MOM
    for r in rows:
        for p in range(N_MOM):
            m = r[MOM0 + 4 * p:MOM0 + 4 * p + 3]
            acc[p] = merge_moments(acc[p], (float(m[0]), float(m[1]), float(m[2])))
    mean = [m[1] for m in acc]
    std = [math.sqrt(m[2] / m[0]) for m in acc]
    meta = np.array([[s["lat"], s["lon"], s["population"], s["delta_time_years"]] for s in samples], dtype=np.float64)
    series = np.concatenate([np.asarray(temp_query.query(s["lat"], s["lon"], int(s["t1_year"]), int(s["t1_month"])), dtype=np.float64)
                             for s in samples])
    return {"rgb_mean": mean[:3], "rgb_std": std[:3], "temp_mean": mean[3], "temp_std": std[3],
            "meta_mean": np.mean(meta, axis=0).tolist(), "meta_std": np.std(meta, axis=0).tolist(),
            "temp_series_mean": float(np.mean(series)), "temp_series_std": float(np.std(series))}


def norm_of(metrics: Mapping) -> List[float]:
    return [float(x) for x in metrics["rgb_mean"]] + [float(x) for x in metrics["rgb_std"]] + [float(metrics["temp_mean"]),
                                                                                               float(metrics["temp_std"])]


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def _name(s: Mapping) -> str:
    return f"{s.get('city_name')}_{s.get('city_id')}"


def _batches(samples, target_shape, batch_size, what):
    """(samples, stacked rasters) per batch; a sample whose rasters cannot be read is logged and skipped."""
    for i in range(0, len(samples), batch_size):
        got, raws = [], []
        for s in samples[i:i + batch_size]:
            try:
                raws.append(read_sample(s, target_shape))
                got.append(s)
            except Exception as e:
                print(f"Failed during {what} for sample {_name(s)}: {e}. Skipping.")
        if got:
            yield got, {k: np.stack([r[k] for r in raws]) for k in RAW_KEYS}


def _run(raw, device, norm, rows, planes):
    """One batch through the kernel (device tensors back) or through the twins (numpy back)."""
    if device is None:
        r = raw_rows_host(*(raw[k] for k in RAW_KEYS)) if rows else None
        c, t = normalise_host(*(raw[k] for k in RAW_KEYS[2:]), norm) if planes else (None, None)
        return r, c, t
    import torch
    dev = [torch.from_numpy(raw[k]).to(device, non_blocking=False) for k in RAW_KEYS]
    return raw_tile_process(*dev, norm=norm, rows=rows, planes=planes)


def _host(t):
    return t if t is None or isinstance(t, np.ndarray) else t.cpu().numpy()


def _decide(samples, rows, subset):
    """The kept (sample, row) pairs of a subset, logging what the reference logs."""
    kept, filtered = [], 0
    for s, r in zip(samples, rows):
        keep, message = row_decision(r)
        if message is not None:
            print(f"Failed during filtering for sample {_name(s)}: {message}. Skipping.")
        elif not keep:
            nd, td, dd = filter_values(r)
            print(f"Filtering out sample {output_filename(s)} due to negligible changes: NDVI diff={nd}, Temp diff={td}, DW diff={dd}")
            filtered += 1
        else:
            kept.append((s, r))
    print(f"Filtered out {filtered} of {len(samples)} samples for {subset}.")
    return kept


def _save(sample, raw, i, cont, targets, metrics, temp_query, path):
    """One tile in the reference's four keys (process.py:182-187)."""
    from .data import expand_input
    inp = expand_input(raw["dw_t1"][i], raw["dw_t2"][i], cont[i], NUM_CLASSES)
    meta = (np.array([sample["lat"], sample["lon"], sample["population"], sample["delta_time_years"]]) - metrics["meta_mean"]) / metrics["meta_std"]
    series = (np.array(temp_query.query(sample["lat"], sample["lon"], int(sample["t1_year"]), int(sample["t1_month"])))
              - metrics["temp_series_mean"]) / metrics["temp_series_std"]
    np.savez_compressed(path, input=inp.astype(np.float32), target=targets[i].astype(np.float32), metadata=meta.astype(np.float32),
                        temperature_serie=series.astype(np.float32))


def build(raw_dir: str, processed_dir: str, temp_query, cities_csv: Optional[str] = None, device="cuda", batch_size: int = 64,
          holdout_ratio: float = 0.01, seed: int = 0, target_shape: Optional[Tuple[int, int]] = None) -> dict:
    """The whole stage.  ``temp_query``: anything with ``.query(lat, lon, year, month)`` (:class:`ArrayTemperatureQuery`).  ``device``
    'cpu' runs the numpy twins.  Returns ``{"metrics": ..., "kept": {split: [file names]}, "written": {split: [file names]}}``."""
    if batch_size <= 0:
        raise ValueError(f"dataset_build: batch size must be positive, got {batch_size}")
    if not os.path.isdir(raw_dir):
        raise FileNotFoundError(f"Raw tile directory not found at {raw_dir}")
    dev = None
    if str(device).lower() != "cpu":
        import torch
        dev = torch.device("cuda:0" if str(device).lower() == "gpu" else device)
        if dev.type != "cuda":
            raise RuntimeError(f"dataset_build: device {device!r}: 'cpu' (the numpy twins) or a 'cuda' (ROCm) device")
    samples = list_samples(raw_dir, cities_csv)
    if not samples:
        raise FileNotFoundError(f"No (t1, t2) samples found in {raw_dir}")
    if target_shape is None:
        target_shape = raster_shape(samples[0]["files"]["ndvi"])
    train, val, test = split_samples(samples, holdout_ratio, random.Random(seed))
    print(f"Train samples: {len(train)}\nValidation samples: {len(val)}\nTest samples: {len(test)}")
    os.makedirs(processed_dir, exist_ok=True)
    metrics_path = os.path.join(processed_dir, "normalization_metrics.json")
    kept: Dict[str, List[dict]] = {}

    if os.path.exists(metrics_path):
        print(f"Loading existing normalization metrics from {metrics_path}")
        with open(metrics_path) as f:
            metrics = json.load(f)
    else:
        # one pass of rows over the train split: the rows stay on the device and are read back once
        got, parts = [], []
        for ss, raw in _batches(train, target_shape, batch_size, "metric calculation"):
            parts.append(_run(raw, dev, None, True, False)[0])
            got += ss
        if dev is not None and parts:
            import torch
            rows = torch.cat(parts).cpu().numpy()
        else:
            rows = np.concatenate(parts) if parts else np.zeros((0, ROW))
        pairs = _decide(got, rows, "train")
        metrics = metrics_from_rows([r for _, r in pairs], [s for s, _ in pairs], temp_query)
        with open(metrics_path, "w") as f:
            json.dump(metrics, f, indent=4)
        print(f"Saved new normalization metrics to {metrics_path}")
        kept["train"] = [s for s, _ in pairs]
    norm = norm_of(metrics)
    if dev is not None:
        import torch
        norm = torch.tensor(norm, dtype=torch.float64, device=dev)

    written: Dict[str, List[str]] = {}
    for split, subset in (("train", train), ("val", val), ("test", test)):
        out_dir = os.path.join(processed_dir, split)
        os.makedirs(out_dir, exist_ok=True)
        decided = split in kept                               # the train split after its statistics pass: only the planes are left
        todo = kept[split] if decided else subset
        keep_list, written[split] = [], []
        for ss, raw in _batches(todo, target_shape, batch_size, "processing" if decided else "filtering"):
            rows, cont, targets = (_host(t) for t in _run(raw, dev, norm, not decided, True))
            for i, s in enumerate(ss):
                if not decided:
                    keep, message = row_decision(rows[i])
                    if message is not None:
                        print(f"Failed during filtering for sample {_name(s)}: {message}. Skipping.")
                    elif not keep:
                        nd, td, dd = filter_values(rows[i])
                        print(f"Filtering out sample {output_filename(s)} due to negligible changes: NDVI diff={nd}, Temp diff={td}, DW diff={dd}")
                    if not keep:
                        continue
                keep_list.append(s)
                path = os.path.join(out_dir, output_filename(s))
                if os.path.exists(path):
                    continue
                try:
                    _save(s, raw, i, cont, targets, metrics, temp_query, path)
                    written[split].append(os.path.basename(path))
                except Exception as e:
                    print(f"Failed to process and save sample {_name(s)}: {e}")
        kept[split] = keep_list
        print(f"Kept {len(keep_list)} of {len(subset)} samples for {split}; wrote {len(written[split])} tiles to {out_dir}")
    return {"metrics": metrics, "kept": {k: [output_filename(s) for s in v] for k, v in kept.items()}, "written": written}


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.dataset_build", description=__doc__.split("\n\n")[0])
    p.add_argument("--raw-dir", required=True, help="directory of raw rasters <city>_<id>_<lat>_<lon>_<offx>_<offy>_<year>_<month>_<type>.tif|.npy")
    p.add_argument("--processed-dir", required=True, help="where normalization_metrics.json and train / val / test are written")
    p.add_argument("--cities-csv", default=None, help="CSV with columns id, population (population 0 without it)")
    p.add_argument("--temperature", required=True, help=".npz with data (T,lat,lon), lats, lons, start_year: the monthly temperature series")
    p.add_argument("--device", default="gpu", help="'gpu', a torch device name, or 'cpu' (the numpy twins)")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--holdout-ratio", type=float, default=0.01)
    p.add_argument("--seed", type=int, default=0, help="seed of the holdout-city shuffle")
    a = p.parse_args(argv)
    try:
        temp_query = ArrayTemperatureQuery.from_npz(a.temperature)
        build(a.raw_dir, a.processed_dir, temp_query, a.cities_csv, a.device, a.batch_size, a.holdout_ratio, a.seed)
    except (OSError, ValueError, KeyError, RuntimeError) as err:
        print(f"Error: {' '.join(str(err).split())}")
        return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
