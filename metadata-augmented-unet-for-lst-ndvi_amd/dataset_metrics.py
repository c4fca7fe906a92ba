"""Dataset survey (the reference's ``src/utils/visualize_npz.py extract``): one CSV row per processed tile -- mean / std / min / max of
the 23 input planes and both targets, land-cover proportions and entropies, statistics of the t1 -> t2 change of NDVI and
temperature, and temperature-series statistics.  The CSV is what the reference's ``visualize_csv`` / ``analyze_csv`` and the Dataset
page of its app read.

The reference loads every tile densely and reduces in float32.  Here

* ``tile_stats`` is ONE launch (``mau_tile_stats``) over the compact batch the package's pipeline already delivers (two uint8 class
  maps + five fp32 planes + two targets: 30 bytes per pixel, each read once): per sample an fp64 row of class histograms and, for
  nine value planes (the seven stored ones and the two t2 - t1 differences, never written to memory), n, mean, M2, min, max,
  sum |x|, NaN and non-finite counts -- the two-pass, fixed-order, chunk-merged arithmetic of ``mau_plane_moments``;
* ``sample_metrics`` turns the rows of a batch, after ONE read-back, into the reference's columns.  The one-hot planes' statistics
  come from the pixel counts; the affine un-normalisation of the temperature is applied to the MOMENTS, never per pixel; the
  temperature-series columns are a few dozen values per sample and stay on the host (numpy only);
* ``tile_metrics_host`` is the float64 numpy twin for one dense sample (``tile_rows_host`` + the same ``sample_metrics``).

    python -m mau_amd.dataset_metrics extract <input_dir> <output_csv> [--metrics-json P] [--batch-size 64] [--num-workers 0]
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

DW_CLASS_NAMES = ["water", "trees", "grass", "flooded_vegetation", "crops", "shrub_and_scrub", "built", "bare", "snow_and_ice"]
META_KEYS = ["lat", "lon", "population", "delta_time_years"]
NUM_CLASSES, N_CONT, N_TGT = 9, 5, 2
LAYOUT = f"{NUM_CLASSES} classes + {N_CONT} continuous planes (r, g, b, ndvi_t1, temp_t1) + {N_TGT} targets (ndvi_t2, temp_t2)"
CONT_NAMES = ["rgb_r", "rgb_g", "rgb_b", "ndvi_t1", "temp_t1"]
TARGET_NAMES = ["ndvi_t2", "temp_t2"]
_STATS = ("mean", "std", "min", "max")
_SERIES = ("mean", "std", "slope", "autocorr_1", "seasonal_amplitude")

# the row of mau_tile_stats (include/mau_hip.h)
MAX_CLASSES = 16
OOR = 2 * MAX_CLASSES                                   # [32], [33]: class values >= num_classes of cls_a, cls_b
PLANES0 = OOR + 2
PLANE_ROW = 8
P_N, P_MEAN, P_M2, P_MIN, P_MAX, P_L1, P_NAN, P_BAD = range(PLANE_ROW)
PLANE_NDVI_DIFF, PLANE_TEMP_DIFF = 7, 8
N_PLANES = 9
ROW = PLANES0 + N_PLANES * PLANE_ROW


def __getattr__(name):
    if name == "CHUNK_PIX":                             # the library's chunk (csrc/chunk_reduce.h): a power of two
        from ._lib import lib
        return (1 << 30) // lib.mau_plane_moments_chunks(1 << 30)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _columns() -> List[str]:
    cols = ["filepath", "split"] + [f"meta_{k}" for k in META_KEYS]                      # visualize_npz.py:23-36, :873-876
    names = [f"dw_t1_{c}" for c in DW_CLASS_NAMES] + CONT_NAMES + [f"dw_t2_{c}" for c in DW_CLASS_NAMES]
    cols += [f"input_{n}_{s}" for n in names for s in _STATS]                            # :46-51
    cols += [f"target_{n}_{s}" for n in TARGET_NAMES for s in _STATS]                    # :53-58
    for c in DW_CLASS_NAMES:                                                             # :72-74
        cols += [f"dw_t1_prop_{c}", f"dw_t2_prop_{c}"]
    cols += ["dw_t1_entropy", "dw_t2_entropy"]
    cols += [f"temp_series_{s}" for s in _SERIES]                                        # :79-111
    cols += ["delta_ndvi_l1_norm", "delta_ndvi_l2_norm", "delta_temp_l1_norm", "delta_temp_l2_norm", "pop_density_proxy"]
    cols += [f"{n}_{s}" for n in ("ndvi_diff", "temp_diff", "dw_diff") for s in _STATS]  # :122-133
    return cols


COLUMNS = _columns()


# --------------------------------------------------------------------------- #
# temperature series (host, float64)
# --------------------------------------------------------------------------- #
def series_metrics(x) -> Dict[str, float]:
    """The five ``temp_series_*`` columns of one un-normalised, un-padded series (visualize_npz.py:79-111) in float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    nan = float("nan")
    if n <= 1:                                                                           # :106-111
        return {"mean": nan if n == 0 else float(x[0]), "std": 0.0, "slope": 0.0, "autocorr_1": nan, "seasonal_amplitude": nan}
    t = np.arange(n)
    constant = bool(np.all(x == x[0]))
    out = {"mean": float(x.mean()), "std": float(x.std())}
    out["slope"] = 0.0 if constant else float(np.polyfit(t, x, 1)[0])
    # lag-1 autocorrelation: Pearson of x[1:] with x[:-1]; NaN for a series without spread (and for a single pair: 0 / 0)
    if constant or not float(x.std(ddof=1)) > 0:
        out["autocorr_1"] = nan
    else:
        a, b = x[1:] - x[1:].mean(), x[:-1] - x[:-1].mean()
        with np.errstate(invalid="ignore", divide="ignore"):
            out["autocorr_1"] = float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))
    if n > 12:                                                                           # :91-103
        detrended = x - np.polyval(np.polyfit(t, x, 1), t)
        yf = np.fft.fft(detrended)
        xf = np.fft.fftfreq(n, 1 / 12.0)
        pos = np.where(xf > 0)[0]
        out["seasonal_amplitude"] = float(2.0 / n * np.abs(yf[pos[np.argmin(np.abs(xf[pos] - 1.0))]])) if pos.size else nan
    else:
        out["seasonal_amplitude"] = nan
    return out


# --------------------------------------------------------------------------- #
# rows -> the reference's columns
# --------------------------------------------------------------------------- #
def _plane_stats(pr: np.ndarray, scale: float = 1.0):
    """(mean, std, min, max) of ``scale * x`` from the plane row of x: the un-normalisation acts on the moments."""
    n, bad_nan = pr[P_N], pr[P_NAN] != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        std = abs(scale) * math.sqrt(pr[P_M2] / n) if not math.isnan(pr[P_M2]) else float("nan")
    lo, hi = (pr[P_MIN], pr[P_MAX]) if scale >= 0 else (pr[P_MAX], pr[P_MIN])
    nan = float("nan")
    return float(pr[P_MEAN] * scale), float(std), nan if bad_nan else float(lo * scale), nan if bad_nan else float(hi * scale)


def _norms(pr: np.ndarray, scale: float = 1.0):
    """(L1, L2) norms of ``scale * x`` from the plane row of x: |s| sum |x| and |s| sqrt(M2 + n mean^2)."""
    return float(abs(scale) * pr[P_L1]), float(abs(scale) * math.sqrt(pr[P_M2] + pr[P_N] * pr[P_MEAN] ** 2)
                                               if not math.isnan(pr[P_M2] + pr[P_MEAN]) else float("nan"))


def _entropy2(p: np.ndarray) -> float:
    p = p[p > 0]
    return float(-np.sum(p * np.log(p)) / math.log(2.0))


def check_class_range(rows) -> None:
    """Raises when a class map of the batch held a value >= 9: the one-hot statistics would then miss pixels."""
    r = np.asarray(rows)
    bad = r[:, OOR] + r[:, OOR + 1]
    if np.any(bad != 0):
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"dataset_metrics: sample {i} of the batch has {int(bad[i])} class values outside [0, {NUM_CLASSES}) "
                         f"(the layout is {LAYOUT})")


def sample_metrics(rows, metadata, temp_series, lengths, metrics: Mapping) -> List[dict]:
    """rows (B, R) fp64 as read back from :func:`tile_stats`, metadata (B, >= 4) float32 (normalised, as the dataset holds it),
    temp_series (B, T) float32 padded, lengths (B,) the un-padded lengths -> per sample the reference's columns (all of ``COLUMNS``
    but ``filepath`` and ``split``), float64."""
    rows = np.asarray(rows, dtype=np.float64)
    md = np.asarray(metadata)
    ts = np.asarray(temp_series)
    lengths = np.asarray(lengths).reshape(-1)
    if rows.ndim != 2 or rows.shape[1] != ROW:
        raise ValueError(f"sample_metrics: rows must be (B, {ROW}), got {rows.shape}")
    if md.dtype != np.float32 or md.ndim != 2 or md.shape[0] != rows.shape[0] or md.shape[1] < len(META_KEYS):
        raise ValueError(f"sample_metrics: metadata must be ({rows.shape[0]}, >= {len(META_KEYS)}) float32, got {md.shape} {md.dtype}")
    if ts.ndim != 2 or ts.shape[0] != rows.shape[0] or lengths.shape[0] != rows.shape[0]:
        raise ValueError("sample_metrics: one (padded) temperature series and one length per row")
    meta_std, meta_mean = np.array(metrics["meta_std"]), np.array(metrics["meta_mean"])   # :30-32, the reference's own promotion:
    meta = md[:, :len(meta_std)] * meta_std + meta_mean                                   # float32 * float64 + float64
    s = float(metrics["temp_std"])
    out = []
    for i, r in enumerate(rows):
        planes = r[PLANES0:].reshape(N_PLANES, PLANE_ROW)
        n = planes[0, P_N]
        m = {f"meta_{k}": meta[i, j] for j, k in enumerate(META_KEYS)}
        props = [r[0:NUM_CLASSES] / n, r[MAX_CLASSES:MAX_CLASSES + NUM_CLASSES] / n]
        counts = [r[0:NUM_CLASSES], r[MAX_CLASSES:MAX_CLASSES + NUM_CLASSES]]

        def one_hot(t, c):
            p = float(props[t][c])
            return p, math.sqrt(p * (1.0 - p)), 1.0 if counts[t][c] == n else 0.0, 1.0 if counts[t][c] > 0 else 0.0

        per_plane = [(f"input_dw_t1_{c}", one_hot(0, j)) for j, c in enumerate(DW_CLASS_NAMES)]
        per_plane += [(f"input_{name}", _plane_stats(planes[j])) for j, name in enumerate(CONT_NAMES)]
        per_plane += [(f"input_dw_t2_{c}", one_hot(1, j)) for j, c in enumerate(DW_CLASS_NAMES)]
        per_plane += [(f"target_{name}", _plane_stats(planes[N_CONT + j])) for j, name in enumerate(TARGET_NAMES)]
        for name, st in per_plane:
            m.update({f"{name}_{k}": v for k, v in zip(_STATS, st)})
        for j, c in enumerate(DW_CLASS_NAMES):
            m[f"dw_t1_prop_{c}"], m[f"dw_t2_prop_{c}"] = float(props[0][j]), float(props[1][j])
        m["dw_t1_entropy"], m["dw_t2_entropy"] = _entropy2(props[0]), _entropy2(props[1])
        x = ts[i, :int(lengths[i])].astype(np.float64) * float(metrics["temp_series_std"]) + float(metrics["temp_series_mean"])
        m.update({f"temp_series_{k}": v for k, v in series_metrics(x).items()})
        m["delta_ndvi_l1_norm"], m["delta_ndvi_l2_norm"] = _norms(planes[PLANE_NDVI_DIFF])
        m["delta_temp_l1_norm"], m["delta_temp_l2_norm"] = _norms(planes[PLANE_TEMP_DIFF], s)
        m["pop_density_proxy"] = float(m["meta_population"] / (props[0][6] + 1e-9))       # :120-121
        dw_diff = props[1] - props[0]
        for name, st in (("ndvi_diff", _plane_stats(planes[PLANE_NDVI_DIFF])), ("temp_diff", _plane_stats(planes[PLANE_TEMP_DIFF], s)),
                         ("dw_diff", (float(dw_diff.mean()), float(dw_diff.std()), float(dw_diff.min()), float(dw_diff.max())))):
            m.update({f"{name}_{k}": v for k, v in zip(_STATS, st)})
        out.append(m)
    return out


# --------------------------------------------------------------------------- #
# the float64 numpy twin
# --------------------------------------------------------------------------- #
def tile_rows_host(cls_a, cls_b, cont, targets, num_classes: int = NUM_CLASSES) -> np.ndarray:
    """float64 numpy twin of :func:`tile_stats`: (B,H,W) uint8 x 2, (B,5,H,W), (B,2,H,W) -> (B, R).  np.mean / np.sum instead of the
    kernel's chunked order: equal to it within the rounding of the sums, not bit for bit."""
    a, b = np.asarray(cls_a), np.asarray(cls_b)
    c, t = np.asarray(cont, dtype=np.float32).astype(np.float64), np.asarray(targets, dtype=np.float32).astype(np.float64)
    B = a.shape[0]
    rows = np.zeros((B, ROW), dtype=np.float64)
    for i in range(B):
        for m, cm in enumerate((a[i], b[i])):
            rows[i, m * MAX_CLASSES:m * MAX_CLASSES + num_classes] = np.bincount(cm.reshape(-1), minlength=256)[:num_classes]
            rows[i, OOR + m] = int((cm >= num_classes).sum())
        vals = [c[i, j] for j in range(N_CONT)] + [t[i, j] for j in range(N_TGT)]
        with np.errstate(invalid="ignore"):
            vals += [t[i, 0] - c[i, 3], t[i, 1] - c[i, 4]]
        for p, v in enumerate(vals):
            v = v.reshape(-1)
            with np.errstate(invalid="ignore", over="ignore"):
                mean = v.mean()
                finite = v[~np.isnan(v)]
                rows[i, PLANES0 + p * PLANE_ROW:PLANES0 + (p + 1) * PLANE_ROW] = [
                    v.size, mean, np.sum((v - mean) ** 2), finite.min() if finite.size else np.inf, finite.max() if finite.size else -np.inf,
                    np.abs(v).sum(), np.isnan(v).sum(), (~np.isfinite(v)).sum()]
    return rows


def tile_metrics_host(sample_arrays: Mapping, metrics: Mapping) -> dict:
    """The columns of ONE dense sample (a mapping with ``input`` (23,H,W), ``target`` (2,H,W), ``metadata``, ``temperature_serie``, as
    a processed ``.npz`` holds them) in float64 numpy: for callers without a device, and the yardstick of the device path."""
    from .data import compact_input
    inp, tgt = np.asarray(sample_arrays["input"]), np.asarray(sample_arrays["target"])
    if inp.ndim != 3 or inp.shape[0] != 2 * NUM_CLASSES + N_CONT or tgt.shape != (N_TGT,) + inp.shape[1:]:
        raise ValueError(f"tile_metrics_host: input {inp.shape} / target {tgt.shape}: the layout is {LAYOUT}")
    a, b, cont = compact_input(inp, NUM_CLASSES)
    rows = tile_rows_host(a[None], b[None], cont[None], tgt[None])
    ts = np.asarray(sample_arrays["temperature_serie"], dtype=np.float32).reshape(1, -1)
    md = np.asarray(sample_arrays["metadata"], dtype=np.float32).reshape(1, -1)
    return sample_metrics(rows, md, ts, [ts.shape[1]], metrics)[0]


# --------------------------------------------------------------------------- #
# the kernel
# --------------------------------------------------------------------------- #
def tile_stats(cls_a, cls_b, cont, targets):
    """(B,H,W) uint8 x 2, (B,5,H,W) fp32, (B,2,H,W) fp32 on the device -> (B, R) fp64 device tensor (the row of ``mau_tile_stats``,
    include/mau_hip.h), one launch per 64 samples, no synchronisation.  A row depends on its own sample only: not on B, not on
    the sample's position; repeated calls agree bit for bit."""
    import torch
    from . import functional as F_
    from .functional import call, lib
    a = F_._device_planes(cls_a, "tile_stats", "cls_a", torch.uint8, 3, "(B, H, W)")
    b = F_._device_planes(cls_b, "tile_stats", "cls_b", torch.uint8, 3, "(B, H, W)")
    c = F_._device_planes(cont, "tile_stats", "cont", torch.float32, 4, "(B, 5, H, W)")
    t = F_._device_planes(targets, "tile_stats", "targets", torch.float32, 4, "(B, 2, H, W)")
    B, H, W = a.shape
    if b.shape != a.shape or c.shape != (B, N_CONT, H, W) or t.shape != (B, N_TGT, H, W):
        raise ValueError(f"tile_stats: cls_a {tuple(a.shape)}, cls_b {tuple(b.shape)}, cont {tuple(c.shape)}, targets {tuple(t.shape)}: "
                         f"the layout is {LAYOUT}")
    dev = a.device
    if b.device != dev or c.device != dev or t.device != dev:
        raise RuntimeError("tile_stats: all four tensors must be on the same device")
    rows = torch.empty((B, ROW), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.mau_tile_stats_ws_elems(B, H * W), dtype=torch.float64, device=dev)
    call("mau_tile_stats", a.data_ptr(), b.data_ptr(), c.data_ptr(), t.data_ptr(), rows.data_ptr(), ws.data_ptr(),
         F_._tickets(dev).data_ptr(), B, H * W, NUM_CLASSES, F_._stream())
    return rows


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def _collate(batch):
    from .data import collate_fn
    kept = [s for s in batch if s is not None]
    return (collate_fn(kept) if kept else None), [s["filepath"] for s in kept]


def extract(input_dir: str, output_csv: Optional[str] = None, metrics_path: Optional[str] = None, batch_size: int = 64,
            num_workers: int = 0, device="cuda"):
    """One pass over every ``.npz`` tile of every split folder of ``input_dir`` (sorted; without sub-folders ``input_dir`` itself is
    the one split, ``unknown``): a ``pandas.DataFrame`` with ``COLUMNS``, written to ``output_csv`` when given.  A tile that cannot
    be read or is not one-hot is reported (``Failed to process <file>: <error>``) and has no row."""
    import pandas as pd
    if metrics_path is None:
        metrics_path = os.path.join(input_dir, "normalization_metrics.json")
    if not os.path.exists(metrics_path):
        raise FileNotFoundError(f"Normalization metrics not found at {metrics_path}")
    with open(metrics_path) as f:
        metrics = json.load(f)
    import torch
    from torch.utils.data import DataLoader
    from .data import FuturePredictionDataset
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("dataset_metrics.extract: this is the MI355X-native path; it has no CPU fallback (tile_metrics_host is the "
                           "numpy twin)")
    splits = sorted(d for d in os.listdir(input_dir) if os.path.isdir(os.path.join(input_dir, d)))
    if not splits:
        print(f"No split subdirectories found in {input_dir}. Looking for .npz files directly.")
        splits = ["."]
    records: List[dict] = []
    for split in splits:
        name = split if split != "." else "unknown"
        ds = FuturePredictionDataset(split=split, processed_dir=input_dir, compact=True, skip_errors=True)
        if len(ds) == 0:
            if split != ".":
                print(f"No .npz files found in split: {split}")
            continue
        print(f"Processing {len(ds)} files from split: {name}")
        keep = None
        for host, files in DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers, collate_fn=_collate):
            if host is None:
                continue
            if host.cont.shape[1] != N_CONT or host.targets.shape[1] != N_TGT or host.num_classes != NUM_CLASSES:
                raise ValueError(f"dataset_metrics.extract: {host.cont.shape[1]} continuous planes and {host.targets.shape[1]} targets in "
                                 f"split {name!r}: the layout is {LAYOUT}")
            # only the compact batch crosses to the device; its pinned buffers stay referenced until the next batch has been queued
            pinned = tuple(t.pin_memory() for t in (host.cls_a, host.cls_b, host.cont, host.targets))
            rows = tile_stats(*(t.to(dev, non_blocking=True) for t in pinned)).cpu().numpy()      # the batch's one read-back
            keep = pinned
            check_class_range(rows)
            per = sample_metrics(rows, host.metadatas.numpy(), host.temp_series.numpy(), host.temp_series_lengths.numpy(), metrics)
            for fp, m in zip(files, per):
                records.append({"filepath": fp, "split": name, **m})
        del keep
    if not records:
        raise FileNotFoundError(f"No metrics were extracted from any split of {input_dir}")
    df = pd.DataFrame(records, columns=COLUMNS)
    if output_csv is not None:
        out_dir = os.path.dirname(os.path.abspath(output_csv))
        os.makedirs(out_dir, exist_ok=True)
        df.to_csv(output_csv, index=False)
        print(f"Metrics for all splits saved to {output_csv}")
    return df


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.dataset_metrics", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    e = sub.add_parser("extract", help="Extract per-tile metrics from a directory of processed tiles to a CSV file.")
    e.add_argument("input_dir", help="directory that holds the split folders (train / val / test) of .npz tiles")
    e.add_argument("output_csv", help="path of the CSV file to write")
    e.add_argument("--metrics-json", default=None, help="normalization_metrics.json (default: <input_dir>/normalization_metrics.json)")
    e.add_argument("--batch-size", type=int, default=64)
    e.add_argument("--num-workers", type=int, default=0)
    e.add_argument("--device", default="gpu", help="'gpu' or a torch device name; this path has no CPU fallback")
    a = p.parse_args(argv)
    from .functional import argparse_device
    device = argparse_device(p, a.device)
    try:
        extract(a.input_dir, a.output_csv, a.metrics_json, a.batch_size, a.num_workers, device)
    except FileNotFoundError as err:
        print(f"Error: {err}")
        return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
