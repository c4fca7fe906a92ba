"""Ground-truth sensitivity (the reference's ``test/generate_ground_truth_sensitivity.py``): mean and standard deviation of the
targets of a split, binned by latitude and by longitude -- the curves ``test/compare_sensitivity.py`` draws the model sweeps of
``mau_amd.sensitivity`` against.

The reference keeps every target of the split on the host (``targets_all``) and reduces in float32.  Here

* ``plane_moments`` is ONE launch (``mau_plane_moments``): per (sample, channel) plane the fp64 row (n, mean, M2 = sum (x - mean)^2,
  non-finite count), two passes over register-resident values, chunk rows merged in chunk order;
* ``BinStats.update`` adds ONE more (``mau_bin_moments``): the rows of the batch merged, in sample order, into a device-resident
  table [axis][bin][channel] of such rows.  Nothing is read back per batch and nothing synchronises;
* ``BinStats.result`` reads the table back once and applies the affine un-normalisation to the bin's MOMENTS (mean -> scale * mean +
  shift, std -> |scale| * sqrt(M2 / n)), never per pixel.

    python -m mau_amd.ground_truth --processed-dir data/processed [--split test] [--output-dir reports/tests/sensitivity]
                                   [--batch-size 256] [--num-workers 0]

``bin_stats_host`` is the float64 numpy twin (same moments, same merge) for callers without the device table.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from .functional import call, lib

LAT_RANGE = np.linspace(-60, 70, 50)                   # generate_ground_truth_sensitivity.py:92-95
LON_RANGE = np.linspace(-180, 180, 50)
FILENAME = "sensitivity_data_ground_truth.json"
_ROW = 4                                                # include/mau_hip.h: n, mean, M2, non-finite values


def bin_edges(centers) -> np.ndarray:
    """The reference's bin edges (:107-111) in float64: midpoints between the centres, the two outer edges half a step outside."""
    c = np.asarray(centers, dtype=np.float64)
    if c.ndim != 1 or c.size < 2:
        raise ValueError("bin_edges: at least two bin centres")
    return np.concatenate([[c[0] - (c[1] - c[0]) / 2], (c[:-1] + c[1:]) / 2, [c[-1] + (c[-1] - c[-2]) / 2]])


def merge_moments(a: Tuple[float, float, float], b: Tuple[float, float, float]) -> Tuple[float, float, float]:
    """(n, mean, M2) of the union of two sets: the pairwise update of ``mau_bin_moments`` / ``mau_plane_moments``, operation for
    operation (Python floats are IEEE doubles and nothing is contracted)."""
    na, ma, qa = a
    nb, mb, qb = b
    if na == 0.0:
        return nb, mb, qb
    delta = mb - ma
    n = na + nb
    return n, ma + (delta * nb) / n, (qa + qb) + (delta * delta) * ((na * nb) / n)


def bin_stats_host(coords, planes, centers):
    """float64 numpy twin of the device path for ONE channel: coords (N,) un-normalised coordinates, planes (N, ...) the values of
    every sample, centers the bin centres.  Returns (means, stds, counts): per bin the mean and population standard deviation over
    ALL values of ALL samples whose coordinate ``np.digitize`` puts there (NaN where there is none) and the number of samples."""
    x = np.asarray(coords, dtype=np.float64).reshape(-1)
    y = np.asarray(planes, dtype=np.float64)
    if y.shape[0] != x.shape[0]:
        raise ValueError(f"bin_stats_host: {x.shape[0]} coordinates for {y.shape[0]} samples")
    y = y.reshape(x.shape[0], -1)
    edges = bin_edges(centers)
    nbins = len(edges) - 1
    idx = np.digitize(x, edges)
    acc = [(0.0, 0.0, 0.0)] * nbins
    counts = [0] * nbins
    for i in range(x.shape[0]):                          # sample order, as the device walks a batch
        k = int(idx[i])
        if 1 <= k <= nbins and y.shape[1]:
            m = float(np.mean(y[i]))
            acc[k - 1] = merge_moments(acc[k - 1], (float(y.shape[1]), m, float(np.sum((y[i] - m) ** 2))))
            counts[k - 1] += 1
    means = [m if n else float("nan") for n, m, _ in acc]
    stds = [math.sqrt(q / n) if n and not math.isnan(q) else float("nan") for n, _, q in acc]
    return means, stds, counts


# --------------------------------------------------------------------------- #
# the kernels
# --------------------------------------------------------------------------- #
def plane_moments(targets: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, C, H, W) fp32 on the device -> (B, C, 4) fp64 device tensor of (n, mean, M2, non-finite count) per plane, one launch per
    64 planes.  A row depends on its own plane only: not on B, not on the plane's position; repeated calls agree bit for bit.
    ws: an fp64 device workspace of at least ``mau_plane_moments_ws_elems(B, C, H * W)`` elements (None: allocated here)."""
    t = F_._device_planes(targets, "plane_moments", "targets", torch.float32, 4, "(B, C, H, W)")
    B, C, H, W = t.shape
    dev = t.device
    rows = torch.empty((B, C, _ROW), dtype=torch.float64, device=dev)
    if ws is None:
        ws = torch.empty(lib.mau_plane_moments_ws_elems(B, C, H * W), dtype=torch.float64, device=dev)
    call("mau_plane_moments", t.data_ptr(), rows.data_ptr(), ws.data_ptr(), F_._tickets(dev).data_ptr(), B, C, H * W, F_._stream())
    return rows


@dataclass(frozen=True)
class Axis:
    """One binning axis: the metadata column it reads, what un-normalises that column (coordinate = meta * std + mean) and the bin
    centres."""
    name: str
    column: int
    centers: Sequence[float]
    std: float = 1.0
    mean: float = 0.0


class BinStats:
    """Device-resident table [axis][bin][channel] of moment rows over every sample seen by :meth:`update`.  All axes have the same
    number of bins; ``len(axes) * bins * channels`` is at most ``mau_bin_moments_max_entries()``.  The edges are checked to ascend
    here: the device cannot."""

    def __init__(self, axes: Sequence[Axis], channels: int, device="cuda"):
        self.axes = list(axes)
        self.channels = int(channels)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BinStats: this is the MI355X-native path; it has no CPU fallback (bin_stats_host is the numpy twin)")
        if not self.axes or self.channels < 1:
            raise ValueError("BinStats: at least one axis and one channel")
        edges = [bin_edges(a.centers) for a in self.axes]
        self.bins = len(edges[0]) - 1
        if any(len(e) != self.bins + 1 for e in edges):
            raise ValueError("BinStats: every axis must have the same number of bins")
        for a, e in zip(self.axes, edges):
            if not (np.all(np.isfinite(e)) and np.all(np.diff(e) > 0)):
                raise ValueError(f"BinStats: the bin edges of axis {a.name!r} must be finite and ascending")
            if a.column < 0:
                raise ValueError(f"BinStats: axis {a.name!r} reads metadata column {a.column}")
        n = len(self.axes)
        if n > 4 or n * self.bins * self.channels > lib.mau_bin_moments_max_entries():
            raise ValueError(f"BinStats: {n} axes x {self.bins} bins x {self.channels} channels do not fit one workgroup "
                             f"(at most 4 axes and {lib.mau_bin_moments_max_entries()} entries)")
        self._cols = (ctypes.c_int * n)(*[int(a.column) for a in self.axes])
        self._std = (ctypes.c_double * n)(*[float(a.std) for a in self.axes])
        self._mean = (ctypes.c_double * n)(*[float(a.mean) for a in self.axes])
        self._edges = torch.from_numpy(np.stack(edges)).to(self.device)
        self.table = torch.zeros((n, self.bins, self.channels, _ROW), dtype=torch.float64, device=self.device)
        self.plane_pixels: Optional[int] = None
        self._ws = None

    def update(self, targets: torch.Tensor, metadata: torch.Tensor) -> None:
        """Two launches on the current stream, no host synchronisation.  targets (B, channels, H, W) fp32, metadata (B, F) fp32 --
        normalised, as the dataset holds it -- both on the device."""
        t = F_._device_planes(targets, "BinStats.update", "targets", torch.float32, 4, "(B, C, H, W)")
        F_._require_cuda(metadata, "BinStats.update")
        B, C, H, W = t.shape
        if C != self.channels:
            raise ValueError(f"BinStats.update: {C} target channels, the table has {self.channels}")
        if metadata.dtype != torch.float32 or metadata.dim() != 2 or metadata.shape[0] != B:
            raise ValueError(f"BinStats.update: metadata must be ({B}, F) float32, got {tuple(metadata.shape)} {metadata.dtype}")
        if max(a.column for a in self.axes) >= metadata.shape[1]:
            raise ValueError(f"BinStats.update: metadata has {metadata.shape[1]} columns")
        if self.plane_pixels not in (None, H * W):
            raise ValueError(f"BinStats.update: planes of {H * W} pixels after planes of {self.plane_pixels} (sample counts are "
                             "pixel counts over the plane size)")
        self.plane_pixels = H * W
        md = metadata.detach()
        if md.stride(1) != 1 or md.stride(0) < md.shape[1]:
            md = md.contiguous()
        need = lib.mau_plane_moments_ws_elems(B, C, H * W)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float64, device=self.device)
        rows = plane_moments(t, self._ws)
        call("mau_bin_moments", rows.data_ptr(), md.data_ptr(), md.stride(0), self._cols, self._std, self._mean, self._edges.data_ptr(),
             self.table.data_ptr(), B, C, len(self.axes), self.bins, F_._stream())

    def result(self, scale=None, shift=None) -> Dict[str, dict]:
        """The single read-back.  Per axis name: ``x`` (bin centres), ``mean`` and ``std`` (channels, bins) float64 arrays of
        ``scale * mean + shift`` and ``|scale| * sqrt(M2 / n)`` (population, as ``np.std``; NaN in both for an empty bin),
        ``count`` (bins,) samples per bin and ``nonfinite`` (channels, bins) non-finite values per bin.  scale / shift: one value
        per channel (None = 1 / 0)."""
        sc = np.ones(self.channels) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
        sh = np.zeros(self.channels) if shift is None else np.asarray(shift, dtype=np.float64).reshape(-1)
        if sc.size != self.channels or sh.size != self.channels:
            raise ValueError(f"BinStats.result: scale and shift must hold one value per channel ({self.channels})")
        tab = self.table.cpu().numpy()                                                # (axes, bins, C, 4)
        out = {}
        for a, axis in enumerate(self.axes):
            n, mean, m2, bad = (tab[a, :, :, k].T for k in range(_ROW))               # (C, bins) each
            with np.errstate(invalid="ignore", divide="ignore"):
                mean_u = np.where(n > 0, sc[:, None] * mean + sh[:, None], np.nan)
                std_u = np.abs(sc)[:, None] * np.sqrt(m2 / n)                         # 0 / 0: NaN for an empty bin
            count = np.rint(n[0] / self.plane_pixels).astype(np.int64) if self.plane_pixels else np.zeros(self.bins, dtype=np.int64)
            out[axis.name] = {"x": np.asarray(axis.centers, dtype=np.float64), "mean": mean_u, "std": std_u, "count": count,
                              "nonfinite": bad.astype(np.int64)}
        return out


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def channel_affine(channels: Sequence[str], metrics: dict):
    """(scale, shift) per target channel: the temperature channels are un-normalised, the others left as they are (:75-80)."""
    scale = [float(metrics["temp_std"]) if "temp" in ch.lower() else 1.0 for ch in channels]
    shift = [float(metrics["temp_mean"]) if "temp" in ch.lower() else 0.0 for ch in channels]
    return scale, shift


def export_dict(result: Dict[str, dict], channels: Sequence[str]) -> dict:
    """The reference's export dictionary (:97-157) from :meth:`BinStats.result`."""
    sweeps = {}
    for name, r in result.items():
        sweeps[name] = {"x": [float(v) for v in r["x"]],
                        "channels": {ch: {"mean": [float(v) for v in r["mean"][c]], "std": [float(v) for v in r["std"][c]]}
                                     for c, ch in enumerate(channels)}}
    return {"model_name": "Ground Truth (Dataset)", "model_type": "dataset", "sweeps": sweeps, "heatmaps": {}}


def ground_truth_stats(processed_dir: str, split: str = "test", batch_size: int = 256, num_workers: int = 0,
                       channels: Sequence[str] = ("after_ndvi", "after_temp"), device="cuda") -> Dict[str, dict]:
    """One pass over ``<processed_dir>/<split>``: :meth:`BinStats.result` of the latitude and longitude axes, un-normalised with
    ``<processed_dir>/normalization_metrics.json``."""
    from .data import create_dataloader
    metrics_path = os.path.join(processed_dir, "normalization_metrics.json")
    if not os.path.exists(metrics_path):
        raise FileNotFoundError(f"Metrics file not found at {metrics_path}")
    with open(metrics_path) as f:
        metrics = json.load(f)
    meta_mean, meta_std = metrics["meta_mean"], metrics["meta_std"]            # meta indices: 0 = lat, 1 = lon (:34-36)
    dev = torch.device(device)
    stats = BinStats([Axis("latitude", 0, LAT_RANGE, float(meta_std[0]), float(meta_mean[0])),
                      Axis("longitude", 1, LON_RANGE, float(meta_std[1]), float(meta_mean[1]))], len(channels), dev)
    loader = create_dataloader(split, batch_size, False, num_workers=num_workers, processed_dir=processed_dir, device=None)
    keep = None
    for host in loader:
        # only what the statistics read crosses to the device; the pinned buffers of a batch stay referenced until the next batch
        # has been queued behind its copy (DeviceLoader keeps them the same way)
        pinned = (host.targets.pin_memory(), host.metadatas.pin_memory())
        stats.update(pinned[0].to(dev, non_blocking=True), pinned[1].to(dev, non_blocking=True))
        keep = pinned
    scale, shift = channel_affine(channels, metrics)
    res = stats.result(scale, shift)                                            # the pass's only synchronisation
    del keep
    return res


def ground_truth_sensitivity(processed_dir: str, split: str = "test", batch_size: int = 256, num_workers: int = 0,
                             channels: Sequence[str] = ("after_ndvi", "after_temp"), device="cuda") -> dict:
    """The reference's ground-truth export for a split: keys ``model_name``, ``model_type`` ("dataset"), ``sweeps`` (latitude /
    longitude -> ``x`` and per channel ``mean`` / ``std`` over all pixels of all samples of a bin, NaN for an empty bin) and an
    empty ``heatmaps``."""
    return export_dict(ground_truth_stats(processed_dir, split, batch_size, num_workers, channels, device), channels)


def save(data: dict, output_dir: str) -> str:
    """Write ``sensitivity_data_ground_truth.json`` (:159-164; NaN is written as Python's ``NaN``, as the reference does)."""
    os.makedirs(output_dir, exist_ok=True)
    out_path = os.path.join(output_dir, FILENAME)
    with open(out_path, "w") as f:
        json.dump(data, f, indent=4)
    return out_path


def main(argv=None) -> int:
    from .config import CONFIG
    p = argparse.ArgumentParser(prog="python -m mau_amd.ground_truth", description=__doc__.split("\n\n")[0])
    p.add_argument("--processed-dir", required=True, help="directory that holds the splits and normalization_metrics.json")
    p.add_argument("--split", default="test")
    p.add_argument("--output-dir", default="reports/tests/sensitivity")
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--num-workers", type=int, default=0)
    p.add_argument("--device", default="gpu", help="'gpu' or a torch device name; this path has no CPU fallback")
    a = p.parse_args(argv)
    device = F_.argparse_device(p, a.device)
    channels = list(CONFIG.dataset.target_channels)
    print(f"Target Channels: {channels}")
    try:
        data = ground_truth_sensitivity(a.processed_dir, a.split, a.batch_size, a.num_workers, channels, device)
    except FileNotFoundError as e:
        print(f"Error: {e}")
        return 1
    print(f"Saved Ground Truth sensitivity data to: {save(data, a.output_dir)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
