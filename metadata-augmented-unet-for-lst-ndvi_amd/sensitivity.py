"""Metadata sensitivity sweeps (the reference's ``test/metadata_sensitivity.py``) for both model types.

The reference repeats ONE test tile 50 times, changes only the latitude (then the longitude, then both over a 20x20
grid in chunks of 50), runs the model on the repeated tile and keeps ``np.mean`` of every ``(H, W)`` output map
(:294-325, :340-366, :394-444).  Here

* the part of the network that does not see the metadata runs once per tile, at batch 1 -- the U-Net's encoder, the
  U-Net++'s encoder column ``x^{0..4,0}`` -- and only the rest runs at batch B (``sweep_outputs``);
* the per-sample means come out of the head's own launch (``mau_head_mean``: 1x1 head + fp64 spatial mean, the
  ``(B, C, H, W)`` map is never written), as a ``(B, C)`` fp64 table on the device (``sweep_means``);
* ``metadata_rows`` builds the rows of a sweep, ``SensitivityReport`` collects the curves and heatmaps and writes the
  ``sensitivity_data_<model_name>.json`` that the reference's ``test/compare_sensitivity.py`` reads (:627-683).

    python -m mau_amd.sensitivity --checkpoint best.pth --samples 10 --output-dir reports/sensitivity [--precision bf16] [--heatmaps 2]

runs the sweeps of a reference-layout checkpoint on synthetic tiles in the loader's tuple layout (the dataset is not
shipped; ``train.py`` does the same).  No plotting, pandas or wandb.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import functional as F_
from .functional import call, dtype_code, lib
from .model import UrbanPredictor

LAT_RANGE = (-60.0, 70.0)          # "avoid extreme poles", test/metadata_sensitivity.py:219
LON_RANGE = (-180.0, 180.0)
SWEEP_STEPS = 50                   # :217-218
HEATMAP_STEPS = 20                 # :383-386
CHUNK = 50                         # heatmap_batch_size, :408


# --------------------------------------------------------------------------- #
# the sweeps
# --------------------------------------------------------------------------- #
def _net(model):
    return model.model if isinstance(model, UrbanPredictor) else model


def _final(net) -> torch.nn.Conv2d:
    return net.final


def _chunks(B: int, chunk: int):
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    return [(b0, min(B, b0 + chunk)) for b0 in range(0, B, chunk)]


def _rows(t: torch.Tensor, b0: int, b1: int) -> torch.Tensor:
    return t if t.shape[0] == 1 else t[b0:b1]


@torch.no_grad()
def sweep_outputs(model, maps, temp_series, metadata, chunk: int = CHUNK) -> torch.Tensor:
    """One tile x B metadata vectors -> (B, out_channels, H, W) fp32, equal to the eval-mode forward on the tile repeated B
    times.  maps (1,C,H,W); temp_series (1,T) or (B,T); metadata (B,F).  The metadata-independent encoder runs once, at
    batch 1, for all chunks; the rest of the network runs ``chunk`` rows at a time.  Both model types
    (``"unet"``: ``forward_metadata_sweep``)."""
    net = _net(model)
    enc = net._sweep_encoder(maps)
    outs = [net._head(net._sweep_trunk(enc, _rows(temp_series, b0, b1), metadata[b0:b1]))
            for b0, b1 in _chunks(metadata.shape[0], chunk)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def _coeffs(v, Co: int, dev, what: str) -> Optional[torch.Tensor]:
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=torch.float64).to(dev).reshape(-1).contiguous()
    if t.numel() != Co:
        raise ValueError(f"{what} must hold one value per output channel ({Co}), got {t.numel()}")
    return t


def head_mean(a: torch.Tensor, C: int, weight, bias, scale=None, shift=None, activate: bool = True, out: Optional[torch.Tensor] = None):
    """``scale * mean_HW(head(a)) + shift`` of an NHWC-ld activation: (N, Co) fp64 on the device, one launch
    (``mau_head_mean``).  The head is ``functional.Head``'s: 1x1 conv, tanh on channel 0 when Co == 2."""
    F_._require_cuda(a, "head_mean")
    a = F_._as_nhwc(a)
    N, H, W, _ = a.shape
    Co = weight.shape[0]
    w2 = weight.detach().reshape(Co, C).contiguous().float()
    scale, shift = _coeffs(scale, Co, a.device, "scale"), _coeffs(shift, Co, a.device, "shift")
    if out is None:
        out = torch.empty((N, Co), dtype=torch.float64, device=a.device)
    if tuple(out.shape) != (N, Co) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("head_mean: out must be a contiguous (N, Co) fp64 tensor")
    ws = torch.empty(lib.mau_head_mean_ws_elems(N, H * W, Co), dtype=torch.float64, device=a.device)
    call("mau_head_mean", a.data_ptr(), F_._ld(a), w2.data_ptr(), bias.detach().data_ptr(),
         None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(), out.data_ptr(), ws.data_ptr(),
         F_._tickets(a.device).data_ptr(), 1 if (Co == 2 and activate) else 0, dtype_code(a.dtype), N, H * W, C, Co, F_._stream())
    return out


@torch.no_grad()
def sweep_means(model, maps, temp_series, metadata, scale=None, shift=None, chunk: int = CHUNK) -> torch.Tensor:
    """``scale * sweep_outputs(...).mean((2, 3)) + shift`` as a (B, out_channels) fp64 tensor on the device, without the
    maps: the trunk of ``sweep_outputs`` with ``mau_head_mean`` in place of the head.  ``scale`` / ``shift``: one value per
    output channel (the sensitivity script un-normalises the temperature channel, ``y * temp_std + temp_mean``,
    test/metadata_sensitivity.py:22-39); None = identity.  A row's value depends on nothing but its own metadata: not on B,
    not on ``chunk``; repeated calls agree bit for bit."""
    net = _net(model)
    enc = net._sweep_encoder(maps)
    final = _final(net)
    B, Co = metadata.shape[0], final.weight.shape[0]
    scale, shift = _coeffs(scale, Co, metadata.device, "scale"), _coeffs(shift, Co, metadata.device, "shift")
    means = torch.empty((B, Co), dtype=torch.float64, device=metadata.device)
    for b0, b1 in _chunks(B, chunk):
        a = net._sweep_trunk(enc, _rows(temp_series, b0, b1), metadata[b0:b1])
        head_mean(a.t, a.C, final.weight, final.bias, scale, shift, out=means[b0:b1])
    return means


# --------------------------------------------------------------------------- #
# the rows of a sweep
# --------------------------------------------------------------------------- #
def metadata_rows(metadata, t1, t2, column, values, meta_mean, meta_std, n_meta: int) -> torch.Tensor:
    """The metadata rows of one sweep (test/metadata_sensitivity.py:294-304, :383-406): the sample's z-scored metadata
    ``(1, F)`` repeated once per value, ``column`` (0 = latitude, 1 = longitude) replaced by ``(values - mean) / std``, and
    ``t1``, ``t2`` (the two ``(1, 2)`` date pairs of the loader's tuple) appended when ``n_meta == 8``.
    2-D form: ``column=(0, 1)`` and ``values=(lats, lons)`` -- both columns replaced, rows in the order of
    ``np.meshgrid(lats, lons, indexing='ij')`` flattened (latitude-major)."""
    meta_mean, meta_std = np.asarray(meta_mean, dtype=np.float64), np.asarray(meta_std, dtype=np.float64)
    if isinstance(column, (tuple, list)):
        cols = [int(c) for c in column]
        grids = np.meshgrid(*[np.asarray(v, dtype=np.float64) for v in values], indexing="ij")
        vals = [g.flatten() for g in grids]
    else:
        cols, vals = [int(column)], [np.asarray(values, dtype=np.float64).reshape(-1)]
    if len(cols) != len(vals) or any(c not in (0, 1) for c in cols):
        raise ValueError("column is 0 (latitude), 1 (longitude) or (0, 1) with values=(lats, lons)")
    n = len(vals[0])
    rows = metadata.repeat(n, 1)
    for c, v in zip(cols, vals):
        rows[:, c] = torch.tensor((v - meta_mean[c]) / meta_std[c], device=rows.device, dtype=rows.dtype)
    if n_meta == 8:
        rows = torch.cat([rows, t1.repeat(n, 1), t2.repeat(n, 1)], dim=1)
    return rows


def model_name_of(temporal_embeddings: bool, metadata_embeddings: bool, model_type: str) -> str:
    """test/metadata_sensitivity.py:108-118."""
    name = "emb" if temporal_embeddings and metadata_embeddings else "metaemb" if metadata_embeddings \
        else "tempemb" if temporal_embeddings else "noemb"
    return name + ("++" if "++" in model_type else "")


# --------------------------------------------------------------------------- #
# the report
# --------------------------------------------------------------------------- #
class SensitivityReport:
    """Collects per-sample latitude / longitude curves and optional latitude x longitude heatmaps, and exports the dictionary
    of test/metadata_sensitivity.py:627-683 (``sensitivity_data_<model_name>.json``, read by test/compare_sensitivity.py)."""

    def __init__(self, model_name: str, model_type: str, channels: Sequence[str] = ("after_ndvi", "after_temp"),
                 lat_range=None, lon_range=None, heat_lats=None, heat_lons=None):
        self.model_name, self.model_type, self.channels = model_name, model_type, list(channels)
        self.lat_range = np.linspace(*LAT_RANGE, SWEEP_STEPS) if lat_range is None else np.asarray(lat_range, dtype=np.float64)
        self.lon_range = np.linspace(*LON_RANGE, SWEEP_STEPS) if lon_range is None else np.asarray(lon_range, dtype=np.float64)
        self.heat_lats = np.linspace(*LAT_RANGE, HEATMAP_STEPS) if heat_lats is None else np.asarray(heat_lats, dtype=np.float64)
        self.heat_lons = np.linspace(*LON_RANGE, HEATMAP_STEPS) if heat_lons is None else np.asarray(heat_lons, dtype=np.float64)
        self.lat_curves: List[np.ndarray] = []          # per sample: (len(lat_range), channels)
        self.lon_curves: List[np.ndarray] = []
        self.heatmaps: Dict[str, dict] = {}

    # -- accumulation -----------------------------------------------------------
    @staticmethod
    def _host(a) -> np.ndarray:
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    def add_curves(self, lat_curve, lon_curve):
        """One sample's curves: (len(lat_range), channels) and (len(lon_range), channels)."""
        lat, lon = self._host(lat_curve), self._host(lon_curve)
        if lat.shape != (len(self.lat_range), len(self.channels)) or lon.shape != (len(self.lon_range), len(self.channels)):
            raise ValueError(f"curves must be (steps, {len(self.channels)}): got {lat.shape} and {lon.shape}")
        self.lat_curves.append(lat)
        self.lon_curves.append(lon)

    def add_heatmap(self, idx, values, sample_label: Optional[str] = None, orig_lat: float = 0.0, orig_lon: float = 0.0):
        """One sample's grid: (len(heat_lats) * len(heat_lons), channels), rows latitude-major (``metadata_rows`` 2-D order)."""
        v = self._host(values)
        nl, no = len(self.heat_lats), len(self.heat_lons)
        if v.shape != (nl * no, len(self.channels)):
            raise ValueError(f"heatmap values must be ({nl * no}, {len(self.channels)}): got {v.shape}")
        # the reference pivots on (latitude, longitude): both axes ascending (:672-677)
        il, io = np.argsort(self.heat_lats, kind="stable"), np.argsort(self.heat_lons, kind="stable")
        grid = v.reshape(nl, no, len(self.channels))[il][:, io]
        self.heatmaps[str(idx)] = {
            "sample_label": f"Sample {idx}" if sample_label is None else sample_label,
            "orig_lat": float(orig_lat), "orig_lon": float(orig_lon),
            "channels": {ch: {"values": grid[:, :, c].tolist(), "lats": self.heat_lats[il].tolist(), "lons": self.heat_lons[io].tolist()}
                         for c, ch in enumerate(self.channels)}}

    def run_sample(self, model, maps, temp_series, metadata, t1, t2, meta_mean, meta_std, n_meta: int, scale=None, shift=None,
                   heatmap: bool = False, idx=None, chunk: int = CHUNK):
        """The sweeps of one sample (one tile of the loader's tuple): latitude, longitude and -- ``heatmap=True`` -- the 2-D
        grid, as ONE ``sweep_means`` call over all their rows (the encoder runs once per sample) and one read-back."""
        rows = [metadata_rows(metadata, t1, t2, 0, self.lat_range, meta_mean, meta_std, n_meta),
                metadata_rows(metadata, t1, t2, 1, self.lon_range, meta_mean, meta_std, n_meta)]
        if heatmap:
            rows.append(metadata_rows(metadata, t1, t2, (0, 1), (self.heat_lats, self.heat_lons), meta_mean, meta_std, n_meta))
        means = sweep_means(model, maps, temp_series, torch.cat(rows, dim=0), scale, shift, chunk).cpu().numpy()
        n_lat, n_lon = len(self.lat_range), len(self.lon_range)
        self.add_curves(means[:n_lat], means[n_lat:n_lat + n_lon])
        if heatmap:
            m = np.asarray(meta_mean, dtype=np.float64), np.asarray(meta_std, dtype=np.float64)
            self.add_heatmap(len(self.lat_curves) - 1 if idx is None else idx, means[n_lat + n_lon:],
                             orig_lat=float(metadata[0, 0]) * m[1][0] + m[0][0], orig_lon=float(metadata[0, 1]) * m[1][1] + m[0][1])
        return means

    # -- export -----------------------------------------------------------------
    def export(self) -> dict:
        if not self.lat_curves:
            raise RuntimeError("SensitivityReport.export: no sample has been added")
        data = {"model_name": self.model_name, "model_type": self.model_type,
                "sweeps": {"latitude": {"x": self.lat_range.tolist(), "channels": {}},
                           "longitude": {"x": self.lon_range.tolist(), "channels": {}}}}
        for key, curves in (("latitude", self.lat_curves), ("longitude", self.lon_curves)):
            stack = np.stack(curves)                                   # (samples, steps, channels)
            for c, ch in enumerate(self.channels):
                data["sweeps"][key]["channels"][ch] = {"mean": np.mean(stack[:, :, c], axis=0).tolist(),
                                                       "std": np.std(stack[:, :, c], axis=0).tolist()}
        data["heatmaps"] = dict(self.heatmaps)
        return data

    def save(self, output_dir: str) -> str:
        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir, f"sensitivity_data_{self.model_name}.json")
        with open(path, "w") as f:
            json.dump(self.export(), f, indent=4)
        return path


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def synthetic_tile(gen: torch.Generator, channels: int, edge: int, seq_len: int, n_meta: int, n_targets: int, device):
    """One tile in the loader's tuple layout (src/dataset.py:87-108, batch 1): (inputs, metadata, temp_series, lengths, t1_dates,
    t2_dates, targets)."""
    mk = lambda *s: torch.randn(*s, generator=gen).to(device)       # noqa: E731
    return (mk(1, channels, edge, edge), mk(1, n_meta - 4 if n_meta >= 8 else n_meta), mk(1, seq_len), torch.full((1,), seq_len),
            mk(1, 2), mk(1, 2), mk(1, n_targets, edge, edge))


def load_for_sensitivity(checkpoint_path: str, seq_len: int, study_name: str = "", device: str = "cuda"):
    """(model in eval mode, model_name, model_type, metadata_input_length) of a reference-layout checkpoint, resolved as
    test/metadata_sensitivity.py:79-133 does (embedding flags, ``model_type`` default 'unet', ``metadata_input_length``
    default 4, ``temporal_dim`` / ``meta_dim`` / ``lstm_hidden`` defaults 16 / 8 / 32).  Input channels and filter width are
    read off the first convolution's weight (the reference takes them from its CONFIG and the constructor default)."""
    from .checkpoint import SENSITIVITY_WIDTHS, load_reference_checkpoint, resolve_embedding_flags
    model, ckpt = load_reference_checkpoint(checkpoint_path, seq_len, SENSITIVITY_WIDTHS, study_name, device)
    model_type = ckpt.get("model_type", "unet")
    return model, model_name_of(*resolve_embedding_flags(ckpt, study_name), model_type), model_type, ckpt.get("metadata_input_length", 4)


def run_cli(checkpoint: str, samples: int, output_dir: str, precision: str = "bf16", heatmaps: int = 0, metrics_json: str = "",
            tile: Optional[int] = None, seq_len: Optional[int] = None, seed: Optional[int] = None, study_name: str = "",
            chunk: int = CHUNK) -> str:
    """Body of the CLI; returns the path of the JSON it wrote."""
    from .config import CONFIG
    from .evaluate import temperature_coeffs
    ds = CONFIG.dataset
    tile = ds.image_shape_edge if tile is None else tile
    seq_len = ds.temporal_length if seq_len is None else seq_len
    model, model_name, model_type, n_meta = load_for_sensitivity(checkpoint, seq_len, study_name)
    model.set_precision(precision)
    net = _net(model)
    channels = list(ds.target_channels)
    Co = _final(net).weight.shape[0]
    if len(channels) != Co:
        channels = [f"channel_{i}" for i in range(Co)]
    if metrics_json:
        with open(metrics_json) as f:
            metrics = json.load(f)
    else:                                                            # identity normalisation
        metrics = {"meta_mean": [0.0] * 4, "meta_std": [1.0] * 4, "temp_mean": 0.0, "temp_std": 1.0}
    # (test/metadata_sensitivity.py:22-39; a metrics file without the temperature keys leaves the channel as it is)
    scale, shift = temperature_coeffs(channels, {"temp_mean": 0.0, "temp_std": 1.0, **metrics})
    report = SensitivityReport(model_name, model_type, channels)
    gen = torch.Generator().manual_seed(CONFIG.seed if seed is None else seed)
    in_ch = net.conv0_0.conv1.in_channels
    for i in range(samples):
        inputs, metadata, temp_series, _lengths, t1, t2, _targets = synthetic_tile(gen, in_ch, tile, seq_len, n_meta, Co, "cuda")
        report.run_sample(model, inputs, temp_series, metadata, t1, t2, metrics["meta_mean"], metrics["meta_std"], n_meta,
                          scale, shift, heatmap=i < heatmaps, idx=i, chunk=chunk)
    path = report.save(output_dir)
    print(f"Saved sensitivity data to {path}")
    return path


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.sensitivity", description=__doc__.split("\n\n")[0])
    p.add_argument("--checkpoint", required=True, help="reference-layout .pth (src/train.py:303-316)")
    p.add_argument("--samples", type=int, required=True, help="number of synthetic tiles to sweep")
    p.add_argument("--output-dir", required=True)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--heatmaps", type=int, default=0, help="the first K samples also get the 20x20 latitude x longitude grid")
    p.add_argument("--metrics-json", default="", help="normalization_metrics.json (meta_mean, meta_std, temp_mean, temp_std); default: identity")
    p.add_argument("--tile", type=int, default=None, help="tile edge (default: dataset.image_shape_edge of the config)")
    p.add_argument("--seq-len", type=int, default=None, help="length of the temperature series (default: dataset.temporal_length)")
    p.add_argument("--seed", type=int, default=None, help="seed of the synthetic tiles (default: the config's seed)")
    p.add_argument("--study-name", default="", help="legacy checkpoints: a name containing 'noemb' selects no embeddings")
    p.add_argument("--chunk", type=int, default=CHUNK, help="rows per forward (the reference uses 50)")
    a = p.parse_args(argv)
    run_cli(a.checkpoint, a.samples, a.output_dir, a.precision, a.heatmaps, a.metrics_json, a.tile, a.seq_len, a.seed, a.study_name, a.chunk)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
