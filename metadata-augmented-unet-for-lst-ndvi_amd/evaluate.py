"""Test-split evaluation (the reference's ``test/evaluate.py``) with the per-class error metrics computed on the device.

The reference copies every output map to the host, rebuilds the land-cover map from nine dense planes and makes about 40
numpy passes per sample and channel (:188-275).  Here

* the class map is the compact pipeline's ``CompactBatch.cls_a`` (one uint8 per pixel; ``dw_class_map`` derives it from a
  dense input with the reference's rule, :212-217);
* ``eval_metrics`` is ONE launch (``mau_eval_metrics``): per (sample, channel) the overall MAE / RMSE, the variance of
  the 5-point Laplacian of prediction and target, MAE / RMSE / pixel count per class, non-finite counts and min / max --
  fp64 sums in a fixed order, a small fp64 row per (sample, channel);
* ``evaluate_checkpoint`` runs a reference-layout checkpoint over the ``test`` split and writes the reference's
  ``*_evaluation.csv`` and ``*_info.csv`` (:244-310) with the stdlib ``csv`` module.  Only the metric rows cross to the
  host, one copy per batch; the output maps never do.

    python -m mau_amd.evaluate best.pth --processed-dir data/processed --device gpu [--study-name test] [--jobid J]
                               [--precision fp32] [--metrics-json normalization_metrics.json] [--output-dir reports/tests]

No plotting, wandb, pandas or skimage.
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import functional as F_
from .functional import call, lib

log = logging.getLogger(__name__)

# Dynamic World land-cover classes in label order (the reference's DW_CLASSES, src/utils/visualization.py)
DW_CLASS_NAMES = ("water", "trees", "grass", "flooded_vegetation", "crops", "shrub_and_scrub", "built", "bare", "snow_and_ice")
MAX_CLASSES = 16
COLUMNS = ("sample_idx", "channel", "dw_class", "mae", "rmse", "laplacian_var_pred", "laplacian_var_gt", "is_known_city",
           "t1_year", "t1_month", "t2_year", "t2_month", "time_delta", "city", "lat", "lon")
METRICS = ("mae", "rmse", "laplacian_var_pred", "laplacian_var_gt")
GROUP_KEYS = ("is_known_city", "t1_year", "channel", "dw_class", "city", "lat", "lon")        # test/evaluate.py:314
_HEAD = 11                                                                                   # include/mau_hip.h, mau_eval_metrics


# --------------------------------------------------------------------------- #
# the class map of a dense input
# --------------------------------------------------------------------------- #
def dw_class_map(inputs: torch.Tensor, num_classes: int = len(DW_CLASS_NAMES)) -> torch.Tensor:
    """Dense (B, >= num_classes, H, W) input -> (B, H, W) uint8 class map by the reference's rule (test/evaluate.py:212-217):
    ``argmax_c(plane_c * c)``, the first maximum winning.  For a valid one-hot input it equals ``CompactBatch.cls_a``."""
    if inputs.dim() != 4 or inputs.shape[1] < num_classes:
        raise ValueError(f"dw_class_map: expected (B, >= {num_classes}, H, W), got {tuple(inputs.shape)}")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"dw_class_map: num_classes must be in [1, {MAX_CLASSES}]")
    planes = inputs[:, :num_classes]
    code = torch.arange(num_classes, dtype=planes.dtype, device=planes.device).view(1, num_classes, 1, 1)
    weighted = planes * code
    # the first index that reaches the maximum (torch.argmax does not promise which of several equal maxima it returns)
    top = weighted.amax(dim=1, keepdim=True)
    idx = torch.arange(num_classes, device=planes.device).view(1, num_classes, 1, 1).expand_as(weighted)
    first = torch.where(weighted == top, idx, torch.full_like(idx, num_classes)).amin(dim=1)
    return first.to(torch.uint8)


# --------------------------------------------------------------------------- #
# the kernel
# --------------------------------------------------------------------------- #
class EvalMetrics:
    """Result of :func:`eval_metrics`: ``rows`` is the (B, C, row_elems) fp64 device tensor ``mau_eval_metrics`` wrote, the
    properties are views of it -- (B, C) each, the per-class ones (B, C, num_classes)."""

    def __init__(self, rows: torch.Tensor, num_classes: int):
        self.rows, self.num_classes = rows, num_classes

    mae = property(lambda self: self.rows[..., 0])
    rmse = property(lambda self: self.rows[..., 1])
    laplacian_var_pred = property(lambda self: self.rows[..., 2])
    laplacian_var_gt = property(lambda self: self.rows[..., 3])
    nonfinite_pred = property(lambda self: self.rows[..., 4])
    nonfinite_gt = property(lambda self: self.rows[..., 5])
    min_pred = property(lambda self: self.rows[..., 6])
    max_pred = property(lambda self: self.rows[..., 7])
    min_gt = property(lambda self: self.rows[..., 8])
    max_gt = property(lambda self: self.rows[..., 9])
    other_count = property(lambda self: self.rows[..., 10])             # pixels whose class id is >= num_classes
    class_count = property(lambda self: self.rows[..., _HEAD:_HEAD + self.num_classes])
    class_mae = property(lambda self: self.rows[..., _HEAD + self.num_classes:_HEAD + 2 * self.num_classes])
    class_rmse = property(lambda self: self.rows[..., _HEAD + 2 * self.num_classes:_HEAD + 3 * self.num_classes])

    def cpu(self) -> "EvalMetrics":
        return EvalMetrics(self.rows.cpu(), self.num_classes)


def chunks_per_map(H: int, W: int) -> int:
    """Workgroups that share one (H, W) map in ``mau_eval_metrics``: a function of the map's shape alone."""
    return lib.mau_eval_metrics_chunks(H, W)


def _coeffs(v, C: int, dev, what: str, default: float) -> torch.Tensor:
    t = torch.full((C,), default, dtype=torch.float64) if v is None else torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    if t.numel() != C:
        raise ValueError(f"eval_metrics: {what} must hold one value per channel ({C}), got {t.numel()}")
    return t.to(dev).contiguous()


def _checked_args(fn: str, outputs, targets, cls, scale, shift, num_classes: int, max_models: int = 0):
    """The argument check of ``eval_metrics`` and ``statistics.eval_metrics_multi`` (``fn``: the caller's name in the messages):
    outputs, targets fp32 and cls uint8 on the device, targets (B, C, H, W), cls (B, H, W), outputs of targets' shape -- with
    ``max_models`` behind a leading M in [1, max_models] --, ``num_classes`` in range, nothing empty.  Returns the three tensors
    detached and contiguous and scale, shift as (C,) fp64 device tensors."""
    for t, what in ((outputs, "outputs"), (targets, "targets"), (cls, "cls")):
        F_._require_cuda(t, f"{fn}({what})")
    if outputs.dtype != torch.float32 or targets.dtype != torch.float32:
        raise TypeError(f"{fn}: outputs and targets must be float32, got {outputs.dtype} and {targets.dtype}")
    if cls.dtype != torch.uint8:
        raise TypeError(f"{fn}: cls must be uint8, got {cls.dtype}")
    if max_models:
        if outputs.dim() != 5 or targets.dim() != 4 or outputs.shape[1:] != targets.shape:
            raise ValueError(f"{fn}: outputs must be (M, B, C, H, W) and targets (B, C, H, W), got {tuple(outputs.shape)} and {tuple(targets.shape)}")
        if not 1 <= outputs.shape[0] <= max_models:
            raise ValueError(f"{fn}: M must be in [1, {max_models}], got {outputs.shape[0]}")
    elif outputs.dim() != 4 or outputs.shape != targets.shape:
        raise ValueError(f"{fn}: outputs and targets must be (B, C, H, W) of one shape, got {tuple(outputs.shape)} and {tuple(targets.shape)}")
    B, C, H, W = targets.shape
    if tuple(cls.shape) != (B, H, W):
        raise ValueError(f"{fn}: cls must be {(B, H, W)}, got {tuple(cls.shape)}")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{fn}: num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
    if B * C * H * W == 0:
        raise ValueError(f"{fn}: empty batch")
    dev = outputs.device
    return (outputs.detach().contiguous(), targets.detach().contiguous(), cls.contiguous(),
            _coeffs(scale, C, dev, "scale", 1.0), _coeffs(shift, C, dev, "shift", 0.0))


def eval_metrics(outputs: torch.Tensor, targets: torch.Tensor, cls: torch.Tensor, scale=None, shift=None,
                 num_classes: int = len(DW_CLASS_NAMES)) -> EvalMetrics:
    """Per (sample, channel) metrics of ``outputs * scale + shift`` against ``targets * scale + shift`` in one launch.
    outputs, targets (B, C, H, W) fp32 on the device; cls (B, H, W) uint8; scale / shift: one value per channel (None = 1 / 0).
    A row depends on its own maps only: not on B, not on the sample's position; repeated calls agree bit for bit."""
    outputs, targets, cls, scale, shift = _checked_args("eval_metrics", outputs, targets, cls, scale, shift, num_classes)
    B, C, H, W = targets.shape
    dev = outputs.device
    rows = torch.empty((B, C, lib.mau_eval_metrics_row_elems(num_classes)), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.mau_eval_metrics_ws_elems(B, C, H, W, num_classes), dtype=torch.float64, device=dev)
    call("mau_eval_metrics", outputs.data_ptr(), targets.data_ptr(), cls.data_ptr(), scale.data_ptr(), shift.data_ptr(),
         rows.data_ptr(), ws.data_ptr(), F_._tickets(dev).data_ptr(), B, C, H, W, num_classes, F_._stream())
    return EvalMetrics(rows, num_classes)


# --------------------------------------------------------------------------- #
# rows, files, summary (host, plain Python)
# --------------------------------------------------------------------------- #
def metric_rows(m: EvalMetrics, sample_idx0: int, channels: Sequence[str], infos: Sequence[dict],
                class_names: Sequence[str] = DW_CLASS_NAMES) -> List[dict]:
    """The reference's result rows (test/evaluate.py:244-275) of one batch from host-side metrics: per sample and channel an
    ``overall`` row, then one row per class that has pixels.  ``infos[i]``: the sample's remaining columns (is_known_city,
    dates, time_delta, city, lat, lon).  Repeats the reference's log lines about NaNs and constant maps (:226-230)."""
    rows = m.rows.tolist()
    nc = m.num_classes
    out = []
    for i, per_channel in enumerate(rows):
        idx = sample_idx0 + i
        for c, r in enumerate(per_channel):
            ch = channels[c]
            for what, nonfinite, lo, hi in (("Prediction", r[4], r[6], r[7]), ("Ground Truth", r[5], r[8], r[9])):
                if nonfinite:
                    log.error("Non-finite values found in %s for channel %s at sample index %d", what, ch, idx)
                if lo == hi:
                    log.warning("%s have a single unique value for channel %s at sample index %d", what, ch, idx)
            out.append({"sample_idx": idx, "channel": ch, "dw_class": "overall", "mae": r[0], "rmse": r[1],
                        "laplacian_var_pred": r[2], "laplacian_var_gt": r[3], **infos[i]})
            for k in range(nc):
                if r[_HEAD + k] > 0:
                    out.append({"sample_idx": idx, "channel": ch, "dw_class": class_names[k], "mae": r[_HEAD + nc + k],
                                "rmse": r[_HEAD + 2 * nc + k], "laplacian_var_pred": None, "laplacian_var_gt": None, **infos[i]})
    return out


def tag_of(temporal_embeddings: bool, metadata_embeddings: bool) -> str:
    """test/evaluate.py:120-127."""
    return "emb" if temporal_embeddings and metadata_embeddings else "tempemb" if temporal_embeddings \
        else "metaemb" if metadata_embeddings else "noemb"


def report_paths(output_dir: str, study_name: str, model_type: str, tag_emb: str, trial_id, jobid: str):
    """(evaluation csv, info csv), test/evaluate.py:297-302."""
    stem = f"{study_name}_{model_type}_{tag_emb}_{trial_id}_job{jobid}"
    return os.path.join(output_dir, f"{stem}_evaluation.csv"), os.path.join(output_dir, f"{stem}_info.csv")


def _cell(v):
    return "" if v is None else v           # (pandas writes a missing value as an empty field)


def write_reports(rows: Sequence[dict], output_dir: str, study_name: str, model_type: str, tag_emb: str, trial_id, jobid: str = ""):
    """Write ``*_evaluation.csv`` (the reference's columns, in its order) and ``*_info.csv`` (:297-310); returns both paths."""
    os.makedirs(output_dir, exist_ok=True)
    report_path, info_path = report_paths(output_dir, study_name, model_type, tag_emb, trial_id, jobid)
    with open(report_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for r in rows:
            w.writerow([_cell(r[k]) for k in COLUMNS])
    info = {"evaluation_csv_path": report_path, "model_embedding_type": tag_emb, "study_name": study_name,
            "trial_id": trial_id, "model_architecture": model_type}
    with open(info_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(info.keys())
        w.writerow(info.values())
    return report_path, info_path


def summarize(rows: Sequence[dict]) -> List[dict]:
    """Means of the four metrics grouped by (is_known_city, t1_year, channel, dw_class, city, lat, lon), sorted by the group
    key (test/evaluate.py:314).  A metric no row of the group carries stays None; NaNs are left out of a mean, as pandas does."""
    groups: Dict[tuple, List[dict]] = {}
    for r in rows:
        groups.setdefault(tuple(r[k] for k in GROUP_KEYS), []).append(r)
    out = []
    for key in sorted(groups):
        g = dict(zip(GROUP_KEYS, key))
        for mname in METRICS:
            vals = [r[mname] for r in groups[key] if r[mname] is not None and not math.isnan(r[mname])]
            g[mname] = math.fsum(vals) / len(vals) if vals else None
        out.append(g)
    return out


def format_summary(summary: Sequence[dict]) -> str:
    cols = GROUP_KEYS + METRICS
    lines = ["  ".join(cols)]
    for g in summary:
        lines.append("  ".join("" if g[c] is None else f"{g[c]:.6g}" if isinstance(g[c], float) else str(g[c]) for c in cols))
    return "\n".join(lines)


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
def train_cities(processed_dir: str) -> set:
    """City names of the train split's file names (test/evaluate.py:66-79)."""
    train_dir = os.path.join(processed_dir, "train")
    if not os.path.isdir(train_dir):
        log.warning("Training directory not found at %s. Cannot determine known/unknown cities.", train_dir)
        return set()
    return {" ".join(f.split("_")[:-8]) for f in os.listdir(train_dir) if f.endswith(".npz")}


def load_for_evaluation(checkpoint_path: str, study_name: str = "", device: str = "cuda"):
    """(eval-mode model, checkpoint dict) of a reference-layout checkpoint: ``checkpoint.model_kwargs_from_checkpoint``'s
    rules (embedding flags, ``metadata_input_length``), the config's ``temporal_length`` and target channels as
    test/evaluate.py:152-164; input channels and filter width are read off the first convolution's weight."""
    from .checkpoint import EVAL_WIDTHS, load_reference_checkpoint
    from .config import CONFIG
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint not found at: {checkpoint_path}")
    return load_reference_checkpoint(checkpoint_path, CONFIG.dataset.temporal_length, EVAL_WIDTHS, study_name, device)


def temperature_coeffs(channels: Sequence[str], metrics: Optional[dict]):
    """(scale, shift) per channel that un-normalise the temperature channels ("temp" in the name) with the metrics' ``temp_std`` and
    ``temp_mean`` and leave the others -- NDVI -- as they are (get_unnormalized_data, test/evaluate.py:23-41); no metrics: raw values."""
    scale = [float(metrics["temp_std"]) if metrics and "temp" in ch.lower() else 1.0 for ch in channels]
    shift = [float(metrics["temp_mean"]) if metrics and "temp" in ch.lower() else 0.0 for ch in channels]
    return scale, shift


def open_test_split(checkpoint_paths: Sequence[str], processed_dir: str, *, batch_size: Optional[int], precision: Optional[str],
                    study_name: str, metrics_json: Optional[str], device: str):
    """What a walk over the ``test`` split of ``processed_dir`` needs, for one checkpoint or several: (models -- loaded, frozen --,
    their checkpoint dicts, channel names, scale, shift, the train split's cities, the loader).  batch_size: default the first
    checkpoint's ``hyperparameters.batch_size``, else 16.  ``metrics_json``: default ``<processed_dir>/normalization_metrics.json``
    when it exists, else raw values (test/evaluate.py:169-174)."""
    from .config import CONFIG
    from .data import create_dataloader
    models, ckpts = [], []
    for path in checkpoint_paths:
        model, ckpt = load_for_evaluation(path, study_name, device)
        if precision is not None:
            model.set_precision(precision)
        model.eval().freeze_inference()
        models.append(model)
        ckpts.append(ckpt)
    Co = models[0].model.final.weight.shape[0]
    if any(m.model.final.weight.shape[0] != Co for m in models):
        raise ValueError("compare_checkpoints: the checkpoints do not have the same number of output channels")
    bs = int(batch_size if batch_size is not None else ckpts[0].get("hyperparameters", {}).get("batch_size", 16))
    channels = list(CONFIG.dataset.target_channels)
    if len(channels) != Co:
        channels = [f"channel_{i}" for i in range(Co)]
    if metrics_json is None:
        default = os.path.join(processed_dir, "normalization_metrics.json")
        metrics_json = default if os.path.exists(default) else ""
    metrics = None
    if metrics_json:
        with open(metrics_json) as f:
            metrics = json.load(f)
    else:
        log.warning("Normalization metrics not found. Using raw data.")
    scale, shift = temperature_coeffs(channels, metrics)
    known = train_cities(processed_dir)
    # the plain loader: DeviceLoader's 7-tuple drops cls_a, which the metrics need
    loader = create_dataloader("test", bs, False, processed_dir=processed_dir, device=None)
    return models, ckpts, channels, scale, shift, known, loader


def walk_test_split(loader, known: set, device: str):
    """Per batch of the loader: (the host batch, the batch on the device, the index of its first sample, ``infos``) -- ``infos[i]``
    holds the columns of sample i that are not metrics: is_known_city, the dates, time_delta, and city, lat, lon."""
    dataset = loader.dataset
    sample_idx = 0
    for host in loader:
        batch = host.pin().to(device)
        infos = []
        for i in range(int(host.t1_dates.shape[0])):
            t1y, t1m = int(host.t1_dates[i, 0]), int(host.t1_dates[i, 1])
            t2y, t2m = int(host.t2_dates[i, 0]), int(host.t2_dates[i, 1])
            info = dataset.get_metadata_from_idx(sample_idx + i)
            infos.append({"is_known_city": info["city"] in known, "t1_year": t1y, "t1_month": t1m, "t2_year": t2y,
                          "t2_month": t2m, "time_delta": t2y - t1y, **info})
        yield host, batch, sample_idx, infos
        sample_idx += len(infos)


def network_inputs(batch, model, ckpt: dict, packed: dict):
    """(inputs, temp_series, metadata, targets) of one model for a device batch.  ``packed`` caches the packed batch per network
    dtype (one dict per batch); a checkpoint with ``metadata_input_length`` 8 gets the two dates appended to the metadata."""
    from .data import to_network_inputs
    dtype = model.model._rt.dtype
    if dtype not in packed:
        packed[dtype] = to_network_inputs(batch, dtype)
    inputs, metadata, temp_series, _lengths, t1_dates, t2_dates, targets = packed[dtype]
    if ckpt.get("metadata_input_length", 4) == 8:
        metadata = torch.cat([metadata, t1_dates, t2_dates], dim=1)
    return inputs, temp_series, metadata, targets


@torch.no_grad()
def evaluate_checkpoint(checkpoint_path: str, processed_dir: str, *, batch_size: Optional[int] = None,
                        precision: Optional[str] = None, study_name: str = "test", jobid: str = "",
                        output_dir: str = "reports/tests", metrics_json: Optional[str] = None, device: str = "cuda") -> dict:
    """Evaluate a checkpoint on the ``test`` split of ``processed_dir`` (test/evaluate.py:44-324 without plots and wandb).
    Returns {'rows', 'summary', 'report_path', 'info_path'}.  ``metrics_json``: the normalisation metrics (temp_mean,
    temp_std); default ``<processed_dir>/normalization_metrics.json`` when it exists, else raw values (:169-174)."""
    from .checkpoint import resolve_embedding_flags
    (model,), (ckpt,), channels, scale, shift, known, loader = open_test_split(
        [checkpoint_path], processed_dir, batch_size=batch_size, precision=precision, study_name=study_name, metrics_json=metrics_json,
        device=device)
    rows: List[dict] = []
    for _host, batch, sample_idx, infos in walk_test_split(loader, known, device):
        inputs, temp_series, metadata, targets = network_inputs(batch, model, ckpt, {})
        outputs = model(inputs, temp_series, metadata)
        m = eval_metrics(outputs, targets, batch.cls_a, scale, shift, batch.num_classes).cpu()      # the one copy of the batch
        rows += metric_rows(m, sample_idx, channels, infos)
    report_path, info_path = write_reports(rows, output_dir, study_name, ckpt.get("model_type", "unet"),
                                           tag_of(*resolve_embedding_flags(ckpt, study_name)), ckpt.get("trial_id", "unknown"), jobid)
    return {"rows": rows, "summary": summarize(rows), "report_path": report_path, "info_path": info_path}


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.evaluate", description=__doc__.split("\n\n")[0])
    p.add_argument("checkpoint_path", metavar="CHECKPOINT", help="reference-layout .pth (src/train.py:303-316)")
    p.add_argument("--processed-dir", required=True, help="directory that holds the train/ and test/ splits")
    p.add_argument("--device", default="gpu", help="'gpu' or a torch device name; this path has no CPU fallback")
    p.add_argument("--study-name", default="test")
    p.add_argument("--jobid", default="")
    p.add_argument("--batch-size", type=int, default=None, help="default: the checkpoint's hyperparameters.batch_size, else 16")
    p.add_argument("--precision", default=None, choices=["bf16", "fp16", "fp32"])
    p.add_argument("--metrics-json", default=None, help="normalization_metrics.json (default: the one in --processed-dir, if any)")
    p.add_argument("--output-dir", default="reports/tests")
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s")
    device = F_.argparse_device(p, a.device)
    res = evaluate_checkpoint(a.checkpoint_path, a.processed_dir, batch_size=a.batch_size, precision=a.precision,
                              study_name=a.study_name, jobid=a.jobid, output_dir=a.output_dir, metrics_json=a.metrics_json,
                              device=device)
    print(f"Full evaluation report saved to {res['report_path']}")
    print(f"Evaluation info saved to {res['info_path']}")
    for title, flag in (("--- Known Cities (seen in training) ---", True), ("--- Unknown Cities (not seen in training) ---", False)):
        part = [g for g in res["summary"] if g["is_known_city"] is flag]
        if part:
            print(title)
            print(format_summary(part))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
