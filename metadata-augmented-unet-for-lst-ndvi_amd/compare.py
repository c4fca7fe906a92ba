"""Model comparison sessions: several checkpoints on one tile, their error maps and colour ranges on the device (the reference's
developer app, ``app_dev/pages/1_Model_Comparison.py`` with ``app_dev/app_src/utils.py:170-271``).

The page runs every selected model on the CPU over a dense 23-plane input, copies each output to numpy, un-normalises it,
subtracts the target and takes, for the whole tile and for each of its four quadrants, the colour range of ground truth and
prediction and the symmetric range of the error.  Here

* ``mau_compare_result`` is ONE launch for all M models: un-normalised predictions and target, the error maps and a small fp64
  row per (model, channel) with, per region, pixel count, gt / pred min and max, max |err|, sum |err| and sum err^2 (fixed
  summation order, no float atomics);
* ``mau_compare_inputs`` is ONE launch per tile: the page's views of the compact input sample (RGB bytes, temperature in
  degrees C, NDVI, the two class maps through the palette);
* ``ComparisonSession`` packs the tile once for all models and captures pack -> M networks -> result into one hipGraph, a
  single chain on one stream: a replay costs no host copy, and what the page draws is read back in one piece.

The host twins (pure numpy) spell the page's own arithmetic; the device path is tested against them bit for bit.

    python -m mau_amd.compare CKPT [CKPT ...] --processed-dir D [--split test] (--index I | --filename F) --metrics-json M
                              --palette-json P [--precision fp16] [--output out.npz]
"""
from __future__ import annotations

import argparse
import json
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from ._capture import freeze, warm_up_and_capture
from ._tile import N_CONT, check_metrics, check_ncls, check_palette, norm_row
from .functional import _dev, call, lib
from .scenario import palette_from_hex
REGIONS = ("tile", "top_left", "top_right", "bottom_left", "bottom_right")
ENTRIES = ("count", "gt_min", "gt_max", "pred_min", "pred_max", "max_abs_err", "sum_abs_err", "sum_sq_err")
VIEW_NAMES = ("rgb8", "temp_c", "ndvi", "dw_t1_rgb", "dw_t2_rgb")
CHANNEL_NAMES = ("ndvi", "temp")
SAMPLE_KEYS = ("cls_a", "cls_b", "cont", "metadata", "temp_series", "t1_date", "t2_date", "target")


# --------------------------------------------------------------------------- #
# host twins (numpy): the page's path, in its own arithmetic
# --------------------------------------------------------------------------- #
def quadrants(H: int, W: int) -> Tuple[Tuple[int, int, int, int], ...]:
    """(y1, y2, x1, x2) of top-left, top-right, bottom-left, bottom-right (utils.py:173-178)."""
    return ((0, H // 2, 0, W // 2), (0, H // 2, W // 2, W), (H // 2, H, 0, W // 2), (H // 2, H, W // 2, W))


def _region_entries(g: np.ndarray, p: np.ndarray, e: np.ndarray) -> np.ndarray:
    """The eight entries of one region from its float32 ground truth, prediction and error."""
    a = np.abs(e)
    e64 = e.astype(np.float64).ravel()
    return np.array([g.size,
                     np.fmin.reduce(g.ravel(), initial=np.inf), np.fmax.reduce(g.ravel(), initial=-np.inf),
                     np.fmin.reduce(p.ravel(), initial=np.inf), np.fmax.reduce(p.ravel(), initial=-np.inf),
                     np.fmax.reduce(a.ravel(), initial=0.0), a.astype(np.float64).sum(), (e64 * e64).sum()], dtype=np.float64)


def join_entries(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Two regions' entries joined: counts and sums add, minima and maxima combine (a NaN is skipped by both)."""
    return np.array([a[0] + b[0], np.fmin(a[1], b[1]), np.fmax(a[2], b[2]), np.fmin(a[3], b[3]), np.fmax(a[4], b[4]),
                     np.fmax(a[5], b[5]), a[6] + b[6], a[7] + b[7]], dtype=np.float64)


def compare_host(outputs, target, metrics: dict):
    """outputs (M, 2, H, W), target (2, H, W), float32 and normalised -> (pred (M,2,H,W), gt (2,H,W), err (M,2,H,W), float32;
    rows (M * 2, 40) float64) as ``mau_compare_result`` lays them out.  The temperature channel is ``x * temp_std + temp_mean`` on
    a float32 array with Python-float scalars (utils.py:260-261), the error ``pred - gt`` (1_Model_Comparison.py:146); minima and
    maxima skip a NaN, the float64 sums carry it; the whole-tile entries are ((TL o TR) o BL) o BR."""
    check_metrics(metrics, ("temp_mean", "temp_std"))
    outputs, target = np.asarray(outputs, dtype=np.float32), np.asarray(target, dtype=np.float32)
    if outputs.ndim != 4 or outputs.shape[1] != 2 or outputs.shape[0] < 1 or target.shape != outputs.shape[1:]:
        raise ValueError(f"compare_host: outputs must be (M, 2, H, W) and target (2, H, W), got {outputs.shape} and {target.shape}")
    mean, std = float(metrics["temp_mean"]), float(metrics["temp_std"])
    pred, gt = outputs.copy(), target.copy()
    pred[:, 1] = outputs[:, 1] * std + mean
    gt[1] = target[1] * std + mean
    err = pred - gt[None]
    M, _, H, W = outputs.shape
    rows = np.empty((M * 2, len(REGIONS), len(ENTRIES)), dtype=np.float64)
    for m in range(M):
        for c in range(2):
            quads = [_region_entries(gt[c, y1:y2, x1:x2], pred[m, c, y1:y2, x1:x2], err[m, c, y1:y2, x1:x2])
                     for y1, y2, x1, x2 in quadrants(H, W)]
            rows[m * 2 + c, 0] = join_entries(join_entries(join_entries(quads[0], quads[1]), quads[2]), quads[3])
            rows[m * 2 + c, 1:] = quads
    return pred, gt, err, rows.reshape(M * 2, -1)


def input_views_host(cls_a, cls_b, cont, palette, metrics: dict) -> dict:
    """The page's views of a compact sample (utils.py:224-252): ``rgb8`` (H,W,3) uint8, ``temp_c`` and ``ndvi`` (H,W) float32,
    ``dw_t1_rgb`` and ``dw_t2_rgb`` (H,W,3) uint8.  The colour planes go through float64 (a float32 array times a float64 array),
    are clipped to [0, 255] and truncated; a NaN gives 0; a class id outside the palette gives black."""
    check_metrics(metrics, ("rgb_mean", "rgb_std", "temp_mean", "temp_std"))
    palette = check_palette(palette)
    cont = np.asarray(cont, dtype=np.float32)
    cls_a, cls_b = np.asarray(cls_a), np.asarray(cls_b)
    if cont.ndim != 3 or cont.shape[0] != N_CONT or cls_a.shape != cont.shape[1:] or cls_b.shape != cont.shape[1:]:
        raise ValueError(f"input_views_host: cont must be (5, H, W) and the class maps (H, W), got {cont.shape}, {cls_a.shape}, {cls_b.shape}")
    std, mean = np.array(metrics["rgb_std"], dtype=np.float64), np.array(metrics["rgb_mean"], dtype=np.float64)
    if std.shape != (3,) or mean.shape != (3,):
        raise ValueError("metrics: rgb_mean and rgb_std hold three values each")
    rgb = (cont[:3] * std[:, None, None] + mean[:, None, None]) * 255.0
    rgb = np.clip(rgb.transpose(1, 2, 0), 0, 255)
    rgb8 = np.where(np.isnan(rgb), 0.0, rgb).astype(np.uint8)
    table = np.zeros((256, 3), dtype=np.uint8)
    table[:palette.shape[0]] = palette
    return {"rgb8": rgb8, "temp_c": cont[4] * float(metrics["temp_std"]) + float(metrics["temp_mean"]), "ndvi": cont[3].copy(),
            "dw_t1_rgb": table[cls_a.astype(np.int64)], "dw_t2_rgb": table[cls_b.astype(np.int64)]}


# --------------------------------------------------------------------------- #
# the two launches
# --------------------------------------------------------------------------- #
class ComparisonStats:
    """The (M * 2, 40) fp64 rows of ``mau_compare_result`` with names: ``table`` is the (M, 2, 5, 8) view [model, channel,
    region, entry]; ``region('top_left')`` is (M, 2, 8); an entry by name (``count``, ``gt_min``, ``gt_max``, ``pred_min``,
    ``pred_max``, ``max_abs_err``, ``sum_abs_err``, ``sum_sq_err``) is (M, 2, 5).  Derived, (M, 2, 5) each: ``vmin``, ``vmax`` and
    ``err_max_abs`` -- the colour ranges the page passes to ``imshow`` -- and ``mae``, ``rmse``."""

    def __init__(self, rows: torch.Tensor):
        self.rows = rows
        self.table = rows.view(-1, 2, len(REGIONS), len(ENTRIES))

    def region(self, name: str) -> torch.Tensor:
        return self.table[:, :, REGIONS.index(name)]

    def entry(self, name: str) -> torch.Tensor:
        return self.table[..., ENTRIES.index(name)]

    def __getattr__(self, name):
        if name in ENTRIES:
            return self.entry(name)
        raise AttributeError(name)

    @property
    def vmin(self):
        return torch.minimum(self.gt_min, self.pred_min)

    @property
    def vmax(self):
        return torch.maximum(self.gt_max, self.pred_max)

    @property
    def err_max_abs(self):
        """max |err|, and 1 where that is 0 (utils.py:187)."""
        e = self.max_abs_err
        return torch.where(e > 0, e, torch.ones_like(e))

    @property
    def mae(self):
        return self.sum_abs_err / self.count

    @property
    def rmse(self):
        return torch.sqrt(self.sum_sq_err / self.count)

    def clone(self) -> "ComparisonStats":
        return ComparisonStats(self.rows.clone())

    def cpu(self) -> "ComparisonStats":
        return ComparisonStats(self.rows.cpu())

    def numpy(self) -> np.ndarray:
        return self.table.cpu().numpy()


class ComparisonResult:
    """What ``mau_compare_result`` wrote: ``pred`` (M,2,H,W), ``gt`` (2,H,W), ``err`` (M,2,H,W) fp32 and ``stats``
    (:class:`ComparisonStats`), all on the device.  A session adds ``names`` (the models') and ``views`` (:class:`InputViews`)."""

    def __init__(self, pred, gt, err, stats: ComparisonStats, names: Optional[Sequence[str]] = None, views=None):
        self.pred, self.gt, self.err, self.stats, self.names, self.views = pred, gt, err, stats, names, views

    def clone(self) -> "ComparisonResult":
        return ComparisonResult(self.pred.clone(), self.gt.clone(), self.err.clone(), self.stats.clone(), self.names, self.views)


class InputViews(NamedTuple):
    rgb8: torch.Tensor          # (H, W, 3) uint8
    temp_c: torch.Tensor        # (H, W) fp32, degrees C
    ndvi: torch.Tensor          # (H, W) fp32
    dw_t1_rgb: torch.Tensor     # (H, W, 3) uint8
    dw_t2_rgb: torch.Tensor     # (H, W, 3) uint8


def result(outputs: torch.Tensor, target: torch.Tensor, temp_mean: float, temp_std: float,
           tickets: Optional[torch.Tensor] = None) -> ComparisonResult:
    """One launch (``mau_compare_result``) per ``mau_reduce_tickets_elems()`` rows: the M heads' outputs (M, 2, H, W) fp32 and
    the normalised target (2, H, W) -> :class:`ComparisonResult`.  A (model, channel) row depends on that model's plane and the
    target's alone: not on M, not on the model's place; repeated calls agree bit for bit."""
    outputs = _dev(outputs, "outputs", torch.float32)
    if outputs.dim() != 4 or outputs.shape[1] != 2 or outputs.numel() == 0:
        raise ValueError(f"outputs must be (M, 2, H, W), M, H, W >= 1, got {tuple(outputs.shape)}")
    M, _, H, W = outputs.shape
    target = _dev(target, "target", torch.float32, (2, H, W))
    dev = outputs.device
    pred, err, gt = torch.empty_like(outputs), torch.empty_like(outputs), torch.empty_like(target)
    rows = torch.empty((M * 2, lib.mau_compare_row_elems()), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.mau_compare_ws_elems(M, H, W), dtype=torch.float64, device=dev)
    tickets = F_._tickets(dev) if tickets is None else tickets
    call("mau_compare_result", outputs.data_ptr(), target.data_ptr(), float(temp_mean), float(temp_std), pred.data_ptr(), gt.data_ptr(),
         err.data_ptr(), rows.data_ptr(), ws.data_ptr(), tickets.data_ptr(), M, H, W, F_._stream())
    return ComparisonResult(pred, gt, err, ComparisonStats(rows))


class _ViewTables:
    """The device-side constants of ``mau_compare_inputs`` for one (palette, metrics)."""

    def __init__(self, palette, metrics: dict, dev):
        check_metrics(metrics)
        palette = check_palette(palette)
        self.ncls = check_ncls(palette.shape[0], "mau_compare_inputs")
        self.palette = torch.from_numpy(palette).to(dev)
        self.norm = torch.from_numpy(norm_row(metrics)).to(dev)


def _input_views(cls_a, cls_b, cont, tb: _ViewTables, out: Optional[InputViews] = None) -> InputViews:
    H, W = cls_a.shape
    dev = cls_a.device
    if out is None:
        out = InputViews(torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev),
                         torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W, 3), dtype=torch.uint8, device=dev),
                         torch.empty((H, W, 3), dtype=torch.uint8, device=dev))
    call("mau_compare_inputs", cls_a.data_ptr(), cls_b.data_ptr(), cont.data_ptr(), tb.palette.data_ptr(), tb.norm.data_ptr(),
         out.rgb8.data_ptr(), out.temp_c.data_ptr(), out.ndvi.data_ptr(), out.dw_t1_rgb.data_ptr(), out.dw_t2_rgb.data_ptr(), H, W, tb.ncls,
         F_._stream())
    return out


def input_views(cls_a: torch.Tensor, cls_b: torch.Tensor, cont: torch.Tensor, palette, metrics: dict) -> InputViews:
    """One launch (``mau_compare_inputs``): a compact sample on the device -- cls_a, cls_b (H, W) uint8, cont (5, H, W) fp32
    normalised -- -> :class:`InputViews`.  palette (ncls, 3) uint8 and the metrics dict are host values."""
    cls_a = _dev(cls_a, "cls_a", torch.uint8)
    if cls_a.dim() != 2 or cls_a.numel() == 0:
        raise ValueError(f"cls_a must be (H, W), got {tuple(cls_a.shape)}")
    H, W = cls_a.shape
    cls_b = _dev(cls_b, "cls_b", torch.uint8, (H, W))
    cont = _dev(cont, "cont", torch.float32, (N_CONT, H, W))
    return _input_views(cls_a, cls_b, cont, _ViewTables(palette, metrics, cls_a.device))


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
def _meta_features(model: torch.nn.Module) -> int:
    net = getattr(model, "model", model)
    return int(net.meta_encoder.fc[0].in_features)


class ComparisonSession:
    """``ComparisonSession(models, sample, metrics=..., palette=..., precision=...)() -> ComparisonResult``.

    ``models`` is a list of ``(name, UrbanPredictor)`` on the device -- ``unet`` and ``unet++`` may be mixed, and so may
    checkpoints with 4 and with 8 metadata features; ``sample`` is one compact sample of ``FuturePredictionDataset`` (cls_a, cls_b,
    cont, metadata, temp_series, t1_date, t2_date, target; host or device tensors); ``metrics`` a dict with the keys of
    ``normalization_metrics.json``; ``palette`` the (ncls, 3) uint8 colour table in class order (None: no input views);
    ``precision`` is set on every model (None: as they are -- they must then compute in one type, the tile is packed once).

    The session moves the sample to the device once, freezes every model (``freeze_inference``), warms up on a side stream and
    captures ONE hipGraph, a single chain of launches on one stream without forks: ``mau_pack_tile_onehot`` once for all models,
    then each network in turn, its head's output copied into slice m of one (M, 2, H, W) buffer, then one ``mau_compare_result``.
    The tickets of the captured reduction are the session's own.  ``session()`` replays and returns the result;
    ``session.set_sample(other)`` copies a sample of the same shapes into the session's buffers and replays -- the tile is
    re-packed by the replay, nothing is captured again; a sample of another shape raises ``ValueError``.  ``clone_output=False``
    returns the session's own buffers, valid until the next replay.  Reload weights -> build a new session.

    Metadata: every model gets the row its checkpoint asks for -- the sample's 4 values, or those followed by the two dates
    when its metadata encoder takes 8.  The reference page concatenates the dates onto the SHARED tensor inside its loop over
    the models (1_Model_Comparison.py:82-83), so the second 8-feature model of a selection would be handed 12 values and a
    4-feature model after an 8-feature one 8; that is a defect of the page and is not reproduced here."""

    def __init__(self, models: Sequence[Tuple[str, torch.nn.Module]], sample: dict, *, metrics: dict, palette=None,
                 precision: Optional[str] = None, num_classes: Optional[int] = None, warmup: int = 2, clone_output: bool = True):
        from .data import NUM_CLASSES
        models = list(models)
        if not models:
            raise ValueError("ComparisonSession: at least one model")
        check_metrics(metrics, ("temp_mean", "temp_std"))
        self.names = [str(name) for name, _ in models]
        self.models = [model for _, model in models]
        self.clone_output = clone_output
        self.num_classes = int(num_classes if num_classes is not None else NUM_CLASSES)
        dev = next(self.models[0].parameters()).device
        dtypes = set()
        for name, model in zip(self.names, self.models):
            F_._require_cuda(next(model.parameters()), f"ComparisonSession(model {name!r})")
            if precision is not None:
                model.set_precision(precision)
            dtypes.add(freeze(model))
        if len(dtypes) != 1:
            raise ValueError(f"ComparisonSession: the models compute in {sorted(str(d) for d in dtypes)}; the tile is packed once, "
                             "pass precision= or set one precision on all of them")
        self.dtype = dtypes.pop()
        self._n_meta = [_meta_features(m) for m in self.models]
        for name, n in zip(self.names, self._n_meta):
            if n not in (4, 8):
                raise ValueError(f"ComparisonSession: model {name!r} takes {n} metadata features; 4, or 4 plus the two dates, are known")
        self._mean, self._std = float(metrics["temp_mean"]), float(metrics["temp_std"])
        host = self._checked(sample)
        self._buf = {k: v.to(dev) for k, v in host.items()}
        H, W = self._buf["cls_a"].shape[1:]
        self._outs = torch.zeros((len(self.models), 2, H, W), dtype=torch.float32, device=dev)
        self._tables = None if palette is None else _ViewTables(palette, metrics, dev)
        self.views = None if self._tables is None else _input_views(self._buf["cls_a"][0], self._buf["cls_b"][0], self._buf["cont"][0], self._tables)
        # the tickets of the captured reduction are the session's own: a replay never shares them with a launch on another stream
        self._tickets = torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device=dev)
        self.graph, self._out = warm_up_and_capture(self._run, dev, warmup)
        self._out.names, self._out.views = self.names, self.views

    @staticmethod
    def _rows(sample: dict) -> dict:
        """The sample's tensors in the shapes the session keeps (host or device, not copied)."""
        missing = [k for k in SAMPLE_KEYS if k not in sample]
        if missing:
            raise ValueError(f"ComparisonSession: the sample lacks {missing} (a compact sample of FuturePredictionDataset)")
        t = {k: torch.as_tensor(sample[k]) for k in SAMPLE_KEYS}
        md4 = t["metadata"].float().reshape(1, -1)
        dates = torch.cat([t["t1_date"].float().reshape(1, -1).to(md4.device), t["t2_date"].float().reshape(1, -1).to(md4.device)], dim=1)
        return {"cls_a": t["cls_a"][None], "cls_b": t["cls_b"][None], "cont": t["cont"][None], "md4": md4,
                "md8": torch.cat([md4, dates], dim=1), "ts": t["temp_series"].float().reshape(1, -1), "target": t["target"]}

    def _checked(self, sample: dict) -> dict:
        r = self._rows(sample)
        if r["cls_a"].dim() != 3 or r["cls_a"].numel() == 0:
            raise ValueError(f"ComparisonSession: cls_a must be (H, W), got {tuple(r['cls_a'].shape[1:])}")
        _, H, W = r["cls_a"].shape
        want = {"cls_a": ((1, H, W), torch.uint8), "cls_b": ((1, H, W), torch.uint8), "cont": ((1, N_CONT, H, W), torch.float32),
                "md4": ((1, 4), torch.float32), "md8": ((1, 8), torch.float32), "target": ((2, H, W), torch.float32)}
        for k, (shape, dtype) in want.items():
            if tuple(r[k].shape) != shape or r[k].dtype != dtype:
                raise ValueError(f"ComparisonSession: the sample's {k} must be {shape} {dtype}, got {tuple(r[k].shape)} {r[k].dtype}")
        if r["ts"].shape[1] < 1:
            raise ValueError("ComparisonSession: the sample's temperature series is empty")
        return r

    def _run(self) -> ComparisonResult:
        from .data import pack_tiles
        b = self._buf
        x = pack_tiles(b["cls_a"], b["cls_b"], b["cont"], None, self.dtype, self.num_classes)
        for m, (model, n_meta) in enumerate(zip(self.models, self._n_meta)):
            out = model(x, b["ts"], b["md8"] if n_meta == 8 else b["md4"])
            if tuple(out.shape) != (1,) + tuple(self._outs.shape[1:]):
                raise ValueError(f"ComparisonSession: model {self.names[m]!r} returned {tuple(out.shape)}, expected {(1,) + tuple(self._outs.shape[1:])}")
            self._outs[m].copy_(out[0])
        return result(self._outs, b["target"], self._mean, self._std, self._tickets)

    @torch.no_grad()
    def __call__(self) -> ComparisonResult:
        self.graph.replay()
        return self._out.clone() if self.clone_output else self._out

    @torch.no_grad()
    def set_sample(self, sample: dict) -> ComparisonResult:
        """Another tile of the same shapes: copied into the session's buffers, input views renewed, one replay."""
        new = self._rows(sample)
        for k, buf in self._buf.items():
            if tuple(new[k].shape) != tuple(buf.shape) or new[k].dtype != buf.dtype:
                raise ValueError(f"ComparisonSession was captured for a sample whose {k} is {tuple(buf.shape)} {buf.dtype}, "
                                 f"got {tuple(new[k].shape)} {new[k].dtype}")
        for k, buf in self._buf.items():
            buf.copy_(new[k])
        if self._tables is not None:
            _input_views(self._buf["cls_a"][0], self._buf["cls_b"][0], self._buf["cont"][0], self._tables, self.views)
        return self()


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def compare_checkpoints(checkpoints: Sequence[str], processed_dir: str, *, split: str = "test", index: Optional[int] = None,
                        filename: Optional[str] = None, metrics_json: str, palette_json: str, precision: Optional[str] = "fp16",
                        output: str = "", device: str = "cuda") -> dict:
    """Body of the CLI: the checkpoints (loaded as ``mau_amd.evaluate`` loads them) on one tile of ``processed_dir/split``, chosen by
    ``index`` or by ``filename``.  Returns -- and with ``output`` writes as .npz -- pred, gt, err, stats (M, 2, 5, 8), names and the
    five input views; the returned dict also carries ``lines``, one per model and channel."""
    from .data import FuturePredictionDataset
    from .evaluate import load_for_evaluation
    if not checkpoints:
        raise ValueError("compare_checkpoints: at least one checkpoint")
    if (index is None) == (filename is None):
        raise ValueError("compare_checkpoints: give either index or filename")
    with open(palette_json) as f:
        palette = palette_from_hex(json.load(f))
    with open(metrics_json) as f:
        metrics = json.load(f)
    dataset = FuturePredictionDataset(split, processed_dir=processed_dir)
    if filename is not None:
        names = [os.path.basename(p) for p in dataset.file_list]
        if os.path.basename(filename) not in names:
            raise ValueError(f"compare_checkpoints: no tile {filename!r} in {dataset.data_dir}")
        index = names.index(os.path.basename(filename))
    if not 0 <= index < len(dataset):
        raise ValueError(f"compare_checkpoints: index {index} outside the split's {len(dataset)} tiles")
    models = []
    for path in checkpoints:
        model, _ckpt = load_for_evaluation(path, device=device)
        name, k = os.path.basename(path), 2
        while name in [n for n, _ in models]:              # the page keys its models by file name; keep two of one name apart
            name, k = f"{os.path.basename(path)}#{k}", k + 1
        models.append((name, model))
    sess = ComparisonSession(models, dataset[index], metrics=metrics, palette=palette, precision=precision, clone_output=False)
    r = sess()
    stats = r.stats.cpu()
    res = {"pred": r.pred.cpu().numpy(), "gt": r.gt.cpu().numpy(), "err": r.err.cpu().numpy(), "stats": stats.numpy(),
           "names": np.array(sess.names), "tile": np.array(os.path.basename(dataset.file_list[index])),
           **{k: v.cpu().numpy() for k, v in r.views._asdict().items()}}
    if output:
        np.savez(output, **res)
    lines = []
    for m, name in enumerate(sess.names):
        for c, ch in enumerate(CHANNEL_NAMES):
            lines.append(f"{name} {ch}: mae {float(stats.mae[m, c, 0]):.6g} rmse {float(stats.rmse[m, c, 0]):.6g} "
                         f"vmin {float(stats.vmin[m, c, 0]):.6g} vmax {float(stats.vmax[m, c, 0]):.6g} "
                         f"err_max_abs {float(stats.err_max_abs[m, c, 0]):.6g}")
    res["lines"] = lines
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.compare", description=__doc__.split("\n\n")[0])
    p.add_argument("checkpoints", metavar="CKPT", nargs="+", help="reference-layout .pth files (src/train.py:303-316)")
    p.add_argument("--processed-dir", required=True, help="directory that holds the splits")
    p.add_argument("--split", default="test")
    which = p.add_mutually_exclusive_group(required=True)
    which.add_argument("--index", type=int, default=None, help="the tile's index in the split (sorted file names)")
    which.add_argument("--filename", default=None, help="the tile's file name")
    p.add_argument("--metrics-json", required=True, help="normalization_metrics.json")
    p.add_argument("--palette-json", required=True, help="the palette's hex colours in class order")
    p.add_argument("--precision", default="fp16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--output", default="", help=".npz to write pred, gt, err, stats, names and the input views to")
    p.add_argument("--device", default="gpu", help="'gpu' or a torch device name; this path has no CPU fallback")
    a = p.parse_args(argv)
    device = F_.argparse_device(p, a.device)
    res = compare_checkpoints(a.checkpoints, a.processed_dir, split=a.split, index=a.index, filename=a.filename, metrics_json=a.metrics_json,
                              palette_json=a.palette_json, precision=a.precision, output=a.output, device=device)
    for line in res["lines"]:
        print(line)
    if a.output:
        print(f"Saved comparison to {a.output}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
