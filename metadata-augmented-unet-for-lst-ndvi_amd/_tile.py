"""What the tools around one resident tile or region share (``scenario``, ``placement``, ``region``; the checks also serve ``compare``):
the checks of the tile, the palette, the metrics, the class count and the channel stride, the small device constants, the upload of
a call's input into a session buffer, and the sessions' base class.  Nothing here launches a kernel; capturing is ``_capture.py``'s."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import functional as F_
from ._capture import PinnedStage, freeze, warm_up_and_capture
from .functional import _dev, lib, pad8

N_CONT = 5               # rgb (3) + ndvi + temperature
METRIC_KEYS = ("rgb_mean", "rgb_std", "temp_mean", "temp_std", "meta_mean", "meta_std", "temp_series_mean", "temp_series_std")


def check_palette(palette) -> np.ndarray:
    p = np.asarray(palette)
    if p.ndim != 2 or p.shape[1] != 3 or p.dtype != np.uint8 or p.shape[0] < 1:
        raise ValueError("palette must be an (ncls, 3) uint8 array, ncls >= 1")
    return np.ascontiguousarray(p)


def check_metrics(metrics: dict, keys=METRIC_KEYS[:4]):
    missing = [k for k in keys if k not in metrics]
    if missing:
        raise ValueError(f"metrics lacks {missing} (the keys of normalization_metrics.json)")


def norm_row(metrics: dict) -> np.ndarray:
    """The eight fp64 values the pack kernels normalise with: rgb_mean, rgb_std, temp_mean, temp_std."""
    check_metrics(metrics)
    row = np.array(list(metrics["rgb_mean"]) + list(metrics["rgb_std"]) + [metrics["temp_mean"], metrics["temp_std"]], dtype=np.float64)
    if row.shape != (8,):
        raise ValueError("metrics: rgb_mean and rgb_std hold three values each")
    return row


def check_ncls(ncls: int, kernel: str) -> int:
    ncls = int(ncls)
    if not 1 <= ncls <= lib.mau_scenario_max_classes():
        raise ValueError(f"{kernel} takes 1 to {lib.mau_scenario_max_classes()} classes, got {ncls}")
    return ncls


def check_ld(ld: Optional[int], C: int, who: str) -> int:
    """The channel stride of a packed input of ``C`` channels: ``C`` rounded up to 8 by default, a multiple of 8 and at least ``C``."""
    ld = pad8(C) if ld is None else int(ld)
    if ld % 8 or ld < C:
        raise ValueError(f"{who}: ld must be a multiple of 8 and at least {C}, got {ld}")
    return ld


def const(v, dtype, dev) -> torch.Tensor:
    """A small host array (or device tensor) as a contiguous device tensor."""
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(dev)


def check_tile(dw_t1, rgb, ndvi, temp):
    """The base tile, checked: dw_t1 (H,W) uint8, rgb (3,H,W), ndvi (H,W) | (1,H,W), temp likewise, fp32, on the device."""
    dw_t1 = _dev(dw_t1, "dw_t1", torch.uint8)
    if dw_t1.dim() == 3 and dw_t1.shape[0] == 1:
        dw_t1 = dw_t1[0]
    if dw_t1.dim() != 2:
        raise ValueError(f"dw_t1 must be (H, W), got {tuple(dw_t1.shape)}")
    H, W = dw_t1.shape
    rgb = _dev(rgb, "rgb", torch.float32, (3, H, W))
    ndvi = _dev(ndvi.reshape(H, W) if isinstance(ndvi, torch.Tensor) and ndvi.numel() == H * W else ndvi, "ndvi", torch.float32, (H, W))
    temp = _dev(temp.reshape(H, W) if isinstance(temp, torch.Tensor) and temp.numel() == H * W else temp, "temp", torch.float32, (H, W))
    return dw_t1, rgb, ndvi, temp


def upload(src, dst: torch.Tensor, stage: PinnedStage, what: str) -> None:
    """A call's input into the session buffer ``dst``: a device tensor is copied device to device (not at all when it IS ``dst``),
    a host tensor or array travels through the pinned ``stage``.  Another shape is a ValueError, another element type a TypeError."""
    src = src if isinstance(src, torch.Tensor) else np.asarray(src)
    if tuple(src.shape) != tuple(dst.shape):
        raise ValueError(f"the session was built for a {what} of shape {tuple(dst.shape)}, got {tuple(src.shape)}")
    if str(src.dtype).replace("torch.", "") != str(dst.dtype).replace("torch.", ""):
        raise TypeError(f"{what} must be {dst.dtype}, got {src.dtype}")
    if isinstance(src, torch.Tensor) and src.is_cuda:
        if src.data_ptr() != dst.data_ptr():
            dst.copy_(src, non_blocking=True)
    else:
        stage.upload(src, dst)


class TileSession:
    """What ``ScenarioSession``, ``PlacementSession`` and ``RegionSession`` do alike.  The constructor checks the tile, ``metadata``,
    ``temp_series`` and ``metrics``, sets ``precision`` (None: the model's own), freezes the model, clones the tile and the optional
    (H, W) planes ``dw_t2``, ``roi`` and ``temp_orig`` (None = ``temp``), uploads the normalisation row and expands ``metadata`` and
    ``temp_series`` to ``batch`` samples.  A subclass then allocates its own buffers and calls ``_capture()``: ``_run()`` warmed up and
    captured into one hipGraph (``graph=False``: run once, eagerly).  ``self._out`` is what ``_run()`` returned; ``_replay()`` runs it
    again.  ``_fit(H, W)``, a subclass's own checks against the tile's shape, runs before the model is touched."""

    def __init__(self, model: torch.nn.Module, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics: dict, batch: int, *,
                 precision: Optional[str] = None, dw_t2=None, roi=None, temp_orig=None):
        tile = check_tile(dw_t1, rgb, ndvi, temp)
        for t, what in ((metadata, "metadata"), (temp_series, "temp_series")):
            F_._require_cuda(t, f"{type(self).__name__}({what})")
        check_metrics(metrics)
        self.shape, self.batch, self._device = tuple(tile[0].shape), int(batch), tile[0].device
        self._fit(*self.shape)
        if precision is not None:
            model.set_precision(precision)
        self.model = model
        self.dtype = freeze(model)
        self._tile = tuple(t.detach().clone() for t in tile)
        plane = lambda t, what, dtype: None if t is None else _dev(t, what, dtype, self.shape).detach().clone()      # noqa: E731
        self._dw_t2, self._roi = plane(dw_t2, "dw_t2", torch.uint8), plane(roi, "roi", torch.uint8)
        self._temp_orig = self._tile[3] if temp_orig is None else plane(temp_orig, "temp_orig", torch.float32)
        self._norm = const(norm_row(metrics), torch.float64, self._device)
        self._mean, self._std = float(metrics["temp_mean"]), float(metrics["temp_std"])
        self._md = self._metadata(metadata.detach().float())
        self._ts = temp_series.detach().float().reshape(1, -1).expand(self.batch, -1).contiguous()

    def _fit(self, H: int, W: int) -> None:
        pass

    def _metadata(self, md: torch.Tensor) -> torch.Tensor:
        """The (batch, F) metadata input of a run: the tile's one row for every sample."""
        return md.reshape(1, -1).expand(self.batch, -1).contiguous()

    def _own_tickets(self) -> torch.Tensor:
        """Tickets for a reduction inside the captured graph: a replay never shares them with a launch on another stream."""
        return torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device=self._device)

    def _capture(self, warmup: int = 2, graph: bool = True) -> None:
        self.graph = None
        if graph:
            self.graph, self._out = warm_up_and_capture(self._run, self._device, warmup)
        else:
            self._replay()

    def _replay(self) -> None:
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._out = self._run()
