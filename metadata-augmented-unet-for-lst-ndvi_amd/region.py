"""Region forecasts: a raster larger than one tile, at the resolution the network was trained at, on the device.

The reference resizes whatever region the user draws to ``model.img_size`` = 512 before the network sees it
(app/gee_utils.py:40-87, app/processing_utils.py:122-128): a 40 km city becomes 80 m pixels.  Here the region stays resident on
the device at its own resolution and goes through the network as overlapping full-size windows:

* ``mau_region_gather`` is ONE launch from the resident region (30 B per pixel raw) and B window origins -- read from device
  memory -- to B network inputs, with ``mau_scenario_pack``'s per-pixel arithmetic (one copy of the code);
* ``mau_region_stitch`` is ONE launch from all windows' outputs to the blended map: pixel-owned, integer ramp weights, fp64 in a
  fixed per-pixel order, no atomics -- the blend is exact where one window covers a pixel, returns a field cut into windows bit
  for bit, and does not depend on how the windows were batched;
* ``RegionSession`` captures gather -> network for ``batch`` windows into one hipGraph and replays it per batch after a
  device-to-device copy of the batch's origin rows, then stitches once and hands the map to ``scenario.result``.

The host twins (pure numpy) are the truth the device path is tested against, bit for bit.

    python -m mau_amd.region CHECKPOINT --region region.npz --palette-json P --metrics-json M [--window 512 --overlap 128 --batch 8 --precision fp16 --output out.npz]
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import functional as F_
from . import scenario as S
from ._capture import PinnedStage
from ._tile import N_CONT, TileSession, check_ld, check_ncls, check_palette, check_tile, const, norm_row, upload
from .config import CONFIG
from .functional import Act, call, dtype_code, pad8

MAX_WINDOW = 4096
MAX_COVER = 3            # windows over one coordinate: two of the regular stride (overlap <= T // 2) and the last one, moved back


# --------------------------------------------------------------------------- #
# the window grid and the blend weights
# --------------------------------------------------------------------------- #
def window_origins(n: int, T: int, overlap: int) -> np.ndarray:
    """Origins of the windows of edge ``T`` along an axis of ``n`` pixels (int32): 0, S, 2S, ... with S = T - overlap while a
    further window is needed; the LAST origin is moved back to n - T, so every window is full-size and one captured shape serves
    all.  Strictly ascending, from 0 to n - T, no step wider than S <= T, at most three windows over any pixel."""
    n, T, overlap = int(n), int(T), int(overlap)
    if not 16 <= T <= min(n, MAX_WINDOW):
        raise ValueError(f"window_origins: the window must satisfy 16 <= T <= min(n, {MAX_WINDOW}), got T = {T} for n = {n}")
    if not 0 <= overlap <= T // 2:
        raise ValueError(f"window_origins: the overlap must be in [0, T // 2 = {T // 2}], got {overlap}")
    step, origins = T - overlap, [0]
    while origins[-1] + T < n:
        origins.append(min(origins[-1] + step, n - T))
    return np.asarray(origins, dtype=np.int32)


def blend_weights(T: int, ramp: int) -> np.ndarray:
    """``w1(i) = min(i + 1, T - i, ramp)`` for i in [0, T), int64: a window's weight along one axis (the 2-D weight is the product)."""
    T, ramp = int(T), int(ramp)
    if T < 1 or ramp < 1:
        raise ValueError(f"blend_weights: T and ramp must be >= 1, got {T}, {ramp}")
    i = np.arange(T, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, T - i), ramp)


def default_ramp(overlap: int) -> int:
    """The ramp a session blends with: the overlap itself (two neighbours cross-fade over the strip they share), 1 without overlap."""
    return max(1, int(overlap))


def _check_table(t, n: int, T: int, what: str) -> np.ndarray:
    """The rules ``mau_region_stitch`` relies on and cannot check on the device."""
    t = np.asarray(t)
    if t.ndim != 1 or t.size < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"{what} must be a non-empty 1-D integer array of window origins")
    t = t.astype(np.int64)
    if t[0] != 0 or t[-1] != n - T:
        raise ValueError(f"{what} must start at 0 and end at {n - T} (= {n} - {T}), got {int(t[0])} .. {int(t[-1])}")
    d = np.diff(t)
    if d.size and (d.min() < 1 or d.max() > T):
        raise ValueError(f"{what} must be strictly ascending with no gap wider than the window ({T})")
    if t.size > MAX_COVER and (t[MAX_COVER:] - t[:-MAX_COVER]).min() < T:
        raise ValueError(f"{what}: more than {MAX_COVER} windows cover one coordinate")
    return t.astype(np.int32)


# --------------------------------------------------------------------------- #
# host twins (numpy): the truth of the two launches
# --------------------------------------------------------------------------- #
def _plane(a, shape) -> np.ndarray:
    return np.asarray(a).reshape(shape)


def gather_host(dw_t1, dw_t2, rgb, ndvi, temp, origins, T: int, ncls: int, metrics: dict) -> np.ndarray:
    """The dense inputs of the windows at ``origins`` (B, 2) as a (B, 2 ncls + 5, T, T) fp32 array,
    ``[one-hot dw_t1 | rgb | ndvi | temp | one-hot dw_t2]``: the window is cropped (its origin clamped into the region), the raw
    planes go through ``scenario.normalized_planes_host``, a class id >= ncls sets no channel."""
    dw_t1 = np.asarray(dw_t1)
    dw_t1 = dw_t1[0] if dw_t1.ndim == 3 else dw_t1
    Hr, Wr = dw_t1.shape
    dw_t2, rgb = _plane(dw_t2, (Hr, Wr)), _plane(rgb, (3, Hr, Wr))
    ndvi, temp = _plane(ndvi, (Hr, Wr)), _plane(temp, (Hr, Wr))
    T = int(T)
    if T > min(Hr, Wr):
        raise ValueError(f"gather_host: a window of {T} does not fit a region of {Hr} x {Wr}")
    ids = np.arange(int(ncls), dtype=np.int64).reshape(-1, 1, 1)
    out = []
    for y0, x0 in np.asarray(origins, dtype=np.int64).reshape(-1, 2):
        y0, x0 = int(min(max(y0, 0), Hr - T)), int(min(max(x0, 0), Wr - T))
        ys, xs = slice(y0, y0 + T), slice(x0, x0 + T)
        out.append(np.concatenate([(dw_t1[None, ys, xs].astype(np.int64) == ids).astype(np.float32),
                                   S.normalized_planes_host(rgb[:, ys, xs], ndvi[ys, xs], temp[ys, xs], metrics),
                                   (dw_t2[None, ys, xs].astype(np.int64) == ids).astype(np.float32)]))
    return np.stack(out)


def stitch_host(win, ys, xs, shape: Tuple[int, int], ramp: int) -> np.ndarray:
    """The blend of ``mau_region_stitch`` in float64 numpy: win (ny * nx, C, T, T) fp32, window k = iy * nx + ix at
    (ys[iy], xs[ix]) -> (C, Hr, Wr) fp32.  Per pixel, over the windows that cover it in the order iy ascending, ix ascending:
    ``num += w * v`` (float64, every product exact), ``den += w`` (integer), ``out = float32(num / den)``; NaN where no window
    covers.  (The sum starts at +0.0: a lone -0.0 comes out as +0.0.)"""
    win = np.asarray(win)
    ys, xs = np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)
    Hr, Wr = int(shape[0]), int(shape[1])
    if win.ndim != 4 or win.shape[0] != ys.size * xs.size or win.shape[2] != win.shape[3] or win.dtype != np.float32:
        raise ValueError(f"stitch_host: win must be (ny * nx = {ys.size * xs.size}, C, T, T) float32, got {win.shape} {win.dtype}")
    C, T = win.shape[1], win.shape[2]
    w1 = blend_weights(T, ramp)
    w2 = w1[:, None] * w1[None, :]
    num = np.zeros((C, Hr, Wr), dtype=np.float64)
    den = np.zeros((Hr, Wr), dtype=np.int64)
    for iy, y0 in enumerate(ys):
        for ix, x0 in enumerate(xs):
            num[:, y0:y0 + T, x0:x0 + T] += w2.astype(np.float64)[None] * win[iy * xs.size + ix].astype(np.float64)
            den[y0:y0 + T, x0:x0 + T] += w2
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / den.astype(np.float64)[None]
    out[:, den == 0] = np.nan
    return out.astype(np.float32)


# --------------------------------------------------------------------------- #
# the two launches
# --------------------------------------------------------------------------- #
def _gather(dw_t1, dw_t2, rgb, ndvi, temp, origins, norm, T: int, ncls: int, dtype: torch.dtype, ld: int) -> Act:
    Hr, Wr = dw_t1.shape
    B = origins.shape[0]
    out = torch.empty((B, T, T, ld), dtype=dtype, device=dw_t1.device)
    call("mau_region_gather", dw_t1.data_ptr(), dw_t2.data_ptr(), rgb.data_ptr(), ndvi.data_ptr(), temp.data_ptr(), origins.data_ptr(),
         norm.data_ptr(), out.data_ptr(), ld, dtype_code(dtype), B, T, Hr, Wr, ncls, F_._stream())
    return Act(out, 2 * ncls + N_CONT)


def gather(dw_t1, dw_t2, rgb, ndvi, temp, origins, window: int, ncls: int, metrics: dict, dtype: torch.dtype = torch.bfloat16,
           ld: Optional[int] = None) -> Act:
    """One launch (``mau_region_gather``): the resident region + B window origins -> the network's input ``Act`` (B, T, T, ld).
    dw_t1, dw_t2 (Hr,Wr) uint8 (``dw_t2=None``: no land-cover change), rgb (3,Hr,Wr) raw 0..255, ndvi (Hr,Wr), temp (Hr,Wr) raw
    degrees C, fp32, on the device; ``origins`` (B,2) rows of (y0, x0), a host array or an int32 device tensor, each clamped into
    the region by the kernel; ``ld`` (default: 2 ncls + 5 rounded up to 8) is the channel stride.  Bit-identical to
    ``data.pack_tiles`` on the cropped class maps and ``normalized_planes_host`` of the cropped raw planes."""
    dw_t1, rgb, ndvi, temp = check_tile(dw_t1, rgb, ndvi, temp)
    Hr, Wr = dw_t1.shape
    dw_t2 = dw_t1 if dw_t2 is None else F_._dev(dw_t2, "dw_t2", torch.uint8, (Hr, Wr))
    T, ncls = int(window), check_ncls(ncls, "mau_region_gather")
    if not 1 <= T <= min(Hr, Wr, MAX_WINDOW):
        raise ValueError(f"gather: a window of {T} does not fit a region of {Hr} x {Wr} (windows of at most {MAX_WINDOW}); a region "
                         "smaller than a window is one tile: use ScenarioSession")
    ld = check_ld(ld, 2 * ncls + N_CONT, "gather")
    origins = const(origins, torch.int32, dw_t1.device)
    if origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1:
        raise ValueError(f"origins must be (B, 2) rows of (y0, x0), got {tuple(origins.shape)}")
    norm = const(norm_row(metrics), torch.float64, dw_t1.device)
    return _gather(dw_t1, dw_t2, rgb, ndvi, temp, origins, norm, T, ncls, dtype, ld)


def _stitch(win: torch.Tensor, ys: torch.Tensor, xs: torch.Tensor, Hr: int, Wr: int, ramp: int) -> torch.Tensor:
    _, C, T, _ = win.shape
    out = torch.empty((C, Hr, Wr), dtype=torch.float32, device=win.device)
    call("mau_region_stitch", win.data_ptr(), ys.data_ptr(), xs.data_ptr(), out.data_ptr(), C, T, int(ramp), Hr, Wr, ys.numel(), xs.numel(),
         F_._stream())
    return out


def stitch(win: torch.Tensor, ys, xs, shape: Tuple[int, int], ramp: int) -> torch.Tensor:
    """One launch (``mau_region_stitch``): the windows' outputs win (ny * nx, C, T, T) fp32 on the device, window k = iy * nx + ix
    at (ys[iy], xs[ix]) -> the blended (C, Hr, Wr) fp32 map, bit-identical to ``stitch_host``.  ``ys`` and ``xs`` are HOST arrays:
    the device cannot check them, so this wrapper does -- strictly ascending, from 0 to Hr - T / Wr - T, no gap wider than T and
    at most three windows over a coordinate (what ``window_origins`` gives)."""
    win = F_._dev(win, "win", torch.float32)
    Hr, Wr = int(shape[0]), int(shape[1])
    if win.dim() != 4 or win.shape[2] != win.shape[3] or win.shape[1] < 1:
        raise ValueError(f"win must be (ny * nx, C, T, T), got {tuple(win.shape)}")
    T = win.shape[2]
    if not 1 <= T <= min(Hr, Wr, MAX_WINDOW):
        raise ValueError(f"stitch: a window of {T} does not fit a region of {Hr} x {Wr} (windows of at most {MAX_WINDOW})")
    if int(ramp) < 1:
        raise ValueError(f"stitch: ramp must be >= 1, got {ramp}")
    ys, xs = _check_table(ys, Hr, T, "ys"), _check_table(xs, Wr, T, "xs")
    if win.shape[0] != ys.size * xs.size:
        raise ValueError(f"win holds {win.shape[0]} windows, the tables name {ys.size} x {xs.size}")
    return _stitch(win, const(ys, torch.int32, win.device), const(xs, torch.int32, win.device), Hr, Wr, ramp)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
class RegionResult(S.ScenarioResult):
    """``output`` (1, 2, Hr, Wr) fp32, the stitched map in the network's normalised units; the fields of ``ScenarioResult`` on it
    (``ndvi``, ``temp_c``, ``delta`` (1, Hr, Wr), ``dw_t2``, ``stats`` (1, 5) and the named statistics); ``window_outputs``
    (nWin, 2, T, T) fp32, every window's own output in window order k = iy * nx + ix.  All on the device."""

    def __init__(self, output, window_outputs, ndvi, temp_c, delta, dw_t2, stats):
        super().__init__(ndvi, temp_c, delta, dw_t2, stats)
        self.output, self.window_outputs = output, window_outputs


class RegionSession(TileSession):
    """``RegionSession(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, palette=..., metrics=...)(dw_t2=None) -> RegionResult``.

    The region (device tensors: dw_t1 (Hr,Wr) uint8; rgb (3,Hr,Wr), ndvi (Hr,Wr), temp (Hr,Wr) fp32, raw values) stays resident.
    It is cut into ``window`` x ``window`` tiles at ``window_origins`` of both axes (``ys``, ``xs``; window k = iy * nx + ix) that
    share ``overlap`` pixels with their neighbours and are blended with ``ramp = max(1, overlap)``.  ``overlap=None`` means
    ``window // 4``: a choice, no number has been measured for it.  ``dw_t2``: the edited class map (None = no land-cover
    change); ``metadata`` is (1,F) for the whole region or (nWin,F), one row per window in window order; ``temp_series`` is (1,L);
    ``temp_orig``: the raster the temperature change is taken against (None = ``temp``).  ``palette`` gives the number of classes.

    The session freezes the model, warms up on a side stream and captures gather -> network for ``batch`` windows into ONE
    hipGraph.  A call optionally replaces the edited class map (same shape; a device tensor is copied device to device, a host
    array travels through pinned memory) and then, per batch, copies the batch's origin rows (and metadata rows, if per window)
    into the session's buffers device to device, replays, and copies the valid rows of the output into ``window_outputs``; a
    ragged last batch repeats the last window in its unused slots.  One ``mau_region_stitch`` and one ``scenario.result`` follow.
    There is no host synchronisation inside a call.  The bits of a window's output may depend on ``batch`` (the convolution's
    inference form depends on the launch shape); the gather and the stitch do not.  A region smaller than a window is
    one tile: use ``ScenarioSession``.  Reload weights -> build a new session."""

    def __init__(self, model: torch.nn.Module, dw_t1, rgb, ndvi, temp, metadata, temp_series, *, palette, metrics: dict,
                 window: int = CONFIG.model.img_size, overlap: Optional[int] = None, batch: int = 8, dw_t2=None, temp_orig=None,
                 warmup: int = 2):
        if int(batch) < 1:
            raise ValueError("batch must be >= 1")
        self.window, self.overlap = int(window), int(window) // 4 if overlap is None else int(overlap)
        self._ncls = check_ncls(check_palette(palette).shape[0], "mau_region_gather")
        super().__init__(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics, batch, dw_t2=dw_t2, temp_orig=temp_orig)
        dev, B = self._device, self.batch
        if self._dw_t2 is None:                                                         # no land-cover change; a call may replace it
            self._dw_t2 = self._tile[0].clone()
        self._ys, self._xs = const(self.ys, torch.int32, dev), const(self.xs, torch.int32, dev)
        # the origin rows of all windows, padded to whole batches with the last window
        rows = np.stack([np.repeat(self.ys, self.xs.size), np.tile(self.xs, self.ys.size)], axis=1).astype(np.int32)
        self._origins_all = const(np.concatenate([rows, np.repeat(rows[-1:], self._batches * B - self.windows, 0)]), torch.int32, dev)
        self._origins = self._origins_all[:B].clone()
        self._stage = PinnedStage(self.shape, torch.uint8)                              # a host class map travels through pinned memory
        self._capture(warmup)

    def _fit(self, Hr: int, Wr: int) -> None:
        T = self.window
        if T > min(Hr, Wr):
            raise ValueError(f"RegionSession: the region ({Hr} x {Wr}) is smaller than a window ({T}); one tile is ScenarioSession's case")
        self.ys, self.xs = window_origins(Hr, T, self.overlap), window_origins(Wr, T, self.overlap)
        self.ramp, self.windows = default_ramp(self.overlap), self.ys.size * self.xs.size
        self._batches = -(-self.windows // self.batch)

    def _metadata(self, md: torch.Tensor) -> torch.Tensor:
        """One row for the region, or one per window: then ``_md_all`` holds them, padded to whole batches with the last window's."""
        nWin, B = self.windows, self.batch
        md = md.reshape(1, -1) if md.dim() < 2 else md
        if md.dim() != 2 or md.shape[0] not in (1, nWin):
            raise ValueError(f"metadata must be (1, F) for the region or ({nWin}, F), one row per window, got {tuple(md.shape)}")
        self._md_all = torch.cat([md, md[-1:].expand(self._batches * B - nWin, -1)]).contiguous() if md.shape[0] > 1 else None
        return (md.expand(B, -1) if self._md_all is None else self._md_all[:B]).contiguous().clone()

    def _run(self) -> torch.Tensor:
        x = _gather(self._tile[0], self._dw_t2, *self._tile[1:], self._origins, self._norm, self.window, self._ncls, self.dtype,
                    pad8(2 * self._ncls + N_CONT))
        return self.model(x, self._ts, self._md)

    @torch.no_grad()
    def __call__(self, dw_t2=None) -> RegionResult:
        if dw_t2 is not None:
            upload(dw_t2, self._dw_t2, self._stage, "dw_t2")
        B, nWin, T = self.batch, self.windows, self.window
        wo = torch.empty((nWin,) + tuple(self._out.shape[1:]), dtype=torch.float32, device=self._out.device)
        for i in range(self._batches):
            self._origins.copy_(self._origins_all[i * B:(i + 1) * B], non_blocking=True)
            if self._md_all is not None:
                self._md.copy_(self._md_all[i * B:(i + 1) * B], non_blocking=True)
            self._replay()
            valid = min(B, nWin - i * B)
            wo[i * B:i * B + valid].copy_(self._out[:valid], non_blocking=True)
        out = _stitch(wo, self._ys, self._xs, *self.shape, self.ramp)[None]
        r = S.result(out, self._temp_orig, self._tile[0], self._dw_t2.clone()[None], self._mean, self._std)
        return RegionResult(out, wo, r.ndvi, r.temp_c, r.delta, r.dw_t2, r.stats)


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def run_region(checkpoint: str, region: str, palette_json: str, metrics_json: str, window: int = CONFIG.model.img_size,
               overlap: Optional[int] = None, batch: int = 8, precision: str = "fp16", output: str = "", device: str = "cuda") -> dict:
    """Body of the CLI: one session call on the region of ``region`` (.npz: ``scenario.load_tile``'s keys; dw_t2 is the edited class
    map).  Returns -- and with ``output`` writes as .npz -- output (1,2,Hr,Wr), ndvi, temp_c, delta (1,Hr,Wr), dw_t2, stats and the
    statistics by name, and the window grid: ys, xs, window, overlap, ramp."""
    t = S.load_tile(region, metrics_json, palette_json, device, checkpoint)
    t.model.set_precision(precision)
    sess = RegionSession(*t[:7], palette=t.palette, metrics=t.metrics, window=window, overlap=overlap, batch=batch, dw_t2=t.dw_t2,
                         temp_orig=t.temp_orig)
    r = sess()
    stats = r.stats.cpu().numpy()
    res = {"output": r.output.cpu().numpy(), "ndvi": r.ndvi.cpu().numpy(), "temp_c": r.temp_c.cpu().numpy(), "delta": r.delta.cpu().numpy(),
           "dw_t2": r.dw_t2.cpu().numpy(), "stats": stats, **{name: stats[:, i] for i, name in enumerate(S.STAT_NAMES)},
           "ys": sess.ys, "xs": sess.xs, "window": np.int32(sess.window), "overlap": np.int32(sess.overlap), "ramp": np.int32(sess.ramp)}
    if output:
        np.savez(output, **res)
    return res


def _cli():
    import typer
    app = typer.Typer(add_completion=False)

    @app.command()
    def main(checkpoint: str = typer.Argument(..., help="reference-layout .pth (src/train.py:303-316)"),
             region: str = typer.Option(..., help=".npz: dw, rgb, ndvi, temp, metadata_raw [, dw_t2, temp_series, temp_orig]"),
             palette_json: str = typer.Option(..., help="the palette's hex colours in class order"),
             metrics_json: str = typer.Option(..., help="normalization_metrics.json"),
             window: int = CONFIG.model.img_size, overlap: int = typer.Option(-1, help="pixels neighbouring windows share; -1 = window // 4"),
             batch: int = 8, precision: str = "fp16", output: str = "", device: str = "gpu"):
        """The forecast of a checkpoint for a whole region: overlapping windows at the trained resolution, blended."""
        res = run_region(checkpoint, region, palette_json, metrics_json, window, None if overlap < 0 else overlap, batch, precision, output,
                         F_.typer_device(device))
        ny, nx = len(res["ys"]), len(res["xs"])
        typer.echo(f"region {res['output'].shape[2]} x {res['output'].shape[3]}: {ny} x {nx} windows of {int(res['window'])} "
                   f"(overlap {int(res['overlap'])}, ramp {int(res['ramp'])}), {-(-ny * nx // batch)} batches of {batch}")
        typer.echo("region: " + ", ".join(f"{name} {res[name][0]:.6g}" for name in S.STAT_NAMES))
        if output:
            typer.echo(f"Saved region result to {output}")

    return app


if __name__ == "__main__":
    _cli()()
