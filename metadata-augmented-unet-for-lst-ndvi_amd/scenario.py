"""Scenario sessions: a painted canvas -> forecast and temperature change, on the device (the reference's Streamlit app).

In the app a user paints land-cover changes on a canvas and asks for the forecast (app/Home.py:333-411).  Per click the
reference resizes the RGBA canvas, matches every pixel against the palette (``cdist`` + ``argmin``), merges with the
original class map by alpha, normalises five planes in float64, builds two one-hot stacks, copies a dense 23-plane fp32
tensor to the device (92 B per pixel), and after the forward copies the output back, un-normalises it, subtracts the
original temperature raster and takes the mean (app/processing_utils.py:70-181).  Here

* ``mau_scenario_pack`` is ONE launch from the canvas (4 B per canvas pixel) and the resident base tile to the network's
  input and the edited class map -- nearest-neighbour resize through two index tables, integer palette match, fp64
  normalisation, one-hot channels, NHWC-ld layout and the 16-bit cast;
* ``mau_scenario_result`` is ONE launch from the head's output to NDVI, temperature in degrees C, its difference to the
  original raster and five fp64 statistics per scenario (fixed summation order, no float atomics);
* ``ScenarioSession`` captures pack -> network -> result into one hipGraph: an edit costs one canvas upload, one replay
  and one small read-back.  ``scenarios=N`` evaluates N canvases of one base tile per replay.

The host helpers (pure numpy) spell the reference's own path; ``prepare_input_host`` is the truth the device path is
tested against, bit for bit.

    python -m mau_amd.scenario CHECKPOINT --tile tile.npz --palette-json P --metrics-json M [--precision fp16] [--output out.npz]
"""
from __future__ import annotations

import json
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from ._capture import PinnedStage
from ._tile import METRIC_KEYS, N_CONT, TileSession, check_metrics, check_ncls, check_palette, check_tile, const, norm_row, upload
from .functional import Act, _dev, call, dtype_code, lib, pad8

STAT_NAMES = ("mean_delta", "min_delta", "max_delta", "edited_pixels", "mean_delta_edited")


# --------------------------------------------------------------------------- #
# host helpers (numpy): the reference's path, in its own arithmetic
# --------------------------------------------------------------------------- #
def nearest_index_table(n_in: int, n_out: int) -> np.ndarray:
    """Source index per destination index of Pillow's nearest-neighbour resize from ``n_in`` to ``n_out`` samples (int32).
    Pillow's affine scaler starts at half a step and ACCUMULATES the step in double; the closed form
    ``floor((x + 0.5) * n_in / n_out)`` rounds differently (200 -> 250 disagrees on many pixels)."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"nearest_index_table: sizes must be positive, got {n_in} -> {n_out}")
    a = float(n_in) / float(n_out)
    xo = 0.5 * a
    idx = np.empty(n_out, dtype=np.int32)
    for x in range(n_out):
        idx[x] = min(int(xo), n_in - 1)
        xo += a
    return idx


def palette_from_hex(colours: Sequence[str]) -> np.ndarray:
    """``['#419bdf', ...]`` in class order -> (ncls, 3) uint8 (the reference's ``hex_to_rgb``, :49-51)."""
    return np.array([[int(c.lstrip("#")[i:i + 2], 16) for i in (0, 2, 4)] for c in colours], dtype=np.uint8)


def canvas_to_dw_map_host(canvas: np.ndarray, target_shape: Tuple[int, int], palette, original_map: Optional[np.ndarray] = None) -> np.ndarray:
    """``canvas_to_dw_map`` (:70-110): (Hc, Wc, 4) RGBA -> (H, W) uint8 class map.  The canvas is resized with nearest
    neighbour; a pixel takes the palette entry of smallest RGB distance (the first on a tie -- integer squared distances,
    which order exactly as ``cdist``'s); with ``original_map``, pixels of alpha 0 keep its class."""
    canvas, palette = np.asarray(canvas), check_palette(palette)
    if canvas.ndim != 3 or canvas.shape[2] != 4:
        raise ValueError(f"canvas must be (Hc, Wc, 4) RGBA, got {canvas.shape}")
    H, W = int(target_shape[0]), int(target_shape[1])
    arr = canvas.astype(np.uint8)[nearest_index_table(canvas.shape[0], H)][:, nearest_index_table(canvas.shape[1], W)]
    diff = arr[:, :, None, :3].astype(np.int32) - palette[None, None].astype(np.int32)
    nearest = np.argmin((diff * diff).sum(axis=3), axis=2)
    if original_map is None:
        return nearest.astype(np.uint8)
    original_map = np.asarray(original_map)
    if original_map.ndim == 3:
        original_map = original_map[0]
    return np.where(arr[:, :, 3] > 0, nearest, original_map).astype(np.uint8)


def normalized_planes_host(rgb, ndvi, temp, metrics: dict) -> np.ndarray:
    """The five continuous planes of the network's input, (5, H, W) fp32: float64 arithmetic rounded to float once (:136-139, :149)."""
    check_metrics(metrics)
    row = norm_row(metrics)
    colour = np.asarray(rgb, dtype=np.float64)
    h, w = colour.shape[-2:]
    planes = np.empty((N_CONT, h, w), dtype=np.float64)
    planes[:3] = (colour.reshape(3, h, w) / 255.0 - row[0:3].reshape(3, 1, 1)) / row[3:6].reshape(3, 1, 1)
    planes[3] = np.asarray(ndvi, dtype=np.float64).reshape(h, w)
    planes[4] = (np.asarray(temp, dtype=np.float64).reshape(h, w) - row[6]) / row[7]
    return planes.astype(np.float32)


def prepare_input_host(dw_t1, rgb, ndvi, temp, canvas, palette, metrics: dict) -> np.ndarray:
    """The dense input of ``prepare_input`` (:134-149) as a (1, 2 ncls + 5, H, W) fp32 array:
    ``[one-hot dw_t1 | rgb | ndvi | temp | one-hot dw_t2]``, the planes normalised in float64 and rounded to float once."""
    palette = check_palette(palette)
    dw_t1 = np.asarray(dw_t1)
    if dw_t1.ndim == 3:
        dw_t1 = dw_t1[0]
    dw_t2 = canvas_to_dw_map_host(canvas, dw_t1.shape, palette, original_map=dw_t1)
    ids = np.arange(palette.shape[0], dtype=np.int64).reshape(-1, 1, 1)
    dense = np.concatenate([(dw_t1[None].astype(np.int64) == ids).astype(np.float32), normalized_planes_host(rgb, ndvi, temp, metrics),
                            (dw_t2[None].astype(np.int64) == ids).astype(np.float32)])
    return dense[None]


def metadata_row(lat, lon, population, year_t1, month_t1, year_t2, month_t2, meta_mean, meta_std) -> np.ndarray:
    """The (1, 8) fp32 metadata row of :151-160: z-scored (lat, lon, population, years between the dates), then the two dates."""
    mean, std = np.asarray(meta_mean, dtype=np.float64), np.asarray(meta_std, dtype=np.float64)
    if mean.shape != (4,) or std.shape != (4,):
        raise ValueError("metadata_row: meta_mean and meta_std hold four values each")
    row = np.empty((1, 8), dtype=np.float64)
    row[0, :4] = (np.array([lat, lon, population, (year_t2 - year_t1) + (month_t2 - month_t1) / 12.0], dtype=np.float64) - mean) / std
    row[0, 4:] = year_t1, month_t1, year_t2, month_t2
    return row.astype(np.float32)


def normalize_temp_series(ts, metrics: dict) -> np.ndarray:
    """The (1, T) fp32 temperature series of :167-168."""
    check_metrics(metrics, ("temp_series_mean", "temp_series_std"))
    series = np.asarray(ts, dtype=np.float64).reshape(1, -1)
    return ((series - float(metrics["temp_series_mean"])) / float(metrics["temp_series_std"])).astype(np.float32)


# --------------------------------------------------------------------------- #
# the two launches
# --------------------------------------------------------------------------- #
def _canvas4(canvas: torch.Tensor) -> torch.Tensor:
    if canvas.dim() == 3:
        canvas = canvas[None]
    if canvas.dim() != 4 or canvas.shape[3] != 4:
        raise ValueError(f"canvas must be (Hc, Wc, 4) or (N, Hc, Wc, 4) RGBA, got {tuple(canvas.shape)}")
    return canvas


class _Tables:
    """The device-side constants of ``mau_scenario_pack`` for one (tile shape, canvas shape, palette, metrics)."""

    def __init__(self, tile_shape, canvas_shape, palette, metrics: dict, dev, norm: Optional[torch.Tensor] = None):
        palette = check_palette(palette)
        self.ncls = check_ncls(palette.shape[0], "mau_scenario_pack")
        self.palette = const(palette, torch.uint8, dev)
        self.norm = const(norm_row(metrics), torch.float64, dev) if norm is None else norm      # a session has uploaded its own
        self.yidx = const(nearest_index_table(canvas_shape[0], tile_shape[0]), torch.int32, dev)
        self.xidx = const(nearest_index_table(canvas_shape[1], tile_shape[1]), torch.int32, dev)


def _pack(dw_t1, rgb, ndvi, temp, canvas, tb: _Tables, dtype: torch.dtype):
    N, Hc, Wc, _ = canvas.shape
    H, W = dw_t1.shape
    C = 2 * tb.ncls + N_CONT
    out = torch.empty((N, H, W, pad8(C)), dtype=dtype, device=dw_t1.device)
    dw_t2 = torch.empty((N, H, W), dtype=torch.uint8, device=dw_t1.device)
    call("mau_scenario_pack", dw_t1.data_ptr(), rgb.data_ptr(), ndvi.data_ptr(), temp.data_ptr(), canvas.data_ptr(), tb.yidx.data_ptr(),
         tb.xidx.data_ptr(), tb.palette.data_ptr(), tb.norm.data_ptr(), out.data_ptr(), out.shape[-1], dw_t2.data_ptr(), dtype_code(dtype),
         N, H, W, Hc, Wc, tb.ncls, F_._stream())
    return Act(out, C), dw_t2


def pack(dw_t1, rgb, ndvi, temp, canvas, palette, metrics: dict, dtype: torch.dtype = torch.bfloat16) -> Tuple[Act, torch.Tensor]:
    """One launch (``mau_scenario_pack``): base tile + N painted canvases -> (the network's input ``Act`` (N, H, W, ld),
    dw_t2 (N, H, W) uint8).  dw_t1 (H,W) uint8, rgb (3,H,W) raw 0..255, ndvi (H,W), temp (H,W) raw degrees C, fp32; canvas
    (Hc,Wc,4) or (N,Hc,Wc,4) uint8 RGBA; all on the device.  palette (ncls,3) uint8 and the metrics dict are host values.
    Bit-identical to ``data.pack_tiles`` on the class maps and normalised planes of ``prepare_input_host``."""
    dw_t1, rgb, ndvi, temp = check_tile(dw_t1, rgb, ndvi, temp)
    canvas = _canvas4(_dev(canvas, "canvas", torch.uint8))
    tb = _Tables(dw_t1.shape, canvas.shape[1:3], palette, metrics, dw_t1.device)
    return _pack(dw_t1, rgb, ndvi, temp, canvas, tb, dtype)


class ScenarioResult:
    """What ``mau_scenario_result`` wrote: ``ndvi``, ``temp_c``, ``delta`` (N, H, W) fp32 (``delta`` None without an original
    raster), ``dw_t2`` (N, H, W) uint8 and ``stats`` (N, 5) fp64, all on the device; the named statistics are views of ``stats``."""

    def __init__(self, ndvi, temp_c, delta, dw_t2, stats):
        self.ndvi, self.temp_c, self.delta, self.dw_t2, self.stats = ndvi, temp_c, delta, dw_t2, stats

    mean_delta = property(lambda self: self.stats[:, 0])
    min_delta = property(lambda self: self.stats[:, 1])
    max_delta = property(lambda self: self.stats[:, 2])
    edited_pixels = property(lambda self: self.stats[:, 3])
    mean_delta_edited = property(lambda self: self.stats[:, 4])

    def clone(self) -> "ScenarioResult":
        return ScenarioResult(*(None if t is None else t.clone() for t in (self.ndvi, self.temp_c, self.delta, self.dw_t2, self.stats)))


def result(output: torch.Tensor, temp_orig: Optional[torch.Tensor], dw_t1: torch.Tensor, dw_t2: torch.Tensor, temp_mean: float,
           temp_std: float, tickets: Optional[torch.Tensor] = None) -> ScenarioResult:
    """One launch (``mau_scenario_result``): the head's output (N, 2, H, W) fp32 -> :class:`ScenarioResult`.  temp_orig
    (H, W) fp32 raw degrees C or None (no difference: the delta statistics are NaN); dw_t1 (H, W), dw_t2 (N, H, W) uint8.
    ``temp_c = out * temp_std + temp_mean`` as float32 numpy computes it (two roundings); the statistics are fp64 sums in a
    fixed order: a scenario's row does not depend on N, repeated calls agree bit for bit."""
    output = _dev(output, "output", torch.float32)
    if output.dim() != 4 or output.shape[1] != 2:
        raise ValueError(f"output must be (N, 2, H, W), got {tuple(output.shape)}")
    N, _, H, W = output.shape
    dw_t1 = _dev(dw_t1, "dw_t1", torch.uint8, (H, W))
    dw_t2 = _dev(dw_t2, "dw_t2", torch.uint8, (N, H, W))
    if temp_orig is not None:
        temp_orig = _dev(temp_orig, "temp_orig", torch.float32, (H, W))
    dev = output.device
    ndvi = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    temp_c = torch.empty_like(ndvi)
    delta = torch.empty_like(ndvi) if temp_orig is not None else None
    stats = torch.empty((N, lib.mau_scenario_result_row_elems()), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.mau_scenario_result_ws_elems(N, H, W), dtype=torch.float64, device=dev)
    tickets = F_._tickets(dev) if tickets is None else tickets
    call("mau_scenario_result", output.data_ptr(), None if temp_orig is None else temp_orig.data_ptr(), dw_t1.data_ptr(), dw_t2.data_ptr(),
         float(temp_mean), float(temp_std), ndvi.data_ptr(), temp_c.data_ptr(), None if delta is None else delta.data_ptr(),
         stats.data_ptr(), ws.data_ptr(), tickets.data_ptr(), N, H, W, F_._stream())
    return ScenarioResult(ndvi, temp_c, delta, dw_t2, stats)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
class ScenarioSession(TileSession):
    """``ScenarioSession(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, palette=..., metrics=...)(canvas) -> ScenarioResult``.

    The base tile (device tensors: dw_t1 (H,W) uint8; rgb (3,H,W), ndvi (H,W), temp (H,W) fp32, raw values), the metadata row
    (1,F) and the temperature series (1,T) are fixed at construction; ``palette`` is the (ncls,3) uint8 colour table in class
    order and ``metrics`` a dict with the keys of ``normalization_metrics.json``.  The session freezes the model
    (``freeze_inference``), warms up on a side stream and captures ONE hipGraph: ``mau_scenario_pack`` -> the network ->
    ``mau_scenario_result``.  A call copies the canvas -- (Hc,Wc,4) or (N,Hc,Wc,4) uint8, host array or device tensor, of the
    ``canvas_shape`` and ``scenarios`` given here -- into the session's buffer and replays.  ``temp_orig``: the raster the
    temperature change is taken against (app/Home.py:376-400); None = ``temp``.  ``clone_output=False`` returns the session's
    own buffers, valid until the next call.  Reload weights -> build a new session."""

    def __init__(self, model: torch.nn.Module, dw_t1, rgb, ndvi, temp, metadata, temp_series, *, palette, metrics: dict,
                 canvas_shape: Tuple[int, int] = (512, 512), scenarios: int = 1, temp_orig=None, warmup: int = 2,
                 clone_output: bool = True):
        if scenarios < 1:
            raise ValueError("scenarios must be >= 1")
        super().__init__(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics, scenarios, temp_orig=temp_orig)
        N, (Hc, Wc) = self.batch, (int(canvas_shape[0]), int(canvas_shape[1]))
        self.clone_output = clone_output
        self._tables = _Tables(self.shape, (Hc, Wc), palette, metrics, self._device, norm=self._norm)
        self._canvas = torch.zeros((N, Hc, Wc, 4), dtype=torch.uint8, device=self._device)
        self._stage = PinnedStage((N, Hc, Wc, 4), torch.uint8)                          # host canvases travel through pinned memory
        self._tickets = self._own_tickets()
        self._capture(warmup)

    def _run(self) -> ScenarioResult:
        x, dw_t2 = _pack(*self._tile, self._canvas, self._tables, self.dtype)
        return result(self.model(x, self._ts, self._md), self._temp_orig, self._tile[0], dw_t2, self._mean, self._std, self._tickets)

    @property
    def canvas(self) -> torch.Tensor:
        """The session's own (N, Hc, Wc, 4) uint8 canvas buffer: a caller that fills it and passes it to ``__call__`` pays no copy."""
        return self._canvas

    @torch.no_grad()
    def __call__(self, canvas) -> ScenarioResult:
        src = canvas if isinstance(canvas, torch.Tensor) else np.asarray(canvas)
        upload(src[None] if src.ndim == 3 else src, self._canvas, self._stage, "canvas")     # (Hc, Wc, 4): the one canvas of scenarios == 1
        self._replay()
        return self._out.clone() if self.clone_output else self._out


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
# what ``load_tile`` read; the first seven fields are the positional arguments of the sessions
TileInputs = namedtuple("TileInputs", "model dw rgb ndvi temp metadata temp_series dw_t2 temp_orig metrics palette npz")


def load_tile(npz_path: str, metrics_json: str, palette_json: Optional[str] = None, device: str = "cuda", checkpoint: Optional[str] = None,
              ncls: Optional[int] = None) -> TileInputs:
    """What the command lines of ``scenario``, ``placement`` and ``region`` read.  The .npz holds dw -- (H, W) or (1, H, W) --, rgb,
    ndvi, temp of H * W values per plane, metadata_raw = (lat, lon, population, year_t1, month_t1, year_t2, month_t2) and optionally
    temp_series (raw), dw_t2 and temp_orig.  Returns, on ``device``: dw (H, W) uint8; rgb (3, H, W), ndvi, temp (H, W) fp32; metadata
    (1, 8) (``metadata_row``); temp_series (1, T) (``normalize_temp_series``; zeros (1, 60) without one, :172-175); dw_t2, temp_orig
    (H, W) or None; then the metrics dict (every key of ``METRIC_KEYS``), the palette (ncls, 3) uint8 of ``palette_json`` (hex
    colours in class order) or None, and the opened .npz for a tool's own keys (``canvas``).  ``model`` is ``checkpoint``'s for
    ``ncls`` classes (None: the palette's) -- two one-hot stacks and the five continuous planes -- and series of T, or None."""
    palette = None
    if palette_json:
        with open(palette_json) as f:
            palette = palette_from_hex(json.load(f))
    with open(metrics_json) as f:
        metrics = json.load(f)
    check_metrics(metrics, METRIC_KEYS)
    d = np.load(npz_path)
    md = metadata_row(*[float(v) for v in d["metadata_raw"]], metrics["meta_mean"], metrics["meta_std"])
    ts = normalize_temp_series(d["temp_series"], metrics) if "temp_series" in d else np.zeros((1, 60), dtype=np.float32)
    dw = np.asarray(d["dw"])
    dw = dw[0] if dw.ndim == 3 else dw
    H, W = dw.shape
    model = None
    if checkpoint:
        from .checkpoint import load_model
        model = load_model(checkpoint, device=device, spatial_channels=2 * int(ncls or palette.shape[0]) + N_CONT, seq_len=ts.shape[1])
    dev = lambda a, dt, shape: torch.from_numpy(np.ascontiguousarray(np.reshape(a, shape), dtype=dt)).to(device)       # noqa: E731
    optional = lambda key, dt: dev(d[key], dt, (H, W)) if key in d else None                                           # noqa: E731
    return TileInputs(model, dev(dw, np.uint8, (H, W)), dev(d["rgb"], np.float32, (3, H, W)), dev(d["ndvi"], np.float32, (H, W)),
                      dev(d["temp"], np.float32, (H, W)), dev(md, np.float32, md.shape), dev(ts, np.float32, ts.shape),
                      optional("dw_t2", np.uint8), optional("temp_orig", np.float32), metrics, palette, d)


def run_tile(checkpoint: str, tile: str, palette_json: str, metrics_json: str, precision: str = "fp16", output: str = "",
             device: str = "cuda") -> dict:
    """Body of the CLI: one session call on the tile of ``tile`` (.npz: ``load_tile``'s keys and canvas).  Returns -- and with
    ``output`` writes as .npz -- ndvi, temp_c, delta, dw_t2, stats and the statistics by name."""
    t = load_tile(tile, metrics_json, palette_json, device, checkpoint)
    canvas = np.ascontiguousarray(t.npz["canvas"], dtype=np.uint8)
    t.model.set_precision(precision)
    sess = ScenarioSession(*t[:7], palette=t.palette, metrics=t.metrics, canvas_shape=canvas.shape[-3:-1],
                           scenarios=1 if canvas.ndim == 3 else canvas.shape[0], temp_orig=t.temp_orig)
    r = sess(canvas)
    stats = r.stats.cpu().numpy()
    res = {"ndvi": r.ndvi.cpu().numpy(), "temp_c": r.temp_c.cpu().numpy(), "delta": r.delta.cpu().numpy(), "dw_t2": r.dw_t2.cpu().numpy(),
           "stats": stats, **{name: stats[:, i] for i, name in enumerate(STAT_NAMES)}}
    if output:
        np.savez(output, **res)
    return res


def _cli():
    import typer
    app = typer.Typer(add_completion=False)

    @app.command()
    def main(checkpoint: str = typer.Argument(..., help="reference-layout .pth (src/train.py:303-316)"),
             tile: str = typer.Option(..., help=".npz: dw, rgb, ndvi, temp, canvas, metadata_raw [, temp_series, temp_orig]"),
             palette_json: str = typer.Option(..., help="the palette's hex colours in class order"),
             metrics_json: str = typer.Option(..., help="normalization_metrics.json"),
             precision: str = "fp16", output: str = "", device: str = "gpu"):
        """One scenario (canvas edit -> forecast and temperature change) of a checkpoint on one tile."""
        res = run_tile(checkpoint, tile, palette_json, metrics_json, precision, output, F_.typer_device(device))
        for n in range(res["stats"].shape[0]):
            typer.echo("scenario %d: " % n + ", ".join(f"{name} {res[name][n]:.6g}" for name in STAT_NAMES))
        if output:
            typer.echo(f"Saved scenario result to {output}")

    return app


if __name__ == "__main__":
    _cli()()
