"""Placement sweeps: where on a tile does a block of one land-cover class change the forecast most, on the device.

``ScenarioSession`` answers "what happens if I paint *this*"; the next question is "where does a block of trees, or of built-up
area, cool (or heat) most?".  A placement is a rectangular stamp of ``ph x pw`` pixels of one class written into the tile's
second class map at ``(y0, x0)`` -- the app's canvas edit changes nothing else (app/processing_utils.py:70-110) -- and its effect
is the forecast with the stamp minus the forecast of the unedited tile.  It is the spatial counterpart of the metadata sweeps of
``sensitivity``.  Here

* ``mau_placement_pack`` is ONE launch from the resident tile and B rows of ``(y0, x0, cls)`` -- read from device memory -- to B
  network inputs, with ``mau_scenario_pack``'s per-pixel arithmetic (one copy of the code);
* ``mau_placement_result`` is ONE launch from the head's output of the B samples and of the unedited tile to twelve fp64 figures
  per placement (fixed summation order, no float atomics): the full-resolution maps never leave the device;
* ``PlacementSession`` captures pack -> network -> result for ``batch`` placements into one hipGraph and replays it per batch.
  The baseline goes through the SAME graph at the SAME batch (every row ``cls = -1``): a forward at another batch size may take
  another inference form of the convolution, and that difference would show up as a false effect.

The host twins (pure numpy) are the product's reference; the order-exact twin of the reduction lives with the tests.

    python -m mau_amd.placement CHECKPOINT --tile tile.npz --metrics-json M --classes 1,6 [--patch 32 --stride 16 --batch 8 --roi roi.npy --screen 8 --output out.npz]
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from . import scenario as S
from ._capture import PinnedStage
from ._tile import N_CONT, TileSession, check_ld, check_ncls, check_tile, const, norm_row
from .functional import Act, call, dtype_code, lib, pad8

ROW = 12
ROW_NAMES = ("stamp_pixels", "mean_dt", "min_dt", "max_dt", "mean_dt_stamp", "mean_dt_outside", "roi_pixels", "mean_dt_roi",
             "mean_dn", "mean_dn_stamp", "mean_dn_roi", "non_finite")
NO_EDIT = -1             # the class of a row that leaves the tile as it is: the baseline sample, the padding of a ragged batch
MAX_BATCH = 65535
MAX_PIXELS = 1 << 30
GRID_ENTRIES = (1, 4, 7)                 # the grids the command line writes: mean dT over the tile, the stamp and the roi


# --------------------------------------------------------------------------- #
# the stamp grid and the table of edits
# --------------------------------------------------------------------------- #
def stamp_grid(n: int, p: int, stride: int) -> np.ndarray:
    """Origins of stamps of edge ``p`` along an axis of ``n`` pixels (int32): 0, stride, ... while ``o + p <= n``, and ``n - p``
    appended if the last one is smaller -- every stamp is whole and the far edge is reached.  ``stride > p`` leaves gaps."""
    n, p, stride = int(n), int(p), int(stride)
    if p < 1 or stride < 1:
        raise ValueError(f"stamp_grid: the stamp and the stride must be >= 1, got {p}, {stride}")
    if p > n:
        raise ValueError(f"stamp_grid: a stamp of {p} does not fit an axis of {n}")
    origins = list(range(0, n - p + 1, stride))
    if origins[-1] < n - p:
        origins.append(n - p)
    return np.asarray(origins, dtype=np.int32)


def edits_table(ys, xs, classes) -> np.ndarray:
    """The (K, 3) int32 rows ``(y0, x0, cls)`` of the Cartesian product classes x ys x xs: class-major, then iy, then ix."""
    ys, xs, classes = (np.asarray(v).reshape(-1) for v in (ys, xs, classes))
    for v, what in ((ys, "ys"), (xs, "xs"), (classes, "classes")):
        if v.size < 1 or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"edits_table: {what} must be a non-empty integer array")
    c, y, x = np.meshgrid(classes, ys, xs, indexing="ij")
    return np.stack([y.reshape(-1), x.reshape(-1), c.reshape(-1)], axis=1).astype(np.int32)


def _patch(patch) -> Tuple[int, int]:
    ph, pw = (int(patch), int(patch)) if np.ndim(patch) == 0 else (int(patch[0]), int(patch[1]))
    if ph < 1 or pw < 1:
        raise ValueError(f"a stamp of at least 1 x 1, got {ph} x {pw}")
    return ph, pw


def _edit_rows(edits) -> np.ndarray:
    e = np.asarray(edits)
    if e.ndim != 2 or e.shape[1] != 3 or e.shape[0] < 1 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"edits must be (B, 3) integer rows of (y0, x0, cls), got {e.shape} {e.dtype}")
    if e.min() < -2 ** 31 or e.max() > 2 ** 31 - 1:
        raise ValueError("edits must fit int32")
    return e.astype(np.int64)


def build_edits(shape, patch, ncls: int, classes=None, stride=None, origins=None, edits=None):
    """The table a session call sweeps, ``(edits (K, 3) int32, classes, ys, xs)``: ``classes`` x the stamp grid of both axes at
    ``stride`` (an int or (sy, sx); None = the patch) or x ``origins=(ys, xs)``, in ``edits_table``'s order -- or an explicit
    ``edits`` table, any int32 rows of ``(y0, x0, cls)`` (then classes, ys, xs are None)."""
    (H, W), (ph, pw) = shape, _patch(patch)
    if edits is not None:
        if classes is not None or stride is not None or origins is not None:
            raise ValueError("give an explicit table of edits or classes with a stride or origins, not both")
        return _edit_rows(edits).astype(np.int32), None, None, None
    c = np.asarray([] if classes is None else classes).reshape(-1)
    if c.size < 1 or not np.issubdtype(c.dtype, np.integer) or c.min() < 0 or c.max() >= ncls:
        raise ValueError(f"classes must be integers in [0, {ncls}), got {classes!r}")

    def axis(v, n: int, p: int, what: str) -> np.ndarray:
        v = np.asarray(v).reshape(-1)
        if v.size < 1 or not np.issubdtype(v.dtype, np.integer) or v.min() < 0 or v.max() > n - p:
            raise ValueError(f"{what} must be integer origins in [0, {n - p}] (stamps inside the tile)")
        return v.astype(np.int32)

    if origins is not None:
        if stride is not None:
            raise ValueError("give a stride or the origins, not both")
        ys, xs = axis(origins[0], H, ph, "origins[0]"), axis(origins[1], W, pw, "origins[1]")
    else:
        sy, sx = (ph, pw) if stride is None else _patch(stride)
        ys, xs = stamp_grid(H, ph, sy), stamp_grid(W, pw, sx)
    c = c.astype(np.int32)
    return edits_table(ys, xs, c), c, ys, xs


def stamp_mask(edit, shape: Tuple[int, int], patch) -> np.ndarray:
    """(H, W) bool: the pixels of the tile under the stamp of one row (its rectangle clipped to the tile, whatever its class)."""
    H, W = int(shape[0]), int(shape[1])
    ph, pw = _patch(patch)
    y0, x0 = int(edit[0]), int(edit[1])
    m = np.zeros((H, W), dtype=bool)
    m[min(max(y0, 0), H):min(max(y0 + ph, 0), H), min(max(x0, 0), W):min(max(x0 + pw, 0), W)] = True
    return m


# --------------------------------------------------------------------------- #
# host twins (numpy)
# --------------------------------------------------------------------------- #
def edited_maps_host(dw_t2, edits, patch, ncls: int) -> np.ndarray:
    """The (B, H, W) uint8 second class maps of the rows of ``edits``: ``cls`` under the clipped stamp when 0 <= cls < ncls."""
    dw_t2 = np.asarray(dw_t2)
    dw_t2 = dw_t2[0] if dw_t2.ndim == 3 else dw_t2
    out = np.repeat(dw_t2[None], len(edits), 0).astype(np.uint8)
    for b, e in enumerate(_edit_rows(edits)):
        if 0 <= e[2] < int(ncls):
            out[b][stamp_mask(e, dw_t2.shape, patch)] = e[2]
    return out


def pack_host(dw_t1, dw_t2, rgb, ndvi, temp, edits, patch, ncls: int, metrics: dict) -> np.ndarray:
    """The dense inputs of the placements as a (B, 2 ncls + 5, H, W) fp32 array, ``[one-hot dw_t1 | rgb | ndvi | temp | one-hot
    second map]``: the raw planes through ``scenario.normalized_planes_host``, a class id >= ncls sets no channel.
    ``dw_t2=None``: ``dw_t1``."""
    dw_t1 = np.asarray(dw_t1)
    dw_t1 = dw_t1[0] if dw_t1.ndim == 3 else dw_t1
    H, W = dw_t1.shape
    ncls = int(ncls)
    second = edited_maps_host(dw_t1 if dw_t2 is None else np.reshape(dw_t2, (H, W)), edits, patch, ncls)
    ids = np.arange(ncls, dtype=np.int64).reshape(-1, 1, 1)
    first = (dw_t1[None].astype(np.int64) == ids).astype(np.float32)
    cont = S.normalized_planes_host(np.reshape(rgb, (3, H, W)), np.reshape(ndvi, (H, W)), np.reshape(temp, (H, W)), metrics)
    return np.stack([np.concatenate([first, cont, (m[None].astype(np.int64) == ids).astype(np.float32)]) for m in second])


def result_host(out, base, edits, patch, temp_mean: float, temp_std: float, roi=None) -> np.ndarray:
    """The (B, 12) fp64 rows of ``mau_placement_result`` in plain numpy (``ROW_NAMES``): the same float32 per-pixel values, the
    sums in numpy's own order -- equal to the device's up to the rounding of a float64 sum, not bit for bit."""
    out, base = np.asarray(out, dtype=np.float32), np.asarray(base, dtype=np.float32)
    if out.ndim != 4 or out.shape[1] != 2 or base.shape != out.shape[1:]:
        raise ValueError(f"out must be (B, 2, H, W) and base (2, H, W), got {out.shape}, {base.shape}")
    B, _, H, W = out.shape
    e = _edit_rows(edits)
    if e.shape[0] != B:
        raise ValueError(f"{B} samples, {e.shape[0]} rows of edits")
    std, mean = np.float32(temp_std), np.float32(temp_mean)
    inr = np.zeros((H, W), dtype=bool) if roi is None else np.reshape(roi, (H, W)) != 0
    rows = np.empty((B, ROW), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tb = (base[1] * std).astype(np.float32) + mean                                 # two rounded fp32 operations
        for b in range(B):
            dT = (((out[b, 1] * std).astype(np.float32) + mean) - tb).astype(np.float64)
            dN = (out[b, 0] - base[0]).astype(np.float64)
            m = stamp_mask(e[b], (H, W), patch)
            part = lambda v, k: v[k].mean() if k.any() else np.nan                     # noqa: E731
            lo, hi = np.fmin.reduce(dT, axis=None, initial=np.inf), np.fmax.reduce(dT, axis=None, initial=-np.inf)
            rows[b] = [m.sum(), dT.mean(), lo, hi, part(dT, m), part(dT, ~m), inr.sum(), part(dT, inr), dN.mean(), part(dN, m),
                       part(dN, inr), (~np.isfinite(out[b])).sum()]
    return rows


# --------------------------------------------------------------------------- #
# the two launches
# --------------------------------------------------------------------------- #
def _edits_dev(edits, dev) -> torch.Tensor:
    if not (isinstance(edits, torch.Tensor) and edits.is_cuda):
        edits = _edit_rows(edits.cpu().numpy() if isinstance(edits, torch.Tensor) else edits)
    edits = const(edits, torch.int32, dev)
    if edits.dim() != 2 or edits.shape[1] != 3 or edits.shape[0] < 1:
        raise ValueError(f"edits must be (B, 3) rows of (y0, x0, cls), got {tuple(edits.shape)}")
    if edits.shape[0] > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} placements per launch, got {edits.shape[0]}")
    return edits


def _pack(dw_t1, dw_t2, rgb, ndvi, temp, edits, norm, ph: int, pw: int, ncls: int, dtype: torch.dtype, ld: int) -> Act:
    H, W = dw_t1.shape
    B = edits.shape[0]
    out = torch.empty((B, H, W, ld), dtype=dtype, device=dw_t1.device)
    call("mau_placement_pack", dw_t1.data_ptr(), None if dw_t2 is None else dw_t2.data_ptr(), rgb.data_ptr(), ndvi.data_ptr(), temp.data_ptr(),
         edits.data_ptr(), norm.data_ptr(), out.data_ptr(), ld, dtype_code(dtype), B, H, W, ph, pw, ncls, F_._stream())
    return Act(out, 2 * ncls + N_CONT)


def pack(dw_t1, dw_t2, rgb, ndvi, temp, edits, patch, ncls: int, metrics: dict, dtype: torch.dtype = torch.bfloat16,
         ld: Optional[int] = None) -> Act:
    """One launch (``mau_placement_pack``): the resident tile + B rows of ``(y0, x0, cls)`` -> the network's input ``Act``
    (B, H, W, ld).  dw_t1, dw_t2 (H,W) uint8 (``dw_t2=None``: ``dw_t1``), rgb (3,H,W) raw 0..255, ndvi (H,W), temp (H,W) raw
    degrees C, fp32, on the device; ``edits`` (B,3), a host array or an int32 device tensor -- any int32 is legal: a stamp over an
    edge is clipped, a stamp outside the tile or a class outside [0, ncls) gives the unedited tile; ``patch`` is the stamp's edge
    or (ph, pw); ``ld`` (default: 2 ncls + 5 rounded up to 8) is the channel stride.  Bit-identical to ``data.pack_tiles`` on
    ``edited_maps_host`` and ``normalized_planes_host``."""
    dw_t1, rgb, ndvi, temp = check_tile(dw_t1, rgb, ndvi, temp)
    H, W = dw_t1.shape
    if H * W > MAX_PIXELS:
        raise ValueError(f"pack: tiles of at most 2^30 pixels, got {H} x {W}")
    dw_t2 = None if dw_t2 is None else F_._dev(dw_t2, "dw_t2", torch.uint8, (H, W))
    (ph, pw), ncls = _patch(patch), check_ncls(ncls, "mau_placement_pack")
    ld = check_ld(ld, 2 * ncls + N_CONT, "pack")
    norm = const(norm_row(metrics), torch.float64, dw_t1.device)
    return _pack(dw_t1, dw_t2, rgb, ndvi, temp, _edits_dev(edits, dw_t1.device), norm, ph, pw, ncls, dtype, ld)


def _result(output, base, edits, roi, temp_mean: float, temp_std: float, ph: int, pw: int, tickets) -> torch.Tensor:
    B, _, H, W = output.shape
    rows = torch.empty((B, lib.mau_placement_row_elems()), dtype=torch.float64, device=output.device)
    ws = torch.empty(lib.mau_placement_ws_elems(B, H, W), dtype=torch.float64, device=output.device)
    call("mau_placement_result", output.data_ptr(), base.data_ptr(), edits.data_ptr(), None if roi is None else roi.data_ptr(),
         float(temp_mean), float(temp_std), rows.data_ptr(), ws.data_ptr(), tickets.data_ptr(), B, H, W, ph, pw, F_._stream())
    return rows


def result(output: torch.Tensor, base: torch.Tensor, edits, patch, temp_mean: float, temp_std: float, roi: Optional[torch.Tensor] = None,
           tickets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch (``mau_placement_result``): the head's output (B, 2, H, W) fp32 of the B placements, ``base`` (2, H, W) fp32
    of the unedited tile, ``edits`` (B, 3) and ``roi`` (H, W) uint8 (nonzero = inside) or None -> the (B, 12) fp64 rows
    (``ROW_NAMES``) on the device.  fp64 sums in a fixed order: a row does not depend on B or on its slot, and repeats bit for bit."""
    output = F_._dev(output, "output", torch.float32)
    if output.dim() != 4 or output.shape[1] != 2 or output.shape[0] < 1:
        raise ValueError(f"output must be (B, 2, H, W), got {tuple(output.shape)}")
    B, _, H, W = output.shape
    if H * W > MAX_PIXELS:
        raise ValueError(f"result: tiles of at most 2^30 pixels, got {H} x {W}")
    base = F_._dev(base, "base", torch.float32, (2, H, W))
    roi = None if roi is None else F_._dev(roi, "roi", torch.uint8, (H, W))
    ph, pw = _patch(patch)
    edits = _edits_dev(edits, output.device)
    if edits.shape[0] != B:
        raise ValueError(f"{B} samples, {edits.shape[0]} rows of edits")
    return _result(output, base, edits, roi, temp_mean, temp_std, ph, pw, F_._tickets(output.device) if tickets is None else tickets)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
class PlacementResult:
    """``rows`` (K, 12) fp64 (``ROW_NAMES``) and ``edits`` (K, 3) int32 in the order of ``edits_table`` (class-major, then iy, then
    ix) over ``classes`` x ``ys`` x ``xs``; ``ndvi``, ``temp_c`` (H, W) fp32: the forecast of the unedited tile.  Host arrays."""

    def __init__(self, rows, edits, classes, ys, xs, ndvi, temp_c):
        self.rows, self.edits, self.classes, self.ys, self.xs, self.ndvi, self.temp_c = rows, edits, classes, ys, xs, ndvi, temp_c

    def grid(self, cls: int, entry: int = 1) -> np.ndarray:
        """(ny, nx): entry ``entry`` of the rows of class ``cls``, by stamp origin."""
        if self.classes is None:
            raise ValueError("an explicit table of edits has no grid")
        at = np.flatnonzero(self.classes == int(cls))
        if at.size == 0:
            raise ValueError(f"class {cls} was not swept (classes: {self.classes.tolist()})")
        if not 0 <= int(entry) < ROW:
            raise ValueError(f"entry must be in [0, {ROW}), got {entry}")
        n = self.ys.size * self.xs.size
        return self.rows[at[0] * n:(at[0] + 1) * n, int(entry)].reshape(self.ys.size, self.xs.size)

    def best(self, cls: int, entry: int = 1) -> Tuple[int, int, float]:
        """(y0, x0, value) of the placement of class ``cls`` with the LOWEST value of ``entry`` (NaNs left out; the first on a tie)."""
        g = self.grid(cls, entry)
        if np.isnan(g).all():
            raise ValueError(f"entry {entry} of class {cls} is NaN for every placement")
        iy, ix = np.unravel_index(np.nanargmin(g), g.shape)
        return int(self.ys[iy]), int(self.xs[ix]), float(g[iy, ix])


class PlacementSession(TileSession):
    """``PlacementSession(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics=...)(classes, stride=None) -> PlacementResult``.

    The tile (device tensors: dw_t1 (H,W) uint8; rgb (3,H,W), ndvi (H,W), temp (H,W) fp32, raw values), the metadata row (1,F) and
    the temperature series (1,L) are fixed at construction, as are the stamp ``patch`` (edge or (ph, pw)), ``dw_t2`` (the second
    class map the stamps are written into; None = ``dw_t1``) and ``roi`` ((H,W) uint8, nonzero = inside; None = no region of
    interest).  ``precision``: None keeps the model's.  The session freezes the model, warms up on a side stream and captures ONE
    single-chain hipGraph for ``batch`` placements: ``mau_placement_pack`` -> the network -> ``mau_placement_result``
    (``graph=False`` runs the same three steps eagerly: the same bits).  The baseline comes from the same graph at the same batch:
    one replay with every row ``cls = -1``, sample 0 of its output copied into ``base`` (that replay's own rows, taken against the
    zeroed ``base``, are discarded).

    A call sweeps ``classes`` over the stamp grid -- ``stamp_grid`` of both axes at ``stride`` (an int or (sy, sx); None = the
    patch: stamps side by side), or ``origins=(ys, xs)`` -- in batches: a batch's rows of edits travel through pinned memory, a
    ragged last batch is padded with ``cls = -1`` rows, and the batch's rows of figures are copied device to device into the
    (K, 12) table, which is read back once at the end.  Reload weights -> build a new session."""

    def __init__(self, model: torch.nn.Module, dw_t1, rgb, ndvi, temp, metadata, temp_series, *, metrics: dict, ncls: int = 9,
                 patch=(32, 32), batch: int = 8, dw_t2=None, roi=None, precision: Optional[str] = None, graph: bool = True, warmup: int = 2):
        B = int(batch)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"batch must be in [1, {MAX_BATCH}], got {batch}")
        self.patch, self.ncls = _patch(patch), check_ncls(ncls, "mau_placement_pack")
        super().__init__(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics, B, precision=precision, dw_t2=dw_t2, roi=roi)
        self._no_edit = np.tile(np.array([[0, 0, NO_EDIT]], dtype=np.int32), (B, 1))
        self._edits = const(self._no_edit, torch.int32, self._device)
        self._base = torch.zeros((2, *self.shape), dtype=torch.float32, device=self._device)
        self._stage = PinnedStage((B, 3), torch.int32)                                  # a batch's rows of edits travel through pinned memory
        self._tickets = self._own_tickets()
        self._capture(warmup, graph)                                                    # self._out: (the network's output, the rows of figures)
        # the baseline: the same graph, the same batch, no edit
        self._replay()
        self._base.copy_(self.output[0], non_blocking=True)
        r = S.result(self.output[:1], None, self._tile[0], self._tile[0][None], self._mean, self._std)
        self.ndvi, self.temp_c = r.ndvi[0], r.temp_c[0]

    def _fit(self, H: int, W: int) -> None:
        if H * W > MAX_PIXELS:
            raise ValueError(f"PlacementSession: tiles of at most 2^30 pixels, got {H} x {W}")
        if self.patch[0] > H or self.patch[1] > W:
            raise ValueError(f"PlacementSession: a stamp of {self.patch} does not fit a tile of {H} x {W}")

    def _run(self):
        ld = pad8(2 * self.ncls + N_CONT)
        x = _pack(self._tile[0], self._dw_t2, *self._tile[1:], self._edits, self._norm, *self.patch, self.ncls, self.dtype, ld)
        out = self.model(x, self._ts, self._md)
        return out, _result(out, self._base, self._edits, self._roi, self._mean, self._std, *self.patch, self._tickets)

    @property
    def output(self) -> torch.Tensor:
        """The network's output (batch, 2, H, W) fp32 of the last replay: the session's own buffer."""
        return self._out[0]

    @property
    def base(self) -> torch.Tensor:
        """The network's output (2, H, W) fp32 for the unedited tile."""
        return self._base

    @torch.no_grad()
    def __call__(self, classes=None, stride=None, origins=None, edits=None) -> PlacementResult:
        """``edits``: an explicit (K, 3) table of ``(y0, x0, cls)`` rows instead of ``classes`` x a grid -- the rows a screening
        picked; the result then has no grid (``classes``, ``ys``, ``xs`` are None)."""
        B = self.batch
        edits, classes, ys, xs = build_edits(self.shape, self.patch, self.ncls, classes, stride, origins, edits)
        K = edits.shape[0]
        table = torch.empty((K, ROW), dtype=torch.float64, device=self._base.device)
        for k0 in range(0, K, B):
            valid = min(B, K - k0)
            self._stage.upload(np.concatenate([edits[k0:k0 + valid], self._no_edit[valid:]]), self._edits)
            self._replay()
            table[k0:k0 + valid].copy_(self._out[1][:valid], non_blocking=True)
        return PlacementResult(table.cpu().numpy(), edits, classes, ys, xs, self.ndvi.cpu().numpy(), self.temp_c.cpu().numpy())


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def _int_list(text: str) -> Sequence[int]:
    try:
        return [int(v) for v in str(text).split(",") if v.strip() != ""]
    except ValueError:
        raise ValueError(f"a comma-separated list of integers, got {text!r}") from None


def run_tile(checkpoint: str, tile: str, metrics_json: str, classes="1,6", patch: int = 32, stride: Optional[int] = None, batch: int = 8,
             roi: str = "", ncls: int = 9, precision: str = "fp16", output: str = "", device: str = "cuda", screen: int = 0) -> dict:
    """Body of the CLI: one sweep on the tile of ``tile`` (.npz: ``scenario.load_tile``'s keys; temp_orig is not used); ``roi``: a
    .npy (H, W) mask.  Returns -- and with ``output`` writes as .npz -- rows, edits, classes, ys, xs, ``grid_c<cls>_e<entry>`` per
    class for entries 1, 4 and 7, and the unedited forecast ndvi, temp_c.

    ``screen = N > 0``: the whole grid is screened from one input gradient (``screening.ScreeningSession``, the objective
    "temperature over the roi, else the tile") and only the N candidates per class with the most negative predicted change are swept
    exactly.  The result then holds ``edits`` (all candidates), ``predicted`` (their (P, 4) screening rows), ``pred_grid_c<cls>``,
    ``screened_index`` / ``screened_edits`` (class-major, best first), ``screened_rows`` (their exact (n, 12) rows), ``best`` (per
    class, the screened candidate with the lowest exact mean dT over the roi, else the tile) and ``spearman``: the rank correlation of
    the predicted change with that exact figure over the swept subset."""
    t = S.load_tile(tile, metrics_json, device=device, checkpoint=checkpoint, ncls=ncls)
    cls = _int_list(classes) if isinstance(classes, str) else list(classes)
    mask = torch.from_numpy((np.load(roi) != 0).astype(np.uint8).reshape(tuple(t.dw.shape))).to(device) if roi else None
    if int(screen) < 0:
        raise ValueError(f"--screen takes a number of candidates per class, got {screen}")
    if screen:
        from . import screening
        scr = screening.ScreeningSession(*t[:7], metrics=t.metrics, ncls=ncls, patch=patch, objectives=(("temp", mask),), dw_t2=t.dw_t2,
                                         precision=precision)
        p = scr(cls, stride=stride)
        pick = np.concatenate([p.top_index(screen, 0, c) for c in p.classes])
        sess = PlacementSession(*t[:7], metrics=t.metrics, ncls=ncls, patch=patch, batch=batch, dw_t2=t.dw_t2, roi=mask, precision=precision)
        r = sess(edits=p.edits[pick])
        exact = r.rows[:, 7 if roi else 1]
        res = {"edits": p.edits, "classes": p.classes, "ys": p.ys, "xs": p.xs, "ndvi": r.ndvi, "temp_c": r.temp_c, "predicted": p.rows[0],
               "screened_index": pick, "screened_edits": r.edits, "screened_rows": r.rows,
               "spearman": np.float64(screening.spearman(p.rows[0, pick, 2], exact)),
               **{f"pred_grid_c{c}": p.grid(c) for c in p.classes}}
        best = []
        for c in p.classes:
            at = np.flatnonzero(r.edits[:, 2] == c)
            k = at[np.nanargmin(exact[at])] if at.size and not np.isnan(exact[at]).all() else None
            best.append([np.nan] * 3 if k is None else [r.edits[k, 0], r.edits[k, 1], exact[k]])
        res["best"] = np.array(best, dtype=np.float64)
        if output:
            np.savez(output, **res)
        return res
    sess = PlacementSession(*t[:7], metrics=t.metrics, ncls=ncls, patch=patch, batch=batch, dw_t2=t.dw_t2, roi=mask, precision=precision)
    r = sess(cls, stride=stride)
    res = {"rows": r.rows, "edits": r.edits, "classes": r.classes, "ys": r.ys, "xs": r.xs, "ndvi": r.ndvi, "temp_c": r.temp_c,
           **{f"grid_c{c}_e{e}": r.grid(c, e) for c in r.classes for e in GRID_ENTRIES}}
    res["best"] = np.array([r.best(c, 1) for c in r.classes], dtype=np.float64)
    if output:
        np.savez(output, **res)
    return res


def _cli():
    import typer
    app = typer.Typer(add_completion=False)

    @app.command()
    def main(checkpoint: str = typer.Argument(..., help="reference-layout .pth (src/train.py:303-316)"),
             tile: str = typer.Option(..., help=".npz: dw, rgb, ndvi, temp, metadata_raw [, dw_t2, temp_series]"),
             metrics_json: str = typer.Option(..., help="normalization_metrics.json"),
             classes: str = typer.Option("1,6", help="land-cover classes to place, comma separated"),
             patch: int = 32, stride: int = typer.Option(-1, help="pixels between stamp origins; -1 = the patch"), batch: int = 8,
             roi: str = typer.Option("", help=".npy (H, W) mask of a region of interest"), ncls: int = 9, precision: str = "fp16",
             output: str = "", device: str = "gpu",
             screen: int = typer.Option(0, help="N > 0: screen the grid from one input gradient, sweep only the N best candidates per class")):
        """Where on a tile does a block of one land-cover class change the forecast temperature most?"""
        dev = F_.typer_device(device)
        try:
            res = run_tile(checkpoint, tile, metrics_json, classes, patch, None if stride < 0 else stride, batch, roi, ncls, precision, output, dev,
                           screen)
        except ValueError as e:
            raise typer.BadParameter(str(e))
        ny, nx = len(res["ys"]), len(res["xs"])
        if screen:
            n = res["screened_rows"].shape[0]
            typer.echo(f"tile {res['ndvi'].shape[0]} x {res['ndvi'].shape[1]}: {len(res['classes'])} classes x {ny} x {nx} stamps of {patch} screened "
                       f"from one gradient, {n} swept exactly in {-(-n // batch)} batches of {batch}")
            typer.echo(f"Spearman rank correlation of predicted and exact change over the {n} swept: {float(res['spearman']):.4f}")
            for c, (y0, x0, v) in zip(res["classes"], res["best"]):
                typer.echo(f"class {int(c)}: lowest exact mean_dt{'_roi' if roi else ''} among the screened {v:.6g} at (y0, x0) = ({int(y0)}, {int(x0)})")
            if output:
                typer.echo(f"Saved placement result to {output}")
            return
        K = res["rows"].shape[0]
        typer.echo(f"tile {res['ndvi'].shape[0]} x {res['ndvi'].shape[1]}: {len(res['classes'])} classes x {ny} x {nx} stamps of {patch}, "
                   f"{-(-K // batch)} batches of {batch}")
        for c, (y0, x0, v) in zip(res["classes"], res["best"]):
            typer.echo(f"class {int(c)}: lowest mean_dt {v:.6g} at (y0, x0) = ({int(y0)}, {int(x0)})")
        if output:
            typer.echo(f"Saved placement result to {output}")

    return app


if __name__ == "__main__":
    _cli()()
