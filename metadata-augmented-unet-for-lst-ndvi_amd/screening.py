"""Placement screening: every candidate stamp ranked from ONE input gradient, on the device.

``placement`` answers "where does a block of trees cool most" by brute force: one forward per candidate.  The network's input is
one-hot, so a stamp of class ``c`` changes exactly two channels of a pixel of the second class block by +-1, and its first-order
effect on a scalar objective is a plain sum of input-gradient entries over the stamp's rectangle -- no step size to choose.  One
forward and one data-gradient-only backward at the *linearisation point* (the resident tile, as ``mau_placement_pack`` writes it
with every row ``cls = -1``) therefore rank all candidates at once; the exact ``PlacementSession`` then verifies the best few.

Definitions (include/mau_hip.h states them for the kernels):

* objective k: a channel (``"temp"`` = 1, degrees C; ``"ndvi"`` = 0) and an optional roi plane (H, W) uint8, nonzero = inside; J_k
  is the mean of the forecast over the roi (no plane: the tile), n_k the roi's pixel count;
* seed: ``dout[k, ch_k, p] = seed_scale * [p in roi_k]``, the other channel 0; ``seed_scale`` is a positive power of two that moves
  fp16 gradients away from overflow or underflow and is undone exactly in the coefficient;
* gradient ``G`` (K, H, W, ld) in the activation type: of ``sum_k <dout_k, out_k>`` with respect to the packed input of K copies;
* swap term ``s_k(p, c) = G[k,p,off+c] - (cur(p) < ncls ? G[k,p,off+cur(p)] : 0)`` in fp64, ``cur = dw_t2``, ``off = ncls + 5``;
* coefficient ``coef_k = (ch_k == 1 ? temp_std : 1) / (seed_scale * n_k)`` in fp64, applied once, after the sum.

``mau_screen_seed``, ``mau_screen_rows`` and ``mau_screen_maps`` are one launch each; ``ScreeningSession`` runs the network once,
eagerly (one call per linearisation point; capturing an autograd backward is ``GraphedTrainStep``'s own machinery), and a call is
then one launch and one read-back whatever the number of candidates.  The host twins are pure numpy and sum in the device's order.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from . import placement as P
from ._tile import N_CONT, check_metrics, check_ncls, check_tile, const, norm_row
from .functional import _dev, call, dtype_code, lib, pad8

ROW = 4
ROW_NAMES = ("stamp_pixels", "changed_pixels", "predicted", "non_finite")
CHANNELS = {"ndvi": 0, "temp": 1}
MAX_OBJECTIVES = 65535


def second_block(ncls: int) -> int:
    """The channel offset of the second one-hot block of a packed input: ``[one-hot dw_t1 | rgb, ndvi, temp | one-hot second map]``."""
    return int(ncls) + N_CONT


# --------------------------------------------------------------------------- #
# argument checks
# --------------------------------------------------------------------------- #
def _scale(seed_scale) -> float:
    s = float(seed_scale)
    if not (s > 0.0 and math.isfinite(s)) or math.frexp(s)[0] != 0.5 or not -125 <= math.frexp(s)[1] <= 128:
        raise ValueError(f"seed_scale must be a positive power of two (a normal float), got {seed_scale!r}")
    return s


def _objs(objs, R: int) -> np.ndarray:
    """(K, 2) integer rows of (channel, roi index or -1), checked against ``R`` roi planes."""
    o = np.asarray(objs)
    if o.ndim != 2 or o.shape[1] != 2 or not 1 <= o.shape[0] <= MAX_OBJECTIVES or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f"objectives must be (K, 2) integer rows of (channel, roi index or -1), 1 <= K <= {MAX_OBJECTIVES}, got {o.shape} {o.dtype}")
    if not np.isin(o[:, 0], (0, 1)).all():
        raise ValueError(f"an objective's channel is 0 (NDVI) or 1 (temperature), got {o[:, 0].tolist()}")
    if o[:, 1].min() < -1 or o[:, 1].max() >= R:
        raise ValueError(f"an objective names a roi plane that is not there: indices {o[:, 1].tolist()}, {R} planes")
    return o.astype(np.int32)


def _shape(shape) -> Tuple[int, int]:
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1 or int(shape[0]) * int(shape[1]) > P.MAX_PIXELS:
        raise ValueError(f"a tile of (H, W), 1 to 2^30 pixels, got {tuple(shape)}")
    return int(shape[0]), int(shape[1])


def _g64(G) -> np.ndarray:
    """The gradient's values as float64 (exact for fp32, bf16 and fp16), (K, H, W, C)."""
    g = G.detach().cpu().double().numpy() if isinstance(G, torch.Tensor) else np.asarray(G).astype(np.float64)
    if g.ndim != 4:
        raise ValueError(f"G must be (K, H, W, channels), got {g.shape}")
    return g


def _host_args(G, dw_t2, counts, objs, ncls: int, seed_scale):
    g = _g64(G)
    K, H, W, C = g.shape
    ncls = int(ncls)
    if not 1 <= ncls <= 16 or C < 2 * ncls + N_CONT:
        raise ValueError(f"1 to 16 classes and at least 2 ncls + {N_CONT} channels, got ncls {ncls}, {C} channels")
    cur = np.asarray(dw_t2)
    if cur.shape != (H, W) or cur.dtype != np.uint8:
        raise ValueError(f"dw_t2 must be ({H}, {W}) uint8, got {cur.shape} {cur.dtype}")
    n = np.asarray(counts, dtype=np.float64).reshape(-1)
    o = _objs(objs, 1 << 30)
    if n.shape != (K,) or o.shape[0] != K:
        raise ValueError(f"{K} objectives in G, {n.size} counts, {o.shape[0]} rows of objectives")
    return g, cur.astype(np.int64), n, o, ncls, _scale(seed_scale)


def _coef(ch: int, n: float, temp_std: float, seed_scale: float) -> np.float64:
    with np.errstate(divide="ignore"):
        return (np.float64(temp_std) if ch == 1 else np.float64(1.0)) / (np.float64(seed_scale) * np.float64(n))


# --------------------------------------------------------------------------- #
# host twins (numpy)
# --------------------------------------------------------------------------- #
def seed_host(objs, rois, shape, seed_scale: float = 1.0):
    """``mau_screen_seed`` in numpy: (dout (K, 2, H, W) float32, counts (K,) float64)."""
    H, W = _shape(shape)
    rois = None if rois is None else np.asarray(rois)
    if rois is not None and (rois.ndim != 3 or rois.shape[1:] != (H, W) or rois.dtype != np.uint8):
        raise ValueError(f"rois must be (R, {H}, {W}) uint8, got {rois.shape} {rois.dtype}")
    o, s = _objs(objs, 0 if rois is None else rois.shape[0]), _scale(seed_scale)
    dout = np.zeros((o.shape[0], 2, H, W), dtype=np.float32)
    counts = np.empty(o.shape[0], dtype=np.float64)
    for k, (ch, r) in enumerate(o):
        inside = np.ones((H, W), dtype=bool) if r < 0 else rois[r] != 0
        dout[k, ch][inside] = np.float32(s)
        counts[k] = inside.sum()
    return dout, counts


def _block_join(acc: np.ndarray) -> np.float64:
    """The sum of the 256 threads' values in the device's order: xor butterfly 32..1 over the lanes of a wave, the waves in order."""
    a = acc.reshape(4, 64)
    lane = np.arange(64)
    s = 32
    while s:
        a = a + a[:, lane ^ s]
        s >>= 1
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def rows_host(G, dw_t2, edits, counts, objs, patch, ncls: int, temp_std: float, seed_scale: float = 1.0) -> np.ndarray:
    """``mau_screen_rows`` in numpy: the (K, P, 4) float64 rows (``ROW_NAMES``), summed in the device's order -- slot i of the
    unclipped rectangle belongs to thread i % 256, a thread adds its slots in increasing i and skips a slot outside the tile, then
    the butterfly and the waves -- so the rows agree with the device's bit for bit."""
    g, cur, n, o, ncls, s = _host_args(G, dw_t2, counts, objs, ncls, seed_scale)
    K, H, W, _ = g.shape
    (ph, pw), off, e = P._patch(patch), second_block(ncls), P._edit_rows(edits)
    rows = np.zeros((K, e.shape[0], ROW), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, (y0, x0, cls) in enumerate(e.tolist()):
            r = np.arange(max(0, -y0), min(ph, H - y0), dtype=np.int64)
            c = np.arange(max(0, -x0), min(pw, W - x0), dtype=np.int64)
            rows[:, j, 0] = r.size * c.size
            live = 0 <= cls < ncls
            for k in range(K):
                rows[k, j, 2] = 0.0 if n[k] > 0 else np.nan
            if not live or r.size * c.size == 0:
                continue
            slot = (r[:, None] * pw + c[None, :]).reshape(-1)                         # ascending
            y, x = np.broadcast_to(y0 + r[:, None], (r.size, c.size)).reshape(-1), np.broadcast_to(x0 + c[None, :], (r.size, c.size)).reshape(-1)
            was = cur[y, x]
            has = was < ncls
            rows[:, j, 1] = (was != cls).sum()
            step, thread = slot // 256, slot % 256
            bounds = np.flatnonzero(np.diff(step, prepend=step[0] - 1))               # the first slot of every step that holds one
            for k in range(K):
                a, b = g[k, y, x, off + cls], g[k, y, x, off + np.where(has, was, 0)]
                term = a - np.where(has, b, 0.0)
                acc = np.zeros(256, dtype=np.float64)
                for lo, hi in zip(bounds, list(bounds[1:]) + [slot.size]):
                    acc[thread[lo:hi]] = acc[thread[lo:hi]] + term[lo:hi]
                rows[k, j, 3] = (~np.isfinite(a)).sum() + (has & ~np.isfinite(b)).sum()
                if n[k] > 0:
                    rows[k, j, 2] = _coef(o[k, 0], n[k], temp_std, s) * _block_join(acc)
    return rows


def maps_host(G, dw_t2, counts, objs, k: int, ncls: int, temp_std: float, seed_scale: float = 1.0) -> np.ndarray:
    """``mau_screen_maps`` in numpy: (ncls, H, W) float32, ``fl32(coef_k * s_k(p, c))``; NaN everywhere when n_k == 0."""
    g, cur, n, o, ncls, s = _host_args(G, dw_t2, counts, objs, ncls, seed_scale)
    if not 0 <= int(k) < g.shape[0]:
        raise ValueError(f"objective {k} of {g.shape[0]}")
    off, has = second_block(ncls), cur < ncls
    gcur = np.where(has, np.take_along_axis(g[k], (off + np.where(has, cur, 0))[..., None], axis=2)[..., 0], 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if not n[k] > 0:
            return np.full((ncls, *cur.shape), np.nan, dtype=np.float32)
        coef = _coef(o[k, 0], n[k], temp_std, s)
        return np.stack([(coef * (g[k, :, :, off + c] - gcur)).astype(np.float32) for c in range(ncls)])


# --------------------------------------------------------------------------- #
# the three launches
# --------------------------------------------------------------------------- #
def _objs_dev(objs, R: int, dev) -> torch.Tensor:
    if isinstance(objs, torch.Tensor):
        objs = objs.cpu().numpy()
    return const(_objs(objs, R), torch.int32, dev)


def _gradient(G: torch.Tensor, ncls: int, who: str):
    """A (K, H, W, C) device tensor or channel-sliced view of one in an activation type -> (K, H, W, its pixel stride)."""
    if not isinstance(G, torch.Tensor):
        raise TypeError(f"{who}: G must be a torch tensor on the device, got {type(G).__name__}")
    F_._require_cuda(G, f"{who}: G")
    dtype_code(G.dtype)
    if G.dim() != 4 or G.numel() == 0 or G.shape[3] < 2 * ncls + N_CONT:
        raise ValueError(f"{who}: G must be (K, H, W, >= {2 * ncls + N_CONT}), got {tuple(G.shape)}")
    K, H, W, _ = G.shape
    ld = G.stride(2)
    if G.stride(3) != 1 or ld < G.shape[3] or G.stride(1) != W * ld or G.stride(0) != H * W * ld:
        raise ValueError(f"{who}: G must be dense but for its channel stride, got shape {tuple(G.shape)} strides {G.stride()}")
    if not 1 <= K <= MAX_OBJECTIVES or H * W > P.MAX_PIXELS:
        raise ValueError(f"{who}: 1 to {MAX_OBJECTIVES} objectives and tiles of at most 2^30 pixels, got {tuple(G.shape)}")
    return K, H, W, ld


def seed(objs, rois: Optional[torch.Tensor], shape, seed_scale: float = 1.0, device="cuda"):
    """One launch (``mau_screen_seed``): the objective table ``objs`` (K, 2) of (channel, roi index or -1) and the roi planes
    ``rois`` (R, H, W) uint8 on the device (None: no row names one) -> (dout (K, 2, H, W) fp32, counts (K,) fp64) on the device."""
    H, W = _shape(shape)
    rois = None if rois is None else _dev(rois, "rois", torch.uint8)
    if rois is not None and (rois.dim() != 3 or tuple(rois.shape[1:]) != (H, W)):
        raise ValueError(f"rois must be (R, {H}, {W}), got {tuple(rois.shape)}")
    dev = rois.device if rois is not None else torch.device(device)
    o, s = _objs_dev(objs, 0 if rois is None else rois.shape[0], dev), _scale(seed_scale)
    return _seed(o, rois, H, W, s)


def _seed(objs: torch.Tensor, rois, H: int, W: int, seed_scale: float):
    K = objs.shape[0]
    dout = torch.empty((K, 2, H, W), dtype=torch.float32, device=objs.device)
    counts = torch.empty(K, dtype=torch.float64, device=objs.device)
    call("mau_screen_seed", objs.data_ptr(), None if rois is None else rois.data_ptr(), 0 if rois is None else rois.shape[0], seed_scale,
         dout.data_ptr(), counts.data_ptr(), K, H, W, F_._stream())
    return dout, counts


def _table_args(G, dw_t2, counts, objs, ncls, seed_scale, who):
    ncls = check_ncls(ncls, who)
    K, H, W, ld = _gradient(G, ncls, who)
    dw_t2 = _dev(dw_t2, "dw_t2", torch.uint8, (H, W))
    counts = _dev(counts, "counts", torch.float64, (K,))
    objs = _objs_dev(objs, 1 << 30, G.device)
    if objs.shape[0] != K:
        raise ValueError(f"{who}: {K} objectives in G, {objs.shape[0]} rows of objectives")
    return ncls, K, H, W, ld, dw_t2, counts, objs, _scale(seed_scale)


def rows(G: torch.Tensor, dw_t2, edits, counts, objs, patch, ncls: int, temp_std: float, seed_scale: float = 1.0) -> torch.Tensor:
    """One launch (``mau_screen_rows``): the gradient ``G`` (K, H, W, C) -- or a channel-sliced view of a wider tensor -- in fp32,
    bf16 or fp16, the second class map ``dw_t2`` (H, W) uint8 of the linearisation point, ``edits`` (P, 3) rows of ``(y0, x0, cls)``
    (a host array or an int32 device tensor; any int32 is legal), ``counts`` (K,) fp64 and ``objs`` (K, 2) as ``seed`` gives and
    takes them -> the (K, P, 4) fp64 rows (``ROW_NAMES``) on the device.  A row's bits depend on its own table row, its objective
    and the tile alone, and repeat."""
    ncls, K, H, W, ld, dw_t2, counts, objs, s = _table_args(G, dw_t2, counts, objs, ncls, seed_scale, "mau_screen_rows")
    edits = const(P._edit_rows(edits.cpu().numpy() if isinstance(edits, torch.Tensor) else edits), torch.int32, G.device)
    return _rows(G, ld, dw_t2, edits, counts, objs, float(temp_std), s, P._patch(patch), ncls)


def _rows(G, ld, dw_t2, edits, counts, objs, temp_std, seed_scale, patch, ncls) -> torch.Tensor:
    K, H, W, _ = G.shape
    out = torch.empty((K, edits.shape[0], lib.mau_screen_row_elems()), dtype=torch.float64, device=G.device)
    call("mau_screen_rows", G.data_ptr(), ld, dtype_code(G.dtype), dw_t2.data_ptr(), edits.data_ptr(), counts.data_ptr(), objs.data_ptr(),
         temp_std, seed_scale, out.data_ptr(), K, edits.shape[0], H, W, *patch, ncls, F_._stream())
    return out


def maps(G: torch.Tensor, dw_t2, counts, objs, k: int, ncls: int, temp_std: float, seed_scale: float = 1.0) -> torch.Tensor:
    """One launch (``mau_screen_maps``): for objective ``k``, the (ncls, H, W) fp32 maps ``coef_k * s_k(p, c)`` on the device --
    what every pixel would do as class c."""
    ncls, K, H, W, ld, dw_t2, counts, objs, s = _table_args(G, dw_t2, counts, objs, ncls, seed_scale, "mau_screen_maps")
    if not 0 <= int(k) < K:
        raise ValueError(f"objective {k} of {K}")
    out = torch.empty((ncls, H, W), dtype=torch.float32, device=G.device)
    call("mau_screen_maps", G.data_ptr(), ld, dtype_code(G.dtype), dw_t2.data_ptr(), counts.data_ptr(), objs.data_ptr(), float(temp_std), s,
         out.data_ptr(), int(k), K, H, W, ncls, F_._stream())
    return out


# --------------------------------------------------------------------------- #
# the result and the session
# --------------------------------------------------------------------------- #
class ScreeningResult:
    """``rows`` (K, P, 4) fp64 (``ROW_NAMES``) per objective and ``edits`` (P, 3) int32; with a grid sweep ``classes``, ``ys``, ``xs``
    in the order of ``placement.edits_table`` (an explicit table: None).  Host arrays."""

    def __init__(self, rows, edits, classes=None, ys=None, xs=None):
        self.rows, self.edits, self.classes, self.ys, self.xs = rows, edits, classes, ys, xs

    def grid(self, cls: int, k: int = 0, entry: int = 2) -> np.ndarray:
        """(ny, nx): entry ``entry`` of objective ``k`` of the rows of class ``cls``, by stamp origin."""
        if self.classes is None:
            raise ValueError("an explicit table of edits has no grid")
        at = np.flatnonzero(self.classes == int(cls))
        if at.size == 0:
            raise ValueError(f"class {cls} was not screened (classes: {self.classes.tolist()})")
        if not 0 <= int(entry) < ROW or not 0 <= int(k) < self.rows.shape[0]:
            raise ValueError(f"entry must be in [0, {ROW}) and k in [0, {self.rows.shape[0]}), got {entry}, {k}")
        n = self.ys.size * self.xs.size
        return self.rows[int(k), at[0] * n:(at[0] + 1) * n, int(entry)].reshape(self.ys.size, self.xs.size)

    def top_index(self, n: int, k: int = 0, cls: Optional[int] = None, sign: int = -1) -> np.ndarray:
        """Table indices of the ``n`` rows (of class ``cls``; None: of any) with the most negative (``sign = -1``) or most positive
        (``sign = +1``) predicted change of objective ``k``; ties go to the lower table index, NaN rows come last."""
        if int(n) < 0 or sign not in (-1, 1) or not 0 <= int(k) < self.rows.shape[0]:
            raise ValueError(f"n >= 0, sign -1 or +1 and k in [0, {self.rows.shape[0]}), got {n}, {sign}, {k}")
        at = np.arange(self.edits.shape[0]) if cls is None else np.flatnonzero(self.edits[:, 2] == int(cls))
        v = self.rows[int(k), at, 2]
        nan = np.isnan(v)
        key = np.where(nan, 0.0, v if sign == -1 else -v)
        return at[np.lexsort((key, nan))][:int(n)]                                     # (a stable sort: by NaN-ness, then by value)

    def top(self, n: int, k: int = 0, cls: Optional[int] = None, sign: int = -1) -> np.ndarray:
        """The ``n`` edits ``(y0, x0, cls)`` of ``top_index``, (<= n, 3) int32."""
        return self.edits[self.top_index(n, k, cls, sign)]


def _objectives(objectives) -> Tuple[np.ndarray, list]:
    """``(("temp" | "ndvi", roi plane or None), ...)`` -> the (K, 2) table and the list of the planes it names."""
    table, planes = [], []
    try:
        items = [(str(name), roi) for name, roi in objectives]
    except (TypeError, ValueError):
        raise ValueError("objectives must be pairs of (\"temp\" | \"ndvi\", roi plane or None)") from None
    if not 1 <= len(items) <= MAX_OBJECTIVES:
        raise ValueError(f"1 to {MAX_OBJECTIVES} objectives, got {len(items)}")
    for name, roi in items:
        if name not in CHANNELS:
            raise ValueError(f"an objective is \"temp\" or \"ndvi\", got {name!r}")
        table.append((CHANNELS[name], -1 if roi is None else len(planes)))
        if roi is not None:
            planes.append(roi)
    return np.asarray(table, dtype=np.int32), planes


class _ModelState:
    """What a linearisation changes on the model for its one run, put back on exit: every module's ``training`` flag, every block's
    frozen inference caches (the very objects: a captured session of the same model keeps reading them), the precision and every
    parameter's ``requires_grad``.  Inside: eval mode, un-frozen (a frozen convolution saves nothing for a backward), parameters out
    of the graph -- the backward is data gradients only."""

    def __init__(self, model: torch.nn.Module, precision: Optional[str]):
        self.model, self.net, self.precision = model, getattr(model, "model", model), precision

    def __enter__(self):
        # every snapshot first (a model without ``_rt`` fails here, untouched), then the changes, undone if one of them raises
        self.was = self.net._rt.precision
        self.training = [(m, m.training) for m in self.model.modules()]
        self.frozen = [(m, m._frozen) for m in self.model.modules() if hasattr(m, "_frozen")]
        self.needs = [(p, p.requires_grad) for p in self.model.parameters()]
        try:
            if self.precision is not None:
                self.net._rt.precision = self.precision
            for m, _ in self.training:
                m.training = False
            for m, _ in self.frozen:
                m._frozen = None
            for p, _ in self.needs:
                p.requires_grad_(False)
            return self.net._rt.dtype
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        self.net._rt.precision = self.was
        for m, f in self.frozen:
            m._frozen = f
        for m, t in self.training:
            m.training = t
        for p, r in self.needs:
            p.requires_grad_(r)
        return False


class ScreeningSession:
    """``ScreeningSession(model, dw_t1, rgb, ndvi, temp, metadata, temp_series, metrics=...)(classes, stride=None) -> ScreeningResult``.

    The tile, the metadata row and the temperature series are ``PlacementSession``'s; ``objectives`` are pairs of ``"temp"`` or
    ``"ndvi"`` and an (H, W) uint8 roi plane on the device (nonzero = inside) or None (the whole tile).  The constructor keeps the
    tile resident, packs K = ``len(objectives)`` copies through ``mau_placement_pack`` with every row ``cls = -1``, and runs the
    network ONCE, eagerly: eval mode with saved tensors, ``torch.autograd.grad`` of the output with respect to the packed input with
    ``grad_outputs = dout`` of ``mau_screen_seed``.  For that run the model is un-frozen and its parameters are taken out of the graph
    (no weight-gradient launch, no ``.grad``); afterwards its ``training`` flags, frozen caches, precision and ``requires_grad`` are
    as they were.  ``precision``: None = the model's own.  A call builds the table of edits as ``PlacementSession`` does
    (``classes`` x the stamp grid at ``stride``, ``origins=(ys, xs)``, or an explicit ``edits`` table) and is ONE launch and one
    read-back, whatever the number of rows.  ``set_dw_t2`` moves the linearisation point and runs the network again."""

    def __init__(self, model: torch.nn.Module, dw_t1, rgb, ndvi, temp, metadata, temp_series, *, metrics: dict, ncls: int = 9,
                 patch=32, objectives: Sequence = (("temp", None),), precision: Optional[str] = None, dw_t2=None, seed_scale: float = 1.0):
        if getattr(getattr(model, "model", model), "deep_supervision", False):
            raise ValueError("screening needs a single output: deep_supervision=True is not supported")
        self.patch, self.ncls, self.seed_scale = P._patch(patch), check_ncls(ncls, "mau_screen_rows"), _scale(seed_scale)
        table, planes = _objectives(objectives)
        if precision is not None and precision not in ("bf16", "fp16", "fp32"):
            raise ValueError(f"precision must be bf16, fp16 or fp32, got {precision!r}")
        check_metrics(metrics)
        tile = check_tile(dw_t1, rgb, ndvi, temp)
        for t, what in ((metadata, "metadata"), (temp_series, "temp_series")):
            F_._require_cuda(t, f"ScreeningSession({what})")
        self.shape, self._device, self.K = tuple(tile[0].shape), tile[0].device, table.shape[0]
        H, W = self.shape
        if H * W > P.MAX_PIXELS or self.patch[0] > H or self.patch[1] > W:
            raise ValueError(f"ScreeningSession: a stamp of {self.patch} on a tile of {H} x {W} (at most 2^30 pixels)")
        self.model, self.precision = model, precision
        self._tile = tuple(t.detach().clone() for t in tile)
        self._rois = torch.stack([_dev(r, "roi", torch.uint8, self.shape) for r in planes]) if planes else None
        self._objs = const(table, torch.int32, self._device)
        self._norm = const(norm_row(metrics), torch.float64, self._device)
        self._mean, self._std = float(metrics["temp_mean"]), float(metrics["temp_std"])
        self._md = metadata.detach().float().reshape(1, -1).expand(self.K, -1).contiguous()
        self._ts = temp_series.detach().float().reshape(1, -1).expand(self.K, -1).contiguous()
        self._no_edit = const(np.tile(np.array([[0, 0, P.NO_EDIT]], dtype=np.int32), (self.K, 1)), torch.int32, self._device)
        self.set_dw_t2(dw_t2)

    def set_dw_t2(self, dw_t2) -> None:
        """Another second class map (None: ``dw_t1``) -- a new linearisation point: one forward, one backward."""
        self._dw_t2 = self._tile[0] if dw_t2 is None else _dev(dw_t2, "dw_t2", torch.uint8, self.shape).detach().clone()
        H, W = self.shape
        with _ModelState(self.model, self.precision) as dtype:
            self.dtype = dtype
            self.dout, self.counts = _seed(self._objs, self._rois, H, W, self.seed_scale)
            x = P._pack(self._tile[0], self._dw_t2, *self._tile[1:], self._no_edit, self._norm, *self.patch, self.ncls, dtype,
                        pad8(2 * self.ncls + N_CONT))
            x.t.requires_grad_(True)
            with torch.enable_grad():
                out = self.model(x, self._ts, self._md)
                (g,) = torch.autograd.grad(out, x.t, grad_outputs=self.dout)
        self.output, self.gradient = out.detach(), g.detach()

    def _table(self, edits: np.ndarray) -> np.ndarray:
        dev_edits = const(edits, torch.int32, self._device)
        K, H, W, _ = self.gradient.shape
        ld = self.gradient.stride(2)
        return _rows(self.gradient, ld, self._dw_t2, dev_edits, self.counts, self._objs, self._std, self.seed_scale, self.patch, self.ncls).cpu().numpy()

    def __call__(self, classes=None, stride=None, origins=None, edits=None) -> ScreeningResult:
        edits, classes, ys, xs = P.build_edits(self.shape, self.patch, self.ncls, classes, stride, origins, edits)
        return ScreeningResult(self._table(edits), edits, classes, ys, xs)

    def maps(self, k: int = 0) -> np.ndarray:
        """(ncls, H, W) fp32: what every pixel would do to objective ``k`` as class c, ``coef_k * s_k(p, c)``.  A host array."""
        return maps(self.gradient, self._dw_t2, self.counts, self._objs, k, self.ncls, self._std, self.seed_scale).cpu().numpy()


def spearman(a, b) -> float:
    """Spearman's rank correlation of two vectors in plain numpy (average ranks on ties; pairs with a NaN are left out; NaN when
    fewer than two pairs remain or one side is constant)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError(f"two vectors of one length, got {a.shape}, {b.shape}")
    ok = ~(np.isnan(a) | np.isnan(b))
    a, b = a[ok], b[ok]

    def rank(v):
        order = np.argsort(v, kind="stable")
        r = np.empty(v.size, dtype=np.float64)
        r[order] = np.arange(v.size, dtype=np.float64)
        for val in np.unique(v):                                                       # ties: the mean of their ranks
            m = v == val
            r[m] = r[m].mean()
        return r

    if a.size < 2:
        return float("nan")
    ra, rb = rank(a) - (a.size - 1) / 2, rank(b) - (b.size - 1) / 2
    den = math.sqrt(float((ra * ra).sum()) * float((rb * rb).sum()))
    return float((ra * rb).sum() / den) if den > 0 else float("nan")
