"""Plain references of the streaming spatial operators (csrc/spatial.hip), numpy / torch on the CPU, no GPU.

Bilinear resize, align_corners=True: ``resize_tables`` is the host twin of the kernels' ``ac_scale`` / ``ac_src`` -- the same IEEE
float32 operations, each rounded on its own -- and ``resize_fwd_ref`` evaluates ``lerp4`` the same way (numpy never contracts a
multiply and an add into an FMA: they are separate ufunc calls).  For float32 data it is therefore a BIT-EXACT oracle of every
forward kernel, and for the 16-bit types too once input and result are rounded with torch's conversion (round to nearest even, what
the kernels' conversions do).  The adjoint is accumulated in float64 from the same float32 tables and comes with the quantities its
error bound is made of.  Pool, broadcast, copy and flip are index arithmetic."""
import numpy as np
import torch

F32 = np.float32


def pad8(c):
    return (c + 7) // 8 * 8


# ---- bilinear, align_corners=True -------------------------------------------------------------------------------------------
def resize_tables(n_in, n_out):
    """(i0, i1, l0, l1) per destination index: scale = (in-1)/(out-1) in float32 (0 when out == 1), s = fl(scale * dst), i0 = (int)s
    clamped to in-1, i1 = i0 + (i0 < in-1), l1 = fl(s - i0), l0 = fl(1 - l1)."""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)
    assert isinstance(scale, np.float32)
    s = scale * np.arange(n_out, dtype=F32)
    assert s.dtype == F32
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(F32)
    l0 = F32(1.0) - l1
    assert l0.dtype == F32 and l1.dtype == F32
    return i0, i1, l0, l1


def _round_to(x, dtype):
    """float32 numpy array -> the values of ``dtype`` (torch's conversion), as float32"""
    if dtype == torch.float32:
        return np.ascontiguousarray(x, dtype=F32)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(dtype).float().numpy()


def resize_fwd_ref(x, H, W, dtype=torch.float32):
    """x (N, C, h, w) -> (N, C, H, W) float32 numpy: ly0*(lx0*v00 + lx1*v01) + ly1*(lx0*v10 + lx1*v11) in float32, every operation
    rounded separately; input and result rounded to ``dtype``."""
    x = _round_to(np.asarray(x, dtype=F32), dtype)
    h, w = x.shape[2:]
    y0, y1, ly0, ly1 = resize_tables(h, H)
    x0, x1, lx0, lx1 = resize_tables(w, W)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == F32
    return _round_to(out, dtype)


def resize_fwd_ref_torch(x, H, W, dtype):
    """The same arithmetic with eager torch float32 operations (each an own kernel, each rounding separately) on a channels-last
    (N, h, w, C) tensor of ``dtype``: for the shapes that are too large for the numpy form's temporaries.  -> (N, H, W, C) ``dtype``"""
    x = x.float()
    h, w = x.shape[1:3]
    y0, y1, ly0, ly1 = resize_tables(h, H)
    x0, x1, lx0, lx1 = resize_tables(w, W)
    ty0, ty1, tx0, tx1 = (torch.from_numpy(v) for v in (y0, y1, x0, x1))
    ly0, ly1 = (torch.from_numpy(v)[:, None, None] for v in (ly0, ly1))
    lx0, lx1 = (torch.from_numpy(v)[:, None] for v in (lx0, lx1))
    r0, r1 = x[:, ty0], x[:, ty1]
    top = lx0 * r0[:, :, tx0] + lx1 * r0[:, :, tx1]
    bot = lx0 * r1[:, :, tx0] + lx1 * r1[:, :, tx1]
    return (ly0 * top + ly1 * bot).to(dtype)


def _weight_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of the float32 table weights, and the (n_out, n_in) boolean matrix of index hits"""
    i0, i1, l0, l1 = resize_tables(n_in, n_out)
    Wm = np.zeros((n_out, n_in), dtype=np.float64)
    hit = np.zeros((n_out, n_in), dtype=bool)
    k = np.arange(n_out)
    np.add.at(Wm, (k, i0), l0.astype(np.float64))
    np.add.at(Wm, (k, i1), l1.astype(np.float64))
    hit[k, i0] = True
    hit[k, i1] = True
    return Wm, hit


def resize_bwd_ref(dy, h, w):
    """Adjoint of the resize: dy (N, C, H, W) -> (dx float64 (N, C, h, w), S = sum |weight * g| per source element, n = number of
    destination pixels that have the source pixel as y0|y1 and x0|x1 (h, w), touch_nonzero (h, w), touch_index (h, w))."""
    dy = np.asarray(dy, dtype=np.float64)
    H, W = dy.shape[2:]
    Wy, hy = _weight_matrix(h, H)
    Wx, hx = _weight_matrix(w, W)
    dx = np.einsum("jy,ncjk,kx->ncyx", Wy, dy, Wx, optimize=True)
    S = np.einsum("jy,ncjk,kx->ncyx", np.abs(Wy), np.abs(dy), np.abs(Wx), optimize=True)
    n = np.outer(hy.sum(0), hx.sum(0))
    touch_nonzero = np.outer((Wy != 0).any(0), (Wx != 0).any(0))
    touch_index = np.outer(hy.any(0), hx.any(0))
    return dx, S, n, touch_nonzero, touch_index


def resize_bwd_ref_nhwc(dy, h, w):
    """The same adjoint for a channels-last (N, H, W, C) tensor without the dense weight matrices (index_add of the float32 table
    weights in float64, columns first, then rows): for shapes with thousands of rows.  -> (dx (N, h, w, C) float64, S, n (h, w))"""
    dy = dy.double()
    H, W = dy.shape[1:3]
    y0, y1, ly0, ly1 = resize_tables(h, H)
    x0, x1, lx0, lx1 = resize_tables(w, W)

    def adjoint(g):
        t = torch.zeros((g.shape[0], H, w, g.shape[3]), dtype=torch.float64)
        for idx, l in ((x0, lx0), (x1, lx1)):
            t.index_add_(2, torch.from_numpy(idx), g * torch.from_numpy(l).double()[:, None])
        out = torch.zeros((g.shape[0], h, w, g.shape[3]), dtype=torch.float64)
        for idx, l in ((y0, ly0), (y1, ly1)):
            out.index_add_(1, torch.from_numpy(idx), t * torch.from_numpy(l).double()[:, None, None])
        return out

    hy, hx = np.zeros((H, h), dtype=bool), np.zeros((W, w), dtype=bool)
    hy[np.arange(H), y0] = hy[np.arange(H), y1] = True
    hx[np.arange(W), x0] = hx[np.arange(W), x1] = True
    return adjoint(dy), adjoint(dy.abs()), np.outer(hy.sum(0), hx.sum(0))


def resize_touch(h, w, H, W, j, k):
    """The source pixels ONE destination pixel (j, k) reaches: (touch_nonzero, touch_index), both (h, w) boolean."""
    Wy, hy = _weight_matrix(h, H)
    Wx, hx = _weight_matrix(w, W)
    return np.outer(Wy[j] != 0, Wx[k] != 0), np.outer(hy[j], hx[k])


def resize_fwd_bound(h, w, xmax):
    """float32 forward against a float64 evaluation: the coordinate fl(scale * dst) carries at most 3 roundings (the two int -> float
    conversions are exact; the division, the product -- and the scale's own error times dst) at magnitude up to in-1, per axis:
    3 * 2^-24 * (h + w) relative to the data's range once it becomes a weight error (|d out| <= |d l| * 2 max|x| per axis); 1 - l1
    adds one rounding per axis, the interpolation three."""
    return 2.0 ** -23 * (3 * (h + w) + 8) * xmax


def half_ulp(v, dtype):
    """Half the spacing of ``dtype`` at |v| (float64 array): the most one rounding to nearest can move a value of that size."""
    p, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}[dtype]
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - (p - 1))


def resize_bwd_bound(ref, S, n, dtype):
    """|got - ref| of an adjoint that forms each weight wy * wx in float32 (one rounding) and accumulates n terms with one rounding
    each (fmaf), every partial sum bounded by S: (n + 1) * 2^-24 * S; a 16-bit result adds the rounding of the stored value, half
    an ulp of the type at the result's magnitude."""
    b = (n + 1) * 2.0 ** -24 * S
    if dtype != torch.float32:
        b = b + half_ulp(np.abs(ref) + b, dtype)
    return b


# ---- MaxPool2d(2, 2), floor mode ---------------------------------------------------------------------------------------------
def _windows(x):
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2)
    return np.stack([v[:, :, :, 0, :, 0], v[:, :, :, 0, :, 1], v[:, :, :, 1, :, 0], v[:, :, :, 1, :, 1]], 0)      # scan order


def maxpool_fwd_ref(x):
    return _windows(np.asarray(x)).max(0)


def maxpool_bwd_ref(x, dy):
    """dx: the window's gradient goes to its FIRST maximum in scan order (0,0), (0,1), (1,0), (1,1) under strict '>' (np.argmax
    returns the first of equal maxima; +0.0 and -0.0 are equal); uncovered odd rows / columns get 0."""
    x, dy = np.asarray(x), np.asarray(dy)
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    arg = _windows(x).argmax(0)
    dx = np.zeros(x.shape, dtype=dy.dtype)
    for q, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, :, a:2 * Ho:2, b:2 * Wo:2] = np.where(arg == q, dy, 0)
    return dx


def pool_input(shape, seed):
    """Tie-heavy pool input (what a ReLU leaves): values from {0, 0, 0, 1, 2}, a third of the zeros as -0.0 -- about four windows
    in ten have more than one maximum, and +0.0 / -0.0 pairs among them.  float32 torch tensor, exact in every dtype."""
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor([0.0, 0.0, 0.0, 1.0, 2.0])[torch.randint(0, 5, shape, generator=g)]
    return torch.where((x == 0) & (torch.rand(shape, generator=g) < 1 / 3), torch.tensor(-0.0), x)


# ---- embedding broadcast, channel copy, flip ---------------------------------------------------------------------------------
def bcast_bwd_ref(dx_nhwc, choff, E):
    """dx (N, HW, ld) -> demb (N, E) float64"""
    return np.asarray(dx_nhwc, dtype=np.float64)[:, :, choff:choff + E].sum(1)


def flip_rows_ref(x, flip):
    x = np.asarray(x)
    out = x.copy()
    for n, f in enumerate(flip):
        if f:
            out[n] = x[n, :, :, ::-1]
    return out


# ---- the shapes the resize tests run, by the forward kernel they are meant for: (N, C, h, w, H, W) ---------------------------------
# (the kernel is chosen by the WIDTH ratio alone -- at most 3 destination columns per source column is row-column, whatever the
#  height ratio: (1,3,1,1 -> 3,3), (2,8,1,5 -> 4,5) and (1,8,4,9 -> 13,9) run the row-column kernel, with h = 1 and with up to 5
#  destination rows per source row; the per-cell list has a steep-width case of each kind in their place)
ROWCOL_SHAPES = [(2, 6, 16, 16, 32, 32), (1, 8, 9, 7, 17, 13), (1, 16, 30, 30, 31, 31), (1, 8, 12, 10, 12, 10), (1, 64, 6, 40, 12, 80),
                 (2, 5, 15, 15, 31, 31), (1, 3, 1, 1, 3, 3), (2, 8, 1, 5, 4, 5), (1, 8, 4, 9, 13, 9)]
CELL_SHAPES = [(1, 8, 5, 4, 15, 12), (1, 8, 6, 1, 6, 7), (2, 8, 1, 2, 4, 9), (1, 8, 4, 3, 13, 12), (1, 3, 1, 1, 5, 5)]
DEST_SHAPES = [(1, 8, 16, 12, 8, 6), (1, 8, 4, 12, 8, 6), (1, 8, 7, 5, 1, 1), (1, 8, 7, 5, 1, 9)]
# backward only.  The 2x2 adjoint takes its general loop where a block's window has more than 8 destination columns: at
# (4, 3) <- (16, 12) the first block column's has 11 and the second's 6 (both forms in one launch), at (3, 2) <- (7, 12) the only
# block's has 12; the first two shapes have windows of exactly 8 columns, the widest the unrolled form takes.
BWD_EXTRA_SHAPES = [(1, 8, 5, 4, 15, 12), (1, 8, 4, 3, 16, 9), (1, 8, 4, 3, 16, 12), (1, 8, 3, 2, 7, 12)]
# (C, h, w, H, W) of the three large row-column cases and the source rows per workgroup each is meant for; the batch size is the
# smallest one at which the plan query reports that count
LARGE_ROWS_SHAPES = {2: (256, 33, 32, 66, 64), 4: (24, 2046, 11, 4092, 22), 8: (24, 4093, 11, 8186, 22)}


RESIZE_FWD_ROWCOL = 0                                         # MAU_RESIZE_FWD_ROWCOL of include/mau_hip.h


def large_rows_batch(plan, rows):
    """Smallest N at which ``plan(N, h, w, H, W, C)`` -> (fwd kernel, rows, bwd kernel) gives the row-column kernel ``rows`` source rows"""
    C, h, w, H, W = LARGE_ROWS_SHAPES[rows]
    for N in range(1, 65):
        if plan(N, h, w, H, W, C)[:2] == (RESIZE_FWD_ROWCOL, rows):
            return N
    return None


POOL_SHAPES = [(2, 8, 2, 3), (1, 24, 9, 11), (3, 64, 31, 17), (1, 72, 6, 64), (2, 5, 8, 8)]      # (N, C, H, W)
