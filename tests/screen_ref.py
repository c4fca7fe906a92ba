"""Host references of csrc/screen.hip, written from include/mau_hip.h.

``screen_rows`` is the order-exact float64 twin of ``mau_screen_rows``, spelled the naive way with the joins of
``tests/reduce_ref.py``: thread t walks the slots i = t, t + 256, ... of the UNCLIPPED ph x pw rectangle (row-major), skips a slot
outside the tile, and adds the rest in that order; then the xor butterfly over the lanes and the waves in wave order.  (The product's
``screening.rows_host`` walks only the clipped rectangle; the two spellings must agree.)  ``screen_maps`` and ``screen_seed`` are
element-wise.

``brute_rows`` spells the DEFINITIONS with exact rational arithmetic: the sum of the swap terms as a ``Fraction``, rounded once.  On
dyadic gradients (``dyadic``: values m * 2^j) ``exact_sums`` asserts from the data that every partial sum in any order is exact in
fp64 -- then twin, brute force and device must agree bit for bit, whatever their order.

Values are float64 throughout: fp32, bf16 and fp16 widen exactly.  Results are compared by 64-bit pattern, any NaN matching any NaN."""
from fractions import Fraction

import numpy as np

from tests.reduce_ref import THREADS, block_join, thread_join

ROW = 4
N_CONT = 5


def off_of(ncls):
    """[one-hot dw_t1 (ncls) | rgb, ndvi, temp (5) | one-hot second map (ncls)]: where the second block starts"""
    return ncls + N_CONT


def dyadic(rng, shape, bits=7, exp=-4):
    """m * 2^exp with |m| < 2^bits: exact in fp32, fp16 and (bits <= 7) bf16"""
    return (rng.integers(-(1 << bits) + 1, 1 << bits, shape) * 2.0 ** exp).astype(np.float64)


def exact_sums(g):
    """True when every sum of any subset of the finite values of ``g``, in any order, is exact in float64: all are multiples of one
    power of two, and the sum of their magnitudes, counted in that unit, stays below 2^53 (twice over: a swap term is a difference)."""
    v = np.abs(np.asarray(g, dtype=np.float64))
    v = v[np.isfinite(v) & (v > 0)]
    if v.size == 0:
        return True
    den = max(Fraction(x).denominator for x in np.unique(v).tolist())                 # a power of two: every value is a multiple of 1 / den
    return 2 * sum(Fraction(x) for x in v.tolist()) * den < 2 ** 53


def coef_of(ch, n, temp_std, seed_scale):
    with np.errstate(divide="ignore"):
        return (np.float64(temp_std) if ch == 1 else np.float64(1.0)) / (np.float64(seed_scale) * np.float64(n))


def inside(y0, x0, ph, pw, H, W):
    """(H, W) bool, the header's inequalities on Python-sized integers"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    dy, dx = y - np.int64(y0), x - np.int64(x0)
    return (dy >= 0) & (dy < ph) & (dx >= 0) & (dx < pw)


def screen_seed(objs, rois, H, W, seed_scale=1.0):
    objs = np.asarray(objs)
    dout = np.zeros((len(objs), 2, H, W), dtype=np.float32)
    counts = np.zeros(len(objs), dtype=np.float64)
    for k, (ch, r) in enumerate(objs.tolist()):
        m = np.ones((H, W), dtype=bool) if r == -1 else np.asarray(rois)[r] != 0
        dout[k, ch][m] = seed_scale
        counts[k] = int(m.sum())
    return dout, counts


def _terms(g, cur, cls, ncls):
    """per pixel: the swap term in float64 and the non-finite values read, (H, W) each"""
    off = off_of(ncls)
    has = cur < ncls
    a = g[..., off + cls]
    b = np.take_along_axis(g, (off + np.where(has, cur, 0))[..., None].astype(np.int64), axis=2)[..., 0]
    with np.errstate(invalid="ignore", over="ignore"):
        return a - np.where(has, b, 0.0), (~np.isfinite(a)).astype(np.float64) + (has & ~np.isfinite(b)).astype(np.float64)


def screen_rows(G, dw_t2, edits, counts, objs, ph, pw, ncls, temp_std, seed_scale=1.0):
    """``mau_screen_rows``: G (K, H, W, C) float64 -> (K, P, 4) float64, in the device's order"""
    G, cur = np.asarray(G, dtype=np.float64), np.asarray(dw_t2).astype(np.int64)
    K, H, W, _ = G.shape
    rows = np.zeros((K, len(edits), ROW), dtype=np.float64)
    steps = -(-(ph * pw) // THREADS)
    i = np.arange(steps)[:, None] * THREADS + np.arange(THREADS)[None, :]              # slot of step m of thread t
    for j, (y0, x0, cls) in enumerate(np.asarray(edits, dtype=np.int64).tolist()):
        y, x = y0 + i // pw, x0 + i % pw
        ok = (i < ph * pw) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        yy, xx = np.where(ok, y, 0), np.where(ok, x, 0)
        live = 0 <= cls < ncls
        for k in range(K):
            n = counts[k]
            ones = np.ones(i.shape)
            rows[k, j, 0] = block_join(thread_join(ones, ok))
            if live:
                term, bad = _terms(G[k], cur, cls, ncls)
                rows[k, j, 1] = block_join(thread_join((cur[yy, xx] != cls).astype(np.float64), ok))
                rows[k, j, 3] = block_join(thread_join(bad[yy, xx], ok))
                with np.errstate(invalid="ignore", over="ignore"):
                    total = coef_of(objs[k][0], n, temp_std, seed_scale) * block_join(thread_join(term[yy, xx], ok))
            else:
                total = np.float64(0.0)
            rows[k, j, 2] = total if n > 0 else np.nan
    return rows


def brute_rows(G, dw_t2, edits, counts, objs, ph, pw, ncls, temp_std, seed_scale=1.0):
    """The definitions, with the sum of the swap terms exact (a Fraction, rounded to float64 once); a non-finite term makes it NaN
    or an infinity as IEEE addition in any order would when no two infinities of opposite sign meet"""
    G, cur = np.asarray(G, dtype=np.float64), np.asarray(dw_t2).astype(np.int64)
    K, H, W, _ = G.shape
    rows = np.zeros((K, len(edits), ROW), dtype=np.float64)
    for j, (y0, x0, cls) in enumerate(np.asarray(edits, dtype=np.int64).tolist()):
        m = inside(y0, x0, ph, pw, H, W)
        rows[:, j, 0] = int(m.sum())
        for k in range(K):
            n = counts[k]
            total = np.float64(0.0)
            if 0 <= cls < ncls:
                term, bad = _terms(G[k], cur, cls, ncls)
                rows[k, j, 1] = int((m & (cur != cls)).sum())
                rows[k, j, 3] = bad[m].sum()
                t = term[m]
                if np.isfinite(t).all():
                    s = np.float64(float(sum((Fraction(v) for v in t.tolist()), Fraction(0))))
                else:
                    with np.errstate(invalid="ignore"):
                        s = np.float64(t[~np.isfinite(t)].sum())
                with np.errstate(invalid="ignore", over="ignore"):
                    total = coef_of(objs[k][0], n, temp_std, seed_scale) * s
            rows[k, j, 2] = total if n > 0 else np.nan
    return rows


def screen_maps(G, dw_t2, counts, objs, k, ncls, temp_std, seed_scale=1.0):
    """``mau_screen_maps``: (ncls, H, W) float32"""
    G, cur = np.asarray(G, dtype=np.float64), np.asarray(dw_t2).astype(np.int64)
    if not counts[k] > 0:
        return np.full((ncls, *cur.shape), np.nan, dtype=np.float32)
    c = coef_of(objs[k][0], counts[k], temp_std, seed_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(c * _terms(G[k], cur, cls, ncls)[0]).astype(np.float32) for cls in range(ncls)])


def same(got, want):
    """two float arrays agree by bit pattern; any NaN matches any NaN.  What differs is printed."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        print("shapes or types differ:", got.shape, got.dtype, want.shape, want.dtype)
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    differ = (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)) & ~(np.isnan(got) & np.isnan(want))
    if differ.any():
        at = np.argwhere(differ)[:8]
        print("differ at", at.tolist(), [float(got[tuple(i)]).hex() for i in at], "against", [float(want[tuple(i)]).hex() for i in at])
        return False
    return True
