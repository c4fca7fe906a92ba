"""Host references of csrc/placement.hip, written from include/mau_hip.h.

``placement_result`` is the order-exact float64 twin of ``mau_placement_result``, built from the joins of ``tests/reduce_ref.py``:
a thread joins its 16 slots in slot order (``chunk_slots``: slot 4k + j of thread t is pixel (k * 256 + t) * 4 + j with 16-byte
accesses, slot k is pixel k * 256 + t without), the 64 lanes by the xor butterfly, the waves in wave order, the chunks in chunk
order.  A sum over a subset (stamp, outside, roi) adds +0.0 for a pixel outside the subset, as the device does.  Results are
compared by their 64-bit patterns (any NaN matches any NaN).

``edited_maps`` / ``pack_dense`` restate ``mau_placement_pack`` per pixel with the header's inequalities on Python-sized integers
-- no clipping of a rectangle, so the path is not ``placement.stamp_mask``'s."""
import numpy as np

from tests.reduce_ref import ADD, CHUNK, FMAX, FMIN, block_join, chunk_slots, thread_join

ROW = 12
# the join and the identity of the twelve accumulators: stamp pixels, sum dT, min dT, max dT, sum dT in the stamp, sum dT outside,
# roi pixels, sum dT over the roi, sum dN, sum dN in the stamp, sum dN over the roi, non-finite values
OPS = [ADD, ADD, FMIN, FMAX] + [ADD] * 8
INIT = [0.0, 0.0, np.inf, -np.inf] + [0.0] * 8


def stamp(edit, H, W, ph, pw):
    """(H, W) bool: y0 <= y < y0 + ph and x0 <= x < x0 + pw, in int64"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    dy, dx = y - np.int64(edit[0]), x - np.int64(edit[1])
    return (dy >= 0) & (dy < ph) & (dx >= 0) & (dx < pw)


def edited_maps(dw_t2, edits, ph, pw, ncls):
    """(B, H, W) uint8: cls under the stamp when 0 <= cls < ncls, dw_t2 elsewhere"""
    dw_t2 = np.asarray(dw_t2)
    H, W = dw_t2.shape
    out = []
    for e in np.asarray(edits, dtype=np.int64):
        hit = stamp(e, H, W, ph, pw) & bool(0 <= e[2] < ncls)
        out.append(np.where(hit, e[2], dw_t2).astype(np.uint8))
    return np.stack(out)


def pack_dense(dw_t1, dw_t2, cont, edits, ph, pw, ncls):
    """(B, 2 ncls + 5, H, W) float32 from the class maps and the five NORMALISED planes ``cont`` (5, H, W)"""
    ids = np.arange(ncls).reshape(-1, 1, 1)
    first = (np.asarray(dw_t1)[None] == ids).astype(np.float32)
    return np.stack([np.concatenate([first, np.asarray(cont, dtype=np.float32), (m[None] == ids).astype(np.float32)])
                     for m in edited_maps(dw_t1 if dw_t2 is None else dw_t2, edits, ph, pw, ncls)])


def placement_result(out, base, edits, roi, temp_mean, temp_std, ph, pw, vec4=None):
    """``mau_placement_result``: out (B, 2, H, W), base (2, H, W) float32 -> (B, 12) float64 rows"""
    out, base = np.asarray(out, dtype=np.float32), np.asarray(base, dtype=np.float32)
    B, _, H, W = out.shape
    hw = H * W
    vec4 = hw % 4 == 0 if vec4 is None else vec4
    std, mean = np.float32(temp_std), np.float32(temp_mean)
    inr = np.zeros(hw, dtype=bool) if roi is None else np.asarray(roi).reshape(-1) != 0
    rows = np.empty((B, ROW), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tb = (base[1].reshape(-1) * std).astype(np.float32) + mean                     # two rounded fp32 operations
        for b in range(B):
            t = (out[b, 1].reshape(-1) * std).astype(np.float32) + mean
            assert t.dtype == np.float32 and tb.dtype == np.float32
            dT = (t - tb).astype(np.float64)
            dN = (out[b, 0].reshape(-1) - base[0].reshape(-1)).astype(np.float64)
            m = stamp(edits[b], H, W, ph, pw).reshape(-1)
            bad = (~np.isfinite(out[b, 0].reshape(-1))).astype(np.float64) + (~np.isfinite(out[b, 1].reshape(-1))).astype(np.float64)
            vals = [m.astype(np.float64), dT, dT, dT, np.where(m, dT, 0.0), np.where(~m, dT, 0.0), inr.astype(np.float64),
                    np.where(inr, dT, 0.0), dN, np.where(m, dN, 0.0), np.where(inr, dN, 0.0), bad]
            tot = None
            for q in range(0, hw, CHUNK):
                idx, ok = chunk_slots(min(CHUNK, hw - q), vec4)
                part = [block_join(thread_join(v[q:q + CHUNK][idx], ok, op, s0), op) for v, op, s0 in zip(vals, OPS, INIT)]
                tot = part if tot is None else [op(x, y) for op, x, y in zip(OPS, tot, part)]
            n, cnt, nroi = np.float64(hw), tot[0], tot[6]
            rest = n - cnt
            nan = np.float64(np.nan)
            rows[b] = [cnt, tot[1] / n, tot[2], tot[3], tot[4] / cnt if cnt > 0 else nan, tot[5] / rest if rest > 0 else nan, nroi,
                       tot[7] / nroi if nroi > 0 else nan, tot[8] / n, tot[9] / cnt if cnt > 0 else nan,
                       tot[10] / nroi if nroi > 0 else nan, tot[11]]
    return rows


def same_rows(got, want):
    """(B, 12) float64 rows agree by 64-bit pattern; any NaN matches any NaN.  What differs is printed."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        print("shapes differ:", got.shape, want.shape)
        return False
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    if differ.any():
        at = np.argwhere(differ)[:8]
        print("rows differ at", at.tolist(), [float(got[tuple(i)]).hex() for i in at], "against", [float(want[tuple(i)]).hex() for i in at])
        return False
    return True
