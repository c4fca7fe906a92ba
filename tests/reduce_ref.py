"""Order-exact float64 host references of the chunked fp64 reductions (csrc/chunk_reduce.h): every join restated operation for
operation -- a thread's values in slot / index order, the xor butterfly over the 64 lanes of a wave, the waves 0..3 in order, the
chunks in order, moment rows by ``ground_truth.merge_moments``.  numpy's element-wise float64 operations are the IEEE operations
the device performs (nothing is contracted on either side), so the results are compared by their 64-bit patterns.  The 256
threads of a workgroup are an array axis; every add along a thread's own values, the lanes, the waves and the chunks is an
explicit sequential one (``np.sum`` / ``np.mean`` are pairwise and do not match)."""
import numpy as np

CHUNK, THREADS, SLOTS = 4096, 256, 16
_LANE = np.arange(64)
ADD, FMIN, FMAX = np.add, np.fmin, np.fmax               # fmin / fmax skip a NaN, as the device's do


def merge_moments(a, b):
    """ground_truth.merge_moments (kept here so that the reference imports nothing that needs the library)"""
    na, ma, qa = a
    nb, mb, qb = b
    if na == 0.0:
        return nb, mb, qb
    delta = mb - ma
    n = na + nb
    return n, ma + (delta * nb) / n, (qa + qb) + (delta * delta) * ((na * nb) / n)


def block_join(per_thread, op=ADD):
    """(256,) float64 -> the workgroup's value: butterfly 32..1 within each wave, then the waves in wave order"""
    a = np.asarray(per_thread, dtype=np.float64).reshape(4, 64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = 32
        while s >= 1:
            a = op(a, a[:, _LANE ^ s])
            s >>= 1
        r = a[0, 0]
        for w in range(1, 4):
            r = op(r, a[w, 0])
    return np.float64(r)


def thread_join(vals, mask, op=ADD, init=0.0):
    """vals, mask (steps, 256): a thread joins its values in step order, a masked-out step is skipped"""
    acc = np.full(THREADS, init, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, m in zip(vals, mask):
            acc = np.where(m, op(acc, v), acc)
    return acc


def chunk_slots(npx, vec4):
    """(16, 256) pixel index of slot s of thread t within a chunk of npx pixels, and which slots are inside it"""
    s, t = np.meshgrid(np.arange(SLOTS), np.arange(THREADS), indexing="ij")
    idx = ((s >> 2) * THREADS + t) * 4 + (s & 3) if vec4 else s * THREADS + t
    ok = idx < npx
    return np.where(ok, idx, 0), ok


def chunk_moments(x, vec4):
    """the moment row (n, mean, M2, min, max, sum |x|, NaNs, non-finite values) of one chunk x (float64, <= 4096 values)"""
    idx, ok = chunk_slots(x.size, vec4)
    v = x[idx]
    n = np.float64(x.size)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = block_join(thread_join(v, ok)) / n
        d = v - mean
        return [n, mean, block_join(thread_join(d * d, ok)), block_join(thread_join(v, ok, FMIN, np.inf), FMIN),
                block_join(thread_join(v, ok, FMAX, -np.inf), FMAX), block_join(thread_join(np.abs(v), ok)),
                block_join(thread_join(np.isnan(v).astype(np.float64), ok)), block_join(thread_join((~np.isfinite(v)).astype(np.float64), ok))]


def plane_row(x, vec4):
    """the 8-entry plane row of ``mau_tile_stats`` for one plane of float64 values: chunk rows joined in chunk order"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    rows = [chunk_moments(x[q:q + CHUNK], vec4) for q in range(0, x.size, CHUNK)]
    acc, (mn, mx, l1, nan, bad) = tuple(rows[0][:3]), rows[0][3:]
    with np.errstate(invalid="ignore", over="ignore"):
        for r in rows[1:]:
            acc = merge_moments(acc, tuple(r[:3]))
            mn, mx, l1, nan, bad = FMIN(mn, r[3]), FMAX(mx, r[4]), l1 + r[5], nan + r[6], bad + r[7]
    return np.array([acc[0], acc[1], acc[2], mn, mx, l1, nan, bad], dtype=np.float64)


def plane_moments(x, vec4=None):
    """``mau_plane_moments``: (B, C, H, W) float32 -> (B, C, 4) rows (n, mean, M2, non-finite values)"""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape[:2]
    hw = x[0, 0].size
    vec4 = hw % 4 == 0 if vec4 is None else vec4
    out = np.empty((B, C, 4), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            out[b, c] = plane_row(x[b, c].astype(np.float64), vec4)[[0, 1, 2, 7]]
    return out


def tile_stats(cls_a, cls_b, cont, targets, num_classes=9, vec4=None):
    """``mau_tile_stats``: (B, 34 + 9 * 8) rows"""
    a, b = np.asarray(cls_a), np.asarray(cls_b)
    c, t = np.asarray(cont, dtype=np.float32).astype(np.float64), np.asarray(targets, dtype=np.float32).astype(np.float64)
    B = a.shape[0]
    hw = a[0].size
    vec4 = hw % 4 == 0 if vec4 is None else vec4
    rows = np.zeros((B, 34 + 72), dtype=np.float64)
    for i in range(B):
        for m, cm in enumerate((a[i], b[i])):
            rows[i, 16 * m:16 * m + num_classes] = np.bincount(cm.reshape(-1), minlength=256)[:num_classes]
            rows[i, 32 + m] = int((cm >= num_classes).sum())
        with np.errstate(invalid="ignore"):
            planes = [c[i, j] for j in range(5)] + [t[i, 0], t[i, 1], t[i, 0] - c[i, 3], t[i, 1] - c[i, 4]]
        for p, v in enumerate(planes):
            rows[i, 34 + 8 * p:42 + 8 * p] = plane_row(v, vec4)
    return rows


def _index_steps(npx):
    """(steps, 256) pixel index of step m of thread t (idx = t, t + 256, ...) within a chunk of npx pixels, and the mask"""
    steps = -(-npx // THREADS)
    idx = np.arange(steps)[:, None] * THREADS + np.arange(THREADS)[None, :]
    ok = idx < npx
    return np.where(ok, idx, 0), ok


def scenario_result(out, temp_orig, dw_t1, dw_t2, temp_mean, temp_std):
    """``mau_scenario_result``'s statistics: out (N, 2, H, W) float32 -> (N, 5) rows (mean, min, max of the temperature
    difference, edited pixels, mean of the difference over them)"""
    out = np.asarray(out, dtype=np.float32)
    N = out.shape[0]
    hw = out[0, 0].size
    have = temp_orig is not None
    rows = np.empty((N, 5), dtype=np.float64)
    d1 = np.asarray(dw_t1).reshape(-1)
    for n in range(N):
        t = (out[n, 1].reshape(-1) * np.float32(temp_std)).astype(np.float32) + np.float32(temp_mean)     # two rounded fp32 operations
        edited = np.asarray(dw_t2)[n].reshape(-1) != d1
        d = (t - np.asarray(temp_orig, dtype=np.float32).reshape(-1)).astype(np.float64) if have else np.zeros(hw)
        part = []
        for q in range(0, hw, CHUNK):
            idx, ok = _index_steps(min(CHUNK, hw - q))
            dc, ec = d[q:q + CHUNK][idx], edited[q:q + CHUNK][idx]
            part.append([block_join(thread_join(dc, ok)), block_join(thread_join(dc, ok, FMIN, np.inf), FMIN),
                         block_join(thread_join(dc, ok, FMAX, -np.inf), FMAX), block_join(thread_join(ec.astype(np.float64), ok)),
                         block_join(thread_join(np.where(ec, dc, 0.0), ok))])
        tot = list(part[0])
        with np.errstate(invalid="ignore"):
            for r in part[1:]:
                tot = [tot[0] + r[0], FMIN(tot[1], r[1]), FMAX(tot[2], r[2]), tot[3] + r[3], tot[4] + r[4]]
            cnt = tot[3]
            rows[n] = [tot[0] / np.float64(hw), tot[1], tot[2], cnt, tot[4] / cnt if cnt > 0.0 else np.nan] if have else \
                [np.nan, np.nan, np.nan, cnt, np.nan]
    return rows


def eval_metrics(out, tgt, cls, scale, shift, ncls):
    """``mau_eval_metrics``: out, tgt (B, C, H, W) float32, cls (B, H, W) uint8 -> (B * C, 11 + 3 * ncls) rows"""
    out, tgt, cls = np.asarray(out, dtype=np.float32), np.asarray(tgt, dtype=np.float32), np.asarray(cls)
    B, C, H, W = out.shape
    NB = 10 if ncls <= 9 else 17
    rpc = 1 if W >= CHUNK else CHUNK // W
    rows = np.empty((B * C, 11 + 3 * ncls), dtype=np.float64)
    ops = [ADD] * 8 + [FMIN, FMAX, FMIN, FMAX] + [ADD] * (3 * NB)
    init = [0.0] * 8 + [np.inf, -np.inf, np.inf, -np.inf] + [0.0] * (3 * NB)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    up, dn, lf, rt = np.maximum(ii - 1, 0), np.minimum(ii + 1, H - 1), np.maximum(jj - 1, 0), np.minimum(jj + 1, W - 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for row in range(B * C):
            b, c = divmod(row, C)
            sc, sh = np.float64(scale[c]), np.float64(shift[c])
            of, tf = out[b, c], tgt[b, c]
            p, g = of.astype(np.float64) * sc + sh, tf.astype(np.float64) * sc + sh
            lp = (((p[up, jj] + p[dn, jj]) + p[ii, lf]) + p[ii, rt]) - 4.0 * p
            lg = (((g[up, jj] + g[dn, jj]) + g[ii, lf]) + g[ii, rt]) - 4.0 * g
            d = p - g
            a, d2 = np.abs(d), d * d
            bins = np.where(cls[b] < ncls, cls[b].astype(np.int64), NB - 1)
            vals = [a, d2, lp, lp * lp, lg, lg * lg, (~np.isfinite(of)).astype(np.float64), (~np.isfinite(tf)).astype(np.float64), p, p, g, g]
            vals += [(bins == k).astype(np.float64) for k in range(NB)] + [np.where(bins == k, a, 0.0) for k in range(NB)]
            vals += [np.where(bins == k, d2, 0.0) for k in range(NB)]
            tot = None
            for i0 in range(0, H, rpc):
                i1 = min(i0 + rpc, H)
                idx, ok = _index_steps((i1 - i0) * W)
                part = [block_join(thread_join(v[i0:i1].reshape(-1)[idx], ok, op, s0), op) for v, op, s0 in zip(vals, ops, init)]
                tot = part if tot is None else [op(x, y) for op, x, y in zip(ops, tot, part)]
            n = np.float64(H * W)
            r = [tot[0] / n, np.sqrt(tot[1] / n)]
            for e in (2, 3):
                m = tot[2 * e - 2] / n
                val = tot[2 * e - 1] / n - m * m
                r.append(np.float64(0.0) if val < 0.0 else val)
            r += tot[6:12] + [tot[12 + NB - 1]]
            cnt = tot[12:12 + ncls]
            r += cnt + [tot[12 + NB + k] / cnt[k] for k in range(ncls)] + [np.sqrt(tot[12 + 2 * NB + k] / cnt[k]) for k in range(ncls)]
            rows[row] = r
    return rows
