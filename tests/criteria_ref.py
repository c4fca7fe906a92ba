"""Plain references of the training criteria (csrc/head.hip: mse_kernel, l1_gradient_loss_kernel), the embedding fold
(csrc/embfold.hip), the gradient sum (csrc/spatial.hip: sum_tensors_kernel) and the layout boundary (nchw_to_nhwc / nhwc_to_nchw):
numpy on the CPU, written from the formulas, no device.

The criteria's references repeat the kernels' OPERATIONS, not only their formulas: float32 differences and terms, float64 sums of the
float32 terms, one rounding of the mean to float32, dout built in float32 in the kernel's order.  The generators of the "exact" cases
live here too: multiples of 1/8 in [-4, 4] (criteria) and integers in [-3, 3] (fold), so that every float32 term is exact and every
sum is exact in any order (tests/test_criteria_host.py proves that for every generated case) and a kernel's result must equal the
reference bit for bit."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
FOLD_CO_CHUNK = 32                                            # output channels per first-level workgroup of emb_fold_bwd_e_kernel
LOSS_WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 2.5), (0.0, 0.0)]


def pad8(c):
    return (c + 7) // 8 * 8


def _rng(*key):
    return np.random.default_rng([abs(int(v)) for v in key])


def _sgn(v):
    """sign as the array's own type, sgn(0) = 0"""
    return np.sign(v).astype(v.dtype)


# ---- MSE ----------------------------------------------------------------------------------------------------------------------------
def mse_ref(out, tgt):
    """-> (loss float32, dout float32 array, S float64): d = out - tgt in float32, S = sum (float64)(d * d) with the product formed in
    float32, loss = float32(S * (1.0 / n)), dout = d * float32(2.0 / float32(n)): mse_kernel and mse_final_kernel, operation for operation"""
    o, t = np.asarray(out, dtype=F32), np.asarray(tgt, dtype=F32)
    n = o.size
    d = o - t
    S = (d * d).astype(F64).sum()
    return F32(S * (1.0 / n)), d * (F32(2.0) / F32(n)), S


# ---- L1 + finite-difference gradient loss ------------------------------------------------------------------------------------------
def l1_gradient_counts(shape):
    B, C, H, W = shape
    return B * C * H * W, B * C * (H - 1) * W, B * C * H * (W - 1)


def criteria_differences(o, t):
    """o - t, dy o, |dy o| - |dy t|, dx o, |dx o| - |dx t| in the type of ``o`` and ``t``; the criterion's terms are the magnitudes of
    the first, third and fifth"""
    ay, by = o[:, :, 1:] - o[:, :, :-1], t[:, :, 1:] - t[:, :, :-1]
    ax, bx = o[..., 1:] - o[..., :-1], t[..., 1:] - t[..., :-1]
    return o - t, ay, np.abs(ay) - np.abs(by), ax, np.abs(ax) - np.abs(bx)


def l1_gradient_ref(out, tgt, w_l1, w_grad, real=F32):
    """-> (terms, dout, sums).  ``real`` = float32: the kernel's operations.  The three sums are float64 sums of ``real`` terms
    |o - t|, | |dy o| - |dy t| |, | |dx o| - |dx t| |; terms[k] = float32(S_k * inv_k), inv = 1 / count in float64, 0 for an empty
    count (H == 1, W == 1).  dout in ``real``, in the kernel's order: g = k_l1 * sgn(o - t); minus the down-difference term (the pair
    (y, y + 1), this element the subtrahend); plus the up-difference term (the pair (y - 1, y)); minus the right-difference term; plus
    the left-difference term.  k_l1 = w_l1 / real(n), k_gy = w_grad / real(ny) or 0 when ny == 0, k_gx likewise; the weights are the
    float32 values the entry point receives.  sgn(0) = 0.  (A product with a sign is exact: whether the compiler contracts
    ``g -= k * s`` into an FMA cannot change a bit.)  ``real`` = float64: the same formulas without the float32 roundings, terms
    unrounded."""
    o, t = np.asarray(out, dtype=F32).astype(real), np.asarray(tgt, dtype=F32).astype(real)
    n, ny, nx = l1_gradient_counts(o.shape)
    w_l1, w_grad = real(F32(w_l1)), real(F32(w_grad))
    k_l1 = w_l1 / real(n)
    k_gy = w_grad / real(ny) if ny > 0 else real(0)
    k_gx = w_grad / real(nx) if nx > 0 else real(0)
    d0, ay, dy, ax, dx = criteria_differences(o, t)
    sums = np.array([np.abs(v).astype(F64).sum() for v in (d0, dy, dx)])
    inv = np.array([1.0 / n, 1.0 / ny if ny > 0 else 0.0, 1.0 / nx if nx > 0 else 0.0])
    terms = (sums * inv).astype(F32) if real is F32 else sums * inv
    g = k_l1 * _sgn(d0)
    ty, tx = k_gy * _sgn(dy) * _sgn(ay), k_gx * _sgn(dx) * _sgn(ax)
    g[:, :, :-1] = g[:, :, :-1] - ty
    g[:, :, 1:] = g[:, :, 1:] + ty
    g[..., :-1] = g[..., :-1] - tx
    g[..., 1:] = g[..., 1:] + tx
    assert g.dtype == real and ty.dtype == real
    return terms, g, sums


def dout_bound(shape, w_l1, w_grad):
    """8 * 2^-24 * (|k_l1| + 2 |k_gy| + 2 |k_gx|): dout is five float32 terms, each at most a coefficient in magnitude, so each of the
    four adds rounds a partial sum of at most the bracket (4 * 2^-24), and each coefficient is a float32 quotient of a float32 weight
    (2^-24 relative: at most 1 more bracket); 8 leaves room for both"""
    n, ny, nx = l1_gradient_counts(shape)
    return 8 * 2.0 ** -24 * (abs(w_l1) / n + (2 * abs(w_grad) / ny if ny else 0.0) + (2 * abs(w_grad) / nx if nx else 0.0))


def tie_counts(out, tgt):
    """how many elements / neighbour pairs of a case sit on a tie, in all and on the image borders (a pair is "on" a border row or
    column when one of its two elements lies there)"""
    o, t = np.asarray(out, dtype=F64), np.asarray(tgt, dtype=F64)
    eq = o == t
    ay, by = o[:, :, 1:] - o[:, :, :-1], t[:, :, 1:] - t[:, :, :-1]
    ax, bx = o[..., 1:] - o[..., :-1], t[..., 1:] - t[..., :-1]
    c = {"eq": int(eq.sum()), "eq_first_row": int(eq[:, :, 0].sum()), "eq_last_row": int(eq[:, :, -1].sum()),
         "eq_first_col": int(eq[..., 0].sum()), "eq_last_col": int(eq[..., -1].sum())}
    for name, a, b, ax_ in (("dy", ay, by, 2), ("dx", ax, bx, 3)):
        zero, same = a == 0, (np.abs(a) == np.abs(b)) & (a != 0)
        first, last = [slice(None)] * 4, [slice(None)] * 4
        first[ax_], last[ax_] = 0, -1
        if a.shape[ax_] == 0:
            c.update({f"{name}_zero": 0, f"{name}_abs": 0, f"{name}_zero_first": 0, f"{name}_zero_last": 0, f"{name}_abs_first": 0, f"{name}_abs_last": 0})
            continue
        c.update({f"{name}_zero": int(zero.sum()), f"{name}_abs": int(same.sum()),
                  f"{name}_zero_first": int(zero[tuple(first)].sum()), f"{name}_zero_last": int(zero[tuple(last)].sum()),
                  f"{name}_abs_first": int(same[tuple(first)].sum()), f"{name}_abs_last": int(same[tuple(last)].sum())})
    return c


def _eighths(r, shape, lo=-32, hi=32):
    return (r.integers(lo, hi + 1, shape) / 8.0).astype(F32)


def _force_pairs(o, t, axis, first, kind_a, pick=True):
    """the neighbour pairs (first, first + 1) along ``axis`` (2: rows, 3: columns) -- ``first`` an index, or None for every even one
    at once --, where ``pick`` holds (masks of the shape of the rows / columns taken): where ``kind_a``,  d o == 0  (the second
    element copies the first);  elsewhere  |d o| == |d t|  with opposite signs (tgt = -out on both elements).  Both keep every value
    a multiple of 1/8 in [-4, 4]."""
    ov, tv = (o, t) if axis == 2 else (o.swapaxes(2, 3), t.swapaxes(2, 3))          # views
    n = ov.shape[2]
    a, b = (slice(0, n - 1, 2), slice(1, n, 2)) if first is None else (first, first + 1)
    za, zb = pick & kind_a, pick & ~kind_a
    ov[:, :, b] = np.where(za, ov[:, :, a], ov[:, :, b])
    tv[:, :, a] = np.where(zb, -ov[:, :, a], tv[:, :, a])
    tv[:, :, b] = np.where(zb, -ov[:, :, b], tv[:, :, b])


def exact_criteria_case(shape, seed=0, share=0.125):
    """-> (out, tgt) float32 (B, C, H, W), every value a multiple of 1/8 in [-4, 4].

    1. Uniform values.  2. Two consecutive planes must not leak into each other: on the last row of every plane out is in [3, 4], on
    the first row in [-4, -3], tgt in [-1, 1] on both (a dy across a plane boundary would add about 7 to the dy sum); the same on the
    last and first column (a dx across a row end).  3. ``share`` of the elements get out == tgt; ``share`` of the vertical pairs
    (y even) get a tie, half of them dy o == 0 and half |dy o| == |dy t|; the same for the horizontal pairs (x even) -- later steps
    undo a part of the earlier ones, ``tie_counts`` says what is left.  4. Ties on the borders, one kind per plane (plane index mod 3):
    plane 0 ties the pairs of the first and of the last row along y, alternating by column between the two kinds; plane 1 the same
    along x; plane 2 sets out == tgt on every other element of the first and last row and column.  A case of one plane (1, 1, 1, 1)
    gets out == tgt when its seed is even."""
    B, C, H, W = shape
    r = _rng(11, B, C, H, W, seed)
    P = B * C
    o, t = _eighths(r, (1, P, H, W)), _eighths(r, (1, P, H, W))
    if H > 1:
        o[:, :, -1], o[:, :, 0] = _eighths(r, (1, P, W), 24, 32), _eighths(r, (1, P, W), -32, -24)
        t[:, :, -1], t[:, :, 0] = _eighths(r, (1, P, W), -8, 8), _eighths(r, (1, P, W), -8, 8)
    if W > 1:
        o[..., -1], o[..., 0] = _eighths(r, (1, P, H), 24, 32), _eighths(r, (1, P, H), -32, -24)
        t[..., -1], t[..., 0] = _eighths(r, (1, P, H), -8, 8), _eighths(r, (1, P, H), -8, 8)
    eq = r.random(o.shape) < share
    t[eq] = o[eq]
    for axis, n in ((2, H), (3, W)):
        pairs = (1, P, n // 2, W if axis == 2 else H)
        _force_pairs(o, t, axis, None, r.random(pairs) < 0.5, r.random(pairs) < share)
    for p in range(P):
        op, tp = o[:, p:p + 1], t[:, p:p + 1]
        kind = p % 3
        if kind == 0 and H > 1:
            even = (np.arange(W) % 2 == 0)[None, None]
            _force_pairs(op, tp, 2, 0, even)
            _force_pairs(op, tp, 2, H - 2, ~even)
        elif kind == 1 and W > 1:
            even = (np.arange(H) % 2 == 0)[None, None]
            _force_pairs(op, tp, 3, 0, even)
            _force_pairs(op, tp, 3, W - 2, ~even)
        elif kind == 2:
            tp[:, :, 0, ::2], tp[:, :, -1, ::-2] = op[:, :, 0, ::2], op[:, :, -1, ::-2]
            tp[:, :, ::2, 0], tp[:, :, ::-2, -1] = op[:, :, ::2, 0], op[:, :, ::-2, -1]
    if P * H * W == 1 and seed % 2 == 0:
        t[:] = o
    return o.reshape(shape), t.reshape(shape)


def exact_flat_case(n, seed=0):
    """the MSE's operands: ``exact_criteria_case`` of one row of n elements"""
    o, t = exact_criteria_case((1, 1, 1, n), seed, share=0.25)
    return o.reshape(n), t.reshape(n)


def is_eighths(x, bound=4.0):
    x = np.asarray(x, dtype=F64)
    return bool((x * 8 == np.round(x * 8)).all() and (np.abs(x) <= bound).all())


def random_criteria_case(shape, seed=0):
    """randn float32 operands of the real-valued case; the target is the output plus noise, as in training"""
    r = _rng(12, *shape, seed)
    o = r.standard_normal(shape).astype(F32)
    return o, (o + 0.5 * r.standard_normal(shape)).astype(F32)


def sign_margin(out, tgt):
    """the smallest distance, in units of its float32 rounding error, of any argument of a sgn() from 0, over the three kinds of
    argument: (o - t) never changes sign under rounding (a float32 difference is 0 only for equal operands); |a| - |b| of two
    rounded differences is off by at most 2^-24 (|a| + |b|) before and 2^-24 ||a| - |b|| after its own rounding.  A case whose
    margin is above 2 has the same signs in float32 as in float64: its dout can be held to ``dout_bound``."""
    o, t = np.asarray(out, dtype=F64), np.asarray(tgt, dtype=F64)
    worst = np.inf
    for ax_ in (2, 3):
        a, b = np.diff(o, axis=ax_), np.diff(t, axis=ax_)
        if a.size:
            worst = min(worst, float((np.abs(np.abs(a) - np.abs(b)) / (2.0 ** -24 * (np.abs(a) + np.abs(b)) + 1e-300)).min()))
    return worst


# ---- embedding fold ---------------------------------------------------------------------------------------------------------------
def emb_fold_ref(w, emb, Ct, Ep):
    """W_eff (Cout, Ct + Ep, 9) = [ W[:, :Ct] | T | 0 ],  T[co][i][tap] = sum_e W[co][Ct + e][tap] * emb[i][e]; float64"""
    w, emb = np.asarray(w, dtype=F64), np.asarray(emb, dtype=F64)
    Cout, N = w.shape[0], emb.shape[0]
    weff = np.zeros((Cout, Ct + Ep, 9))
    weff[:, :Ct] = w[:, :Ct]
    weff[:, Ct:Ct + N] = np.einsum("oet,ie->oit", w[:, Ct:], emb)
    return weff


def emb_fold_bwd_ref(w, emb, dweff, Ct, Ep):
    """-> (dW (Cout, Ct + E, 9), demb (N, E)):  dW[:, :Ct] = dW_eff[:, :Ct],  dW[co][Ct + e][tap] = sum_i dW_eff[co][Ct + i][tap] * emb[i][e],
    demb[i][e] = sum_{co, tap} dW_eff[co][Ct + i][tap] * W[co][Ct + e][tap]; float64"""
    w, emb, dweff = np.asarray(w, dtype=F64), np.asarray(emb, dtype=F64), np.asarray(dweff, dtype=F64)
    N = emb.shape[0]
    dT = dweff[:, Ct:Ct + N]
    dw = np.concatenate([dweff[:, :Ct], np.einsum("oit,ie->oet", dT, emb)], axis=1)
    return dw, np.einsum("oit,oet->ie", dT, w[:, Ct:])


def emb_fold_abs_sums(w, emb, dweff, Ct):
    """sum |products| of the three contractions (for the summation bounds): of W_eff's T columns, of dW's embedding columns, of demb"""
    w, emb, dweff = np.abs(np.asarray(w, dtype=F64)), np.abs(np.asarray(emb, dtype=F64)), np.abs(np.asarray(dweff, dtype=F64))
    N = emb.shape[0]
    dT = dweff[:, Ct:Ct + N]
    return np.einsum("oet,ie->oit", w[:, Ct:], emb), np.einsum("oit,ie->oet", dT, emb), np.einsum("oit,oet->ie", dT, w[:, Ct:])


FOLD_EXACT = [(24, 40, 128, 3, 16),                           # (Cout, Ct, E, N, Ep): one chunk
              (33, 0, 64, 16, 16),                            # two chunks, one channel in the second; Ct = 0; Ep == N
              (70, 8, 100, 5, 16),                            # three chunks, the last partial; E no multiple of 64 (the e < E guard)
              (130, 16, 128, 2, 32),                          # five chunks
              (1, 8, 1, 1, 16)]
FOLD_RANDOM = (1024, 64, 128, 16, 16)                         # the deepest folded layer: 32 chunks


def fold_case(dims, seed=0, exact=True):
    """w (Cout, Ct + E, 9), emb (N, E), dweff (Cout, Ct + Ep, 9): integers in [-3, 3], or randn rounded to float32; float64 arrays"""
    Cout, Ct, E, N, Ep = dims
    r = _rng(13, *dims, seed)
    shapes = ((Cout, Ct + E, 9), (N, E), (Cout, Ct + Ep, 9))
    if exact:
        return tuple(r.integers(-3, 4, s).astype(F64) for s in shapes)
    return tuple(r.standard_normal(s).astype(F32).astype(F64) for s in shapes)


# ---- gradient sum -----------------------------------------------------------------------------------------------------------------
def sum_tensors_ref(srcs, dt):
    """float32 adds in the order given, then one conversion to ``dt`` with torch; ``srcs``: tensors holding values of ``dt``"""
    acc = srcs[0].float().clone()
    for s in srcs[1:]:
        acc = acc + s.float()
    return acc.to(dt)


def sum_pixb(C):
    """pixels per workgroup of sum_tensors_kernel: (256 / min(nv, 256)) pixel slots, 8 pixels each"""
    nv = pad8(C) // 8
    return 256 // min(nv, 256) * 8


SUM_K = [1, 2, 8]
SUM_C = [8, 20, 24, 2056]          # nv = 1: pixb = 2048; pad lanes; nv = 3: an idle remainder of threads; nv = 257 > 256: vv strides


def sum_npix(C):
    b = sum_pixb(C)
    return [1, b - 1, b + 1, 3 * b + 5]


# ---- layout boundary --------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(2, 6, 9, 11), (1, 23, 16, 16), (3, 64, 8, 5), (1, 1, 1, 1), (2, 9, 17, 31)]


def _from_bits(patterns):
    return np.array(patterns, dtype=np.uint32).view(F32)


def planted_values():
    """float32 values a conversion to a 16-bit type can get wrong, both signs of each where that makes sense:
    bf16: exact ties (low half 0x8000) under an even and under an odd kept mantissa -- round down, round up --, one above and one
    below a tie, the largest finite value, the largest float32 that still rounds to it, the tie above it (the first value that rounds
    to infinity);  fp16: ties at 1 + 2^-11 (down to even) and 1 + 3 * 2^-11 (up to even), their neighbours, 65504, the largest float32
    below 65520 (rounds to 65504), 65520 (the first value that rounds to infinity), and the subnormal range: 2^-24, the ties 2^-25 (to
    0) and 3 * 2^-25 (to 2^-23), 761.5 * 2^-24 (a tie between subnormals, to even 762), just above 2^-25, 2^-14 - 2^-25 (rounds up
    to the smallest normal), values below half the smallest subnormal;  both infinities, -0.0, a NaN."""
    pos = list(_from_bits([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x40490FDB, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x00800000, 0x3EAA8000]))
    h = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, np.nextafter(F32(1 + 2.0 ** -11), F32(2)), np.nextafter(F32(1 + 3 * 2.0 ** -11), F32(0)),
         65504.0, np.nextafter(F32(65520.0), F32(0)), 65520.0, 65536.0, 1e5,
         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 761.5 * 2.0 ** -24, np.nextafter(F32(2.0 ** -25), F32(1)), 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14,
         2.0 ** -26, 5.3e-6, 3.1e-5, 6.0e-5, 2.5 * 2.0 ** -24, 1023.5 * 2.0 ** -24]
    pos = np.array(pos + h, dtype=F32)
    return np.concatenate([pos, -pos, np.array([np.inf, -np.inf, -0.0, 0.0, np.nan], dtype=F32)])


def layout_case(shape, seed=0):
    """(N, C, H, W) float32: randn with the planted values spread over it (a tensor smaller than their list holds its first ones)"""
    r = _rng(14, *shape, seed)
    x = r.standard_normal(shape).astype(F32)
    v = planted_values()
    flat = x.reshape(-1)
    if flat.size <= v.size:
        flat[:] = v[:flat.size]
    else:
        step = flat.size // v.size
        flat[(np.arange(v.size) * step + seed) % flat.size] = v
    return x
