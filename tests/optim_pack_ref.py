"""Plain references of the fused optimizer step (csrc/optim.hip: ``opt_pack_kernel`` behind ``mau_opt_pack_step`` / ``mau_adamw_pack_step``)
and of the matrix-core weight packs (csrc/conv3x3.hip: ``pack_tile`` behind ``mau_conv3x3_pack_weights`` / ``_multi``): numpy float64 and
torch on the CPU, written from include/mau_hip.h and the opening comment of optim.hip, no device.

``step_ref`` is the update rule in float64, ``pack_ref`` the placement of an OIHW tensor into a pack buffer.  The generators of the
"exact" cases live here too: dyadic inputs and power-of-two (or 3/4) hyper-parameters, for which every intermediate of the rules is a
float32 (tests/test_optim_pack_host.py asserts that per intermediate), so that neither the order of the operations nor a fused
multiply-add can change a bit and the device must return the reference's bits.  ``adam_bound`` is the tolerance rule of what is not exact."""
import numpy as np
import torch

ADAMW, ADAM, SGD = 0, 1, 2                                    # MAU_OPT_* of include/mau_hip.h
RULES = {"adamw": ADAMW, "adam": ADAM, "sgd": SGD}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
KC = 16                                                       # channels of a chunk, every type
# (Cout, Cin): one element; less than a chunk; a ragged second chunk; one full block; a 1-row / 1-column second block; ragged last
# blocks in both dimensions with 2 x 3 and 3 x 2 blocks; 13 chunks against 2 over 4 blocks; 2 x 2 full blocks
SHAPES = [(1, 1), (3, 5), (16, 23), (64, 64), (65, 64), (64, 65), (72, 130), (130, 72), (17, 200), (128, 128)]
SHAPE_IDS = [f"{a}x{b}" for a, b in SHAPES]


def f32(x):
    """a hyper-parameter as the C ABI receives it: rounded to float32, widened again"""
    return float(np.float32(x))


def is_f32(x):
    """every element exactly representable in float32"""
    x = np.asarray(x, dtype=np.float64)
    return bool((x.astype(np.float32).astype(np.float64) == x).all())


def to_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).float()


# ---- the update rules ------------------------------------------------------------------------------------------------------------------
def step_ref(rule, p, g, m, v, *, step=1, lr, beta1, beta2=0.0, eps=0.0, wd=0.0, nesterov=False, grad_scale=None, f32_hyper=True, trace=None):
    """One step of ``rule`` in float64 -> the new (p, m, v); ``m`` / ``v`` come back None where the rule has none.

    AdamW:  p <- p (1 - lr wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    Adam:   g <- g + wd p, then the moments and the step above without the decay
    SGD:    g <- g + wd p;  buf <- mu buf + g;  p <- p - lr (nesterov ? g + mu buf : buf);  beta1 is mu, m the buffer (None: p <- p - lr g)
    ``grad_scale`` multiplies g before anything else.  The hyper-parameters are rounded to float32 first, as the C ABI receives them
    (``f32_hyper=False``: taken as they are, for the comparison with torch in float64).  ``trace``: a dict that receives every
    intermediate by name."""
    h = f32 if f32_hyper else float
    lr, b1, b2, eps, wd = h(lr), h(beta1), h(beta2), h(eps), h(wd)
    t = float(step)
    tr = trace if trace is not None else {}
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if grad_scale is not None:
        g = tr["g_scaled"] = g * h(grad_scale)
    if rule == SGD:
        if wd != 0.0:
            tr["wd_p"] = wd * p
            g = tr["g_decayed"] = g + wd * p
        if m is not None:
            tr["mu_buf"] = b1 * np.asarray(m, dtype=np.float64)
            m = tr["buf"] = tr["mu_buf"] + g
            if nesterov:
                tr["mu_newbuf"] = b1 * m
                g = tr["g_nesterov"] = g + b1 * m
            else:
                g = m
        tr["lr_g"] = lr * g
        p = tr["p"] = p - lr * g
        return p, m, None
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if rule == ADAMW:
        tr["decay"] = np.float64(1.0 - lr * wd)
        p = tr["p_decayed"] = p * (1.0 - lr * wd)
    elif wd != 0.0:
        tr["wd_p"] = wd * p
        g = tr["g_decayed"] = g + wd * p
    tr["b1_m"], tr["omb1_g"] = b1 * m, (1.0 - b1) * g
    m = tr["m"] = b1 * m + (1.0 - b1) * g
    tr["b2_v"], tr["g2"], tr["omb2_g2"] = b2 * v, g * g, (1.0 - b2) * g * g
    v = tr["v"] = b2 * v + (1.0 - b2) * g * g
    tr["b1_t"], tr["b2_t"] = np.float64(b1 ** t), np.float64(b2 ** t)
    bc1, bc2 = tr["bc1"], tr["bc2"] = np.float64(1.0 - b1 ** t), np.float64(1.0 - b2 ** t)
    step_size = lr / bc1
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    tr["update"] = step_size * m / denom
    p = tr["p"] = p - tr["update"]
    return p, m, v


# The tolerance rule of the Adam family.  With e = 2^-24 (half a unit in the last place, the relative error of ONE rounding) the kernel's
# chain is, every figure relative to the quantity named:
#   the parameter itself                                                                        relative to |p_ref|
#     1 - lr wd (its product's error is lr wd e: nothing), p * decay, the final subtraction      3    (*)
#   the update D = step_size * (m / denom)                                                      relative to |D|
#     g * grad_scale, where there is one: once in m, once in denom (twice in v, halved by the root)   2
#     m:  (1 - b1) g, the multiply-add                                                           2
#     v:  (1 - b2) g, * g, the multiply-add: 3, halved by the root; sqrtf                        2.5
#     sqrt(1 - b2^t): the subtraction halved by the root, sqrtf                                  1.5
#     / bc2s, + eps, m / denom, lr / bc1 and bc1's subtraction, step_size * ( )                  6
#     (*) the two roundings in front of the subtraction are relative to |p decay| <= |p_ref| + |D|       2
#                                                                                                16 in all, 14 without grad_scale
#   powf, allowed 2 units in the last place = 4 e: 1 - b^t magnifies it by b^t / (1 - b^t), the root of the second halves it; with
#   4 <= K these are the two amplification terms of the bound, which are derived, not tuned.
# Hence  |p_got - p_ref| <= K e (|p_ref| + |D| (1 + b1^t / (1 - b1^t) + b2^t / (2 (1 - b2^t)))),  K = 16, D the reference's update.
# m and v on their own: 3 and 5 roundings with grad_scale, each relative to the magnitude of what is added: v's addends are >= 0, so
# that is v itself; exp_avg's are b1 m and (1 - b1) g, which may cancel, and a rounding of an addend is relative to the addend, not to
# a difference that can be arbitrarily small: |b1 m| + |(1 - b1) g|, which is |m_new| wherever the two have one sign.
K = 16.0
E32 = 2.0 ** -24


def adam_bound(p_ref, trace):
    """the bound of |p_got - p_ref| from the trace of the ``step_ref`` call that gave ``p_ref``"""
    a1 = trace["b1_t"] / trace["bc1"]
    a2 = trace["b2_t"] / trace["bc2"]
    return K * E32 * (np.abs(p_ref) + np.abs(trace["update"]) * (1.0 + a1 + 0.5 * a2))


def moment_bounds(trace):
    """the bounds of |m_got - m_ref| and |v_got - v_ref|: K roundings of their own magnitude"""
    return K * E32 * (np.abs(trace["b1_m"]) + np.abs(trace["omb1_g"])), K * E32 * trace["v"]


# ---- the packs -------------------------------------------------------------------------------------------------------------------------
def pad64(c):
    return (c + 63) // 64 * 64


def packed_elems(rows, k):
    """mau_conv3x3_packed_elems(dtype, nout = rows, nin = k): [k / 16][9][rows64][16]"""
    return -(-k // KC) * 9 * pad64(rows) * KC


def row_channel(q, dtype):
    """the channel that position q of the row dimension holds: inside every 64-row block, 2 (q & 31) + (q >> 5) for the 16-bit types"""
    q = np.asarray(q)
    if dtype == torch.float32:
        return q
    r = q & 63
    return (q - r) + 2 * (r & 31) + (r >> 5)


def _place(a, dtype, fill):
    """a (rows, k, 9) tensor, tap order as stored -> flat [chunk][tap][rows64][16], ``fill`` where the channel lies beyond rows or k"""
    rows, k, _ = a.shape
    nch, rp = -(-k // KC), pad64(rows)
    full = torch.full((rp, nch * KC, 9), fill, dtype=a.dtype)
    full[:rows, :k] = a
    full = full[torch.from_numpy(row_channel(np.arange(rp), dtype))]
    return full.reshape(rp, nch, KC, 9).permute(1, 3, 0, 2).reshape(-1).contiguous()


def _as_rows(w, which):
    """OIHW (Cout, Cin, 3, 3) -> (rows, k, 9): the forward pack keeps (co, ci, tap); the data-gradient pack has rows ci, k co and the
    taps rotated by 180 degrees (tap 8 - t of the pack holds tap t of w)"""
    w = w.reshape(w.shape[0], w.shape[1], 9)
    if which == "wf":
        return w
    assert which == "wd", which
    return w.permute(1, 0, 2).flip(-1)


def pack_ref(w, dtype, which):
    """-> (the pack ``which`` in {"wf", "wd"} of the float32 OIHW tensor ``w`` as a flat tensor of ``dtype``, the boolean mask of the
    elements a launch must write).  The mask is the whole buffer: the zero pads of channels beyond Cout / Cin are written too."""
    assert w.dtype == torch.float32 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
    out = _place(_as_rows(w, which), dtype, 0.0).to(dtype)
    return out, torch.ones(out.shape, dtype=torch.bool)


def pack_index(Cout, Cin, dtype, which):
    """the placement alone: for every element of the pack the flat index into the OIHW tensor of the weight it holds, -1 for a pad"""
    idx = torch.arange(Cout * Cin * 9, dtype=torch.int64).reshape(Cout, Cin, 3, 3)
    return _place(_as_rows(idx, which), dtype, -1)


def pack_loop(w, dtype, which):
    """``pack_ref`` once more, element by element from the header's sentence -- the check of the vectorised form on small shapes"""
    Cout, Cin = w.shape[:2]
    rows, k = (Cout, Cin) if which == "wf" else (Cin, Cout)
    rp = pad64(rows)
    out = torch.zeros(packed_elems(rows, k), dtype=torch.float32)
    for co in range(Cout):
        for ci in range(Cin):
            row, kk = (co, ci) if which == "wf" else (ci, co)
            pos = [q for q in range(row & ~63, (row & ~63) + 64) if int(row_channel(q, dtype)) == row]
            assert len(pos) == 1
            for tap in range(9):
                tp = tap if which == "wf" else 8 - tap
                out[(((kk // KC) * 9 + tp) * rp + pos[0]) * KC + kk % KC] = w[co, ci, tap // 3, tap % 3]
    return out.to(dtype)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20240611, *key])


def random_weights(Cout, Cin, seed=0):
    return to_f32(_rng(1, Cout, Cin, seed).standard_normal((Cout, Cin, 3, 3)))


def tie_weights(Cout, Cin, seed=0):
    """dyadic weights with many exact ties of round-to-nearest-even: (2 j + 1) 2^-9 s with j < 256 is an odd multiple of half a unit of
    the 8-bit significand of bf16, (2 j + 1) 2^-12 s with j < 2048 of the 11-bit one of fp16 (s a power of two in fp16's normal range);
    both kinds with both parities of the kept last bit, some values exact in either type, signs mixed"""
    r = _rng(2, Cout, Cin, seed)
    n = Cout * Cin * 9
    kind = r.integers(0, 3, n)
    s = 2.0 ** r.integers(-6, 4, n)
    odd8, odd11 = 2 * r.integers(128, 256, n) + 1, 2 * r.integers(1024, 2048, n) + 1
    val = np.where(kind == 0, odd8 * 2.0 ** -9, np.where(kind == 1, odd11 * 2.0 ** -12, r.integers(128, 256, n) * 2.0 ** -8)) * s
    val *= r.choice([-1.0, 1.0], n)
    assert is_f32(val)
    return to_f32(val.reshape(Cout, Cin, 3, 3))


def exact_values(Cout, Cin, dtype, seed=0):
    """random weights exact in ``dtype`` (8 significant bits: exact in every type), nonzero, for the inversion of the placement"""
    r = _rng(3, Cout, Cin, seed)
    return to_f32((r.integers(128, 256, (Cout, Cin, 3, 3)) * 2.0 ** r.integers(-8, 0, (Cout, Cin, 3, 3))) * r.choice([-1.0, 1.0], (Cout, Cin, 3, 3)))


# the exact grids: p in k/8, |k| <= 16;  g in k/4, |k| <= 8;  a momentum buffer / exp_avg from p's grid;  v in k/16, 0 <= k <= 32
SGD_EXACT = dict(lr=2.0 ** -3, beta1=0.5, wd=0.25)
SGD_EXACT_SCALE = 0.5
ADAM_EXACT = dict(lr=2.0 ** -6, beta1=0.5, beta2=0.75, eps=2.0 ** -10)
ADAM_EXACT_WD = 0.25
EXACT_STEPS = [1, 2, 7, 12]
# plain (no buffer), momentum, nesterov with weight decay
SGD_CONFIGS = {"plain": dict(momentum=False, nesterov=False, wd=0.0), "momentum": dict(momentum=True, nesterov=False, wd=0.0),
               "nesterov_wd": dict(momentum=True, nesterov=True, wd=SGD_EXACT["wd"])}


def exact_case(Cout, Cin, seed=0):
    """{"p", "g", "m", "v"}: float64 arrays (Cout, Cin, 3, 3) on the dyadic grids"""
    r = _rng(4, Cout, Cin, seed)
    shape = (Cout, Cin, 3, 3)
    return {"p": r.integers(-16, 17, shape) / 8.0, "g": r.integers(-8, 9, shape) / 4.0, "m": r.integers(-16, 17, shape) / 8.0,
            "v": r.integers(0, 33, shape) / 16.0}


PRODUCTION_STEPS = [1, 2, 10, 1000, 100000]


def random_case(Cout, Cin, seed=0):
    """float32-valued float64 arrays: weights of a few tenths, gradients and exp_avg of both signs over three decades, exp_avg_sq over
    six (independent of g: the denominator is tried against every size of the numerator); one element in 16 has g = 0, half of those
    v = 0 as well (m / eps: the largest update there is)"""
    r = _rng(5, Cout, Cin, seed)
    shape = (Cout, Cin, 3, 3)
    f = lambda x: x.astype(np.float32).astype(np.float64)      # noqa: E731
    p = r.standard_normal(shape) * 0.2
    g = r.standard_normal(shape) * 10.0 ** r.uniform(-4, -1, shape)
    m = r.standard_normal(shape) * 10.0 ** r.uniform(-4, -1, shape)
    v = 10.0 ** r.uniform(-9, -3, shape)
    zero = r.integers(0, 16, shape)
    g[zero <= 1] = 0.0
    v[zero == 0] = 0.0
    return {"p": f(p), "g": f(g), "m": f(m), "v": f(v)}
