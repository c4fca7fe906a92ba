"""Plain references of the BatchNorm-backward kernels (csrc/bn.hip), their fused forms and the output head (csrc/bn_fused.hip,
csrc/head.hip): numpy float64 on the CPU, written from the formulas, no device.

Layout: an activation-like tensor is a float64 array (npix, C), pixels in NHWC order (n, y, x); the head's out / dout are
(N, Co, HW).  Rounding to the tensor type is ``torch.Tensor.to(dtype)`` (``round_t``).  The generators of the "exact" cases live
here too: every addend of every sum they lead to is a small integer or dyadic fraction, so the sums are exact in float32 in any
order (tests/test_bn_head_host.py proves that for every generated case) and a kernel's result must equal the reference bit for bit."""
import numpy as np
import torch

BLOCK = 1024                                                  # BWD_PIX_PER_BLOCK / HEAD_PIX_PER_BLOCK: pixels per slab row
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]


def pad8(c):
    return (c + 7) // 8 * 8


def round_t(x, dt):
    """float64 array -> the values of ``dt``, as float64 (through float32: exact where the value is a float32, as in the exact cases)"""
    if dt in (None, torch.float64):
        return np.asarray(x, dtype=np.float64)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).float()
    return t.to(dt).double().numpy()


def is_f32(x):
    """every element exactly representable in float32"""
    x = np.asarray(x, dtype=np.float64)
    return bool((x.astype(np.float32).astype(np.float64) == x).all())


# ---- BatchNorm + ReLU forward, 2x2 max pool, its adjoint ---------------------------------------------------------------------
def bn_relu_apply(y, scale, shift, dt):
    return round_t(np.maximum(scale * y + shift, 0.0), dt)


def _windows(a, N, H, W):
    """(4, N, Ho, Wo, C): the four pixels of every 2x2 window in scan order (position 2*dy + dx), floor semantics"""
    Ho, Wo = H // 2, W // 2
    v = a.reshape(N, H, W, -1)
    return np.stack([v[:, dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)])


def pool_first_max(a, N, H, W):
    """a (npix, C), already rounded to the tensor type -> pooled (nwin, C), position of the window's FIRST maximum (nwin, C):
    numpy's argmax returns the first occurrence in scan order, i.e. a later element wins only if strictly greater."""
    win = _windows(a, N, H, W)
    C = a.shape[1]
    return win.max(0).reshape(-1, C), win.argmax(0).reshape(-1, C)


def pack_argidx(arg):
    """(nwin, C) positions -> (nwin, C8 / 8) uint16, 2 bits per channel; pad lanes hold four equal zeros: position 0"""
    nwin, C = arg.shape
    full = np.zeros((nwin, pad8(C)), dtype=np.int64)
    full[:, :C] = arg
    return (full.reshape(nwin, -1, 8) << (2 * np.arange(8))).sum(-1).astype(np.uint16)


def pool_scatter(dpl, arg, N, H, W):
    """dpl (nwin, C) to the pixel ``arg`` names in each window, 0 elsewhere (and in a last odd row / column) -> (npix, C)"""
    Ho, Wo = H // 2, W // 2
    C = dpl.shape[1]
    out = np.zeros((N, H, W, C))
    g, k = dpl.reshape(N, Ho, Wo, C), arg.reshape(N, Ho, Wo, C)
    for u in range(4):
        out[:, u // 2:2 * Ho:2, u % 2:2 * Wo:2] = np.where(k == u, g, 0.0)
    return out.reshape(-1, C)


def pool_da_pre(dpl, arg, dskip, N, H, W):
    """dskip + scatter(dpl) before rounding; either term may be None"""
    r = 0.0
    if dpl is not None:
        r = r + pool_scatter(dpl, arg, N, H, W)
    if dskip is not None:
        r = r + dskip
    return r


# ---- BatchNorm backward ----------------------------------------------------------------------------------------------------
def block_sums(x):
    """(npix, ...) -> (blocks, ...): sums over blocks of BLOCK consecutive pixels"""
    return np.add.reduceat(x, np.arange(0, x.shape[0], BLOCK), axis=0) + 0.0          # (+ 0.0: a sum of zeros is +0, as a sum that starts at +0 is)


class BnBwd:
    """dz = (scale*y+shift > 0) ? da : 0;  slab[b] = [sum dz | sum dz*xhat] over block b;  dy = sc*(dz - m1 - xhat*m2) with the
    means over ``count`` (the pixel count unless given).  ``dy`` is not rounded."""

    def __init__(self, da, y, k, count=None):
        self.act = k["scale"] * y + k["shift"]
        self.dz = np.where(self.act > 0, da, 0.0)
        self.xhat = (y - k["mean"]) * k["invstd"]
        self.add1, self.add2 = self.dz, self.dz * self.xhat
        self.slab = np.stack([block_sums(self.add1), block_sums(self.add2)], axis=1)            # (blocks, 2, C)
        self.sums = np.concatenate([self.add1.sum(0), self.add2.sum(0)]) + 0.0
        self.count = float(y.shape[0] if count is None else count)
        self.m1, self.m2 = self.sums[:y.shape[1]] / self.count, self.sums[y.shape[1]:] / self.count
        self.dy = k["scale"] * (self.dz - self.m1 - self.xhat * self.m2)


# ---- the head ---------------------------------------------------------------------------------------------------------------
def head_pre(a, w, b, N, HW):
    """1x1 conv + bias: a (npix, C), w (Co, C), b (Co) -> (N, Co, HW), before the tanh"""
    return (a @ w.T + b).reshape(N, HW, -1).transpose(0, 2, 1)


def head_fwd(a, w, b, N, HW, tanh0):
    out = head_pre(a, w, b, N, HW).copy()
    if tanh0:
        out[:, 0] = np.tanh(out[:, 0])
    return out


class HeadBwd:
    """dz = dout * (1 - out^2) on the tanh channel;  da = W^T dz (``da_pre``, not rounded);  per block dW = sum dz (x) a, db = sum dz"""

    def __init__(self, a, w, out, dout, tanh0):
        N, Co, HW = dout.shape
        dz = dout.copy()
        if tanh0:
            dz[:, 0] = dout[:, 0] * (1.0 - out[:, 0] ** 2)
        self.dz = dz.transpose(0, 2, 1).reshape(N * HW, Co)                                   # (npix, Co)
        self.da_pre = self.dz @ w + 0.0
        self.addw = self.dz[:, :, None] * a[:, None, :]                                       # (npix, Co, C)
        self.dW, self.db = block_sums(self.addw), block_sums(self.dz)

    def slab(self, C):
        """rows [Co][C8 + 8]: dW in columns [0, C), 0 in the pad lanes, db at column C8, NaN in the 7 columns nothing writes"""
        nb, Co = self.db.shape
        C8 = pad8(C)
        s = np.full((nb, Co, C8 + 8), np.nan)
        s[:, :, :C], s[:, :, C:C8], s[:, :, C8] = self.dW, 0.0, self.db
        return s


def ulp_distance_f32(got, want):
    """distance in float32 units in the last place between two float32 arrays (same sign or zero)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(got) - key(want))


# ---- shapes -------------------------------------------------------------------------------------------------------------------
BN_NPIX = [5, 33, 1023, 1024, 1025, 2 * 1024 + 97]
BN_C = [3, 8, 20, 64, 70, 130]
BN_WIDE = [(70, 1024), (40, 2056)]                            # (npix, C): nv = 128 (two pixel slots), nv > 256 (the outer vector loop)
POOL_SHAPES = [(1, 2, 2), (2, 5, 7), (3, 4, 3), (1, 33, 31), (2, 32, 34)]
POOL_C = [3, 20, 64, 70]
HEAD_CO = [1, 2, 3, 4]
HEAD_BN_C = [3, 20, 64]
HEAD_C = [3, 64, 72, 130]
HEAD_BN_SHAPES = [(3, 35), (1, 32), (2, 1024 + 37), (5, 300)]
HEAD_SHAPES = HEAD_BN_SHAPES + [(4, 12)]
RANDOM_C, RANDOM_POOL, RANDOM_HEAD = 70, (2, 33, 32), (2, 1056)      # about 2100 pixels
RANDOM_HEAD_C = 64                                           # (the BatchNorm-fused head takes at most 64 channels)
EXACT_COUNT = 4096.0                                         # the power-of-two ``count`` of the exact apply cases ...
HEAD_EXACT_COUNT = 64.0                                      # ... and of the head's, whose da has 1/32 as its unit: dy stays within 24 bits


# ---- generators ---------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([abs(int(v)) for v in key])


def exact_coefs(C, seed):
    """scale, invstd: powers of two; shift, mean: integers or halves"""
    r = _rng(1, C, seed)
    return {"scale": r.choice([0.25, 0.5, 1.0, 2.0], C), "invstd": r.choice([0.5, 1.0, 2.0], C),
            "shift": r.integers(-4, 5, C) / 2.0, "mean": r.integers(-4, 5, C) / 2.0}


def random_coefs(C, seed):
    r = _rng(2, C, seed)
    f = lambda v: v.astype(np.float32).astype(np.float64)      # noqa: E731  (the kernels receive float32 coefficients)
    return {"scale": f(r.standard_normal(C)), "invstd": f(r.uniform(0.5, 2.0, C)), "shift": f(r.standard_normal(C)), "mean": f(r.standard_normal(C))}


def ints(r, shape, lo, hi):
    return r.integers(lo, hi + 1, shape).astype(np.float64)


def exact_bn_case(npix, C, seed=0):
    r = _rng(3, npix, C, seed)
    return {"y": ints(r, (npix, C), -4, 4), "da": ints(r, (npix, C), -3, 3), "k": exact_coefs(C, seed)}


def exact_pool_case(N, H, W, C, seed=0):
    """y in -2..2: relu(scale*y+shift) takes few values and many zeros: most windows have several maxima"""
    r = _rng(4, N, H, W, C, seed)
    return {"y": ints(r, (N * H * W, C), -2, 2), "dpl": ints(r, (N * (H // 2) * (W // 2), C), -3, 3), "dskip": ints(r, (N * H * W, C), -3, 3),
            "k": exact_coefs(C, seed)}


def exact_head_case(N, HW, C, Co, seed=0):
    """The head's operands.  ``a`` (the plain head's input): quarters in [0, 2], half of them 0; ``y`` + ``k`` (the BatchNorm-fused
    head's input): relu(scale*y+shift) is a multiple of 1/8 below 10.  Weights: small integers, those of channel 0 in halves so
    that the tanh's exact argument spreads over a few units instead of saturating.  out[:, 0] in {0, +-0.25, +-0.5}."""
    r = _rng(5, N, HW, C, Co, seed)
    npix = N * HW
    w = ints(r, (Co, C), -2, 2)
    w[0] /= 2.0
    out = ints(r, (N, Co, HW), -3, 3)
    out[:, 0] = r.choice([0.0, 0.25, -0.25, 0.5, -0.5], (N, HW))
    return {"a": ints(r, (npix, C), 0, 8) / 4.0 * (r.random((npix, C)) < 0.5), "y": ints(r, (npix, C), -4, 4), "k": exact_coefs(C, seed),
            "w": w, "b": r.integers(-4, 5, Co) / 4.0, "out": out, "dout": ints(r, (N, Co, HW), -3, 3)}


def random_case(npix, C, seed, dt, extra=()):
    """randn tensors rounded to ``dt`` (what the device tensor holds): y, da and the named extras, all (npix, C)"""
    r = _rng(6, npix, C, seed)
    return {name: round_t(r.standard_normal((npix, C)), dt) for name in ("y", "da") + tuple(extra)}


# ---- bounds of the random cases (issue, section 3) ----------------------------------------------------------------------------
def slab_bound(addends):
    """fp32 accumulation of a block's addends in any order: 2^-24 * n * sum |addend|, per block"""
    n = np.diff(np.append(np.arange(0, addends.shape[0], BLOCK), addends.shape[0]))
    return 2.0 ** -24 * n.reshape((-1,) + (1,) * (addends.ndim - 1)) * block_sums(np.abs(addends))


def dy_bound_f32(B, y, k):
    """8 * 2^-24 * (|sc*dz| + |sc*m1| + |k1| * (|mean| + |y|)), k1 = sc*m2*invstd: six roundings of the k0 / k1 form plus slack"""
    k1 = k["scale"] * B.m2 * k["invstd"]
    return 8 * 2.0 ** -24 * (np.abs(k["scale"] * B.dz) + np.abs(k["scale"] * B.m1) + np.abs(k1) * (np.abs(k["mean"]) + np.abs(y)))


def type_ulp(v, dt):
    """spacing of ``dt`` at |v| (float64 array), subnormal range included"""
    p, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dt]
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return 2.0 ** (e - (p - 1))


def mask_uncertain(B, y, k):
    """pixels whose scale*y+shift lies within the fp32 dy bound of 0: the kernel's mask may legitimately differ there"""
    return np.abs(B.act) <= dy_bound_f32(B, y, k)
