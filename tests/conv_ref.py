"""Data builders and float64 references of the 3x3 convolution tests (tests/test_conv_pinned_host.py proves them on the CPU,
tests/test_gpu_conv_pinned.py holds the kernels to them).

DYADIC FULL-MANTISSA DATA.  One operand of every product is "full": m * 2^-s with |m| < 2^p, p the significand width of the tensor
type (bf16 8, fp16 11; fp32 starts at 12), and in more than half of the values m is odd with its top bit set -- the highest and the
lowest significand bit are both in use.  The other operand is sign * 2^j, sign in {-1, 0, +1}.  Every product is then a multiple of
the PRODUCT QUANTUM q (the smallest power of two that divides every term), and while sum |x| |w| + |b| < 2^24 * q per output element
every partial sum ANY summation order can form is a multiple of q below 2^24 * q: an exactly representable fp32 number.  The float64
convolution is then the exact real result, an fp32 kernel must reproduce it bit for bit whatever its tiling, and a 16-bit kernel that
result rounded ONCE, to nearest even.  A kernel that drops an operand bit, accumulates in 16 bits, or truncates on the store does not.

The bound is asserted from the data of every case (``assert_exact``), never taken from the seed."""
import functools

import torch
import torch.nn.functional as TF

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16, F32)
DT_NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
SIG_BITS = {BF16: 8, F16: 11, F32: 24}                       # significand width of the type
FULL_P = {BF16: 8, F16: 11, F32: 12}                          # significand bits of the full operand (fp32: narrowed where K is wide)
U32 = 2.0 ** -24                                              # unit roundoff of fp32


def gamma(n):
    """the fp32 recursive-summation constant n u / (1 - n u)"""
    return n * U32 / (1.0 - n * U32)


# ------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------
def full_operand(g, shape, p):
    """float64 values m * 2^-(p-1), |m| < 2^p: 60 % of them (counted, at random places) with m odd and |m| >= 2^(p-1), the rest uniform
    over the whole range"""
    top = (1 << (p - 1)) + 2 * torch.randint(0, 1 << (p - 2), shape, generator=g) + 1
    rest = torch.randint(0, 1 << p, shape, generator=g)
    n = top.numel()
    pick = (torch.randperm(n, generator=g) < -(-3 * n // 5)).view(shape)
    m = torch.where(pick, top, rest) * (1 - 2 * torch.randint(0, 2, shape, generator=g))
    return m.double() * 2.0 ** -(p - 1)


def pow2_operand(g, shape, js, zero):
    """float64 values sign * 2^j, j drawn from ``js`` and sign from {-1, +1} independently per element, 0 with probability ``zero``"""
    j = torch.tensor(js, dtype=torch.float64)[torch.randint(0, len(js), shape, generator=g)]
    sign = (1 - 2 * torch.randint(0, 2, shape, generator=g)).double() * (torch.rand(shape, generator=g) >= zero).double()
    return sign * torch.exp2(j)


def quantum(*tensors):
    """the largest power of two that divides every non-zero element of the tensors (1.0 when there is none)"""
    q = float("inf")
    for t_ in tensors:
        a = t_.double().abs().flatten()
        a = a[a != 0]
        if a.numel() == 0:
            continue
        m, e = torch.frexp(a)                                 # a = m * 2^e, m in [0.5, 1): k = m * 2^53 is the integer significand
        k = (m * 2.0 ** 53).to(torch.int64)
        low = (k & -k).double()                               # its lowest set bit
        q = min(q, float((low * torch.exp2((e - 53).double())).min()))
    return 1.0 if q == float("inf") else q


def full_share(t_, p):
    """share of the elements whose significand is p bits wide with the top AND the bottom bit set (m odd, |m| >= 2^(p-1))"""
    m = (t_.double().abs() * 2.0 ** (p - 1)).to(torch.int64)
    return float(((m >= (1 << (p - 1))) & (m % 2 == 1)).double().mean())


def representable(t_, dt):
    return t_.double() == t_.to(dt).double() if dt != F32 else t_.double() == t_.float().double()


def round_dt(y64, dt):
    """a float64 result that is exact in fp32, rounded ONCE to the tensor type (nearest even), as float32"""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "the reference is not exact in fp32"
    return y32.to(dt).float()


def trunc_sig(t_, bits):
    """every element with its significand cut to ``bits`` bits, toward zero (float64 in, float64 out)"""
    m, e = torch.frexp(t_.double())
    return torch.ldexp(torch.trunc(m * 2.0 ** bits) * 2.0 ** -bits, e)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
ROLES = ("x-full", "w-full")
# what is tried, in this order, until the data satisfy the bound: the exponent set of the power-of-two operand and its share of zeros
_LADDER = (((-1, 0, 1), 1 / 3), ((0,), 1 / 3), ((0,), 0.75), ((0,), 0.9375))


def _seed(*key):
    return sum((i + 1) * 1000003 * int(v) for i, v in enumerate(key)) % (2 ** 31)


class Case:
    """One convolution: x (N,Cin,H,W), w (Cout,Cin,3,3), b, post_scale, post_shift as float64 tensors that the tensor type ``dt`` (x)
    and fp32 / ``dt`` (w: the pack converts it) hold exactly; q the product quantum; y / post the exact results (float64)."""

    def __init__(self, shape, dt, role, p, js, zero, emb=0, salt=0):
        N, Cin, Cout, H, W = shape
        self.shape, self.dt, self.role, self.p, self.js, self.zero, self.E = shape, dt, role, p, js, zero, emb
        g = torch.Generator().manual_seed(_seed(*shape, p, len(js), int(zero * 16), role == "x-full", emb, salt))
        xs, ws = (N, Cin, H, W), (Cout, Cin, 3, 3)
        if role == "x-full":
            self.x, self.w = full_operand(g, xs, p), pow2_operand(g, ws, js, zero)
        else:
            self.x, self.w = pow2_operand(g, xs, js, zero), full_operand(g, ws, p)
        if emb:                                               # the last ``emb`` channels: one value per image (the broadcast embedding)
            self.x[:, Cin - emb:] = self.x[:, Cin - emb:, :1, :1].clone()
        self.q = quantum(self.x) * quantum(self.w)
        self.b = torch.randint(-64, 65, (Cout,), generator=g).double() * self.q
        # inference epilogue relu(scale * (conv + bias) + shift): scales +-2^j, one in four negative; shifts multiples of the quantum
        self.sc = torch.exp2(torch.randint(-1, 2, (Cout,), generator=g).double()) * (1 - 2 * (torch.arange(Cout) % 4 == 1).double())
        self.qpost = self.q * 0.5
        self.sh = torch.randint(-256, 257, (Cout,), generator=g).double() * self.qpost

    @functools.cached_property
    def absum(self):
        """sum |x| |w| + |b| per output element, float64 (exact: the same quantum argument)"""
        return TF.conv2d(self.x.abs(), self.w.abs(), self.b.abs(), padding=1)

    def exact(self):
        post = self.absum * self.sc.abs()[None, :, None, None] + self.sh.abs()[None, :, None, None]
        return float(self.absum.max()) < 2.0 ** 24 * self.q and float(post.max()) < 2.0 ** 24 * self.qpost

    @functools.cached_property
    def y(self):
        return TF.conv2d(self.x, self.w, self.b, padding=1)

    @functools.cached_property
    def y_nobias(self):
        return TF.conv2d(self.x, self.w, None, padding=1)

    @functools.cached_property
    def post(self):
        return torch.relu(self.sc[None, :, None, None] * self.y + self.sh[None, :, None, None])

    @property
    def full(self):
        return self.x if self.role == "x-full" else self.w


def assert_operands(c):
    """the operands are what the docstring of this module promises: representable, and more than half full"""
    assert bool(representable(c.x, c.dt).all()) and bool(representable(c.w, c.dt).all())
    assert bool(representable(c.b, F32).all()) and bool(representable(c.sc, F32).all()) and bool(representable(c.sh, F32).all())
    assert c.p <= SIG_BITS[c.dt] and (c.dt == F32 or c.p == SIG_BITS[c.dt])
    assert full_share(c.full, c.p) >= 0.5, full_share(c.full, c.p)


def assert_exact(c):
    """exactness of everything the tests compare bit for bit rests on this, not on the seed"""
    assert c.exact(), (c.shape, DT_NAME[c.dt], c.role, float(c.absum.max()), 2.0 ** 24 * c.q)


@functools.lru_cache(maxsize=12)
def conv_case(shape, dt, role, emb=0, salt=0):
    """The first rung of the ladder whose DATA satisfy the bound; fp32 narrows p below 12 once the ladder is used up."""
    p = FULL_P[dt]
    while True:
        for js, zero in _LADDER:
            c = Case(shape, dt, role, p, js, zero, emb, salt)
            if c.exact():
                assert_exact(c)
                return c
        assert dt == F32 and p > 8, f"no exact case for {shape} {DT_NAME[dt]} {role}"
        p -= 1


def dgrad_case(shape, dt, role):
    """The data gradient of the layer ``shape`` = (N, Cin, Cout, H, W) as the convolution it is: input dy (N,Cout,H,W), weights
    w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx], no bias.  Returns (case over dy and w', the layer's OIHW weights w)."""
    N, Cin, Cout, H, W = shape
    c = conv_case((N, Cout, Cin, H, W), dt, role, 0, 1)
    return c, c.w.transpose(0, 1).flip(2, 3).contiguous()


class WgradCase:
    """x (N,Cin,H,W) and dy (N,Cout,H,W): the weight gradient sums over PIXELS, so the bound is on sum over pixels |x| |dy| per dw
    element.  Role "x-full": x full, dy a power of two; "w-full": dy full, x a power of two."""

    def __init__(self, shape, dt, role, p, js, zero, emb=0):
        N, Cin, Cout, H, W = shape
        self.shape, self.dt, self.role, self.p, self.js, self.zero, self.E = shape, dt, role, p, js, zero, emb
        g = torch.Generator().manual_seed(_seed(*shape, p, len(js), int(zero * 16), role == "x-full", emb, 77))
        xs, ds = (N, Cin, H, W), (N, Cout, H, W)
        if role == "x-full":
            self.x, self.dy = full_operand(g, xs, p), pow2_operand(g, ds, js, zero)
        else:
            self.x, self.dy = pow2_operand(g, xs, js, zero), full_operand(g, ds, p)
        if emb:
            self.x[:, Cin - emb:] = self.x[:, Cin - emb:, :1, :1].clone()
        self.q = quantum(self.x) * quantum(self.dy)

    @functools.cached_property
    def absum(self):
        N, Cin, Cout, H, W = self.shape
        return torch.nn.grad.conv2d_weight(self.x.abs(), (Cout, Cin, 3, 3), self.dy.abs(), padding=1)

    def exact(self):
        return float(self.absum.max()) < 2.0 ** 24 * self.q

    @functools.cached_property
    def dw(self):
        """autograd's weight gradient in float64: the exact real result, NOT rounded anywhere"""
        N, Cin, Cout, H, W = self.shape
        w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
        TF.conv2d(self.x, w, None, padding=1).backward(self.dy)
        return w.grad

    @property
    def full(self):
        return self.x if self.role == "x-full" else self.dy


@functools.lru_cache(maxsize=8)
def wgrad_case(shape, dt, role, emb=0):
    p = FULL_P[dt]
    while True:
        for js, zero in _LADDER:
            c = WgradCase(shape, dt, role, p, js, zero, emb)
            if c.exact():
                assert float(c.absum.max()) < 2.0 ** 24 * c.q                # (from the data)
                return c
        assert dt == F32 and p > 8, f"no exact weight-gradient case for {shape} {DT_NAME[dt]} {role}"
        p -= 1


# ------------------------------------------------------------------------------------------------------------------------------
# the case table (N, Cin, Cout, H, W), shared by the host checks and the GPU tests
# ------------------------------------------------------------------------------------------------------------------------------
# Share of the 16-bit outputs (plain epilogue, x-full / w-full) that the type cannot represent -- the store must ROUND them; the host
# test demands a quarter everywhere:
#                                   bf16          fp16
#   (2, 6, 16, 8, 16)            0.79 / 0.78   0.80 / 0.79
#   (1, 23, 40, 19, 21)          0.88 / 0.88   0.88 / 0.87
#   (2, 72, 130, 9, 33)          0.92 / 0.92   0.92 / 0.92
#   (9, 20, 5, 1, 1)             0.62 / 0.71   0.76 / 0.71
#   (1, 16, 256, 12, 20)         0.86 / 0.86   0.86 / 0.86
#   (6, 40, 384, 20, 17)         0.90 / 0.90   0.90 / 0.90
#   (6, 32, 512, 33, 17)         0.89 / 0.89   0.89 / 0.89
#   (6, 24, 130, 70, 100)        0.88 / 0.88   0.88 / 0.88
#   (1, 128, 1024, 32, 32)       0.94 / 0.94   0.94 / 0.94
#   PAIR_CASES (all three)       0.89 .. 0.95  0.89
#   FIRST_CASES, VIEW_SHAPE, two-source shapes: 0.69 .. 0.93
# (the inference epilogue's ReLU zeroes about half of the outputs: 0.36 .. 0.56 there, every case; the host test demands a quarter of
#  those too and prints both shares of every case)
FWD_CASES = [
    (2, 6, 16, 8, 16),            # one stage, Cin % 16 != 0; small enough for exact channel sums (the slab case)
    (1, 23, 40, 19, 21),          # two stages, Cin % 16 != 0, ragged bottom and right edge, Cout % 64 != 0
    (2, 72, 130, 9, 33),          # five stages (odd), three 64-channel output tiles, ragged
    (9, 20, 5, 1, 1),             # 1-pixel images (only the centre tap meets data: 20 channels keep the sums wide enough to round)
    (1, 16, 256, 12, 20),         # small-image form, 8-row tiles <64,1,4>
    (6, 40, 384, 20, 17),         # small-image form, 16-row tiles <64,2,4>; three stages, Cin % 16 != 0, ragged
    (6, 32, 512, 33, 17),         # 128 output channels per workgroup; ragged
    (6, 24, 130, 70, 100),        # more work items than workgroups, 32-row tiles <64,4,4>, ragged
    (1, 128, 1024, 32, 32),       # two K groups
]
# (tile rows, waves, output channels per workgroup, K groups) that mau_conv3x3_variant must report for the 16-bit types
FWD_VARIANTS = {(1, 16, 256, 12, 20): (8, 4, 64, 1), (6, 40, 384, 20, 17): (16, 4, 64, 1), (6, 32, 512, 33, 17): (16, 8, 128, 1),
                (6, 24, 130, 70, 100): (32, 4, 64, 1), (1, 128, 1024, 32, 32): (8, 4, 64, 2)}
SLAB_EXACT = [(2, 6, 16, 8, 16), (9, 20, 5, 1, 1)]            # sum y per channel is exact here (asserted from the data)
# The big tiles of the training step (four tile-row groups per wave), dense sources on the buffer-addressed loader with an EVEN number
# of 16-channel stages: the 16x16x32 stage-pair loop.  16-bit types only.  shape -> what mau_conv3x3_variant must report
PAIR_CASES = {(11, 32, 192, 126, 17): (32, 4, 64, 1),       # <64,4,4>, one stage pair, ragged bottom (126 = 3 * 32 + 30) and right edge
              (11, 32, 128, 190, 17): (32, 8, 128, 1),      # <128,4,8>
              (11, 224, 192, 126, 17): (64, 8, 64, 1)}      # <64,4,8>: more than 192 input channels, an even number of 32-row tiles
PAIR_TILINGS = {(32, 4, 64), (32, 8, 128), (64, 8, 64)}      # (tile rows, waves, output channels) of the tilings with four row groups


def runs_pair_loop(variant, Cin, ldx, ldx1=None, C0=None):
    """The launch rule of the stage-pair loop, stated independently of the library: a four-row-group tiling, every 16-channel stage
    inside one tensor at a pitch that is a multiple of 16 (the buffer-addressed loader), an even number of stages."""
    if ldx1 is None:
        fast = ldx % 16 == 0 and -(-Cin // 16) * 16 <= ldx
    else:
        fast = C0 % 16 == 0 and C0 <= ldx and -(-(Cin - C0) // 16) * 16 <= ldx1
    return tuple(variant[:3]) in PAIR_TILINGS and fast and -(-Cin // 16) % 2 == 0


def wgrad_runs_16x16x32(H, W):
    """Which 16-bit weight-gradient kernel multiplies a layer (sources within 31-bit byte offsets): the 16x16x32 one on 4 x 32 pixel
    tiles unless they cover over 8 % more area than the 32x32x16 kernel's 8 x 16 tiles."""
    a16 = -(-H // 4) * 4 * -(-W // 32) * 32
    a32 = -(-H // 8) * 8 * -(-W // 16) * 16
    return a16 <= 1.08 * a32


DGRAD_CASES = [(2, 6, 16, 8, 16), (1, 23, 40, 19, 21), (2, 72, 130, 9, 33), (2, 128, 32, 16, 16), (1, 256, 16, 12, 20)]
WGRAD_CASES = [(2, 6, 16, 8, 16), (1, 23, 40, 19, 21), (2, 72, 130, 9, 33), (9, 1, 1, 1, 1), (3, 64, 128, 24, 40), (6, 24, 130, 70, 100),
               (4, 64, 128, 40, 64)]      # 16x16x32 kernel, 128-wide output block, four pixel tiles per split
# (N, C0, C1, Cout, H, W, E): two tensor sources + a broadcast embedding
TWO_SOURCE_CASES = [(2, 16, 24, 40, 19, 21, 8), (1, 64, 128, 64, 16, 16, 16), (2, 16, 24, 72, 19, 21, 0)]
# (N, Cin, Cout, H, W) of the first-layer kernels
FIRST_CASES = [(1, 3, 8, 9, 11),                              # (few pixels: exact channel sums in every type)
               (3, 3, 8, 31, 47), (2, 8, 16, 16, 64), (2, 6, 96, 33, 65), (1, 6, 64, 40, 70)]


VIEW_SHAPE = (2, 32, 64, 19, 21)                              # Cin % 16 == 0 (every view is legal), Cout % 64 == 0 (a slot is legal)
SECOND_VIEW_CASE = (1, 64, 32, 64, 16, 16, 16)                # two sources + embedding, both tensors slots of wider rows


def forward_table():
    """every forward case the GPU tests build: (shape (N,Cin,Cout,H,W), embedding channels, tensor types)"""
    rows = [(s, 0, DTYPES) for s in FWD_CASES] + [(s, 0, (BF16, F16)) for s in list(PAIR_CASES) + FIRST_CASES] + [(VIEW_SHAPE, 0, DTYPES)]
    rows += [((N, C0 + C1 + E, Cout, H, W), E, (BF16, F16)) for N, C0, C1, Cout, H, W, E in TWO_SOURCE_CASES + [SECOND_VIEW_CASE]]
    return rows


def first_p12_case(dt):
    """The first layer on 12-bit inputs: (x, x rounded to ``dt`` nearest-even, w, the exact convolution of the ROUNDED input); the
    bound is asserted on the rounded data."""
    N, Cin, Cout, H, W = 2, 6, 16, 19, 37
    g = torch.Generator().manual_seed(12)
    x = full_operand(g, (N, Cin, H, W), 12)
    w = pow2_operand(g, (Cout, Cin, 3, 3), (-1, 0, 1), 1 / 3)
    xr = x.float().to(dt).double()
    q = quantum(xr) * quantum(w)
    assert float(TF.conv2d(xr.abs(), w.abs(), None, padding=1).max()) < 2.0 ** 24 * q
    return x, xr, w, TF.conv2d(xr, w, None, padding=1)


def stats_of(y64):
    """(sum y, sum y^2, sum |y|) per channel over batch and pixels, float64"""
    return y64.sum(dim=(0, 2, 3)), (y64 ** 2).sum(dim=(0, 2, 3)), y64.abs().sum(dim=(0, 2, 3))


def rounding_share(y64, dt):
    """share of the outputs the 16-bit type cannot represent"""
    return float((~representable(y64, dt)).double().mean())


# ------------------------------------------------------------------------------------------------------------------------------
# host mutants: what a subtly wrong kernel would compute
# ------------------------------------------------------------------------------------------------------------------------------
def mutant_truncated_operands(c):
    """both operands cut to p - 1 significand bits (a lost low mantissa bit in a layout conversion, a pack or an LDS repack)"""
    return TF.conv2d(trunc_sig(c.x, c.p - 1), trunc_sig(c.w, c.p - 1), c.b, padding=1)


def mutant_truncating_store(y64, dt):
    """the 16-bit output cut toward zero instead of rounded to nearest even"""
    return trunc_sig(y64, SIG_BITS[dt]).float().to(dt).float()


def mutant_fp16_accumulation(c):
    """the accumulator rounded to fp16 after every 16-channel stage (accumulation in the operand type)"""
    acc = torch.zeros_like(c.y)
    for c0 in range(0, c.shape[1], 16):
        acc = (acc + TF.conv2d(c.x[:, c0:c0 + 16], c.w[:, c0:c0 + 16], None, padding=1)).half().double()
    return (acc + c.b[None, :, None, None]).float().to(F16).float()
