"""The 3x3 convolution kernels (csrc/conv3x3_bf16.hip and its translation units, conv3x3.hip, conv3x3_wgrad_bf16.hip,
conv3x3_wgrad16.hip, conv3x3_first.hip) through the C ABI against the float64 references of tests/conv_ref.py.

DATA.  Dyadic full-mantissa cases (tests/conv_ref.py; tests/test_conv_pinned_host.py proves them exact in fp32 in any summation order
and sensitive to a dropped operand bit, a truncating store and a 16-bit accumulator): an fp32 result must equal the float64 reference
bit for bit, a 16-bit one that reference rounded once to nearest even, a weight gradient the reference with no rounding at all.

VIEWS.  Every tensor goes through ``Buf``: NaN in the sentinel pixels at both ends and in every lane outside the tensor, 0 in the pad
lanes.  Sources are read dense, at a pixel pitch with ld % 16 == 8 (the general halo loader) and as a channel slot of a wider row
buffer (ld = C + 64, pointer 64 channels in: the buffer-addressed loader inside a wider row); outputs are written dense, into a slot
of a row buffer (Cout % 64 == 0: nothing outside the slot may change), and at Cout % 64 != 0 with ldy > pad8(Cout), where the
kernels zero the rest of the 64-channel block -- the sentence of include/mau_hip.h beside mau_conv3x3_fwd, pinned here.
Slabs, split-K accumulators, workspaces and gradients sit between NaN sentinels too, and the spare part behind what the size query
reports must still be NaN after the call."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from tests import conv_ref as R
from tests._helpers import Buf, _call, _stream, mau, pad8, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

BF16, F16, F32 = R.BF16, R.F16, R.F32
LP = (BF16, F16)
FRONT = 64                                                    # sentinel elements in front of a flat buffer


def _id(v):
    return R.DT_NAME[v] if isinstance(v, torch.dtype) else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def _code(dt):
    from mau_amd import _lib
    return {F32: _lib.MAU_F32, BF16: _lib.MAU_BF16, F16: _lib.MAU_F16}[dt]


def _lib():
    from mau_amd import _lib as L
    return L.lib


def _variant(dt, shape):
    from mau_amd._lib import conv3x3_variant
    N, Cin, Cout, H, W = shape
    return conv3x3_variant(_code(dt), N, H, W, Cout, Cin)


def _f32(t64):
    """a float64 tensor that fp32 holds exactly, on the device"""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64)
    return t32.contiguous().cuda()


class Flat:
    """n elements between NaN sentinels: FRONT in front, ``spare`` behind (the part a size query does not report)"""

    def __init__(self, n, spare=FRONT, dt=torch.float32):
        self.n, self.spare = int(n), int(spare)
        self.dev = torch.full((FRONT + self.n + self.spare,), float("nan"), dtype=dt, device="cuda")

    @property
    def ptr(self):
        return self.dev.data_ptr() + FRONT * self.dev.element_size()

    def back(self, written=True):
        torch.cuda.synchronize()
        r = self.dev.cpu()
        assert bool(torch.isnan(r[:FRONT]).all()), "elements in front of the buffer were written"
        assert bool(torch.isnan(r[FRONT + self.n:]).all()), f"elements behind the {self.n} reported ones were written"
        body = r[FRONT:FRONT + self.n]
        assert not written or not bool(torch.isnan(body).any()), "elements of the buffer were left unwritten"
        return body


def _pack(w64, dt, forward=True):
    """the forward pack of OIHW weights, or their data-gradient pack"""
    Cout, Cin = w64.shape[:2]
    code, wd = _code(dt), _f32(w64)
    n = _lib().mau_conv3x3_packed_elems(code, Cout, Cin) if forward else _lib().mau_conv3x3_packed_elems(code, Cin, Cout)
    pk = torch.zeros(n, dtype=dt, device="cuda")
    _call("mau_conv3x3_pack_weights", wd.data_ptr(), pk.data_ptr() if forward else None, None if forward else pk.data_ptr(), code, Cout, Cin,
          _stream())
    return pk


def _src(x64, dt, view="dense", junk=False):
    """(Buf, pointer, pixel pitch) of an (N,C,H,W) source: dense | ld8 (pitch % 16 == 8) | pad16 (pitch roundup(C, 16)) | slot (pitch
    C + 64, 64 channels in).  junk: the lanes [pad8(C), roundup(C, 16)) hold a finite non-zero value instead of NaN."""
    N, C, H, W = x64.shape
    if view == "dense":
        ld, off = pad8(C), 0
    elif view == "ld8":
        ld, off = (C + 15) // 16 * 16 + 8, 0
        assert C % 16 == 0 or junk                             # (lanes up to the end of the last 16-channel stage are read)
    elif view == "pad16":
        ld, off = (C + 15) // 16 * 16, 0
    else:
        ld, off = C + 64, 64
        assert view == "slot" and C % 16 == 0
    assert bool(R.representable(x64, dt).all())
    b = Buf(N * H * W, ld, dt).put(x64.float(), off)
    if junk:
        b.body[:, off + pad8(C):off + (C + 15) // 16 * 16] = 3.0
    b.cuda()
    return b, b.ptr + off * b.dev.element_size(), ld


def _dst(N, C, H, W, dt, view="dense"):
    """(Buf, pointer, pitch, channel offset) of an output: dense | slot (pitch C + 128, 64 channels in) | wide (pitch 128, C % 64 != 0)"""
    if view == "dense":
        ld, off = pad8(C), 0
    elif view == "slot":
        ld, off = C + 128, 64
        assert C % 64 == 0
    else:
        ld, off = (C + 63) // 64 * 64 + 64, 0
        assert view == "wide" and C % 64 != 0
    b = Buf(N * H * W, ld, dt).cuda()
    return b, b.ptr + off * b.dev.element_size(), ld, off


def _read(b, shape, view, off):
    """(N,C,H,W) float32 of a written output and the check of everything around it"""
    N, C, H, W = shape
    if view != "wide":
        return b.get(shape, choff=off)
    # Cout % 64 != 0 and ldy > pad8(Cout): [0, Cout) the result, [Cout, min(round_up(Cout, 64), ldy)) zero, the rest untouched
    v = b.back().view(N, H, W, b.ld).float()
    zend = min((C + 63) // 64 * 64, b.ld)
    assert bool((v[..., C:zend] == 0).all()), "channels [Cout, round_up(Cout, 64)) are not 0"
    assert bool(torch.isnan(v[..., zend:]).all()), "channels behind round_up(Cout, 64) were written"
    return v[..., :C].permute(0, 3, 1, 2).contiguous()


def _want(y64, dt):
    return y64.float() if dt == F32 else R.round_dt(y64, dt)


def _conv(dt, parts, wpk, Cout, bias=None, sc=None, sh=None, emb=None, slab=False, xview="dense", yview="dense", pool=None, junk=False):
    """One mau_conv3x3_fwd / _fwd2 / _fwd_pool call.  parts: one or two (N,C,H,W) float64 sources; emb (N,E) float64 or None.
    Returns (y, slab rows or None, pooled or None, emb_ws or None)."""
    code, st = _code(dt), _stream()
    N, _, H, W = parts[0].shape
    srcs = [_src(p, dt, xview if i == 0 or xview != "ld8" else "dense", junk) for i, p in enumerate(parts)]
    yb, yp, ldy, yoff = _dst(N, Cout, H, W, dt, yview)
    keep = [_f32(v) if v is not None else None for v in (bias, sc, sh, emb)]
    bp, scp, shp, ep = (k.data_ptr() if k is not None else None for k in keep)
    E = 0 if emb is None else emb.shape[1]
    ews = Buf(N, E, dt).cuda() if E and dt != F32 else None
    sl = None
    if slab:
        rows, cpad = _lib().mau_conv3x3_num_pixel_tiles(code, N, H, W, Cout), (Cout + 63) // 64 * 64
        sl = Buf(rows, 2 * cpad, torch.float32).cuda()
    pb = None
    if pool is not None:
        pb, pp, ldp, poff = _dst(N, Cout, H // 2, W // 2, dt, pool)
        assert len(parts) == 1 and not E
        _call("mau_conv3x3_fwd_pool", srcs[0][1], srcs[0][2], parts[0].shape[1], wpk.data_ptr(), bp, scp, shp, yp, ldy, Cout, pp, ldp, code,
              N, H, W, st)
    elif len(parts) == 2:
        _call("mau_conv3x3_fwd2", srcs[0][1], srcs[0][2], parts[0].shape[1], srcs[1][1], srcs[1][2], parts[1].shape[1], ep,
              ews.ptr if ews else None, E, wpk.data_ptr(), bp, scp, shp, yp, ldy, Cout, sl.ptr if sl else None, code, N, H, W, st)
    else:
        _call("mau_conv3x3_fwd", srcs[0][1], srcs[0][2], parts[0].shape[1], ep, ews.ptr if ews else None, E, wpk.data_ptr(), bp, scp, shp,
              yp, ldy, Cout, sl.ptr if sl else None, code, N, H, W, st)
    y = _read(yb, (N, Cout, H, W), yview, yoff)
    for s_ in srcs:                                           # (a source is never written)
        assert same_bits(s_[0].dev.cpu(), s_[0].host, nan_matches_nan=True)
    pooled = _read(pb, (N, Cout, H // 2, W // 2), pool, poff) if pb is not None else None
    return y, (sl.back() if sl else None), pooled, (ews.back() if ews else None)


_capsys = [None]


@pytest.fixture(autouse=True)
def _uncaptured(capsys):
    _capsys[0] = capsys
    yield


def _report(line):
    """a measured figure, shown whether or not pytest captures the test's output"""
    with _capsys[0].disabled():
        print("\n" + line, end="")


def _check_slab(rows, c, dt, y64):
    """the statistics slab of mau_conv3x3_fwd against the exact result y64 (NOT the rounded output)"""
    N, Cin, Cout, H, W = c.shape
    cpad = (Cout + 63) // 64 * 64
    assert not bool(torch.isnan(rows).any()), "queried slab rows were left unwritten"
    s = rows.double().sum(0)
    assert bool((s[Cout:cpad] == 0).all()) and bool((s[cpad + Cout:] == 0).all())
    s1, s2, sa = R.stats_of(y64)
    th = _variant(dt, c.shape)[0]
    g = R.gamma(th * 16 + 1)
    if float(sa.max()) < 2.0 ** 24 * c.q:                     # every partial sum of y any kernel can form is exact
        assert torch.equal(s[:Cout], s1), "sum y"
    else:                                                     # the same recursive-summation bound, on sum |y|
        assert bool(((s[:Cout] - s1).abs() <= g * sa).all()), "sum y"
    assert c.shape not in R.SLAB_EXACT or float(sa.max()) < 2.0 ** 24 * c.q
    if dt != F32 and c.shape in R.SLAB_EXACT:                 # the case can tell the accumulators from the stored values
        assert not torch.equal(R.round_dt(y64, dt).double().sum(dim=(0, 2, 3)), s1)
    # sum y^2: each slab row may be off by gamma_n times its own sum of squares; the rows' sums of squares add up to s2
    err = (s[cpad:cpad + Cout] - s2).abs()
    rel = float((err / s2.clamp_min(1e-300)).max())
    _report(f"sum y^2 {c.shape} {R.DT_NAME[dt]} {c.role}: relative error {rel:.3e}, bound gamma_{th * 16 + 1} = {g:.3e}")
    assert bool((err <= g * s2).all()), (rel, g)


# ---- 1. mau_conv3x3_fwd: plain, statistics and inference epilogues ----------------------------------------------------------------
def test_case_table_reaches_every_form(mau):
    """the variants the table is built to reach, asserted through mau_conv3x3_variant for both 16-bit types"""
    seen = set()
    for shape, want in R.FWD_VARIANTS.items():
        for dt in LP:
            assert _variant(dt, shape) == want, (shape, _variant(dt, shape))
        seen.add(want)
    assert {(8, 4, 64), (16, 4, 64)} <= {v[:3] for v in seen}                   # both small-image forms <64,1,4>, <64,2,4>
    assert any(v[0] == 32 for v in seen) and any(v[2] == 128 for v in seen) and any(v[3] == 2 for v in seen)
    stages = {-(-s[1] // 16) % 2 for s in R.FWD_CASES}
    assert stages == {0, 1} and any(s[1] % 16 for s in R.FWD_CASES)             # even and odd stage counts, Cin % 16 != 0
    assert any(s[3] == 1 and s[4] == 1 for s in R.FWD_CASES) and any(s[3] % 32 and s[4] % 16 for s in R.FWD_CASES)
    from mau_amd._lib import lib
    N, Cin, Cout, H, W = (6, 24, 130, 70, 100)                                  # more work items than workgroups (256 CUs)
    assert (6, 24, 130, 70, 100) in R.FWD_CASES and N * -(-H // 32) * -(-W // 16) * -(-Cout // 64) > 256
    assert lib.mau_conv3x3_num_pixel_tiles(_code(BF16), N, H, W, Cout) == 4 * N * -(-H // 32) * -(-W // 16)


@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
@pytest.mark.parametrize("shape", R.FWD_CASES, ids=_id)
def test_conv3x3_fwd_dyadic(mau, shape, dt, role):
    """plain (+ bias), statistics and inference epilogue on one case: output bits, pad lanes, slab, sentinels"""
    c = R.conv_case(shape, dt, role)
    R.assert_exact(c)
    if dt != F32 and shape in R.FWD_VARIANTS:
        assert _variant(dt, shape) == R.FWD_VARIANTS[shape]
    Cout = shape[2]
    wpk = _pack(c.w, dt)
    y, _, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b)
    assert same_bits(y, _want(c.y, dt)), "plain epilogue"
    y, rows, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, slab=True)
    assert same_bits(y, _want(c.y, dt)), "statistics epilogue"
    _check_slab(rows, c, dt, c.y)
    y, _, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh)
    assert same_bits(y, _want(c.post, dt), nan_matches_nan=False), "inference epilogue"
    y, _, _, _ = _conv(dt, [c.x], wpk, Cout)                                     # no bias at all (the BIAS = false bodies)
    assert same_bits(y, _want(c.y_nobias, dt)), "no bias"


@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", LP, ids=_id)
@pytest.mark.parametrize("shape", list(R.PAIR_CASES), ids=_id)
def test_conv3x3_stage_pair_loop_dyadic(mau, shape, dt, role):
    """The 16x16x32 stage-pair loop of the big tiles <64,4,4>, <128,4,8>, <64,4,8> -- what the training step's wide layers run -- with
    one source (its ONE form) and with the channels split over two tensors: plain, statistics and inference epilogue, and the pooled
    output taken from the registers of that loop's epilogue.  mau_conv3x3_variant reports the tiling; the loop form follows from the
    launch rule ``conv_ref.runs_pair_loop`` restates: four row groups, buffer-addressed loader, an even stage count."""
    N, Cin, Cout, H, W = shape
    v = _variant(dt, shape)
    assert v == R.PAIR_CASES[shape] and R.runs_pair_loop(v, Cin, pad8(Cin)), v
    c = R.conv_case(shape, dt, role)
    R.assert_exact(c)
    wpk = _pack(c.w, dt)
    assert same_bits(_conv(dt, [c.x], wpk, Cout, bias=c.b)[0], _want(c.y, dt)), "plain epilogue"
    y, rows, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, slab=True)
    assert same_bits(y, _want(c.y, dt)), "statistics epilogue"
    _check_slab(rows, c, dt, c.y)
    y, _, pooled, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh, pool="dense")
    assert same_bits(y, _want(c.post, dt)) and same_bits(pooled, _pooled(_want(c.post, dt))), "inference epilogue + pool"
    assert same_bits(_conv(dt, [c.x], wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh)[0], _want(c.post, dt)), "inference epilogue"
    C0 = Cin // 32 * 16                                        # two tensor sources, each whole 16-channel stages: the two-source form
    assert R.runs_pair_loop(v, Cin, C0, ldx1=Cin - C0, C0=C0)
    parts = [c.x[:, :C0].contiguous(), c.x[:, C0:].contiguous()]
    y, rows, _, _ = _conv(dt, parts, wpk, Cout, bias=c.b, slab=True)
    assert same_bits(y, _want(c.y, dt)), "two sources, statistics epilogue"
    _check_slab(rows, c, dt, c.y)
    assert same_bits(_conv(dt, parts, wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh)[0], _want(c.post, dt)), "two sources, inference epilogue"


# ---- 2. the data gradient: mau_conv3x3_fwd on dy with the wd pack -----------------------------------------------------------------
@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
@pytest.mark.parametrize("shape", R.DGRAD_CASES, ids=_id)
def test_conv3x3_dgrad_dyadic(mau, shape, dt, role):
    c, w = R.dgrad_case(shape, dt, role)
    R.assert_exact(c)
    N, Cin, Cout, H, W = shape
    wd = _pack(w, dt, forward=False)
    dx, _, _, _ = _conv(dt, [c.x], wd, Cin)
    assert same_bits(dx, _want(c.y_nobias, dt))


# ---- 3. two tensor sources + a broadcast embedding --------------------------------------------------------------------------------
@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", LP, ids=_id)
@pytest.mark.parametrize("shape", R.TWO_SOURCE_CASES, ids=_id)
def test_conv3x3_two_sources_and_embedding_dyadic(mau, shape, dt, role):
    """mau_conv3x3_fwd2 and mau_conv3x3_wgrad2 over [x | x1 | broadcast(emb)]: in the x-full role the fp32 embedding carries a full
    significand of the activation type, so emb_ws (the embedding in that type) is pinned bit for bit too"""
    N, C0, C1, Cout, H, W, E = shape
    Cin = C0 + C1 + E
    c = R.conv_case((N, Cin, Cout, H, W), dt, role, E)
    R.assert_exact(c)
    parts = [c.x[:, :C0].contiguous(), c.x[:, C0:C0 + C1].contiguous()]
    emb = c.x[:, C0 + C1:, 0, 0].contiguous() if E else None
    if E and role == "x-full":
        assert R.full_share(emb, c.p) >= 0.5
    wpk = _pack(c.w, dt)
    for kw in (dict(), dict(slab=True), dict(sc=c.sc, sh=c.sh)):
        y, rows, _, ews = _conv(dt, parts, wpk, Cout, bias=c.b, emb=emb, **kw)
        assert same_bits(y, _want(c.post if "sc" in kw else c.y, dt)), kw.keys()
        if E:
            assert same_bits(ews.float(), emb.float())
        if rows is not None:
            _check_slab(rows, c, dt, c.y)
    g = R.wgrad_case((N, Cin, Cout, H, W), dt, role, E)
    gparts = [g.x[:, :C0].contiguous(), g.x[:, C0:C0 + C1].contiguous()]
    gemb = g.x[:, C0 + C1:, 0, 0].contiguous() if E else None
    assert same_bits(_wgrad(dt, gparts, g.dy, gemb), g.dw.float())


# ---- 4. the weight gradient -------------------------------------------------------------------------------------------------------
def _wgrad(dt, parts, dy64, emb=None, xview="dense", dyview="dense"):
    """mau_conv3x3_wgrad(2) + mau_conv3x3_unpack_wgrad; acc NaN-filled and half again longer than the size query reports"""
    code, st, lib = _code(dt), _stream(), _lib()
    N, Cout, H, W = dy64.shape
    E = 0 if emb is None else emb.shape[1]
    Cin = sum(p.shape[1] for p in parts) + E
    srcs = [_src(p, dt, xview if i == 0 or xview != "ld8" else "dense") for i, p in enumerate(parts)]
    dyb, dyp, lddy = _src(dy64, dt, dyview)
    embd = _f32(emb) if E else None
    ews = Buf(N, E, dt).cuda() if E and dt != F32 else None
    elems, ns = lib.mau_conv3x3_wgrad_acc_elems(code, N, H, W, Cout, Cin), lib.mau_conv3x3_wgrad_splits(code, N, H, W, Cout, Cin)
    assert elems == ns * 9 * ((Cout + 63) // 64 * 64) * ((Cin + 63) // 64 * 64)
    acc = Flat(elems, spare=elems // 2 + FRONT)
    if len(parts) == 2:
        _call("mau_conv3x3_wgrad2", srcs[0][1], srcs[0][2], parts[0].shape[1], srcs[1][1], srcs[1][2], parts[1].shape[1],
              embd.data_ptr() if E else None, ews.ptr if ews else None, E, dyp, lddy, Cout, acc.ptr, code, N, H, W, st)
    else:
        _call("mau_conv3x3_wgrad", srcs[0][1], srcs[0][2], parts[0].shape[1], embd.data_ptr() if E else None, ews.ptr if ews else None, E,
              dyp, lddy, Cout, acc.ptr, code, N, H, W, st)
    dw = Flat(Cout * Cin * 9)
    _call("mau_conv3x3_unpack_wgrad", acc.ptr, ns, dw.ptr, Cout, Cin, st)
    acc.back(written=False)                                   # (pad rows of a slab may hold anything; the spare part must be NaN)
    if ews is not None:
        assert same_bits(ews.back().float(), emb.float())
    return dw.back().view(Cout, Cin, 3, 3)


@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
@pytest.mark.parametrize("shape", R.WGRAD_CASES, ids=_id)
def test_conv3x3_wgrad_dyadic(mau, shape, dt, role):
    """dw EQUAL to the float64 weight gradient: no rounding anywhere, the split-K sum of the unpack included"""
    g = R.wgrad_case(shape, dt, role)
    assert float(g.absum.max()) < 2.0 ** 24 * g.q
    if shape == (4, 64, 128, 40, 64) and dt != F32:           # the 16x16x32 kernel on a 128-wide output block, four pixel tiles per split
        N, Cin, Cout, H, W = shape
        ns = _lib().mau_conv3x3_wgrad_splits(_code(dt), N, H, W, Cout, Cin)
        assert R.wgrad_runs_16x16x32(H, W) and Cout % 128 == 0 and N * -(-H // 4) * -(-W // 32) >= 4 * ns > 4
    dw = _wgrad(dt, [g.x], g.dy)
    assert torch.equal(dw.double(), g.dw) and same_bits(dw, g.dw.float())


# ---- 5. mau_conv3x3_fwd_pool ------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 23, 40, 19, 21), (1, 16, 256, 12, 20), (6, 40, 384, 20, 17), (6, 24, 130, 70, 100)]


def _pooled(y32):
    return TF.max_pool2d(y32, 2)


@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
@pytest.mark.parametrize("shape", POOL_CASES, ids=_id)
def test_conv3x3_fwd_pool_dyadic(mau, shape, dt):
    """y and pooled against the REFERENCE (floor-mode windows of the rounded activation), not against the two-call route"""
    assert shape in R.FWD_CASES
    c = R.conv_case(shape, dt, "x-full")
    want = _want(c.post, dt)
    y, _, pooled, _ = _conv(dt, [c.x], _pack(c.w, dt), shape[2], bias=c.b, sc=c.sc, sh=c.sh, pool="dense")
    assert same_bits(y, want) and same_bits(pooled, _pooled(want))
    assert float(pooled.max()) > 0 and bool((pooled == 0).any())


# ---- 6. the first layer -----------------------------------------------------------------------------------------------------------
def _first_fwd(dt, x64, w64, b64, Cout, sc=None, sh=None, slab=False, x8=False):
    code, st, lib = _code(dt), _stream(), _lib()
    N, Cin, H, W = x64.shape
    xd, wd, bd = _f32(x64), _f32(w64), _f32(b64)
    scd, shd = (_f32(sc), _f32(sh)) if sc is not None else (None, None)
    yb, yp, ldy, _ = _dst(N, Cout, H, W, dt)
    cpad = (Cout + 63) // 64 * 64
    sl = Buf(lib.mau_conv3x3_first_rows(N, H, W), 2 * cpad, torch.float32).cuda() if slab else None
    x8b = Buf(N * H * W, 8, dt).cuda() if x8 else None
    _call("mau_conv3x3_first_fwd", xd.data_ptr(), Cin, wd.data_ptr(), bd.data_ptr(), scd.data_ptr() if sc is not None else None,
          shd.data_ptr() if sc is not None else None, yp, ldy, Cout, sl.ptr if sl else None, x8b.ptr if x8b else None, code, N, H, W, st)
    y = yb.get((N, Cout, H, W))
    return y, (sl.back() if sl else None), (x8b.back().view(N, H, W, 8).float() if x8b else None)


@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", LP, ids=_id)
@pytest.mark.parametrize("shape", R.FIRST_CASES, ids=_id)
def test_first_layer_fwd_dyadic(mau, shape, dt, role):
    """mau_conv3x3_first_fwd from the fp32 NCHW input: its in-kernel conversion is exact on a p-bit input, so y, the statistics and the
    NHWC-8 by-product are pinned bit for bit; then the inference epilogue"""
    N, Cin, Cout, H, W = shape
    c = R.conv_case(shape, dt, role)
    R.assert_exact(c)
    y, rows, x8 = _first_fwd(dt, c.x, c.w, c.b, Cout, slab=True, x8=True)
    assert same_bits(y, _want(c.y, dt))
    assert same_bits(x8[..., :Cin], c.x.float().permute(0, 2, 3, 1).contiguous()) and bool((x8[..., Cin:] == 0).all())
    cpad = (Cout + 63) // 64 * 64
    assert not bool(torch.isnan(rows).any())
    # one slab row per persistent workgroup: how many pixels a row sums is the kernel's business, N * H * W at the most -- the
    # recursive-summation bound for THAT many terms holds whatever the split (tests/test_conv_pinned_host.py: the smallest case takes
    # the exact branch in both types and both roles)
    s, (s1, s2, sa), g = rows.double().sum(0), R.stats_of(c.y), R.gamma(N * H * W + 1)
    if float(sa.max()) < 2.0 ** 24 * c.q:
        assert torch.equal(s[:Cout], s1), "sum y"
    else:
        assert bool(((s[:Cout] - s1).abs() <= g * sa).all()), "sum y"
    assert shape != R.FIRST_CASES[0] or float(sa.max()) < 2.0 ** 24 * c.q
    err = (s[cpad:cpad + Cout] - s2).abs()
    _report(f"first layer sum y^2 {shape} {R.DT_NAME[dt]} {role}: relative error {float((err / s2).max()):.3e}, bound gamma_{N * H * W + 1} = {g:.3e}")
    assert bool((err <= g * s2).all())
    assert bool((s[Cout:cpad] == 0).all()) and bool((s[cpad + Cout:] == 0).all())
    y, _, _ = _first_fwd(dt, c.x, c.w, c.b, Cout, sc=c.sc, sh=c.sh)
    assert same_bits(y, _want(c.post, dt))


@pytest.mark.parametrize("dt", LP, ids=_id)
def test_first_layer_input_conversion_is_nearest_even(mau, dt):
    """12-bit inputs: the by-product x8 must be x rounded to the activation type, nearest even, and y the convolution of THAT"""
    x, xr, w, y64 = R.first_p12_case(dt)
    Cout, Cin = w.shape[:2]
    assert float((xr != x).double().mean()) > 0.5 and not torch.equal(R.trunc_sig(x, R.SIG_BITS[dt]), xr)
    y, _, x8 = _first_fwd(dt, x, w, torch.zeros(Cout, dtype=torch.float64), Cout, x8=True)
    assert same_bits(x8[..., :Cin], xr.float().permute(0, 2, 3, 1).contiguous()) and bool((x8[..., Cin:] == 0).all())
    assert same_bits(y, _want(y64, dt))


@pytest.mark.parametrize("role", R.ROLES)
@pytest.mark.parametrize("dt", LP, ids=_id)
@pytest.mark.parametrize("shape", R.FIRST_CASES, ids=_id)
def test_first_layer_wgrad_dyadic(mau, shape, dt, role):
    """mau_conv3x3_first_wgrad: dw equal to the float64 gradient, the workspace not overrun beyond its size query"""
    code, st, lib = _code(dt), _stream(), _lib()
    N, Cin, Cout, H, W = shape
    g = R.wgrad_case(shape, dt, role)
    x8 = Buf(N * H * W, 8, dt).put(g.x.float())
    dzb, dzp, lddz = _src(g.dy, dt)
    n = lib.mau_conv3x3_first_wgrad_ws_elems(N, H, W, Cout)
    ws, dw = Flat(n, spare=n // 2 + FRONT), Flat(Cout * Cin * 9)
    _call("mau_conv3x3_first_wgrad", x8.ptr, dzp, lddz, dw.ptr, ws.ptr, Cin, Cout, code, N, H, W, st)
    ws.back(written=False)
    got = dw.back().view(Cout, Cin, 3, 3)
    assert torch.equal(got.double(), g.dw) and same_bits(got, g.dw.float())


# ---- strided views ----------------------------------------------------------------------------------------------------------------
VIEW_SHAPE = R.VIEW_SHAPE


@functools.lru_cache(maxsize=None)
def _dense_results(dt):
    c = R.conv_case(VIEW_SHAPE, dt, "x-full")
    wpk = _pack(c.w, dt)
    return c, {"plain": _conv(dt, [c.x], wpk, VIEW_SHAPE[2], bias=c.b)[0], "post": _conv(dt, [c.x], wpk, VIEW_SHAPE[2], bias=c.b, sc=c.sc, sh=c.sh)[0]}


@pytest.mark.parametrize("xview", ["ld8", "slot"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_source_views_bitwise(mau, dt, xview):
    """x at a pitch with ld % 16 == 8 (general loader) and as a slot of a wider row (buffer-addressed loader): the dense call's bits and
    the reference's, under the three epilogues"""
    c, dense = _dense_results(dt)
    Cout = VIEW_SHAPE[2]
    wpk = _pack(c.w, dt)
    assert same_bits(dense["plain"], _want(c.y, dt)) and same_bits(dense["post"], _want(c.post, dt))
    y, rows, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, slab=True, xview=xview)
    assert same_bits(y, dense["plain"])
    _check_slab(rows, c, dt, c.y)
    assert same_bits(_conv(dt, [c.x], wpk, Cout, bias=c.b, xview=xview)[0], dense["plain"])
    assert same_bits(_conv(dt, [c.x], wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh, xview=xview)[0], dense["post"])


@pytest.mark.parametrize("dt", LP, ids=_id)
def test_second_source_view_bitwise(mau, dt):
    """x and x1 of the two-source call both slots of wider rows"""
    N, C0, C1, Cout, H, W, E = R.SECOND_VIEW_CASE
    c = R.conv_case((N, C0 + C1 + E, Cout, H, W), dt, "x-full", E)
    parts = [c.x[:, :C0].contiguous(), c.x[:, C0:C0 + C1].contiguous()]
    emb = c.x[:, C0 + C1:, 0, 0].contiguous()
    wpk = _pack(c.w, dt)
    for xview in ("dense", "slot"):
        assert same_bits(_conv(dt, parts, wpk, Cout, bias=c.b, emb=emb, xview=xview)[0], _want(c.y, dt)), xview
    g = R.wgrad_case((N, C0 + C1 + E, Cout, H, W), dt, "x-full", E)
    gparts = [g.x[:, :C0].contiguous(), g.x[:, C0:C0 + C1].contiguous()]
    assert same_bits(_wgrad(dt, gparts, g.dy, g.x[:, C0 + C1:, 0, 0].contiguous(), xview="slot", dyview="slot"), g.dw.float())


@pytest.mark.parametrize("xview,dyview", [("ld8", "ld8"), ("slot", "slot"), ("dense", "slot")])
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_wgrad_views_bitwise(mau, dt, xview, dyview):
    """x through ldx and dy through lddy, at a pitch with ld % 16 == 8 and as slots of wider rows whose other channels are NaN"""
    g = R.wgrad_case(VIEW_SHAPE, dt, "w-full")
    assert same_bits(_wgrad(dt, [g.x], g.dy, xview=xview, dyview=dyview), g.dw.float())


@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_output_slot_of_a_row_buffer(mau, dt):
    """Cout % 64 == 0, ldy = Cout + 128, pointer 64 channels in: y, pooled and the data gradient's dx land in their slot; every other
    channel of the row buffer and every pixel outside the tensor are still NaN (``Buf.get`` asserts both)"""
    c, dense = _dense_results(dt)
    N, Cin, Cout, H, W = VIEW_SHAPE
    wpk = _pack(c.w, dt)
    y, rows, _, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, slab=True, yview="slot")
    assert same_bits(y, dense["plain"])
    _check_slab(rows, c, dt, c.y)
    assert same_bits(_conv(dt, [c.x], wpk, Cout, bias=c.b, yview="slot")[0], dense["plain"])
    y, _, pooled, _ = _conv(dt, [c.x], wpk, Cout, bias=c.b, sc=c.sc, sh=c.sh, yview="slot", pool="slot")
    assert same_bits(y, dense["post"]) and same_bits(pooled, _pooled(dense["post"]))
    d, w = R.dgrad_case((N, 64, Cout, H, W), dt, "w-full")     # dx of a 64 -> 64 layer into a slot, dy read from a slot
    dx, _, _, _ = _conv(dt, [d.x], _pack(w, dt, forward=False), 64, xview="slot", yview="slot")
    assert same_bits(dx, _want(d.y_nobias, dt))


@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_output_wider_than_its_channels(mau, dt):
    """Cout = 40 at ldy = 128 -- what include/mau_hip.h says beside mau_conv3x3_fwd: channels [0, Cout) hold the result, channels
    [Cout, min(round_up(Cout, 64), ldy)) are written as ZERO under every epilogue, everything behind is untouched.  All three types
    do the same (the fp32 kernel stores one element at a time while co < ldy, the 16-bit ones 8-channel vectors while cv < ldy).
    functional.py therefore hands a row-buffer slot to a convolution only when Cout % 64 == 0."""
    shape = (1, 23, 40, 19, 21)
    assert shape in R.FWD_CASES
    c = R.conv_case(shape, dt, "x-full")
    wpk = _pack(c.w, dt)
    y, rows, _, _ = _conv(dt, [c.x], wpk, 40, bias=c.b, slab=True, yview="wide")
    assert same_bits(y, _want(c.y, dt))
    _check_slab(rows, c, dt, c.y)
    assert same_bits(_conv(dt, [c.x], wpk, 40, bias=c.b, yview="wide")[0], _want(c.y, dt))
    y, _, pooled, _ = _conv(dt, [c.x], wpk, 40, bias=c.b, sc=c.sc, sh=c.sh, yview="wide", pool="dense")
    assert same_bits(y, _want(c.post, dt)) and same_bits(pooled, _pooled(_want(c.post, dt)))
    if dt != F32:                                              # mau_conv3x3_fwd2: two sources + embedding, the same three epilogues
        N, C0, C1, Cout, H, W, E = R.TWO_SOURCE_CASES[0]
        assert Cout == 40
        c = R.conv_case((N, C0 + C1 + E, Cout, H, W), dt, "x-full", E)
        parts, emb = [c.x[:, :C0].contiguous(), c.x[:, C0:C0 + C1].contiguous()], c.x[:, C0 + C1:, 0, 0].contiguous()
        wpk = _pack(c.w, dt)
        for kw in (dict(), dict(slab=True), dict(sc=c.sc, sh=c.sh)):
            y = _conv(dt, parts, wpk, Cout, bias=c.b, emb=emb, yview="wide", **kw)[0]
            assert same_bits(y, _want(c.post if "sc" in kw else c.y, dt)), kw.keys()


@pytest.mark.parametrize("xview", ["pad16", "ld8"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_source_lanes_up_to_the_stage_end_are_read_against_zero_weights(mau, dt, xview):
    """C0 = 23 at ldx = 32 (buffer-addressed loader) and ldx = 40 (general loader): the lanes [24, 32) of x -- behind the pad lane, inside
    the last 16-channel stage -- hold a finite non-zero value.  include/mau_hip.h says they are read and meet zero weights: the result
    is the reference's.  (That a NaN there reaches y follows from the same sentence and is not run here.)"""
    shape = (1, 23, 40, 19, 21)
    c = R.conv_case(shape, dt, "x-full")
    y, rows, _, _ = _conv(dt, [c.x], _pack(c.w, dt), 40, bias=c.b, slab=True, xview=xview, junk=True)
    assert same_bits(y, _want(c.y, dt))
    _check_slab(rows, c, dt, c.y)
