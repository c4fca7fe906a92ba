"""The training criteria (csrc/head.hip: mau_mse_fwd_bwd, mau_l1_gradient_loss), the embedding fold (csrc/embfold.hip), the gradient
sum (mau_sum_tensors) and the layout boundary (mau_nchw_to_nhwc, mau_nhwc_to_nchw; csrc/spatial.hip) through the C ABI, each
against the plain reference of tests/criteria_ref.py.

The exact cases (multiples of 1/8 with planted ties, small integers: tests/test_criteria_host.py proves every term and every sum
exact in any order) must equal the reference BIT FOR BIT; one real-valued case per family is held to a bound derived from its
operation count.  Every buffer a kernel writes is NaN-prefilled and carries slack in front and behind that must still be NaN
afterwards: ``Buf`` for NHWC tensors, ``Flat`` for flat fp32 / fp64 buffers."""
import ctypes

import numpy as np
import pytest
import torch

from tests import criteria_ref as R
from tests._helpers import NAN, SLACK, Buf, _call, _stream, mau, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
pad8 = R.pad8
FS = 8                                                        # elements of slack at both ends of a flat buffer (keeps 16-byte alignment)


def _code(dt):
    from mau_amd import _lib
    return {torch.float32: _lib.MAU_F32, torch.bfloat16: _lib.MAU_BF16, torch.float16: _lib.MAU_F16}[dt]


def _lib():
    from mau_amd._lib import lib
    return lib


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


class Flat:
    """n elements of fp32 / fp64 on the device between two NaN slacks of FS elements; NaN everywhere unless ``vals`` is given"""

    def __init__(self, n, dt=torch.float32, vals=None):
        self.n = n
        host = torch.full((n + 2 * FS,), NAN, dtype=dt)
        if vals is not None:
            host[FS:FS + n] = torch.as_tensor(np.ascontiguousarray(vals)).reshape(-1).to(dt)
        self.host, self.dev = host, host.cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + FS * self.dev.element_size()

    def back(self):
        """the n elements after the call; the slack must be untouched"""
        torch.cuda.synchronize()
        r = self.dev.cpu()
        assert bool(torch.isnan(r[:FS]).all()) and bool(torch.isnan(r[FS + self.n:]).all()), "elements outside the buffer were written"
        return r[FS:FS + self.n]

    def unchanged(self):
        torch.cuda.synchronize()
        return same_bits(self.dev.cpu(), self.host)


# ---- mau_mse_fwd_bwd ------------------------------------------------------------------------------------------------------------------
def _mse(o, t):
    """-> (loss bits with dout, loss bits with dout = NULL, dout)"""
    n, lib = o.size, _lib()
    ob, tb = Flat(n, vals=o), Flat(n, vals=t)
    nb = lib.mau_mse_blocks(n)
    res = []
    for with_dout in (True, False):
        part, loss, dout = Flat(nb, torch.float64), Flat(1), Flat(n)
        _call("mau_mse_fwd_bwd", ob.ptr, tb.ptr, part.ptr, loss.ptr, dout.ptr if with_dout else None, n, _stream())
        assert not bool(torch.isnan(part.back()).any()), "a block wrote no partial"
        res.append(loss.back().clone())
        if with_dout:
            d = dout.back().clone()
        else:
            assert dout.unchanged(), "dout = NULL: a buffer was written"
        assert ob.unchanged() and tb.unchanged(), "an operand was written"
    return res[0], res[1], d


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027, "grid"])
def test_mse_exact(mau, n):
    """loss and dout bit for bit against ``mse_ref``: the scalar tail alone (1, 3), one vector (4), vector plus tail (5, 1027), a thread
    boundary (1023, 1024), and the grid-stride loop: n = 4 * 256 * 8 * CUs + 1027 elements, where the grid is at its cap of 8 blocks
    per compute unit and the first blocks walk a second stride that ends in a scalar tail.  dout = NULL: the same loss bits, nothing
    written."""
    if n == "grid":
        blocks = 8 * _cus()
        n = 4 * 256 * blocks + 1027
        assert n % 4 != 0 and _lib().mau_mse_blocks(n) == blocks and _lib().mau_mse_blocks(n - 1027) == blocks
    o, t = R.exact_flat_case(n)
    want_loss, want_dout, _ = R.mse_ref(o, t)
    loss, loss_null, dout = _mse(o, t)
    assert same_bits(loss, torch.tensor([want_loss])), n
    assert same_bits(loss_null, loss), (n, "dout = NULL")
    assert same_bits(dout, torch.from_numpy(want_dout)), n


# ---- mau_l1_gradient_loss -------------------------------------------------------------------------------------------------------------
def _l1(o, t, w_l1, w_grad):
    """-> (terms with dout, terms with dout = NULL, dout (B, C, H, W))"""
    B, C, H, W = o.shape
    n, lib = o.size, _lib()
    ob, tb = Flat(n, vals=o), Flat(n, vals=t)
    nb = lib.mau_l1_gradient_blocks(n)
    res = []
    for with_dout in (True, False):
        part, terms, dout = Flat(3 * nb, torch.float64), Flat(3), Flat(n)
        _call("mau_l1_gradient_loss", ob.ptr, tb.ptr, part.ptr, terms.ptr, dout.ptr if with_dout else None, w_l1, w_grad, B, C, H, W, _stream())
        assert not bool(torch.isnan(part.back()).any()), "a block wrote no partial"
        res.append(terms.back().clone())
        if with_dout:
            d = dout.back().clone().view(B, C, H, W)
        else:
            assert dout.unchanged(), "dout = NULL: a buffer was written"
        assert ob.unchanged() and tb.unchanged(), "an operand was written"
    return res[0], res[1], d


L1_SHAPES = [(1, 1, 1, 1), (2, 2, 1, 9), (2, 2, 9, 1), (3, 2, 2, 2), (2, 2, 17, 13), (1, 3, 16, 16), "grid"]


@pytest.mark.parametrize("shape", L1_SHAPES, ids=str)
def test_l1_gradient_exact(mau, shape):
    """terms bit for bit, dout equal as values (``==``: the sign of a zero is not part of the contract) against ``l1_gradient_ref``, at
    the weights (1, 0), (0, 1), (0.7, 2.5), (0, 0); dout = NULL gives the same term bits.  H == 1 / W == 1: no vertical / horizontal
    pair, the count is 0 and the coefficient takes its guarded branch.  "grid": (1, 3, H, 257) with just above 256 * 8 * CUs elements:
    the grid is at its cap and the stride loop runs twice in the first blocks.

    The generator (``exact_criteria_case``) plants out == tgt, dy o == 0 and |dy o| == |dy t| (and the same along x), on the first and
    last row and column too, and makes the last row of every plane and the first row of the next, and the two ends of every row,
    differ strongly: a dy taken across a plane boundary or a dx across a row end would change the sums, which are compared exactly."""
    seeds = (0, 1)
    if shape == "grid":
        blocks = 8 * _cus()
        H = -(-(256 * blocks + 1) // (3 * 257))
        shape, seeds = (1, 3, H, 257), (0,)
        n = 3 * H * 257
        assert n > 256 * blocks and _lib().mau_l1_gradient_blocks(n) == blocks
    for seed in seeds:
        o, t = R.exact_criteria_case(shape, seed)
        assert R.is_eighths(o) and R.is_eighths(t)
        for w_l1, w_grad in R.LOSS_WEIGHTS:
            want_terms, want_dout, _ = R.l1_gradient_ref(o, t, w_l1, w_grad)
            terms, terms_null, dout = _l1(o, t, w_l1, w_grad)
            what = (shape, seed, w_l1, w_grad)
            assert same_bits(terms, torch.from_numpy(want_terms)), what
            assert same_bits(terms_null, terms), what + ("dout = NULL",)
            bad = dout.numpy() != want_dout
            assert not bad.any(), what + (int(bad.sum()), np.argwhere(bad)[:8].tolist(), dout.numpy()[bad][:8], want_dout[bad][:8])


def test_l1_gradient_random(mau):
    """randn data at (2, 2, 37, 29), more than one block: terms within 1e-6 relative of the float64 reference (the project's figure
    for these sums, tests/test_gpu_loss_terms.py::test_compute_all_loss_agrees_with_the_training_criteria); dout within
    8 * 2^-24 * (|k_l1| + 2 |k_gy| + 2 |k_gx|) per element (``dout_bound``: five float32 terms, each at most a coefficient) -- the
    case has no argument of a sgn() within rounding of 0 (``sign_margin``), so the float32 signs are the float64 ones."""
    shape = (2, 2, 37, 29)
    o, t = R.random_criteria_case(shape)
    assert R.sign_margin(o, t) > 2
    for w_l1, w_grad in R.LOSS_WEIGHTS[:3]:
        want_terms, want_dout, _ = R.l1_gradient_ref(o, t, w_l1, w_grad, real=F64)
        terms, terms_null, dout = _l1(o, t, w_l1, w_grad)
        rel = np.abs(terms.double().numpy() - want_terms) / want_terms
        err, bound = float(np.abs(dout.double().numpy() - want_dout).max()), R.dout_bound(shape, w_l1, w_grad)
        print(f"l1_gradient_loss ({w_l1}, {w_grad}): terms off by {rel.max():.2e} relative, worst |dout err| / bound {err / bound:.3f}")
        assert (rel <= 1e-6).all(), (w_l1, w_grad, rel)
        assert same_bits(terms_null, terms)
        assert err <= bound, (w_l1, w_grad, err, bound)


# ---- mau_emb_fold_fwd / mau_emb_fold_bwd ----------------------------------------------------------------------------------------------
def _fold(dims, w, emb, dweff, form):
    """-> (weff, dw or None, demb or None) as float64 arrays; form: "both", "dw" (ws = NULL) or "demb".  The workspace has exactly
    mau_emb_fold_ws_elems floats between its slacks."""
    Cout, Ct, E, N, Ep = dims
    lib, st = _lib(), _stream()
    wb, eb, gb = Flat(w.size, vals=w), Flat(emb.size, vals=emb), Flat(dweff.size, vals=dweff)
    weff = Flat(Cout * (Ct + Ep) * 9)
    _call("mau_emb_fold_fwd", wb.ptr, eb.ptr, weff.ptr, Cout, Ct, E, N, Ep, st)
    nws = lib.mau_emb_fold_ws_elems(Cout, N, E)
    assert nws == -(-Cout // R.FOLD_CO_CHUNK) * N * E
    dw, demb, ws = Flat(w.size), Flat(N * E), Flat(nws)
    _call("mau_emb_fold_bwd", wb.ptr, eb.ptr, gb.ptr, dw.ptr if form != "demb" else None, demb.ptr if form != "dw" else None,
          ws.ptr if form != "dw" else None, Cout, Ct, E, N, Ep, st)
    got_weff = weff.back().double().numpy().reshape(Cout, Ct + Ep, 9)
    ws.back()
    if form == "demb":
        assert dw.unchanged(), "dw = NULL: a buffer was written"
    if form == "dw":
        assert demb.unchanged() and ws.unchanged(), "demb = NULL: a buffer was written"
    assert wb.unchanged() and eb.unchanged() and gb.unchanged(), "an operand was written"
    return (got_weff, dw.back().double().numpy().reshape(Cout, Ct + E, 9) if form != "demb" else None,
            demb.back().double().numpy().reshape(N, E) if form != "dw" else None)


@pytest.mark.parametrize("form", ["both", "dw", "demb"])
@pytest.mark.parametrize("dims", R.FOLD_EXACT, ids=lambda d: "x".join(map(str, d)))
def test_emb_fold_exact(mau, dims, form):
    """Integer operands: W_eff, dW and demb equal the float64 reference.  One chunk of output channels (today's case), two with a
    single channel in the second (and Ct = 0, Ep == N), three with a partial last one and E no multiple of 64, five, and a fold of
    one weight.  The columns Ct + N .. Ct + Ep of W_eff are exactly 0, dW[:, :Ct] copies dW_eff[:, :Ct]; a NULL output touches
    nothing; a workspace of exactly mau_emb_fold_ws_elems floats is enough; two calls give the same bits."""
    Cout, Ct, E, N, Ep = dims
    w, emb, dweff = R.fold_case(dims)
    weff, dw, demb = _fold(dims, w, emb, dweff, form)
    want_dw, want_demb = R.emb_fold_bwd_ref(w, emb, dweff, Ct, Ep)
    assert (weff == R.emb_fold_ref(w, emb, Ct, Ep)).all() and (weff[:, Ct + N:] == 0).all() and (weff[:, :Ct] == w[:, :Ct]).all(), dims
    if dw is not None:
        assert (dw == want_dw).all() and (dw[:, :Ct] == dweff[:, :Ct]).all(), dims
    if demb is not None:
        assert (demb == want_demb).all(), (dims, np.argwhere(demb != want_demb)[:8].tolist())
    again = _fold(dims, w, emb, dweff, form)
    assert all(a is None and b is None or same_bits(a, b) for a, b in zip((weff, dw, demb), again)), (dims, "second call")


def test_emb_fold_random_deepest_layer(mau):
    """(Cout, Ct, E, N, Ep) = (1024, 64, 128, 16, 16), the deepest folded layer, 32 chunks of output channels, randn operands: each
    element within the standard bound of a float32 sum, n_terms * 2^-24 * sum |products|, of the float64 reference; n_terms = E for
    W_eff (one fmaf chain), N for dW, Cout * 9 + chunks for demb (the fmaf chains of a chunk, their join, the chunks in order).
    Derived, not measured; the largest error is printed as a fraction of it.  The tensor columns are copies: equal."""
    dims = Cout, Ct, E, N, Ep = R.FOLD_RANDOM
    w, emb, dweff = R.fold_case(dims, exact=False)
    weff, dw, demb = _fold(dims, w, emb, dweff, "both")
    want_weff = R.emb_fold_ref(w, emb, Ct, Ep)
    want_dw, want_demb = R.emb_fold_bwd_ref(w, emb, dweff, Ct, Ep)
    a_weff, a_dw, a_demb = R.emb_fold_abs_sums(w, emb, dweff, Ct)
    chunks = -(-Cout // R.FOLD_CO_CHUNK)
    assert chunks == 32
    assert (weff[:, :Ct] == w[:, :Ct]).all() and (dw[:, :Ct] == dweff[:, :Ct]).all() and (weff[:, Ct + N:] == 0).all()
    for name, got, want, n_terms, sums in (("weff", weff[:, Ct:Ct + N], want_weff[:, Ct:Ct + N], E, a_weff), ("dw", dw[:, Ct:], want_dw[:, Ct:], N, a_dw),
                                           ("demb", demb, want_demb, Cout * 9 + chunks, a_demb)):
        bound = n_terms * 2.0 ** -24 * sums
        ratio = float((np.abs(got - want) / bound).max())
        print(f"emb_fold {name}: worst |err| / bound {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)
    again = _fold(dims, w, emb, dweff, "both")
    assert all(same_bits(a, b) for a, b in zip((weff, dw, demb), again)), "second call"


# ---- mau_sum_tensors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("k", R.SUM_K)
def test_sum_tensors_exact(mau, k, dt):
    """Bit for bit against ``sum_tensors_ref`` (float32 adds in the order given, one rounding).  C = 8: one vector per pixel, 2048
    pixels per workgroup; 20: pad lanes (zero in the sources: zero in the sum; for k = 2 they hold values, and the destination's pad
    is their sum); 24; 2056: 257 vectors, the vector loop strides.  Pixel counts 1, one below and one above a workgroup's share,
    three shares and 5.  Every source has its own pitch, every other one is a slot at channel 8 of a wider NaN-filled buffer; the
    destination is a slot at channel 8 of a buffer of pitch C8 + 24: lanes outside [8, 8 + C8) and the slack pixels stay NaN.

    The destination is never one of the sources: ``functional.Fanout.backward`` (the only caller) allocates a fresh tensor for every
    launch, also when it folds more than 8 readers in groups -- there is no aliasing case to test."""
    code, st = _code(dt), _stream()
    esz = torch.empty(0, dtype=dt).element_size()
    for C in R.SUM_C:
        C8 = pad8(C)
        for npix in R.sum_npix(C):
            r = R._rng(15, k, C, npix)
            bufs, vals, ptrs, lds = [], [], [], []
            for i in range(k):
                off = 8 * (i % 2)
                ld = C8 + off + 8 * (i % 3)
                v = torch.from_numpy(r.standard_normal((npix, C8)).astype(F32)).to(dt)
                if k != 2:
                    v[:, C:] = 0
                b = Buf(npix, ld, dt)
                b.body[:, off:off + C8] = v
                bufs.append(b.cuda())
                vals.append(v)
                ptrs.append(b.ptr + off * esz)
                lds.append(ld)
            dst = Buf(npix, C8 + 24, dt).cuda()
            pa, la = (ctypes.c_void_p * k)(*ptrs), (ctypes.c_int * k)(*lds)
            _call("mau_sum_tensors", ctypes.addressof(pa), ctypes.addressof(la), k, dst.ptr + 8 * esz, C8 + 24, code, npix, C, st)
            got = dst.back()
            what = (k, dt, C, npix)
            assert bool(torch.isnan(got[:, :8].float()).all()) and bool(torch.isnan(got[:, 8 + C8:].float()).all()), what + ("lanes outside the slot were written",)
            assert same_bits(got[:, 8:8 + C8], R.sum_tensors_ref(vals, dt)), what
            if k != 2:
                assert bool((got[:, 8 + C:8 + C8] == 0).all()), what
            for b in bufs:
                torch.cuda.synchronize()
                assert same_bits(b.dev.cpu(), b.host, nan_matches_nan=True), what + ("a source was written",)


# ---- mau_nchw_to_nhwc / mau_nhwc_to_nchw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_exact(mau, shape, dt):
    """Forward: the bits of torch's ``.to(dt)`` of the permuted tensor (round to nearest even; any NaN matches any NaN), on randn data
    with planted values: exact ties of bf16 and fp16 in both directions, the largest finite value and the first value that rounds to
    infinity, both infinities, -0.0, a NaN, fp16 subnormals.  Pad lanes [C, C8) are 0, channels [C8, ld) and the slack pixels
    untouched; ld = C8 and C8 + 16.  HW below, at and above a 256-pixel block (99, 256, 40, 1, 527).  Inverse: exact widening of the
    same 16-bit values (pad and outer lanes NaN: none may reach the output), nothing written outside dst."""
    N, C, H, W = shape
    C8, code, st = pad8(C), _code(dt), _stream()
    x = R.layout_case(shape)
    xt = torch.from_numpy(x)
    want = xt.permute(0, 2, 3, 1).reshape(N * H * W, C).to(dt)
    src = Flat(x.size, vals=x)
    for ld in (C8, C8 + 16):
        dst = Buf(N * H * W, ld, dt).cuda()
        _call("mau_nchw_to_nhwc", src.ptr, dst.ptr, code, N, C, H, W, ld, st)
        got = dst.back()
        assert same_bits(got[:, :C], want, nan_matches_nan=True), (shape, dt, ld)
        assert bool((got[:, C:C8].float() == 0).all()) and not bool(torch.signbit(got[:, C:C8].float()).any()), (shape, dt, ld, "pad lanes")
        assert bool(torch.isnan(got[:, C8:].float()).all()), (shape, dt, ld, "channels beyond C8 were written")
        assert src.unchanged()
        back_src = Buf(N * H * W, ld, dt)
        back_src.body[:, :C] = want
        back_src.cuda()
        out = Flat(x.size)
        _call("mau_nhwc_to_nchw", back_src.ptr, out.ptr, code, N, C, H, W, ld, st)
        widened = want.float().view(N, H, W, C).permute(0, 3, 1, 2).reshape(-1)
        assert same_bits(out.back(), widened, nan_matches_nan=True), (shape, dt, ld, "inverse")
