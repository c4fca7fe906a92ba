"""CPU-only checks around the training criteria (csrc/head.hip: mau_mse_fwd_bwd, mau_l1_gradient_loss), the embedding fold
(csrc/embfold.hip), the gradient sum and the layout boundary (csrc/spatial.hip): the references of tests/criteria_ref.py against torch
float64 autograd (an oracle that is wrong proves nothing on the GPU), the proof that every generated "exact" case is exact -- which is
what lets tests/test_gpu_criteria.py demand equality --, the planted values of the layout cases, and the launchers' refusals.  No
kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import unet_ref as O
from tests import criteria_ref as R

F32, F64 = np.float32, np.float64
L1_SHAPES = [(1, 1, 1, 1), (2, 2, 1, 9), (2, 2, 9, 1), (3, 2, 2, 2), (2, 2, 17, 13), (1, 3, 16, 16)]
L1_LARGE_256CU = (1, 3, 681, 257)          # the GPU test's grid-stride case as it comes out on a device of 256 compute units
MSE_N = [1, 3, 4, 5, 1023, 1024, 1027]
MSE_LARGE_256CU = 4 * 256 * 8 * 256 + 1027


@pytest.fixture(scope="module")
def lib():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    return _lib


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err <= tol, (what, err)


# ---- the references against torch float64 autograd -------------------------------------------------------------------------------
def _autograd(o, t, w_l1, w_grad):
    """the criterion of oracle/unet_ref.py (loss_l1_gradient's pixel term, gradient_loss) in float64, weighted with the float32 weights
    the entry point receives; -> (pixel, gradient, d total / d out)"""
    oo = torch.from_numpy(o.astype(F64)).requires_grad_(True)
    tt = torch.from_numpy(t.astype(F64))
    pixel, grad = O.loss_l1_gradient(oo, tt, 1.0)["pixel"], O.gradient_loss(oo, tt)["gradient"]
    (float(F32(w_l1)) * pixel + float(F32(w_grad)) * grad).backward()
    return float(pixel.detach()), float(grad.detach()), oo.grad.numpy()


@pytest.mark.parametrize("shape", [(3, 2, 2, 2), (2, 2, 17, 13), (1, 3, 16, 16), "random"], ids=str)
def test_l1_gradient_reference_against_torch_autograd(shape):
    """Values to 1e-12 relative (the float64 form of the reference; on an exact case the float32 form has the same sums bit for bit);
    the float32 dout against autograd's within ``dout_bound``: five float32 terms, each at most a coefficient.  Autograd's |x| has
    derivative 0 at 0, like sgn(0) = 0: the data has the ties, and how many elements sit on one is printed and must not be zero.
    (H == 1 or W == 1 is not compared here: torch's mean of no elements is NaN, the kernel's term is 0 by its guarded coefficient.)"""
    exact = shape != "random"
    o, t = R.exact_criteria_case(shape) if exact else R.random_criteria_case((2, 2, 37, 29))
    ties = R.tie_counts(o, t)
    print(shape, ties)
    if exact:
        assert ties["eq"] > 0 and ties["dy_zero"] > 0 and ties["dy_abs"] > 0 and ties["dx_zero"] > 0 and ties["dx_abs"] > 0, ties
    else:
        assert R.sign_margin(o, t) > 2                        # the float32 signs are the float64 signs
    for w_l1, w_grad in R.LOSS_WEIGHTS[:3]:
        pixel, grad, dref = _autograd(o, t, w_l1, w_grad)
        terms64, g64, sums64 = R.l1_gradient_ref(o, t, w_l1, w_grad, real=F64)
        _close(terms64[0], pixel, "pixel")
        _close(terms64[1] + terms64[2], grad, "gradient")
        _close(g64, dref, "dout, float64")
        terms, g, sums = R.l1_gradient_ref(o, t, w_l1, w_grad)
        assert g.dtype == F32 and terms.dtype == F32
        if exact:
            assert (sums == sums64).all() and (terms == terms64.astype(F32)).all()
        else:
            _close(terms, terms64, "terms", 1e-6)
        err = np.abs(g.astype(F64) - dref).max()
        assert err <= R.dout_bound(o.shape, w_l1, w_grad), (w_l1, w_grad, err, R.dout_bound(o.shape, w_l1, w_grad))


def test_mse_reference_against_torch_autograd():
    """loss to 1e-12 relative before its rounding to float32; dout within 3 * 2^-24 relative of 2 (o - t) / n per element: the
    difference is exact on these cases, the factor float32(2 / float32(n)) and the product round once each"""
    for n in MSE_N + [4099]:
        o, t = R.exact_flat_case(n)
        oo = torch.from_numpy(o.astype(F64)).requires_grad_(True)
        ref = O.loss_mse(oo, torch.from_numpy(t.astype(F64)))["mse"]
        ref.backward()
        loss, dout, S = R.mse_ref(o, t)
        assert loss.dtype == F32 and dout.dtype == F32
        _close(S / n, float(ref.detach()), ("mse", n))
        assert abs(float(loss) - float(ref.detach())) <= 2.0 ** -24 * float(ref.detach()), n
        assert (np.abs(dout.astype(F64) - oo.grad.numpy()) <= 3 * 2.0 ** -24 * np.abs(oo.grad.numpy())).all(), n


def test_fold_reference_against_torch_autograd():
    """W_eff = [W[:, :Ct] | W[:, Ct:] . emb^T | 0] written with torch.cat / einsum in float64, and its autograd"""
    Cout, Ct, E, N, Ep = dims = (70, 8, 100, 5, 16)
    w, emb, dweff = R.fold_case(dims, exact=False)
    w2 = torch.from_numpy(w.reshape(Cout, Ct + E, 3, 3)).requires_grad_(True)
    e2 = torch.from_numpy(emb).requires_grad_(True)
    T = torch.einsum("oekl,ie->oikl", w2[:, Ct:], e2)
    ref = torch.cat([w2[:, :Ct], T, torch.zeros(Cout, Ep - N, 3, 3, dtype=torch.float64)], dim=1)
    ref.backward(torch.from_numpy(dweff.reshape(Cout, Ct + Ep, 3, 3)))
    _close(R.emb_fold_ref(w, emb, Ct, Ep), ref.detach().numpy().reshape(Cout, Ct + Ep, 9), "weff")
    dw, demb = R.emb_fold_bwd_ref(w, emb, dweff, Ct, Ep)
    _close(dw, w2.grad.numpy().reshape(Cout, Ct + E, 9), "dw")
    _close(demb, e2.grad.numpy(), "demb")


def test_sum_reference_rounds_once():
    """three bf16 values whose float32 sum is representable although the sum of the first two is not: one rounding keeps it"""
    a = [torch.tensor([v]).bfloat16() for v in (1.0, 2.0 ** -9, -1.0)]
    assert float(R.sum_tensors_ref(a, torch.bfloat16)) == 2.0 ** -9 and float((a[0] + a[1]) + a[2]) == 0.0
    assert R.sum_pixb(8) == 2048 and R.sum_pixb(24) == 680 and R.sum_pixb(2056) == 8


# ---- every generated exact case is exact ----------------------------------------------------------------------------------------
def _assert_exact_terms(o, t, what):
    """every float32 term equals its float64 value, and the float64 sums of the terms are the same bits in forward, reversed and
    shuffled order (sequential sums: ``cumsum``): multiples of 1/8 (1/64 for the squares) whose sum stays far below 2^53 / 64"""
    assert R.is_eighths(o) and R.is_eighths(t), what
    o4, t4 = o.reshape((1, 1, 1, -1)) if o.ndim == 1 else o, t.reshape((1, 1, 1, -1)) if t.ndim == 1 else t
    d32, d64 = R.criteria_differences(o4, t4), R.criteria_differences(o4.astype(F64), t4.astype(F64))
    assert all(a.dtype == F32 and (a.astype(F64) == b).all() for a, b in zip(d32, d64)), what
    sq = d32[0] * d32[0]
    assert sq.dtype == F32 and (sq.astype(F64) == d64[0] * d64[0]).all(), what
    rng = np.random.default_rng(5)
    for terms in (sq, np.abs(d32[0]), np.abs(d32[2]), np.abs(d32[4])):
        v = terms.astype(F64).ravel()
        if not v.size:
            continue
        want = v.sum()
        for order in (v, v[::-1], rng.permutation(v)):
            got = np.cumsum(order)[-1]
            assert got.dtype == F64 and got.tobytes() == want.tobytes(), what


def test_exact_criteria_cases_are_exact():
    for shape in L1_SHAPES + [L1_LARGE_256CU]:
        for seed in (0, 1):
            o, t = R.exact_criteria_case(shape, seed)
            _assert_exact_terms(o, t, (shape, seed))
            _, _, sums = R.l1_gradient_ref(o, t, 0.7, 2.5)
            _, _, sums64 = R.l1_gradient_ref(o, t, 0.7, 2.5, real=F64)
            assert sums.tobytes() == sums64.tobytes(), shape
            c = R.tie_counts(o, t)
            B, Cc, H, W = shape
            print(shape, seed, f"{o.size} elements:", c)
            if B * Cc >= 3:                                   # one plane per kind of border tie
                assert min(c["eq_first_row"], c["eq_last_row"], c["eq_first_col"], c["eq_last_col"]) > 0, (shape, c)
                if H > 1:
                    assert c["dy_zero"] > 0 and c["dy_abs"] > 0 and c["dy_zero_first"] + c["dy_abs_first"] > 0 and c["dy_zero_last"] + c["dy_abs_last"] > 0, (shape, c)
                if W > 1:
                    assert c["dx_zero"] > 0 and c["dx_abs"] > 0 and c["dx_zero_first"] + c["dx_abs_first"] > 0 and c["dx_zero_last"] + c["dx_abs_last"] > 0, (shape, c)
                if H > 2 and W > 1:                           # both kinds on both border rows
                    assert min(c["dy_zero_first"], c["dy_abs_first"], c["dy_zero_last"], c["dy_abs_last"]) > 0, (shape, c)
                if W > 2 and H > 1:
                    assert min(c["dx_zero_first"], c["dx_abs_first"], c["dx_zero_last"], c["dx_abs_last"]) > 0, (shape, c)
    assert R.tie_counts(*R.exact_criteria_case((1, 1, 1, 1), 0))["eq"] == 1 and R.tie_counts(*R.exact_criteria_case((1, 1, 1, 1), 1))["eq"] == 0


def test_plane_and_row_ends_differ_strongly():
    """what makes a dy across a plane boundary, or a dx across a row end, change the sums: |dy o| of the pair (last row, first row
    of the next plane) is about 7 where |dy t| is at most 2, except where a forced border tie took the place: the leaked terms average more than 1, eight
    units of the data, over each boundary"""
    for shape in [(2, 2, 17, 13), (1, 3, 16, 16), (3, 2, 2, 2)]:
        o, t = R.exact_criteria_case(shape)
        B, Cc, H, W = shape
        o, t = o.reshape(B * Cc, H, W).astype(F64), t.reshape(B * Cc, H, W).astype(F64)
        leak_y = np.abs(np.abs(o[1:, 0] - o[:-1, -1]) - np.abs(t[1:, 0] - t[:-1, -1]))
        leak_x = np.abs(np.abs(o[:, 1:, 0] - o[:, :-1, -1]) - np.abs(t[:, 1:, 0] - t[:, :-1, -1]))
        assert leak_y.mean() > 1, (shape, leak_y)
        assert leak_x.mean() > 1, (shape, leak_x)


def test_exact_mse_cases_are_exact():
    for n in MSE_N + [MSE_LARGE_256CU]:
        o, t = R.exact_flat_case(n)
        _assert_exact_terms(o, t, n)
        if n > 4:
            assert R.tie_counts(o.reshape(1, 1, 1, n), t.reshape(1, 1, 1, n))["eq"] > 0, n


def test_exact_fold_cases_stay_below_2_to_24():
    """integers in [-3, 3]: every product and every partial sum of the three contractions is an integer below 2^24 in magnitude, so
    fmaf chains and adds in any order are exact in float32"""
    for dims in R.FOLD_EXACT:
        w, emb, dweff = R.fold_case(dims)
        for a in (w, emb, dweff):
            assert (a == np.round(a)).all() and np.abs(a).max() <= 3
        assert max(float(s.max()) for s in R.emb_fold_abs_sums(w, emb, dweff, dims[1])) < 2 ** 24, dims
        assert -(-dims[0] // R.FOLD_CO_CHUNK) == {24: 1, 33: 2, 70: 3, 130: 5, 1: 1}[dims[0]]
    assert -(-R.FOLD_RANDOM[0] // R.FOLD_CO_CHUNK) == 32


def test_planted_layout_values():
    """the planted values are what their description says, judged by torch's conversion: the ties go to the even neighbour in both
    directions, the largest finite values stay finite, the next tie becomes infinite, fp16 subnormals survive"""
    v = torch.from_numpy(R.planted_values())
    f = lambda x: torch.tensor([x], dtype=torch.float32)      # noqa: E731
    b = lambda bits: torch.tensor([bits], dtype=torch.int32).view(torch.float32)      # noqa: E731
    assert b(0x3F808000).bfloat16().view(torch.int16).item() == 0x3F80 and b(0x3F818000).bfloat16().view(torch.int16).item() == 0x3F82
    assert torch.isfinite(b(0x7F7F7FFF).bfloat16()).all() and torch.isinf(b(0x7F7F8000).bfloat16()).all()
    assert f(1 + 2.0 ** -11).half().item() == 1.0 and f(1 + 3 * 2.0 ** -11).half().item() == 1 + 2.0 ** -9
    assert f(np.nextafter(F32(65520.0), F32(0))).half().item() == 65504.0 and torch.isinf(f(65520.0).half()).all()
    assert f(2.0 ** -25).half().item() == 0.0 and f(3 * 2.0 ** -25).half().item() == 2.0 ** -23 and f(761.5 * 2.0 ** -24).half().item() == 762 * 2.0 ** -24
    for x in (0x3F808000, 0x3F818000, 0x7F7F8000):
        assert (v.view(torch.int32) == x).any() and (v.view(torch.int32) == x - 0x80000000).any()          # both signs
    assert torch.isnan(v).sum() == 1 and torch.isinf(v).sum() >= 2 and ((v == 0) & torch.signbit(v)).any()
    for shape in R.LAYOUT_SHAPES:
        x = R.layout_case(shape)
        if x.size > v.numel():
            assert np.isnan(x).sum() == 1 and np.isinf(x).sum() >= 2, shape
            assert np.isin(v[~torch.isnan(v)].numpy().view(np.uint32), x.view(np.uint32)).all(), shape


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(lib):
    """Refused on the host with MAU_ERR_ARG, before any launch (the pointers are never dereferenced), with the entry point's own
    message in mau_last_error."""
    raw = (C.c_char * 512)()
    p = (C.addressof(raw) + 63) // 64 * 64                    # 64-byte aligned, 448 bytes behind it
    odd = p + 4                                               # 4-byte aligned only
    L, F = lib.lib, lib.MAU_F32
    srcs, lds = (C.c_void_p * 8)(*[p] * 8), (C.c_int * 8)(*[24] * 8)
    sigs = {
        "mse_fwd_bwd": dict(out=p, tgt=p, partial=p, loss=p, dout=p, n=64, stream=None),
        "l1_gradient_loss": dict(out=p, tgt=p, partial=p, terms=p, dout=p, w_l1=1.0, w_grad=1.0, B=2, C=2, H=4, W=4, stream=None),
        "sum_tensors": dict(srcs=C.addressof(srcs), lds=C.addressof(lds), k=2, dst=p, lddst=24, dtype=F, npix=4, C=20, stream=None),
        "emb_fold_fwd": dict(w=p, emb=p, weff=p, Cout=4, Ct=8, E=64, N=3, Ep=16, stream=None),
        "emb_fold_bwd": dict(w=p, emb=p, dweff=p, dw=p, demb=p, ws=p, Cout=4, Ct=8, E=64, N=3, Ep=16, stream=None),
        "nchw_to_nhwc": dict(src=p, dst=p, dtype=F, N=1, C=20, H=2, W=2, ld=24, stream=None),
        "nhwc_to_nchw": dict(src=p, dst=p, dtype=F, N=1, C=20, H=2, W=2, ld=24, stream=None),
    }
    n = 0

    def refused(name, why, **changed):
        nonlocal n
        args = dict(sigs[name], **changed)
        assert len(args) == len(lib.PROTOTYPES["mau_" + name][1]), name
        status = getattr(L, "mau_" + name)(*args.values())
        msg = L.mau_last_error()
        assert status == 1 and (name + ": ").encode() in msg and b"_kernel" not in msg, (name, why, changed, status, msg)
        n += 1

    for arg in ("out", "tgt", "dout"):
        refused("mse_fwd_bwd", "misaligned " + arg, **{arg: odd})
    refused("mse_fwd_bwd", "n = 0", n=0)
    for arg in ("out", "tgt", "partial", "loss"):
        refused("mse_fwd_bwd", "null " + arg, **{arg: None})
    for arg in "BCHW":
        refused("l1_gradient_loss", arg + " = 0", **{arg: 0})
    for arg in ("out", "tgt", "partial", "terms"):
        refused("l1_gradient_loss", "null " + arg, **{arg: None})
    refused("sum_tensors", "k = 0", k=0)
    refused("sum_tensors", "k = 9", k=L.mau_sum_tensors_max() + 1)
    assert L.mau_sum_tensors_max() == 8
    refused("sum_tensors", "misaligned destination", dst=odd)
    refused("sum_tensors", "lddst % 8", lddst=28)
    refused("sum_tensors", "lddst < C8", lddst=16)
    for i in (0, 1):
        for why, (ptr, ld) in {"ld % 8": (p, 28), "ld < C8": (p, 16), "misaligned": (odd, 24), "null": (None, 24)}.items():
            s2, l2 = (C.c_void_p * 8)(*[p] * 8), (C.c_int * 8)(*[24] * 8)
            s2[i], l2[i] = ptr, ld
            refused("sum_tensors", f"source {i}: {why}", srcs=C.addressof(s2), lds=C.addressof(l2))
    s2, l2 = (C.c_void_p * 8)(*[p] * 8), (C.c_int * 8)(*[24] * 8)
    s2[2], l2[2] = None, 3                                    # beyond k: not looked at
    for name in ("emb_fold_fwd", "emb_fold_bwd"):
        refused(name, "Ep < N", Ep=2)
        refused(name, "E, N over 64 KB of LDS", E=1024, N=16)         # fwd: (9 + 16) * 1024 floats; bwd: 16 * (9 + 1024)
        refused(name, "Ct < 0", Ct=-1)
    refused("emb_fold_fwd", "no output", weff=None)
    refused("emb_fold_bwd", "no output", dw=None, demb=None)
    refused("emb_fold_bwd", "demb without ws", ws=None)
    refused("emb_fold_bwd", "demb without ws, no dw", dw=None, ws=None)
    for name in ("nchw_to_nhwc", "nhwc_to_nchw"):
        refused(name, "ld < C", ld=16)
        refused(name, "ld % 8", ld=28)
        refused(name, "null src", src=None)
        refused(name, "null dst", dst=None)
    print(f"{n} refusals")
