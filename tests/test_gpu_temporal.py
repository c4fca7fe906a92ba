"""The embedding branch's kernels through the C ABI (ctypes): the persistent LSTM forward and backward and the chunked dW_hh product of
csrc/lstm.hip at every hidden-size class (HP = 32 / 64 / 96 / 128, CPT = 2 / 6 / 8), around the class boundaries, the 8-step blocks of
the backward and the 512-row chunks of dW_hh; the Linear and metadata-MLP kernels of csrc/head.hip.  References: tests/temporal_ref.py
(pinned on the CPU by tests/test_temporal_host.py).

Buffers.  Everything a kernel writes is over-allocated by PAD floats at both ends and NaN-prefilled: the sentinels must still be NaN after
the call and every element inside finite (h_last, gates, cells, the gradients, the workspace of exactly mau_lstm_bwd_ws_elems floats).
Inputs carry NaN directly in front of and behind their elements, so a read outside poisons the result.

Tolerance.  For one output tensor, err = max |got - ref64| / max |ref64| may be at most 16 * e32 with a floor of 2^-20, e32 being the same
figure of the plain fp32 CPU loop (libm nonlinearities, left-to-right sums) against the float64 loop.  Where the reference is exactly zero
the bound is absolute, 2^-20.  The kernel forms tanh as 1 - 2 rcp(1 + exp(2x)) on the hardware exp / rcp (absolute error about an ulp of
1.0, three times per unit and step) and sums each dot product in four quarters and two interleaved halves: hence a factor, 16.

Measured on one MI355X, largest err / e32 per output with its case (B, T, H), over the grid, the seam cases and saturation (cases whose
bound is the floor, 16 * e32 < 2^-20, counted apart: there the largest err was 0.27 * 2^-20, h_last at (3, 1, 5)); none above 16:
  gates 3.43 (3, 41, 127) | cells 6.84 (3, 1, 127) | h_last 11.90 (3, 1, 63) | dw_ih 2.62 (3, 8, 5) | dw_hh 3.39 (3, 8, 127) |
  db_ih = db_hh 3.11 (3, 8, 5)          (the two large ones are single steps, where e32 itself is below 1e-7: err is 1.2e-6 and 6.6e-7)
  module level (4, 20, 128): embedding 3.19, fc.weight 4.51, weight_hh 2.25, weight_ih 1.71, biases 1.00 at (4, 20, 64)
  Linear (37, 96, 64): out 0.81, dx 1.00, dw 1.00, db 1.54;  metadata MLP (50, 4, 32, 64): 0.84 .. 1.39
The file runs in 4.4 s there (50 tests), the slowest test in 0.9 s.

Bitwise structure tests.  Reading lstm.hip, no summation order depends on H inside one hidden-size class: the forward's k quarters, the
backward's 16 parts of the gate-gradient vector and the dW_hh tile's (sample, step) order are fixed by HP, CPT, B and T alone, so padding
invariance compares every output bit for bit.  One comparison of the prefix property cannot be bitwise: h_last against o * tanh(c) of the
last step.  The kernel evaluates that tanh on the hardware exp / rcp, which no CPU evaluation reproduces bit for bit; the test holds it to
the absolute bound 2^-20 instead (exp 1 ulp, the sum half an ulp, rcp 1 ulp: 2.5 * 2^-23 relative on r <= 1, twice that on 2r, half an
ulp each for 1 - 2r and the product with o: 6 * 2^-23 < 2^-20), and to the inference path's h_last bit for bit."""
import math
import types

import pytest
import torch

from tests import temporal_ref as TR
from tests._helpers import _bits_equal, _call, _nbits_differ, _stream, mau  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64                                                      # sentinel floats in front of and behind every buffer
FLOOR = 2.0 ** -20
FACTOR = 16.0


class In:
    """a kernel input: the float32 values with PAD NaNs in front and behind"""

    def __init__(self, values):
        v = values.detach().float().reshape(-1)
        host = torch.full((v.numel() + 2 * PAD,), NAN)
        host[PAD:PAD + v.numel()] = v
        self.dev = host.cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * PAD


class Out:
    """a buffer a kernel writes: NaN everywhere, PAD sentinels at both ends"""

    def __init__(self, *shape):
        self.shape, self.n = shape, math.prod(shape)
        self.dev = torch.full((self.n + 2 * PAD,), NAN, device="cuda")

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * PAD

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.dev).all())

    def back(self):
        torch.cuda.synchronize()
        r = self.dev.cpu()
        assert bool(torch.isnan(r[:PAD]).all()) and bool(torch.isnan(r[PAD + self.n:]).all()), "elements outside the buffer were written"
        body = r[PAD:PAD + self.n]
        assert bool(torch.isfinite(body).all()), f"{int((~torch.isfinite(body)).sum())} of {self.n} elements not finite (unwritten, or poisoned by a read outside an input)"
        return body.view(self.shape).clone()


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------------
_worst = {}


def _within(name, got, ref64, val32, case, absolute_where_zero=False):
    """err <= max(16 * e32, 2^-20) in the normalisation of temporal_ref.yardstick; prints the figures before it asserts"""
    got, ref64 = got.double(), ref64.double()
    den = float(ref64.abs().max())
    if absolute_where_zero or den == 0.0:
        zero = ref64 == 0
        if bool(zero.any()):
            worst0 = float(got[zero].abs().max())
            assert worst0 <= FLOOR, (name, case, "reference exactly 0", worst0)
        if den == 0.0:
            return
    e32 = TR.yardstick(ref64, val32)
    err = TR.yardstick(ref64, got)
    bound = max(FACTOR * e32, FLOOR)
    floored = FACTOR * e32 < FLOOR
    ratio = err / e32 if e32 > 0 else float("inf")
    key = (name, "floor" if floored else "e32")
    fig = err / FLOOR if floored else ratio
    if fig > _worst.get(key, (0.0, None))[0]:
        _worst[key] = (fig, case)
    print(f"RATIO {name:7s} case {case} err {err:.3e} e32 {e32:.3e} err/e32 {ratio:.3f} err/bound {err / bound:.3f}" + (" (floor)" if floored else ""))
    assert err <= bound, (name, case, err, e32, ratio)


def _print_worst():
    for (name, kind), (fig, case) in sorted(_worst.items()):
        print(f"WORST {name:7s} {'err/2^-20 under the floor' if kind == 'floor' else 'err/e32'} {fig:.3f} at {case}")


# ---- launching the LSTM -------------------------------------------------------------------------------------------------------------------
def _lstm_fwd(c, B, T, H, save=True):
    """mau_lstm_fwd on the inputs of ``c``; the buffers stay on the device for a backward"""
    assert c["x"].shape == (B, T) and c["w_hh"].shape == (4 * H, H)
    f = types.SimpleNamespace(B=B, T=T, H=H)
    f.ins = {k: In(c[k]) for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh")}
    f.h = Out(B, H)
    f.gates = Out(B, T, 4 * H) if save else None
    f.cells = Out(B, T, H) if save else None
    i = f.ins
    _call("mau_lstm_fwd", i["x"].ptr, i["w_ih"].ptr, i["w_hh"].ptr, i["b_ih"].ptr, i["b_hh"].ptr, f.h.ptr,
          f.gates.ptr if save else None, f.cells.ptr if save else None, B, T, H, _stream())
    f.out = {"h_last": f.h.back()}
    if save:
        f.out["gates"], f.out["cells"] = f.gates.back(), f.cells.back()
    return f


def _lstm_bwd(f, dh_last):
    """mau_lstm_bwd behind ``_lstm_fwd``: fresh NaN-filled gradients and a workspace of exactly the queried size"""
    from mau_amd._lib import lib
    B, T, H = f.B, f.T, f.H
    need = lib.mau_lstm_bwd_ws_elems(B, T, H)
    assert need == B * T * 4 * H + B * 8 * H + -(-B * T // 512) * 4 * H * H
    ws, dh = Out(need), In(dh_last)
    g = {"dw_ih": Out(4 * H), "dw_hh": Out(4 * H, H), "db_ih": Out(4 * H), "db_hh": Out(4 * H)}
    _call("mau_lstm_bwd", f.ins["x"].ptr, f.ins["w_hh"].ptr, f.gates.ptr, f.cells.ptr, dh.ptr, g["dw_ih"].ptr, g["dw_hh"].ptr,
          g["db_ih"].ptr, g["db_hh"].ptr, ws.ptr, B, T, H, _stream())
    out = {k: v.back() for k, v in g.items()}
    ws.back()
    assert _bits_equal(f.gates.back(), f.out["gates"]) and _bits_equal(f.cells.back(), f.out["cells"])          # inputs of the backward
    return out


def _compare_case(B, T, H, seed, **kw):
    """forward + backward of one case against the float64 reference at the tolerance rule; returns the kernel's outputs"""
    c, ref, y32 = TR.lstm_case_refs(B, T, H, seed, **kw)
    f = _lstm_fwd(c, B, T, H)
    out = dict(f.out)
    out.update(_lstm_bwd(f, c["dh_last"]))
    case = (B, T, H)
    sat = "bias" in kw
    for k in TR.LSTM_OUTPUTS:
        _within(k, out[k], ref[k], y32[k], case, absolute_where_zero=sat and k.startswith("d"))
    assert _bits_equal(out["db_ih"], out["db_hh"])
    return out


# ---- a. accuracy grid -------------------------------------------------------------------------------------------------------------------------
GRID_H = [1, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
GRID_T = [1, 7, 8, 9, 16, 17, 41]


@pytest.mark.parametrize("H", GRID_H)
def test_lstm_accuracy_grid(mau, H):
    """B = 3, every T of the grid: gates, cells, h_last and the four gradients within 16 * e32 (floor 2^-20) of the float64 loop; db_ih and
    db_hh the same bits.  H on both sides of every class boundary, not a multiple of 4, 1; T = 1, below, at and above one and two 8-step
    blocks (1, 2, 3 and 6 blocks of the backward)."""
    for T in GRID_T:
        out = _compare_case(3, T, H, seed=1000 * H + T)
        if T == 1:
            assert float(out["dw_hh"].abs().max()) == 0.0      # h_0 = 0
    _print_worst()


# ---- b. exact structure -------------------------------------------------------------------------------------------------------------------------
def _embed(c, H, HP):
    """the H-unit problem inside an HP-unit one: the extra units have zero rows and columns of w_hh, zero w_ih, biases and dh_last"""
    def rows(v):                                              # (4H, ...) -> (4HP, ...), gate blocks kept
        out = torch.zeros((4, HP) + tuple(v.shape[1:]))
        out[:, :H] = v.view((4, H) + tuple(v.shape[1:]))
        return out.view((4 * HP,) + tuple(v.shape[1:]))
    w = torch.zeros(4 * H, HP)
    w[:, :H] = c["w_hh"]
    dh = torch.zeros(c["dh_last"].shape[0], HP)
    dh[:, :H] = c["dh_last"]
    return {"x": c["x"], "w_ih": rows(c["w_ih"]), "w_hh": rows(w), "b_ih": rows(c["b_ih"]), "b_hh": rows(c["b_hh"]), "dh_last": dh}


@pytest.mark.parametrize("H,HP", [(5, 32), (37, 64), (70, 96), (101, 128)])
def test_lstm_padding_invariance_bitwise(mau, H, HP):
    """The H-unit run and the same weights embedded in the HP-unit problem of its class select the same instantiations and sum in the same
    order: every output of the real units bit for bit, every extra unit exactly 0.  Checks each ``live`` / ``< H`` mask exactly."""
    B, T = 3, 17
    c = TR.lstm_case(B, T, H, seed=77 * H)
    e = _embed(c, H, HP)
    f, fe = _lstm_fwd(c, B, T, H), _lstm_fwd(e, B, T, HP)
    ge = fe.out["gates"].view(B, T, 4, HP)
    assert _bits_equal(ge[..., :H].reshape(B, T, 4 * H), f.out["gates"]), _nbits_differ(ge[..., :H].reshape(B, T, 4 * H), f.out["gates"])
    assert _bits_equal(fe.out["cells"][..., :H], f.out["cells"]) and _bits_equal(fe.out["h_last"][:, :H], f.out["h_last"])
    if HP > H:
        assert float(fe.out["cells"][..., H:].abs().max()) == 0.0 and float(fe.out["h_last"][:, H:].abs().max()) == 0.0
    g, gE = _lstm_bwd(f, c["dh_last"]), _lstm_bwd(fe, e["dh_last"])
    for k in ("dw_ih", "db_ih", "db_hh"):
        got = gE[k].view(4, HP)[:, :H].reshape(4 * H)
        assert _bits_equal(got, g[k]), (k, _nbits_differ(got, g[k]))
        assert float(gE[k].view(4, HP)[:, H:].abs().max()) == 0.0, k
    got = gE["dw_hh"].view(4, HP, HP)[:, :H, :H].reshape(4 * H, H)
    assert _bits_equal(got, g["dw_hh"]), _nbits_differ(got, g["dw_hh"])
    assert float(gE["dw_hh"].view(4, HP, HP)[:, H:].abs().max()) == 0.0 and float(gE["dw_hh"].view(4, HP, HP)[:, :, H:].abs().max()) == 0.0


@pytest.mark.parametrize("H", [33, 128])
def test_lstm_prefix_property_bitwise(mau, H):
    """gates[:, :T'] and cells[:, :T'] of the T = 41 run are those of the T'-run on x[:, :T'], bit for bit; the T'-run's h_last is o * tanh(c)
    of its last step (absolute 2^-20: the kernel's tanh is the hardware's, see the module docstring) and, bit for bit, the h_last of the
    path that saves nothing."""
    B, T = 3, 41
    c = TR.lstm_case(B, T, H, seed=41 * H)
    full = _lstm_fwd(c, B, T, H).out
    for Tp in (1, 7, 8, 9, 16, 17):
        cp = dict(c, x=c["x"][:, :Tp].contiguous())
        o = _lstm_fwd(cp, B, Tp, H).out
        assert _bits_equal(o["gates"], full["gates"][:, :Tp]), (Tp, _nbits_differ(o["gates"], full["gates"][:, :Tp]))
        assert _bits_equal(o["cells"], full["cells"][:, :Tp]), Tp
        implied = o["gates"][:, -1, 3 * H:].double() * torch.tanh(o["cells"][:, -1].double())
        assert float((o["h_last"].double() - implied).abs().max()) <= FLOOR, Tp
        assert _bits_equal(_lstm_fwd(cp, B, Tp, H, save=False).out["h_last"], o["h_last"]), Tp


@pytest.mark.parametrize("H", [5, 64, 96, 128])
def test_lstm_samples_are_independent_bitwise(mau, H):
    """one workgroup per sample: row b of every forward output of a B = 5 run is the B = 1 run on that sample"""
    B, T = 5, 17
    c = TR.lstm_case(B, T, H, seed=5 * H)
    full = _lstm_fwd(c, B, T, H).out
    for b in range(B):
        one = _lstm_fwd(dict(c, x=c["x"][b:b + 1].contiguous()), 1, T, H).out
        for k in ("gates", "cells", "h_last"):
            assert _bits_equal(one[k], full[k][b:b + 1]), (b, k)


@pytest.mark.parametrize("H", [31, 64, 65, 128])
def test_lstm_inference_path_equals_saving_path_bitwise(mau, H):
    """gates = cells = NULL (what the sensitivity sweeps run): the same h_last, one H per instantiation"""
    B, T = 3, 17
    c = TR.lstm_case(B, T, H, seed=3 * H)
    assert _bits_equal(_lstm_fwd(c, B, T, H, save=False).out["h_last"], _lstm_fwd(c, B, T, H).out["h_last"])


@pytest.mark.parametrize("H", [33, 128])
def test_lstm_backward_replays_bitwise(mau, H):
    """fixed-order sums, no atomics: the same backward twice into fresh NaN-filled buffers gives the same bits"""
    B, T = 3, 41
    c = TR.lstm_case(B, T, H, seed=9 * H)
    f = _lstm_fwd(c, B, T, H)
    g1, g2 = _lstm_bwd(f, c["dh_last"]), _lstm_bwd(f, c["dh_last"])
    for k in g1:
        assert _bits_equal(g1[k], g2[k]), k


# ---- c. dW_hh chunk seams -----------------------------------------------------------------------------------------------------------------------
SEAM_CASES = [(3, 200, 20), (5, 128, 128), (2, 257, 70), (1, 512, 33)]


@pytest.mark.parametrize("B,T,H", SEAM_CASES, ids=["x".join(map(str, s)) for s in SEAM_CASES])
def test_lstm_dwhh_chunk_seams(mau, B, T, H):
    """512 rows of the (sample, step) axis per chunk: a seam in the middle of a sample (row 512 of 600), a seam exactly at a sample's first
    step (5 x 128: also CPT = 8 with two chunk rows), a last chunk of 2 rows -- less than one 16-row stage -- and exactly one full chunk."""
    rows = B * T
    assert {(3, 200, 20): rows == 600 and 512 % T != 0, (5, 128, 128): rows == 640 and 512 % T == 0 and H > 96,
            (2, 257, 70): rows - 512 == 2 and 2 < 16, (1, 512, 33): rows == 512}[(B, T, H)]
    _compare_case(B, T, H, seed=B * T + H)
    _print_worst()


def test_lstm_dwhh_chunk_seam_inside_a_sample_with_long_memory(mau):
    """(3, 200, 20) again with 5 added to the forget gate's bias.  With torch's initialisation the gradient that reaches step 112 of a
    200-step sample -- the seam at row 512 -- from h_last is some ten orders of magnitude below the last steps' (a version of the product
    that drops the 16 rows in front of the seam passes the case above); here the cell state persists, the 16 rows in front of the seam
    carry more than a hundredth of max |dw_hh| (asserted on the float64 loop), and that version fails."""
    B, T, H, seed = 3, 200, 20, 620
    c, ref, y32 = TR.lstm_case_refs(B, T, H, seed, forget_bias=5.0)
    seam = 512 - 2 * T                                         # the step of sample 2 at row 512
    part = TR.lstm_dw_hh_of_steps(c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["dh_last"], 2, seam - 16, seam)
    share = float(part.abs().max()) / float(ref["dw_hh"].abs().max())
    assert share > 0.01 and share > 10 * max(FACTOR * TR.yardstick(ref["dw_hh"], y32["dw_hh"]), FLOOR), share       # ten times the bound
    _compare_case(B, T, H, seed, forget_bias=5.0)
    _print_worst()


def test_lstm_dwhh_is_additive_across_the_sample_seam(mau):
    """dw_hh is linear in dh_last: at (5, 128, 128), where the second chunk is exactly the last sample, the gradient of dh_last with only
    that sample kept plus the gradient of the complement equals the full gradient within the tolerance rule (isolates a seam error from
    a recurrence error: the last sample's run touches no row of the first chunk)."""
    B, T, H = 5, 128, 128
    c, ref, y32 = TR.lstm_case_refs(B, T, H, B * T + H)
    f = _lstm_fwd(c, B, T, H)
    last, rest = c["dh_last"].clone(), c["dh_last"].clone()
    last[:-1] = 0
    rest[-1] = 0
    gf, gl, gr = _lstm_bwd(f, c["dh_last"]), _lstm_bwd(f, last), _lstm_bwd(f, rest)
    for k in ("dw_ih", "dw_hh", "db_ih"):
        den = float(ref[k].abs().max())
        err = float((gl[k].double() + gr[k].double() - gf[k].double()).abs().max()) / den
        bound = max(FACTOR * TR.yardstick(ref[k], y32[k]), FLOOR)
        print(f"additivity {k}: |last + rest - full| / max|ref| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


# ---- d. saturation ------------------------------------------------------------------------------------------------------------------------------
def test_lstm_saturated_gates_stay_finite(mau):
    """inputs times 200, biases of +-30: gates at exactly 0 or 1, exp overflows inside the kernel's sigmoid and tanh; everything finite
    (Out.back asserts it) and within the tolerance rule, absolute 2^-20 where the reference gradient is exactly zero"""
    B, T, H = 3, 17, 33
    c, ref, _ = TR.lstm_case_refs(B, T, H, 4242, x_scale=200.0, bias=30.0)
    pre_in = c["x"][:, :, None] * c["w_ih"] + c["b_ih"] + c["b_hh"]                  # pre-activations but for the recurrent term, |h| <= 1
    slack = float(c["w_hh"].abs().sum(1).max())
    assert float(pre_in.min()) + slack < -89 and float(pre_in.max()) - slack > 89      # exp(-pre) and exp(2 pre) overflow fp32
    assert bool((ref["gates"] == 1).any()) and bool((ref["gates"] == -1).any()) and bool((ref["dw_hh"] == 0).any())
    out = _compare_case(B, T, H, seed=4242, x_scale=200.0, bias=30.0)
    assert bool((out["gates"] == 0).any()) and bool((out["gates"] == 1).any()) and bool((out["gates"] == -1).any())
    _print_worst()


# ---- e. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_lstm_refusals_launch_nothing(mau):
    from mau_amd._lib import lib
    assert lib.mau_lstm_max_hidden() == 128
    B, T = 2, 4
    for H, with_gates, with_cells in ((129, True, True), (129, False, False), (8, True, False)):
        c = TR.lstm_case(B, T, H, seed=H)
        i = {k: In(c[k]) for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "dh_last")}
        h, gates, cells = Out(B, H), Out(B, T, 4 * H), Out(B, T, H)
        st = lib.mau_lstm_fwd(i["x"].ptr, i["w_ih"].ptr, i["w_hh"].ptr, i["b_ih"].ptr, i["b_hh"].ptr, h.ptr, gates.ptr if with_gates else None,
                              cells.ptr if with_cells else None, B, T, H, _stream())
        assert st != 0 and lib.mau_last_error()
        assert h.untouched() and gates.untouched() and cells.untouched()
        g = [Out(4 * H), Out(4 * H, H), Out(4 * H), Out(4 * H), Out(lib.mau_lstm_bwd_ws_elems(B, T, H))]
        st = lib.mau_lstm_bwd(i["x"].ptr, i["w_hh"].ptr, gates.ptr if with_gates else None, cells.ptr if with_cells else None, i["dh_last"].ptr,
                              g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, g[4].ptr, B, T, H, _stream())
        assert st != 0 and all(o.untouched() for o in g)
    enc = mau.TemporalEncoder(T, 129, 4).cuda()
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(B, T, device="cuda"))


# ---- f. Linear and the metadata MLP -------------------------------------------------------------------------------------------------------------
def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def _run_linear(x, w, b, dout, want_dx):
    N, F = x.shape
    D = w.shape[0]
    i = {"x": In(x), "w": In(w), "dout": In(dout)}
    bi = In(b) if b is not None else None
    out, dx, dw, db = Out(N, D), Out(N, F), Out(D, F), Out(D)
    _call("mau_linear_fwd", i["x"].ptr, i["w"].ptr, bi.ptr if bi else None, out.ptr, N, F, D, _stream())
    _call("mau_linear_bwd", i["x"].ptr, i["w"].ptr, i["dout"].ptr, dx.ptr if want_dx else None, dw.ptr, db.ptr, N, F, D, _stream())
    r = {"out": out.back(), "dw": dw.back(), "db": db.back()}
    if want_dx:
        r["dx"] = dx.back()
    else:
        assert dx.untouched()
    return r


LINEAR_CASES = [(1, 1, 1), (3, 96, 64), (50, 7, 1), (2, 128, 100), (300, 12, 16)]


@pytest.mark.parametrize("N,F,D", LINEAR_CASES, ids=["x".join(map(str, s)) for s in LINEAR_CASES])
def test_linear_exact_on_small_integers(mau, N, F, D):
    """values in [-4, 4]: every fp32 sum is exact, the result IS the float64 reference -- D*F above and below N*F, D < N, more than one block
    of 256 threads; with and without bias, dx requested and NULL (the three roles of a thread of the backward are independent)"""
    g = torch.Generator().manual_seed(N * 7 + F * 3 + D)
    x, w, b, dout = _ints(g, N, F), _ints(g, D, F), _ints(g, D), _ints(g, N, D)
    for bias in (b, None):
        ref = TR.linear_ref(x, w, bias, dout)
        assert max(float(v.abs().max()) for v in ref.values()) < 2 ** 24
        for want_dx in (True, False):
            got = _run_linear(x, w, bias, dout, want_dx)
            for k, v in got.items():
                assert torch.equal(v.double(), ref[k]), (k, bias is not None, want_dx)


def test_linear_real_valued(mau):
    N, F, D = 37, 96, 64
    g = torch.Generator().manual_seed(11)
    x, w, b, dout = (torch.randn(s, generator=g) for s in ((N, F), (D, F), (D,), (N, D)))
    ref, y32 = TR.linear_ref(x, w, b, dout), TR.linear_ref(x, w, b, dout, torch.float32)
    got = _run_linear(x, w, b, dout, True)
    for k in ("out", "dx", "dw", "db"):
        _within("lin." + k, got[k], ref[k], y32[k], (N, F, D))
    _print_worst()


def _run_mlp_fwd(md, w0, b0, w2, b2):
    N, F = md.shape
    Hd, D = w0.shape[0], w2.shape[0]
    i = [In(v) for v in (md, w0, b0, w2, b2)]
    hidden, emb = Out(N, Hd), Out(N, D)
    _call("mau_meta_mlp_fwd", *(v.ptr for v in i), hidden.ptr, emb.ptr, N, F, Hd, D, _stream())
    return hidden.back(), emb.back()


def _run_mlp_bwd(md, w0, w2, hidden, demb):
    N, F = md.shape
    Hd, D = w0.shape[0], w2.shape[0]
    i = [In(v) for v in (md, w0, w2, hidden, demb)]
    o = {"dw0": Out(Hd, F), "db0": Out(Hd), "dw2": Out(D, Hd), "db2": Out(D), "dhidden": Out(N, Hd)}
    _call("mau_meta_mlp_bwd", *(v.ptr for v in i), o["dw0"].ptr, o["db0"].ptr, o["dw2"].ptr, o["db2"].ptr, o["dhidden"].ptr, N, F, Hd, D, _stream())
    return {k: v.back() for k, v in o.items()}


MLP_CASES = [(1, 4, 32, 8), (50, 4, 32, 64), (300, 1, 32, 256), (7, 4, 5, 3)]


@pytest.mark.parametrize("N,F,Hd,D", MLP_CASES, ids=["x".join(map(str, s)) for s in MLP_CASES])
def test_meta_mlp_exact_on_small_integers(mau, N, F, Hd, D):
    """values in [-4, 4], every sum exact: forward, the saved hidden and all gradients ARE the float64 reference; one pre-activation is
    exactly 0 and its dhidden 0 (relu'(0) = 0); the backward consumes the hidden it is given (a different saved activation gives that
    activation's gradients -- nothing is recomputed from md)."""
    g = torch.Generator().manual_seed(N + 3 * F + 5 * Hd + 7 * D)
    md, w0, b0, w2, b2, demb = _ints(g, N, F), _ints(g, Hd, F), _ints(g, Hd), _ints(g, D, Hd), _ints(g, D), _ints(g, N, D)
    j0 = 1 % Hd
    w0[j0] = 0
    w0[j0, 0] = 1
    md[0, 0] = -b0[j0]                                        # pre[0, j0] = 0 exactly
    demb[0] = demb[0].abs().clamp_min(1)
    w2[:, j0] = 1                                             # without the mask that unit's dhidden would be sum(demb[0]) > 0
    ref = TR.meta_mlp_ref(md, w0, b0, w2, b2, demb)
    assert float(ref["pre"][0, j0]) == 0.0 and float((demb[0] @ w2)[j0]) > 0
    assert max(float(v.abs().max()) for v in ref.values()) < 2 ** 24
    hidden, emb = _run_mlp_fwd(md, w0, b0, w2, b2)
    assert torch.equal(hidden.double(), ref["hidden"]) and torch.equal(emb.double(), ref["emb"])
    got = _run_mlp_bwd(md, w0, w2, hidden, demb)
    assert float(got["dhidden"][0, j0]) == 0.0
    for k, v in got.items():
        assert torch.equal(v.double(), ref[k]), k
    other = torch.roll(hidden, 1, dims=1) if Hd > 1 else hidden + 1       # another saved activation: other units masked
    dh2 = (demb.double() @ w2.double()) * (other > 0)
    got2 = _run_mlp_bwd(md, w0, w2, other, demb)
    want2 = {"dhidden": dh2, "dw2": demb.double().t() @ other.double(), "db2": ref["db2"], "dw0": dh2.t() @ md.double(), "db0": dh2.sum(0)}
    assert not torch.equal(dh2, ref["dhidden"]) or N * Hd == 1
    for k, v in got2.items():
        assert torch.equal(v.double(), want2[k]), ("other hidden", k)


def test_meta_mlp_real_valued(mau):
    N, F, Hd, D = 50, 4, 32, 64
    g = torch.Generator().manual_seed(14)
    md, w0, b0, w2, b2, demb = (torch.randn(s, generator=g) for s in ((N, F), (Hd, F), (Hd,), (D, Hd), (D,), (N, D)))
    ref, y32 = TR.meta_mlp_ref(md, w0, b0, w2, b2, demb), TR.meta_mlp_ref(md, w0, b0, w2, b2, demb, torch.float32)
    assert float(ref["pre"].abs().min()) > 1e-4                # no unit so close to 0 that fp32 and fp64 disagree about the ReLU
    hidden, emb = _run_mlp_fwd(md, w0, b0, w2, b2)
    got = dict(_run_mlp_bwd(md, w0, w2, hidden, demb), hidden=hidden, emb=emb)
    for k in ("hidden", "emb", "dhidden", "dw2", "db2", "dw0", "db0"):
        _within("mlp." + k, got[k], ref[k], y32[k], (N, F, Hd, D))
    _print_worst()


# ---- g. module level ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 128])
def test_temporal_encoder_module_against_torch_double(mau, H):
    """mau.TemporalEncoder on the GPU against its own state dict in a CPU nn.LSTM + nn.Linear in double: the embedding and every parameter
    gradient through autograd (LSTMLast, Linear, the view of dw_ih as (4H, 1)), at the tolerance rule with e32 from the same modules in
    float32 on the CPU"""
    T, B, D = 20, 4, 16
    torch.manual_seed(H)
    enc = mau.TemporalEncoder(T, H, D)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(H + 1)
    x, demb = torch.randn((B, T), generator=g), torch.randn((B, D), generator=g)

    def cpu(dtype):
        lstm, fc = torch.nn.LSTM(1, H, batch_first=True).to(dtype), torch.nn.Linear(H, D).to(dtype)
        lstm.load_state_dict({k[5:]: v.to(dtype) for k, v in sd.items() if k.startswith("lstm.")})
        fc.load_state_dict({k[3:]: v.to(dtype) for k, v in sd.items() if k.startswith("fc.")})
        _, (hn, _) = lstm(x.to(dtype).unsqueeze(-1))
        emb = fc(hn[-1])
        emb.backward(demb.to(dtype))
        r = {"emb": emb.detach()}
        r.update({"lstm." + k: p.grad for k, p in lstm.named_parameters()})
        r.update({"fc." + k: p.grad for k, p in fc.named_parameters()})
        return r

    ref, y32 = cpu(torch.float64), cpu(torch.float32)
    enc = enc.cuda()
    emb = enc(x.cuda())
    emb.backward(demb.cuda())
    torch.cuda.synchronize()
    got = {"emb": emb.detach().cpu()}
    got.update({k: p.grad.cpu() for k, p in enc.named_parameters()})
    assert set(got) == set(ref) and got["lstm.weight_ih_l0"].shape == (4 * H, 1)
    for k in sorted(ref):
        _within("mod." + k.replace("lstm.", "").replace("_l0", ""), got[k], ref[k], y32[k], (B, T, H))
    assert torch.equal(got["lstm.bias_ih_l0"], got["lstm.bias_hh_l0"])
    _print_worst()
