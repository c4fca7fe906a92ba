"""CPU-only checks around ``mau_ssim_loss_grad``: the float64 closed form of ``tests/ssim_grad_ref.py`` against float64 autograd of
the torch spelling, ``torch.clamp``'s backward on and beside its bounds with planted values, the entry point's refusals (which
need no device), the ABI rows, and the driver's refusal of ``--ssim-gradient`` with a loss that has no SSIM term."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import ssim_grad_ref as R
from tests._helpers import ssim_value_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_differentiable_spelling_is_the_helpers_value():
    """``ssim_loss_torch`` is ``ssim_value_torch`` without ``no_grad``: the same bits, in both precisions."""
    for dtype in (torch.float32, torch.float64):
        out, tgt = (v.to(dtype) for v in R.make_inputs((2, 2, 27, 43), 3))
        want = 1 - ssim_value_torch(R.prepare(out), R.prepare(tgt)).mean()
        assert torch.equal(R.ssim_loss_torch(out, tgt), want)
    out, tgt = (v.double() for v in R.make_inputs((1, 2, 640, 640), 4))           # f = round(2.5) = 2
    assert torch.equal(R.ssim_loss_torch(out, tgt), 1 - ssim_value_torch(R.prepare(out), R.prepare(tgt)).mean())
    assert R.pool_factor(384, 384) == 2 and R.pool_factor(640, 640) == 2 and R.pool_factor(385, 391) == 2 and R.pool_factor(383, 900) == 1


@pytest.mark.parametrize("shape,prep", R.SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"prep{int(v)}")
def test_closed_form_against_float64_autograd(shape, prep):
    """Both sides are float64 spellings of one formula: 1e-12 of max|g| (5e-15 was seen)."""
    out, tgt = R.make_inputs(shape, 11)
    want = R.ssim_grad_autograd(out, tgt, prep)
    got = R.ssim_grad_ref(out, tgt, prep)
    assert got.shape == want.shape == tuple(shape) and got.dtype == torch.float64
    err = R.rel_max(got, want)
    print(f"{shape} prep={prep}: closed form against float64 autograd {err:.2e}")
    assert err <= 1e-12
    assert R.rel_max(R.ssim_grad_ref(out, tgt, prep, scale=0.25), 0.25 * want) <= 1e-12


def test_closed_form_on_flat_input():
    out, tgt = R.make_flat_inputs(12)
    assert R.rel_max(R.ssim_grad_ref(out, tgt), R.ssim_grad_autograd(out, tgt)) <= 1e-12


def test_dropped_rows_and_columns_get_exact_zeros():
    out, tgt = R.make_inputs((1, 2, 385, 391), 13)
    for g in (R.ssim_grad_ref(out, tgt), R.ssim_grad_autograd(out, tgt)):
        assert not g[:, :, 384:, :].any() and not g[:, :, :, 390:].any()
        assert g[:, 0, :384, :390].ne(0).all()


def test_clamp_bounds_with_planted_values():
    """torch.clamp's backward passes the gradient ON the bounds (0.0 and 1.0 exactly) and none outside, not even one ulp outside; the
    twin agrees, with exact zeros."""
    out, tgt = R.make_inputs((1, 2, 20, 20), 14)
    out[:, 1].clamp_(0.05, 0.95)                                                 # then plant: every other value is inside
    planted = {(5, 5): 0.0, (5, 9): 1.0, (9, 5): float(torch.nextafter(torch.tensor(0.0), torch.tensor(-1.0))), (9, 9): float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0))),
               (12, 4): -0.3, (12, 12): 1.7, (3, 14): -0.0}
    for (r, c), v in planted.items():
        out[0, 1, r, c] = v
    assert float(out[0, 1, 9, 5]) < 0 and float(out[0, 1, 9, 9]) > 1               # (float32 holds both neighbours)
    want = R.ssim_grad_autograd(out, tgt)
    got = R.ssim_grad_ref(out, tgt)
    assert R.rel_max(got, want) <= 1e-12
    w32 = R.ssim_grad_autograd(out, tgt, dtype=torch.float32)
    for g in (want, got, w32):
        for (r, c), v in planted.items():
            inside = 0.0 <= v <= 1.0
            assert (float(g[0, 1, r, c]) != 0.0) == inside, (r, c, v, float(g[0, 1, r, c]))
        assert int((g[0, 1] == 0).sum()) == 4
    assert got[0, 1, 9, 5].item() == 0.0 and math.copysign(1.0, got[0, 1, 9, 5].item()) == 1.0


def test_header_declares_and_binding_mirrors_the_entry_point():
    from mau_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+mau_ssim_loss_grad\s*\(([^)]*)\)", txt)
    assert m, "include/mau_hip.h does not declare mau_ssim_loss_grad"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* out", "const float* tgt", "float* dout", "float scale", "int prep", "int B", "int C", "int H", "int W",
                      "mau_stream_t stream"]
    assert hasattr(_lib.lib, "mau_ssim_loss_grad")
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["mau_ssim_loss_grad"] == (i, [vp, vp, vp, f, i, i, i, i, i, vp])
    assert _lib.lib.mau_abi_version() == 5                                 # additive: the version does not move


def test_refusals_need_no_device():
    from mau_amd import _lib
    lib = _lib.lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = [p, p, p, 1.0, 1, 1, 2, 32, 32, None]
    for change, word in (({0: None}, b"bad arguments"), ({1: None}, b"bad arguments"), ({2: None}, b"bad arguments"),
                         ({5: 0}, b"bad arguments"), ({6: 0}, b"bad arguments"),
                         ({7: 8, 8: 8}, b"smaller than the 11x11 window"), ({7: 10}, b"smaller than the 11x11 window"),
                         ({8: 10}, b"smaller than the 11x11 window"),
                         ({5: 32768, 6: 2}, b"must fit a grid dimension"), ({5: 65536, 6: 1}, b"must fit a grid dimension")):
        args = list(good)
        for k, v in change.items():
            args[k] = v
        status = lib.mau_ssim_loss_grad(*args)
        msg = lib.mau_last_error()
        assert status == 1 and msg.startswith(b"ssim_loss_grad:") and word in msg, (change, status, msg)        # MAU_ERR_ARG
    if not torch.cuda.is_available():
        # nothing to launch on: an error code and a message, no crash (the host buffers are never dereferenced)
        status = lib.mau_ssim_loss_grad(*good)
        assert status != 0 and lib.mau_last_error().startswith(b"ssim_grad_kernel")


def test_criterion_is_exported_and_refuses_cpu_tensors():
    import mau_amd
    from mau_amd import losses, train
    assert "compute_loss_l1_grad_ssim_trained" in mau_amd.__all__
    assert mau_amd.compute_loss_l1_grad_ssim_trained is losses.compute_loss_l1_grad_ssim_trained is train.compute_loss_l1_grad_ssim_trained
    assert mau_amd.compute_loss_l1_grad_ssim_trained is not mau_amd.compute_loss_l1_grad_ssim
    with pytest.raises(RuntimeError, match="no CPU"):
        mau_amd.compute_loss_l1_grad_ssim_trained(torch.zeros(1, 2, 16, 16, requires_grad=True), torch.zeros(1, 2, 16, 16))


def test_ssim_gradient_with_another_loss_is_refused_before_the_device(monkeypatch):
    from mau_amd import train
    from mau_amd.config import CONFIG
    for loss in ("mse", "mse-gradient"):
        monkeypatch.setitem(CONFIG.training, "loss", loss)
        with pytest.raises(ValueError, match="ssim-gradient"):
            train.run(device="gpu", model_type="unet", temporal_embeddings=False, ssim_gradient=True)
