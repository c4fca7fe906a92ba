"""CPU-only checks around ``mau_loss_terms`` (every term of compute_all_loss in one launch) and the dataset mode of the training
driver: the ABI rows, the size helper and the refusals without a GPU, ``RunningLoss`` against hand-computed sequences, and the
driver's argument checks that must come before anything touches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_mirrors_the_entry_points():
    from mau_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mau_loss_terms_ws_elems", "mau_loss_terms"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib, name)
    assert _lib.PROTOTYPES["mau_loss_terms_ws_elems"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    ret, args = _lib.PROTOTYPES["mau_loss_terms"]
    assert ret is ctypes.c_int and len(args) == 14
    assert args[:7] == [ctypes.c_void_p] * 7 and args[7:9] == [ctypes.c_float] * 2 and args[9:13] == [ctypes.c_int] * 4
    assert args[13] is ctypes.c_void_p
    assert _lib.lib.mau_abi_version() == 5                                 # additive: the version does not move


def test_ws_elems_without_a_gpu():
    from mau_amd import _lib
    ws = _lib.lib.mau_loss_terms_ws_elems
    sizes = [ws(b, 2, 250, 250) for b in (1, 2, 3, 16)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))                    # strictly monotone in B
    assert sizes[1] == 2 * sizes[0]
    # five fp64 partials per 16x16 tile of the (H/f - 10) x (W/f - 10) SSIM map of every (image, channel) plane
    assert ws(1, 2, 250, 250) == 5 * 2 * 15 * 15
    assert ws(3, 2, 11, 11) == 5 * 3 * 2 and ws(3, 2, 37, 29) == 5 * 3 * 2 * 2 * 2 and ws(3, 2, 26, 42) == 5 * 3 * 2 * 1 * 2
    assert ws(1, 2, 387, 389) == 5 * 2 * 12 * 12                           # f = 2: 193 x 194 pooled, 183 x 184 windows
    assert ws(3, 2, 10, 40) == 0 and ws(0, 2, 64, 64) == 0 and ws(1, 2, 0, 64) == 0


def test_refusals_and_a_call_without_a_device():
    import torch
    from mau_amd import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = [p, p, p, p, p, p, None, 0.1, 0.5, 3, 2, 40, 40, None]
    for change, word in (({0: None}, b"null"), ({1: None}, b"null"), ({2: None}, b"null"), ({3: None}, b"null"), ({4: None}, b"null"),
                         ({5: None}, b"null"), ({9: 0}, b"dimension"), ({11: -1}, b"dimension"), ({10: 3}, b"C must be 2"),
                         ({10: 1}, b"C must be 2"), ({11: 10}, b"smaller than the 11x11 window"), ({12: 9}, b"smaller than the 11x11 window")):
        args = list(good)
        for i, v in change.items():
            args[i] = v
        status = lib.mau_loss_terms(*args)
        msg = lib.mau_last_error()
        assert status == 1 and msg.startswith(b"loss_terms") and word in msg, (change, status, msg)        # MAU_ERR_ARG
    if not torch.cuda.is_available():
        # nothing to launch on: an error code and a message, no crash (the host buffers are never dereferenced)
        status = lib.mau_loss_terms(*good)
        assert status != 0 and lib.mau_last_error().startswith(b"loss_terms_kernel")


def test_compute_all_loss_refuses_cpu_tensors_and_is_exported():
    import torch
    import mau_amd
    assert "compute_all_loss" in mau_amd.__all__
    with pytest.raises(RuntimeError, match="no CPU"):
        mau_amd.compute_all_loss(torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16))


def test_running_loss_modes_against_hand_computed_sequences():
    from mau_amd.metrics import RunningLoss
    cum = RunningLoss(mode="cumulative")
    assert cum.get() == 0.0
    assert cum.update(2.0, n=2) == pytest.approx(2.0, rel=1e-9)                       # 4 / 2
    assert cum.update(5.0, n=1) == pytest.approx(3.0, rel=1e-9)                       # 9 / 3
    assert cum.update(1.0, n=3) == pytest.approx(2.0, rel=1e-9) == cum.get()          # 12 / 6
    ema = RunningLoss(mode="ema", ema_alpha=0.5)
    assert ema.get() is None
    assert ema.update(4.0) == 4.0                                                     # seeded with the first value
    assert ema.update(2.0) == 3.0 and ema.update(1.0) == 2.0 and ema.get() == 2.0
    ema98 = RunningLoss(mode="ema")
    ema98.update(1.0)
    assert ema98.update(0.0) == pytest.approx(0.98, rel=1e-12)
    sma = RunningLoss(mode="sma", window_size=3)
    assert sma.update(3.0) == pytest.approx(3.0, rel=1e-9)
    assert sma.update(6.0) == pytest.approx(4.5, rel=1e-9)
    assert sma.update(9.0) == pytest.approx(6.0, rel=1e-9)
    assert sma.update(12.0) == pytest.approx(9.0, rel=1e-9) == sma.get()              # 3.0 left the window
    assert sma.update(0.0, n=2) == pytest.approx(4.0, rel=1e-9)                       # window 12, 0, 0
    sma.reset()
    assert sma.get() == 0.0 and sma.update(7.0) == pytest.approx(7.0, rel=1e-9)
    with pytest.raises(ValueError):
        RunningLoss(mode="median")


def test_dataset_mode_checks_come_before_the_device(tmp_path):
    import typer
    from mau_amd import train
    (tmp_path / "train").mkdir()
    with pytest.raises(typer.BadParameter):                                # still the MI355X-native path only
        train.run(device="cpu", processed_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError, match="val"):                    # train/ exists, val/ does not
        train.run(device="gpu", processed_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError, match="train"):
        train.run(device="gpu", processed_dir=str(tmp_path / "nowhere"))
