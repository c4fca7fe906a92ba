"""CPU-only checks of the optimizer family (``mau_amd.SGD`` / ``Adam`` / ``AdamW``, ``mau_opt_pack_step``, ``mau_grad_norm_clip``):
constructor validation, the new symbols in header, binding and library, and the host-side argument checks of the two entry points
(no device is touched: a refused call returns before any launch)."""
import ctypes
import os
import re

import pytest
import torch

from tests._helpers import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mau_opt_pack_desc_fill", "mau_opt_pack_step", "mau_grad_norm_chunk", "mau_grad_norm_seg_bytes", "mau_grad_norm_seg_fill",
       "mau_grad_norm_clip"]


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 4, 3, 3)), torch.nn.Parameter(torch.zeros(4))]


def test_constructor_arguments_are_validated():
    import mau_amd
    # what the fused kernel does not implement is refused at construction: never a silent fallback
    with pytest.raises(ValueError, match="dampening"):
        mau_amd.SGD(_params(), lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="maximize"):
        mau_amd.SGD(_params(), lr=0.1, maximize=True)
    with pytest.raises(ValueError, match="Nesterov"):
        mau_amd.SGD(_params(), lr=0.1, momentum=0.0, nesterov=True)
    for cls in (mau_amd.Adam, mau_amd.AdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls(_params(), lr=1e-3, amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls(_params(), lr=1e-3, maximize=True)
        for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1e-2),
                    dict(max_grad_norm=-1.0)):
            with pytest.raises(ValueError):
                cls(_params(), **bad)
    for bad in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-2), dict(lr=0.1, max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            mau_amd.SGD(_params(), **bad)
    # torch's defaults and group layout (the state_dict's param_groups carry no option torch does not know)
    sgd = mau_amd.SGD(_params(), lr=0.1, momentum=0.9, nesterov=True, max_grad_norm=2.0)
    assert {k: v for k, v in sgd.param_groups[0].items() if k != "params"} == dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True)
    adam = mau_amd.Adam(_params())
    assert {k: v for k, v in adam.param_groups[0].items() if k != "params"} == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    assert mau_amd.AdamW(_params()).param_groups[0]["weight_decay"] == 1e-2
    assert sgd.max_grad_norm == 2.0 and adam.max_grad_norm == 0.0 and adam.last_grad_norm is None
    assert "max_grad_norm" not in sgd.state_dict()["param_groups"][0]
    # a step without gradients is a no-op on any device
    sgd.step()
    adam.step()


def test_new_symbols_in_header_binding_and_library():
    from mau_amd import _lib
    syms = header_symbols()
    for name in NEW:
        assert name in syms, f"{name} is not declared in include/mau_hip.h"
        assert name in _lib.PROTOTYPES, f"{name} has no binding"
    if os.path.exists(_lib.LIB_PATH):
        so = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW:
            assert hasattr(so, name), f"libmau_hip.so does not export {name}"
    assert _lib.lib.mau_abi_version() == 5                                  # additive: the ABI version stays
    assert (_lib.MAU_OPT_ADAMW, _lib.MAU_OPT_ADAM, _lib.MAU_OPT_SGD) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    for k, v in (("MAU_OPT_ADAMW", 0), ("MAU_OPT_ADAM", 1), ("MAU_OPT_SGD", 2)):
        assert re.search(rf"#define {k} {v}\b", hdr), k


def _refused(status):
    from mau_amd import _lib
    msg = _lib.lib.mau_last_error()
    assert status == 1 and msg, (status, msg)          # MAU_ERR_ARG
    return msg.decode()


def test_entry_points_refuse_bad_arguments_on_the_host():
    from mau_amd import _lib
    lib = _lib.lib
    one = ctypes.create_string_buffer(64)                # any non-NULL address: a refused call never reads it
    a = ctypes.addressof(one)
    step = lambda descs, n, tiles, rule, stp, b1=0.9, b2=0.999, nesterov=0: lib.mau_opt_pack_step(       # noqa: E731
        descs, n, tiles, _lib.MAU_F32, rule, stp, None, 1e-3, b1, b2, 1e-8, 0.0, nesterov, None)
    assert "opt_pack_step" in _refused(step(None, 1, 1, _lib.MAU_OPT_SGD, None))                  # NULL table
    assert "opt_pack_step" in _refused(step(a, 0, 1, _lib.MAU_OPT_SGD, None))                     # no rows
    assert "opt_pack_step" in _refused(step(a, 1, 0, _lib.MAU_OPT_SGD, None))                     # no tiles
    assert "opt_pack_step" in _refused(step(a, -3, -1, _lib.MAU_OPT_ADAM, a))
    assert "rule" in _refused(step(a, 1, 1, 7, a))                                                # unknown rule
    assert "step count" in _refused(step(a, 1, 1, _lib.MAU_OPT_ADAM, None))                       # Adam without a device step count
    assert "step count" in _refused(step(a, 1, 1, _lib.MAU_OPT_ADAMW, a, b1=1.0))                 # beta1 out of range
    assert "nesterov" in _refused(step(a, 1, 1, _lib.MAU_OPT_SGD, None, b1=0.0, nesterov=1))      # Nesterov without momentum
    assert "adamw_pack_step" in _refused(lib.mau_adamw_pack_step(a, 1, 1, _lib.MAU_F32, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None))
    nxt = ctypes.c_int(0)
    assert "opt_pack_desc_fill" in _refused(lib.mau_opt_pack_desc_fill(None, 0, a, a, None, None, None, None, 4, 4, 0, ctypes.addressof(nxt)))
    assert "opt_pack_desc_fill" in _refused(lib.mau_opt_pack_desc_fill(a, 0, a, None, None, None, None, None, 4, 4, 0, ctypes.addressof(nxt)))
    assert "adamw_pack_desc_fill" in _refused(lib.mau_adamw_pack_desc_fill(a, 0, a, a, a, None, None, None, 4, 4, 0, ctypes.addressof(nxt)))
    # a row without moments is what the new fill is for; the row layout and the tile count are those of the AdamW fill
    row = ctypes.create_string_buffer(lib.mau_adamw_pack_desc_bytes())
    row2 = ctypes.create_string_buffer(lib.mau_adamw_pack_desc_bytes())
    assert lib.mau_opt_pack_desc_fill(ctypes.addressof(row), 0, a, a, None, None, None, None, 70, 130, 5, ctypes.addressof(nxt)) == 0
    assert nxt.value == 5 + 2 * 3
    assert lib.mau_opt_pack_desc_fill(ctypes.addressof(row), 0, a, a, a, a, None, None, 70, 130, 5, ctypes.addressof(nxt)) == 0
    assert lib.mau_adamw_pack_desc_fill(ctypes.addressof(row2), 0, a, a, a, a, None, None, 70, 130, 5, ctypes.addressof(nxt)) == 0
    assert row.raw == row2.raw

    clip = lambda segs, nsegs, blocks, ws=a, tk=a, mx=1.0, no=a, co=a: lib.mau_grad_norm_clip(segs, nsegs, blocks, ws, tk, mx, no, co, None)   # noqa: E731
    assert "grad_norm_clip" in _refused(clip(None, 1, 1))                                         # NULL table
    assert "grad_norm_clip" in _refused(clip(a, 0, 1))                                            # no segments
    assert "grad_norm_clip" in _refused(clip(a, 1, 0))                                            # no blocks
    assert "grad_norm_clip" in _refused(clip(a, 3, 2))                                            # fewer blocks than segments
    assert "grad_norm_clip" in _refused(clip(a, 1, 1, ws=None))
    assert "grad_norm_clip" in _refused(clip(a, 1, 1, tk=None))
    assert "grad_norm_clip" in _refused(clip(a, 1, 1, mx=0.0))
    assert "grad_norm_clip" in _refused(clip(a, 1, 1, no=None))
    chunk = lib.mau_grad_norm_chunk()
    assert chunk > 0 and chunk % 4 == 0
    seg = ctypes.create_string_buffer(lib.mau_grad_norm_seg_bytes() * 2)
    assert "grad_norm_seg_fill" in _refused(lib.mau_grad_norm_seg_fill(None, 0, a, 5, 0, ctypes.addressof(nxt)))
    assert "grad_norm_seg_fill" in _refused(lib.mau_grad_norm_seg_fill(ctypes.addressof(seg), 0, None, 5, 0, ctypes.addressof(nxt)))
    assert "grad_norm_seg_fill" in _refused(lib.mau_grad_norm_seg_fill(ctypes.addressof(seg), 0, a, 0, 0, ctypes.addressof(nxt)))
    assert "grad_norm_seg_fill" in _refused(lib.mau_grad_norm_seg_fill(ctypes.addressof(seg), 0, a + 2, 5, 0, ctypes.addressof(nxt)))   # not a float address
    assert lib.mau_grad_norm_seg_fill(ctypes.addressof(seg), 0, a, 1, 0, ctypes.addressof(nxt)) == 0 and nxt.value == 1
    assert lib.mau_grad_norm_seg_fill(ctypes.addressof(seg), 1, a, 2 * chunk + 1, nxt.value, ctypes.addressof(nxt)) == 0 and nxt.value == 4
