"""Shared helpers for the test-suite (fixture loading, error metrics, the recorder of ``functional.call``)."""
import contextlib
import ctypes
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def t(a):
    return torch.from_numpy(np.array(a, copy=True))


def sub(d, prefix):
    """{'sd0/foo': x} -> {'foo': tensor}"""
    p = prefix + "/"
    return {k[len(p):]: t(v) for k, v in d.items() if k.startswith(p)}


def meta_of(d):
    return json.loads(bytes(d["meta"]).decode())


def rel_err(a, b):
    """max |a-b| / max(|b|) -- the 'relative fp32 tolerance' of the north star, scale-normalised."""
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    denom = b.abs().max().clamp_min(1e-30)
    return float((a - b).abs().max() / denom)


def rel_l2(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def ssim_value_torch(x, y, data_range=1.0, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The same quantity spelled with torch ops (the checker of the HIP kernel in tests/): per-image SSIM averaged over
    channels (piq.ssim defaults, reduction='none')."""
    with torch.no_grad():
        x, y = x / data_range, y / data_range
        f = max(1, round(min(x.shape[-2:]) / 256))
        if f > 1:
            x, y = torch.nn.functional.avg_pool2d(x, f), torch.nn.functional.avg_pool2d(y, f)
        c = torch.arange(kernel_size, dtype=x.dtype, device=x.device) - (kernel_size - 1) / 2.0
        g1 = torch.exp(-(c ** 2) / (2 * sigma ** 2))
        k = (g1[:, None] * g1[None, :])
        k = (k / k.sum())[None, None].repeat(x.shape[1], 1, 1, 1)
        C = x.shape[1]
        mu_x, mu_y = torch.nn.functional.conv2d(x, k, groups=C), torch.nn.functional.conv2d(y, k, groups=C)
        sxx = torch.nn.functional.conv2d(x * x, k, groups=C) - mu_x ** 2
        syy = torch.nn.functional.conv2d(y * y, k, groups=C) - mu_y ** 2
        sxy = torch.nn.functional.conv2d(x * y, k, groups=C) - mu_x * mu_y
        c1, c2 = k1 ** 2, k2 ** 2
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        ss = (2 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1) * cs
        return ss.mean(dim=(-1, -2)).mean(dim=1)


# --------------------------------------------------------------------------- #
# the recorder of the launch traces (tests/test_gpu_launch_trace.py, tests/test_gpu_session_trace.py)
# --------------------------------------------------------------------------- #
HOST_ONLY = ("mau_conv3x3_pack_desc_fill",)           # fills a host table: its last argument is no stream
_FLOATS = (ctypes.c_float, ctypes.c_double)


@contextlib.contextmanager
def patched(mod, **attrs):
    old = {k: getattr(mod, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(mod, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


def encode(prototypes, name, args, main):
    """One call as ``[name, args...]``: a scalar verbatim (a float as ``float.hex``), a pointer as 0 / 1 (null or not), the trailing
    stream as "main" (the handle ``main``) or "side"."""
    argtypes = prototypes[name][1]
    assert len(args) == len(argtypes), (name, len(args), len(argtypes))
    row = [name]
    last = len(args) - 1
    for i, (a, ty) in enumerate(zip(args, argtypes)):
        if ty is ctypes.c_void_p:
            if i == last and name not in HOST_ONLY:
                row.append("main" if (a or 0) == main else "side")
            else:
                row.append(1 if a else 0)
        elif ty in _FLOATS:
            row.append(float(a).hex())
        else:
            row.append(int(a))
    return row


@contextlib.contextmanager
def recorded_calls(mau, modules=()):
    """Yields the list that every call through ``functional.call`` is appended to, encoded, while the block runs; the real call
    still runs.  "main" is the stream current on entry.  A module that bound ``call`` by name (``from .functional import call``)
    holds its own reference: name it in ``modules`` and it is patched too."""
    from mau_amd import functional as F_
    rows = []
    main = torch.cuda.current_stream().cuda_stream
    real = F_.call

    def spy(name, *args):
        rows.append(encode(mau._lib.PROTOTYPES, name, args, main))
        return real(name, *args)

    with contextlib.ExitStack() as stack:
        for mod in (F_, *modules):
            stack.enter_context(patched(mod, call=spy))
        yield rows


def first_difference(got, want, label):
    """None when two recorded traces agree call for call, else a message that shows the first call that differs."""
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"{label}: call {i} differs\n   now: {a}\n  then: {b}\n  (before it: {got[max(0, i - 3):i]})"
    n = min(len(got), len(want))
    if len(got) != len(want):
        return f"{label}: {len(got)} calls now, {len(want)} recorded; the first one more: {(got[n:] + want[n:])[0]}"
    return None
