"""Shared helpers for the test-suite: the fixtures every GPU module needs, fixture loading, error metrics, bit-pattern comparison, the
parser of include/mau_hip.h, and the recorder of ``functional.call``.  A test module imports the fixtures by name
(``from tests._helpers import mau  # noqa: F401``): pytest collects a fixture that sits in the module's namespace."""
import contextlib
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------- #
# fixtures and small helpers of the GPU modules
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def mau():
    """The package, for a test that runs on the device: no device, or one the library refuses, is a failure and never a skip."""
    import mau_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mau_amd import _lib
    _lib.check(_lib.lib.mau_device_check(), "mau_device_check")
    return mau_amd


@pytest.fixture(scope="module")
def palette():
    from tests.test_scenario_host import load_palette
    return load_palette()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from mau_amd._lib import call
    call(name, *args)


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
# bit patterns
# --------------------------------------------------------------------------- #
def bits(x):
    """The elements of a numpy array or a torch tensor as integers of their own width."""
    if isinstance(x, torch.Tensor):
        return x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(got, want, nan_matches_nan=False):
    """True when two arrays or tensors have one shape, one type and the same bit pattern in every element.  A NaN's sign and payload
    are not values: ``nan_matches_nan`` is for a comparison with a host reference, where any NaN matches any NaN; between two results
    of the device they are compared like every other bit.  What differs is printed: the first indices and the values there."""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        print("bits differ:", tuple(got.shape), got.dtype, "against", tuple(want.shape), want.dtype)
        return False
    differ = bits(got) != bits(want)
    if nan_matches_nan:
        differ &= ~(torch.isnan(got) & torch.isnan(want))
    if differ.any():
        print("bits differ at", differ.nonzero()[:8].tolist(), got[differ][:8].tolist(), "against", want[differ][:8].tolist(),
              "patterns", [hex(v) for v in bits(got)[differ][:8].tolist()], "against", [hex(v) for v in bits(want)[differ][:8].tolist()])
        return False
    return True


def _float32(a):
    return torch.as_tensor(a).detach().float()


def _bits_equal(a, b):
    """``same_bits`` of the float32 values (bf16 and fp16 widen exactly)"""
    return same_bits(_float32(a), _float32(b))


def _nbits_differ(a, b):
    return int((bits(_float32(a)) != bits(_float32(b))).sum())


# --------------------------------------------------------------------------- #
# the sentinel buffer of the C-ABI kernel tests (tests/test_gpu_spatial.py, tests/test_gpu_bn_head.py)
# --------------------------------------------------------------------------- #
NAN = float("nan")
SLACK = 3                                                     # pixels of sentinel in front of and behind every tensor


def pad8(c):
    return (c + 7) // 8 * 8


class Buf:
    """(npix, ld) tensor of ``dt`` with SLACK sentinel pixels at both ends, staged on the CPU, NaN everywhere until written"""

    def __init__(self, npix, ld, dt, fill=NAN):
        self.npix, self.ld, self.dt = npix, ld, dt
        self.host = torch.full((npix + 2 * SLACK, ld), fill, dtype=dt)
        self.dev = None

    @property
    def body(self):
        return self.host[SLACK:SLACK + self.npix]

    def put(self, x_nchw, choff=0):
        """channels [choff, choff + C) <- x (N, C, H, W), pad lanes up to the next multiple of 8 <- 0"""
        N, C, H, W = x_nchw.shape
        v = self.body.view(N, H, W, self.ld)
        v[..., choff:choff + C] = x_nchw.permute(0, 2, 3, 1).to(self.dt)
        v[..., choff + C:choff + pad8(C)] = 0
        return self

    def cuda(self):
        self.dev = self.host.cuda()
        return self

    @property
    def ptr(self):
        if self.dev is None:
            self.cuda()
        return self.dev.data_ptr() + SLACK * self.ld * self.dev.element_size()

    def back(self):
        """the tensor's pixels after the call; the sentinel pixels must be untouched"""
        torch.cuda.synchronize()
        r = self.dev.cpu()
        assert bool(torch.isnan(r[:SLACK].float()).all()) and bool(torch.isnan(r[SLACK + self.npix:].float()).all()), "pixels outside the tensor were written"
        return r[SLACK:SLACK + self.npix]

    def get(self, shape, choff=0):
        """(N, C, H, W) float32 of channels [choff, choff + C); every channel outside [choff, choff + C8) still NaN, pad lanes 0"""
        N, C, H, W = shape
        b = self.back().view(N, H, W, self.ld).float()
        C8 = pad8(C)
        assert bool(torch.isnan(b[..., :choff]).all()) and bool(torch.isnan(b[..., choff + C8:]).all()), "channels outside [choff, choff + C8) were written"
        assert bool((b[..., choff + C:choff + C8] == 0).all()), "pad lanes are not 0"
        return b[..., choff:choff + C].permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- #
# include/mau_hip.h as the bindings must see it
# --------------------------------------------------------------------------- #
# the ctypes type of a C type; any pointer is c_void_p, but the ``const char*`` a function RETURNS is c_char_p
CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "mau_stream_t": ctypes.c_void_p}


def _header_text():
    with open(os.path.join(ROOT, "include", "mau_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_symbols():
    """Every ``mau_*`` name followed by a parenthesis: what ``header_prototypes`` must have read, found without reading a prototype."""
    return sorted(set(re.findall(r"\b(mau_[a-z0-9_]+)\s*\(", _header_text())))


def header_prototypes():
    """{name: (return type, [argument types])} of every function declared in include/mau_hip.h, as the ctypes types of ``CTYPES``.
    A type the table does not hold fails by name."""
    txt = re.sub(r"//[^\n]*", "", _header_text())
    txt = re.sub(r"^\s*#[^\n]*$", "", txt, flags=re.M)                 # (comments are gone: no #define continues on another line)

    def kind(decl, what, is_return=False):
        words = decl.replace("*", " * ").split()
        if "*" in words:
            if is_return:
                assert words == ["const", "char", "*"], (what, decl)
                return ctypes.c_char_p
            return ctypes.c_void_p
        words = [w for w in words if w != "const"]
        if not is_return:
            assert len(words) == 2, f"{what}: cannot read the parameter {decl!r}"       # type + name
            words = words[:1]
        assert len(words) == 1, (what, decl)
        assert words[0] in CTYPES, f"{what}: no ctypes type for {decl!r}"
        return CTYPES[words[0]]

    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(mau_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        assert name not in protos, name
        params = [] if args == "void" else [a.strip() for a in args.split(",")]
        protos[name] = (kind(ret, name, True), [kind(a, name) for a in params])
    return protos


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
