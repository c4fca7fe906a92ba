"""Host-only: every dispatch decision of the 16-bit 3x3 convolution and its weight gradient equals the recorded one.

``tests/golden/dispatch_decisions.json`` was recorded (``tests/golden/make_dispatch_golden.py``) from the library BEFORE the size
queries and the launchers were rebuilt on one launch plan: the tile variant, K groups and statistics-slab rows of the forward /
data-gradient launch over the grid of ``test_slab_query_matches_launch_geometry_sweep``, and the split count and workspace size of
the weight gradient.  The sweeps have hundreds of thousands of rows, so the file keeps one SHA-256 per group over the text encoding
below, and in readable form the rows of the layers the networks actually run (to diagnose a mismatch).

Without a device the library assumes the MI355X shape (256 CUs, 8 XCDs), so the same file holds on a host without a GPU and on
the GPU machine."""
import ctypes
import hashlib
import itertools
import json
import os

from tests.test_dispatch_geometry_host import BROKEN, CINS, COUTS, HEIGHTS, UNET_B32_VARIANTS, WIDTHS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_decisions.json")

DTYPES = ("bf16", "f16")
CONV_NS = list(range(1, 34))
WGRAD_NS = [1, 2, 8, 16, 32]
WGRAD_CINS = [8, 64, 192, 256, 576, 1536]


def _code(_lib, dtype):
    return _lib.MAU_BF16 if dtype == "bf16" else _lib.MAU_F16


def conv_sweep_digest(_lib, dtype):
    """one line per (N, H, W, Cout): 'N H W Cout rows' + ' th,nw,bn,kg' per Cin of CINS"""
    code, fn, rows_fn = _code(_lib, dtype), _lib.lib.mau_conv3x3_variant, _lib.lib.mau_conv3x3_num_pixel_tiles
    th, nw, bn, kg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(th), ctypes.byref(nw), ctypes.byref(bn), ctypes.byref(kg))
    h, n = hashlib.sha256(), 0
    for N, H, W, Cout in itertools.product(CONV_NS, HEIGHTS, WIDTHS, COUTS):
        line = [f"{N} {H} {W} {Cout} {rows_fn(code, N, H, W, Cout)}"]
        for Cin in CINS:
            assert fn(code, N, H, W, Cin, Cout, *out) == 0
            line.append(f"{th.value},{nw.value},{bn.value},{kg.value}")
            n += 1
        h.update((" ".join(line) + "\n").encode())
    return h.hexdigest(), n


def wgrad_sweep_digest(_lib, dtype):
    """one line per (N, H, W, Cout, Cin): 'N H W Cout Cin splits acc_elems'"""
    code, sp, el = _code(_lib, dtype), _lib.lib.mau_conv3x3_wgrad_splits, _lib.lib.mau_conv3x3_wgrad_acc_elems
    h, n = hashlib.sha256(), 0
    for N, H, W, Cout, Cin in itertools.product(WGRAD_NS, HEIGHTS, WIDTHS, COUTS, WGRAD_CINS):
        h.update(f"{N} {H} {W} {Cout} {Cin} {sp(code, N, H, W, Cout, Cin)} {el(code, N, H, W, Cout, Cin)}\n".encode())
        n += 1
    return h.hexdigest(), n


def named_layers():
    """(group, N, H, W, Cin, Cout) of the rows kept readable: the U-Net's 13 layer shapes at B = 32, 256 x 256; the six shapes of the
    slab overrun (256 -> 64); the same 13 layers in single-tile inference (N = 1, 512 x 512 input, levels 0-4)"""
    rows = [("unet_b32", 32, H, H, Cin, Cout) for Cin, Cout, H, _ in UNET_B32_VARIANTS]
    rows += [("broken", N, H, W, 256, 64) for (N, H, W), _, _ in BROKEN]
    rows += [("infer512_b1", 1, 2 * H, 2 * H, Cin, Cout) for Cin, Cout, H, _ in UNET_B32_VARIANTS]
    return rows


def named_rows(_lib, dtype):
    code, out = _code(_lib, dtype), []
    for group, N, H, W, Cin, Cout in named_layers():
        out.append({"group": group, "N": N, "H": H, "W": W, "Cin": Cin, "Cout": Cout,
                    "variant": list(_lib.conv3x3_variant(code, N, H, W, Cout, Cin=Cin)),
                    "slab_rows": _lib.lib.mau_conv3x3_num_pixel_tiles(code, N, H, W, Cout),
                    "wgrad_splits": _lib.lib.mau_conv3x3_wgrad_splits(code, N, H, W, Cout, Cin),
                    "wgrad_acc_elems": _lib.lib.mau_conv3x3_wgrad_acc_elems(code, N, H, W, Cout, Cin)})
    return out


def record(_lib):
    doc = {"grid": {"conv_N": [CONV_NS[0], CONV_NS[-1]], "heights": HEIGHTS, "widths": WIDTHS, "couts": COUTS, "conv_cins": CINS,
                    "wgrad_N": WGRAD_NS, "wgrad_cins": WGRAD_CINS},
           "sha256": {}, "count": {}, "rows": {}}
    for dtype in DTYPES:
        doc["sha256"][f"conv/{dtype}"], doc["count"][f"conv/{dtype}"] = conv_sweep_digest(_lib, dtype)
        doc["sha256"][f"wgrad/{dtype}"], doc["count"][f"wgrad/{dtype}"] = wgrad_sweep_digest(_lib, dtype)
        doc["rows"][dtype] = named_rows(_lib, dtype)
    return doc


def test_dispatch_decisions_equal_the_recorded_ones():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record(_lib)
    assert got["grid"] == want["grid"], "the fixture was recorded over another grid"
    assert len(named_layers()) == 13 + 6 + 13
    # the readable rows first: a mismatch names the layer and the field
    for dtype in DTYPES:
        for g, w in zip(got["rows"][dtype], want["rows"][dtype]):
            assert g == w, (dtype, f"now {g}", f"recorded {w}")
        assert len(got["rows"][dtype]) == len(want["rows"][dtype]) == 32
    assert got["count"] == want["count"]
    n_conv = len(CONV_NS) * len(HEIGHTS) * len(WIDTHS) * len(COUTS) * len(CINS)
    n_wgrad = len(WGRAD_NS) * len(HEIGHTS) * len(WIDTHS) * len(COUTS) * len(WGRAD_CINS)
    assert got["count"] == {"conv/bf16": n_conv, "wgrad/bf16": n_wgrad, "conv/f16": n_conv, "wgrad/f16": n_wgrad}
    assert got["sha256"] == want["sha256"]
