"""Host side of the first layer's fused dz route: the default threshold lies above every size of tests/golden/launch_trace.json, and the
new entry is declared, bound and exported with one signature."""
import ctypes

from tests._helpers import header_prototypes


def test_default_threshold_is_above_the_traced_sizes():
    """tests/test_gpu_launch_trace.py records N = 2 at up to 64 x 64 pixels with the hooks it pins; _FIRST_DZ_FUSED_MIN_WORK is not one
    of them, so those cases run at the default: it must keep them on the recorded route."""
    import mau_amd  # noqa: F401
    from mau_amd import functional as F_
    assert isinstance(F_._FIRST_DZ_FUSED_MIN_WORK, int)
    assert F_._FIRST_DZ_FUSED_MIN_WORK > 2 * 64 * 64


def test_entry_is_declared_bound_and_exported():
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    name = "mau_conv3x3_first_wgrad_bn"
    ret, args = header_prototypes()[name]
    assert (ret, list(args)) == (_lib.PROTOTYPES[name][0], list(_lib.PROTOTYPES[name][1]))
    assert len(args) == 20 and args[10] is ctypes.c_double and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # refused without touching a device: more than 8 input channels, a pitch below the padded channel count, no workspace
    p = ctypes.c_void_p(4096)
    call = lambda ldda, ws, Cin: _lib.lib.mau_conv3x3_first_wgrad_bn(p, p, ldda, p, 64, p, p, p, p, p, 128.0, p, ws, Cin, 64, _lib.MAU_BF16, 1, 4, 4, None)  # noqa: E731
    assert call(64, p, 9) != 0 and call(56, p, 6) != 0 and call(64, None, 6) != 0
