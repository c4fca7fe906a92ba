"""The chunked fp64 reductions (csrc/chunk_reduce.h) at the C ABI against the order-exact host references of tests/reduce_ref.py:
equality of the 64-bit patterns.  The shapes are the smallest at which the shared code takes another path: one pixel, one full
chunk (16-byte loads), a last chunk of one pixel (scalar loads) and of one quad, the 250 x 250 tile (16 chunks, the last partial),
more rows than tickets (two launches reuse the workspace) and a base one float off a 16-byte boundary (scalar loads at a size
that is eligible for 16-byte ones).  The entries that pass through an fp64 division or square root (MAE, RMSE, the Laplacian
variances, the means) are compared exactly too: both sides perform the correctly rounded IEEE operation."""
import numpy as np
import pytest

from . import reduce_ref as R
from ._helpers import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def K():
    import mau_amd  # noqa: F401
    from mau_amd import _lib

    class Kit:
        dev = torch.device("cuda:0")
        lib, call = _lib.lib, staticmethod(_lib.call)
        tickets = torch.zeros(_lib.lib.mau_reduce_tickets_elems(), dtype=torch.int32, device="cuda:0")

        @staticmethod
        def f64(n):
            return torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda:0")

        @staticmethod
        def off_base(t):
            """the same values on a base one float past a 16-byte boundary"""
            buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
            k = 1 + (-(buf.data_ptr() // 4) % 4)
            v = buf[k:k + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
            return v
    return Kit


def _planes(rng, *shape, bad=True):
    x = (rng.standard_normal(shape) * 9.0 + 290.0).astype(np.float32)          # |mean| >> std, as a temperature in kelvin
    if bad and x[0, 0].size > 8:
        x.reshape(shape[0], shape[1], -1)[0, 0, 3] = np.nan
        x.reshape(shape[0], shape[1], -1)[-1, -1, -1] = np.inf
    return x


PLANE_CASES = [(2, 2, 1, False), (2, 1, 4096, False), (2, 2, 4097, False), (1, 2, 4100, False), (1, 2, 62500, False), (70, 1, 4097, False),
               (2, 1, 4100, True)]


@pytest.mark.parametrize("B,C,HW,off", PLANE_CASES)
def test_plane_moments_bits(K, B, C, HW, off):
    x = _planes(np.random.default_rng(HW + B), B, C, HW)
    xd = torch.from_numpy(x).to(K.dev)
    xd = K.off_base(xd) if off else xd
    rows, ws = K.f64(B * C * 4), K.f64(K.lib.mau_plane_moments_ws_elems(B, C, HW))
    K.call("mau_plane_moments", xd.data_ptr(), rows.data_ptr(), ws.data_ptr(), K.tickets.data_ptr(), B, C, HW, None)
    assert same_bits(rows.cpu().numpy().reshape(B, C, 4), R.plane_moments(x, vec4=HW % 4 == 0 and not off), nan_matches_nan=True)


@pytest.mark.parametrize("B,HW,off", [(2, 1, False), (1, 4096, False), (2, 4097, False), (1, 4100, False), (1, 62500, False), (70, 4097, False),
                                      (1, 4100, True)])
def test_tile_stats_bits(K, B, HW, off):
    rng = np.random.default_rng(7 * HW + B)
    a, b = (rng.integers(0, 11, (B, HW)).astype(np.uint8) for _ in range(2))    # 9, 10: values outside the 9 classes
    cont, tg = _planes(rng, B, 5, HW), _planes(rng, B, 2, HW)
    ad, bd, cd, td = (torch.from_numpy(v).to(K.dev) for v in (a, b, cont, tg))
    cd = K.off_base(cd) if off else cd
    R_ = K.lib.mau_tile_stats_row_elems()
    rows, ws = K.f64(B * R_), K.f64(K.lib.mau_tile_stats_ws_elems(B, HW))
    K.call("mau_tile_stats", ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), td.data_ptr(), rows.data_ptr(), ws.data_ptr(),
           K.tickets.data_ptr(), B, HW, 9, None)
    assert same_bits(rows.cpu().numpy().reshape(B, R_), R.tile_stats(a, b, cont, tg, 9, vec4=HW % 4 == 0 and not off), nan_matches_nan=True)


@pytest.mark.parametrize("have", [True, False])
@pytest.mark.parametrize("N,H,W", [(2, 1, 1), (3, 64, 65), (70, 64, 65)])
def test_scenario_result_bits(K, N, H, W, have):
    rng = np.random.default_rng(N * H + W)
    out = rng.standard_normal((N, 2, H, W)).astype(np.float32)
    to = (rng.standard_normal((H, W)) * 9.0 + 288.0).astype(np.float32) if have else None
    d1, d2 = rng.integers(0, 3, (H, W)).astype(np.uint8), rng.integers(0, 3, (N, H, W)).astype(np.uint8)
    if N == 3:
        d2[1] = d1                                                               # a scenario without an edited pixel
    od, d1d, d2d = (torch.from_numpy(v).to(K.dev) for v in (out, d1, d2))
    tod = torch.from_numpy(to).to(K.dev) if have else None
    nd, tc, dl = (torch.zeros(N, H * W, device=K.dev) for _ in range(3))
    rows, ws = K.f64(N * 5), K.f64(K.lib.mau_scenario_result_ws_elems(N, H, W))
    K.call("mau_scenario_result", od.data_ptr(), tod.data_ptr() if have else None, d1d.data_ptr(), d2d.data_ptr(), 288.5, 9.25,
           nd.data_ptr(), tc.data_ptr(), dl.data_ptr(), rows.data_ptr(), ws.data_ptr(), K.tickets.data_ptr(), N, H, W, None)
    assert same_bits(rows.cpu().numpy().reshape(N, 5), R.scenario_result(out, to, d1, d2, 288.5, 9.25), nan_matches_nan=True)


@pytest.mark.parametrize("ncls", [9, 12])
@pytest.mark.parametrize("H,W", [(1, 1), (31, 17), (40, 250), (3, 4097)])
def test_eval_metrics_bits(K, H, W, ncls):
    B, C = 2, 2
    rng = np.random.default_rng(H * W + ncls)
    out, tgt = rng.standard_normal((B, C, H, W)).astype(np.float32), rng.standard_normal((B, C, H, W)).astype(np.float32)
    cls = rng.integers(0, ncls + 1, (B, H, W)).astype(np.uint8)                  # ncls: a value outside the classes
    if H * W > 8:
        out[0, 1, 0, 3] = np.nan
        cls[1][cls[1] == 2] = 3                                                  # a class without a pixel in sample 1
    scale, shift = np.array([1.0, 7.5]), np.array([0.0, 290.0])
    od, td, cd, sd, hd = (torch.from_numpy(v).to(K.dev) for v in (out, tgt, cls, scale, shift))
    R_ = K.lib.mau_eval_metrics_row_elems(ncls)
    rows, ws = K.f64(B * C * R_), K.f64(K.lib.mau_eval_metrics_ws_elems(B, C, H, W, ncls))
    K.call("mau_eval_metrics", od.data_ptr(), td.data_ptr(), cd.data_ptr(), sd.data_ptr(), hd.data_ptr(), rows.data_ptr(), ws.data_ptr(),
           K.tickets.data_ptr(), B, C, H, W, ncls, None)
    assert same_bits(rows.cpu().numpy().reshape(B * C, R_), R.eval_metrics(out, tgt, cls, scale, shift, ncls), nan_matches_nan=True)
