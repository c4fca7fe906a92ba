"""CPU-only checks of ``mau_amd.screening``: the numpy twins against the order twin and the exact brute force of
tests/screen_ref.py on dyadic gradients (bit for bit, whatever the order); the sign, the channel offset and the ``cur >= ncls`` rule
tied to ``placement.pack_host`` itself through a linear stand-in network; ``ScreeningResult.top``; every refusal; and the C ABI of
the new entry points (refusals run without a device)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import screen_ref as SR
from tests.test_scenario_host import METRICS, make_tile

NCLS = 9
STD = METRICS["temp_std"]
I32 = np.iinfo(np.int32)


def S():
    from mau_amd import screening
    return screening


def make_case(H, W, ncls=NCLS, K=3, seed=0, C=None):
    """A dyadic gradient (K, H, W, C), a second class map with ids >= ncls among its pixels, K objectives (temperature over the tile,
    NDVI over a partial roi, temperature over an empty roi) and their counts."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    C = 2 * ncls + 5 + 1 if C is None else C
    G = SR.dyadic(rng, (K, H, W, C))
    dw2 = rng.integers(0, ncls + 3, (H, W)).astype(np.uint8)
    dw2[rng.random((H, W)) < 0.1] = 255
    rois = np.stack([(rng.random((H, W)) < 0.4).astype(np.uint8) * 7, np.zeros((H, W), dtype=np.uint8)])
    objs = np.array([[1, -1], [0, 0], [1, 1]], dtype=np.int32)[:K]
    return G, dw2, rois, objs


def edits_for(H, W, ph, pw, ncls=NCLS):
    """interior, clipped at each of the four edges and two corners, fully outside on four sides, the ends of int32, cls = -1 and
    cls = ncls, a duplicate"""
    e = [[1, 1, 3 % ncls], [-1, 2, 0], [H - 1, 1, ncls - 1], [2, -2, 1 % ncls], [1, W - 1, 2 % ncls], [-ph + 1, -pw + 1, 0], [H - 1, W - 1, 0],
         [H, 0, 0], [-ph, 0, 0], [0, W, 0], [0, -pw, 0], [I32.min, I32.min, 0], [I32.max, I32.max, 0], [I32.min, 0, 0], [0, I32.max, 0],
         [1, 1, -1], [1, 1, ncls], [1, 1, I32.max], [1, 1, I32.min], [1, 1, 3 % ncls], [0, 0, 0]]
    return np.array(e, dtype=np.int64)


# --------------------------------------------------------------------------- #
# twin against brute force, dyadic data
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("ncls", [9, 1])
@pytest.mark.parametrize("H,W,ph,pw", [(5, 7, 1, 1), (5, 7, 3, 5), (8, 8, 3, 5), (16, 20, 40, 33), (16, 20, 3, 5)])
def test_twins_equal_brute_force_on_dyadic_gradients(H, W, ph, pw, ncls):
    G, dw2, rois, objs = make_case(H, W, ncls)
    assert SR.exact_sums(G)                                                            # every partial sum is exact: order cannot matter
    edits = edits_for(H, W, ph, pw, ncls)
    dout, counts = S().seed_host(objs, rois, (H, W))
    rd, rc = SR.screen_seed(objs, rois, H, W)
    assert SR.same(dout, rd) and SR.same(counts, rc) and counts[0] == H * W and counts[2] == 0 and 0 < counts[1] < H * W
    assert dout[0, 0].sum() == 0 and (dout[0, 1] == 1).all() and dout[1, 1].sum() == 0 and dout[1, 0].sum() == counts[1]
    got = S().rows_host(G, dw2, edits, counts, objs, (ph, pw), ncls, STD)
    twin = SR.screen_rows(G, dw2, edits, counts, objs, ph, pw, ncls, STD)
    brute = SR.brute_rows(G, dw2, edits, counts, objs, ph, pw, ncls, STD)
    assert got.shape == (3, len(edits), 4) and got.dtype == np.float64
    assert SR.same(got, twin) and SR.same(got, brute)
    # what the rows must say
    assert got[0, 0, 0] == min(ph, H - 1) * min(pw, W - 1) and (got[:, 7:15, 0] == 0).all()
    assert (got[:2, 15:19, 1:] == 0).all() and (got[:2, 15:19, 2].view(np.uint64) == 0).all() and (got[:, 15:19, 0] == got[0, 0, 0]).all()
    assert np.isnan(got[2, :, 2]).all() and np.isfinite(got[:2]).all() and (got[..., 3] == 0).all()
    assert SR.same(got[:, 19], got[:, 0]) and np.abs(got[:2, :7, 2]).max() > 0
    assert (got[:, :, 1] <= got[:, :, 0]).all()
    for k in range(3):
        assert SR.same(S().maps_host(G, dw2, counts, objs, k, ncls, STD), SR.screen_maps(G, dw2, counts, objs, k, ncls, STD))


def test_rows_host_matches_the_order_twin_on_general_data_and_carries_non_finite_values():
    H, W, ph, pw = 16, 20, 40, 33
    rng = np.random.default_rng(7)
    _, dw2, rois, objs = make_case(H, W)
    G = rng.standard_normal((3, H, W, 24)).astype(np.float32).astype(np.float64) * 10.0 ** rng.integers(-6, 6, (3, H, W, 24))
    G = G.astype(np.float32).astype(np.float64)
    G[0, 3, 4, 14 + 3], G[1, 9, 9, 14 + 5], dw2[3, 4], dw2[9, 9] = np.nan, np.inf, 0, 5
    edits = edits_for(H, W, ph, pw)
    _, counts = S().seed_host(objs, rois, (H, W))
    got = S().rows_host(G, dw2, edits, counts, objs, (ph, pw), NCLS, STD, seed_scale=4.0)
    assert SR.same(got, SR.screen_rows(G, dw2, edits, counts, objs, ph, pw, NCLS, STD, 4.0))
    # the NaN sits in channel off + 3 of pixel (3, 4): rows of class 3 whose stamp holds the pixel read it
    hit = np.array([SR.inside(e[0], e[1], ph, pw, H, W)[3, 4] and e[2] == 3 for e in edits])
    assert hit.any() and (got[0, :, 3] == hit).all() and (np.isnan(got[0, :, 2]) == hit).all()
    # the infinity sits in the CURRENT class's channel of pixel (9, 9): every live row whose stamp holds the pixel subtracts it
    hit = np.array([SR.inside(e[0], e[1], ph, pw, H, W)[9, 9] and 0 <= e[2] < NCLS for e in edits])
    assert hit.any() and (got[1, :, 3] >= hit).all() and (~np.isfinite(got[1, hit, 2])).all() and np.isfinite(got[1, ~hit, 2]).all()


# --------------------------------------------------------------------------- #
# the convention: a linear stand-in network over placement.pack_host
# --------------------------------------------------------------------------- #
def test_rows_are_the_change_of_a_linear_network_over_pack_host_exactly():
    """J(x) = <w, x> over the packed input, w dyadic.  Its input gradient is w, whatever the tile: entry 2 (coefficient 1: an NDVI
    objective, seed_scale 1, n = 1) must equal J(pack_host(stamped)) - J(pack_host(base)) -- computed in exact rational arithmetic --
    for interior, clipped, outside, cls = -1 and cls = ncls stamps and for pixels whose current class id is >= ncls."""
    from mau_amd import placement as P
    H, W, ph, pw = 9, 11, 3, 4
    rng = np.random.default_rng(11)
    dw, rgb, ndvi, temp = make_tile(rng, H, W)
    dw2 = rng.integers(0, NCLS + 2, (H, W)).astype(np.uint8)
    assert (dw2 >= NCLS).any()
    w = SR.dyadic(rng, (2 * NCLS + 5, H, W))
    edits = np.array([[2, 3, 4], [-1, -2, 6], [7, 9, 0], [9, 0, 1], [-3, 0, 2], [2, 3, -1], [2, 3, NCLS], [0, 0, 8]], dtype=np.int32)
    base = P.pack_host(dw, dw2, rgb, ndvi, temp, np.array([[0, 0, -1]], dtype=np.int32), (ph, pw), NCLS, METRICS)[0]
    stamped = P.pack_host(dw, dw2, rgb, ndvi, temp, edits, (ph, pw), NCLS, METRICS)

    def J(x):
        return sum((Fraction(a) * Fraction(b) for a, b in zip(w.reshape(-1).tolist(), x.astype(np.float64).reshape(-1).tolist())), Fraction(0))

    want = np.array([float(J(x) - J(base)) for x in stamped])
    G = np.zeros((1, H, W, 24))
    G[0, :, :, :23] = w.transpose(1, 2, 0)
    got = S().rows_host(G, dw2, edits, [1.0], [[0, -1]], (ph, pw), NCLS, STD)
    assert SR.same(got[0, :, 2], want) and np.abs(want[[0, 1, 2, 7]]).min() > 0 and (want[[3, 4, 5, 6]] == 0).all()
    assert SR.same(got, SR.screen_rows(G, dw2, edits, [1.0], [[0, -1]], ph, pw, NCLS, STD))
    assert SR.off_of(NCLS) == S().second_block(NCLS) == 14
    # the class maps say the same, pixel by pixel: a 1 x 1 stamp of class c at p changes J by maps[c, p]
    maps = S().maps_host(G, dw2, [1.0], [[0, -1]], 0, NCLS, STD)
    one = np.array([[4, 5, 3], [0, 0, 7]], dtype=np.int32)
    r1 = S().rows_host(G, dw2, one, [1.0], [[0, -1]], 1, NCLS, STD)
    assert [float(maps[3, 4, 5]), float(maps[7, 0, 0])] == r1[0, :, 2].tolist()


# --------------------------------------------------------------------------- #
# top()
# --------------------------------------------------------------------------- #
def test_top_orders_breaks_ties_by_index_and_puts_nan_last():
    R = S().ScreeningResult
    pred = np.array([0.5, -2.0, np.nan, -2.0, 3.0, -0.0, 0.0, -7.0, np.nan, 3.0])
    rows = np.zeros((2, 10, 4))
    rows[0, :, 2], rows[1, :, 2] = pred, -pred
    edits = np.stack([np.arange(10), np.arange(10), np.array([1, 1, 1, 6, 6, 6, 1, 6, 6, 1])], axis=1).astype(np.int32)
    r = R(rows, edits)
    assert r.top_index(10).tolist() == [7, 1, 3, 5, 6, 0, 4, 9, 2, 8]
    assert r.top_index(3).tolist() == [7, 1, 3] and r.top_index(0).tolist() == [] and r.top_index(99).size == 10
    assert r.top_index(10, sign=1).tolist() == [4, 9, 0, 5, 6, 1, 3, 7, 2, 8]
    assert r.top_index(10, cls=1).tolist() == [1, 6, 0, 9, 2] and r.top_index(2, cls=6).tolist() == [7, 3]
    assert r.top_index(10, k=1).tolist() == r.top_index(10, sign=1).tolist()
    assert np.array_equal(r.top(3), edits[[7, 1, 3]]) and r.top(3).dtype == np.int32
    assert r.top_index(5, cls=4).size == 0
    for bad in (dict(n=-1), dict(n=1, sign=0), dict(n=1, k=2), dict(n=1, k=-1)):
        with pytest.raises(ValueError):
            r.top_index(**bad)
    with pytest.raises(ValueError):
        r.grid(1)                                                                      # an explicit table has no grid
    from mau_amd import placement as P
    e, c, ys, xs = P.build_edits((16, 16), 8, NCLS, [1, 6], 8)
    g = R(np.arange(2 * 8 * 4, dtype=np.float64).reshape(2, 8, 4), e, c, ys, xs)
    assert g.grid(6).tolist() == [[18, 22], [26, 30]] and g.grid(1, k=1, entry=0).tolist() == [[32, 36], [40, 44]]
    for bad in (dict(cls=2), dict(cls=1, entry=4), dict(cls=1, k=2)):
        with pytest.raises(ValueError):
            g.grid(**bad)


def test_spearman_in_plain_numpy():
    sp = S().spearman
    assert sp([1, 2, 3, 4], [10, 20, 30, 40]) == 1.0 and sp([1, 2, 3, 4], [4, 3, 2, 1]) == -1.0
    assert abs(sp([1, 2, 3, 4, 5], [2, 1, 4, 3, 5]) - 0.8) < 1e-15                     # 1 - 6 * 4 / (5 * 24)
    assert abs(sp([1, 1, 2, 3], [1, 2, 3, 3]) - 8 / 9) < 1e-12                         # average ranks on ties: (0.5,0.5,2,3) x (0,1,2.5,2.5)
    assert sp([1, np.nan, 2, 3], [1, 5, 2, 3]) == 1.0 and np.isnan(sp([1.0], [2.0])) and np.isnan(sp([1, 1, 1], [1, 2, 3]))


# --------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------- #
def test_host_twins_refuse_bad_arguments():
    G, dw2, rois, objs = make_case(5, 7)
    _, counts = S().seed_host(objs, rois, (5, 7))
    ok = dict(G=G, dw_t2=dw2, edits=[[0, 0, 1]], counts=counts, objs=objs, patch=(2, 2), ncls=NCLS, temp_std=STD)
    assert S().rows_host(**ok).shape == (3, 1, 4)
    for kw in (dict(G=G[0]), dict(G=G[..., :22]), dict(dw_t2=dw2[:4]), dict(dw_t2=dw2.astype(np.int32)), dict(edits=[[0, 0]]), dict(edits=[[0.5, 0, 1]]),
               dict(edits=[[2 ** 31, 0, 1]]), dict(counts=counts[:2]), dict(objs=objs[:2]), dict(objs=[[2, -1]] * 3), dict(objs=[[1, -2]] * 3),
               dict(patch=0), dict(patch=(2, 0)), dict(patch=-1), dict(ncls=0), dict(ncls=17), dict(seed_scale=0.0), dict(seed_scale=-2.0),
               dict(seed_scale=3.0), dict(seed_scale=float("inf")), dict(seed_scale=float("nan")), dict(seed_scale=2.0 ** -140)):
        with pytest.raises(ValueError):
            S().rows_host(**{**ok, **kw})
    for kw in (dict(objs=[[1, 2]]), dict(objs=[[1, 0]], rois=None), dict(rois=rois[0]), dict(rois=rois.astype(np.float32)), dict(shape=(5, 8)),
               dict(shape=(0, 7)), dict(seed_scale=0.75), dict(objs=np.zeros((0, 2), dtype=np.int32)), dict(objs=[[0.0, -1.0]])):
        with pytest.raises(ValueError):
            S().seed_host(**{**dict(objs=objs, rois=rois, shape=(5, 7)), **kw})
    for kw in (dict(k=3), dict(k=-1), dict(seed_scale=6.0), dict(ncls=12)):
        with pytest.raises(ValueError):
            S().maps_host(**{**dict(G=G, dw_t2=dw2, counts=counts, objs=objs, k=0, ncls=NCLS, temp_std=STD), **kw})
    assert S().seed_host(objs, rois, (5, 7), seed_scale=2.0 ** -8)[0].max() == 2.0 ** -8


def test_session_refuses_before_it_touches_the_device():
    import mau_amd
    H = W = 32
    dw, rgb, ndvi, temp = (torch.from_numpy(a) for a in make_tile(np.random.default_rng(3), H, W))
    md, ts = torch.zeros(1, 8), torch.zeros(1, 12)
    net = mau_amd.UrbanPredictor("unet++", 23, 12, 8, 8, 8, 12, 2, base_filters=8, deep_supervision=True)
    with pytest.raises(ValueError, match="deep_supervision"):
        mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, metrics=METRICS)
    net = mau_amd.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=8, temporal_embeddings=False)
    roi = torch.ones(H, W, dtype=torch.uint8)
    for kw in (dict(patch=0), dict(patch=(8, -1)), dict(seed_scale=0), dict(seed_scale=-1.0), dict(seed_scale=3.0), dict(ncls=0), dict(ncls=17),
               dict(objectives=()), dict(objectives=(("lst", None),)), dict(objectives=("temp",)), dict(objectives=(("temp", None, 1),)),
               dict(precision="fp8"), dict(metrics={"temp_mean": 0.0})):
        with pytest.raises(ValueError):
            mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, **{**dict(metrics=METRICS, objectives=(("temp", roi),)), **kw})
    with pytest.raises(RuntimeError, match="no CPU"):                                  # and then the tile itself: this is the device path
        mau_amd.ScreeningSession(net, dw, rgb, ndvi, temp, md, ts, metrics=METRICS)
    assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())


def test_model_state_guard_puts_everything_back_when_entering_fails():
    """Snapshots first, then the changes: a model the guard cannot handle is left untouched, and a change that raises part-way is
    undone."""
    import mau_amd
    from mau_amd.screening import _ModelState
    foreign = torch.nn.Sequential(torch.nn.Linear(2, 2))
    with pytest.raises(AttributeError):
        with _ModelState(foreign, None):
            pass
    assert foreign.training and all(p.requires_grad for p in foreign.parameters())
    net = mau_amd.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=8, temporal_embeddings=False).train()
    net.freeze_inference(True)
    frozen = [m._frozen for m in net.modules() if hasattr(m, "_frozen")]

    class Boom(torch.nn.Parameter):
        def requires_grad_(self, flag=True):
            if not flag:
                raise RuntimeError("boom")
            return super().requires_grad_(flag)

    net.model.final.bias = Boom(net.model.final.bias.data)
    was = net.model._rt.precision
    with pytest.raises(RuntimeError, match="boom"):
        with _ModelState(net, "fp32"):
            pass
    assert net.model._rt.precision == was != "fp32"
    assert all(m.training for m in net.modules()) and all(a is b for a, b in zip(frozen, [m._frozen for m in net.modules() if hasattr(m, "_frozen")]))
    assert all(p.requires_grad for p in net.parameters())


def test_c_abi_refusals_without_a_device():
    from mau_amd import _lib
    lib = _lib.lib
    assert lib.mau_screen_row_elems() == 4 == len(S().ROW_NAMES)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    seed = dict(objs=p, rois=None, R=0, seed_scale=1.0, dout=p, counts=p, K=1, H=4, W=4)
    rows = dict(G=p, ld=24, dtype=0, dw_t2=p, edits=p, counts=p, objs=p, temp_std=1.0, seed_scale=1.0, rows=p, K=1, P=1, H=4, W=4, ph=1, pw=1, ncls=9)
    maps = dict(G=p, ld=24, dtype=0, dw_t2=p, counts=p, objs=p, temp_std=1.0, seed_scale=1.0, maps=p, k=0, K=1, H=4, W=4, ncls=9)
    cases = [("mau_screen_seed", seed, kw) for kw in (dict(objs=None), dict(dout=None), dict(counts=None), dict(K=0), dict(K=65536), dict(R=-1),
                                                      dict(H=0), dict(H=1 << 16, W=1 << 15), dict(seed_scale=0.0), dict(seed_scale=3.0))]
    cases += [("mau_screen_rows", rows, kw) for kw in (dict(G=None), dict(dw_t2=None), dict(edits=None), dict(counts=None), dict(objs=None),
                                                       dict(rows=None), dict(ph=0), dict(pw=0), dict(H=1 << 16, W=1 << 15), dict(ncls=0),
                                                       dict(ncls=17), dict(ld=22), dict(K=0), dict(P=0), dict(dtype=3), dict(seed_scale=-1.0))]
    cases += [("mau_screen_maps", maps, kw) for kw in (dict(G=None), dict(maps=None), dict(k=1), dict(k=-1), dict(ncls=17), dict(ld=16),
                                                       dict(W=0), dict(dtype=7), dict(seed_scale=0.3))]
    for name, base, kw in cases:
        a = {**base, **kw}
        assert getattr(lib, name)(*a.values(), None) == 1, (name, kw)                   # MAU_ERR_ARG, nothing launched
        assert lib.mau_last_error()
