"""GPU tests of ``mau_amd.screening``: the three kernels against the order twin and the exact brute force of tests/screen_ref.py by bit
pattern (dyadic and general gradients, every stamp kind, both load forms, planted non-finite values, row independence, the
seed scale as an equality); ``ScreeningSession`` split into "the gradient is right" (against ``oracle/unet_ref.py`` on the CPU, by
the project's own yardsticks, computed here) and "the reduction is right" (bit-equal to ``rows_host`` on that gradient); what a
session leaves behind on the model; and the command line.

Yardsticks.  fp32: the session's gradient against the oracle's fp64 gradient, within twice the oracle's own
fp32-versus-fp64 deviation.  bf16 / fp16: against the oracle's fp32 gradient, within twice the error of the oracle's own CPU
bf16-autocast gradient.  Both in L2 over the whole gradient; no fixed constant."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import screen_ref as SR
from tests._helpers import dev, mau, recorded_calls, same_bits  # noqa: F401
from tests.test_scenario_host import METRICS, make_tile
from tests.test_screening_host import NCLS, STD, edits_for, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAN = float("nan")


def g_dev(G, dt, ld):
    """The gradient in ``dt`` as a dense tensor (ld == its channels) or as the 24-channel view of a 32-wide one"""
    C = G.shape[-1]
    buf = torch.full((*G.shape[:3], ld), NAN, dtype=dt, device="cuda")
    buf[..., :C] = torch.from_numpy(G).to(dt).cuda()
    return buf if ld == C else buf[..., :C]


# --------------------------------------------------------------------------- #
# the seed
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W", [(5, 7), (16, 20)])
def test_seed_writes_every_element_and_counts_exactly(mau, H, W):
    S = mau.screening
    _, _, rois, objs = make_case(H, W)
    K, n = 3, 3 * 2 * H * W
    for scale in (1.0, 2.0 ** -8, 2.0 ** 8):
        want, counts = SR.screen_seed(objs, rois, H, W, scale)
        dout, cnt = S.seed(objs, dev(rois), (H, W), scale)
        assert SR.same(dout.cpu().numpy(), want) and SR.same(cnt.cpu().numpy(), counts) and counts.tolist() == [H * W, int((rois[0] != 0).sum()), 0]
    # the C entry point on NaN-prefilled, over-allocated buffers: everything inside is written, nothing outside
    buf = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    cb = torch.full((K + 4,), NAN, dtype=torch.float64, device="cuda")
    d_objs, d_rois = dev(objs), dev(rois)                                              # (named: a temporary's memory is free for the next one)
    mau._lib.call("mau_screen_seed", d_objs.data_ptr(), d_rois.data_ptr(), 2, 1.0, buf.data_ptr(), cb.data_ptr(), K, H, W,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want, counts = SR.screen_seed(objs, rois, H, W)
    assert SR.same(buf[:n].cpu().numpy().reshape(want.shape), want) and bool(torch.isnan(buf[n:]).all())
    assert SR.same(cb[:K].cpu().numpy(), counts) and bool(torch.isnan(cb[K:]).all())
    # no roi planes at all
    dout, cnt = S.seed([[0, -1]], None, (H, W))
    assert cnt.tolist() == [H * W] and bool((dout[0, 0] == 1).all()) and bool((dout[0, 1] == 0).all())
    for kw in (dict(objs=[[1, 2]]), dict(objs=[[2, -1]]), dict(seed_scale=3.0), dict(shape=(H, W + 1))):
        with pytest.raises(ValueError):
            S.seed(**{**dict(objs=objs, rois=dev(rois), shape=(H, W)), **kw})


# --------------------------------------------------------------------------- #
# the rows and the maps
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("ncls", [9, 1])
@pytest.mark.parametrize("ld", [24, 32])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("H,W,ph,pw", [(5, 7, 1, 1), (5, 7, 3, 5), (8, 8, 3, 5), (16, 20, 40, 33)])
def test_rows_and_maps_on_dyadic_gradients_bit_for_bit(mau, H, W, ph, pw, prec, ld, ncls):
    S, dt = mau.screening, DTYPES[prec]
    G, dw2, rois, objs = make_case(H, W, ncls, C=24)
    assert SR.exact_sums(G)
    edits = edits_for(H, W, ph, pw, ncls)
    _, counts = SR.screen_seed(objs, rois, H, W)
    g = g_dev(G, dt, ld)
    assert torch.equal(g.double().cpu(), torch.from_numpy(G))                          # the values are exact in this type
    got = S.rows(g, dev(dw2), edits, dev(counts), objs, (ph, pw), ncls, STD).cpu().numpy()
    assert SR.same(got, SR.screen_rows(G, dw2, edits, counts, objs, ph, pw, ncls, STD))
    assert SR.same(got, SR.brute_rows(G, dw2, edits, counts, objs, ph, pw, ncls, STD))
    assert SR.same(got, S.rows_host(G, dw2, edits, counts, objs, (ph, pw), ncls, STD))
    assert np.isnan(got[2, :, 2]).all() and (got[:2, 15:19, 2].view(np.uint64) == 0).all()         # an empty roi; no class: +0.0
    # K = 1 equals slice k of K = 3
    for k in range(3):
        one = S.rows(g[k:k + 1], dev(dw2), edits, dev(counts[k:k + 1]), objs[k:k + 1], (ph, pw), ncls, STD).cpu().numpy()
        assert same_bits(one[0], got[k])
    # the maps, both load forms: the aligned tensor, and the same values one element off a 16-byte boundary
    for k in range(3):
        want = SR.screen_maps(G, dw2, counts, objs, k, ncls, STD)
        out = S.maps(g, dev(dw2), dev(counts), objs, k, ncls, STD)
        assert SR.same(out.cpu().numpy(), want) and SR.same(S.maps_host(G, dw2, counts, objs, k, ncls, STD), want)
    flat = torch.full((3 * H * W * ld + 8,), NAN, dtype=dt, device="cuda")
    off = flat[1:1 + 3 * H * W * ld].view(3, H, W, ld)
    off[..., :24] = g
    assert off.data_ptr() % 16 != 0
    assert same_bits(S.maps(off[..., :24], dev(dw2), dev(counts), objs, 0, ncls, STD), S.maps(g, dev(dw2), dev(counts), objs, 0, ncls, STD))
    assert same_bits(S.rows(off[..., :24], dev(dw2), edits, dev(counts), objs, (ph, pw), ncls, STD).cpu().numpy(), got)


def test_maps_write_every_element_and_nothing_else(mau):
    S = mau.screening
    H, W = 5, 7
    G, dw2, rois, objs = make_case(H, W, C=24)
    _, counts = SR.screen_seed(objs, rois, H, W)
    g, n = g_dev(G, torch.bfloat16, 24), NCLS * H * W
    buf = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    d_dw2, d_counts, d_objs = dev(dw2), dev(counts), dev(objs)                         # (named: a temporary's memory is free for the next one)
    mau._lib.call("mau_screen_maps", g.data_ptr(), 24, mau.functional.dtype_code(g.dtype), d_dw2.data_ptr(), d_counts.data_ptr(),
                  d_objs.data_ptr(), STD, 1.0, buf.data_ptr(), 1, 3, H, W, NCLS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert SR.same(buf[:n].cpu().numpy().reshape(NCLS, H, W), SR.screen_maps(G, dw2, counts, objs, 1, NCLS, STD))
    assert bool(torch.isfinite(buf[:n]).all()) and bool(torch.isnan(buf[n:]).all())
    assert bool(torch.isnan(S.maps(g, dev(dw2), dev(counts), objs, 2, NCLS, STD)).all())           # an empty roi


@pytest.fixture(scope="module")
def general_case(mau):
    """A general fp32 gradient on 16 x 20 with a planted NaN and a planted infinity, 300 rows of random edits around the tile with
    the stamp 40 x 33 (more than four slots per thread), and the device's rows -- computed once, never written."""
    H, W, ph, pw = 16, 20, 40, 33
    rng = np.random.default_rng(21)
    _, dw2, rois, objs = make_case(H, W)
    G = (rng.standard_normal((3, H, W, 24)) * 10.0 ** rng.integers(-6, 6, (3, H, W, 24))).astype(np.float32).astype(np.float64)
    G[0, 3, 4, 14 + 3], G[1, 9, 9, 14 + 5], dw2[3, 4], dw2[9, 9] = np.nan, np.inf, 0, 5
    edits = np.stack([rng.integers(-45, 20, 300), rng.integers(-40, 24, 300), rng.integers(-1, NCLS + 1, 300)], axis=1).astype(np.int64)
    edits[:len(edits_for(H, W, ph, pw))] = edits_for(H, W, ph, pw)
    _, counts = SR.screen_seed(objs, rois, H, W)
    g = g_dev(G, torch.float32, 24)
    got = mau.screening.rows(g, dev(dw2), edits, dev(counts), objs, (ph, pw), NCLS, STD).cpu().numpy()
    return (H, W, ph, pw), G, g, dw2, objs, counts, edits, got


def test_rows_on_general_gradients_equal_the_order_twin(mau, general_case):
    (H, W, ph, pw), G, g, dw2, objs, counts, edits, got = general_case
    assert got.shape == (3, 300, 4)
    assert SR.same(got, SR.screen_rows(G, dw2, edits, counts, objs, ph, pw, NCLS, STD))
    assert SR.same(got, mau.screening.rows_host(G, dw2, edits, counts, objs, (ph, pw), NCLS, STD))
    # the planted NaN (channel off + 3 of pixel (3, 4), objective 0): counted and carried by exactly the class-3 rows that hold it
    hit = np.array([SR.inside(e[0], e[1], ph, pw, H, W)[3, 4] and e[2] == 3 for e in edits])
    assert hit.sum() > 3 and (got[0, :, 3] == hit).all() and (np.isnan(got[0, :, 2]) == hit).all()
    # the planted infinity (the current class's channel of pixel (9, 9), objective 1): every live row that holds the pixel
    hit = np.array([SR.inside(e[0], e[1], ph, pw, H, W)[9, 9] and 0 <= e[2] < NCLS for e in edits])
    assert hit.sum() > 10 and (got[1, :, 3] >= hit).all() and (~np.isfinite(got[1, hit, 2])).all() and np.isfinite(got[1, ~hit, 2]).all()
    assert (got[1, ~hit, 3] == 0).all() and np.isnan(got[2, :, 2]).all()


def test_rows_repeat_and_do_not_depend_on_the_table(mau, general_case):
    S = mau.screening
    (H, W, ph, pw), G, g, dw2, objs, counts, edits, got = general_case
    run = lambda e: S.rows(g, dev(dw2), e, dev(counts), objs, (ph, pw), NCLS, STD).cpu().numpy()      # noqa: E731
    assert same_bits(run(edits), got)                                                  # a second call: identical bits
    for j in (0, 5, 19, 150, 299):                                                     # a row alone (P = 1) is its row of the table
        assert same_bits(run(edits[j:j + 1])[:, 0], got[:, j]), j
    perm = np.random.default_rng(22).permutation(300)
    assert same_bits(run(edits[perm]), got[:, perm])
    on_device = S.rows(g, dev(dw2), dev(edits.astype(np.int32)), dev(counts), objs, (ph, pw), NCLS, STD).cpu().numpy()
    assert same_bits(on_device, got)


def test_seed_scale_is_undone_exactly(mau, general_case):
    """fp32: a gradient scaled by 2^-8 or 2^8 with the matching seed_scale gives the SAME bits as scale 1 -- an equality."""
    S = mau.screening
    (H, W, ph, pw), G, g, dw2, objs, counts, edits, got = general_case
    for scale in (2.0 ** -8, 2.0 ** 8):
        gs = (g * scale).contiguous()
        assert torch.equal(gs / scale, g) or bool(torch.isnan(g).any())
        r = S.rows(gs, dev(dw2), edits, dev(counts), objs, (ph, pw), NCLS, STD, seed_scale=scale).cpu().numpy()
        assert SR.same(r, got)
        for k in range(2):
            assert SR.same(S.maps(gs, dev(dw2), dev(counts), objs, k, NCLS, STD, seed_scale=scale).cpu().numpy(),
                           S.maps(g, dev(dw2), dev(counts), objs, k, NCLS, STD).cpu().numpy())


def test_device_wrappers_validate(mau, general_case):
    S = mau.screening
    (H, W, ph, pw), G, g, dw2, objs, counts, edits, got = general_case
    ok = dict(G=g, dw_t2=dev(dw2), edits=edits[:4], counts=dev(counts), objs=objs, patch=(ph, pw), ncls=NCLS, temp_std=STD)
    for kw in (dict(G=g[0]), dict(G=g[..., :22]), dict(G=g[:, :, ::2]), dict(dw_t2=dev(dw2)[:5]), dict(counts=dev(counts)[:2]), dict(objs=objs[:2]),
               dict(patch=0), dict(ncls=17), dict(seed_scale=5.0), dict(edits=edits[:, :2])):
        with pytest.raises(ValueError):
            S.rows(**{**ok, **kw})
    with pytest.raises(TypeError):
        S.rows(**{**ok, "G": g.double()})
    with pytest.raises(RuntimeError, match="no CPU"):
        S.rows(**{**ok, "G": g.cpu()})
    with pytest.raises(ValueError):
        S.maps(g, dev(dw2), dev(counts), objs, 3, NCLS, STD)


# --------------------------------------------------------------------------- #
# the session: the gradient against the oracle, the rows against rows_host on that gradient
# --------------------------------------------------------------------------- #
TH, TW, PATCH, CLASSES = 32, 48, 8, [1, 6]
NET = {"unet": dict(temporal_embeddings=False, metadata_embeddings=True), "unet++": {}}


@pytest.fixture(scope="module")
def tile_case():
    rng = np.random.default_rng(31)
    tile = make_tile(rng, TH, TW)
    dw2 = np.where(rng.random((TH, TW)) < 0.3, rng.integers(0, NCLS, (TH, TW)), tile[0]).astype(np.uint8)
    roi = (rng.random((TH, TW)) < 0.3).astype(np.uint8)
    g = torch.Generator().manual_seed(32)
    return tile, dw2, roi, torch.randn(1, 12, generator=g), torch.randn(1, 8, generator=g)


def make_net(mau, mt, prec):
    torch.manual_seed(33)
    net = mau.UrbanPredictor(mt, 23, 12, 16, 8, 16, 24, 2, base_filters=8, **NET[mt])
    return net.cuda().set_precision(prec).eval()


def oracle_gradients(mau, net, mt, tile_case, dout):
    """The oracle's input gradient of sum_k <dout_k, out_k> on the CPU: in fp64, in fp32 and under bf16 autocast, (K, H, W, 23) each"""
    from oracle import unet_ref as R
    tile, dw2, _, ts, md = tile_case
    K = dout.shape[0]
    x = torch.from_numpy(mau.placement.pack_host(tile[0], dw2, *tile[1:], np.tile([[0, 0, -1]], (K, 1)), PATCH, NCLS, METRICS))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}

    def grad(cast, autocast=False):
        s = {k: (cast(v) if v.is_floating_point() else v) for k, v in sd.items()}
        xi = cast(x).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            out = R.forward(mt, s, xi, cast(ts.expand(K, -1)), cast(md.expand(K, -1)), False, **NET[mt])
        return torch.autograd.grad(out, xi, grad_outputs=cast(dout).to(out.dtype))[0].double().permute(0, 2, 3, 1).numpy()

    return grad(lambda v: v.double()), grad(lambda v: v.float()), grad(lambda v: v.float(), True)


def session_for(mau, net, tile_case, **kw):
    tile, dw2, roi, ts, md = tile_case
    objectives = (("temp", None), ("ndvi", dev(roi)), ("temp", dev(roi)))
    return mau.ScreeningSession(net, *(dev(a) for a in tile), md.cuda(), ts.cuda(), metrics=METRICS, ncls=NCLS, patch=PATCH,
                                objectives=objectives, dw_t2=dev(dw2), **kw)


def l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


@pytest.mark.parametrize("mt", ["unet", "unet++"])
def test_session_fp32_gradient_against_the_oracle_and_rows_against_rows_host(mau, tile_case, mt):
    S = mau.screening
    net = make_net(mau, mt, "fp32")
    sess = session_for(mau, net, tile_case)
    tile, dw2, roi, ts, md = tile_case
    assert tuple(sess.gradient.shape) == (3, TH, TW, 24) and sess.gradient.dtype == torch.float32 and sess.counts.tolist() == [TH * TW, roi.sum(), roi.sum()]
    g64, g32, _ = oracle_gradients(mau, net, mt, tile_case, sess.dout.cpu())
    got = sess.gradient.double().cpu().numpy()
    err, yard = l2(got[..., :23] - g64), l2(g32 - g64)
    print(f"screening {mt} fp32: input gradient against the fp64 oracle {err:.3e} (L2; the gradient's norm {l2(g64):.3e}), "
          f"the oracle's own fp32-vs-fp64 deviation {yard:.3e}, ratio {err / yard:.2f}")
    assert np.isfinite(got).all() and l2(g64) > 0 and (got[..., 23] == 0).all()
    assert err <= 2.0 * yard, (err, yard)
    # the reduction: bit-equal to rows_host on the gradient the session used
    r = sess(CLASSES, stride=8)
    assert r.rows.shape == (3, 48, 4) and np.array_equal(r.edits, mau.placement.edits_table(r.ys, r.xs, CLASSES))
    host = S.rows_host(sess.gradient, dw2, r.edits, sess.counts.cpu().numpy(), [[1, -1], [0, 0], [1, 0]], PATCH, NCLS, STD)
    assert SR.same(r.rows, host) and (r.rows[..., 0] == 64).all() and (r.rows[..., 3] == 0).all() and len(set(r.rows[0, :, 2])) > 24
    assert np.array_equal(r.grid(6, 2), r.rows[2, 24:, 2].reshape(4, 6))
    e = np.array([[-3, 40, 2], [5, 5, -1], [31, 47, 0]], dtype=np.int32)
    assert SR.same(sess(edits=e).rows, S.rows_host(sess.gradient, dw2, e, sess.counts.cpu().numpy(), [[1, -1], [0, 0], [1, 0]], PATCH, NCLS, STD))
    assert SR.same(sess.maps(1), S.maps_host(sess.gradient, dw2, sess.counts.cpu().numpy(), [[1, -1], [0, 0], [1, 0]], 1, NCLS, STD))
    # the first-order prediction against the exact sweep of the same grid, on this random-weight network: a figure, not a bar
    exact = mau.PlacementSession(net, *(dev(a) for a in tile), md.cuda(), ts.cuda(), metrics=METRICS, ncls=NCLS, patch=PATCH, batch=4,
                                 dw_t2=dev(dw2), roi=dev(roi))(CLASSES, stride=8)
    print(f"screening {mt} fp32: Spearman of predicted and exact mean dT over 48 stamps {S.spearman(r.rows[0, :, 2], exact.rows[:, 1]):.3f} "
          f"(tile), {S.spearman(r.rows[2, :, 2], exact.rows[:, 7]):.3f} (roi)")
    # the seed scale, through the whole backward: exact powers of two, the same bits
    for scale in (2.0 ** -8, 2.0 ** 8):
        assert SR.same(session_for(mau, net, tile_case, seed_scale=scale)(CLASSES, stride=8).rows, r.rows), scale


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("mt", ["unet", "unet++"])
def test_session_16_bit_gradient_against_the_autocast_yardstick(mau, tile_case, mt, prec):
    S = mau.screening
    net = make_net(mau, mt, prec)
    sess = session_for(mau, net, tile_case)
    _, dw2, _, _, _ = tile_case
    assert sess.gradient.dtype == DTYPES[prec]
    _, g32, gac = oracle_gradients(mau, net, mt, tile_case, sess.dout.cpu())
    got = sess.gradient.double().cpu().numpy()
    err, yard = l2(got[..., :23] - g32), l2(gac - g32)
    print(f"screening {mt} {prec}: input gradient against the fp32 oracle {err:.3e} (L2; the gradient's norm {l2(g32):.3e}), "
          f"the oracle's own bf16-autocast error {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 2.0 * yard, (err, yard)
    r = sess(CLASSES, stride=8)
    assert (r.rows[..., 3] == 0).all() and np.isfinite(r.rows).all()
    assert SR.same(r.rows, S.rows_host(sess.gradient, dw2, r.edits, sess.counts.cpu().numpy(), [[1, -1], [0, 0], [1, 0]], PATCH, NCLS, STD))


# --------------------------------------------------------------------------- #
# what a session leaves behind
# --------------------------------------------------------------------------- #
SESSION_LAUNCHES = {
    "mau_screen_seed", "mau_screen_rows", "mau_screen_maps", "mau_placement_pack",
    # the forward in eval mode with saved tensors
    "mau_conv3x3_pack_desc_fill", "mau_conv3x3_pack_weights_multi", "mau_conv3x3_pack_weights", "mau_meta_mlp_fwd", "mau_lstm_fwd", "mau_linear_fwd",
    "mau_conv3x3_fwd", "mau_conv3x3_fwd2", "mau_bn_coeffs_eval", "mau_bn_relu_apply", "mau_bn_relu_apply_pool", "mau_resize_bilinear_bn_fwd",
    "mau_resize_bilinear_fwd", "mau_head_bn_fwd", "mau_head_fwd", "mau_maxpool2x2_fwd", "mau_copy_channels", "mau_bcast_fill",
    # the backward: dz (two passes around one reduction), the data gradient, the adjoints of pool, resize and concat
    "mau_head_bn_bwd_reduce", "mau_head_bn_bwd_apply", "mau_head_bwd", "mau_bn_relu_bwd_reduce", "mau_bn_relu_bwd_apply", "mau_pool_bn_bwd_reduce",
    "mau_pool_bn_bwd_apply", "mau_reduce_rows_f64_f32", "mau_resize_bilinear_bwd", "mau_maxpool2x2_bwd", "mau_maxpool2x2_bwd_add", "mau_sum_tensors",
    "mau_bcast_bwd",
}


def test_packs_follow_the_precision_without_an_optimizer_step(mau, tile_case):
    """``PackGroup.ensure``: bf16 -> fp16 -> bf16 with no optimizer step and no load in between.  The group's packs of a type stay
    current, but a parameter's own entry names the packs of the type that ran last: the forward in the first type must come back
    bit for bit (it once ran on the other type's packs)."""
    tile, dw2, _, ts, md = tile_case
    net = make_net(mau, "unet", "bf16")
    P = mau.placement
    e = np.array([[0, 0, -1], [4, 8, 6]], dtype=np.int32)

    def forward(prec):
        net.set_precision(prec)
        x = P.pack(*(dev(a) for a in tile[:1]), dev(dw2), *(dev(a) for a in tile[1:]), e, PATCH, NCLS, METRICS, DTYPES[prec])
        with torch.no_grad():
            return net(x, ts.cuda().expand(2, -1).contiguous(), md.cuda().expand(2, -1).contiguous()).clone()

    first, other = forward("bf16"), forward("fp16")
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, other)
    assert same_bits(forward("bf16"), first) and same_bits(forward("fp16"), other)


def test_session_leaves_the_model_as_it_found_it(mau, tile_case):
    tile, dw2, roi, ts, md = tile_case
    net = make_net(mau, "unet", "bf16")
    args = (*(dev(a) for a in tile), md.cuda(), ts.cuda())
    pk = dict(metrics=METRICS, ncls=NCLS, patch=PATCH, batch=4, dw_t2=dev(dw2), roi=dev(roi))
    place = mau.PlacementSession(net, *args, **pk)                                     # freezes the model, captures a graph
    before = place(CLASSES, stride=8).rows
    frozen = [m._frozen for m in net.modules() if hasattr(m, "_frozen")]
    assert all(f is not None for f in frozen)
    net.model.conv0_0.conv1.weight.requires_grad_(False)                               # one parameter is frozen by its owner
    needs = [p.requires_grad for p in net.parameters()]
    with recorded_calls(mau, (mau.placement, mau.screening)) as calls:
        sess = session_for(mau, net, tile_case, precision="fp16")
        r = sess(CLASSES, stride=8)
        sess.maps(0)
    names = [c[0] for c in calls]
    assert names.count("mau_screen_seed") == 1 and names.count("mau_screen_rows") == 1 and names.count("mau_screen_maps") == 1
    assert names.count("mau_placement_pack") == 1 and sum(n.startswith("mau_conv3x3_fwd") for n in names) > 18
    assert not [n for n in names if "wgrad" in n or "opt_pack" in n or "adamw" in n or "grad_norm" in n], names
    # every launch of the run, by name: the forward, the data gradients and the streaming backward passes.  The BatchNorm backward's
    # reduce passes (mau_*_bwd_reduce, mau_reduce_rows_f64_f32) form dgamma / dbeta as by-products of dz and are accepted; the sum
    # of the head's parameter slab (mau_reduce_rows_f32) is not: no head parameter takes a gradient
    assert set(names) <= SESSION_LAUNCHES, sorted(set(names) - SESSION_LAUNCHES)
    assert "mau_reduce_rows_f32" not in names and "mau_head_bn_bwd_reduce" in names
    assert sess.dtype == torch.float16 and net.model._rt.precision == "bf16" and not net.training
    assert [p.requires_grad for p in net.parameters()] == needs and all(p.grad is None for p in net.parameters())
    assert all(a is b for a, b in zip(frozen, [m._frozen for m in net.modules() if hasattr(m, "_frozen")]))
    assert same_bits(place(CLASSES, stride=8).rows, before)                            # the captured session still reads what it read
    assert same_bits(mau.PlacementSession(net, *args, **pk)(CLASSES, stride=8).rows, before)
    # and in the other order, on a model in training mode: screening first, then a placement session
    net2 = make_net(mau, "unet", "bf16").train()
    first = session_for(mau, net2, tile_case)(CLASSES, stride=8)
    assert net2.training and all(m.training for m in net2.modules()) and all(p.requires_grad and p.grad is None for p in net2.parameters())
    assert all(m._frozen is None for m in net2.modules() if hasattr(m, "_frozen"))
    assert same_bits(mau.PlacementSession(net2, *args, **pk)(CLASSES, stride=8).rows, before)
    assert same_bits(session_for(mau, net2, tile_case)(CLASSES, stride=8).rows, first.rows)
    # an explicit table through the placement session: the same rows as the grid sweep's
    pick = np.array([40, 3, 17, 3, 0])
    sub = place(edits=place(CLASSES, stride=8).edits[pick])
    assert same_bits(sub.rows, before[pick]) and sub.classes is None
    with pytest.raises(ValueError):
        place(CLASSES, edits=np.zeros((1, 3), dtype=np.int32))
    with pytest.raises(ValueError):
        mau.ScreeningSession(mau.UrbanPredictor("unet++", 23, 12, 8, 8, 8, 12, 2, base_filters=8, deep_supervision=True).cuda(), *args, metrics=METRICS)


# --------------------------------------------------------------------------- #
# the command line
# --------------------------------------------------------------------------- #
def test_command_line_screen(mau, tmp_path):
    """``python -m mau_amd.placement ... --screen 3`` in a fresh process on a synthetic 32 x 32 tile, patch 8, stride 8: the new keys,
    and the exact rows of the screened subset bit-identical to the same edits' rows of a full sweep (a placement row depends on its own
    sample only); without ``--screen`` the output has the keys it always had."""
    from mau_amd import checkpoint as C
    torch.manual_seed(7)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "temporal_embeddings": False, "metadata_embeddings": True}
    net = mau.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    ck = str(tmp_path / "tiny.pth")
    C.save_checkpoint(ck, net, None, epoch=0, step=0, loss=0.0, hyperparameters=hyper, model_type="unet", study_name="s", trial_id=0,
                      metadata_input_length=8)
    rng = np.random.default_rng(84)
    dw, rgb, ndvi, temp = make_tile(rng, 32, 32)
    roi = rng.random((32, 32)) < 0.3
    tile_path, roi_path, mj = str(tmp_path / "tile.npz"), str(tmp_path / "roi.npy"), str(tmp_path / "metrics.json")
    np.savez(tile_path, dw=dw, rgb=rgb, ndvi=ndvi, temp=temp, metadata_raw=np.array([48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9], dtype=np.float64),
             temp_series=rng.standard_normal(12))
    np.save(roi_path, roi)
    with open(mj, "w") as f:
        json.dump(METRICS, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "mau_amd.placement", ck, "--tile", tile_path, "--metrics-json", mj, "--classes", "1,6", "--patch", "8",
           "--stride", "8", "--batch", "5", "--roi", roi_path, "--precision", "fp16"]
    full_path, scr_path = str(tmp_path / "full.npz"), str(tmp_path / "screen.npz")
    p = subprocess.run(cmd + ["--output", full_path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0 and "7 batches of 5" in p.stdout and "screened" not in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    full = np.load(full_path)
    assert set(full.files) == {"rows", "edits", "classes", "ys", "xs", "ndvi", "temp_c", "best", *(f"grid_c{c}_e{e}" for c in (1, 6) for e in (1, 4, 7))}
    p = subprocess.run(cmd + ["--screen", "3", "--output", scr_path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "6 swept exactly in 2 batches of 5" in p.stdout and "Spearman rank correlation" in p.stdout
    got = np.load(scr_path)
    assert set(got.files) == {"edits", "classes", "ys", "xs", "ndvi", "temp_c", "best", "predicted", "screened_index", "screened_edits", "screened_rows",
                              "spearman", "pred_grid_c1", "pred_grid_c6"}
    assert np.array_equal(got["edits"], full["edits"]) and got["predicted"].shape == (32, 4) and got["screened_rows"].shape == (6, 12)
    idx = got["screened_index"]
    assert np.array_equal(got["screened_edits"], full["edits"][idx]) and (idx[:3] < 16).all() and (idx[3:] >= 16).all() and np.unique(idx).size == 6
    assert np.array_equal(got["screened_rows"].view(np.uint64), full["rows"][idx].view(np.uint64))
    assert np.array_equal(got["ndvi"].view(np.uint32), full["ndvi"].view(np.uint32))
    for half, c in ((slice(0, 16), 1), (slice(16, 32), 6)):                            # the three most negative predictions of each class, in order
        order = np.argsort(got["predicted"][half, 2], kind="stable")[:3] + half.start
        assert np.array_equal(idx[3 * (c == 6):3 * (c == 6) + 3], order)
        assert np.array_equal(got[f"pred_grid_c{c}"], got["predicted"][half, 2].reshape(4, 4))
    want = mau.screening.spearman(got["predicted"][idx, 2], got["screened_rows"][:, 7])
    assert (np.isnan(want) and np.isnan(got["spearman"])) or float(got["spearman"]) == want
    assert (got["predicted"][:, 3] == 0).all() and (got["predicted"][:, 0] == 64).all()
    bad = subprocess.run(cmd + ["--screen", "-1"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert bad.returncode != 0
