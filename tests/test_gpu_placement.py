"""GPU tests of ``mau_amd.placement``: ``mau_placement_pack`` against the host truth (``data.pack_tiles`` on host-edited class maps
and ``normalized_planes_host``, bit for bit) and against ``mau_region_gather``; ``mau_placement_result`` against its order-exact
float64 twin (tests/placement_ref.py) by bit pattern; ``PlacementSession`` against the same three steps composed by hand, eagerly
and twice; and the command line in a fresh process.

Bounds.  Everything is compared as bit patterns except one figure: a placement's temperature change rebuilt from two batch-1
eager forwards against the session's at batch 5 -- the convolution's inference form depends on the launch shape (DESIGN.md
section 2), so the bar is the project's fp32 parity bar, 1e-3 of the max-norm of the two temperature maps (the bar
tests/test_gpu_region.py uses between batch sizes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import placement_ref as PR
from tests._helpers import bits, dev, mau, same_bits  # noqa: F401
from tests.test_placement_host import EDITS, H, NCLS, PH, PW, STAMP_PIXELS, W
from tests.test_scenario_host import METRICS, make_tile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MEAN, STD = METRICS["temp_mean"], METRICS["temp_std"]


# --------------------------------------------------------------------------- #
# the pack
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def pack_case(mau):
    """One 37 x 45 tile (H * W is no multiple of 4; host arrays, never written), a second class map of its own, and the truth of
    the rows of EDITS: interior, over every edge and two corners (negative origins), wholly outside on all four sides, cls = -1
    and cls = 9, a duplicate, and the ends of int32."""
    rng = np.random.default_rng(80)
    dw, rgb, ndvi, temp = make_tile(rng, H, W)
    dw2 = np.where(rng.random((H, W)) < 1 / 3, (dw + rng.integers(1, NCLS, (H, W))) % NCLS, dw).astype(np.uint8)
    maps = PR.edited_maps(dw2, EDITS, PH, PW, NCLS)
    assert [int((m != dw2).sum()) <= n for m, n in zip(maps, STAMP_PIXELS)] == [True] * len(EDITS)
    for b in (7, 8, 9, 10, 11, 12, 14, 15, 16):                                        # outside, cls = -1, cls = 9, int32 ends: the baseline
        assert np.array_equal(maps[b], dw2), b
    assert np.array_equal(maps[0], maps[13]) and (maps[0][10:15, 12:19] == 3).all() and not np.array_equal(maps[0], dw2)
    cont = mau.scenario.normalized_planes_host(rgb, ndvi, temp, METRICS)
    return (dw, dw2, rgb, ndvi, temp), maps, cont


@pytest.mark.parametrize("ld", [24, 32])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_pack_matches_host_truth_bit_for_bit(mau, pack_case, prec, ld):
    P, dt = mau.placement, DTYPES[prec]
    (dw, dw2, rgb, ndvi, temp), maps, cont = pack_case
    B = len(EDITS)
    ref = mau.data.pack_tiles(dev(np.repeat(dw[None], B, 0)), dev(maps), dev(np.repeat(cont[None], B, 0)), None, dt)
    assert ref.C == 23 and tuple(ref.t.shape) == (B, H, W, 24)
    x = P.pack(dev(dw), dev(dw2), dev(rgb), dev(ndvi), dev(temp), EDITS, (PH, PW), NCLS, METRICS, dt, ld=ld)
    assert x.C == 23 and tuple(x.t.shape) == (B, H, W, ld) and x.t.dtype == dt
    assert same_bits(x.t[..., :24], ref.t)
    assert int((bits(x.t)[..., 23:] != 0).sum()) == 0                                  # the padding channels are zero bits
    # the C entry point on an over-allocated, NaN-prefilled buffer with the edits as a device tensor: nothing beyond B*H*W*ld moves
    n, extra = B * H * W * ld, 4096
    buf = torch.full((n + extra,), float("nan"), dtype=dt, device="cuda")
    before = bits(buf).clone()
    t = [dev(a) for a in (dw, dw2, rgb, ndvi, temp)]
    from mau_amd._tile import norm_row
    norm, edits = dev(norm_row(METRICS)), dev(EDITS)
    mau._lib.call("mau_placement_pack", *(v.data_ptr() for v in t), edits.data_ptr(), norm.data_ptr(), buf.data_ptr(), ld,
                  mau.functional.dtype_code(dt), B, H, W, PH, PW, NCLS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf)[:n].view(B, H, W, ld), bits(x.t)) and torch.equal(bits(buf)[n:], before[n:])
    # the dense view is pack_host's, rounded to the network's type
    dense = P.pack_host(dw, dw2, rgb, ndvi, temp, EDITS, (PH, PW), NCLS, METRICS)
    assert torch.equal(x.t[..., :23].permute(0, 3, 1, 2), dev(dense).to(dt))


def test_pack_equals_region_gather_and_validates(mau, pack_case):
    """One arithmetic in three entry points: a 32 x 32 tile as one window of ``mau_region_gather`` with the host-edited map
    (``dw_t2 = NULL`` here: the stamps go into dw_t1's own map)."""
    P, R = mau.placement, mau.region
    dw, rgb, ndvi, temp = make_tile(np.random.default_rng(81), 32, 32)
    edits = np.array([[5, 9, 6], [-3, 28, 1], [0, 0, -1]], dtype=np.int32)
    maps = PR.edited_maps(dw, edits, PH, PW, NCLS)
    origin = dev(np.zeros((1, 2), dtype=np.int32))
    for dt in (torch.bfloat16, torch.float32):
        got = P.pack(dev(dw), None, dev(rgb), dev(ndvi), dev(temp), dev(edits), (PH, PW), NCLS, METRICS, dt)
        for b in range(len(edits)):
            want = R.gather(dev(dw), dev(maps[b]), dev(rgb), dev(ndvi), dev(temp), origin, 32, NCLS, METRICS, dt)
            assert same_bits(got.t[b:b + 1], want.t) and got.C == want.C
    (dw, dw2, rgb, ndvi, temp), _, _ = pack_case
    args = (dev(dw), dev(dw2), dev(rgb), dev(ndvi), dev(temp))
    for kw in (dict(patch=0), dict(patch=(PH, 0)), dict(ncls=0), dict(ncls=17), dict(ld=20), dict(ld=16), dict(edits=EDITS[:, :2]),
               dict(edits=np.zeros((65536, 3), dtype=np.int32))):
        a = dict(edits=EDITS, patch=(PH, PW), ncls=NCLS, ld=None)
        a.update(kw)
        with pytest.raises(ValueError):
            P.pack(*args, a["edits"], a["patch"], a["ncls"], METRICS, ld=a["ld"])
    with pytest.raises(RuntimeError, match="no CPU"):
        P.pack(torch.from_numpy(dw), *args[1:], EDITS, (PH, PW), NCLS, METRICS)


# --------------------------------------------------------------------------- #
# the result
# --------------------------------------------------------------------------- #
def make_result_case(h, w, B=5, seed=0):
    """Sample 3 carries a NaN (temperature plane, inside its stamp) and both infinities (NDVI plane); sample 2's stamp is empty."""
    rng = np.random.default_rng(seed + h * w)
    base = rng.standard_normal((2, h, w)).astype(np.float32)
    out = (base[None] + 0.1 * rng.standard_normal((B, 2, h, w))).astype(np.float32)
    out[3, 1, 2, 3], out[3, 0, h - 1, w - 1], out[3, 0, 4, 0] = np.nan, np.inf, -np.inf
    roi = (rng.random((h, w)) < 0.3).astype(np.uint8) * 200
    edits = np.array([[3, 4, 1], [-2, -3, 6], [h, 0, 1], [1, 2, 2], [h - 2, w - 3, -1]], dtype=np.int32)[:B]
    return out, base, roi, edits


# 37 x 45: one ragged chunk, 4-byte accesses; 64 x 64: exactly one chunk; 65 x 64: a second chunk of 64 pixels; 96 x 128: three chunks
@pytest.mark.parametrize("with_roi", [True, False], ids=["roi", "no_roi"])
@pytest.mark.parametrize("h,w", [(37, 45), (64, 64), (65, 64), (96, 128)])
def test_result_matches_the_order_exact_twin_bit_for_bit(mau, h, w, with_roi):
    P = mau.placement
    out, base, roi, edits = make_result_case(h, w)
    roi = roi if with_roi else None
    tickets = torch.zeros(mau._lib.lib.mau_reduce_tickets_elems(), dtype=torch.int32, device="cuda")

    def run(o, e, patch=(PH, PW)):
        return P.result(dev(o), dev(base), e, patch, MEAN, STD, roi=None if roi is None else dev(roi), tickets=tickets).cpu().numpy()

    got = run(out, edits)
    want = PR.placement_result(out, base, edits, roi, MEAN, STD, PH, PW)
    assert got.shape == (5, 12) and got.dtype == np.float64 and PR.same_rows(got, want)
    assert got[:, 0].tolist() == [35, 12, 0, 35, 6] and got[:, 11].tolist() == [0, 0, 0, 3, 0]
    assert np.isnan(got[2, [4, 9]]).all() and np.isnan(got[3, 1]) and np.isfinite(got[3, [2, 3]]).all()
    assert (got[:, 6] == (int((roi != 0).sum()) if with_roi else 0)).all() and np.isnan(got[:, [7, 10]]).all() == (not with_roi)
    assert int(tickets.abs().sum()) == 0                                               # the tickets are left zeroed
    assert same_bits(run(out, edits), got)                                             # a second call: identical bits
    # a sample in another slot, or alone: the same row bits (device against device: NaN payloads included)
    perm = [4, 2, 0, 3, 1]
    assert same_bits(run(out[perm], edits[perm]), got[perm])
    for b in (1, 3):
        assert same_bits(run(out[b:b + 1], edits[b:b + 1]), got[b:b + 1])
    # a stamp that covers the tile: [5] is NaN, [4] is [1] up to the order of the sums
    e = np.array([[0, 0, 1], [-1, -2, 1]], dtype=np.int32)
    cover = run(out[:2], e, (h + 1, w + 2))
    assert PR.same_rows(cover, PR.placement_result(out[:2], base, e, roi, MEAN, STD, h + 1, w + 2))
    assert (cover[:, 0] == h * w).all() and np.isnan(cover[:, 5]).all() and np.isfinite(cover[:, 4]).all()
    assert int(tickets.abs().sum()) == 0


def test_result_unedited_sample_is_exactly_zero_and_validates(mau):
    P = mau.placement
    out, base, roi, edits = make_result_case(37, 45)
    out[1] = base                                                                      # a sample equal to the base, bit for bit
    got = P.result(dev(out), dev(base), edits, (PH, PW), MEAN, STD, roi=dev(roi)).cpu().numpy()
    assert (got[1, [1, 2, 3, 4, 5, 7, 8, 9, 10]].view(np.uint64) == 0).all()           # +0.0, not -0.0
    o, b = dev(out), dev(base)
    with pytest.raises(ValueError):
        P.result(o[:, :1], b, edits, (PH, PW), MEAN, STD)
    with pytest.raises(ValueError):
        P.result(o, b[:, :30], edits, (PH, PW), MEAN, STD)
    with pytest.raises(ValueError):
        P.result(o, b, edits[:4], (PH, PW), MEAN, STD)
    with pytest.raises(ValueError):
        P.result(o, b, edits, (0, PW), MEAN, STD)
    with pytest.raises(ValueError):
        P.result(o, b, edits, (PH, PW), MEAN, STD, roi=dev(roi)[:30])
    with pytest.raises(RuntimeError, match="no CPU"):
        P.result(torch.from_numpy(out), b, edits, (PH, PW), MEAN, STD)


def test_result_more_samples_than_tickets(mau):
    """One sample more than a ticket buffer covers: two launches, every row still its own."""
    P = mau.placement
    B = mau._lib.lib.mau_reduce_tickets_elems() + 1
    assert B <= 4096
    rng = np.random.default_rng(82)
    base = rng.standard_normal((2, 8, 8)).astype(np.float32)
    out = (base[None] + 0.1 * rng.standard_normal((B, 2, 8, 8))).astype(np.float32)
    roi = (rng.random((8, 8)) < 0.5).astype(np.uint8)
    edits = np.stack([rng.integers(-2, 8, B), rng.integers(-2, 8, B), rng.integers(0, 9, B)], axis=1).astype(np.int32)
    got = P.result(dev(out), dev(base), edits, (3, 2), MEAN, STD, roi=dev(roi)).cpu().numpy()
    assert PR.same_rows(got, PR.placement_result(out, base, edits, roi, MEAN, STD, 3, 2))
    alone = P.result(dev(out[B - 1:]), dev(base), edits[B - 1:], (3, 2), MEAN, STD, roi=dev(roi)).cpu().numpy()
    assert same_bits(alone, got[B - 1:])


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
TS, PATCH, BATCH, CLASSES = 32, 8, 5, [1, 6]


@pytest.fixture(scope="module")
def session_case(mau):
    """The small U-Net of the scenario and region tests in fp32, a 32 x 32 tile, and ONE sweep of the captured session: patch 8,
    stride 8, classes [1, 6] at batch 5 -- 32 edits, 7 replays, the last one ragged."""
    torch.manual_seed(5)
    net = mau.UrbanPredictor("unet", 23, 12, 16, 8, 16, 24, 2, base_filters=8, temporal_embeddings=False, metadata_embeddings=True)
    net = net.cuda().set_precision("fp32").eval()
    rng = np.random.default_rng(83)
    tile = tuple(dev(a) for a in make_tile(rng, TS, TS))
    roi = dev((rng.random((TS, TS)) < 0.3).astype(np.uint8))
    g = torch.Generator().manual_seed(6)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    kw = dict(metrics=METRICS, ncls=NCLS, patch=PATCH, batch=BATCH, roi=roi)
    sess = mau.PlacementSession(net, *tile, md, ts, **kw)
    first = sess.output.clone()                                                        # the all-baseline replay of the constructor
    return net, tile, roi, ts, md, kw, sess, first, sess(CLASSES, stride=8)


def test_session_baseline_samples_are_bit_identical(mau, session_case):
    """Checked first: every sample of the all-baseline replay is the same input, so the exact translation properties of the
    convolution forms say the ``batch`` outputs agree bit for bit -- the baseline may then be taken from sample 0."""
    _, _, _, _, _, _, sess, first, _ = session_case
    assert first.shape == (BATCH, 2, TS, TS) and bool(torch.isfinite(first).all())
    for b in range(1, BATCH):
        assert same_bits(first[b], first[0]), b
    assert same_bits(sess.base, first[0])


def test_session_rows_are_the_three_steps_composed_by_hand(mau, session_case):
    P = mau.placement
    net, tile, roi, ts, md, kw, sess, _, r = session_case
    assert r.rows.shape == (32, 12) and r.rows.dtype == np.float64 and r.edits.shape == (32, 3) and r.edits.dtype == np.int32
    assert r.ys.tolist() == r.xs.tolist() == [0, 8, 16, 24] and r.classes.tolist() == CLASSES
    assert np.array_equal(r.edits, P.edits_table(r.ys, r.xs, CLASSES)) and (r.rows[:, 0] == 64).all() and (r.rows[:, 11] == 0).all()
    assert (r.rows[:, 6] == float(roi.count_nonzero())).all() and np.isfinite(r.rows).all()
    assert np.abs(r.rows[:, 4]).max() > 0 and len({v for v in r.rows[:, 1]}) > 16                                   # the stamps do act
    tsb, mdb = ts.expand(BATCH, -1).contiguous(), md.expand(BATCH, -1).contiguous()
    pad = np.array([[0, 0, -1]], dtype=np.int32)
    for k0 in range(0, 32, BATCH):
        e = np.concatenate([r.edits[k0:k0 + BATCH], np.repeat(pad, max(0, k0 + BATCH - 32), 0)])
        with torch.no_grad():
            out = net(P.pack(*tile[:1], None, *tile[1:], e, PATCH, NCLS, METRICS, torch.float32), tsb, mdb)
            rows = P.result(out, sess.base, e, PATCH, MEAN, STD, roi=roi).cpu().numpy()
        valid = min(BATCH, 32 - k0)
        assert same_bits(rows[:valid], r.rows[k0:k0 + valid]), k0
        for b in range(valid, BATCH):                                                  # a row with cls = -1: exactly +0.0
            assert (rows[b, [1, 2, 3, 8]].view(np.uint64) == 0).all() and rows[b, 0] == 64
    # the unedited forecast is the base, un-normalised by the rule of mau_scenario_result
    base = sess.base.cpu().numpy()
    assert np.array_equal(r.ndvi.view(np.uint32), base[0].view(np.uint32))
    assert np.array_equal(r.temp_c.view(np.uint32), ((base[1] * np.float32(STD)).astype(np.float32) + np.float32(MEAN)).view(np.uint32))


def test_session_repeats_and_the_eager_session_gives_the_same_bits(mau, session_case):
    net, tile, _, ts, md, kw, sess, _, r = session_case
    again = sess(CLASSES, stride=8)
    assert same_bits(again.rows, r.rows) and np.array_equal(again.edits, r.edits)
    by_origins = sess(CLASSES, origins=([0, 8, 16, 24], [0, 8, 16, 24]))
    assert same_bits(by_origins.rows, r.rows)
    eager = mau.PlacementSession(net, *tile, md, ts, graph=False, **kw)
    assert eager.graph is None and same_bits(eager.base, sess.base)
    re = eager(CLASSES, stride=8)
    assert same_bits(re.rows, r.rows) and np.array_equal(re.ndvi, r.ndvi) and np.array_equal(re.temp_c, r.temp_c)
    # grid and best are numpy on rows
    for ci, c in enumerate(CLASSES):
        for entry in (1, 4, 7):
            assert np.array_equal(r.grid(c, entry), r.rows[16 * ci:16 * ci + 16, entry].reshape(4, 4))
        k = 16 * ci + int(np.argmin(r.rows[16 * ci:16 * ci + 16, 1]))
        assert r.best(c) == (int(r.edits[k, 0]), int(r.edits[k, 1]), float(r.rows[k, 1]))
    for bad in (dict(classes=[9]), dict(classes=[-1]), dict(classes=[]), dict(classes=[1], stride=0), dict(classes=[1], origins=([25], [0])),
                dict(classes=[1], stride=8, origins=([0], [0]))):
        with pytest.raises(ValueError):
            sess(**bad)
    for bad in (dict(patch=33), dict(batch=0), dict(ncls=17), dict(patch=0)):
        with pytest.raises(ValueError):
            mau.PlacementSession(net, *tile, md, ts, **{**kw, **bad})
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.PlacementSession(net, tile[0].cpu(), *tile[1:], md, ts, **kw)
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.PlacementSession(net, *tile, md.cpu(), ts, **kw)


def test_session_against_two_batch_one_forwards(mau, session_case):
    """The temperature change of two placements rebuilt from eager forwards at batch 1 (the stamped tile, the unedited tile):
    another inference form of the convolution may run there, so the bar is 1e-3 of the max-norm of the two temperature maps."""
    P = mau.placement
    net, tile, roi, ts, md, kw, sess, _, r = session_case

    def temp_map(edit):
        with torch.no_grad():
            o = net(P.pack(*tile[:1], None, *tile[1:], np.asarray([edit], dtype=np.int32), PATCH, NCLS, METRICS, torch.float32), ts, md)
        return o[0, 1].double().cpu().numpy() * STD + MEAN

    t0 = temp_map([0, 0, -1])
    inr = roi.cpu().numpy() != 0
    for k in (5, 27):
        t1 = temp_map(r.edits[k])
        d = t1 - t0
        bar = 1e-3 * max(np.abs(t0).max(), np.abs(t1).max())
        m = P.stamp_mask(r.edits[k], (TS, TS), PATCH)
        want = {1: d.mean(), 2: d.min(), 3: d.max(), 4: d[m].mean(), 5: d[~m].mean(), 7: d[inr].mean()}
        err = {e: abs(r.rows[k, e] - v) for e, v in want.items()}
        print(f"placement session fp32, edit {k}: batch 5 against two batch-1 forwards, |difference| per entry {err}, bar {bar:.3e}")
        assert max(err.values()) <= bar, (k, err, bar)
        assert np.abs(d).max() > 0                                                     # the stamp does act


# --------------------------------------------------------------------------- #
# the command line
# --------------------------------------------------------------------------- #
def test_command_line(mau, tmp_path):
    """``python -m mau_amd.placement`` in a fresh process on a tiny checkpoint and a 32 x 32 tile: the arrays it writes against a
    direct session call."""
    from mau_amd import checkpoint as C
    S = mau.scenario
    torch.manual_seed(7)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "temporal_embeddings": False, "metadata_embeddings": True}
    net = mau.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    ck = str(tmp_path / "tiny.pth")
    C.save_checkpoint(ck, net, None, epoch=0, step=0, loss=0.0, hyperparameters=hyper, model_type="unet", study_name="s", trial_id=0,
                      metadata_input_length=8)
    rng = np.random.default_rng(84)
    dw, rgb, ndvi, temp = make_tile(rng, TS, TS)
    roi = rng.random((TS, TS)) < 0.3
    raw = np.array([48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9], dtype=np.float64)
    series = rng.standard_normal(12)
    tile_path, roi_path, out_path = str(tmp_path / "tile.npz"), str(tmp_path / "roi.npy"), str(tmp_path / "out.npz")
    np.savez(tile_path, dw=dw, rgb=rgb, ndvi=ndvi, temp=temp, metadata_raw=raw, temp_series=series)
    np.save(roi_path, roi)
    mj = str(tmp_path / "metrics.json")
    with open(mj, "w") as f:
        json.dump(METRICS, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "mau_amd.placement", ck, "--tile", tile_path, "--metrics-json", mj, "--classes", "1,6", "--patch", "8",
           "--stride", "8", "--batch", "5", "--roi", roi_path, "--precision", "fp16"]
    p = subprocess.run(cmd + ["--output", out_path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "2 classes x 4 x 4 stamps of 8, 7 batches of 5" in p.stdout and "class 1: lowest mean_dt" in p.stdout and "class 6: lowest mean_dt" in p.stdout
    assert "Saved placement result" in p.stdout
    got = np.load(out_path)
    assert set(got.files) == {"rows", "edits", "classes", "ys", "xs", "ndvi", "temp_c", "best", *(f"grid_c{c}_e{e}" for c in (1, 6) for e in (1, 4, 7))}
    model = C.load_model(ck, device="cuda", spatial_channels=23, seq_len=12).set_precision("fp16")
    sess = mau.PlacementSession(model, dev(dw), dev(rgb), dev(ndvi), dev(temp), dev(S.metadata_row(*raw, METRICS["meta_mean"], METRICS["meta_std"])),
                                dev(S.normalize_temp_series(series, METRICS)), metrics=METRICS, patch=8, batch=5, roi=dev(roi.astype(np.uint8)))
    direct = sess([1, 6], stride=8)
    assert got["rows"].shape == (32, 12) and np.array_equal(got["rows"].view(np.uint64), direct.rows.view(np.uint64))
    assert np.array_equal(got["edits"], direct.edits) and got["ys"].tolist() == got["xs"].tolist() == [0, 8, 16, 24]
    assert np.array_equal(got["ndvi"].view(np.uint32), direct.ndvi.view(np.uint32)) and np.array_equal(got["temp_c"].view(np.uint32), direct.temp_c.view(np.uint32))
    for c in (1, 6):
        for e in (1, 4, 7):
            assert np.array_equal(got[f"grid_c{c}_e{e}"], direct.grid(c, e))
    assert np.array_equal(got["best"], np.array([direct.best(1), direct.best(6)], dtype=np.float64))
    assert (got["rows"][:, 6] == roi.sum()).all()
    bad = subprocess.run(cmd + ["--device", "cpu"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert bad.returncode != 0
