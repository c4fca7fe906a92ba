"""GPU tests of ``mau_amd.region``: ``mau_region_gather`` against the host truth (``data.pack_tiles`` on the cropped class maps and
``normalized_planes_host`` of the cropped raw planes, bit for bit) and against ``mau_scenario_pack``; ``mau_region_stitch``
against ``stitch_host``, bit for bit; ``RegionSession`` against the eager forward where the blend is exact, against
``stitch_host`` and the ``batch=1`` session where it is not; and the command line in a fresh process.

Bounds.  Everything is compared as bit patterns (``torch.equal`` on the exact session cases) except one figure: a window's output
at ``batch=5`` against the same window at ``batch=1`` -- the convolution's inference form depends on the launch shape
(DESIGN.md section 2), so the bar is the project's fp32 parity bar, 1e-3 of the window's max-norm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import bits, dev, mau, palette, same_bits  # noqa: F401
from tests.test_scenario_host import METRICS, make_tile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NCLS = 9


def make_region(rng, Hr, Wr, edited=1 / 3):
    """Raw planes of a region and an edited class map that differs from dw_t1 on about ``edited`` of the pixels."""
    dw, rgb, ndvi, temp = make_tile(rng, Hr, Wr)
    dw2 = np.where(rng.random((Hr, Wr)) < edited, (dw + rng.integers(1, NCLS, (Hr, Wr))) % NCLS, dw).astype(np.uint8)
    return dw, dw2, rgb, ndvi, temp


# --------------------------------------------------------------------------- #
# gather
# --------------------------------------------------------------------------- #
GH, GW, GT = 37, 45, 16                                    # H * W is no multiple of 4; a window is exactly one 256-pixel workgroup
ORIGINS = np.array([[0, 0], [GH - GT, GW - GT], [7, 13], [7, 13], [100, -4]], dtype=np.int32)      # corners, interior, duplicate, clamped
CLAMPED = [(0, 0), (GH - GT, GW - GT), (7, 13), (7, 13), (GH - GT, 0)]


@pytest.fixture(scope="module")
def gather_case(mau):
    """One region (host arrays, never written) and the cropped truth of the five windows."""
    dw, dw2, rgb, ndvi, temp = make_region(np.random.default_rng(70), GH, GW)
    assert 0.25 < (dw != dw2).mean() < 0.42
    crop = lambda a: np.stack([a[..., y:y + GT, x:x + GT] for y, x in CLAMPED])       # noqa: E731
    cont = np.stack([mau.scenario.normalized_planes_host(rgb[:, y:y + GT, x:x + GT], ndvi[y:y + GT, x:x + GT], temp[y:y + GT, x:x + GT], METRICS)
                     for y, x in CLAMPED])
    return (dw, dw2, rgb, ndvi, temp), (crop(dw), crop(dw2), cont)


@pytest.mark.parametrize("ld", [24, 32])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_gather_matches_host_truth_bit_for_bit(mau, gather_case, prec, ld):
    R, dt = mau.region, DTYPES[prec]
    (dw, dw2, rgb, ndvi, temp), (ca, cb, cont) = gather_case
    B = len(ORIGINS)
    ref = mau.data.pack_tiles(dev(ca), dev(cb), dev(cont), None, dt)
    assert ref.C == 23 and tuple(ref.t.shape) == (B, GT, GT, 24)
    x = R.gather(dev(dw), dev(dw2), dev(rgb), dev(ndvi), dev(temp), ORIGINS, GT, NCLS, METRICS, dt, ld=ld)
    assert x.C == 23 and tuple(x.t.shape) == (B, GT, GT, ld) and x.t.dtype == dt
    assert same_bits(x.t[..., :24], ref.t)
    assert int((bits(x.t)[..., 23:] != 0).sum()) == 0                                  # the padding channels are zero bits
    # the C entry point on an over-allocated, NaN-prefilled buffer with the origins as a device tensor: nothing beyond B*T*T*ld moves
    n, extra = B * GT * GT * ld, 4096
    buf = torch.full((n + extra,), float("nan"), dtype=dt, device="cuda")
    before = bits(buf).clone()
    t = [dev(a) for a in (dw, dw2, rgb, ndvi, temp)]
    from mau_amd._tile import norm_row
    norm = dev(norm_row(METRICS))
    mau._lib.call("mau_region_gather", *(v.data_ptr() for v in t), dev(ORIGINS).data_ptr(), norm.data_ptr(), buf.data_ptr(), ld,
                  mau.functional.dtype_code(dt), B, GT, GH, GW, NCLS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf)[:n].view(B, GT, GT, ld), bits(x.t)) and torch.equal(bits(buf)[n:], before[n:])
    # the dense view is gather_host's, rounded to the network's type
    dense = R.gather_host(dw, dw2, rgb, ndvi, temp, ORIGINS, GT, NCLS, METRICS)
    assert torch.equal(x.t[..., :23].permute(0, 3, 1, 2), dev(dense).to(dt))


def test_gather_equals_scenario_pack_and_validates(mau, gather_case, palette):
    R, S = mau.region, mau.scenario
    (dw, dw2, rgb, ndvi, temp), _ = gather_case
    y, x, T = 7, 13, 20                                     # 400 pixels per window: two workgroups, the second one ragged
    clear = np.zeros((8, 8, 4), dtype=np.uint8)
    for dt in (torch.bfloat16, torch.float32):
        want, t2 = S.pack(dev(dw[y:y + T, x:x + T]), dev(rgb[:, y:y + T, x:x + T]), dev(ndvi[y:y + T, x:x + T]),
                          dev(temp[y:y + T, x:x + T]), dev(clear), palette, METRICS, dt)
        got = R.gather(dev(dw), None, dev(rgb), dev(ndvi), dev(temp), dev(np.array([[y, x]], dtype=np.int32)), T, NCLS, METRICS, dt)
        assert same_bits(got.t, want.t) and got.C == want.C and torch.equal(t2[0], dev(dw[y:y + T, x:x + T]))
    args = (dev(dw), dev(dw2), dev(rgb), dev(ndvi), dev(temp))
    with pytest.raises(ValueError, match="ScenarioSession"):
        R.gather(*args, ORIGINS, 40, NCLS, METRICS)
    with pytest.raises(ValueError):
        R.gather(*args, ORIGINS, GT, NCLS, METRICS, ld=20)
    with pytest.raises(ValueError):
        R.gather(*args, ORIGINS, GT, 17, METRICS)
    with pytest.raises(ValueError):
        R.gather(*args, ORIGINS[:, :1], GT, NCLS, METRICS)
    with pytest.raises(RuntimeError, match="no CPU"):
        R.gather(torch.from_numpy(dw), *args[1:], ORIGINS, GT, NCLS, METRICS)


# --------------------------------------------------------------------------- #
# stitch
# --------------------------------------------------------------------------- #
def footprint(R, Hr, Wr, T, overlap, k):
    ys, xs = R.window_origins(Hr, T, overlap), R.window_origins(Wr, T, overlap)
    m = np.zeros((Hr, Wr), dtype=bool)
    m[ys[k // xs.size]:ys[k // xs.size] + T, xs[k % xs.size]:xs[k % xs.size] + T] = True
    return m


# ragged both ways with 16-byte stores impossible; small odd sizes; the aligned Wr % 4 == 0 path; a single window; and the aligned
# path with overlapping windows whose edges fall inside a thread's four pixels (xs = 0, 11, 22, 33, 36)
@pytest.mark.parametrize("Hr,Wr,T,overlap", [(70, 83, 32, 8), (41, 47, 16, 5), (64, 64, 32, 0), (32, 32, 32, 8), (40, 52, 16, 5)])
def test_stitch_matches_host_twin_bit_for_bit(mau, Hr, Wr, T, overlap):
    R = mau.region
    rng = np.random.default_rng(Hr + Wr)
    ys, xs, ramp = R.window_origins(Hr, T, overlap), R.window_origins(Wr, T, overlap), R.default_ramp(overlap)
    win = (rng.standard_normal((ys.size * xs.size, 2, T, T)) * 300).astype(np.float32)         # NOT cut from a field: the division works
    want = R.stitch_host(win, ys, xs, (Hr, Wr), ramp)
    got = R.stitch(dev(win), ys, xs, (Hr, Wr), ramp)
    assert got.shape == (2, Hr, Wr) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the C entry point on an over-allocated, NaN-prefilled buffer (16-byte aligned base: the wide stores where Wr % 4 == 0)
    n, extra = 2 * Hr * Wr, 4096
    buf = torch.full((n + extra,), float("nan"), dtype=torch.float32, device="cuda")
    before = bits(buf).clone()
    d = (dev(win), dev(ys), dev(xs))
    mau._lib.call("mau_region_stitch", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), buf.data_ptr(), 2, T, ramp, Hr, Wr, ys.size, xs.size,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf)[:n], bits(got).flatten()) and torch.equal(bits(buf)[n:], before[n:])
    if Wr % 4 == 0:                                         # a base that is 4-byte aligned only: the narrow stores, the same bits
        mau._lib.call("mau_region_stitch", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), buf.data_ptr() + 4, 2, T, ramp, Hr, Wr, ys.size,
                      xs.size, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(bits(buf)[1:n + 1], bits(got).flatten()) and torch.equal(bits(buf)[n + 1:], before[n + 1:])
    # a window of NaNs reaches exactly the pixels that window covers
    k = win.shape[0] // 2
    sick = win.copy()
    sick[k] = np.nan
    out = R.stitch(dev(sick), ys, xs, (Hr, Wr), ramp).cpu().numpy()
    mask = footprint(R, Hr, Wr, T, overlap, k)
    assert np.array_equal(np.isnan(out), np.broadcast_to(mask, out.shape))
    assert np.array_equal(out[:, ~mask].view(np.uint32), R.stitch_host(sick, ys, xs, (Hr, Wr), ramp)[:, ~mask].view(np.uint32))


def test_stitch_returns_a_cut_field_and_validates(mau):
    R = mau.region
    Hr, Wr, T, overlap = 70, 83, 32, 8
    rng = np.random.default_rng(71)
    field = (rng.standard_normal((2, Hr, Wr)) * 300).astype(np.float32)
    ys, xs = R.window_origins(Hr, T, overlap), R.window_origins(Wr, T, overlap)
    win = np.stack([field[:, y:y + T, x:x + T] for y in ys for x in xs])
    got = R.stitch(dev(win), ys, xs, (Hr, Wr), overlap)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), field.view(np.uint32))
    with pytest.raises(ValueError):
        R.stitch(dev(win), ys[::-1], xs, (Hr, Wr), overlap)
    with pytest.raises(ValueError):
        R.stitch(dev(win), ys, xs[:-1], (Hr, Wr), overlap)
    with pytest.raises(ValueError):
        R.stitch(dev(win)[:-1], ys, xs, (Hr, Wr), overlap)
    with pytest.raises(ValueError):
        R.stitch(dev(win), ys, xs, (Hr, Wr), 0)
    with pytest.raises(RuntimeError, match="no CPU"):
        R.stitch(torch.from_numpy(win), ys, xs, (Hr, Wr), overlap)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
def make_net(mau, model_type, prec, seed=5):
    flags = {} if model_type == "unet++" else dict(temporal_embeddings=False, metadata_embeddings=True)
    torch.manual_seed(seed)
    return mau.UrbanPredictor(model_type, 23, 12, 16, 8, 16, 24, 2, base_filters=8, **flags).cuda().set_precision(prec).eval()


def assert_result_of(S, r, temp_orig, dw):
    """ndvi, temp_c, delta and the statistics are scenario.result on the stitched map."""
    e = S.result(r.output, temp_orig, dw, r.dw_t2, METRICS["temp_mean"], METRICS["temp_std"])
    for name in ("ndvi", "temp_c", "delta", "stats"):
        assert same_bits(getattr(r, name), getattr(e, name)), name
    assert torch.equal(r.mean_delta, r.stats[:, 0]) and r.stats.shape == (1, 5)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("model_type", ["unet", "unet++"])
def test_session_exact_cases(mau, palette, model_type, prec):
    R, S = mau.region, mau.scenario
    net = make_net(mau, model_type, prec)
    g = torch.Generator().manual_seed(6)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    rng = np.random.default_rng(72)
    kw = dict(palette=palette, metrics=METRICS, window=32, batch=1)

    def forward(region, y, x):
        with torch.no_grad():
            a = R.gather(*region, torch.tensor([[y, x]], dtype=torch.int32, device="cuda"), 32, NCLS, METRICS, DTYPES[prec])
            return net(a, ts, md)

    # a region of exactly one window: the frozen model's eager forward on gather's Act
    dw, dw2, rgb, ndvi, temp = (dev(a) for a in make_region(rng, 32, 32))
    sess = mau.RegionSession(net, dw, rgb, ndvi, temp, md, ts, dw_t2=dw2, **kw)
    r = sess()
    assert (sess.windows, sess.ys.tolist(), sess.xs.tolist(), sess.overlap, sess.ramp) == (1, [0], [0], 8, 8)
    want = forward((dw, dw2, rgb, ndvi, temp), 0, 0)
    assert r.output.shape == (1, 2, 32, 32) and torch.equal(r.output, want) and torch.equal(r.window_outputs, want)
    assert torch.equal(r.dw_t2[0], dw2) and float(r.edited_pixels[0]) == float((dw2 != dw).sum()) > 0
    assert_result_of(S, r, temp, dw)                                                   # temp_orig=None: against the region's own raster
    # 64 x 64, no overlap: the four windows' forwards side by side
    dw, dw2, rgb, ndvi, temp = (dev(a) for a in make_region(rng, 64, 64))
    temp_orig = dev(rng.uniform(5, 55, (64, 64)).astype(np.float32))
    sess = mau.RegionSession(net, dw, rgb, ndvi, temp, md, ts, dw_t2=dw2, overlap=0, temp_orig=temp_orig, **kw)
    r = sess()
    assert (sess.windows, sess.ys.tolist(), sess.xs.tolist(), sess.ramp) == (4, [0, 32], [0, 32], 1)
    want = torch.empty(1, 2, 64, 64, device="cuda")
    for y in (0, 32):
        for x in (0, 32):
            want[:, :, y:y + 32, x:x + 32] = forward((dw, dw2, rgb, ndvi, temp), y, x)
    assert torch.equal(r.output, want) and r.window_outputs.shape == (4, 2, 32, 32)
    assert_result_of(S, r, temp_orig, dw)


def test_session_ragged_batch(mau, palette):
    R = mau.region
    net = make_net(mau, "unet", "fp32")
    Hr, Wr = 70, 83
    rng = np.random.default_rng(73)
    dw, dw2, rgb, ndvi, temp = (dev(a) for a in make_region(rng, Hr, Wr))
    g = torch.Generator().manual_seed(8)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(12, 8, generator=g).cuda()      # one metadata row per window, all different
    kw = dict(palette=palette, metrics=METRICS, window=32, overlap=8)
    sess = mau.RegionSession(net, dw, rgb, ndvi, temp, md, ts, dw_t2=dw2, batch=5, **kw)
    assert sess.windows == 12 and sess.ys.tolist() == [0, 24, 38] and sess.xs.tolist() == [0, 24, 48, 51] and sess._batches == 3
    r1 = sess()
    assert r1.window_outputs.shape == (12, 2, 32, 32) and r1.output.shape == (1, 2, Hr, Wr) and bool(torch.isfinite(r1.output).all())
    want = R.stitch_host(r1.window_outputs.cpu().numpy(), sess.ys, sess.xs, (Hr, Wr), sess.ramp)
    assert np.array_equal(r1.output[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    # window k against the batch=1 session: the project's fp32 parity bar
    one = mau.RegionSession(net, dw, rgb, ndvi, temp, md, ts, dw_t2=dw2, batch=1, **kw)()
    a, b = r1.window_outputs.double(), one.window_outputs.double()
    rel = ((a - b).abs().amax(dim=(1, 2, 3)) / b.abs().amax(dim=(1, 2, 3))).cpu().numpy()
    print(f"region session fp32, batch 5 against batch 1: max relative max-norm difference over 12 windows = {rel.max():.3e}")
    assert (rel <= 1e-3).all(), rel
    assert not same_bits(one.window_outputs[0], one.window_outputs[11])                # the windows (and their metadata rows) do differ
    # the per-window metadata rows are used: one row for the whole region gives the same first window and another last one
    whole = mau.RegionSession(net, dw, rgb, ndvi, temp, md[:1], ts, dw_t2=dw2, batch=1, **kw)().window_outputs
    assert same_bits(whole[0], one.window_outputs[0]) and not same_bits(whole[11], one.window_outputs[11])
    assert same_bits(sess().output, r1.output)                                         # a second call: identical bits
    r2 = sess(dw)                                                                      # a new edited map (here: no edit)
    assert not same_bits(r2.output, r1.output) and float(r2.edited_pixels[0]) == 0 and torch.equal(r2.dw_t2[0], dw)
    r3 = sess(dw2.cpu().numpy())                                                       # the old one again, as a host array
    assert same_bits(r3.output, r1.output) and same_bits(r3.stats, r1.stats) and same_bits(r3.window_outputs, r1.window_outputs)
    assert torch.equal(r1.dw_t2[0], dw2)                                               # an earlier result keeps its own class map
    with pytest.raises(ValueError):
        sess(dw[:-1])
    with pytest.raises(ValueError, match="ScenarioSession"):
        mau.RegionSession(net, dw, rgb, ndvi, temp, md[:1], ts, palette=palette, metrics=METRICS, window=96)
    with pytest.raises(ValueError):
        mau.RegionSession(net, dw, rgb, ndvi, temp, md[:5], ts, batch=5, **kw)
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.RegionSession(net, dw.cpu(), rgb, ndvi, temp, md, ts, **kw)


def test_command_line(mau, palette, tmp_path):
    """``python -m mau_amd.region`` in a fresh process on a tiny checkpoint and a 48 x 40 region: the arrays it writes against a
    direct session call."""
    from mau_amd import checkpoint as C
    S = mau.scenario
    torch.manual_seed(7)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "temporal_embeddings": False, "metadata_embeddings": True}
    net = mau.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    ck = str(tmp_path / "tiny.pth")
    C.save_checkpoint(ck, net, None, epoch=0, step=0, loss=0.0, hyperparameters=hyper, model_type="unet", study_name="s", trial_id=0,
                      metadata_input_length=8)
    Hr, Wr = 48, 40
    rng = np.random.default_rng(74)
    dw, dw2, rgb, ndvi, temp = make_region(rng, Hr, Wr)
    raw = np.array([48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9], dtype=np.float64)
    series = rng.standard_normal(12)
    region_path, out_path = str(tmp_path / "region.npz"), str(tmp_path / "out.npz")
    np.savez(region_path, dw=dw, dw_t2=dw2, rgb=rgb, ndvi=ndvi, temp=temp, metadata_raw=raw, temp_series=series)
    mj = str(tmp_path / "metrics.json")
    with open(mj, "w") as f:
        json.dump(METRICS, f)
    pj = os.path.join(ROOT, "tests", "golden", "dw_palette.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "mau_amd.region", ck, "--region", region_path, "--palette-json", pj, "--metrics-json", mj, "--window", "32",
           "--overlap", "8", "--batch", "3", "--precision", "fp16"]
    p = subprocess.run(cmd + ["--output", out_path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "2 x 2 windows of 32 (overlap 8, ramp 8), 2 batches of 3" in p.stdout and "region: mean_delta" in p.stdout
    assert "Saved region result" in p.stdout
    got = np.load(out_path)
    assert set(got.files) == {"output", "ndvi", "temp_c", "delta", "dw_t2", "stats", *S.STAT_NAMES, "ys", "xs", "window", "overlap", "ramp"}
    assert got["output"].shape == (1, 2, Hr, Wr) and got["output"].dtype == np.float32
    for name in ("ndvi", "temp_c", "delta", "dw_t2"):
        assert got[name].shape == (1, Hr, Wr), name
    assert got["stats"].shape == (1, 5) and np.array_equal(got["dw_t2"][0], dw2)
    assert got["ys"].tolist() == [0, 16] and got["xs"].tolist() == [0, 8] and (int(got["window"]), int(got["overlap"]), int(got["ramp"])) == (32, 8, 8)
    model = C.load_model(ck, device="cuda", spatial_channels=23, seq_len=12).set_precision("fp16")
    sess = mau.RegionSession(model, dev(dw), dev(rgb), dev(ndvi), dev(temp), dev(S.metadata_row(*raw, METRICS["meta_mean"], METRICS["meta_std"])),
                             dev(S.normalize_temp_series(series, METRICS)), palette=palette, metrics=METRICS, window=32, overlap=8, batch=3,
                             dw_t2=dev(dw2))
    direct = sess()
    assert np.array_equal(got["output"].view(np.uint32), direct.output.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["stats"].view(np.uint64), direct.stats.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["mean_delta"], got["stats"][:, 0]) and np.array_equal(got["temp_c"], direct.temp_c.cpu().numpy())
    bad = subprocess.run(cmd + ["--device", "cpu"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert bad.returncode != 0
