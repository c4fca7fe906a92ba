"""GPU tests of ``mau_amd.scenario``: ``mau_scenario_pack`` against the host truth (``prepare_input_host`` through
``data.pack_tiles``, bit for bit), ``mau_scenario_result`` against the float32 numpy spelling of the app, ``ScenarioSession``
against the eager path on both model types, and the command line.

Bounds.  Class maps, packed inputs, ``ndvi``, ``temp_c``, ``delta``, minima, maxima and counts are compared exactly.  The two
means are fp64 sums of n = H * W float32 values divided once: against numpy's float64 mean of the same values they may differ
by the first-order error bound of a length-n fp64 sum, n * 2^-52 * mean|delta| (the kernel's own tree is about 30 additions
deep, numpy's pairwise sum shallower still; the bound is the issue's)."""
import json
import os

import numpy as np
import pytest
import torch

from tests._helpers import bits, dev, mau, palette, same_bits  # noqa: F401
from tests.test_scenario_host import METRICS, make_canvas, make_tile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 300                    # more than one 256-thread block along x, with a ragged tail
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def tile():
    """One base tile (host arrays) and its normalised planes, shared and never written."""
    from mau_amd import scenario as S
    dw, rgb, ndvi, temp = make_tile(np.random.default_rng(10), H, W)
    return dw, rgb, ndvi, temp, S.normalized_planes_host(rgb, ndvi, temp, METRICS)


def device_pack(S, tile, canvases, palette, dtype):
    dw, rgb, ndvi, temp, _ = tile
    return S.pack(dev(dw), dev(rgb), dev(ndvi), dev(temp), dev(canvases), palette, METRICS, dtype)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("canvas_shape", [(53, 41), (600, 91)], ids=["upsampled", "downsampled"])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_pack_matches_host_truth_bit_for_bit(mau, palette, tile, prec, canvas_shape, N):
    S = mau.scenario
    dw, rgb, ndvi, temp, cont = tile
    rng = np.random.default_rng(20 + N)
    canvases = np.stack([make_canvas(rng, *canvas_shape, palette) for _ in range(N)])
    x, dw_t2 = device_pack(S, tile, canvases if N > 1 else canvases[0], palette, DTYPES[prec])
    want_t2 = np.stack([S.canvas_to_dw_map_host(c, (H, W), palette, dw) for c in canvases])
    assert dw_t2.dtype == torch.uint8 and np.array_equal(dw_t2.cpu().numpy(), want_t2)
    assert (want_t2 != dw[None]).mean() > 0.3                          # the canvases do edit the map
    ref = mau.data.pack_tiles(dev(np.repeat(dw[None], N, 0)), dev(want_t2), dev(np.repeat(cont[None], N, 0)), None, DTYPES[prec])
    assert x.C == ref.C == 23 and tuple(x.t.shape) == tuple(ref.t.shape) == (N, H, W, 24) and x.t.dtype == DTYPES[prec]
    assert torch.equal(bits(x.t), bits(ref.t))
    assert int((bits(x.t)[..., 23] != 0).sum()) == 0                   # the padding channel
    # ... and it is the dense tensor of prepare_input_host, rounded to the network's type
    dense = np.concatenate([S.prepare_input_host(dw, rgb, ndvi, temp, c, palette, METRICS) for c in canvases])
    assert torch.equal(x.t[..., :23].permute(0, 3, 1, 2), dev(dense).to(DTYPES[prec]))


def test_pack_transparent_and_opaque_canvases(mau, palette, tile):
    S = mau.scenario
    dw = tile[0]
    clear = np.zeros((2, 53, 41, 4), dtype=np.uint8)
    clear[..., :3] = 200                                               # colour without alpha paints nothing
    x, dw_t2 = device_pack(S, tile, clear, palette, torch.bfloat16)
    assert np.array_equal(dw_t2.cpu().numpy(), np.repeat(dw[None], 2, 0))
    assert torch.equal(x.t[..., :9], x.t[..., 14:23])
    solid = np.zeros((53, 41, 4), dtype=np.uint8)
    solid[..., :3], solid[..., 3] = palette[6], 1
    x, dw_t2 = device_pack(S, tile, solid, palette, torch.bfloat16)
    assert dw_t2.shape == (1, H, W) and int((dw_t2 != 6).sum()) == 0
    assert int((x.t[..., 14 + 6] != 1).sum()) == 0 and float(x.t[..., 14:23].float().sum()) == H * W
    with pytest.raises(RuntimeError, match="no CPU"):
        S.pack(torch.from_numpy(dw), dev(tile[1]), dev(tile[2]), dev(tile[3]), dev(solid), palette, METRICS)
    with pytest.raises(ValueError):
        device_pack(S, tile, solid[..., :3], palette, torch.bfloat16)


def result_truth(out, temp_orig, dw_t1, dw_t2):
    """The app's arithmetic on float32 arrays with Python-float scalars (processing_utils.py:179-181, Home.py:400-410)."""
    ndvi = out[:, 0]
    temp_c = (out[:, 1] * METRICS["temp_std"]) + METRICS["temp_mean"]
    assert temp_c.dtype == np.float32
    delta = None if temp_orig is None else temp_c - temp_orig[None]
    return ndvi, temp_c, delta, dw_t2 != dw_t1[None]


def check_result(r, out, temp_orig, dw_t1, dw_t2):
    ndvi, temp_c, delta, edited = result_truth(out, temp_orig, dw_t1, dw_t2)
    n = dw_t1.size
    assert np.array_equal(r.ndvi.cpu().numpy().view(np.uint32), ndvi.view(np.uint32))
    assert np.array_equal(r.temp_c.cpu().numpy().view(np.uint32), temp_c.view(np.uint32))
    stats = r.stats.cpu().numpy()
    assert stats.shape == (out.shape[0], 5) and stats.dtype == np.float64
    assert np.array_equal(stats[:, 3], edited.reshape(len(out), -1).sum(1).astype(np.float64))
    for name, col in (("mean_delta", 0), ("min_delta", 1), ("max_delta", 2), ("edited_pixels", 3), ("mean_delta_edited", 4)):
        assert torch.equal(getattr(r, name), r.stats[:, col])
    if temp_orig is None:
        assert r.delta is None and np.isnan(stats[:, [0, 1, 2, 4]]).all()
        return stats
    assert np.array_equal(r.delta.cpu().numpy().view(np.uint32), delta.view(np.uint32))
    for i in range(len(out)):
        d64 = delta[i].astype(np.float64)
        bound = n * 2.0 ** -52 * np.abs(d64).mean()
        err = abs(stats[i, 0] - d64.mean())
        if i < 3:
            print(f"scenario.result n={n} scenario {i}: |mean - m64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert stats[i, 1] == d64.min() and stats[i, 2] == d64.max()
        if edited[i].any():
            de = d64[edited[i]]
            assert abs(stats[i, 4] - de.mean()) <= de.size * 2.0 ** -52 * np.abs(de).mean()
        else:
            assert np.isnan(stats[i, 4])
    return stats


def make_result_case(N, h, w, seed):
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((N, 2, h, w)).astype(np.float32)
    temp_orig = rng.uniform(5, 55, (h, w)).astype(np.float32)
    dw_t1 = rng.integers(0, 9, (h, w)).astype(np.uint8)
    dw_t2 = np.where(rng.random((N, h, w)) < 0.4, rng.integers(0, 9, (N, h, w)), dw_t1[None]).astype(np.uint8)
    return out, temp_orig, dw_t1, dw_t2


def run_result(S, out, temp_orig, dw_t1, dw_t2):
    return S.result(dev(out), None if temp_orig is None else dev(temp_orig), dev(dw_t1), dev(dw_t2), METRICS["temp_mean"], METRICS["temp_std"])


# (37, 300): three chunks, the last one ragged; (5, 7): one partial chunk, fewer pixels than threads; (64, 64): one exact chunk
@pytest.mark.parametrize("N,h,w", [(1, H, W), (3, H, W), (2, 5, 7), (1, 64, 64)])
def test_result_matches_float32_numpy(mau, N, h, w):
    S = mau.scenario
    out, temp_orig, dw_t1, dw_t2 = make_result_case(N, h, w, 30 + N)
    r = run_result(S, out, temp_orig, dw_t1, dw_t2)
    stats = check_result(r, out, temp_orig, dw_t1, dw_t2)
    again = run_result(S, out, temp_orig, dw_t1, dw_t2)
    for a, b in ((r.stats, again.stats), (r.delta, again.delta), (r.temp_c, again.temp_c)):
        assert same_bits(a, b)                                         # two calls: identical bits
    if N > 1:                                                          # a scenario's row does not depend on its place in the batch
        solo = run_result(S, out[1:2], temp_orig, dw_t1, dw_t2[1:2]).stats.cpu().numpy()
        assert np.array_equal(solo[0].view(np.uint64), stats[1].view(np.uint64))


def test_result_without_original_and_without_edits(mau):
    S = mau.scenario
    out, temp_orig, dw_t1, dw_t2 = make_result_case(3, H, W, 40)
    check_result(run_result(S, out, None, dw_t1, dw_t2), out, None, dw_t1, dw_t2)
    same = np.repeat(dw_t1[None], 3, 0)                                # a transparent canvas: no edited pixel
    stats = check_result(run_result(S, out, temp_orig, dw_t1, same), out, temp_orig, dw_t1, same)
    assert (stats[:, 3] == 0).all() and np.isnan(stats[:, 4]).all() and np.isfinite(stats[:, :3]).all()
    with pytest.raises(ValueError):
        S.result(dev(out)[:, :1], dev(temp_orig), dev(dw_t1), dev(dw_t2), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        S.result(torch.from_numpy(out), dev(temp_orig), dev(dw_t1), dev(dw_t2), 0.0, 1.0)


def test_result_more_scenarios_than_tickets(mau):
    """More scenarios than one ticket buffer covers: several launches, every row still its own."""
    S = mau.scenario
    N = mau._lib.lib.mau_reduce_tickets_elems() + 3
    out, temp_orig, dw_t1, dw_t2 = make_result_case(N, 9, 11, 41)
    check_result(run_result(S, out, temp_orig, dw_t1, dw_t2), out, temp_orig, dw_t1, dw_t2)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
TH, TW, CH, CW = 48, 48, 64, 80


@pytest.mark.parametrize("model_type", ["unet", "unet++"])
def test_session_replays_the_eager_path(mau, palette, model_type):
    S = mau.scenario
    flags = {} if model_type == "unet++" else dict(temporal_embeddings=False, metadata_embeddings=True)
    torch.manual_seed(5)
    net = mau.UrbanPredictor(model_type, 23, 12, 16, 8, 16, 24, 2, base_filters=8, **flags).cuda().set_precision("fp16").eval()
    rng = np.random.default_rng(50)
    dw, rgb, ndvi, temp = (dev(a) for a in make_tile(rng, TH, TW))
    g = torch.Generator().manual_seed(6)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    c1, c2 = make_canvas(rng, CH, CW, palette), make_canvas(rng, CH, CW, palette, transparent=0.6)
    temp_orig = dev(rng.uniform(5, 55, (TH, TW)).astype(np.float32))
    kw = dict(palette=palette, metrics=METRICS, canvas_shape=(CH, CW))
    sess = mau.ScenarioSession(net, dw, rgb, ndvi, temp, md, ts, temp_orig=temp_orig, **kw)

    def eager(canvases):
        n = 1 if canvases.ndim == 3 else len(canvases)
        with torch.no_grad():
            x, t2 = S.pack(dw, rgb, ndvi, temp, dev(canvases), palette, METRICS, torch.float16)
            return S.result(net(x, ts.expand(n, -1).contiguous(), md.expand(n, -1).contiguous()), temp_orig, dw, t2,
                            METRICS["temp_mean"], METRICS["temp_std"])

    def assert_same(r, e):
        for name in ("ndvi", "temp_c", "delta", "stats"):
            assert same_bits(getattr(r, name), getattr(e, name)), name
        assert torch.equal(r.dw_t2, e.dw_t2)

    r1, e1 = sess(c1), eager(c1)
    assert_same(r1, e1)
    assert np.array_equal(r1.dw_t2.cpu().numpy()[0], S.canvas_to_dw_map_host(c1, (TH, TW), palette, dw.cpu().numpy()))
    r2 = sess(dev(c2))                                                 # a device canvas
    assert_same(r2, eager(c2))
    assert not torch.equal(r2.dw_t2, r1.dw_t2) and not same_bits(r2.temp_c, r1.temp_c) and not same_bits(r2.stats, r1.stats)
    assert_same(sess(c1), r1)                                          # the first canvas again: the first result, bit for bit
    assert float(r1.edited_pixels[0]) == float((r1.dw_t2[0] != dw).sum()) > 0
    # temp_orig=None: the change is taken against the tile's own temperature plane
    sess0 = mau.ScenarioSession(net, dw, rgb, ndvi, temp, md, ts, clone_output=False, **kw)
    r0 = sess0(c1)
    assert same_bits(r0.temp_c, r1.temp_c) and same_bits(r0.delta, r1.temp_c - temp) and r0.delta.data_ptr() == sess0(c2).delta.data_ptr()
    # two scenarios per replay: the class maps and the edited counts of two single sessions; the outputs of the eager
    # forward at batch 2 (a layer's K-group form, and with it the last bits, may differ between batch 1 and batch 2)
    sess2 = mau.ScenarioSession(net, dw, rgb, ndvi, temp, md, ts, temp_orig=temp_orig, scenarios=2, **kw)
    both = np.stack([c1, c2])
    rb = sess2(both)
    assert torch.equal(rb.dw_t2, torch.cat([r1.dw_t2, r2.dw_t2])) and torch.equal(rb.stats[:, 3], torch.cat([r1.stats[:, 3], r2.stats[:, 3]]))
    assert_same(rb, eager(both))
    with pytest.raises(ValueError):
        sess(np.zeros((CH, CW + 1, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        sess2(c1)
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.ScenarioSession(net, dw.cpu(), rgb, ndvi, temp, md, ts, **kw)
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.ScenarioSession(net, dw, rgb, ndvi, temp, md.cpu(), ts, **kw)


def test_command_line(mau, palette, tmp_path):
    """``python -m mau_amd.scenario``'s typer application on a tiny checkpoint and a 32 x 32 tile: the arrays it writes, and its
    statistics against a direct session call."""
    from typer.testing import CliRunner
    from mau_amd import checkpoint as C
    S = mau.scenario
    torch.manual_seed(7)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "temporal_embeddings": False, "metadata_embeddings": True}
    net = mau.UrbanPredictor("unet", 23, 12, 8, 8, 8, 12, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    ck = str(tmp_path / "tiny.pth")
    C.save_checkpoint(ck, net, None, epoch=0, step=0, loss=0.0, hyperparameters=hyper, model_type="unet", study_name="s", trial_id=0,
                      metadata_input_length=8)
    rng = np.random.default_rng(60)
    dw, rgb, ndvi, temp = make_tile(rng, 32, 32)
    canvas = make_canvas(rng, 40, 40, palette)
    raw = np.array([48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9], dtype=np.float64)
    series = rng.standard_normal(12)
    tile_path, out_path = str(tmp_path / "tile.npz"), str(tmp_path / "out.npz")
    np.savez(tile_path, dw=dw, rgb=rgb, ndvi=ndvi, temp=temp, canvas=canvas, metadata_raw=raw, temp_series=series)
    mj = str(tmp_path / "metrics.json")
    with open(mj, "w") as f:
        json.dump(METRICS, f)
    pj = os.path.join(ROOT, "tests", "golden", "dw_palette.json")
    res = CliRunner().invoke(S._cli(), [ck, "--tile", tile_path, "--palette-json", pj, "--metrics-json", mj, "--precision", "fp16", "--output", out_path])
    assert res.exit_code == 0, res.output
    assert "scenario 0: mean_delta" in res.output and "Saved scenario result" in res.output
    got = np.load(out_path)
    for name in ("ndvi", "temp_c", "delta", "dw_t2"):
        assert got[name].shape == (1, 32, 32), name
    assert got["stats"].shape == (1, 5) and got["dw_t2"].dtype == np.uint8 and got["temp_c"].dtype == np.float32
    assert np.array_equal(got["dw_t2"][0], S.canvas_to_dw_map_host(canvas, (32, 32), palette, dw))
    model = C.load_model(ck, device="cuda", spatial_channels=23, seq_len=12).set_precision("fp16")
    sess = mau.ScenarioSession(model, dev(dw), dev(rgb), dev(ndvi), dev(temp), dev(S.metadata_row(*raw, METRICS["meta_mean"], METRICS["meta_std"])),
                               dev(S.normalize_temp_series(series, METRICS)), palette=palette, metrics=METRICS, canvas_shape=(40, 40))
    direct = sess(canvas)
    assert np.array_equal(got["stats"].view(np.uint64), direct.stats.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["mean_delta"], got["stats"][:, 0]) and np.array_equal(got["temp_c"], direct.temp_c.cpu().numpy())
    bad = CliRunner().invoke(S._cli(), [ck, "--tile", tile_path, "--palette-json", pj, "--metrics-json", mj, "--device", "cpu"])
    assert bad.exit_code != 0
