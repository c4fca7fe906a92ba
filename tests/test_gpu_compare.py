"""GPU tests of ``mau_amd.compare``: ``mau_compare_result`` and ``mau_compare_inputs`` against their host twins,
``ComparisonSession`` against the eager path on a ``unet`` with 4 and a ``unet++`` with 8 metadata features, and the command line.

Shapes.  (7, 9): one partial chunk, 4-byte loads, four unequal quadrants.  (67, 63): H * W % 4 != 0, two chunks, the chunk
boundary (pixel 4096 = row 65, column 1) inside a row that goes on to cross the column split.  (250, 250): 16-byte loads, 16
chunks of which the last is partial (1060 pixels) -- the workload's own shape.  33 models at (5, 7): 66 rows, more than one
ticket buffer covers, two launches.

Bounds.  ``pred``, ``gt``, ``err`` and entries 0-5 of every region (count, the four range ends, max |err|) are compared bit for
bit.  Entries 6 and 7 are fp64 sums of n <= 62 500 non-negative terms: summed in any order they differ from the exact sum by at
most (n - 1) * 2^-53 relative, so two orders differ by less than 1e-11 relative; that is the bound, derived and not measured."""
import json
import os

import numpy as np
import pytest
import torch

from tests._helpers import bits, dev, mau, palette, same_bits  # noqa: F401
from tests.test_compare_host import make_outputs, make_sample
from tests.test_scenario_host import METRICS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 9), (67, 63), (250, 250)]
REL = 1e-11


@pytest.fixture(scope="module")
def cases():
    """Per shape: three heads' outputs, the target and the host twin's answer for all three, computed once and never written."""
    from mau_amd import compare as C
    made = {}
    for i, (H, W) in enumerate(SHAPES):
        out, tgt = make_outputs(np.random.default_rng(200 + i), 3, H, W)
        made[(H, W)] = (out, tgt, C.compare_host(out, tgt, METRICS))
    return made


def run_result(C, out, tgt, tickets=None):
    return C.result(dev(out), dev(tgt), METRICS["temp_mean"], METRICS["temp_std"], tickets)


def check_against_host(r, host, label):
    pred, gt, err, rows = host
    for name, want in (("pred", pred), ("gt", gt), ("err", err)):
        assert np.array_equal(bits(getattr(r, name).cpu().numpy()), bits(want)), (label, name)
    got = r.stats.rows.cpu().numpy()
    assert got.shape == rows.shape and got.dtype == np.float64
    got, rows = got.reshape(-1, 5, 8), rows.reshape(-1, 5, 8)
    assert np.array_equal(bits(got[..., :6]), bits(rows[..., :6])), label
    diff, size = np.abs(got[..., 6:] - rows[..., 6:]), rows[..., 6:]
    worst = float((diff[size > 0] / size[size > 0]).max()) if (size > 0).any() else 0.0
    print(f"compare.result {label}: largest relative difference of the sums {worst:.3e}, bound {REL:.0e}")
    assert (diff <= REL * size).all(), (label, worst)                  # (a sum of zeros is zero on both sides)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_result_matches_the_host_twin(mau, cases, shape, M):
    C = mau.compare
    out, tgt, (pred, gt, err, rows) = cases[shape]
    tickets = torch.zeros(mau._lib.lib.mau_reduce_tickets_elems(), dtype=torch.int32, device="cuda")
    r = run_result(C, out[:M], tgt, tickets)
    check_against_host(r, (pred[:M], gt, err[:M], rows[:2 * M]), f"{shape} M={M}")
    assert int(tickets.abs().sum()) == 0                               # the ticket buffer is left zeroed
    again = run_result(C, out[:M], tgt, tickets)                       # two calls: identical bits
    for a, b in ((r.stats.rows, again.stats.rows), (r.pred, again.pred), (r.gt, again.gt), (r.err, again.err)):
        assert same_bits(a, b)
    assert int(tickets.abs().sum()) == 0
    # the named views and the page's derived numbers
    t = r.stats.table
    assert tuple(t.shape) == (M, 2, 5, 8) and torch.equal(r.stats.region("top_right"), t[:, :, 2]) and torch.equal(r.stats.gt_max, t[..., 2])
    assert torch.equal(r.stats.vmin, torch.minimum(t[..., 1], t[..., 3])) and torch.equal(r.stats.vmax, torch.maximum(t[..., 2], t[..., 4]))
    assert torch.equal(r.stats.err_max_abs, t[..., 5]) and torch.equal(r.stats.mae, t[..., 6] / t[..., 0])
    assert torch.equal(r.stats.rmse, torch.sqrt(t[..., 7] / t[..., 0]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_do_not_depend_on_the_number_of_models_or_the_place(mau, cases, shape):
    C = mau.compare
    out, tgt, _ = cases[shape]
    all3 = run_result(C, out, tgt)
    for m in range(3):
        solo = run_result(C, out[m:m + 1], tgt)
        assert same_bits(solo.stats.rows, all3.stats.rows[2 * m:2 * m + 2]), m
        assert same_bits(solo.pred[0], all3.pred[m]) and same_bits(solo.err[0], all3.err[m]) and same_bits(solo.gt, all3.gt)


def test_result_issues_one_launch_and_refuses_bad_arguments(mau, cases, monkeypatch):
    C = mau.compare
    out, tgt, _ = cases[(7, 9)]
    calls = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    assert 3 * 2 <= mau._lib.lib.mau_reduce_tickets_elems()
    run_result(C, out, tgt)
    assert calls == ["mau_compare_result"]
    with pytest.raises(ValueError):
        C.result(dev(out)[:, :1], dev(tgt), 0.0, 1.0)
    with pytest.raises(ValueError):
        C.result(dev(out), dev(tgt)[:, :-1], 0.0, 1.0)
    with pytest.raises(TypeError):
        C.result(dev(out).double(), dev(tgt), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        C.result(torch.from_numpy(out), dev(tgt), 0.0, 1.0)


def test_result_more_rows_than_tickets(mau):
    """66 rows: two launches that share one workspace; every row is still its own, and a perfect prediction gives the range 1."""
    C = mau.compare
    M = mau._lib.lib.mau_reduce_tickets_elems() // 2 + 1
    out, tgt = make_outputs(np.random.default_rng(210), M, 5, 7)
    out[M - 1] = tgt
    r = run_result(C, out, tgt)
    check_against_host(r, C.compare_host(out, tgt, METRICS), f"M={M}")
    assert (r.stats.err_max_abs[M - 1] == 1).all() and (r.stats.max_abs_err[M - 1] == 0).all() and (r.stats.err_max_abs[:M - 1] != 1).all()


def test_nan_is_skipped_by_ranges_and_carried_by_sums(mau):
    C = mau.compare
    out, tgt = make_outputs(np.random.default_rng(211), 2, 67, 63)
    out[1, 1, 66, 62], tgt[0, 0, 0] = np.nan, np.nan                   # bottom-right of one model; top-left of the NDVI target
    r = run_result(C, out, tgt)
    got, want = r.stats.rows.cpu().numpy().reshape(4, 5, 8), C.compare_host(out, tgt, METRICS)[3].reshape(4, 5, 8)
    assert np.array_equal(bits(got[..., :6]), bits(want[..., :6])) and np.isfinite(got[..., :6]).all()
    assert np.array_equal(np.isnan(got[..., 6:]), np.isnan(want[..., 6:]))
    assert np.isnan(got[3, [0, 4], 6:]).all() and np.isnan(got[[0, 2]][:, [0, 1], 6:]).all() and np.isnan(got[..., 6:]).sum() == 12


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_views_match_the_host_twin(mau, palette, shape):
    C = mau.compare
    cls_a, cls_b, cont = make_sample(np.random.default_rng(220), *shape)
    cls_a[0, 0], cls_b[-1, -1], cls_b[0, 1] = 9, 255, 16               # ids the palette does not have
    cont[1, 2, 3] = np.nan
    got = C.input_views(dev(cls_a), dev(cls_b), dev(cont), palette, METRICS)
    want = C.input_views_host(cls_a, cls_b, cont, palette, METRICS)
    assert got._fields == C.VIEW_NAMES
    for name in C.VIEW_NAMES:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, name
        assert np.array_equal(bits(g), bits(want[name])), name
    assert not got.dw_t1_rgb[0, 0].any() and not got.dw_t2_rgb[-1, -1].any() and not got.dw_t2_rgb[0, 1].any()
    assert int(got.rgb8[2, 3, 1]) == 0
    with pytest.raises(ValueError):
        C.input_views(dev(cls_a), dev(cls_b), dev(cont)[:4], palette, METRICS)
    with pytest.raises(ValueError):
        C.input_views(dev(cls_a), dev(cls_b), dev(cont), np.zeros((17, 3), dtype=np.uint8), METRICS)
    with pytest.raises(RuntimeError, match="no CPU"):
        C.input_views(torch.from_numpy(cls_a), dev(cls_b), dev(cont), palette, METRICS)


# --------------------------------------------------------------------------- #
# the session
# --------------------------------------------------------------------------- #
EDGE, T = 48, 12


def make_compact_sample(seed, edge=EDGE, t=T):
    """One compact sample in the form ``FuturePredictionDataset`` yields (host tensors)."""
    rng = np.random.default_rng(seed)
    cls_a, cls_b, cont = make_sample(rng, edge, edge)
    g = torch.Generator().manual_seed(seed)
    return {"cls_a": torch.from_numpy(cls_a), "cls_b": torch.from_numpy(cls_b), "cont": torch.from_numpy(cont), "flip": False,
            "metadata": torch.randn(4, generator=g), "temp_series": torch.randn(t, generator=g),
            "t1_date": torch.tensor([2019.0, 3.0]), "t2_date": torch.tensor([2022.0, 9.0]),
            "target": torch.from_numpy(make_outputs(rng, 1, edge, edge)[1])}


def make_models(mau):
    torch.manual_seed(5)
    unet = mau.UrbanPredictor("unet", 23, T, 16, 4, 16, 24, 2, base_filters=8, temporal_embeddings=False, metadata_embeddings=True)
    unetpp = mau.UrbanPredictor("unet++", 23, T, 16, 8, 16, 24, 2, base_filters=8)
    return [("plain", unet.cuda().eval()), ("nested", unetpp.cuda().eval())]


def eager_outputs(mau, models, sample):
    """Each model's own eager forward on the packed tile, with the metadata row its checkpoint asks for: 4 values, or 4 and the dates."""
    md4 = sample["metadata"].reshape(1, 4).cuda()
    md8 = torch.cat([md4, sample["t1_date"].reshape(1, 2).cuda(), sample["t2_date"].reshape(1, 2).cuda()], dim=1)
    x = mau.data.pack_tiles(sample["cls_a"][None].cuda(), sample["cls_b"][None].cuda(), sample["cont"][None].cuda(), None, torch.float16)
    ts = sample["temp_series"].reshape(1, -1).cuda()
    with torch.no_grad():
        return torch.cat([model(x, ts, md8 if name == "nested" else md4) for name, model in models])


def assert_same_result(a, b):
    for name in ("pred", "gt", "err"):
        assert same_bits(getattr(a, name), getattr(b, name)), name
    assert same_bits(a.stats.rows, b.stats.rows)


def test_session_replays_the_eager_path(mau, palette):
    C = mau.compare
    models = make_models(mau)
    one, other = make_compact_sample(50), make_compact_sample(51)
    sess = mau.ComparisonSession(models, one, metrics=METRICS, palette=palette, precision="fp16")
    assert sess.names == ["plain", "nested"] and sess._n_meta == [4, 8] and sess.dtype == torch.float16

    def check(r, sample):
        outs = eager_outputs(mau, models, sample)
        host = outs.cpu().numpy()
        for m in range(2):                                             # the page's un-normalisation of that model's own output
            want = host[m].copy()
            want[1] = host[m, 1] * METRICS["temp_std"] + METRICS["temp_mean"]
            assert np.array_equal(bits(r.pred[m].cpu().numpy()), bits(want)), m
        assert_same_result(r, C.result(outs, sample["target"].cuda(), METRICS["temp_mean"], METRICS["temp_std"]))
        want = C.input_views_host(sample["cls_a"].numpy(), sample["cls_b"].numpy(), sample["cont"].numpy(), palette, METRICS)
        for name in C.VIEW_NAMES:
            assert np.array_equal(bits(getattr(r.views, name).cpu().numpy()), bits(want[name])), name

    r1 = sess()
    assert r1.names == ["plain", "nested"] and tuple(r1.pred.shape) == (2, 2, EDGE, EDGE) and tuple(r1.stats.rows.shape) == (4, 40)
    check(r1, one)
    assert not same_bits(r1.pred[0], r1.pred[1])
    assert_same_result(sess(), r1)                                     # a second replay: the same bits
    r2 = sess.set_sample(other)                                        # another tile: no new capture
    graph = sess.graph
    check(r2, other)
    assert not same_bits(r2.pred, r1.pred) and not same_bits(r2.gt, r1.gt) and sess.graph is graph
    fresh = mau.ComparisonSession(models, other, metrics=METRICS, palette=palette, precision="fp16", clone_output=False)
    f = fresh()
    assert_same_result(r2, f)
    assert f.pred.data_ptr() == fresh().pred.data_ptr()                # clone_output=False: the session's own buffers
    assert_same_result(sess.set_sample(one), r1)                       # and back: the first result, bit for bit
    with pytest.raises(ValueError):
        sess.set_sample(make_compact_sample(52, edge=EDGE + 16))
    with pytest.raises(ValueError):
        sess.set_sample(make_compact_sample(52, t=T + 1))
    with pytest.raises(ValueError):
        sess.set_sample({k: v for k, v in one.items() if k != "target"})
    assert_same_result(sess(), r1)                                     # a refused sample leaves the session as it was
    with pytest.raises(ValueError):
        mau.ComparisonSession([], one, metrics=METRICS)
    with pytest.raises(RuntimeError, match="no CPU"):
        mau.ComparisonSession([("host", mau.UrbanPredictor("unet", 23, T, 16, 4, 16, 24, 2, base_filters=8))], one, metrics=METRICS)
    models[0][1].set_precision("fp32")                                 # two compute types and no precision=: the tile is packed once
    with pytest.raises(ValueError, match="packed once"):
        mau.ComparisonSession(models, one, metrics=METRICS)


def test_command_line(mau, palette, tmp_path, capsys):
    """``python -m mau_amd.compare``'s body on a two-tile split and two checkpoints written with ``save_checkpoint``."""
    from mau_amd import checkpoint as CK
    from tests.test_eval_metrics_host import write_split
    C = mau.compare
    rng = np.random.default_rng(60)
    data = str(tmp_path / "processed")
    names = write_split(os.path.join(data, "test"), rng, [("Alpha", 0, (2019, 3), (2022, 9), None, T), ("Beta", 1, (2020, 2), (2023, 9), None, T)], H=32, W=32)
    paths = []
    torch.manual_seed(61)
    for model_type, n_meta in (("unet", 4), ("unet++", 8)):
        flags = dict(temporal_embeddings=model_type == "unet++", metadata_embeddings=True)
        net = mau.UrbanPredictor(model_type, 23, T, 8, n_meta, 8, 12, 2, base_filters=8, **flags)
        hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "batch_size": 1, **flags}
        paths.append(str(tmp_path / f"{model_type.replace('+', 'p')}.pth"))
        CK.save_checkpoint(paths[-1], net, None, epoch=1, step=2, loss=0.5, hyperparameters=hyper, model_type=model_type,
                           study_name="urban-predictor", trial_id=3, metadata_input_length=n_meta)
    mj, out_path = str(tmp_path / "metrics.json"), str(tmp_path / "out.npz")
    with open(mj, "w") as f:
        json.dump(METRICS, f)
    pj = os.path.join(ROOT, "tests", "golden", "dw_palette.json")
    assert C.main([*paths, "--processed-dir", data, "--filename", names[1], "--metrics-json", mj, "--palette-json", pj, "--precision", "fp16",
                   "--output", out_path]) == 0
    printed = capsys.readouterr().out.splitlines()
    got = np.load(out_path)
    assert set(got.files) >= {"pred", "gt", "err", "stats", "names", "rgb8", "temp_c", "ndvi", "dw_t1_rgb", "dw_t2_rgb"}
    assert got["pred"].shape == got["err"].shape == (2, 2, 32, 32) and got["gt"].shape == (2, 32, 32) and got["stats"].shape == (2, 2, 5, 8)
    assert list(got["names"]) == ["unet.pth", "unetpp.pth"] and got["rgb8"].shape == (32, 32, 3) and got["rgb8"].dtype == np.uint8
    assert str(got["tile"]) == names[1]
    lines = [ln for ln in printed if " mae " in ln]
    assert len(lines) == 4 and lines[0].startswith("unet.pth ndvi: mae ") and lines[3].startswith("unetpp.pth temp: mae ")
    stats = C.ComparisonStats(torch.from_numpy(got["stats"].reshape(4, 40)))
    for i, ln in enumerate(lines):
        m, c = divmod(i, 2)
        words = ln.split()
        for key, value in (("mae", stats.mae), ("rmse", stats.rmse), ("vmin", stats.vmin), ("vmax", stats.vmax), ("err_max_abs", stats.err_max_abs)):
            assert words[words.index(key) + 1] == f"{float(value[m, c, 0]):.6g}", (ln, key)
    # the same tile by index, through the body: the same arrays; and against a session built by hand
    res = C.compare_checkpoints(paths, data, index=1, metrics_json=mj, palette_json=pj, precision="fp16")
    for key in ("pred", "gt", "err", "stats", "rgb8", "dw_t2_rgb"):
        assert np.array_equal(bits(res[key]), bits(got[key])), key
    E = mau.evaluate
    models = [(os.path.basename(p), E.load_for_evaluation(p)[0]) for p in paths]
    sample = mau.data.FuturePredictionDataset("test", processed_dir=data)[1]
    direct = mau.ComparisonSession(models, sample, metrics=METRICS, palette=palette, precision="fp16")()
    assert np.array_equal(bits(direct.stats.numpy()), bits(got["stats"])) and np.array_equal(bits(direct.err.cpu().numpy()), bits(got["err"]))
    with pytest.raises(SystemExit):
        C.main([*paths, "--processed-dir", data, "--index", "0", "--metrics-json", mj, "--palette-json", pj, "--device", "cpu"])
    with pytest.raises(SystemExit):
        C.main([*paths, "--processed-dir", data, "--metrics-json", mj, "--palette-json", pj])          # neither --index nor --filename
    with pytest.raises(ValueError):
        C.compare_checkpoints(paths, data, index=5, metrics_json=mj, palette_json=pj)
