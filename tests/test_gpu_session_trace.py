"""The launch sequence of the captured sessions and of the two test-split drivers: every call through ``functional.call`` while a
session is built and used, or a driver walks a small split, compared call for call with ``tests/golden/session_trace.json`` -- recorded
by ``tests/golden/make_session_trace.py`` at the PARENT of a change that moves their host code around without changing what is
launched.  A call is encoded as in ``tests/test_gpu_launch_trace.py`` (``tests/_helpers.py``: scalars verbatim, pointers null or not,
the stream "main" or "side").  The warm-up runs on a side stream and a capture on the capture's own: both read "side"; a replay
launches through no ``call`` and leaves no row, the copies and launches around it do.

The drivers also write their CSV files; those are compared byte for byte with the files the parent wrote,
``tests/golden/session_trace_reports/``.

Shapes: the smallest the session tests use (test_gpu_model.py, test_gpu_scenario.py, test_gpu_compare.py, test_gpu_region.py,
test_gpu_statistics.py)."""
import filecmp
import importlib
import json
import os
import signal

import numpy as np
import pytest
import torch

from tests._helpers import dev, first_difference, mau, recorded_calls  # noqa: F401
from tests.test_eval_metrics_host import write_split
from tests.test_scenario_host import METRICS, load_palette, make_canvas, make_tile

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "session_trace.json")
GOLDEN_REPORTS = os.path.join(HERE, "golden", "session_trace_reports")
TIME_LIMIT = 120.0                                         # seconds for the whole file: a case is a few seconds
# the modules that bound ``call`` by name and launch in these cases
CALLERS = ("data", "scenario", "placement", "compare", "region", "evaluate", "statistics")

UNET = dict(temporal_embeddings=False, metadata_embeddings=True)
TRAIN_TILES = [("Alpha Town", 0, (2018, 3), (2020, 4), None, 12), ("Beta", 1, (2019, 1), (2021, 2), None, 9)]
# three tiles, batch size 2: a short last batch; two known cities in one group (a paired test needs two samples) and an unknown one
TEST_TILES = [("Alpha Town", 1, (2019, 1), (2021, 2), None, 12), ("Beta", 2, (2020, 6), (2022, 7), [6], 9),
              ("Gamma Ville", 0, (2024, 2), (2025, 3), None, 9)]
EVAL_METRICS = {"meta_mean": [20.0, 10.0, 3.0, 1.0], "meta_std": [15.0, 60.0, 2.0, 0.5], "temp_mean": 14.5, "temp_std": 8.25}
REPORTS = ("st_unet_metaemb_3_jobe_evaluation.csv", "st_unet_metaemb_3_jobe_info.csv", "st_unet_metaemb_3_jobc_evaluation.csv",
           "st_unet_metaemb_3_jobc_info.csv", "st_unet++_emb_4_jobc_evaluation.csv", "st_unet++_emb_4_jobc_info.csv", "st_paired_tests.csv")


def recording(mau):
    torch.cuda.synchronize()
    return recorded_calls(mau, [importlib.import_module("mau_amd." + name) for name in CALLERS])


def small_net(mau, model_type, n_meta=8, **flags):
    torch.manual_seed(5)
    flags = flags or ({} if model_type == "unet++" else UNET)
    return mau.UrbanPredictor(model_type, 23, 12, 16, n_meta, 16, 24, 2, base_filters=8, **flags).cuda().eval()


def graphed_inference(mau, work):
    """Construct, then two calls: other values in device tensors (one multi-tensor copy), then host tensors (plain copies)."""
    net = small_net(mau, "unet", temporal_embeddings=True, metadata_embeddings=True)
    g = torch.Generator().manual_seed(4)
    mk = lambda: (torch.randn(1, 23, 96, 96, generator=g).cuda(), torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda())  # noqa: E731
    a, b = mk(), mk()
    with recording(mau) as rows:
        sess = mau.GraphedInference(net, *a)
        sess(*b)
        sess(*(t.cpu() for t in a))
        torch.cuda.synchronize()
    return rows


def scenario_session(mau, work):
    """Construct, then one call from a host canvas and one from a device canvas."""
    palette = load_palette()
    net = small_net(mau, "unet").set_precision("fp16")
    rng = np.random.default_rng(50)
    dw, rgb, ndvi, temp = (dev(a) for a in make_tile(rng, 48, 48))
    g = torch.Generator().manual_seed(6)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    c1, c2 = make_canvas(rng, 64, 80, palette), dev(make_canvas(rng, 64, 80, palette, transparent=0.6))
    with recording(mau) as rows:
        sess = mau.ScenarioSession(net, dw, rgb, ndvi, temp, md, ts, palette=palette, metrics=METRICS, canvas_shape=(64, 80))
        sess(c1)
        sess(c2)
        torch.cuda.synchronize()
    return rows


def placement_session(mau, work):
    """48 x 48, 9 classes, stamps of 16 in batches of two, captured (``precision`` given) and eager; each: construct (the baseline
    replay included), a sweep of three placements -- one class over three origins: the last batch is ragged -- and a second call by
    stride, four placements in two whole batches."""
    net = small_net(mau, "unet")
    rng = np.random.default_rng(52)
    tile = tuple(dev(a) for a in make_tile(rng, 48, 48))
    roi = dev((rng.random((48, 48)) < 0.3).astype(np.uint8))
    g = torch.Generator().manual_seed(6)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    with recording(mau) as rows:
        for graph in (True, False):
            sess = mau.PlacementSession(net, *tile, md, ts, metrics=METRICS, ncls=9, patch=16, batch=2, roi=roi,
                                        precision="fp16" if graph else None, graph=graph)
            assert (sess.graph is not None) == graph and sess.dtype == torch.float16
            assert sess([1], origins=([0, 32, 16], [0])).rows.shape == (3, 12)
            assert sess([6], stride=32).rows.shape == (4, 12)
        torch.cuda.synchronize()
    return rows


def comparison_session(mau, work):
    """One 4-feature and one 8-feature model; construct, then ``set_sample``."""
    from tests.test_gpu_compare import make_compact_sample, make_models
    models = make_models(mau)
    one, other = make_compact_sample(50), make_compact_sample(51)
    with recording(mau) as rows:
        sess = mau.ComparisonSession(models, one, metrics=METRICS, palette=load_palette(), precision="fp16")
        sess.set_sample(other)
        torch.cuda.synchronize()
    return rows


def region_session(mau, work):
    """48 x 40 in windows of 32: two per axis, four in batches of three -- the last batch is ragged; construct, then one call with a
    host ``dw_t2``."""
    from tests.test_gpu_region import make_region
    net = small_net(mau, "unet").set_precision("fp16")
    dw, dw2, rgb, ndvi, temp = make_region(np.random.default_rng(74), 48, 40)
    g = torch.Generator().manual_seed(8)
    ts, md = torch.randn(1, 12, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    with recording(mau) as rows:
        sess = mau.RegionSession(net, dev(dw), dev(rgb), dev(ndvi), dev(temp), md, ts, palette=load_palette(), metrics=METRICS, window=32,
                                 overlap=8, batch=3)
        assert (sess.ys.tolist(), sess.xs.tolist(), sess._batches) == ([0, 16], [0, 8], 2)
        sess(dw2)
        torch.cuda.synchronize()
    return rows


def eval_drivers(mau, work):
    """``evaluate_checkpoint`` of one checkpoint, then ``statistics.compare_checkpoints`` of two, on a test split of three tiles with
    batch size 2; the reports go to ``work/reports`` (given as a relative path: ``*_info.csv`` holds the path it was given)."""
    from tests.test_gpu_statistics import make_checkpoint
    rng = np.random.default_rng(21)
    data = os.path.join(work, "processed")
    write_split(os.path.join(data, "train"), rng, TRAIN_TILES)
    write_split(os.path.join(data, "test"), rng, TEST_TILES)
    with open(os.path.join(data, "normalization_metrics.json"), "w") as f:
        json.dump(EVAL_METRICS, f)
    paths = [os.path.join(work, "a.pth"), os.path.join(work, "b.pth")]
    make_checkpoint(mau, paths[0], "unet", 8, 3, 22)
    make_checkpoint(mau, paths[1], "unet++", 4, 4, 23)
    kw = dict(batch_size=2, precision="fp32", study_name="st", output_dir="reports")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with recording(mau) as rows:
            mau.evaluate.evaluate_checkpoint(paths[0], data, jobid="e", **kw)
            mau.statistics.compare_checkpoints(paths, data, jobid="c", **kw)
            torch.cuda.synchronize()
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(os.path.join(work, "reports"))) == sorted(REPORTS)
    return rows


CASES = {"graphed_inference": graphed_inference, "scenario_session": scenario_session, "placement_session": placement_session,
         "comparison_session": comparison_session,
         "region_session": region_session, "eval_drivers": eval_drivers}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module", autouse=True)
def time_limit():
    """One alarm for the whole file."""
    def expired(signum, frame):
        raise TimeoutError(f"tests/test_gpu_session_trace.py ran past its {TIME_LIMIT:.0f} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.setitimer(signal.ITIMER_REAL, TIME_LIMIT)
    yield
    signal.setitimer(signal.ITIMER_REAL, 0)
    signal.signal(signal.SIGALRM, old)


def test_golden_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert all(len(rows) > 50 for rows in golden["cases"].values())
    assert sorted(os.listdir(GOLDEN_REPORTS)) == sorted(REPORTS)


@pytest.mark.parametrize("name", list(CASES))
def test_session_trace_matches_the_recorded_one(mau, golden, tmp_path, name):
    diff = first_difference(CASES[name](mau, str(tmp_path)), golden["cases"][name], name)
    assert diff is None, diff
    if name == "eval_drivers":
        for report in REPORTS:
            assert filecmp.cmp(os.path.join(str(tmp_path), "reports", report), os.path.join(GOLDEN_REPORTS, report), shallow=False), \
                f"{report} must be byte-identical to the recorded one"
