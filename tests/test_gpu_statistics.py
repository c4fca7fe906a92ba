"""GPU tests of ``mau_amd.statistics``: ``mau_eval_metrics_multi`` against ``mau_eval_metrics`` bit for bit, its independence of M
and of the model's place, ``mau_paired_accumulate`` against its float64 twin bit for bit, the refusals, and the command line on a
small test split against ``evaluate_checkpoint`` of each checkpoint alone."""
import csv
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import mau, same_bits  # noqa: F401
from tests.test_eval_metrics_host import write_split
from tests.test_statistics_host import HEAD, random_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, SHIFT = [1.0, 7.3], [0.0, 21.5]
# (62, 62): one chunk; (70, 70): two chunks, the last ragged; (33, 129): odd W, several chunks; (3, 5): fewer pixels than threads;
# (2, 4100): wider than a chunk, the target values are formed again per model
SHAPES = [(3, 5), (62, 62), (70, 70), (33, 129), (2, 4100)]


def make_case(M, B, C, H, W, ncls, seed):
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((M, B, C, H, W)).astype(np.float32)
    tgt = rng.standard_normal((B, C, H, W)).astype(np.float32)
    cls = rng.integers(0, ncls + 3, (B, H, W)).astype(np.uint8)   # class ids beyond ncls
    cls[0] = 3                                                   # one sample of a single class
    out[M - 1, 1, 0, H // 2, W // 3] = np.nan                    # one model's output holds a NaN and an inf
    out[M - 1, 2, 1, 0, W - 1] = np.inf
    return torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(cls).cuda()


# ---- 1. the multi kernel against the one-model kernel ------------------------------------------------------------
@pytest.mark.parametrize("ncls", [9, 16])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_multi_rows_are_the_single_kernels_bits(mau, M, ncls):
    S, E = mau.statistics, mau.evaluate
    for H, W in SHAPES:
        out, tgt, cls = make_case(M, 3, 2, H, W, ncls, 100 * M + H)
        rows = S.eval_metrics_multi(out, tgt, cls, SCALE, SHIFT, ncls)
        assert rows.shape == (M, 3, 2, HEAD + 3 * ncls)
        for m in range(M):
            want = E.eval_metrics(out[m], tgt, cls, SCALE, SHIFT, ncls).rows
            assert same_bits(rows[m], want), (M, ncls, H, W, m)
        assert rows[M - 1, 1, 0, 4] == 1 and rows[M - 1, 2, 1, 4] == 1 and torch.isnan(rows[M - 1, 1, 0, 0])
        assert rows[0, 0, 0, HEAD + 3] == H * W and rows[M - 1, 1, 1, 10] == int((cls[1] >= ncls).sum())


def test_multi_rows_do_not_depend_on_m_or_place(mau):
    S = mau.statistics
    out, tgt, cls = make_case(4, 3, 2, 70, 70, 9, 7)
    full = S.eval_metrics_multi(out, tgt, cls, SCALE, SHIFT)
    assert same_bits(full, S.eval_metrics_multi(out, tgt, cls, SCALE, SHIFT)), "a repeated call must agree bit for bit"
    perm = [2, 0, 3, 1]
    moved = S.eval_metrics_multi(out[perm].contiguous(), tgt, cls, SCALE, SHIFT)
    for at, m in enumerate(perm):
        assert same_bits(moved[at], full[m])
    alone = S.eval_metrics_multi(out[1:2].contiguous(), tgt, cls, SCALE, SHIFT)
    assert same_bits(alone[0], full[1])
    # more rows than one ticket buffer covers: several launches
    per = mau._lib.lib.mau_reduce_tickets_elems()
    B = per // 2 + 3
    rng = np.random.default_rng(8)
    o = torch.from_numpy(rng.standard_normal((2, B, 2, 8, 8)).astype(np.float32)).cuda()
    t = torch.from_numpy(rng.standard_normal((B, 2, 8, 8)).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.integers(0, 9, (B, 8, 8)).astype(np.uint8)).cuda()
    rows = S.eval_metrics_multi(o, t, c)
    for m in range(2):
        assert same_bits(rows[m], mau.evaluate.eval_metrics(o[m], t, c).rows)


# ---- 2. the table against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 8])
def test_paired_table_is_the_twins_bits(mau, M):
    S = mau.statistics
    rng = np.random.default_rng(40 + M)
    C, ncls = 2, 9
    r1, r2 = random_rows(rng, M, 5, C, ncls), random_rows(rng, M, 3, C, ncls)
    r1[M - 1, 1, 1, 1] = np.inf                                   # a non-finite sample: overall rmse of channel 1
    r2[0, 0, 0, HEAD + ncls + 2] = np.nan                         # and a class mae that is NaN although the class has pixels
    r2[:, 0, :, HEAD + 2] = 17
    g1, g2 = [4, 4, 1, 8, 4], [1, 200, 4]                         # ids 8 and 200 are dropped
    want = S.paired_accumulate_host(S.paired_accumulate_host(S.new_table(M, C, ncls), r1, g1, ncls), r2, g2, ncls)
    stats = S.PairedStats(M, C, ncls)
    stats.update(torch.from_numpy(r1).cuda(), torch.tensor(g1, dtype=torch.uint8).cuda())
    stats.update(torch.from_numpy(r2).cuda(), torch.tensor(g2, dtype=torch.uint8).cuda())
    two = stats.result()
    assert two.shape == want.shape and two.tobytes() == want.tobytes(), "the device table must have the twin's bits"
    one = S.PairedStats(M, C, ncls)
    one.update(torch.from_numpy(np.concatenate([r1, r2], axis=1)).cuda(), torch.tensor(g1 + g2, dtype=torch.uint8).cuda())
    assert one.result().tobytes() == two.tobytes(), "two batches must give the bits of one"
    assert two[4, 1, 1, 1] == 1 and two[1, 0, 4 + 2 * 2, 1] == 1 and two[4, 0, 0, 0] == 4 and two[1, 0, 0, 0] == 2
    assert not two[[0, 2, 3, 5, 6, 7]].any()


def test_paired_table_sixteen_classes(mau):
    S = mau.statistics
    rows = random_rows(np.random.default_rng(50), 3, 6, 1, 16)
    groups = [0, 7, 7, 0, 3, 7]
    stats = S.PairedStats(3, 1, 16)
    stats.update(torch.from_numpy(rows).cuda(), torch.tensor(groups, dtype=torch.uint8).cuda())
    assert stats.result().tobytes() == S.paired_accumulate_host(S.new_table(3, 1, 16), rows, groups, 16).tobytes()


# ---- 3. refusals -------------------------------------------------------------------------------------------------
def test_error_paths(mau):
    S = mau.statistics
    o, t = torch.zeros(2, 2, 2, 6, 5, device="cuda"), torch.zeros(2, 2, 6, 5, device="cuda")
    c = torch.zeros(2, 6, 5, dtype=torch.uint8, device="cuda")
    S.eval_metrics_multi(o, t, c)
    with pytest.raises(ValueError, match="M must be"):
        S.eval_metrics_multi(o[:0], t, c)
    with pytest.raises(ValueError, match="M must be"):
        S.eval_metrics_multi(torch.zeros(9, 2, 2, 6, 5, device="cuda"), t, c)
    with pytest.raises(RuntimeError, match="no CPU"):
        S.eval_metrics_multi(o.cpu(), t, c)
    with pytest.raises(RuntimeError, match="no CPU"):
        S.eval_metrics_multi(o, t, c.cpu())
    with pytest.raises(TypeError):
        S.eval_metrics_multi(o.double(), t, c)
    with pytest.raises(TypeError):
        S.eval_metrics_multi(o, t, c.long())
    with pytest.raises(ValueError):
        S.eval_metrics_multi(o[0], t, c)
    with pytest.raises(ValueError):
        S.eval_metrics_multi(o, t[:, :1], c)
    with pytest.raises(ValueError):
        S.eval_metrics_multi(o, t, c[:, :5])
    with pytest.raises(ValueError):
        S.eval_metrics_multi(o, t, c, num_classes=17)
    for M in (0, 9):
        with pytest.raises(ValueError):
            S.PairedStats(M, 2)
    with pytest.raises(RuntimeError, match="no CPU"):
        S.PairedStats(2, 2, device="cpu")
    stats = S.PairedStats(2, 2)
    rows = torch.zeros(2, 3, 2, HEAD + 27, dtype=torch.float64, device="cuda")
    g = torch.zeros(3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU"):
        stats.update(rows.cpu(), g)
    with pytest.raises(TypeError):
        stats.update(rows.float(), g)
    with pytest.raises(TypeError):
        stats.update(rows, g.int())
    with pytest.raises(ValueError):
        stats.update(rows[:1], g)
    with pytest.raises(ValueError):
        stats.update(rows[..., :-1], g)
    with pytest.raises(ValueError, match="groups must be"):
        stats.update(rows, g[:2])
    assert not stats.result().any(), "a refused call launches nothing"


# ---- 4. end to end -----------------------------------------------------------------------------------------------
TRAIN_TILES = [("Alpha Town", 0, (2018, 3), (2020, 4), None, 12), ("Beta", 1, (2019, 1), (2021, 2), None, 9)]
# known / long: 2019, 2020, 2021; known / mid: 2022, 2023; one unknown / short sample
TEST_TILES = [("Alpha Town", 1, (2019, 1), (2021, 2), None, 12), ("Alpha Town", 2, (2020, 6), (2022, 7), [6], 9),
              ("Beta", 3, (2021, 11), (2023, 12), [0, 8], 12), ("Beta", 4, (2022, 5), (2024, 5), None, 7),
              ("Beta", 5, (2023, 2), (2025, 9), [1, 2, 4], 12), ("Gamma Ville", 0, (2024, 2), (2025, 3), None, 9)]
METRICS = {"meta_mean": [20.0, 10.0, 3.0, 1.0], "meta_std": [15.0, 60.0, 2.0, 0.5], "temp_mean": 14.5, "temp_std": 8.25}


def make_checkpoint(mau, path, model_type, n_meta, trial, seed):
    from mau_amd import checkpoint as C
    torch.manual_seed(seed)
    flags = dict(temporal_embeddings=model_type == "unet++", metadata_embeddings=True)
    net = mau.UrbanPredictor(model_type, 23, 12, 8, n_meta, 8, 12, 2, base_filters=8, **flags)
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "batch_size": 3, **flags}
    C.save_checkpoint(path, net, None, epoch=1, step=2, loss=0.5, hyperparameters=hyper, model_type=model_type,
                      study_name="urban-predictor", trial_id=trial, metadata_input_length=n_meta)


def test_cli_end_to_end(mau, tmp_path):
    S = mau.statistics
    rng = np.random.default_rng(21)
    data = str(tmp_path / "processed")
    write_split(os.path.join(data, "train"), rng, TRAIN_TILES)
    write_split(os.path.join(data, "test"), rng, TEST_TILES)
    json.dump(METRICS, open(os.path.join(data, "normalization_metrics.json"), "w"))
    paths = [str(tmp_path / "a.pth"), str(tmp_path / "b.pth")]
    make_checkpoint(mau, paths[0], "unet", 8, 3, 22)
    make_checkpoint(mau, paths[1], "unet++", 4, 4, 23)
    alone = [mau.evaluate.evaluate_checkpoint(p, data, batch_size=4, precision="fp32", study_name="st", jobid="7",
                                              output_dir=str(tmp_path / "alone")) for p in paths]
    out_dir = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.statistics", *paths, "--processed-dir", data, "--device", "gpu", "--study-name", "st",
                        "--jobid", "7", "--precision", "fp32", "--batch-size", "4", "--output-dir", out_dir],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    names = ["st_unet_metaemb_3_job7", "st_unet++_emb_4_job7"]
    reports = [os.path.join(out_dir, f"{n}_evaluation.csv") for n in names]
    for mine, ref in zip(reports, alone):
        assert os.path.basename(ref["report_path"]) == os.path.basename(mine)
        assert filecmp.cmp(mine, ref["report_path"], shallow=False), "the per-model report must be byte-identical"
        assert os.path.exists(mine.replace("_evaluation.csv", "_info.csv"))
    # the paired tests: the host twin fed from those CSVs
    channels = ["after_ndvi", "after_temp"]
    table = S.table_from_reports(reports, channels)
    assert [int(table[g, 0, 0, 0]) for g in range(8)] == [0, 0, 1, 0, 3, 2, 0, 0]
    want = S.paired_tests(table, names, channels)
    assert want and all(r["is_known_city"] for r in want)
    ref_csv = S.write_paired_tests(want, str(tmp_path / "want"), "st")
    assert filecmp.cmp(os.path.join(out_dir, "st_paired_tests.csv"), ref_csv, shallow=False)
    got = list(csv.DictReader(open(os.path.join(out_dir, "st_paired_tests.csv"))))
    assert list(got[0]) == list(S.CSV_COLUMNS) and len(got) == len(want)
    # the table on stdout: the reference's header, the two long / mid groups, no row of the one-sample unknown group
    assert "--- Comparative Analysis: Paired T-Test Results ---" in p.stdout
    assert f"--- Comparing {names[0]} vs {names[1]} ---" in p.stdout
    assert S.format_table(want, names) in p.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(("Known ", "Unknown "))]
    assert len(lines) == len(want) and not any(ln.startswith("Unknown") for ln in lines) and "short_distance" not in p.stdout
