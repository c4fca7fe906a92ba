"""GPU tests of ``mau_amd.rank_tests``: the table of ``mau_rank_tests`` against the numpy twin as int64, bit for bit, at every size
around the kernel's tile; independence of the batching; the refusals; the command line with and without ``--rank-tests``."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import mau  # noqa: F401
from tests.test_eval_metrics_host import write_split
from tests.test_gpu_statistics import METRICS, TEST_TILES, TRAIN_TILES, make_checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("continuous", "rounded", "identical", "all_known", "none_known", "nonfinite")


def tile_sizes(T):
    return [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 1000]


def make_case(rng, M, Q, N, variant, slack):
    """cols (Q, M, N + slack) and known (N + slack,): the first N entries are the samples, the rest is never to be read."""
    x = rng.uniform(0.05, 0.30, (Q, M, N))
    known = (rng.random(N) < 0.4).astype(np.uint8)
    if variant in ("rounded", "nonfinite"):
        x = np.round(x, 2)
    if variant == "identical" and M >= 2:
        x[:, 1] = x[:, 0]                                            # n_used == 0 for the pair (0, 1)
    if variant == "all_known":
        known[:] = 1
    if variant == "none_known":
        known[:] = 0
    if variant == "nonfinite":
        x[0, M - 1, N // 2] = np.nan                                 # a NaN and an inf in the last model
        x[Q - 1, M - 1, N - 1] = np.inf
    cols = np.empty((Q, M, N + slack))
    cols[..., :N] = x
    # the slack: NaN, or garbage that would change every count if it were read (values inside the range, huge ones, zeros)
    cols[..., N:] = np.nan if variant in ("continuous", "identical", "none_known") else rng.choice([0.0, 0.17, 1e300, -1e300], (Q, M, slack))
    return cols, np.concatenate([known, np.ones(slack, dtype=np.uint8)])


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_table_is_the_twins_integers(mau, M):
    R = mau.rank_tests
    T = R.TILE
    assert T == mau._lib.lib.mau_rank_tile() and T >= 64
    rng = np.random.default_rng(70 + M)
    for N in tile_sizes(T):
        for Q in (1, 4):
            for v, variant in enumerate(VARIANTS):
                slack = 0 if (v + N) % 3 == 0 else 5
                cols, known = make_case(rng, M, Q, N, variant, slack)
                got = R.rank_tests_device(torch.from_numpy(cols).cuda(), torch.from_numpy(known).cuda(), n=N)
                want = R.rank_tests_host(cols[..., :N], known[:N])
                assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape == (Q, R.q_elems(M))
                assert np.array_equal(got, want), (M, N, Q, variant, np.argwhere(got != want)[:8].tolist())
                if variant == "identical" and M >= 2:
                    assert (got[:, 0] == 0).all() and (got[:, 1] == N).all()          # pair (0, 1): n_used 0, n_zero N
                if variant == "nonfinite":
                    assert N - got[0, -4] // M in (1, 2), "the non-finite samples are dropped for every model"


def test_batching_and_repetition_do_not_change_a_bit(mau):
    R = mau.rank_tests
    rng = np.random.default_rng(9)
    M, C, N, ncols = 3, 2, 2 * R.TILE + 37, 11 + 3 * 9
    rows = rng.uniform(0.05, 0.3, (M, N, C, ncols))
    rows[..., :2] = np.round(rows[..., :2], 2)
    rows[M - 1, 5, 1, 0] = np.nan
    known = (rng.random(N) < 0.5).astype(np.uint8)
    drows, dknown = torch.from_numpy(rows).cuda(), torch.from_numpy(known).cuda()
    one = R.RankStats(M, C, N)
    one.update(drows, dknown)
    first = one.result()
    assert np.array_equal(first, one.result()), "a repeated result() must agree bit for bit"
    three = R.RankStats(M, C, N + 100)                               # a capacity above N: the slack of the store is never read
    cuts = [0, 7, R.TILE + 1, N]
    for a, b in zip(cuts, cuts[1:]):
        three.update(drows[:, a:b].contiguous(), dknown[a:b])
    assert three.n == N and np.array_equal(three.result(), first), "three batches must give the bits of one"
    # q = 2 c + (0 mae, 1 rmse), the columns in sample order
    cols = rows[..., :2].transpose(2, 3, 0, 1).reshape(2 * C, M, N)
    assert np.array_equal(first, R.rank_tests_host(cols, known))
    assert first[2, 2] == 1 and (first[[0, 1, 3], 2] == 0).all()     # the NaN: channel 1, mae


def test_refusals(mau):
    R = mau.rank_tests
    lib = mau._lib.lib
    for M in (0, 9):
        with pytest.raises(ValueError):
            R.RankStats(M, 2, 16)
        assert lib.mau_rank_table_elems(M, 4) == 0
        with pytest.raises(ValueError):
            R.rank_tests_device(torch.zeros(1, M, 4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        R.RankStats(2, 2, R.MAX_SAMPLES + 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        R.RankStats(2, 2, 16, device="cpu")
    assert R.MAX_SAMPLES == 1 << 20 and lib.mau_rank_ws_elems(1, R.MAX_SAMPLES + 1) == 0
    # the C entry point itself: N above the cap, M out of range, a null pointer -- refused before any launch
    cols = torch.zeros(1, 2, 4, dtype=torch.float64, device="cuda")
    known = torch.zeros(4, dtype=torch.uint8, device="cuda")
    table = torch.full((R.q_elems(2),), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(8, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for M, N, cap, ptr in ((2, R.MAX_SAMPLES + 1, R.MAX_SAMPLES + 1, cols.data_ptr()), (0, 4, 4, cols.data_ptr()), (9, 4, 4, cols.data_ptr()),
                           (2, 4, 3, cols.data_ptr()), (2, 0, 4, cols.data_ptr()), (2, 4, 4, None)):
        assert lib.mau_rank_tests(ptr, known.data_ptr(), table.data_ptr(), ws.data_ptr(), M, 1, N, cap, stream) == 1, (M, N, cap)
        assert b"rank_tests" in lib.mau_last_error()
    torch.cuda.synchronize()
    assert bool((table == -7).all()), "a refused call launches nothing"
    stats = R.RankStats(2, 2, 8)
    rows = torch.zeros(2, 3, 2, 38, dtype=torch.float64, device="cuda")
    k = torch.zeros(3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="no sample"):
        stats.result()
    with pytest.raises(RuntimeError, match="no CPU"):
        stats.update(rows.cpu(), k)
    with pytest.raises(RuntimeError, match="no CPU"):
        stats.update(rows, k.cpu())
    with pytest.raises(TypeError):
        stats.update(rows.float(), k)
    with pytest.raises(TypeError):
        stats.update(rows, k.int())
    with pytest.raises(ValueError):
        stats.update(rows[:1], k)
    with pytest.raises(ValueError):
        stats.update(rows, k[:2])
    with pytest.raises(TypeError):
        R.rank_tests_device(cols.float(), known)
    with pytest.raises(TypeError):
        R.rank_tests_device(cols, known.long())
    with pytest.raises(RuntimeError, match="no CPU"):
        R.rank_tests_device(cols.cpu(), known)
    with pytest.raises(ValueError):
        R.rank_tests_device(cols, known, n=5)
    assert stats.n == 0
    stats.update(rows, k)
    stats.update(rows, k)
    with pytest.raises(ValueError, match="capacity"):
        stats.update(rows, k)
    assert stats.n == 6


def test_cli_with_and_without_rank_tests(mau, tmp_path, capsys):
    S, R = mau.statistics, mau.rank_tests
    rng = np.random.default_rng(21)
    data = str(tmp_path / "processed")
    write_split(os.path.join(data, "train"), rng, TRAIN_TILES)
    write_split(os.path.join(data, "test"), rng, TEST_TILES)
    json.dump(METRICS, open(os.path.join(data, "normalization_metrics.json"), "w"))
    paths = [str(tmp_path / "a.pth"), str(tmp_path / "b.pth")]
    make_checkpoint(mau, paths[0], "unet", 8, 3, 22)
    make_checkpoint(mau, paths[1], "unet++", 4, 4, 23)
    common = [*paths, "--processed-dir", data, "--device", "gpu", "--study-name", "st", "--jobid", "7", "--precision", "fp32", "--batch-size", "4"]
    # without the flag, in this process: what the tool printed and wrote before there were rank tests
    plain_dir = str(tmp_path / "plain")
    capsys.readouterr()
    assert S.main(common + ["--output-dir", plain_dir]) == 0
    plain_out = capsys.readouterr().out
    # with the flag, the command line itself
    rank_dir = str(tmp_path / "rank")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.statistics", *common, "--output-dir", rank_dir, "--rank-tests"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    names = ["st_unet_metaemb_3_job7", "st_unet++_emb_4_job7"]
    files = [f"{n}_{kind}.csv" for n in names for kind in ("evaluation", "info")] + ["st_paired_tests.csv"]
    assert sorted(os.listdir(plain_dir)) == sorted(files), "without the flag: the files of before, no other"
    assert sorted(os.listdir(rank_dir)) == sorted(files + ["st_rank_tests.csv"])
    for f in files:
        if not f.endswith("_info.csv"):                              # (the info file names its own directory)
            assert filecmp.cmp(os.path.join(plain_dir, f), os.path.join(rank_dir, f), shallow=False), f
    # the CSV: the twin fed from the written reports
    reports = [os.path.join(rank_dir, f"{n}_evaluation.csv") for n in names]
    want = R.rank_tests_from_reports(reports, ["after_ndvi", "after_temp"], names)
    assert len(want) == 2 * 2 * 3 and {r["n"] for r in want} == {6} and {r["skipped"] for r in want} == {0}
    ref_csv = R.write_rank_tests(want, str(tmp_path / "want"), "st")
    assert filecmp.cmp(os.path.join(rank_dir, "st_rank_tests.csv"), ref_csv, shallow=False)
    # stdout: with the flag, what the plain run prints plus one line and the two tables; without, nothing of them
    assert "Wilcoxon" not in plain_out and "Mann-Whitney" not in plain_out and "Rank tests saved" not in plain_out
    tables = R.format_tables(want, names, R.axis_ranges(R.rank_tests_host(*R.columns_from_reports(reports, ["after_ndvi", "after_temp"])),
                                                        ["after_ndvi", "after_temp"], 2))
    assert "--- Pairwise Wilcoxon P-Values (after_ndvi, MAE) ---" in tables and "Mann-Whitney U (after_temp, RMSE)" in tables
    head, sep, tail = plain_out.replace(plain_dir, rank_dir).partition("Paired tests saved to " + os.path.join(rank_dir, "st_paired_tests.csv") + "\n")
    assert sep and p.stdout == head + sep + f"Rank tests saved to {os.path.join(rank_dir, 'st_rank_tests.csv')}\n" + tail + tables + "\n"
