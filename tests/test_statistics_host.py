"""CPU-only checks of ``mau_amd.statistics``: the C ABI of the two kernels (header, binding, size queries, refusals without a
GPU), the float64 twin of ``mau_paired_accumulate`` against direct numpy, the t-test against recorded ``scipy.stats.ttest_rel``
results and the printed table against the captured output of the reference's ``comparative_analysis``.  The fixtures are written
by tests/golden/make_statfix.py; nothing here needs scipy or pandas."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEAD = 11
# Largest relative deviation of paired_tests' p from scipy 1.15.3 over tests/golden/paired_ttest_cases.json, measured on the CPU:
# 4.2e-13 (n = 500, t = 40, p = 8.8e-158; EXPERIMENTS.md).  The bound is 100 x that, well inside the 1e-9 the check may not exceed.
P_REL = 4.2e-11
P_ABS = 1e-300


@pytest.fixture(scope="module")
def S():
    from mau_amd import statistics
    return statistics


def random_rows(rng, M, B, C, ncls, absent=0.3):
    """Rows in the layout of mau_eval_metrics: finite metrics, some classes without pixels (count 0, NaN means), the same class
    counts in every model's row."""
    rows = rng.uniform(0.1, 5.0, (M, B, C, HEAD + 3 * ncls))
    counts = rng.integers(1, 400, (B, ncls)).astype(np.float64) * (rng.random((B, ncls)) >= absent)
    rows[..., HEAD:HEAD + ncls] = counts[None, :, None, :]
    gone = np.broadcast_to(counts[None, :, None, :] == 0, rows[..., HEAD:HEAD + ncls].shape)
    rows[..., HEAD + ncls:HEAD + 2 * ncls][gone] = np.nan
    rows[..., HEAD + 2 * ncls:][gone] = np.nan
    return rows


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("mau_eval_metrics_multi_max_models", "mau_eval_metrics_multi_ws_elems", "mau_eval_metrics_multi", "mau_paired_groups",
               "mau_paired_entry_elems", "mau_paired_table_elems", "mau_paired_accumulate")


def test_abi_symbols_sizes_and_entry_layout(S):
    from mau_amd import _lib
    lib = _lib.lib
    header = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and f"{name}(" in header
    assert lib.mau_abi_version() == 5
    assert lib.mau_eval_metrics_multi_max_models() == 8 == S.MAX_MODELS and lib.mau_paired_groups() == 8 == S.GROUPS
    # the entry: n, skipped, mean[M], the upper triangle of Cm
    assert "2 + M + M (M + 1) / 2" in header
    for M, want in ((1, 4), (2, 7), (8, 46)):
        assert lib.mau_paired_entry_elems(M) == want == S.entry_elems(M) == 2 + M + M * (M + 1) // 2
        assert [S.tri_index(i, j, M) for i in range(M) for j in range(i, M)] == list(range(M * (M + 1) // 2))
        for C, ncls in ((2, 9), (1, 16), (3, 1)):
            assert lib.mau_paired_table_elems(M, C, ncls) == 8 * C * (4 + 2 * ncls) * want == S.new_table(M, C, ncls).size
    assert lib.mau_paired_entry_elems(0) == lib.mau_paired_entry_elems(9) == 0
    assert lib.mau_paired_table_elems(0, 2, 9) == lib.mau_paired_table_elems(9, 2, 9) == lib.mau_paired_table_elems(2, 2, 17) == 0
    # the workspace: per row of a launch and chunk, the target's partials once and every model's
    per = lib.mau_reduce_tickets_elems()
    for M, B, C, H, W, ncls in ((1, 3, 2, 62, 62, 9), (4, 16, 2, 250, 250, 9), (8, 3, 2, 70, 70, 16), (2, 200, 2, 8, 8, 9)):
        nb = 10 if ncls <= 9 else 17
        want = min(B * C, per) * lib.mau_eval_metrics_chunks(H, W) * ((5 + nb) + M * (7 + 2 * nb))
        assert lib.mau_eval_metrics_multi_ws_elems(M, B, C, H, W, ncls) == want
    assert lib.mau_eval_metrics_multi_ws_elems(0, 3, 2, 8, 8, 9) == lib.mau_eval_metrics_multi_ws_elems(9, 3, 2, 8, 8, 9) == 0
    # slot -> row entry, as the header documents it
    assert [S.slot_column(s, 9) for s in (0, 3, 4, 5, 20, 21)] == [(0, None), (3, None), (20, 11), (29, 11), (28, 19), (37, 19)]


def test_refusals_reach_no_launch():
    """Argument errors are found on the host, before any launch: they are refused on a machine without a GPU too."""
    from mau_amd import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for M in (0, 9):
        assert lib.mau_eval_metrics_multi(p, p, p, None, None, p, p, p, M, 1, 1, 2, 2, 9, None) != 0
        assert b"M must be in [1,8]" in lib.mau_last_error()
        assert lib.mau_paired_accumulate(p, p, p, M, 1, 1, 9, None) != 0
        assert b"M must be in [1,8]" in lib.mau_last_error()
    assert lib.mau_eval_metrics_multi(p, p, p, None, None, p, p, p, 2, 1, 1, 2, 2, 17, None) != 0
    assert lib.mau_eval_metrics_multi(p, None, p, None, None, p, p, p, 2, 1, 1, 2, 2, 9, None) != 0
    assert lib.mau_eval_metrics_multi(p, p, p, None, None, p, p, p, 2, 0, 1, 2, 2, 9, None) != 0
    assert lib.mau_paired_accumulate(p, p, p, 2, 0, 1, 9, None) != 0
    assert lib.mau_paired_accumulate(p, None, p, 2, 1, 1, 9, None) != 0
    assert lib.mau_paired_accumulate(p, p, p, 2, 1, 1, 0, None) != 0


# ---- 2. the twin against direct numpy --------------------------------------------------------------------------
def test_twin_against_numpy_and_batch_split(S):
    rng = np.random.default_rng(31)
    M, C, ncls = 3, 2, 9
    r1, r2 = random_rows(rng, M, 7, C, ncls), random_rows(rng, M, 5, C, ncls)
    r1[1, 2, 0, 0] = np.nan                                       # one sample, one model: overall mae of channel 0
    r1[:, 4, :, HEAD + 6] = 0                                     # class 6 absent in sample 4 ...
    r1[:, 4, :, HEAD + ncls + 6] = r1[:, 4, :, HEAD + 2 * ncls + 6] = np.nan
    g1, g2 = [0, 0, 0, 5, 0, 5, 9], [0, 5, 0, 255, 5]             # groups 0 and 5; ids 9 and 255 are dropped
    two = S.paired_accumulate_host(S.paired_accumulate_host(S.new_table(M, C, ncls), r1, g1, ncls), r2, g2, ncls)
    rows, groups = np.concatenate([r1, r2], axis=1), np.array(g1 + g2)
    one = S.paired_accumulate_host(S.new_table(M, C, ncls), rows, groups, ncls)
    assert one.tobytes() == two.tobytes(), "two batches must give the bits of one"
    assert not one[[1, 2, 3, 4, 6, 7]].any(), "only groups 0 and 5 were fed"

    worst, skipped_total = 0.0, 0
    for g in (0, 5):
        sel = groups == g
        for c in range(C):
            for s in range(4 + 2 * ncls):
                col, cnt = S.slot_column(s, ncls)
                x = rows[:, sel, c, col]                          # (M, samples of the group)
                present = np.ones(x.shape[1], bool) if cnt is None else rows[0, sel, c, cnt] > 0
                finite = np.isfinite(x).all(axis=0)
                x = x[:, present & finite]
                e = one[g, c, s]
                assert e[0] == x.shape[1] and e[1] == np.count_nonzero(present & ~finite)
                skipped_total += int(e[1])
                if x.shape[1] == 0:
                    continue
                mean = e[2:2 + M]
                assert np.all(np.abs(mean - x.mean(axis=1)) <= 1e-10 * np.abs(x.mean(axis=1)))
                if x.shape[1] >= 2:
                    cov = np.cov(x, ddof=1)
                    scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))       # a covariance is bounded relative to the two spreads
                    for i in range(M):
                        for j in range(i, M):
                            got = e[2 + M + S.tri_index(i, j, M)] / (x.shape[1] - 1)
                            worst = max(worst, abs(got - cov[i, j]) / scale[i, j])
                            assert abs(got - cov[i, j]) <= 1e-10 * scale[i, j]
    print(f"twin against np.cov: worst |difference| / spread = {worst:.3g}")
    assert skipped_total == 1, "the one NaN sample is counted in exactly one entry"
    # the host merge of groups gives the moments of their union
    merged = S.merge_entries(one[0, 0, 0], one[5, 0, 0], M)
    x = rows[:, :, 0, 0][:, np.isin(groups, (0, 5)) & np.isfinite(rows[:, :, 0, 0]).all(axis=0)]
    assert merged[0] == x.shape[1] and merged[1] == 1
    assert np.allclose(merged[2:2 + M], x.mean(axis=1), rtol=1e-12, atol=0)
    assert np.allclose([merged[2 + M + S.tri_index(i, j, M)] / (x.shape[1] - 1) for i in range(M) for j in range(i, M)],
                       [np.cov(x, ddof=1)[i, j] for i in range(M) for j in range(i, M)], rtol=1e-10, atol=1e-12)


def test_twin_refuses_misfits(S):
    rows = np.zeros((2, 3, 2, HEAD + 27))
    with pytest.raises(ValueError):
        S.paired_accumulate_host(S.new_table(3, 2, 9), rows, [0, 0, 0], 9)
    with pytest.raises(ValueError):
        S.paired_accumulate_host(S.new_table(2, 2, 9), rows, [0, 0], 9)
    assert [S.group_id(k, y) for k, y in ((False, 2019), (False, 2022), (False, 2024), (True, 2021), (True, 2023), (True, 2030))] == [0, 1, 2, 4, 5, 6]


# ---- 3. the t-test against scipy's recorded results ---------------------------------------------------------------
def table_of_pair(S, a, b):
    n = len(a)
    rows = np.full((2, n, 1, HEAD + 3), np.nan)
    rows[..., HEAD] = 0                                           # the one class has no pixels: only the overall slots count
    rows[0, :, 0, 0], rows[1, :, 0, 0] = a, b
    rows[0, :, 0, 1], rows[1, :, 0, 1] = b, a                     # rmse: the pair the other way round
    return S.paired_accumulate_host(S.new_table(2, 1, 1), rows, [4] * n, 1)


def test_paired_tests_match_scipy(S):
    with open(os.path.join(GOLDEN, "paired_ttest_cases.json")) as f:
        fixture = json.load(f)
    cases = fixture["cases"]
    assert {c["n"] for c in cases} >= {2, 3, 10, 500} and max(abs(c["t"]) for c in cases if math.isfinite(c["t"])) > 39
    worst = 0.0
    for c in cases:
        res = S.paired_tests(table_of_pair(S, c["a"], c["b"]), ["m1", "m2"], ["ch"], ["k"])
        assert [(r["metric"], r["dw_class"], r["is_known_city"], r["temporal_distance"], r["n"]) for r in res] == \
            [("mae", "overall", True, "long_distance", c["n"]), ("rmse", "overall", True, "long_distance", c["n"])]
        fwd, rev = res
        assert abs(fwd["mean_diff"] - c["mean_diff"]) <= 1e-12 * max(np.abs(c["a"]).max(), 1.0) and rev["mean_diff"] == -fwd["mean_diff"]
        if math.isnan(c["p"]):                                     # no spread, no difference
            assert math.isnan(fwd["p_value"]) and math.isnan(fwd["t"]) and fwd["winner"] == rev["winner"] == "Insignificant"
            continue
        for r in (fwd, rev):
            dev = abs(r["p_value"] - c["p"])
            worst = max(worst, dev / c["p"] if c["p"] > 0 else dev)
            assert dev <= max(P_REL * c["p"], P_ABS), (c["name"], r["p_value"], c["p"])
        if math.isinf(c["t"]):                                     # no spread, a difference
            assert fwd["t"] == c["t"] and fwd["p_value"] == 0.0
        else:
            assert abs(fwd["t"] - c["t"]) <= 1e-9 * abs(c["t"]) + 1e-12
        want = "Insignificant" if not c["p"] < 0.05 else "m2" if c["mean_diff"] > 0 else "m1"
        assert fwd["winner"] == want and rev["winner"] == {"m1": "m2", "m2": "m1"}.get(want, want)
        r = np.corrcoef(c["a"], c["b"])[0, 1]                     # the page's sample-wise error correlation (section 8)
        assert abs(fwd["pearson_r"] - r) <= 1e-10 and abs(rev["pearson_r"] - r) <= 1e-10
    print(f"p against scipy {fixture['scipy']}: worst relative deviation {worst:.3g} (bound {P_REL:g})")


def test_student_t_known_values(S):
    # df = 1 is the Cauchy distribution: P(|T| >= t) = 1 - 2 atan(t) / pi; df = 2: 1 - t / sqrt(2 + t^2)
    for t in (0.0, 0.1, 1.0, 5.0, 300.0):
        assert math.isclose(S.student_t_two_sided(t, 1), 1 - 2 * math.atan(t) / math.pi, rel_tol=1e-12, abs_tol=1e-15)
        assert math.isclose(S.student_t_two_sided(-t, 2), 1 - t / math.sqrt(2 + t * t), rel_tol=1e-11, abs_tol=1e-15)
    assert S.student_t_two_sided(float("inf"), 3) == 0.0 and math.isnan(S.student_t_two_sided(float("nan"), 3))


# ---- 4. the reference's table ----------------------------------------------------------------------------------
def parse_reference(text):
    """(pair, metric, known, temporal distance, channel, class, mean diff text, p text, winner) of every result line."""
    out, pair, metric = [], None, None
    for line in text.splitlines():
        if line.startswith("--- Comparing "):
            pair = tuple(line[len("--- Comparing "):-len(" ---")].split(" vs "))
        elif line.startswith("** Metric: "):
            metric = line.split()[2].lower()
        elif line.startswith(("Known ", "Unknown ")) and not line.startswith("Known/Unknown"):
            f = line.split()
            out.append((pair, metric, f[0] == "Known", f[1], f[2], f[3], f[4], f[5], f[6]))
    return out


def test_table_is_the_references(S):
    fix = os.path.join(GOLDEN, "statfix")
    paths = [os.path.join(fix, f"model_{m}_evaluation.csv") for m in "ab"]
    names = [os.path.basename(p).replace("_evaluation.csv", "") for p in paths]
    channels = ["after_ndvi", "after_temp"]
    table = S.table_from_reports(paths, channels)
    # six samples: three known / long, two known / mid, one unknown / short
    assert [int(table[g, 0, 0, 0]) for g in range(8)] == [0, 0, 1, 0, 3, 2, 0, 0]
    tests = S.paired_tests(table, names, channels)
    with open(os.path.join(fix, "reference_table_stdout.txt")) as f:
        captured = f.read()
    want = parse_reference(captured)
    assert len(want) == 20 and not any(w[2] is False for w in want), "the fixture: the one-sample unknown group gives no row"
    got = [((r["model_1"], r["model_2"]), r["metric"], r["is_known_city"], r["temporal_distance"], r["channel"], r["dw_class"],
            f"{r['mean_diff']:.4f}", f"{r['p_value']:.4f}", r["winner"]) for r in tests]
    assert got == want                                            # the same groups in the same order, winners, four decimals
    assert {w[8] for w in want} == {"Insignificant", "model_a"}
    assert all(r["n"] >= 2 for r in tests) and not any(r["temporal_distance"] == "short_distance" for r in tests)
    # and the printed form, line for line
    assert S.format_table(tests, names).splitlines() == captured.splitlines()
    assert "--- Comparative Analysis: Paired T-Test Results ---" in captured


def test_single_model_interpretation_and_summary(S):
    fix = os.path.join(GOLDEN, "statfix")
    table = S.table_from_reports([os.path.join(fix, "model_a_evaluation.csv")], ["after_ndvi", "after_temp"])
    assert table.shape == (8, 2, 22, 4)
    text = S.format_interpretation(table, "model_a", ["after_ndvi", "after_temp"])
    assert "--- Analysis for Known Cities | Temporal Distance: long_distance ---" in text
    assert "--- Analysis for Unknown Cities | Temporal Distance: short_distance ---" in text and "mid_distance" in text
    assert text.count("Channel: after_temp") == 3 and "Smoothness (Laplacian Var): Pred=" in text
    summary = S.global_summary(table, ["model_a"], ["after_ndvi", "after_temp"])
    import csv
    rows = [r for r in csv.DictReader(open(os.path.join(fix, "model_a_evaluation.csv"))) if r["dw_class"] == "overall" and r["channel"] == "after_temp"]
    mae = np.array([float(r["mae"]) for r in rows])
    got = next(g for g in summary if g["channel"] == "after_temp" and g["metric"] == "mae")
    assert got["n"] == 6 and math.isclose(got["mean"], mae.mean(), rel_tol=1e-12) and math.isclose(got["std"], mae.std(ddof=1), rel_tol=1e-10)
