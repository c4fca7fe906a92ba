"""Host tests of ``mau_amd.rank_tests``: the numpy twin's integers and the plain-Python statistics against scipy -- live where scipy
is installed, and from the recorded fixture tests/golden/rankfix_cases.json (tests/golden/make_rankfix.py) everywhere --, the
metadata correlations against recorded ``pearsonr`` values, the CSV, ``rank_tests_from_reports`` on the statistics fixtures and the
drop rule."""
import csv
import importlib.util
import math
import os

import numpy as np
import pytest

import mau_amd  # noqa: F401
from mau_amd import rank_tests as R
from tests._helpers import GOLDEN

# p-values: the formulas here and scipy's agree to 3e-15 (measured over the fixture's cases); 1e-12 leaves room for another libm
P_REL = 1e-12


def _generator():
    spec = importlib.util.spec_from_file_location("make_rankfix", os.path.join(GOLDEN, "make_rankfix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    cases, pearson = _generator().load()
    return {"cases": cases, "pearson": pearson}


def same_p(got, want):
    if want is None:
        return math.isnan(got)
    return math.isclose(got, want, rel_tol=P_REL, abs_tol=0.0)


def check_case(case, want):
    """One case against what scipy said: statistics equal, p within P_REL, the method the branch scipy took."""
    x = np.asarray(case["x"], dtype=np.float64)
    n = x.shape[1]
    for split, mask in case["known"].items():
        table = R.rank_tests_host(x[None], mask)
        assert table.shape == (1, R.q_elems(2)) and table.dtype == np.int64
        n_used, n_zero, skipped, wp, wm, tie, small = (int(v) for v in R.pair_entry(table[0], 0))
        d = x[0] - x[1]
        assert (n_used, n_zero, skipped) == (int((d != 0).sum()), int((d == 0).sum()), 0) and wp + wm == n_used * (n_used + 1)
        w = R.wilcoxon_from_counts(n_used, n_zero, wp, wm, tie, small)
        sw = want["wilcoxon"]
        assert sw.get("raised") or w["statistic"] == sw["statistic"], (case["name"], w, sw)
        assert same_p(w["p_value"], sw["p"]), (case["name"], w, sw)
        assert w["method"] == sw["method"], (case["name"], w, sw)
        for m in range(2):
            n1, n2, r2, mtie = (int(v) for v in R.model_entry(table[0], m, 2))
            assert (n1, n2) == (int(np.sum(mask)), n - int(np.sum(mask)))
            mw = R.mannwhitney_from_counts(n1, n2, r2, mtie)
            sm = want["mannwhitney"][split][m]
            if sm is None:
                assert math.isnan(mw["p_value"]) and math.isnan(mw["statistic"]), (case["name"], split, mw)
                continue
            assert mw["statistic"] == sm["statistic"], (case["name"], split, mw, sm)
            assert same_p(mw["p_value"], sm["p"]), (case["name"], split, mw, sm)
            assert mw["method"] == sm["method"], (case["name"], split, mw, sm)
        g = R.axis_range(R.pool_entry(table[0], 2))
        assert g["n"] == 2 * n and g["min"] == want["min"] and g["p98"] == want["p98"], (case["name"], g, want["p98"])
        pad = (want["p98"] - want["min"]) * 0.05
        assert g["ylim_min"] == max(0, want["min"] - pad) and g["ylim_max"] == want["p98"] + pad


def test_twin_against_scipy_live():
    pytest.importorskip("scipy")
    gen = _generator()
    cases = gen.cases()
    assert len(cases) == 62 * 3
    methods = set()
    for case in cases:
        want = gen.scipy_results(case)
        check_case(case, want)
        methods.add(("w", want["wilcoxon"]["method"], case["name"].split("_")[1]))
        methods |= {("m", r["method"]) for rows in want["mannwhitney"].values() for r in rows if r}
    # every branch was met: exact and approximate Wilcoxon with and without ties, both Mann-Whitney branches
    assert {("w", "exact", "continuous"), ("w", "approx", "continuous"), ("w", "exact", "rounded"), ("w", "approx", "rounded"),
            ("w", "exact", "identical"), ("w", "approx", "identical"), ("m", "exact"), ("m", "approx")} <= methods


def test_twin_against_recorded_scipy(fixture):
    assert len(fixture["cases"]) == 62 * 3
    for case, want in fixture["cases"]:
        check_case(case, want)
    ident = {c["name"]: w["wilcoxon"] for c, w in fixture["cases"] if c["name"].endswith("identical")}
    assert ident["n60_identical"]["p"] is None and ident["n1000_identical"]["p"] is None       # no used sample: NaN


def test_counting_identities():
    """less / eq by sorting against the definition, the tie term against the tie groups, the small-sample tie groups."""
    rng = np.random.default_rng(3)
    v = np.round(rng.uniform(0, 1, 300), 2)
    less, eq = R._counts(v)
    assert np.array_equal(less, (v[None, :] < v[:, None]).sum(1)) and np.array_equal(eq, (v[None, :] == v[:, None]).sum(1))
    _, t = np.unique(v, return_counts=True)
    assert int((eq * eq - 1).sum()) == int((t ** 3 - t).sum())
    x = np.array([[[0.3, 0.1, 0.5, 0.2, 0.2, 0.9, 0.4]]])           # (1, 1, 7): one model
    assert R.rank_tests_host(x, np.ones(7)).shape == (1, R.q_elems(1)) == (1, 8)
    two = np.array([[[5.0, 1.0, 4.0, 3.0, 3.0, 9.0], [3.0, 3.0, 2.0, 1.0, 3.0, 5.0]]])  # d = 2, -2, 2, 2, 0, 4
    e = R.pair_entry(R.rank_tests_host(two, np.ones(6))[0], 0)
    # |d|: 2 four times (ranks 1-4, mid 2.5), 4 once (rank 5): groups of 4 at position 0 and of 1 at position 4
    assert list(e) == [5, 1, 0, 3 * 5 + 10, 5, 4 ** 3 - 4, 4 + (1 << 16)]


def test_drop_rule_counts_the_sample_for_every_model():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.1, 0.4, (2, 3, 40))
    x[0, 2, 7] = np.nan                                              # q 0: a NaN in the last model drops sample 7 for all models
    x[1, 0, 11] = np.inf
    x[1, 2, 12] = -np.inf
    known = rng.random(40) < 0.5
    table = R.rank_tests_host(x, known)
    for q, dropped in ((0, [7]), (1, [11, 12])):
        keep = np.ones(40, bool)
        keep[dropped] = False
        assert np.array_equal(table[q], R.rank_tests_host(x[q:q + 1][:, :, keep], known[keep])[0] +
                              np.array(([0, 0, len(dropped), 0, 0, 0, 0] * 3) + [0] * 16))
        for p in range(3):
            assert R.pair_entry(table[q], p)[2] == len(dropped) and R.pair_entry(table[q], p)[:2].sum() == 40 - len(dropped)
        for m in range(3):
            assert R.model_entry(table[q], m, 3)[:2].sum() == 40 - len(dropped)
        assert R.pool_entry(table[q], 3)[0] == 3 * (40 - len(dropped))
    rows = R.rank_test_rows(table, ["a", "b", "c"], ["after_ndvi"], n_samples=40)
    assert [r["skipped"] for r in rows[:6]] == [1] * 6 and [r["skipped"] for r in rows[6:]] == [2] * 6
    one = R.rank_test_rows(R.rank_tests_host(x[:, 2:], known), ["c"], ["after_ndvi"], n_samples=40)
    assert [r["skipped"] for r in one] == [1, 1] and all(r["test"] == "mannwhitney" for r in one)


def test_metadata_correlations_against_recorded_pearsonr(fixture):
    # r: two normalised dot products, n roundings of 1e-16 each; p: the incomplete beta function of statistics.py, whose own
    # tests bound it by 1e-11 relative against closed forms, times the slope d log p / d log r (below 1e2 at these p-values)
    for c in fixture["pearson"]:
        r, p = R.pearson(c["y"], c["x"])
        assert math.isclose(r, c["r"], rel_tol=0, abs_tol=1e-13), (c["n"], r, c["r"])
        assert math.isclose(p, c["p"], rel_tol=1e-9, abs_tol=1e-300), (c["n"], p, c["p"])
    assert all(math.isnan(v) for v in R.pearson([1.0], [2.0])) and all(math.isnan(v) for v in R.pearson([1.0, 2.0, 3.0], [2.0, 2.0, 2.0]))
    # the page's section 4 on one model's rows: the city's sample count, the subsets, NaN for a single year
    big = next(c for c in fixture["pearson"] if c["n"] == 10)
    rows = []
    for i, (lat, y) in enumerate(zip(big["x"], big["y"])):
        info = {"sample_idx": i, "is_known_city": i % 2 == 0, "t1_year": 2020 + (i % 2) * (i % 3), "city": "A" if i < 7 else "B",
                "lat": lat, "lon": -lat}
        rows.append({"channel": "after_temp", "dw_class": "overall", "mae": y, "rmse": 2 * y, **info})
        rows.append({"channel": "after_temp", "dw_class": "trees", "mae": 9.0, "rmse": 9.0, **info})
    got = {(g["metric"], g["subset"], g["variable"]): g for g in R.metadata_correlations(rows)}
    assert len(got) == 2 * 3 * 4
    assert math.isclose(got["mae", "all", "lat"]["r"], big["r"], abs_tol=1e-13) and math.isclose(got["mae", "all", "lat"]["p_value"], big["p"], rel_tol=1e-9)
    assert math.isclose(got["rmse", "all", "lon"]["r"], -big["r"], abs_tol=1e-13) and got["mae", "all", "lat"]["n"] == 10
    count = np.array([7.0] * 7 + [3.0] * 3)
    assert math.isclose(got["mae", "all", "city_sample_count"]["r"], np.corrcoef(np.array(big["y"]), count)[0, 1], abs_tol=1e-12)
    assert got["mae", "known", "lat"]["n"] == 5 and math.isnan(got["mae", "known", "t1_year"]["r"])       # known: every year 2020
    assert not math.isnan(got["mae", "unknown", "t1_year"]["r"]) and not math.isnan(got["mae", "all", "t1_year"]["p_value"])


def test_rank_tests_from_reports_and_csv(tmp_path):
    paths = [os.path.join(GOLDEN, "statfix", f"model_{m}_evaluation.csv") for m in "ab"]
    rows = R.rank_tests_from_reports(paths)
    names = ["model_a", "model_b"]
    assert [(r["test"], r["channel"], r["metric"], r["model_1"], r["model_2"]) for r in rows] == [
        (t, ch, me, *mm) for ch in ("after_ndvi", "after_temp") for me in ("mae", "rmse")
        for t, mm in (("wilcoxon", ("model_a", "model_b")), ("mannwhitney", ("model_a", "")), ("mannwhitney", ("model_b", "")))]
    recs = {m: [r for r in csv.DictReader(open(p)) if r["dw_class"] == "overall"] for m, p in zip(names, paths)}
    for r in rows:
        a = np.array([float(x[r["metric"]]) for x in recs["model_a"] if x["channel"] == r["channel"]])
        b = np.array([float(x[r["metric"]]) for x in recs["model_b"] if x["channel"] == r["channel"]])
        known = np.array([x["is_known_city"] == "True" for x in recs["model_a"] if x["channel"] == r["channel"]])
        assert r["skipped"] == 0 and r["method"] == "exact"
        if r["test"] == "wilcoxon":
            # six samples, model b worse on every temperature sample: W+ = 0, p = 2 / 2^6
            assert r["n"] == 6 and r["n_zero"] == 0
            if r["channel"] == "after_temp":
                assert r["statistic"] == 0.0 and r["p_value"] == 2 / 64
        else:
            v = a if r["model_1"] == "model_a" else b
            assert r["n"] == 6 and math.isclose(r["mean_known"], v[known].mean(), rel_tol=1e-12)
            assert math.isclose(r["mean_unknown"], v[~known].mean(), rel_tol=1e-12)
            assert math.isclose(r["mean_diff"], v[~known].mean() - v[known].mean(), rel_tol=1e-9)
            # five known cities against one unknown: U1 = the number of known values above it, p = 2 P(U' >= U) over 6 places
            u1 = float((v[known] > v[~known][0]).sum())
            assert r["statistic"] == u1 and math.isclose(r["p_value"], min(1.0, 2 * (5 - max(u1, 5 - u1) + 1) / 6), rel_tol=1e-15)
    path = R.write_rank_tests(rows, str(tmp_path), "st")
    assert os.path.basename(path) == "st_rank_tests.csv"
    back = list(csv.DictReader(open(path)))
    assert list(back[0]) == list(R.CSV_COLUMNS) == ["test", "channel", "metric", "model_1", "model_2", "n", "n_zero", "skipped", "statistic",
                                                     "z", "p_value", "method", "mean_known", "mean_unknown", "mean_diff"]
    assert len(back) == len(rows) and float(back[0]["p_value"]) == rows[0]["p_value"] and back[1]["model_2"] == ""
    text = R.format_tables(rows, names)
    assert "--- Pairwise Wilcoxon P-Values (after_temp, MAE) ---" in text and "--- Known vs Unknown Cities: Mann-Whitney U (after_ndvi, RMSE) ---" in text
    assert f"{2 / 64:.1e}" in text


def test_refusals_of_the_twin():
    with pytest.raises(ValueError):
        R.rank_tests_host(np.zeros((1, 9, 4)), np.zeros(4))
    with pytest.raises(ValueError):
        R.rank_tests_host(np.zeros((1, 0, 4)), np.zeros(4))
    with pytest.raises(ValueError):
        R.rank_tests_host(np.zeros((1, 2, 4)), np.zeros(3))
    with pytest.raises(ValueError):
        R.rank_tests_host(np.zeros((2, 4)), np.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU"):
        R.RankStats(2, 2, 16, device="cpu")
