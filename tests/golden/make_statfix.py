"""Writes the fixtures of tests/test_statistics_host.py: tests/golden/paired_ttest_cases.json and tests/golden/statfix/.

    python tests/golden/make_statfix.py --reference /path/to/the/reference/checkout

* ``paired_ttest_cases.json``: pairs of score vectors with what ``scipy.stats.ttest_rel`` says about them (n = 2, 3, 10, 500; |t|
  from 0 to about 40; differences without spread, with and without a mean).  Needs scipy.
* ``statfix/model_a_evaluation.csv`` / ``model_b_evaluation.csv``: two small evaluation reports of six samples -- known cities with t1 years
  2019, 2020, 2021 (long distance) and 2022, 2023 (mid distance), one unknown city with t1 year 2024 (a group of one sample, which
  the comparison must skip) -- and ``reference_table_stdout.txt``: what the reference's ``comparative_analysis``
  (test/statistical_tests.py) prints for them.  Needs pandas, scipy and the reference checkout; nothing of the reference is copied,
  it is imported and run.  Without ``--reference`` only the t-test cases are written.
"""
import argparse
import contextlib
import csv
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "statfix")
COLUMNS = ("sample_idx", "channel", "dw_class", "mae", "rmse", "laplacian_var_pred", "laplacian_var_gt", "is_known_city",
           "t1_year", "t1_month", "t2_year", "t2_month", "time_delta", "city", "lat", "lon")


def ttest_cases():
    from scipy.stats import ttest_rel
    rng = np.random.default_rng(20261020)
    cases = []

    def add(name, a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        res = ttest_rel(a, b)
        cases.append({"name": name, "a": a.tolist(), "b": b.tolist(), "n": int(a.size), "t": float(res.statistic),
                      "p": float(res.pvalue), "mean_diff": float(a.mean() - b.mean())})

    for n in (2, 3, 10, 500):
        a = rng.uniform(0.5, 3.0, n)
        noise = rng.standard_normal(n)
        noise -= noise.mean()
        sd = noise.std(ddof=1)
        for target in (0.0, 0.3, 2.0, 8.0, 40.0) if n < 500 else (0.0, 2.0, 40.0):     # t = shift / (sd / sqrt(n)), up to rounding
            shift = target * sd / np.sqrt(n)
            add(f"n{n}_t{target:g}", a, a - shift - noise)
        if n < 500:
            add(f"n{n}_negative", a, a + 3.0 * sd / np.sqrt(n) - noise)
    # differences without spread: values that every operation of the moment update represents exactly
    add("constant_zero", [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0])
    add("constant_shift", [1.0, 2.0, 3.0, 4.0], [0.5, 1.5, 2.5, 3.5])
    add("constant_shift_n2", [2.0, 4.0], [3.0, 5.0])
    with open(os.path.join(HERE, "paired_ttest_cases.json"), "w") as f:
        json.dump({"scipy": __import__("scipy").__version__, "cases": cases}, f, indent=0)
    print(f"{len(cases)} t-test cases")


SAMPLES = [("Alpha Town", True, 2019, 3, 2022, 4), ("Alpha Town", True, 2020, 5, 2023, 5), ("Beta", True, 2021, 7, 2024, 8),
           ("Beta", True, 2022, 1, 2024, 2), ("Alpha Town", True, 2023, 9, 2025, 9), ("Gamma Ville", False, 2024, 6, 2025, 6)]
CLASSES = {0: ("trees", "built"), 1: ("built",), 2: ("trees", "built"), 3: ("trees", "built"), 4: ("built", "water"), 5: ("trees",)}


def reports(rng):
    """Rows of two models over the same samples; model b is clearly worse on the temperature channel."""
    out = {"a": [], "b": []}
    for idx, (city, known, y1, m1, y2, m2) in enumerate(SAMPLES):
        info = {"is_known_city": known, "t1_year": y1, "t1_month": m1, "t2_year": y2, "t2_month": m2, "time_delta": y2 - y1,
                "city": city, "lat": 48.8566, "lon": 2.3522}
        for ch, level in (("after_ndvi", 0.08), ("after_temp", 2.5)):
            lap_gt = float(rng.uniform(0.5, 1.5))
            for cl in ("overall",) + CLASSES[idx]:
                base = level * float(rng.uniform(0.7, 1.3))
                for model, worse in (("a", 1.0), ("b", 1.6 if ch == "after_temp" else 1.02)):
                    mae = base * worse * float(rng.uniform(0.97, 1.03))
                    row = {"sample_idx": idx, "channel": ch, "dw_class": cl, "mae": mae, "rmse": mae * float(rng.uniform(1.2, 1.4)),
                           "laplacian_var_pred": lap_gt * float(rng.uniform(0.4, 1.2)) if cl == "overall" else "",
                           "laplacian_var_gt": lap_gt if cl == "overall" else "", **info}
                    out[model].append(row)
    return out


def reference_table(reference_dir):
    import pandas as pd
    rng = np.random.default_rng(7)
    paths = []
    for model, rows in reports(rng).items():
        path = os.path.join(OUT, f"model_{model}_evaluation.csv")
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(COLUMNS)
            for r in rows:
                w.writerow([r[k] for k in COLUMNS])
        paths.append(path)
    try:
        import typer  # noqa: F401
    except ImportError:                                            # the module only decorates its command line with it
        stub = types.ModuleType("typer")
        stub.Typer = lambda *a, **k: types.SimpleNamespace(command=lambda *a, **k: (lambda fn: fn))
        stub.Argument = lambda *a, **k: None
        sys.modules["typer"] = stub
    spec = importlib.util.spec_from_file_location("reference_statistical_tests", os.path.join(reference_dir, "test", "statistical_tests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    names = [os.path.basename(p).replace("_evaluation.csv", "") for p in paths]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mod.comparative_analysis([pd.read_csv(p) for p in paths], names)
    with open(os.path.join(OUT, "reference_table_stdout.txt"), "w") as f:
        f.write(buf.getvalue())
    print(buf.getvalue())


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", default=None, help="checkout of the reference project (for the table fixture)")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    ttest_cases()
    if a.reference:
        reference_table(a.reference)
