"""Writes tests/golden/rankfix_cases.json, the fixture of tests/test_rank_tests_host.py: pairs of score columns with what the
installed scipy says about them.

    python tests/golden/make_rankfix.py

* ``cases``: n = 1..60, 200 and 1000 samples of two models, continuous values, values rounded to 0.01 (heavy ties, zero differences)
  and identical columns (every difference zero), stored as integers over a power of ten, each with four splits into known and unknown cities (about half, a few known
  ones -- the small group of the exact Mann-Whitney branch --, all, none).  Recorded: ``scipy.stats.wilcoxon(a, b)``,
  ``mannwhitneyu(known, unknown, alternative='two-sided')`` per model and split, ``np.percentile(pooled, 98)`` and the minimum --
  statistic, p-value and the BRANCH scipy's ``method='auto'`` took, observed by watching which of its own routines it called (the
  exact null distribution or the enumeration of sign flips: ``exact``; otherwise ``approx``), not derived from a reading of its rules.
  Where scipy raises (one sample whose difference is zero) the page's fallback, p = 1, is recorded with ``raised``.
* ``pearson``: vectors with ``scipy.stats.pearsonr``'s r and p.

Needs scipy; tests/test_rank_tests_host.py imports ``cases`` and ``scipy_results`` from here to repeat the comparison live.
"""
import json
import math
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = list(range(1, 61)) + [200, 1000]
KINDS = ("continuous", "rounded", "identical")
SPLITS = ("half", "few", "all", "none")


def _case(n, kind, k, half):
    """The case the tests see, from what the file holds: integer values over ``DIV[kind]`` (exact doubles), the second column of
    an identical pair left out, the `half` split as a string of 0 / 1; the other splits follow from n."""
    k = np.asarray(k, dtype=np.int64)
    x = np.stack([k[0], k[-1]]) / DIV[kind]
    masks = {"half": [int(c) for c in half], "few": [int(i < min(5, n - 1)) for i in range(n)], "all": [1] * n, "none": [0] * n}
    return {"name": f"n{n}_{kind}", "x": x.tolist(), "known": masks}


DIV = {"continuous": 1e7, "rounded": 100.0, "identical": 100.0}


def stored_cases():
    """(n, kind, integer values, the `half` split) of every case, as the file holds them."""
    rng = np.random.default_rng(20261020)
    out = []
    for n in SIZES:
        for kind in KINDS:
            k = rng.integers(500000, 3000000, (2, n)) if kind == "continuous" else rng.integers(5, 30, (2, n))
            if kind == "identical":
                k = k[:1]
            out.append((n, kind, k.tolist(), "".join("1" if v else "0" for v in rng.random(n) < 0.5)))
    return out


def cases():
    return [_case(*c) for c in stored_cases()]


def pack(res):
    """scipy_results() in the file's short form: [statistic, p, 'e' | 'a'] per test, the splits without a test left out."""
    short = lambda r: [r.get("statistic"), r["p"], r["method"][0]] + (["raised"] if r.get("raised") else [])   # noqa: E731
    return {"w": short(res["wilcoxon"]), "mw": {s: [short(r) for r in rows] for s, rows in res["mannwhitney"].items() if rows[0]},
            "p98": res["p98"], "min": res["min"]}


def unpack(rec):
    long = lambda r: {"statistic": r[0], "p": r[1], "method": {"e": "exact", "a": "approx"}[r[2]], "raised": len(r) > 3}   # noqa: E731
    return {"wilcoxon": long(rec["w"]), "mannwhitney": {s: [long(r) for r in rec["mw"][s]] if s in rec["mw"] else [None, None] for s in SPLITS},
            "p98": rec["p98"], "min": rec["min"]}


def load(path=None):
    """[(case, what scipy said)] and the pearson cases of the committed file."""
    with open(path or os.path.join(HERE, "rankfix_cases.json")) as f:
        d = json.load(f)
    return [(_case(c["n"], c["kind"], c["k"], c["half"]), unpack(c)) for c in d["cases"]], d["pearson"]


def _number(v):
    v = float(v)
    return None if math.isnan(v) else v


def scipy_results(case):
    """What scipy says about one case, with the branch it took."""
    import scipy.stats as st
    from scipy.stats import _mannwhitneyu as mw
    from scipy.stats import _wilcoxon as wx
    x = np.asarray(case["x"], dtype=np.float64)
    took = []

    class Watched(wx.WilcoxonDistribution):
        def __init__(self, *a, **k):
            took.append("exact")
            super().__init__(*a, **k)

    real_dist, real_perm, real_choose = wx.WilcoxonDistribution, st.permutation_test, mw._mwu_choose_method

    def perm(*a, **k):
        took.append("exact")
        return real_perm(*a, **k)

    def choose(*a, **k):
        took.append("exact" if real_choose(*a, **k) == "exact" else "approx")
        return real_choose(*a, **k)

    wx.WilcoxonDistribution, st.permutation_test, mw._mwu_choose_method = Watched, perm, choose
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                res = st.wilcoxon(x[0], x[1])
                out = {"wilcoxon": {"statistic": _number(res.statistic), "p": _number(res.pvalue), "method": took[-1] if took else "approx"}}
            except ValueError:                                         # one sample, a zero difference: scipy refuses to enumerate
                out = {"wilcoxon": {"raised": True, "p": 1.0, "method": took[-1]}}       # the page's `except ValueError: p = 1.0`
            out["mannwhitney"] = {}
            for split, mask in case["known"].items():
                mask = np.asarray(mask, dtype=bool)
                rows = []
                for m in range(2):
                    if mask.all() or not mask.any():
                        rows.append(None)                                  # the page does not call scipy with an empty group
                        continue
                    del took[:]
                    r = st.mannwhitneyu(x[m][mask], x[m][~mask], alternative="two-sided")
                    assert len(took) == 1
                    rows.append({"statistic": float(r.statistic), "p": float(r.pvalue), "method": took[0]})
                out["mannwhitney"][split] = rows
    finally:
        wx.WilcoxonDistribution, st.permutation_test, mw._mwu_choose_method = real_dist, real_perm, real_choose
    out["p98"] = float(np.percentile(x.reshape(-1), 98))
    out["min"] = float(x.min())
    return out


def pearson_cases():
    from scipy.stats import pearsonr
    rng = np.random.default_rng(4)
    out = []
    for n in (2, 3, 10, 200):
        for slope in (0.0, 0.05, 2.0):
            x = np.round(rng.uniform(-60, 60, n), 2)
            y = np.round(0.1 + slope * x / 60 + rng.standard_normal(n) * 0.05, 5)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = pearsonr(y, x)
            out.append({"n": n, "x": x.tolist(), "y": y.tolist(), "r": float(r.statistic), "p": float(r.pvalue)})
    return out


if __name__ == "__main__":
    import scipy
    recorded = [{"n": n, "kind": kind, "k": k, "half": half, **pack(scipy_results(_case(n, kind, k, half)))} for n, kind, k, half in stored_cases()]
    path = os.path.join(HERE, "rankfix_cases.json")
    with open(path, "w") as f:
        json.dump({"scipy": scipy.__version__, "numpy": np.__version__, "cases": recorded, "pearson": pearson_cases()}, f, separators=(",", ":"))
    print(f"{len(recorded)} cases, {os.path.getsize(path)} bytes")
