#!/usr/bin/env python3
"""Times ``rank_tests.RankStats.result()`` (``mau_rank_tests``: four launches and the read-back of the table) against scipy on the
host over the same columns -- the reference's way: ``wilcoxon`` per pair, ``mannwhitneyu`` per model, ``np.percentile`` of the
pooled values, per channel and metric.

    python scripts/rank_tests_bench.py [--n 1000 4000 16000] [--models 8] [--channels 2] [--repeats 5] [--no-scipy]

Pass the size of a test split with ``--n``.  Prints one JSON line per size.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mau_amd  # noqa: E402
from mau_amd import rank_tests as R  # noqa: E402


def scipy_seconds(cols, known):
    from scipy.stats import mannwhitneyu, wilcoxon
    known = known.astype(bool)
    t0 = time.perf_counter()
    for q in range(cols.shape[0]):
        for a, b in itertools.combinations(range(cols.shape[1]), 2):
            wilcoxon(cols[q, a], cols[q, b])
        for m in range(cols.shape[1]):
            mannwhitneyu(cols[q, m][known], cols[q, m][~known], alternative="two-sided")
        np.percentile(cols[q].reshape(-1), 98)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 4000, 16000])
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    for n in a.n:
        rows = rng.gamma(2.0, 0.05, (a.models, n, a.channels, 2))        # heavy-tailed, as per-sample errors are
        known = (rng.random(n) < 0.6).astype(np.uint8)
        stats = R.RankStats(a.models, a.channels, n)
        stats.update(torch.from_numpy(rows).cuda(), torch.from_numpy(known).cuda())
        table = stats.result()                                           # warm-up, and the check against the twin
        cols = rows.transpose(2, 3, 0, 1).reshape(2 * a.channels, a.models, n)
        t0 = time.perf_counter()
        want = R.rank_tests_host(cols, known)
        twin_s = time.perf_counter() - t0
        assert np.array_equal(table, want), "the device table differs from the twin"
        times = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats.result()
            times.append(time.perf_counter() - t0)
        out = {"n": n, "models": a.models, "channels": a.channels, "result_ms_median": 1e3 * float(np.median(times)),
               "result_ms_min": 1e3 * min(times), "numpy_twin_ms": 1e3 * twin_s}
        if not a.no_scipy:
            out["scipy_host_ms"] = 1e3 * scipy_seconds(cols, known)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
