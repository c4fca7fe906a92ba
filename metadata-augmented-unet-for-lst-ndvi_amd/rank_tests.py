"""Rank tests of checkpoints: the headline numbers of the developer app's *Statistical Comparison* page
(``app_dev/pages/3_Statistical_Comparison.py``) that need ranks -- section 7, the pairwise Wilcoxon signed-rank p-values; section 3,
Mann-Whitney U of known against unknown cities per model; sections 1-2, the pooled minimum and 98th percentile behind the axis range --
and section 4, the Pearson correlations of the metric with the sample's metadata.

Ranks come from COUNTING, in integers, not from sorting: for element i of a multiset v, ``less_i = #{j: v_j < v_i}`` and
``eq_i = #{j: v_j == v_i}`` (i included) give twice the mid-rank ``2 less_i + eq_i + 1`` and the tie term
``sum (t^3 - t) = sum_i (eq_i^2 - 1)``.  ``RankStats`` keeps the ``overall`` mae / rmse columns of every model on the device
(``update``, a slice copy per batch, no synchronisation) and ``result()`` runs ``mau_rank_tests`` (``csrc/rankstats.hip``): an O(n^2)
compare, one thread per i, ``TILE`` values of j staged in LDS per step, int64 partial sums joined by integer atomic adds.  Every entry
of the table is an exact integer (or the bit pattern of an input value), so any summation order gives the same bits and
``rank_tests_host``, the numpy twin (sort-based counting), reproduces the table to the bit.  The table's layout is in
``include/mau_hip.h``.

Statistics and p-values are plain Python from those integers, no scipy at run time, and follow ``scipy.stats.wilcoxon`` /
``mannwhitneyu(alternative='two-sided')`` with ``method='auto'`` (checked against scipy 1.15.3 in tests/test_rank_tests_host.py):

* Wilcoxon, zeros removed (``zero_method='wilcox'``), no continuity correction: T = min(W+, W-), mn = n (n + 1) / 4,
  se = sqrt(n (n + 1) (2 n + 1) / 24 - tie / 48), p = erfc(|T - mn| / se / sqrt 2); no used sample -> NaN.  The exact null
  distribution (all sign assignments of the mid-ranks, a dynamic programme over doubled rank sums) replaces it where scipy does so:
  at most 50 kept samples without ties or zeros, or at most 13 kept samples whatever the ties (scipy enumerates the 2^n sign
  flips there; the table's seventh pair entry carries the tie groups this needs).
* Mann-Whitney, two-sided, continuity corrected: U1 = R_known - n1 (n1 + 1) / 2, U = max(U1, n1 n2 - U1),
  s = sqrt(n1 n2 / 12 ((n + 1) - tie / (n (n - 1)))), p = min(1, erfc((U - n1 n2 / 2 - 1/2) / s / sqrt 2)); exact (the coefficients of
  the Gaussian binomial, Python integers) when min(n1, n2) <= 8 without ties; an empty group -> NaN.
* 98th percentile: numpy's linear rule between the two order statistics; ``ylim_min`` / ``ylim_max`` with the page's 5 % padding.

Difference from the reference, on purpose: for Mann-Whitney the page hands a model's NaNs to scipy, which answers NaN.  Here the
module's drop rule holds everywhere: a sample with a non-finite value in ANY of the M models is dropped for ALL of them, and the
row counts it (``skipped``).  For the Wilcoxon part this is the page's ``pivot_table(...).dropna()``.

Figures and the binned trend correlations of sections 9-11 are out of scope.
"""
from __future__ import annotations

import csv
import itertools
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import functional as F_
from .functional import call, lib

MAX_MODELS = 8
TILE = int(lib.mau_rank_tile())                    # values of j a workgroup stages per step
MAX_SAMPLES = int(lib.mau_rank_max_samples())      # 2^20: sum eq^2 stays inside int64
PAIR_ELEMS, MODEL_ELEMS, POOL_ELEMS = 7, 4, 4
SMALL = 13                                         # kept samples up to which the tie groups are written
METRICS = ("mae", "rmse")
CSV_COLUMNS = ("test", "channel", "metric", "model_1", "model_2", "n", "n_zero", "skipped", "statistic", "z", "p_value", "method",
               "mean_known", "mean_unknown", "mean_diff")
NAN = float("nan")


# --------------------------------------------------------------------------- #
# table layout
# --------------------------------------------------------------------------- #
def num_pairs(M: int) -> int:
    return M * (M - 1) // 2


def q_elems(M: int) -> int:
    return PAIR_ELEMS * num_pairs(M) + MODEL_ELEMS * M + POOL_ELEMS


def pair_entry(row: np.ndarray, p: int) -> np.ndarray:
    return row[PAIR_ELEMS * p:PAIR_ELEMS * (p + 1)]


def model_entry(row: np.ndarray, m: int, M: int) -> np.ndarray:
    at = PAIR_ELEMS * num_pairs(M) + MODEL_ELEMS * m
    return row[at:at + MODEL_ELEMS]


def pool_entry(row: np.ndarray, M: int) -> np.ndarray:
    return row[PAIR_ELEMS * num_pairs(M) + MODEL_ELEMS * M:]


# --------------------------------------------------------------------------- #
# the numpy twin
# --------------------------------------------------------------------------- #
def _counts(v: np.ndarray):
    """(less, eq) of every element of v by sorting."""
    s = np.sort(v)
    less = np.searchsorted(s, v, side="left").astype(np.int64)
    return less, np.searchsorted(s, v, side="right").astype(np.int64) - less


def rank_tests_host(cols, known) -> np.ndarray:
    """The int64 table (Q, q_elems(M)) of ``mau_rank_tests`` for cols (Q, M, N) float64 and known (N,): the same integers."""
    cols = np.asarray(cols, dtype=np.float64)
    if cols.ndim != 3 or not 1 <= cols.shape[1] <= MAX_MODELS or not 1 <= cols.shape[2] <= MAX_SAMPLES or cols.shape[0] < 1:
        raise ValueError(f"rank_tests_host: cols must be (Q, 1..{MAX_MODELS}, 1..{MAX_SAMPLES}), got {cols.shape}")
    Q, M, N = cols.shape
    known = np.asarray(known).reshape(-1) != 0
    if known.shape[0] != N:
        raise ValueError(f"rank_tests_host: {known.shape[0]} known flags for {N} samples")
    table = np.zeros((Q, q_elems(M)), dtype=np.int64)
    for q in range(Q):
        keep = np.isfinite(cols[q]).all(axis=0)
        x, kn = cols[q][:, keep], known[keep]
        nk = int(keep.sum())
        for p, (a, b) in enumerate(itertools.combinations(range(M), 2)):
            d = x[a] - x[b]
            used = d != 0.0
            du = d[used]
            less, eq = _counts(np.abs(du))
            twice = 2 * less + eq + 1
            small = int((np.int64(1) << (4 * less)).sum()) if nk <= SMALL else 0
            pair_entry(table[q], p)[:] = [du.size, nk - du.size, N - nk, twice[du > 0].sum(), twice[du < 0].sum(), (eq * eq - 1).sum(), small]
        for m in range(M):
            less, eq = _counts(x[m])
            twice = 2 * less + eq + 1
            model_entry(table[q], m, M)[:] = [kn.sum(), nk - kn.sum(), twice[kn].sum(), (eq * eq - 1).sum()]
        pooled = np.sort(x.reshape(-1) + 0.0)
        n = pooled.size
        if n:
            lo = (n - 1) * 49 // 50
            pool_entry(table[q], M)[:] = [n] + list(pooled[[0, lo, min(lo + 1, n - 1)]].view(np.int64))
    return table


# --------------------------------------------------------------------------- #
# statistics and p-values from the integers
# --------------------------------------------------------------------------- #
def _sign_flip_tail(ranks2: Sequence[int], w2: int) -> float:
    """min(1, 2 min(P(W <= w), P(W >= w))) of W = the sum of a uniformly random subset of the mid-ranks, all in doubled integers."""
    counts = [1]
    for r in ranks2:
        new = counts + [0] * r
        for s, c in enumerate(counts):
            new[s + r] += c
        counts = new
    le, ge = sum(counts[:w2 + 1]), sum(counts[w2:])
    return min(1.0, 2.0 * min(le, ge) / float(1 << len(ranks2)))


def wilcoxon_from_counts(n_used: int, n_zero: int, w_plus2: int, w_minus2: int, tie: int, small: int = 0) -> dict:
    """{'statistic', 'z', 'p_value', 'method'} of the two-sided signed-rank test from a pair's table entry."""
    n, kept = int(n_used), int(n_used) + int(n_zero)
    stat = min(w_plus2, w_minus2) / 2.0
    if kept == 0:
        return {"statistic": NAN, "z": NAN, "p_value": NAN, "method": "approx"}
    mn = n * (n + 1) / 4.0
    se = math.sqrt(max(n * (n + 1) * (2 * n + 1) / 24.0 - tie / 48.0, 0.0))
    z = (stat - mn) / se if se > 0.0 else NAN
    clean = tie == 0 and n_zero == 0
    if kept <= 50 and (clean or kept <= SMALL):
        if clean:
            ranks2 = [2 * (r + 1) for r in range(n)]
        else:                                                       # the tie group of size t that starts at position p: mid-rank p + (t + 1) / 2
            ranks2 = [2 * p + t + 1 for p in range(n) for t in [(int(small) >> (4 * p)) & 15] for _ in range(t)]
            if len(ranks2) != n:
                raise ValueError(f"wilcoxon_from_counts: the tie groups {int(small):#x} do not describe {n} used samples")
        return {"statistic": stat, "z": z, "p_value": _sign_flip_tail(ranks2, int(w_plus2)), "method": "exact"}
    p = math.erfc(abs(z) / math.sqrt(2.0)) if se > 0.0 else NAN
    return {"statistic": stat, "z": z, "p_value": p, "method": "approx"}


def _mwu_counts(n1: int, n2: int, kmax: int) -> List[int]:
    """Number of arrangements with U = 0..kmax of n1 against n2 values without ties: the coefficients of the Gaussian binomial
    prod_{i=1..n1} (1 - q^(n2+i)) / (1 - q^i)."""
    c = [1] + [0] * kmax
    for i in range(1, n1 + 1):
        d = n2 + i
        for k in range(kmax, d - 1, -1):
            c[k] -= c[k - d]
        for k in range(i, kmax + 1):
            c[k] += c[k - i]
    return c


def mannwhitney_from_counts(n_known: int, n_unknown: int, r_known2: int, tie: int) -> dict:
    """{'statistic' (U of the known cities), 'z', 'p_value', 'method'} of the two-sided test from a model's table entry."""
    n1, n2 = int(n_known), int(n_unknown)
    if n1 == 0 or n2 == 0:
        return {"statistic": NAN, "z": NAN, "p_value": NAN, "method": "approx"}
    n = n1 + n2
    u1 = r_known2 / 2.0 - n1 * (n1 + 1) / 2.0
    u = max(u1, n1 * n2 - u1)
    s = math.sqrt(n1 * n2 / 12.0 * ((n + 1) - tie / (n * (n - 1.0))))
    num = u - n1 * n2 / 2.0 - 0.5
    z = num / s if s > 0.0 else math.copysign(math.inf, num)
    if min(n1, n2) <= 8 and tie == 0:
        k = n1 * n2 - int(u)                                         # P(U' >= u) = P(U' <= n1 n2 - u)
        p = sum(_mwu_counts(min(n1, n2), max(n1, n2), k)) / math.comb(n, n1)
        return {"statistic": u1, "z": z, "p_value": min(1.0, 2.0 * p), "method": "exact"}
    return {"statistic": u1, "z": z, "p_value": min(1.0, math.erfc(z / math.sqrt(2.0))), "method": "approx"}


def axis_range(entry) -> dict:
    """{'n', 'min', 'p98', 'ylim_min', 'ylim_max'} of a pooled entry: ``np.percentile(values, 98)`` (linear) and the page's limits."""
    n = int(entry[0])
    if n == 0:
        return {"n": 0, "min": NAN, "p98": NAN, "ylim_min": NAN, "ylim_max": NAN}
    lowest, a, b = (float(v) for v in np.asarray(entry[1:4], dtype=np.int64).view(np.float64))
    virtual = (n - 1) * 0.98
    t = virtual - math.floor(virtual)
    p98 = b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t
    pad = (p98 - lowest) * 0.05
    return {"n": n, "min": lowest, "p98": p98, "ylim_min": max(0.0, lowest - pad), "ylim_max": p98 + pad}


def group_means(paired_table: np.ndarray, c: int, metric: str, M: int):
    """(mean of the known cities, of the unknown ones) per model, from the joint-moment table of ``statistics`` (the groups merged)."""
    from .statistics import GROUPS, OVERALL_METRICS, entry_elems, merge_entries
    out = []
    for groups in (range(4, GROUPS), range(0, 4)):
        e = np.zeros(entry_elems(M))
        for g in groups:
            e = merge_entries(e, paired_table[g, c, OVERALL_METRICS.index(metric)], M)
        out.append([float(e[2 + i]) if e[0] else NAN for i in range(M)])
    return out


def rank_test_rows(table: np.ndarray, names: Sequence[str], channels: Sequence[str], paired_table: Optional[np.ndarray] = None,
                   n_samples: Optional[int] = None) -> List[dict]:
    """One row of ``CSV_COLUMNS`` per test: per channel and metric the Wilcoxon tests of ``itertools.combinations(names, 2)``, then the
    Mann-Whitney test of every model.  ``paired_table`` (``statistics``' joint moments of the same samples) gives the group means,
    ``n_samples`` (all samples seen) the skipped count of a Mann-Whitney row when there is one model only."""
    M = len(names)
    table = np.asarray(table)
    if table.shape != (len(channels) * len(METRICS), q_elems(M)):
        raise ValueError(f"rank_test_rows: table {table.shape} does not fit {M} models and {len(channels)} channels")
    out = []
    for c, ch in enumerate(channels):
        for w, metric in enumerate(METRICS):
            row = [int(v) for v in table[c * len(METRICS) + w]]
            for p, (i, j) in enumerate(itertools.combinations(range(M), 2)):
                n_used, n_zero, skipped, wp, wm, tie, small = row[PAIR_ELEMS * p:PAIR_ELEMS * (p + 1)]
                out.append({"test": "wilcoxon", "channel": ch, "metric": metric, "model_1": names[i], "model_2": names[j], "n": n_used,
                            "n_zero": n_zero, "skipped": skipped, **wilcoxon_from_counts(n_used, n_zero, wp, wm, tie, small),
                            "mean_known": "", "mean_unknown": "", "mean_diff": ""})
            known, unknown = group_means(paired_table, c, metric, M) if paired_table is not None else ([NAN] * M, [NAN] * M)
            skipped = row[2] if M > 1 else None if n_samples is None else n_samples - row[0] - row[1]
            for m in range(M):
                n1, n2, r2, tie = model_entry(np.asarray(row), m, M)
                out.append({"test": "mannwhitney", "channel": ch, "metric": metric, "model_1": names[m], "model_2": "", "n": int(n1 + n2),
                            "n_zero": "", "skipped": "" if skipped is None else skipped,
                            **mannwhitney_from_counts(n1, n2, r2, tie), "mean_known": known[m], "mean_unknown": unknown[m],
                            "mean_diff": unknown[m] - known[m] if n1 and n2 else NAN})
    return out


def axis_ranges(table: np.ndarray, channels: Sequence[str], M: int) -> List[dict]:
    return [{"channel": ch, "metric": metric, **axis_range(pool_entry(np.asarray(table)[c * len(METRICS) + w], M))}
            for c, ch in enumerate(channels) for w, metric in enumerate(METRICS)]


def write_rank_tests(rows: Sequence[dict], output_dir: str, study_name: str) -> str:
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{study_name}_rank_tests.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for r in rows:
            w.writerow([r[k] for k in CSV_COLUMNS])
    return path


def format_tables(rows: Sequence[dict], names: Sequence[str], ranges: Sequence[dict] = ()) -> str:
    """The page's two tables: per channel and metric the matrix of pairwise Wilcoxon p-values (section 7, '.1e' as its heat map)
    and the known / unknown table (section 3, four decimals)."""
    lines = []
    keys = list(dict.fromkeys((r["channel"], r["metric"]) for r in rows))
    width = max([len(n) for n in names] + [10])
    for ch, metric in keys:
        sel = [r for r in rows if (r["channel"], r["metric"]) == (ch, metric)]
        lines += ["", f"--- Pairwise Wilcoxon P-Values ({ch}, {metric.upper()}) ---"]
        pv = {(r["model_1"], r["model_2"]): r["p_value"] for r in sel if r["test"] == "wilcoxon"}
        lines.append(" " * width + "".join(f" {n:>{width}}" for n in names))
        for a in names:
            cells = [NAN if a == b else pv.get((a, b), pv.get((b, a), NAN)) for b in names]
            lines.append(f"{a:<{width}}" + "".join(f" {v:>{width}.1e}" for v in cells))
        lines += ["", f"--- Known vs Unknown Cities: Mann-Whitney U ({ch}, {metric.upper()}) ---",
                  f"{'Model':<{width}} {'Mean (Known)':>14} {'Mean (Unknown)':>14} {'Diff':>10} {'p-value':>10} {'method':>7}"]
        for r in sel:
            if r["test"] == "mannwhitney":
                lines.append(f"{r['model_1']:<{width}} {r['mean_known']:>14.4f} {r['mean_unknown']:>14.4f} {r['mean_diff']:>10.4f} "
                             f"{r['p_value']:>10.4f} {r['method']:>7}")
        for g in ranges:
            if (g["channel"], g["metric"]) == (ch, metric):
                lines.append(f"98th percentile of the pooled {metric.upper()}: {g['p98']:.4f} (minimum {g['min']:.4f}, axis "
                             f"{g['ylim_min']:.4f} .. {g['ylim_max']:.4f}, n = {g['n']})")
    return "\n".join(lines)


# --------------------------------------------------------------------------- #
# from reports that already exist
# --------------------------------------------------------------------------- #
def columns_from_reports(report_paths_: Sequence[str], channels: Sequence[str]):
    """(cols (Q, M, N), known (N,)) of M ``*_evaluation.csv`` files of the SAME samples, sample order; a missing value is NaN."""
    per_model = []
    for path in report_paths_:
        with open(path, newline="") as f:
            per_model.append([r for r in csv.DictReader(f) if r["dw_class"] == "overall"])
    samples = sorted({int(r["sample_idx"]) for r in per_model[0]})
    at = {s: b for b, s in enumerate(samples)}
    cols = np.full((len(channels) * len(METRICS), len(report_paths_), len(samples)), np.nan)
    known = np.zeros(len(samples), dtype=np.uint8)
    for m, recs in enumerate(per_model):
        for r in recs:
            b, c = at[int(r["sample_idx"])], list(channels).index(r["channel"])
            known[b] = r["is_known_city"] == "True"
            for w, metric in enumerate(METRICS):
                cols[c * len(METRICS) + w, m, b] = float(r[metric]) if r[metric] != "" else np.nan
    return cols, known


def rank_tests_from_reports(report_paths_: Sequence[str], channels: Sequence[str] = ("after_ndvi", "after_temp"),
                            names: Optional[Sequence[str]] = None) -> List[dict]:
    """The rows ``compare_checkpoints(..., rank_tests=True)`` writes, for reports that already exist, through the numpy twin (as
    ``statistics.table_from_reports``)."""
    from .statistics import table_from_reports
    if names is None:
        names = [os.path.basename(p).replace("_evaluation.csv", "") for p in report_paths_]
    cols, known = columns_from_reports(report_paths_, channels)
    return rank_test_rows(rank_tests_host(cols, known), names, channels, table_from_reports(report_paths_, channels), cols.shape[2])


# --------------------------------------------------------------------------- #
# section 4: correlations with the metadata (host only: the rows cross to the host anyway)
# --------------------------------------------------------------------------- #
def pearson(x, y):
    """(r, two-sided p) as ``scipy.stats.pearsonr``: float64, p from Student's t with n - 2 degrees of freedom.  NaN for fewer than
    two samples, a constant or a non-finite input; n = 2 gives (+-1, 1)."""
    from .statistics import student_t_two_sided
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.size
    if n < 2 or not (np.isfinite(x).all() and np.isfinite(y).all()):
        return NAN, NAN
    xm, ym = x - x.mean(), y - y.mean()
    nx, ny = math.sqrt(float(np.dot(xm, xm))), math.sqrt(float(np.dot(ym, ym)))
    if nx == 0.0 or ny == 0.0:
        return NAN, NAN
    r = max(-1.0, min(1.0, float(np.dot(xm / nx, ym / ny))))
    if n == 2:
        return r, 1.0
    if abs(r) == 1.0:
        return r, 0.0
    df = n - 2.0
    return r, student_t_two_sided(r * math.sqrt(df / ((1.0 - r) * (1.0 + r))), df)


CORRELATION_VARIABLES = ("lat", "lon", "city_sample_count", "t1_year")


def metadata_correlations(rows: Sequence[dict], metrics: Sequence[str] = METRICS) -> List[dict]:
    """Section 4 of the page for ONE model's evaluation rows (``evaluate.metric_rows`` or a ``*_evaluation.csv`` read back): per
    channel and metric, Pearson r and p of the ``overall`` metric against lat, lon, the city's sample count (distinct sample
    indices of that city) and t1_year, over all samples and over known and unknown cities separately.  NaN where the page gives
    NaN: fewer than two samples, or a single year."""
    overall = [r for r in rows if r["dw_class"] == "overall"]
    per_city: Dict[str, set] = {}
    for r in rows:
        per_city.setdefault(r["city"], set()).add(int(r["sample_idx"]))
    out = []
    for ch in dict.fromkeys(r["channel"] for r in overall):
        sel = [r for r in overall if r["channel"] == ch]
        known = np.array([str(r["is_known_city"]) == "True" for r in sel], dtype=bool)
        var = {"lat": [float(r["lat"]) for r in sel], "lon": [float(r["lon"]) for r in sel],
               "city_sample_count": [float(len(per_city[r["city"]])) for r in sel], "t1_year": [float(r["t1_year"]) for r in sel]}
        for metric in metrics:
            y = np.array([float(r[metric]) if r[metric] not in ("", None) else np.nan for r in sel])
            for subset, mask in (("all", np.ones(len(sel), dtype=bool)), ("known", known), ("unknown", ~known)):
                for name in CORRELATION_VARIABLES:
                    x = np.array(var[name])[mask]
                    single_year = name == "t1_year" and np.unique(x).size <= 1
                    r, p = (NAN, NAN) if single_year else pearson(y[mask], x)
                    out.append({"channel": ch, "metric": metric, "subset": subset, "variable": name, "n": int(mask.sum()), "r": r, "p_value": p})
    return out


# --------------------------------------------------------------------------- #
# the device side
# --------------------------------------------------------------------------- #
class RankStats:
    """The device-resident column store (channels x {mae, rmse}, models, capacity) of every sample seen by :meth:`update`, and the
    rank-test table of those samples (:meth:`result`)."""

    def __init__(self, models: int, channels: int, capacity: int, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RankStats: this is the MI355X-native path; it has no CPU fallback (rank_tests_host is the numpy twin)")
        if not 1 <= models <= MAX_MODELS:
            raise ValueError(f"RankStats: the number of models must be in [1, {MAX_MODELS}], got {models}")
        if channels < 1 or not 1 <= capacity <= MAX_SAMPLES:
            raise ValueError(f"RankStats: at least one channel and a capacity in [1, {MAX_SAMPLES}], got {channels} and {capacity}")
        self.models, self.channels, self.capacity = int(models), int(channels), int(capacity)
        self.Q = self.channels * len(METRICS)
        self.n = 0
        self.cols = torch.full((self.Q, self.models, self.capacity), NAN, dtype=torch.float64, device=self.device)
        self.known = torch.zeros(self.capacity, dtype=torch.uint8, device=self.device)
        assert lib.mau_rank_table_elems(self.models, self.Q) == self.Q * q_elems(self.models)
        self.table = torch.empty((self.Q, q_elems(self.models)), dtype=torch.int64, device=self.device)
        self.ws = torch.empty(lib.mau_rank_ws_elems(self.Q, self.capacity), dtype=torch.int64, device=self.device)

    def update(self, rows: torch.Tensor, known: torch.Tensor) -> None:
        """Appends a batch: rows (M, B, C, row_elems) fp64 as ``statistics.eval_metrics_multi`` returns them (entries [0] mae and [1]
        rmse of the ``overall`` row are kept), known (B,) uint8, both on the device.  Two slice copies, no host synchronisation."""
        F_._require_cuda(rows, "RankStats.update(rows)")
        F_._require_cuda(known, "RankStats.update(known)")
        if rows.dtype != torch.float64:
            raise TypeError(f"RankStats.update: rows must be float64, got {rows.dtype}")
        if known.dtype != torch.uint8:
            raise TypeError(f"RankStats.update: known must be uint8, got {known.dtype}")
        if rows.dim() != 4 or rows.shape[0] != self.models or rows.shape[2] != self.channels or rows.shape[3] < 2 or rows.shape[1] == 0:
            raise ValueError(f"RankStats.update: rows must be ({self.models}, B, {self.channels}, row_elems), got {tuple(rows.shape)}")
        B = rows.shape[1]
        if tuple(known.shape) != (B,):
            raise ValueError(f"RankStats.update: known must be ({B},), got {tuple(known.shape)}")
        if self.n + B > self.capacity:
            raise ValueError(f"RankStats.update: {self.n} + {B} samples exceed the capacity {self.capacity}")
        view = self.cols.view(self.channels, len(METRICS), self.models, self.capacity)
        view[..., self.n:self.n + B].copy_(rows[..., :len(METRICS)].permute(2, 3, 0, 1))
        self.known[self.n:self.n + B].copy_(known)
        self.n += B

    def result(self) -> np.ndarray:
        """Runs the kernels on the current stream and reads the table back: the single read-back.  (Q, q_elems(M)) int64."""
        if self.n == 0:
            raise ValueError("RankStats.result: no sample")
        call("mau_rank_tests", self.cols.data_ptr(), self.known.data_ptr(), self.table.data_ptr(), self.ws.data_ptr(), self.models,
             self.Q, self.n, self.capacity, F_._stream())
        return self.table.cpu().numpy()


def rank_tests_device(cols: torch.Tensor, known: torch.Tensor, n: Optional[int] = None) -> np.ndarray:
    """``mau_rank_tests`` on a column store as it is: cols (Q, M, Ncap) fp64 and known (>= n,) uint8 on the device, the first ``n``
    (default Ncap) samples of every column."""
    F_._require_cuda(cols, "rank_tests_device(cols)")
    F_._require_cuda(known, "rank_tests_device(known)")
    if cols.dtype != torch.float64:
        raise TypeError(f"rank_tests_device: cols must be float64, got {cols.dtype}")
    if known.dtype != torch.uint8:
        raise TypeError(f"rank_tests_device: known must be uint8, got {known.dtype}")
    if cols.dim() != 3:
        raise ValueError(f"rank_tests_device: cols must be (Q, M, Ncap), got {tuple(cols.shape)}")
    Q, M, cap = cols.shape
    n = cap if n is None else int(n)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"rank_tests_device: M must be in [1, {MAX_MODELS}], got {M}")
    if not 1 <= n <= min(cap, MAX_SAMPLES) or Q < 1:
        raise ValueError(f"rank_tests_device: 1 <= n <= min(Ncap, {MAX_SAMPLES}) and Q >= 1, got n = {n}, Ncap = {cap}, Q = {Q}")
    if known.dim() != 1 or known.shape[0] < n:
        raise ValueError(f"rank_tests_device: known must hold {n} flags, got {tuple(known.shape)}")
    cols, known = cols.contiguous(), known.contiguous()
    table = torch.empty((Q, q_elems(M)), dtype=torch.int64, device=cols.device)
    ws = torch.empty(lib.mau_rank_ws_elems(Q, n), dtype=torch.int64, device=cols.device)
    call("mau_rank_tests", cols.data_ptr(), known.data_ptr(), table.data_ptr(), ws.data_ptr(), M, Q, n, cap, F_._stream())
    return table.cpu().numpy()
