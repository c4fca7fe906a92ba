"""Statistical comparison of checkpoints (the reference's ``test/statistical_tests.py`` and the numbers of the developer app's
*Statistical Comparison* page, ``app_dev/pages/3_Statistical_Comparison.py``): paired t-tests of M checkpoints per channel and
land-cover class, on known and on unknown cities and per temporal distance, from ONE pass over the ``test`` split.

The reference evaluates every checkpoint in a run of its own and joins the CSVs with pandas.  Here a batch is packed once, the M
forwards fill one (M, B, C, H, W) buffer and two launches follow:

* ``eval_metrics_multi`` (``mau_eval_metrics_multi``): all models' per-(sample, channel) rows, each with the bits ``eval_metrics``
  gives for that model alone; the target and the class map are read once, not once per model;
* ``PairedStats.update`` (``mau_paired_accumulate``): the batch merged into a device-resident table of joint moments -- per group
  (is_known_city x temporal distance), channel and slot (four overall metrics, mae / rmse per class) the count, the M means and the
  upper triangle of the co-moment matrix Cm_ij = sum (x_i - mean_i)(x_j - mean_j).

The rows cross to the host once per batch (they are the per-model ``*_evaluation.csv``), the table once at the end; no output map
does.  One table serves the paired t-test of models i, j (mean difference mean_i - mean_j, variance of the differences
(Cm_ii + Cm_jj - 2 Cm_ij) / (n - 1)), the page's sample-wise error correlation Cm_ij / sqrt(Cm_ii Cm_jj) and its global summary
(mean and standard deviation per model, the groups merged on the host with the pairwise update of ``ground_truth.merge_moments``
extended to co-moments).

    python -m mau_amd.statistics a.pth b.pth [c.pth ...] --processed-dir data/processed --device gpu [--study-name test]
           [--jobid J] [--batch-size N] [--precision P] [--metrics-json F] [--output-dir reports/tests] [--rank-tests]

writes each model's ``*_evaluation.csv`` / ``*_info.csv``, ``<study>_paired_tests.csv`` and prints the reference's table; with one
checkpoint it prints the single-model interpretation (thresholds and layout of ``interpret_metrics``, the verdicts in this
project's words).

Difference from the reference, on purpose: the reference drops a sample PER PAIR when either value is NaN.  Here a non-finite value
of ANY of the M models drops the sample from that entry for ALL models, and the entry counts it (``skipped``).  With finite outputs
the two agree.

``paired_accumulate_host`` is the float64 twin of the kernel, operation for operation.  The Student-t survival function is the
regularised incomplete beta function by Lentz's continued fraction in plain Python: no scipy, no pandas at run time.

``--rank-tests`` adds the page's rank tests from the same pass (``rank_tests.RankStats``: the overall mae / rmse columns stay on the
device, ``mau_rank_tests`` ranks them by counting, one more read-back): the pairwise Wilcoxon p-values, Mann-Whitney U of known
against unknown cities and the pooled 98th percentile, written to ``<study>_rank_tests.csv`` and printed as the page's two tables.
Without the flag nothing changes.  Plots and the page's binned trend correlations are out of scope: they need figures and read
the per-sample CSVs this tool writes.
"""
from __future__ import annotations

import argparse
import csv
import itertools
import logging
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import functional as F_
from .evaluate import (DW_CLASS_NAMES, MAX_CLASSES, _HEAD, _checked_args, metric_rows, network_inputs, open_test_split, report_paths,
                       tag_of, walk_test_split, write_reports, EvalMetrics)
from .functional import call, lib

log = logging.getLogger(__name__)

MAX_MODELS = 8
GROUPS = 8                                                        # include/mau_hip.h, mau_paired_accumulate
TEMPORAL = ("long_distance", "mid_distance", "short_distance", "other")
OVERALL_METRICS = ("mae", "rmse", "laplacian_var_pred", "laplacian_var_gt")
CSV_COLUMNS = ("model_1", "model_2", "metric", "is_known_city", "temporal_distance", "channel", "dw_class", "n", "mean_diff", "t",
               "p_value", "winner", "pearson_r")
ALPHA = 0.05


# --------------------------------------------------------------------------- #
# groups and table layout
# --------------------------------------------------------------------------- #
def temporal_distance(t1_year: int) -> int:
    """Index into ``TEMPORAL`` (statistical_tests.py:12-20)."""
    if t1_year <= 2021:
        return 0
    if t1_year in (2022, 2023):
        return 1
    if t1_year > 2023:
        return 2
    return 3


def group_id(is_known_city: bool, t1_year: int) -> int:
    return 4 * int(bool(is_known_city)) + temporal_distance(t1_year)


def entry_elems(M: int) -> int:
    """n, skipped, mean[M], the upper triangle of Cm."""
    return 2 + M + M * (M + 1) // 2


def num_slots(num_classes: int) -> int:
    return len(OVERALL_METRICS) + 2 * num_classes


def tri_index(i: int, j: int, M: int) -> int:
    """Place of Cm[i][j] (i <= j) in the row-major upper triangle."""
    i, j = (i, j) if i <= j else (j, i)
    return i * M - i * (i - 1) // 2 + (j - i)


def slot_column(slot: int, num_classes: int):
    """(row entry a slot reads, row entry of the class's pixel count or None)."""
    if slot < len(OVERALL_METRICS):
        return slot, None
    k, w = divmod(slot - len(OVERALL_METRICS), 2)
    return _HEAD + num_classes * (1 + w) + k, _HEAD + k


def slot_of(metric: str, dw_class: str, class_names: Sequence[str]) -> int:
    if dw_class == "overall":
        return OVERALL_METRICS.index(metric)
    return len(OVERALL_METRICS) + 2 * list(class_names).index(dw_class) + ("mae", "rmse").index(metric)


def new_table(M: int, channels: int, num_classes: int) -> np.ndarray:
    return np.zeros((GROUPS, channels, num_slots(num_classes), entry_elems(M)), dtype=np.float64)


def paired_accumulate_host(table: np.ndarray, rows, groups, num_classes: int) -> np.ndarray:
    """The float64 twin of ``mau_paired_accumulate``: merges rows (M, B, C, 11 + 3 num_classes) of one batch, groups (B,) ids, into
    table (GROUPS, C, 4 + 2 num_classes, entry_elems(M)) in place, sample by sample with the kernel's update (Python floats are
    IEEE doubles and nothing is contracted).  Returns the table."""
    rows = np.asarray(rows, dtype=np.float64)
    M, B, C, R = rows.shape
    if R != _HEAD + 3 * num_classes or table.shape != (GROUPS, C, num_slots(num_classes), entry_elems(M)):
        raise ValueError(f"paired_accumulate_host: rows {rows.shape} and table {table.shape} do not fit {num_classes} classes")
    groups = [int(g) for g in np.asarray(groups).reshape(-1)]
    if len(groups) != B:
        raise ValueError(f"paired_accumulate_host: {len(groups)} group ids for {B} samples")
    rl = rows.tolist()
    for b, g in enumerate(groups):
        if not 0 <= g < GROUPS:
            continue
        for c in range(C):
            for s in range(table.shape[2]):
                col, cnt = slot_column(s, num_classes)
                if cnt is not None and not rl[0][b][c][cnt] > 0.0:
                    continue
                e = table[g, c, s]
                x = [rl[m][b][c][col] for m in range(M)]
                if not all(math.isfinite(v) for v in x):
                    e[1] += 1.0
                    continue
                n = float(e[0]) + 1.0
                mean = [float(v) for v in e[2:2 + M]]
                d = [x[i] - mean[i] for i in range(M)]
                mean = [mean[i] + d[i] / n for i in range(M)]
                p = 2 + M
                for i in range(M):
                    for j in range(i, M):
                        e[p] = float(e[p]) + d[i] * (x[j] - mean[j])
                        p += 1
                e[0] = n
                e[2:2 + M] = mean
    return table


def merge_entries(a: np.ndarray, b: np.ndarray, M: int) -> np.ndarray:
    """The entry of the union of two disjoint sample sets: ``ground_truth.merge_moments`` extended to co-moments,
    Cm_ij = (Cm_a + Cm_b) + delta_i delta_j (n_a n_b / n).  An empty side gives the other as it is (the skipped counts add)."""
    na, nb = float(a[0]), float(b[0])
    out = np.array(b if na == 0.0 else a, dtype=np.float64)
    out[1] = a[1] + b[1]
    if na == 0.0 or nb == 0.0:
        return out
    n = na + nb
    delta = b[2:2 + M] - a[2:2 + M]
    out[0] = n
    out[2:2 + M] = a[2:2 + M] + (delta * nb) / n
    p = 2 + M
    for i in range(M):
        for j in range(i, M):
            out[p] = (a[p] + b[p]) + (delta[i] * delta[j]) * ((na * nb) / n)
            p += 1
    return out


def global_summary(table: np.ndarray, names: Sequence[str], channels: Sequence[str]) -> List[dict]:
    """The page's global performance summary (section 1): per channel, overall metric and model the mean and the sample standard
    deviation over ALL groups, the groups merged on the host."""
    M = len(names)
    out = []
    for c, ch in enumerate(channels):
        for s, metric in enumerate(OVERALL_METRICS):
            e = np.zeros(entry_elems(M))
            for g in range(GROUPS):
                e = merge_entries(e, table[g, c, s], M)
            n = e[0]
            for i, name in enumerate(names):
                var = e[2 + M + tri_index(i, i, M)] / (n - 1) if n >= 2 else float("nan")
                out.append({"model": name, "channel": ch, "metric": metric, "n": int(n), "mean": float(e[2 + i]) if n else float("nan"),
                            "std": math.sqrt(var) if var >= 0 else float("nan")})
    return out


# --------------------------------------------------------------------------- #
# Student's t, without scipy
# --------------------------------------------------------------------------- #
def _betacf(a: float, b: float, x: float) -> float:
    """The continued fraction of the incomplete beta function by the modified Lentz method."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def betainc(a: float, b: float, x: float, xc: Optional[float] = None) -> float:
    """The regularised incomplete beta function I_x(a, b); ``xc`` = 1 - x where the caller has it without cancellation."""
    if xc is None:
        xc = 1.0 - x
    if x <= 0.0:
        return 0.0
    if xc <= 0.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(xc))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, xc) / b


def student_t_two_sided(t: float, df: float) -> float:
    """P(|T| >= |t|) of Student's t with ``df`` degrees of freedom = I_{df / (df + t^2)}(df / 2, 1 / 2).  NaN for a NaN t, 0 for an
    infinite one."""
    if math.isnan(t) or df <= 0:
        return float("nan")
    if math.isinf(t):
        return 0.0
    t2 = t * t
    return betainc(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2))


def paired_t(n: float, mean_d: float, var_d: float):
    """(t, two-sided p) of a paired t-test from the count, the mean and the sample variance of the differences, the degenerate
    cases as scipy.stats.ttest_rel has them: no spread and no difference -> (NaN, NaN); no spread, a difference -> (+-inf, 0)."""
    if n < 2 or math.isnan(mean_d) or math.isnan(var_d):
        return float("nan"), float("nan")
    se = math.sqrt(max(var_d, 0.0) / n)
    if se == 0.0:
        t = float("nan") if mean_d == 0.0 else math.copysign(float("inf"), mean_d)
    else:
        t = mean_d / se
    return t, student_t_two_sided(t, n - 1.0)


def paired_tests(table: np.ndarray, names: Sequence[str], channels: Sequence[str] = ("after_ndvi", "after_temp"),
                 class_names: Sequence[str] = DW_CLASS_NAMES) -> List[dict]:
    """The reference's comparative analysis (statistical_tests.py:118-168) from the table: for each pair of
    ``itertools.combinations(names, 2)``, metric in (mae, rmse) and entry with n >= 2, in the reference's order (pandas sorts the
    group keys: unknown before known cities, then temporal distance, channel and class name alphabetically), a row of
    ``CSV_COLUMNS``.  Winner (:161-166): p < 0.05 and mean_diff > 0 -> model 2 (lower is better), p < 0.05 otherwise -> model 1,
    else 'Insignificant'."""
    M = len(names)
    G, C, S, E = table.shape
    nc = (S - len(OVERALL_METRICS)) // 2
    if G != GROUPS or E != entry_elems(M) or C != len(channels) or nc > len(class_names):
        raise ValueError(f"paired_tests: table {table.shape} does not fit {M} models, {len(channels)} channels, {len(class_names)} class names")
    classes = ["overall"] + list(class_names[:nc])
    out = []
    for (i, m1), (j, m2) in itertools.combinations(enumerate(names), 2):
        for metric in ("mae", "rmse"):
            for known in (False, True):
                for td in sorted(TEMPORAL):
                    g = 4 * int(known) + TEMPORAL.index(td)
                    for c in sorted(range(C), key=lambda q: channels[q]):
                        for cl in sorted(classes):
                            e = table[g, c, slot_of(metric, cl, class_names)]
                            n = float(e[0])
                            if n < 2:
                                continue
                            cii, cjj, cij = (float(e[2 + M + tri_index(a, b, M)]) for a, b in ((i, i), (j, j), (i, j)))
                            mean_diff = float(e[2 + i]) - float(e[2 + j])
                            t, p = paired_t(n, mean_diff, ((cii + cjj) - 2.0 * cij) / (n - 1.0))
                            winner = "Insignificant"
                            if p < ALPHA:
                                winner = m2 if mean_diff > 0 else m1
                            den = math.sqrt(cii * cjj) if cii >= 0 and cjj >= 0 else float("nan")
                            out.append({"model_1": m1, "model_2": m2, "metric": metric, "is_known_city": known, "temporal_distance": td,
                                        "channel": channels[c], "dw_class": cl, "n": int(n), "mean_diff": mean_diff, "t": t, "p_value": p,
                                        "winner": winner, "pearson_r": cij / den if den > 0 else float("nan")})
    return out


def format_table(tests: Sequence[dict], names: Sequence[str]) -> str:
    """What the reference prints for these rows (statistical_tests.py:118-168), line for line."""
    lines = ["", "--- Comparative Analysis: Paired T-Test Results ---",
             "A low p-value (< 0.05) suggests a statistically significant difference between models."]
    for m1, m2 in itertools.combinations(names, 2):
        lines += ["", f"--- Comparing {m1} vs {m2} ---"]
        for metric in ("mae", "rmse"):
            lines += ["", f"** Metric: {metric.upper()} **",
                      f"{'Known/Unknown':<15} {'Temporal Dist':<15} {'Channel':<15} {'DW Class':<20} {'Mean Diff (M1-M2)':<20} {'P-Value':<10} {'Winner'}",
                      "-" * 120]
            for r in tests:
                if (r["model_1"], r["model_2"], r["metric"]) == (m1, m2, metric):
                    known = "Known" if r["is_known_city"] else "Unknown"
                    lines.append(f"{known:<15} {r['temporal_distance']:<15} {r['channel']:<15} {r['dw_class']:<20} "
                                 f"{r['mean_diff']:<20.4f} {r['p_value']:<10.4f} {r['winner']}")
    return "\n".join(lines)


def format_interpretation(table: np.ndarray, name: str, channels: Sequence[str]) -> str:
    """The single-model reading of the overall metrics per group (the layout and thresholds of ``interpret_metrics``,
    statistical_tests.py:23-88), from the same table with M = 1."""
    lines = [f"--- Individual Analysis for {name} ---", "", f"--- Interpreting metrics for {name} ---", "",
             "Note: MAE and RMSE are errors of a regression: lower is better."]
    for known in (False, True):
        for td in sorted(TEMPORAL):
            g = 4 * int(known) + TEMPORAL.index(td)
            if not table[g, :, :len(OVERALL_METRICS), 0].any():
                continue
            lines += ["", f"--- Analysis for {'Known Cities' if known else 'Unknown Cities'} | Temporal Distance: {td} ---"]
            for c in sorted(range(len(channels)), key=lambda q: channels[q]):
                mae, rmse, lp, lgt = (float(table[g, c, s, 2]) if table[g, c, s, 0] > 0 else float("nan") for s in range(4))
                lines += ["", f"Channel: {channels[c]}", f"  MAE: {mae:.4f}, RMSE: {rmse:.4f}"]
                if "temp" in channels[c]:
                    verdict = "excellent (mean error below 2 degrees C)" if mae < 2.0 else \
                        "good (mean error below 4 degrees C)" if mae < 4.0 else "needs improvement (mean error of 4 degrees C or more)"
                    lines.append(f"  Interpretation (°C deviation): {verdict}")
                elif "ndvi" in channels[c]:
                    verdict = "excellent (mean error below 2.5% of the NDVI range)" if mae < 0.05 else \
                        "good (mean error below 5% of the NDVI range)" if mae < 0.1 else "needs improvement (mean error of 5% of the NDVI range or more)"
                    lines.append(f"  Interpretation (NDVI deviation): {verdict}")
                if not math.isnan(lp) and not math.isnan(lgt) and lgt > 0:
                    ratio = lp / lgt
                    lines.append(f"  Smoothness (Laplacian Var): Pred={lp:.4f}, GT={lgt:.4f}, Ratio={ratio:.2f}")
                    verdict = "noisier than the ground truth: possible artefacts" if ratio > 1.5 else \
                        "smoother than the ground truth: fine detail is lost" if ratio < 0.5 else "a realistic level of detail"
                    lines.append(f"  Interpretation (Smoothness): {verdict}")
                else:
                    lines.append("  Smoothness: Not available (GT Laplacian variance is zero or NaN).")
    return "\n".join(lines)


def write_paired_tests(tests: Sequence[dict], output_dir: str, study_name: str) -> str:
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{study_name}_paired_tests.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for r in tests:
            w.writerow([r[k] for k in CSV_COLUMNS])
    return path


def table_from_reports(report_paths_: Sequence[str], channels: Sequence[str], class_names: Sequence[str] = DW_CLASS_NAMES) -> np.ndarray:
    """The table of M ``*_evaluation.csv`` files of the SAME samples, through the host twin (one batch, sample order): what the
    device pass gives, for reports that already exist."""
    M, nc = len(report_paths_), len(class_names)
    per_model = []
    for path in report_paths_:
        with open(path, newline="") as f:
            per_model.append(list(csv.DictReader(f)))
    samples = sorted({int(r["sample_idx"]) for r in per_model[0]})
    at = {s: b for b, s in enumerate(samples)}
    rows = np.full((M, len(samples), len(channels), _HEAD + 3 * nc), np.nan)
    rows[..., _HEAD:_HEAD + nc] = 0.0
    groups = [GROUPS] * len(samples)
    for m, recs in enumerate(per_model):
        for r in recs:
            b, c = at[int(r["sample_idx"])], list(channels).index(r["channel"])
            groups[b] = group_id(r["is_known_city"] == "True", int(r["t1_year"]))
            val = lambda k: float(r[k]) if r[k] != "" else float("nan")                          # noqa: E731
            if r["dw_class"] == "overall":
                rows[m, b, c, :4] = [val(k) for k in OVERALL_METRICS]
            else:
                k = list(class_names).index(r["dw_class"])
                rows[m, b, c, _HEAD + k] = 1.0
                rows[m, b, c, _HEAD + nc + k], rows[m, b, c, _HEAD + 2 * nc + k] = val("mae"), val("rmse")
    rows[1:, ..., _HEAD:_HEAD + nc] = rows[:1, ..., _HEAD:_HEAD + nc]
    return paired_accumulate_host(new_table(M, len(channels), nc), rows, groups, nc)


# --------------------------------------------------------------------------- #
# the kernels
# --------------------------------------------------------------------------- #
def eval_metrics_multi(outputs: torch.Tensor, targets: torch.Tensor, cls: torch.Tensor, scale=None, shift=None,
                       num_classes: int = len(DW_CLASS_NAMES), ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rows of M models against one target in ONE launch: outputs (M, B, C, H, W) fp32, targets (B, C, H, W) fp32, cls (B, H, W)
    uint8, all on the device -> (M, B, C, row_elems) fp64 device tensor; ``rows[m]`` has exactly the bits of
    ``evaluate.eval_metrics(outputs[m], targets, cls, ...).rows``, whatever M and the model's place.  1 <= M <= 8."""
    outputs, targets, cls, scale, shift = _checked_args("eval_metrics_multi", outputs, targets, cls, scale, shift, num_classes, MAX_MODELS)
    M, B, C, H, W = outputs.shape
    dev = outputs.device
    rows = torch.empty((M, B, C, lib.mau_eval_metrics_row_elems(num_classes)), dtype=torch.float64, device=dev)
    need = lib.mau_eval_metrics_multi_ws_elems(M, B, C, H, W, num_classes)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=dev)
    call("mau_eval_metrics_multi", outputs.data_ptr(), targets.data_ptr(), cls.data_ptr(), scale.data_ptr(), shift.data_ptr(),
         rows.data_ptr(), ws.data_ptr(), F_._tickets(dev).data_ptr(), M, B, C, H, W, num_classes, F_._stream())
    return rows


class PairedStats:
    """The device-resident table (GROUPS, channels, 4 + 2 num_classes, entry_elems(M)) over every sample seen by :meth:`update`."""

    def __init__(self, models: int, channels: int, num_classes: int = len(DW_CLASS_NAMES), device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PairedStats: this is the MI355X-native path; it has no CPU fallback (paired_accumulate_host is the numpy twin)")
        if not 1 <= models <= MAX_MODELS:
            raise ValueError(f"PairedStats: the number of models must be in [1, {MAX_MODELS}], got {models}")
        if channels < 1 or not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"PairedStats: at least one channel and 1..{MAX_CLASSES} classes")
        self.models, self.channels, self.num_classes = int(models), int(channels), int(num_classes)
        shape = (GROUPS, self.channels, num_slots(self.num_classes), entry_elems(self.models))
        assert math.prod(shape) == lib.mau_paired_table_elems(self.models, self.channels, self.num_classes)
        self.table = torch.zeros(shape, dtype=torch.float64, device=self.device)

    def update(self, rows: torch.Tensor, groups: torch.Tensor) -> None:
        """One launch on the current stream, no host synchronisation.  rows (M, B, C, row_elems) fp64 as ``eval_metrics_multi``
        returns them, groups (B,) uint8 (``group_id``; an id >= 8 drops the sample), both on the device."""
        F_._require_cuda(rows, "PairedStats.update(rows)")
        F_._require_cuda(groups, "PairedStats.update(groups)")
        if rows.dtype != torch.float64:
            raise TypeError(f"PairedStats.update: rows must be float64, got {rows.dtype}")
        if groups.dtype != torch.uint8:
            raise TypeError(f"PairedStats.update: groups must be uint8, got {groups.dtype}")
        R = lib.mau_eval_metrics_row_elems(self.num_classes)
        if rows.dim() != 4 or rows.shape[0] != self.models or rows.shape[2] != self.channels or rows.shape[3] != R or rows.shape[1] == 0:
            raise ValueError(f"PairedStats.update: rows must be ({self.models}, B, {self.channels}, {R}), got {tuple(rows.shape)}")
        B = rows.shape[1]
        if tuple(groups.shape) != (B,):
            raise ValueError(f"PairedStats.update: groups must be ({B},), got {tuple(groups.shape)}")
        rows, groups = rows.contiguous(), groups.contiguous()
        call("mau_paired_accumulate", rows.data_ptr(), groups.data_ptr(), self.table.data_ptr(), self.models, B, self.channels,
             self.num_classes, F_._stream())

    def result(self) -> np.ndarray:
        """The single read-back."""
        return self.table.cpu().numpy()


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
@torch.no_grad()
def compare_checkpoints(checkpoint_paths: Sequence[str], processed_dir: str, *, batch_size: Optional[int] = None,
                        precision: Optional[str] = None, study_name: str = "test", jobid: str = "", output_dir: str = "reports/tests",
                        metrics_json: Optional[str] = None, device: str = "cuda", rank_tests: bool = False) -> dict:
    """One pass over the ``test`` split of ``processed_dir`` for M checkpoints.  Writes every model's reports (as
    ``evaluate.evaluate_checkpoint`` does, same rows) and ``<study>_paired_tests.csv``.  Returns {'names', 'channels', 'table',
    'tests', 'rows' (per model), 'report_paths', 'info_paths', 'tests_path'}.  batch_size: default the first checkpoint's
    ``hyperparameters.batch_size``, else 16.  rank_tests: also the rank tests of ``rank_tests.py`` -- 'rank_table', 'rank_tests',
    'axis_ranges', 'rank_tests_path' (``<study>_rank_tests.csv``)."""
    from .checkpoint import resolve_embedding_flags
    M = len(checkpoint_paths)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"compare_checkpoints: between 1 and {MAX_MODELS} checkpoints, got {M}")
    models, ckpts, channels, scale, shift, known, loader = open_test_split(
        checkpoint_paths, processed_dir, batch_size=batch_size, precision=precision, study_name=study_name, metrics_json=metrics_json,
        device=device)
    Co = len(channels)
    idents = [(ck.get("model_type", "unet"), tag_of(*resolve_embedding_flags(ck, study_name)), ck.get("trial_id", "unknown")) for ck in ckpts]
    paths = [report_paths(output_dir, study_name, mt, tag, trial, jobid) for mt, tag, trial in idents]
    names = [os.path.basename(p[0]).replace("_evaluation.csv", "") for p in paths]                 # statistical_tests.py:193
    if len(set(names)) != M:
        raise ValueError(f"compare_checkpoints: the checkpoints' reports would overwrite each other ({names}): give them distinct trial ids")
    rows: List[List[dict]] = [[] for _ in range(M)]
    stats, buf, ws, ranks = None, None, None, None
    for _host, batch, sample_idx, infos in walk_test_split(loader, known, device):
        packed: Dict[torch.dtype, tuple] = {}                       # the batch is packed once per network dtype
        gids = [group_id(info["is_known_city"], info["t1_year"]) for info in infos]
        targets = None
        for m, model in enumerate(models):
            inputs, temp_series, metadata, targets = network_inputs(batch, model, ckpts[m], packed)
            out = model(inputs, temp_series, metadata)
            if buf is None or buf.shape[1:] != out.shape:
                buf = torch.empty((M,) + tuple(out.shape), dtype=torch.float32, device=out.device)
            buf[m].copy_(out)
        need = lib.mau_eval_metrics_multi_ws_elems(M, *buf.shape[1:], batch.num_classes)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.float64, device=buf.device)
        mrows = eval_metrics_multi(buf, targets, batch.cls_a, scale, shift, batch.num_classes, ws)
        if stats is None:
            stats = PairedStats(M, Co, batch.num_classes, buf.device)
        stats.update(mrows, torch.tensor(gids, dtype=torch.uint8).to(buf.device, non_blocking=True))
        if rank_tests:
            if ranks is None:
                from .rank_tests import RankStats
                ranks = RankStats(M, Co, len(loader.dataset), buf.device)
            ranks.update(mrows, torch.tensor([int(bool(info["is_known_city"])) for info in infos], dtype=torch.uint8).to(buf.device, non_blocking=True))
        host_rows = mrows.cpu()                                     # the one copy of the batch
        for m in range(M):
            rows[m] += metric_rows(EvalMetrics(host_rows[m], batch.num_classes), sample_idx, channels, infos)
    if stats is None:
        raise ValueError(f"compare_checkpoints: the test split of {processed_dir} is empty")
    table = stats.result()                                          # the one read-back of the table
    written = [write_reports(rows[m], output_dir, study_name, *idents[m], jobid) for m in range(M)]
    tests = paired_tests(table, names, channels, DW_CLASS_NAMES[:stats.num_classes] if stats.num_classes <= len(DW_CLASS_NAMES)
                         else [f"class_{k}" for k in range(stats.num_classes)])
    res = {"names": names, "channels": channels, "table": table, "tests": tests, "rows": rows,
           "report_paths": [w[0] for w in written], "info_paths": [w[1] for w in written],
           "tests_path": write_paired_tests(tests, output_dir, study_name)}
    if rank_tests:
        from . import rank_tests as R_
        rank_table = ranks.result()                                 # the one read-back of the rank tests
        rank_rows = R_.rank_test_rows(rank_table, names, channels, table, ranks.n)
        res.update(rank_table=rank_table, rank_tests=rank_rows, axis_ranges=R_.axis_ranges(rank_table, channels, M),
                   rank_tests_path=R_.write_rank_tests(rank_rows, output_dir, study_name))
    return res


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m mau_amd.statistics", description=__doc__.split("\n\n")[0])
    p.add_argument("checkpoint_paths", metavar="CHECKPOINT", nargs="+", help=f"1 to {MAX_MODELS} reference-layout .pth files")
    p.add_argument("--processed-dir", required=True, help="directory that holds the train/ and test/ splits")
    p.add_argument("--device", default="gpu", help="'gpu' or a torch device name; this path has no CPU fallback")
    p.add_argument("--study-name", default="test")
    p.add_argument("--jobid", default="")
    p.add_argument("--batch-size", type=int, default=None, help="default: the first checkpoint's hyperparameters.batch_size, else 16")
    p.add_argument("--precision", default=None, choices=["bf16", "fp16", "fp32"])
    p.add_argument("--metrics-json", default=None, help="normalization_metrics.json (default: the one in --processed-dir, if any)")
    p.add_argument("--output-dir", default="reports/tests")
    p.add_argument("--rank-tests", action="store_true", help="also the pairwise Wilcoxon and the known / unknown Mann-Whitney tests "
                   "(<study>_rank_tests.csv and the two tables)")
    a = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s")
    device = F_.argparse_device(p, a.device)
    if len(a.checkpoint_paths) > MAX_MODELS:
        p.error(f"at most {MAX_MODELS} checkpoints")
    res = compare_checkpoints(a.checkpoint_paths, a.processed_dir, batch_size=a.batch_size, precision=a.precision,
                              study_name=a.study_name, jobid=a.jobid, output_dir=a.output_dir, metrics_json=a.metrics_json, device=device,
                              rank_tests=a.rank_tests)
    for path in res["report_paths"]:
        print(f"Full evaluation report saved to {path}")
    print(f"Paired tests saved to {res['tests_path']}")
    if a.rank_tests:
        from .rank_tests import format_tables
        print(f"Rank tests saved to {res['rank_tests_path']}")
    if len(res["names"]) == 1:
        print(format_interpretation(res["table"], res["names"][0], res["channels"]))
        if a.rank_tests:
            print(format_tables(res["rank_tests"], res["names"], res["axis_ranges"]))
        return 0
    print(format_table(res["tests"], res["names"]))
    print("\n--- Global summary (all groups): mean (std) ---")
    for g in global_summary(res["table"], res["names"], res["channels"]):
        if g["metric"] in ("mae", "rmse"):
            print(f"{g['model']:<40} {g['channel']:<15} {g['metric']:<5} n={g['n']:<6} {g['mean']:.4f} ({g['std']:.4f})")
    if a.rank_tests:
        print(format_tables(res["rank_tests"], res["names"], res["axis_ranges"]))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
