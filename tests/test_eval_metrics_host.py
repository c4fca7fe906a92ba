"""CPU-only checks of ``mau_amd.evaluate``: the float64 numpy truth the GPU tests compare ``mau_eval_metrics`` with (its
Laplacian against scipy.ndimage.laplace, its masked means against the direct spelling), ``dw_class_map`` against the numpy
rule of test/evaluate.py:212-217, the C ABI of the kernel (header, binding, refusals without a GPU) and the CSV writer."""
import csv
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = 11                      # row entries in front of the per-class blocks (include/mau_hip.h, mau_eval_metrics)


# --------------------------------------------------------------------------- #
# the truth (float64 numpy); tests/test_gpu_eval_metrics.py imports it from here
# --------------------------------------------------------------------------- #
def laplacian_truth(x):
    """5-point Laplacian x[i-1,j] + x[i+1,j] + x[i,j-1] + x[i,j+1] - 4 x[i,j] of a 2-D float64 field, the edge sample repeated
    beyond the border (numpy's 'symmetric' pad = scipy.ndimage's 'reflect')."""
    x = np.asarray(x, dtype=np.float64)
    e = np.pad(x, 1, mode="symmetric")
    return ((e[:-2, 1:-1] + e[2:, 1:-1]) + e[1:-1, :-2]) + e[1:-1, 2:] - 4.0 * x


def eval_truth(out, tgt, cls, scale, shift, ncls, with_lap_mean_squares=False):
    """Rows of ``mau_eval_metrics`` in float64 numpy: (B, C, 11 + 3 ncls), the layout of include/mau_hip.h.
    ``with_lap_mean_squares``: also (B, C, 2) = E[lap(p)^2], E[lap(g)^2], the scale of the variance entries' rounding error."""
    out, tgt, cls = np.asarray(out), np.asarray(tgt), np.asarray(cls)
    B, C, H, W = out.shape
    rows = np.full((B, C, HEAD + 3 * ncls), np.nan)
    e2 = np.zeros((B, C, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            for c in range(C):
                p = out[b, c].astype(np.float64) * float(scale[c]) + float(shift[c])
                g = tgt[b, c].astype(np.float64) * float(scale[c]) + float(shift[c])
                d = p - g
                r = rows[b, c]
                r[0] = np.abs(d).sum() / d.size
                r[1] = np.sqrt((d * d).sum() / d.size)
                for j, x in enumerate((p, g)):
                    lap = laplacian_truth(x)
                    r[2 + j] = np.var(lap)
                    e2[b, c, j] = np.mean(lap * lap)
                    r[4 + j] = np.count_nonzero(~np.isfinite((out, tgt)[j][b, c]))
                    r[6 + 2 * j] = np.fmin.reduce(x, axis=None, initial=np.inf)
                    r[7 + 2 * j] = np.fmax.reduce(x, axis=None, initial=-np.inf)
                r[10] = np.count_nonzero(cls[b] >= ncls)
                for k in range(ncls):
                    mask = cls[b] == k
                    n = np.count_nonzero(mask)
                    r[HEAD + k] = n
                    r[HEAD + ncls + k] = np.abs(d)[mask].sum() / n if n else np.nan
                    r[HEAD + 2 * ncls + k] = np.sqrt((d * d)[mask].sum() / n) if n else np.nan
    return (rows, e2) if with_lap_mean_squares else rows


def assert_rows_match(got, want, lap_e2, ncls, tol=1e-10):
    """The rule of the GPU tests: counts exact, NaN where the truth is NaN, every other entry within ``tol`` relative -- the
    two variance entries relative to E[lap^2] (what the error of E[x^2] - E[x]^2 scales with).  Returns the worst ratio
    |difference| / (tol * scale) seen."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    exact = [4, 5, 10] + list(range(HEAD, HEAD + ncls))
    assert np.array_equal(got[..., exact], want[..., exact]), "counts differ"
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN entries differ"
    scale = np.abs(want)
    scale[..., 2:4] = lap_e2
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinite entries differ"
    diff = np.abs(got - want)[fin]
    bound = tol * scale[fin]
    assert np.all(diff <= bound), f"worst |difference| / bound = {np.max(diff / np.maximum(bound, 1e-300)):.3g}"
    return float(np.max(diff / np.maximum(bound, 1e-300))) if diff.size else 0.0


def fake_tile(rng, H, W, nc=9, classes=None):
    """A dense 23-channel tile in the stacking order of the reference's processing (one-hot t1, 5 continuous planes, one-hot
    t2) and its two class maps."""
    pick = np.arange(nc) if classes is None else np.asarray(classes)
    a, b = rng.choice(pick, (H, W)), rng.integers(0, nc, (H, W))
    cont = rng.standard_normal((5, H, W)).astype(np.float32)
    dense = np.vstack([np.eye(nc)[a].transpose(2, 0, 1), cont, np.eye(nc)[b].transpose(2, 0, 1)]).astype(np.float32)
    return a, b, dense


def write_split(directory, rng, tiles, H=62, W=62):
    """``.npz`` tiles in the loader's format and file-name scheme.  tiles: (city, index, t1 (y, m), t2 (y, m), classes or None,
    series length).  Returns the file names in the loader's (sorted) order."""
    os.makedirs(directory, exist_ok=True)
    names = []
    for city, i, (y1, m1), (y2, m2), classes, n_ts in tiles:
        _a, _b, dense = fake_tile(rng, H, W, classes=classes)
        name = f"{city}_{i}_48.8566_2.3522_{y1}_{m1:02d}_to_{y2}_{m2:02d}.npz"
        np.savez_compressed(os.path.join(directory, name), input=dense, target=rng.standard_normal((2, H, W)).astype(np.float32),
                            metadata=rng.standard_normal(4).astype(np.float32), temperature_serie=rng.standard_normal(n_ts).astype(np.float32))
        names.append(name)
    return sorted(names)


# --------------------------------------------------------------------------- #
# the truth itself
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", [(31, 17), (1, 5), (1, 1)])
def test_truth_laplacian_is_scipys(shape):
    from scipy.ndimage import laplace
    x = np.random.default_rng(11).standard_normal(shape) * 7.3 + 21.5
    want = laplace(x.astype(np.float64))
    got = laplacian_truth(x)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(x))
    if 1 in shape:                                               # an axis of one pixel contributes nothing
        along = np.pad(x.reshape(-1), 1, mode="symmetric")
        assert np.allclose(got.reshape(-1), along[:-2] + along[2:] - 2 * x.reshape(-1), rtol=0, atol=1e-12 * np.max(np.abs(x)))
    if shape == (1, 1):
        assert got[0, 0] == 0.0


def test_truth_masked_means_are_the_direct_spelling():
    rng = np.random.default_rng(12)
    out, tgt = rng.standard_normal((2, 2, 13, 9)).astype(np.float32), rng.standard_normal((2, 2, 13, 9)).astype(np.float32)
    cls = rng.integers(0, 9, (2, 13, 9)).astype(np.uint8)
    cls[1][cls[1] == 4] = 5                                      # class 4 absent in sample 1
    scale, shift = [1.0, 7.3], [0.0, 21.5]
    rows, e2 = eval_truth(out, tgt, cls, scale, shift, 9, with_lap_mean_squares=True)
    assert rows.shape == (2, 2, HEAD + 27) and e2.shape == (2, 2, 2)
    for b in range(2):
        for c in range(2):
            p = out[b, c].astype(np.float64) * scale[c] + shift[c]
            g = tgt[b, c].astype(np.float64) * scale[c] + shift[c]
            assert np.isclose(rows[b, c, 0], np.mean(np.abs(p - g)), rtol=1e-13, atol=0)
            assert np.isclose(rows[b, c, 1], np.sqrt(np.mean((p - g) ** 2)), rtol=1e-13, atol=0)
            assert rows[b, c, 6] == p.min() and rows[b, c, 7] == p.max() and rows[b, c, 8] == g.min() and rows[b, c, 9] == g.max()
            assert rows[b, c, 4] == rows[b, c, 5] == rows[b, c, 10] == 0
            for k in range(9):
                mask = cls[b] == k
                assert rows[b, c, HEAD + k] == mask.sum()
                if mask.any():
                    assert np.isclose(rows[b, c, HEAD + 9 + k], np.mean(np.abs(p[mask] - g[mask])), rtol=1e-13, atol=0)
                    assert np.isclose(rows[b, c, HEAD + 18 + k], np.sqrt(np.mean((p[mask] - g[mask]) ** 2)), rtol=1e-13, atol=0)
                else:
                    assert (b, k) == (1, 4) and np.isnan(rows[b, c, HEAD + 9 + k]) and np.isnan(rows[b, c, HEAD + 18 + k])
    assert assert_rows_match(rows, rows, e2, 9) == 0.0
    worse = rows.copy()
    worse[0, 1, 1] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        assert_rows_match(worse, rows, e2, 9)


# --------------------------------------------------------------------------- #
# dw_class_map
# --------------------------------------------------------------------------- #
def numpy_class_rule(x, nc=9):
    return np.stack([np.argmax(np.stack([x[i, c] * c for c in range(nc)]), axis=0) for i in range(x.shape[0])])


def test_dw_class_map_follows_the_reference_rule():
    import mau_amd
    from mau_amd.evaluate import dw_class_map
    rng = np.random.default_rng(13)
    tiles = [fake_tile(rng, 20, 18) for _ in range(3)]
    dense = np.stack([t[2] for t in tiles])
    got = dw_class_map(torch.from_numpy(dense))
    assert got.dtype == torch.uint8 and got.shape == (3, 20, 18)
    assert np.array_equal(got.numpy(), numpy_class_rule(dense))
    for i, (a, _b, x) in enumerate(tiles):                       # a valid one-hot stack: the compact pipeline's map
        assert np.array_equal(got[i].numpy(), a) and np.array_equal(got[i].numpy(), mau_amd.data.compact_input(x)[0])
    # not one-hot: ties between weighted planes (the first maximum wins), an all-zero pixel (class 0), negative planes
    soft = rng.integers(-1, 3, (2, 23, 20, 18)).astype(np.float32)
    soft[0, :9, 0, 0] = 0
    soft[0, :9, 0, 1] = [0, 6, 3, 2, 0, 0, 1, 0, 0]              # 1*6 == 2*3 == 3*2 == 6*1: class 1
    soft[1, :9, 5, 5] = [5, 0, 0, 0, 0, 0, 0, 0, 0]              # plane 0 weighs nothing: all products 0 -> class 0
    got = dw_class_map(torch.from_numpy(soft)).numpy()
    assert np.array_equal(got, numpy_class_rule(soft))
    assert got[0, 0, 0] == 0 and got[0, 0, 1] == 1 and got[1, 5, 5] == 0
    assert np.array_equal(dw_class_map(torch.from_numpy(soft), num_classes=4).numpy(), numpy_class_rule(soft, 4))
    with pytest.raises(ValueError):
        dw_class_map(torch.zeros(1, 5, 4, 4))


# --------------------------------------------------------------------------- #
# C ABI
# --------------------------------------------------------------------------- #
def test_eval_metrics_is_part_of_the_c_abi():
    import ctypes
    import mau_amd
    from mau_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    syms = ("mau_eval_metrics", "mau_eval_metrics_ws_elems", "mau_eval_metrics_row_elems", "mau_eval_metrics_chunks")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in syms:
        assert f"{sym}(" in hdr and sym in _lib.PROTOTYPES and hasattr(raw, sym)
    assert len(_lib.PROTOTYPES["mau_eval_metrics"][1]) == 14
    assert _lib.lib.mau_abi_version() == 5 and "#define MAU_ABI_VERSION 5" in hdr
    assert mau_amd.evaluate.eval_metrics is not None and "evaluate" in mau_amd.__all__
    lib = _lib.lib
    # rows: 11 entries + count, MAE, RMSE per class; classes 1..16
    assert [lib.mau_eval_metrics_row_elems(n) for n in (1, 9, 16)] == [14, 38, 59]
    assert lib.mau_eval_metrics_row_elems(0) == 0 and lib.mau_eval_metrics_row_elems(17) == 0
    # chunks: a function of (H, W) alone; a 250 x 250 map is shared by several workgroups, a small one is not
    ch = lib.mau_eval_metrics_chunks
    assert ch(250, 250) > 1 and ch(8, 8) == ch(1, 1) == ch(5, 300) == 1 and ch(0, 4) == 0
    assert ch(500, 250) >= 2 * ch(250, 250) - 1
    # workspace: positive, monotone in every dimension, 0 for a shape the entry point refuses
    ws = lib.mau_eval_metrics_ws_elems
    assert ws(1, 1, 1, 1, 1) > 0
    per = lib.mau_reduce_tickets_elems()
    sizes = [ws(B, 2, 250, 250, 9) for B in (1, 2, 5, 16, per, 4 * per)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[1] == 2 * sizes[0]
    assert ws(2, 2, 250, 250, 9) <= ws(2, 2, 500, 250, 9) and ws(2, 2, 250, 250, 9) <= ws(2, 2, 250, 250, 16)
    assert ws(2, 1, 250, 250, 9) <= ws(2, 2, 250, 250, 9)
    assert ws(0, 2, 8, 8, 9) == 0 and ws(1, 2, 8, 8, 17) == 0
    # refusals, reported through mau_last_error, without a GPU (host pointers are never dereferenced by a refused call)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = [p, p, p, p, p, p, p, p, 1, 1, 4, 4, 9, None]
    for change, word in (({0: None}, b"null"), ({2: None}, b"null"), ({5: None}, b"null"), ({6: None}, b"null"), ({7: None}, b"null"),
                         ({10: 0}, b"dimension"), ({8: -1}, b"dimension"), ({12: 17}, b"ncls"), ({12: 0}, b"ncls")):
        args = list(good)
        for i, v in change.items():
            args[i] = v
        status = lib.mau_eval_metrics(*args)
        msg = lib.mau_last_error()
        assert status == 1 and msg.startswith(b"eval_metrics") and word in msg, (change, status, msg)      # MAU_ERR_ARG


def test_eval_metrics_refuses_cpu_tensors():
    from mau_amd.evaluate import eval_metrics
    o, t, c = torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        eval_metrics(o, t, c)


# --------------------------------------------------------------------------- #
# rows and files
# --------------------------------------------------------------------------- #
def test_class_names_are_the_dynamic_world_labels():
    from mau_amd.evaluate import DW_CLASS_NAMES
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "dw_class_names.json")))
    assert list(DW_CLASS_NAMES) == names and len(names) == 9


def test_csv_writer_rows_columns_and_file_names(tmp_path):
    from mau_amd import evaluate as E
    nc = 9
    rows = np.full((2, 2, HEAD + 3 * nc), np.nan)
    for b in range(2):
        for c in range(2):
            r = rows[b, c]
            r[:4] = [0.5 + b, 0.75 + c, 2.0, 3.0]
            r[4:HEAD] = [0, 0, -1.0, 1.0, -2.0, 2.0, 0]
            r[HEAD:HEAD + nc] = 0
            for k in ((1, 6) if b == 0 else (8,)):
                r[HEAD + k], r[HEAD + nc + k], r[HEAD + 2 * nc + k] = 10 + k, 0.1 * (k + 1), 0.2 * (k + 1)
    m = E.EvalMetrics(torch.from_numpy(rows), nc)
    assert torch.equal(m.mae, m.rows[..., 0]) and m.class_count.shape == (2, 2, nc) and float(m.class_rmse[0, 0, 6]) == pytest.approx(1.4)
    infos = [{"is_known_city": True, "t1_year": 2019, "t1_month": 1, "t2_year": 2021, "t2_month": 2, "time_delta": 2,
              "city": "Some City", "lat": 48.8566, "lon": 2.3522},
             {"is_known_city": False, "t1_year": 2018, "t1_month": 7, "t2_year": 2022, "t2_month": 8, "time_delta": 4,
              "city": "Other", "lat": -3.5, "lon": 100.25}]
    out = E.metric_rows(m, 40, ["after_ndvi", "after_temp"], infos)
    assert [(r["sample_idx"], r["channel"], r["dw_class"]) for r in out] == [
        (40, "after_ndvi", "overall"), (40, "after_ndvi", "trees"), (40, "after_ndvi", "built"),
        (40, "after_temp", "overall"), (40, "after_temp", "trees"), (40, "after_temp", "built"),
        (41, "after_ndvi", "overall"), (41, "after_ndvi", "snow_and_ice"), (41, "after_temp", "overall"), (41, "after_temp", "snow_and_ice")]
    assert out[0]["mae"] == 0.5 and out[3]["rmse"] == 1.75 and out[0]["laplacian_var_pred"] == 2.0 and out[1]["laplacian_var_gt"] is None
    assert out[2]["mae"] == pytest.approx(0.7) and out[7]["rmse"] == pytest.approx(1.8) and out[7]["is_known_city"] is False
    report, info = E.write_reports(out, str(tmp_path / "reports"), "study", "unet++", "metaemb", 3, "J7")
    assert os.path.basename(report) == "study_unet++_metaemb_3_jobJ7_evaluation.csv"
    assert os.path.basename(info) == "study_unet++_metaemb_3_jobJ7_info.csv"
    assert E.report_paths("reports/tests", "test", "unet", "emb", "unknown", "") == \
        ("reports/tests/test_unet_emb_unknown_job_evaluation.csv", "reports/tests/test_unet_emb_unknown_job_info.csv")
    back = list(csv.reader(open(report)))
    assert back[0] == ["sample_idx", "channel", "dw_class", "mae", "rmse", "laplacian_var_pred", "laplacian_var_gt", "is_known_city",
                       "t1_year", "t1_month", "t2_year", "t2_month", "time_delta", "city", "lat", "lon"]
    assert len(back) == 1 + len(out)
    assert back[1] == ["40", "after_ndvi", "overall", "0.5", "0.75", "2.0", "3.0", "True", "2019", "1", "2021", "2", "2", "Some City", "48.8566", "2.3522"]
    assert back[2][2] == "trees" and back[2][5:7] == ["", ""] and float(back[2][3]) == pytest.approx(0.2)
    assert back[-1][:3] == ["41", "after_temp", "snow_and_ice"] and back[-1][7] == "False" and back[-1][13:] == ["Other", "-3.5", "100.25"]
    ib = list(csv.reader(open(info)))
    assert ib == [["evaluation_csv_path", "model_embedding_type", "study_name", "trial_id", "model_architecture"],
                  [report, "metaemb", "study", "3", "unet++"]]
    assert [E.tag_of(*f) for f in ((True, True), (True, False), (False, True), (False, False))] == ["emb", "tempemb", "metaemb", "noemb"]
    # the summary: one group per (is_known_city, t1_year, channel, dw_class, city, lat, lon), means of the four metrics
    twice = out + [dict(r, mae=r["mae"] + 1.0, sample_idx=r["sample_idx"] + 10) for r in out]
    s = E.summarize(twice)
    assert len(s) == len(out)
    g = [x for x in s if x["city"] == "Some City" and x["channel"] == "after_ndvi" and x["dw_class"] == "overall"][0]
    assert g["mae"] == 1.0 and g["rmse"] == 0.75 and g["laplacian_var_pred"] == 2.0 and g["is_known_city"] is True and g["t1_year"] == 2019
    g = [x for x in s if x["city"] == "Other" and x["channel"] == "after_temp" and x["dw_class"] == "snow_and_ice"][0]
    assert g["laplacian_var_pred"] is None and g["mae"] == pytest.approx(0.9 + 0.5)
    assert "Some City" in E.format_summary(s)


def test_known_cities_come_from_the_train_split_file_names(tmp_path):
    from mau_amd.evaluate import train_cities
    rng = np.random.default_rng(14)
    write_split(str(tmp_path / "train"), rng, [("Some City", 0, (2019, 1), (2021, 2), None, 6), ("Rio", 3, (2018, 5), (2020, 6), None, 6)], 4, 4)
    assert train_cities(str(tmp_path)) == {"Some City", "Rio"}
    assert train_cities(str(tmp_path / "nowhere")) == set()
