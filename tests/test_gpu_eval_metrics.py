"""GPU tests of ``mau_amd.evaluate``: ``mau_eval_metrics`` against the float64 numpy truth of tests/test_eval_metrics_host.py,
its bins, flags, determinism and batch independence, the refusals of ``eval_metrics``, and ``evaluate_checkpoint`` / the
command line on a small test split.

Tolerance of every kernel-against-truth comparison: relative 1e-10 on every finite entry.  Both sides hold fp64 sums of at
most 62 500 terms; two summation orders of n terms differ by at most about n * 2^-53 = 7e-12 of the sum of magnitudes, and
1e-10 leaves a factor of ten for the square root and for the subtraction E[x^2] - E[x]^2 of the variance entries, which are
therefore bounded relative to E[x^2].  Counts are exact; an absent class is NaN on both sides."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import mau  # noqa: F401
from tests.test_eval_metrics_host import HEAD, assert_rows_match, eval_truth, write_split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, SHIFT = [1.0, 7.3], [0.0, 21.5]


def coeffs(C):
    """The issue's per-channel coefficients; a single-channel case takes the un-normalised (second) channel's."""
    return SCALE[-C:], SHIFT[-C:]


def make_case(B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((B, C, H, W)).astype(np.float32)
    tgt = rng.standard_normal((B, C, H, W)).astype(np.float32)
    cls = rng.integers(0, 9, (B, H, W)).astype(np.uint8)
    if B >= 2:
        cls[0] = 3                                               # one sample of a single class
        cls[1] = rng.choice([0, 8], (H, W))                      # one sample of classes {0, 8} only
    return out, tgt, cls


def run_kernel(mau, out, tgt, cls, scale, shift, ncls=9):
    m = mau.evaluate.eval_metrics(torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(cls).cuda(),
                                  scale, shift, ncls)
    return m


def big_b(mau):
    """(70, 2, 8, 8) has more rows than one ticket buffer covers; on a library with a larger buffer, the smallest B that does."""
    per = mau._lib.lib.mau_reduce_tickets_elems()
    return 70 if per < 140 else per // 2 + 1


# ---- 1. the kernel against the truth -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 2, 31, 17), (2, 2, 250, 250), (2, 1, 5, 300), ("many", 2, 8, 8)])
def test_kernel_matches_float64_truth(mau, shape):
    B, C, H, W = shape
    if B == "many":
        B = big_b(mau)
        assert B * C > mau._lib.lib.mau_reduce_tickets_elems()                       # several launches
    if (H, W) == (250, 250):
        assert mau.evaluate.chunks_per_map(H, W) > 1                                 # several row chunks per map
    out, tgt, cls = make_case(B, C, H, W, seed=100 + H)
    scale, shift = coeffs(C)
    m = run_kernel(mau, out, tgt, cls, scale, shift)
    assert m.rows.shape == (B, C, HEAD + 27) and m.rows.dtype == torch.float64 and m.rows.is_cuda
    want, e2 = eval_truth(out, tgt, cls, scale, shift, 9, with_lap_mean_squares=True)
    worst = assert_rows_match(m.rows.cpu().numpy(), want, e2, 9)
    print(f"eval_metrics {B}x{C}x{H}x{W}: worst |difference| / (1e-10 * scale) = {worst:.3g}")
    # the named views
    assert torch.equal(m.mae, m.rows[..., 0]) and torch.equal(m.rmse, m.rows[..., 1])
    assert torch.equal(m.laplacian_var_pred, m.rows[..., 2]) and torch.equal(m.laplacian_var_gt, m.rows[..., 3])
    assert m.class_count.shape == m.class_mae.shape == m.class_rmse.shape == (B, C, 9)
    assert np.array_equal(m.class_count.sum(-1).cpu().numpy(), np.full((B, C), H * W))
    if B >= 2:
        cc = m.class_count.cpu().numpy()
        assert cc[0, 0, 3] == H * W and np.isnan(m.class_mae.cpu().numpy()[0, :, [0, 1, 2, 4, 5, 6, 7, 8]]).all()
        assert cc[1, 0, 0] + cc[1, 0, 8] == H * W and not cc[1, 0, 1:8].any()
    if H * W > 1:
        assert float(m.nonfinite_pred.sum()) == 0 and bool((m.min_pred < m.max_pred).all())


# ---- 2. class ids >= ncls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [4, 12])
def test_ids_beyond_ncls_go_to_the_extra_bin(mau, ncls):
    out, tgt, cls = make_case(3, 2, 31, 17, seed=7)
    m = run_kernel(mau, out, tgt, cls, SCALE, SHIFT, ncls)
    want, e2 = eval_truth(out, tgt, cls, SCALE, SHIFT, ncls, with_lap_mean_squares=True)
    assert m.rows.shape == (3, 2, HEAD + 3 * ncls)
    assert_rows_match(m.rows.cpu().numpy(), want, e2, ncls)
    other = m.other_count.cpu().numpy()
    assert np.array_equal(other[:, 0], [(cls[b] >= ncls).sum() for b in range(3)]) and np.array_equal(other[:, 0], other[:, 1])
    if ncls == 4:
        assert other[1, 0] > 0 and other[2, 0] > 0
    else:
        assert not other.any()
    # the overall numbers still cover every pixel: they are those of the 9-class evaluation
    full = run_kernel(mau, out, tgt, cls, SCALE, SHIFT, 9)
    assert torch.equal(m.rows[..., :10], full.rows[..., :10])
    assert np.array_equal((m.class_count.sum(-1) + m.other_count).cpu().numpy(), np.full((3, 2), 31 * 17))


# ---- 3. non-finite values, constant maps ---------------------------------------------------------------------
def test_nonfinite_values_and_constant_maps(mau):
    out, tgt, cls = make_case(3, 2, 31, 17, seed=8)
    out[1, 0, 5, 6] = np.nan
    tgt[2, 0] = 0.25                                             # a constant target map (0.25: its Laplacian is exactly 0)
    m = run_kernel(mau, out, tgt, cls, SCALE, SHIFT)
    want, e2 = eval_truth(out, tgt, cls, SCALE, SHIFT, 9, with_lap_mean_squares=True)
    assert_rows_match(m.rows.cpu().numpy(), want, e2, 9)
    r = m.rows.cpu().numpy()
    nf = m.nonfinite_pred.cpu().numpy()
    assert nf[1, 0] == 1 and nf.sum() == 1 and not m.nonfinite_gt.cpu().numpy().any()
    assert np.isnan(r[1, 0, :3]).all() and np.isfinite(r[1, 0, 3])                   # MAE, RMSE, lap var pred; the target's is finite
    others = np.ones((3, 2), dtype=bool)
    others[1, 0] = False
    assert np.isfinite(r[others][:, :10]).all()
    k = cls[1, 5, 6]
    assert np.isnan(r[1, 0, HEAD + 9 + k]) and np.isfinite(r[1, 0, HEAD + 9 + (0 if k == 8 else 8)])
    assert np.isfinite(r[1, 0, 6]) and r[1, 0, 6] < r[1, 0, 7]                       # min / max skip the NaN
    assert r[2, 0, 8] == r[2, 0, 9] == 0.25 and r[2, 0, 3] == 0.0                    # constant: min == max, no Laplacian
    assert r[2, 1, 8] < r[2, 1, 9] and r[2, 0, 6] < r[2, 0, 7]


# ---- 4. determinism, independence of the batch ---------------------------------------------------------------
@pytest.mark.parametrize("hw", [(250, 250), (31, 17)])
def test_bitwise_repeatable_and_independent_of_the_batch(mau, hw):
    H, W = hw
    out, tgt, cls = make_case(5, 2, H, W, seed=9)
    o, t, c = torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(cls).cuda()
    E = mau.evaluate.eval_metrics
    a, b = E(o, t, c, SCALE, SHIFT).rows, E(o, t, c, SCALE, SHIFT).rows
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # the sample at position 4, alone, and at position 0 of another batch of 5
    alone = E(o[4:5], t[4:5], c[4:5], SCALE, SHIFT).rows
    perm = [4, 0, 1, 2, 3]
    first = E(o[perm].contiguous(), t[perm].contiguous(), c[perm].contiguous(), SCALE, SHIFT).rows
    assert torch.equal(alone[0].view(torch.int64), a[4].view(torch.int64))
    assert torch.equal(first[0].view(torch.int64), a[4].view(torch.int64))
    assert torch.equal(first[1:].view(torch.int64), a[:4].view(torch.int64))


# ---- 5. refusals ---------------------------------------------------------------------------------------------
def test_eval_metrics_error_paths(mau):
    E = mau.evaluate.eval_metrics
    o, t = torch.zeros(2, 2, 6, 5, device="cuda"), torch.zeros(2, 2, 6, 5, device="cuda")
    c = torch.zeros(2, 6, 5, dtype=torch.uint8, device="cuda")
    E(o, t, c)
    with pytest.raises(RuntimeError, match="no CPU"):
        E(o.cpu(), t, c)
    with pytest.raises(RuntimeError, match="no CPU"):
        E(o, t, c.cpu())
    with pytest.raises(TypeError):
        E(o, t.to(torch.uint8), c)
    with pytest.raises(TypeError):
        E(o, t, c.long())
    with pytest.raises(ValueError):
        E(o, t[:, :1], c)
    with pytest.raises(ValueError):
        E(o, t, c[:, :5])
    with pytest.raises(ValueError):
        E(o, t, c, scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        E(o, t, c, num_classes=17)


# ---- 6. the driver -------------------------------------------------------------------------------------------
TRAIN_TILES = [("Alpha Town", 0, (2018, 3), (2020, 4), None, 12), ("Beta", 1, (2019, 1), (2021, 2), None, 9)]
TEST_TILES = [("Alpha Town", 5, (2019, 1), (2021, 2), None, 12), ("Beta", 2, (2018, 6), (2022, 7), [6], 9),
              ("Gamma Ville", 0, (2017, 11), (2020, 12), [0, 8], 12), ("Gamma Ville", 1, (2019, 5), (2020, 5), None, 7),
              ("Beta", 7, (2020, 2), (2023, 9), [1, 2, 4], 12)]
METRICS = {"meta_mean": [20.0, 10.0, 3.0, 1.0], "meta_std": [15.0, 60.0, 2.0, 0.5], "temp_mean": 14.5, "temp_std": 8.25}


def make_split_and_checkpoint(mau, tmp_path, model_type, n_meta):
    import json
    from mau_amd import checkpoint as C
    rng = np.random.default_rng(21)
    data = str(tmp_path / "processed")
    write_split(os.path.join(data, "train"), rng, TRAIN_TILES)
    names = write_split(os.path.join(data, "test"), rng, TEST_TILES)
    json.dump(METRICS, open(os.path.join(data, "normalization_metrics.json"), "w"))
    torch.manual_seed(22)
    flags = dict(temporal_embeddings=model_type == "unet++", metadata_embeddings=True)
    net = mau.UrbanPredictor(model_type, 23, 12, 8, n_meta, 8, 12, 2, base_filters=8, **flags)
    for mod in net.modules():                                    # running statistics that are not the initial 0 / 1
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    hyper = {"temporal_dim": 8, "meta_dim": 8, "lstm_hidden": 12, "batch_size": 3, **flags}
    path = str(tmp_path / "m.pth")
    C.save_checkpoint(path, net, None, epoch=1, step=2, loss=0.5, hyperparameters=hyper, model_type=model_type,
                      study_name="urban-predictor", trial_id=3, metadata_input_length=n_meta)
    return data, names, path


def check_driver_rows(mau, res, data, names, path, n_meta, batch_size):
    """Every row of ``evaluate_checkpoint`` against ``eval_truth`` of the model's own output, sample by sample."""
    from mau_amd.data import create_dataloader, to_network_inputs
    E = mau.evaluate
    model, _ = E.load_for_evaluation(path)
    model.set_precision("fp32").eval().freeze_inference()
    scale, shift = [1.0, METRICS["temp_std"]], [0.0, METRICS["temp_mean"]]
    channels = ["after_ndvi", "after_temp"]
    rows = res["rows"]
    at, idx, worst = 0, 0, 0.0
    for host in create_dataloader("test", batch_size, False, processed_dir=data, device=None):
        dev = host.to("cuda")
        inputs, md, ts, _l, t1, t2, targets = to_network_inputs(dev, torch.float32)
        if n_meta == 8:
            md = torch.cat([md, t1, t2], dim=1)
        with torch.no_grad():
            out = model(inputs, ts, md)
        want, e2 = eval_truth(out.cpu().numpy(), targets.cpu().numpy(), host.cls_a.numpy(), scale, shift, 9, with_lap_mean_squares=True)
        for i in range(out.shape[0]):
            city, _n, _lat, _lon, y1, m1, _to, y2, m2 = names[idx][:-4].split("_")
            for c, ch in enumerate(channels):
                present = [k for k in range(9) if want[i, c, HEAD + k] > 0]
                got = np.full(HEAD + 27, np.nan)
                got[4:HEAD] = want[i, c, 4:HEAD]                                     # not part of a CSV row
                got[HEAD:HEAD + 9] = 0
                r = rows[at]
                assert (r["sample_idx"], r["channel"], r["dw_class"]) == (idx, ch, "overall")
                got[:4] = [r["mae"], r["rmse"], r["laplacian_var_pred"], r["laplacian_var_gt"]]
                for j, k in enumerate(present):
                    rk = rows[at + 1 + j]
                    assert (rk["sample_idx"], rk["channel"], rk["dw_class"]) == (idx, ch, E.DW_CLASS_NAMES[k])
                    assert rk["laplacian_var_pred"] is None and rk["laplacian_var_gt"] is None
                    got[HEAD + k], got[HEAD + 9 + k], got[HEAD + 18 + k] = want[i, c, HEAD + k], rk["mae"], rk["rmse"]
                for rr in rows[at:at + 1 + len(present)]:
                    assert rr["is_known_city"] is (city in ("Alpha Town", "Beta")) and rr["city"] == city
                    assert (rr["t1_year"], rr["t1_month"], rr["t2_year"], rr["t2_month"]) == (int(y1), int(m1), int(y2), int(m2))
                    assert rr["time_delta"] == int(y2) - int(y1) and rr["lat"] == 48.8566 and rr["lon"] == 2.3522
                worst = max(worst, assert_rows_match(got[None, None], want[i:i + 1, c:c + 1], e2[i:i + 1, c:c + 1], 9))
                at += 1 + len(present)
            idx += 1
    assert at == len(rows) and idx == len(names) == 5
    return worst


def test_evaluate_checkpoint_unet_end_to_end_and_cli(mau, tmp_path):
    data, names, path = make_split_and_checkpoint(mau, tmp_path, "unet", 8)
    out_dir = str(tmp_path / "reports")
    res = mau.evaluate.evaluate_checkpoint(path, data, batch_size=2, precision="fp32", study_name="st", jobid="11", output_dir=out_dir)
    assert os.path.basename(res["report_path"]) == "st_unet_metaemb_3_job11_evaluation.csv"
    assert os.path.basename(res["info_path"]) == "st_unet_metaemb_3_job11_info.csv"
    worst = check_driver_rows(mau, res, data, names, path, 8, 2)
    print(f"evaluate_checkpoint unet: worst |difference| / (1e-10 * scale) = {worst:.3g}")
    rows = res["rows"]
    assert [r["sample_idx"] for r in rows if r["dw_class"] == "overall"] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # sorted file names: Alpha Town_5, Beta_2 (class 6 only), Beta_7 (1, 2, 4), Gamma Ville_0 (0, 8), Gamma Ville_1
    per_sample = {i: [r["dw_class"] for r in rows if r["sample_idx"] == i and r["channel"] == "after_temp"] for i in range(5)}
    assert per_sample[1] == ["overall", "built"] and per_sample[2] == ["overall", "trees", "grass", "crops"]
    assert per_sample[3] == ["overall", "water", "snow_and_ice"] and len(per_sample[0]) == 10
    assert [r["is_known_city"] for r in rows if r["dw_class"] == "overall" and r["channel"] == "after_ndvi"] == [True, True, True, False, False]
    back = list(csv.DictReader(open(res["report_path"])))
    assert len(back) == len(rows) and list(back[0]) == list(mau.evaluate.COLUMNS)
    assert float(back[0]["mae"]) == rows[0]["mae"] and back[1]["laplacian_var_pred"] == ""
    assert {g["is_known_city"] for g in res["summary"]} == {True, False}
    # the same through the command line, in a fresh process
    cli_dir = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.evaluate", path, "--processed-dir", data, "--device", "gpu", "--study-name", "st",
                        "--jobid", "12", "--precision", "fp32", "--batch-size", "2", "--output-dir", cli_dir],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Known Cities" in p.stdout and "Unknown Cities" in p.stdout
    report = os.path.join(cli_dir, "st_unet_metaemb_3_job12_evaluation.csv")
    info = os.path.join(cli_dir, "st_unet_metaemb_3_job12_info.csv")
    cli_rows = list(csv.DictReader(open(report)))
    assert len(cli_rows) == len(rows)
    assert [(r["sample_idx"], r["channel"], r["dw_class"], r["mae"], r["rmse"]) for r in cli_rows] == \
        [(r["sample_idx"], r["channel"], r["dw_class"], r["mae"], r["rmse"]) for r in back]
    ib = list(csv.DictReader(open(info)))
    assert len(ib) == 1 and ib[0]["evaluation_csv_path"] == report and ib[0]["model_architecture"] == "unet" and ib[0]["trial_id"] == "3"


def test_evaluate_checkpoint_unetpp(mau, tmp_path):
    """U-Net++ once, 4 metadata features (no dates appended), the checkpoint's own batch size (3: batches of 3 and 2)."""
    data, names, path = make_split_and_checkpoint(mau, tmp_path, "unet++", 4)
    res = mau.evaluate.evaluate_checkpoint(path, data, precision="fp32", output_dir=str(tmp_path / "reports"))
    assert os.path.basename(res["report_path"]) == "test_unet++_emb_3_job_evaluation.csv"
    worst = check_driver_rows(mau, res, data, names, path, 4, 3)
    print(f"evaluate_checkpoint unet++: worst |difference| / (1e-10 * scale) = {worst:.3g}")
