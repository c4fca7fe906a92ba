"""CPU-only check of ``scenario.load_tile``, the one reader of the command lines of ``scenario``, ``placement`` and ``region``: a small
``.npz`` in the loose shapes the files come in (a leading axis on ``dw``, flattened planes), with and without the optional keys."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_scenario_host import METRICS, ROOT, make_tile

H, W = 6, 5
RAW = np.array([48.8566, 2.3522, 2148000.0, 2019, 3, 2022, 9], dtype=np.float64)


def write_metrics(path, metrics):
    with open(path, "w") as f:
        json.dump(metrics, f)
    return str(path)


def test_load_tile(tmp_path):
    from mau_amd import scenario as S
    from mau_amd._tile import METRIC_KEYS
    assert sorted(METRICS) == sorted(METRIC_KEYS) and S.METRIC_KEYS is METRIC_KEYS
    rng = np.random.default_rng(90)
    dw, rgb, ndvi, temp = make_tile(rng, H, W)
    mj = write_metrics(tmp_path / "metrics.json", METRICS)
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, dw=dw[None], rgb=rgb, ndvi=ndvi.reshape(-1), temp=temp.reshape(-1), metadata_raw=RAW, canvas=np.zeros((4, 4, 4), dtype=np.uint8))
    t = S.load_tile(bare, mj, device="cpu")
    want = {"dw": ((H, W), torch.uint8, dw), "rgb": ((3, H, W), torch.float32, rgb), "ndvi": ((H, W), torch.float32, ndvi),
            "temp": ((H, W), torch.float32, temp)}
    for name, (shape, dtype, value) in want.items():
        got = getattr(t, name)
        assert tuple(got.shape) == shape and got.dtype == dtype and got.device.type == "cpu" and got.is_contiguous(), name
        assert np.array_equal(got.numpy(), value), name
    assert t._fields[:7] == ("model", "dw", "rgb", "ndvi", "temp", "metadata", "temp_series") and t.model is None     # the sessions' positional order
    row = S.metadata_row(*[float(v) for v in RAW], METRICS["meta_mean"], METRICS["meta_std"])
    assert tuple(t.metadata.shape) == (1, 8) and t.metadata.dtype == torch.float32
    assert np.array_equal(t.metadata.numpy().view(np.uint32), row.view(np.uint32))
    assert tuple(t.temp_series.shape) == (1, 60) and t.temp_series.dtype == torch.float32 and int(t.temp_series.count_nonzero()) == 0
    assert t.dw_t2 is None and t.temp_orig is None and t.palette is None and t.metrics == METRICS
    assert t.npz["canvas"].shape == (4, 4, 4)                                          # a tool's own keys stay readable
    # the optional keys, and a palette
    series = rng.standard_normal(12)
    dw2, temp_orig = ((dw + 1) % 9).astype(np.uint8), (temp + 1.5).astype(np.float32)
    full = str(tmp_path / "full.npz")
    np.savez(full, dw=dw, rgb=rgb.reshape(-1), ndvi=ndvi[None], temp=temp, metadata_raw=RAW, temp_series=series, dw_t2=dw2.reshape(-1),
             temp_orig=temp_orig[None])
    t = S.load_tile(full, mj, os.path.join(ROOT, "tests", "golden", "dw_palette.json"), "cpu")
    assert np.array_equal(t.rgb.numpy(), rgb) and np.array_equal(t.ndvi.numpy(), ndvi) and tuple(t.dw.shape) == (H, W)
    assert tuple(t.temp_series.shape) == (1, 12) and t.temp_series.dtype == torch.float32
    assert np.array_equal(t.temp_series.numpy().view(np.uint32), S.normalize_temp_series(series, METRICS).view(np.uint32))
    assert tuple(t.dw_t2.shape) == (H, W) and t.dw_t2.dtype == torch.uint8 and np.array_equal(t.dw_t2.numpy(), dw2)
    assert tuple(t.temp_orig.shape) == (H, W) and t.temp_orig.dtype == torch.float32 and np.array_equal(t.temp_orig.numpy(), temp_orig)
    assert t.palette.shape == (9, 3) and t.palette.dtype == np.uint8
    # every key of METRIC_KEYS is required, and the error names the one that is missing
    lacking = write_metrics(tmp_path / "lacking.json", {k: v for k, v in METRICS.items() if k != "temp_std"})
    with pytest.raises(ValueError, match="temp_std"):
        S.load_tile(bare, lacking, device="cpu")
