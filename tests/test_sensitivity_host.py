"""CPU-only checks of ``mau_amd.sensitivity``: the metadata rows of a sweep against a numpy restatement of the reference's
formulas (test/metadata_sensitivity.py:294-304, :383-406), the exported dictionary of ``SensitivityReport`` (:627-683),
and the C ABI of the head-mean kernel (header, binding, ABI version)."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

META_MEAN = np.array([23.5, -12.25, 4.0, 0.5])
META_STD = np.array([17.0, 61.5, 2.5, 0.25])


def sample(n_meta, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, n_meta - 4 if n_meta >= 8 else n_meta, generator=g), torch.randn(1, 2, generator=g),
            torch.randn(1, 2, generator=g))


def reference_rows(md, t1, t2, cols_vals, n_meta):
    """numpy restatement: repeat the sample's row, overwrite the swept columns with (value - mean) / std cast to the
    metadata's dtype, append the date pairs for 8 features."""
    n = len(cols_vals[0][1])
    rows = np.repeat(md.numpy(), n, axis=0)
    for c, v in cols_vals:
        rows[:, c] = ((v - META_MEAN[c]) / META_STD[c]).astype(rows.dtype)
    if n_meta == 8:
        rows = np.concatenate([rows, np.repeat(t1.numpy(), n, axis=0), np.repeat(t2.numpy(), n, axis=0)], axis=1)
    return rows


@pytest.mark.parametrize("n_meta", [4, 8])
def test_metadata_rows_follow_the_reference_formulas(n_meta):
    from mau_amd.sensitivity import metadata_rows
    md, t1, t2 = sample(n_meta)
    before = md.clone()
    lats, lons = np.linspace(-60, 70, 50), np.linspace(-180, 180, 50)
    for col, vals in ((0, lats), (1, lons)):
        rows = metadata_rows(md, t1, t2, col, vals, META_MEAN, META_STD, n_meta)
        assert rows.shape == (50, n_meta) and rows.dtype == md.dtype
        assert np.array_equal(rows.numpy(), reference_rows(md, t1, t2, [(col, vals)], n_meta))
        untouched = [c for c in range(4) if c != col]
        assert torch.equal(rows[:, untouched], md[:, untouched].expand(50, -1))
        if n_meta == 8:
            assert torch.equal(rows[:, 4:6], t1.expand(50, -1)) and torch.equal(rows[:, 6:8], t2.expand(50, -1))
    # the 2-D grid: meshgrid(..., indexing='ij') flattened -- latitude-major
    lats2, lons2 = np.linspace(-60, 70, 20), np.linspace(-180, 180, 20)
    la, lo = np.meshgrid(lats2, lons2, indexing="ij")
    rows = metadata_rows(md, t1, t2, (0, 1), (lats2, lons2), META_MEAN, META_STD, n_meta)
    assert rows.shape == (400, n_meta)
    assert np.array_equal(rows.numpy(), reference_rows(md, t1, t2, [(0, la.flatten()), (1, lo.flatten())], n_meta))
    assert torch.equal(rows[:, 2:4], md[:, 2:4].expand(400, -1))
    assert float(rows[1, 0]) == float(rows[0, 0]) and float(rows[1, 1]) != float(rows[0, 1])       # longitude runs fastest
    assert torch.equal(md, before)                                                                  # the sample's row is not written to
    with pytest.raises(ValueError):
        metadata_rows(md, t1, t2, 2, lats, META_MEAN, META_STD, n_meta)


def test_report_export_layout_and_statistics(tmp_path):
    from mau_amd.sensitivity import SensitivityReport, model_name_of
    assert [model_name_of(*f) for f in ((True, True, "unet"), (False, True, "unet"), (True, False, "unet++"), (False, False, "unet++"))] \
        == ["emb", "metaemb", "tempemb++", "noemb++"]
    rep = SensitivityReport("emb++", "unet++")
    assert np.array_equal(rep.lat_range, np.linspace(-60, 70, 50)) and np.array_equal(rep.lon_range, np.linspace(-180, 180, 50))
    assert np.array_equal(rep.heat_lats, np.linspace(-60, 70, 20)) and np.array_equal(rep.heat_lons, np.linspace(-180, 180, 20))
    rng = np.random.default_rng(3)
    lat = [rng.standard_normal((50, 2)) for _ in range(3)]
    lon = [rng.standard_normal((50, 2)) for _ in range(3)]
    for a, b in zip(lat, lon):
        rep.add_curves(torch.from_numpy(a), b)                    # tensors and arrays are both accepted
    # heatmap of sample 1: value = 1000 * latitude index + longitude index (+ 0.5 on channel 1), rows latitude-major
    ii, jj = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    grid = np.stack([(1000 * ii + jj).flatten(), (1000 * ii + jj).flatten() + 0.5], axis=1).astype(np.float64)
    rep.add_heatmap(1, grid, orig_lat=12.5, orig_lon=-3.0)
    d = rep.export()
    assert set(d) == {"model_name", "model_type", "sweeps", "heatmaps"}
    assert d["model_name"] == "emb++" and d["model_type"] == "unet++"
    assert set(d["sweeps"]) == {"latitude", "longitude"}
    for key, curves, x in (("latitude", lat, rep.lat_range), ("longitude", lon, rep.lon_range)):
        s = d["sweeps"][key]
        assert set(s) == {"x", "channels"} and s["x"] == x.tolist()
        assert list(s["channels"]) == ["after_ndvi", "after_temp"]
        stack = np.stack(curves)
        for c, ch in enumerate(("after_ndvi", "after_temp")):
            assert set(s["channels"][ch]) == {"mean", "std"}
            assert np.array_equal(np.array(s["channels"][ch]["mean"]), np.mean(stack[:, :, c], axis=0))
            assert np.array_equal(np.array(s["channels"][ch]["std"]), np.std(stack[:, :, c], axis=0))
    assert list(d["heatmaps"]) == ["1"]
    h = d["heatmaps"]["1"]
    assert h["orig_lat"] == 12.5 and h["orig_lon"] == -3.0 and set(h["channels"]) == {"after_ndvi", "after_temp"}
    for c, ch in enumerate(("after_ndvi", "after_temp")):
        e = h["channels"][ch]
        assert set(e) == {"values", "lats", "lons"}
        assert e["lats"] == sorted(e["lats"]) == rep.heat_lats.tolist() and e["lons"] == sorted(e["lons"]) == rep.heat_lons.tolist()
        v = np.array(e["values"])
        assert v.shape == (20, 20)
        assert v[3][7] == 3007 + 0.5 * c and v[19][0] == 19000 + 0.5 * c            # values[lat][lon]
    # save(): the reference's file name, and the file round-trips through json
    path = rep.save(str(tmp_path / "out"))
    assert os.path.basename(path) == "sensitivity_data_emb++.json"
    assert json.load(open(path)) == d
    with pytest.raises(ValueError):
        rep.add_curves(lat[0][:10], lon[0])
    with pytest.raises(RuntimeError):
        SensitivityReport("emb", "unet").export()


def test_descending_heatmap_axes_are_exported_ascending():
    from mau_amd.sensitivity import SensitivityReport
    rep = SensitivityReport("emb", "unet", channels=["c"], heat_lats=[30.0, 10.0, 20.0], heat_lons=[5.0, -5.0])
    vals = np.array([[300 + 5], [300 - 5], [100 + 5], [100 - 5], [200 + 5], [200 - 5]], dtype=np.float64)      # 10 * lat + lon
    rep.add_heatmap("a", vals)
    e = rep.heatmaps["a"]["channels"]["c"]
    assert e["lats"] == [10.0, 20.0, 30.0] and e["lons"] == [-5.0, 5.0]
    assert e["values"] == [[95.0, 105.0], [195.0, 205.0], [295.0, 305.0]]


def test_head_mean_is_part_of_the_c_abi():
    import mau_amd
    from mau_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mau_hip.h")).read()
    for sym in ("mau_head_mean", "mau_head_mean_ws_elems"):
        assert f"{sym}(" in hdr and sym in _lib.PROTOTYPES and hasattr(_lib.lib, sym)
    assert len(_lib.PROTOTYPES["mau_head_mean"][1]) == 16
    assert _lib.lib.mau_abi_version() == 5 and "#define MAU_ABI_VERSION 5" in hdr
    # workspace: one fp64 partial per (sample, workgroup of the sample, output channel); the number of workgroups of a
    # sample depends on HW alone
    ws = _lib.lib.mau_head_mean_ws_elems
    assert ws(1, 250 * 250, 2) > 0 and ws(5, 250 * 250, 2) == 5 * ws(1, 250 * 250, 2) and ws(1, 250 * 250, 1) * 2 == ws(1, 250 * 250, 2)
    assert ws(0, 100, 2) == 0
    assert mau_amd.sensitivity.sweep_means is not None and "sensitivity" in mau_amd.__all__
    # a refused call reports through mau_last_error, without a GPU
    assert _lib.lib.mau_head_mean(None, 8, None, None, None, None, None, None, None, 1, 0, 1, 64, 8, 2, None) != 0
    assert b"head_mean" in _lib.lib.mau_last_error()
