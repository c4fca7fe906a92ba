"""``mau_amd.ground_truth`` on the device: ``mau_plane_moments`` against float64 numpy, the two-pass form on data with
|mean| >> std, bitwise repeatability and batch independence, ``BinStats`` against a float64 restatement of the reference's
``compute_bin_stats`` (and against its own float32 spelling), ``np.digitize``'s corner cases on the device, a NaN pixel, and the
pass over a processed directory with its command line.  Made-up normalisation numbers; tiles of 32 x 32."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._helpers import mau  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = {"temp_mean": 29.4173, "temp_std": 11.0291, "meta_mean": [17.25, 9.5, 1250000.5, 2.125],
           "meta_std": [21.75, 68.25, 4900000.25, 1.375]}
CHANNELS = ("after_ndvi", "after_temp")
TOL = 1e-10        # relative to the RMS of the plane / bin: n * 2^-53 ~ 7e-12 at n = 62 500, x 10 for the merges and the root


@pytest.fixture(scope="module")
def G(mau):
    return mau.ground_truth


# --------------------------------------------------------------------------- #
# the float64 restatement of the reference
# --------------------------------------------------------------------------- #
def compute_bin_stats(x_data, y_data, bin_centers):
    """generate_ground_truth_sensitivity.py:102-131 restated (y_data: (N, H, W) values of one channel); also the samples per bin."""
    edges = np.concatenate([[bin_centers[0] - (bin_centers[1] - bin_centers[0]) / 2], (bin_centers[:-1] + bin_centers[1:]) / 2,
                            [bin_centers[-1] + (bin_centers[-1] - bin_centers[-2]) / 2]])
    indices = np.digitize(x_data, edges)
    means, stds, counts = [], [], []
    for i in range(1, len(bin_centers) + 1):
        mask = indices == i
        counts.append(int(mask.sum()))
        if np.any(mask):
            vals = y_data[mask]
            means.append(float(np.mean(vals)))
            stds.append(float(np.std(vals)))
        else:
            means.append(float("nan"))
            stds.append(float("nan"))
    return means, stds, counts, edges


def coordinates(metadata):
    """:65-66: float32 column times np.float64 scalar plus np.float64 scalar -> float64."""
    meta_mean, meta_std = np.array(METRICS["meta_mean"]), np.array(METRICS["meta_std"])
    lats = metadata[:, 0] * meta_std[0] + meta_mean[0]
    lons = metadata[:, 1] * meta_std[1] + meta_mean[1]
    assert lats.dtype == np.float64 and lons.dtype == np.float64
    return lats, lons


def restatement(G, targets, metadata, dtype=np.float64):
    """The script's statistics of (targets, metadata): un-normalised PER PIXEL in `dtype`, np.mean / np.std per bin in `dtype`.
    {axis: {"mean": (C, 50), "std": (C, 50), "count": (50,), "rms": (C, 50)}}; asserts that no sample sits within 1e-6 of a bin
    width of an edge (there the last bit of a coordinate would decide the bin)."""
    lats, lons = coordinates(metadata)
    tn = targets.astype(dtype)
    un = np.zeros_like(tn)
    for i, ch in enumerate(CHANNELS):
        if "temp" in ch.lower():
            un[:, i] = tn[:, i] * METRICS["temp_std"] + METRICS["temp_mean"]
        else:
            un[:, i] = tn[:, i]
    assert un.dtype == dtype
    out = {}
    for name, x, centers in (("latitude", lats, G.LAT_RANGE), ("longitude", lons, G.LON_RANGE)):
        per = [compute_bin_stats(x, un[:, c], centers) for c in range(len(CHANNELS))]
        edges, width = per[0][3], centers[1] - centers[0]
        assert np.abs(x[:, None] - edges[None, :]).min() >= 1e-6 * width
        idx = np.digitize(x, edges)
        rms = np.array([[math.sqrt(float(np.mean(un[idx == i, c].astype(np.float64) ** 2))) if (idx == i).any() else np.nan
                         for i in range(1, 51)] for c in range(len(CHANNELS))])
        out[name] = {"mean": np.array([p[0] for p in per]), "std": np.array([p[1] for p in per]), "count": np.array(per[0][2]), "rms": rms}
    return out


def make_case(n, n_out, seed, hw=32):
    """n samples (2, hw, hw) whose latitude / longitude fall into a handful of bins, between 0.1 and 0.9 of the bin's width from
    its lower edge; the first n_out samples are outside both ranges.  Normalised float32 metadata, as the dataset holds it."""
    rng = np.random.default_rng(seed)
    from mau_amd import ground_truth as G
    coords = []
    for centers, outside in ((G.LAT_RANGE, (-75.0, 80.25, -64.0)), (G.LON_RANGE, (-190.0, 195.5, 188.5))):
        e = G.bin_edges(centers)
        bins = rng.choice(np.array([3, 4, 17, 30, 31, 49, 0]), n)
        x = e[bins] + rng.uniform(0.1, 0.9, n) * (e[bins + 1] - e[bins])
        x[:n_out] = outside[:n_out]
        coords.append(x)
    mean, std = np.array(METRICS["meta_mean"]), np.array(METRICS["meta_std"])
    meta = rng.standard_normal((n, 4))
    meta[:, 0] = (coords[0] - mean[0]) / std[0]
    meta[:, 1] = (coords[1] - mean[1]) / std[1]
    ndvi = np.tanh(rng.standard_normal((n, 1, hw, hw)) + rng.uniform(-0.5, 0.5, (n, 1, 1, 1)))
    temp = 0.8 * rng.standard_normal((n, 1, hw, hw)) + rng.uniform(-1.5, 1.5, (n, 1, 1, 1))
    return np.concatenate([ndvi, temp], axis=1).astype(np.float32), meta.astype(np.float32)


@pytest.fixture(scope="module")
def case24():
    return make_case(24, 3, 77)


@pytest.fixture(scope="module")
def truth24(G, case24):
    return restatement(G, *case24)


def new_stats(G):
    return G.BinStats([G.Axis("latitude", 0, G.LAT_RANGE, METRICS["meta_std"][0], METRICS["meta_mean"][0]),
                       G.Axis("longitude", 1, G.LON_RANGE, METRICS["meta_std"][1], METRICS["meta_mean"][1])], 2, "cuda")


def device_result(G, targets, metadata, splits=None):
    st = new_stats(G)
    t, m = torch.from_numpy(targets).cuda(), torch.from_numpy(metadata).cuda()
    at = 0
    for n in splits or [len(t)]:
        st.update(t[at:at + n], m[at:at + n])
        at += n
    assert at == len(t)
    return st, st.result(*G.channel_affine(CHANNELS, METRICS))


def assert_close(res, want, tol, what):
    worst = 0.0
    for axis in ("latitude", "longitude"):
        assert np.array_equal(res[axis]["count"], want[axis]["count"]), (axis, res[axis]["count"], want[axis]["count"])
        for k in ("mean", "std"):
            got, ref = res[axis][k], want[axis][k]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (axis, k)
            dev = np.nanmax(np.abs(got - ref) / want[axis]["rms"])
            worst = max(worst, float(dev))
    print(f"{what}: worst |difference| / bin RMS = {worst:.3g} (bound {tol:g})")
    assert worst <= tol, (what, worst)
    return worst


# --------------------------------------------------------------------------- #
# 1-3: plane moments
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", [(3, 2, 250, 250), (2, 2, 37, 41), (1, 2, 64, 64), (2, 1, 65, 127)],
                         ids=["250x250-vec4-partial", "37x41-odd-single-partial", "64x64-one-full-chunk", "65x127-c1-tail63"])
def test_plane_moments_against_float64_numpy(G, shape):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * rng.uniform(0.5, 2.0, shape[:2] + (1, 1)) + rng.uniform(-3, 3, shape[:2] + (1, 1))).astype(np.float32)
    rows = G.plane_moments(torch.from_numpy(x).cuda()).cpu().numpy()
    assert rows.shape == shape[:2] + (4,) and rows.dtype == np.float64
    hw = shape[2] * shape[3]
    worst = 0.0
    for b in range(shape[0]):
        for c in range(shape[1]):
            p = x[b, c].astype(np.float64)
            mean = p.mean()
            m2 = ((p - mean) ** 2).sum()
            rms = math.sqrt(float(np.mean(p ** 2)))
            n, gm, gm2, bad = rows[b, c]
            assert n == hw and bad == 0
            worst = max(worst, abs(gm - mean) / rms, abs(math.sqrt(gm2 / n) - math.sqrt(m2 / hw)) / rms)
    print(f"plane_moments {shape}: worst |difference| / plane RMS = {worst:.3g} (bound {TOL:g})")
    assert worst <= TOL


def test_plane_moments_on_offset_data(G):
    """300 + 0.01 N(0, 1): |mean| / std = 3e4.  Error of the two-pass + merge form, u = 2^-53: a chunk mean is a sum tree of depth
    16 + 6 + 3 = 25, off by <= 25 u |mean| = 8e-13; that error enters the chunk's M2 only in second order (n e^2 ~ 3e-21 against
    M2 ~ 0.4) and the differences x - mean, of size 0.01, are formed to u relative, so a chunk's M2 is good to ~25 u.  In the merge
    delta ~ std / sqrt(4096) = 1.6e-4 carries the two means' 1.6e-12, i.e. 1e-8 RELATIVE -- but delta^2 n_a n_b / n is only
    ~6e-5 of M2, which makes 1.2e-12 of M2 and half of that in the std: four orders below the bound of 1e-8.  The one-pass fp64
    form E[x^2] - E[x]^2 cancels 9e4 against 1e-4 and keeps ~1e-7 ... 1e-5 of the std (printed for this data, summed in index
    order as a kernel would)."""
    rng = np.random.default_rng(300)
    x = (300.0 + 0.01 * rng.standard_normal((1, 1, 250, 250))).astype(np.float32)
    n, mean, m2, bad = G.plane_moments(torch.from_numpy(x).cuda()).cpu().numpy()[0, 0]
    p = x.astype(np.float64).reshape(-1)
    tm = p.mean()
    tstd = math.sqrt(((p - tm) ** 2).sum() / p.size)
    got = math.sqrt(m2 / n)
    one_pass = math.sqrt(abs(float(np.cumsum(p * p)[-1]) / p.size - (float(np.cumsum(p)[-1]) / p.size) ** 2))
    print(f"offset data: std {got!r} truth {tstd!r} relative deviation {abs(got - tstd) / tstd:.3g} (bound 1e-08); "
          f"mean deviation {abs(mean - tm) / abs(tm):.3g}; one-pass fp64 form {abs(one_pass - tstd) / tstd:.3g}")
    assert n == p.size and bad == 0
    assert abs(got - tstd) <= 1e-8 * tstd
    assert abs(mean - tm) <= 1e-13 * abs(tm)


@pytest.mark.parametrize("hw", [(64, 100), (65, 127)], ids=["vec4", "scalar"])
def test_plane_moments_bits_repeat_and_do_not_depend_on_the_batch(G, hw):
    rng = np.random.default_rng(9)
    x = torch.from_numpy((rng.standard_normal((3, 2) + hw) + 5.0).astype(np.float32)).cuda()
    rows = G.plane_moments(x)
    assert torch.equal(rows, G.plane_moments(x))
    for i in range(3):                                               # a sample alone == the sample at place i of the batch
        assert torch.equal(G.plane_moments(x[i:i + 1])[0], rows[i]), i
    for perm in ([2, 0, 1], [1, 2, 0]):                              # ... and at every other place
        assert torch.equal(G.plane_moments(x[perm].contiguous()), rows[perm])
    many = x[:1].expand(70, -1, -1, -1).contiguous()                 # 140 planes: three launches of 64 tickets
    got = G.plane_moments(many)
    assert torch.equal(got, rows[:1].expand(70, -1, -1).contiguous())


# --------------------------------------------------------------------------- #
# 3-7: the table
# --------------------------------------------------------------------------- #
def test_bin_stats_tables_do_not_depend_on_the_batching(G, case24):
    t, m = case24[0][3:11], case24[1][3:11]                          # 8 samples in range, several per bin
    tables = [device_result(G, t, m, splits)[0].table for splits in ([5, 3], [8], [1] * 8)]
    assert float(tables[0][..., 0].sum()) == 2 * 2 * 8 * 32 * 32     # every sample counted once per axis and channel
    assert (tables[0][..., 0].amax() > 32 * 32)                      # a bin with more than one sample: the merge ran
    assert torch.equal(tables[0], tables[1]) and torch.equal(tables[0], tables[2])


def test_bin_stats_against_the_float64_restatement(G, case24, truth24):
    st, res = device_result(G, *case24, splits=[10, 14])
    assert int(truth24["latitude"]["count"].sum()) == 21 == int(truth24["longitude"]["count"].sum())      # three samples dropped
    assert int((truth24["latitude"]["count"] == 0).sum()) >= 43                                        # most bins are empty
    assert_close(res, truth24, TOL, "BinStats vs float64 restatement")
    assert all(int(res[a]["nonfinite"].sum()) == 0 for a in res)
    # the host twin holds the same moments
    lats, lons = coordinates(case24[1])
    scale, shift = G.channel_affine(CHANNELS, METRICS)
    for axis, x, centers in (("latitude", lats, G.LAT_RANGE), ("longitude", lons, G.LON_RANGE)):
        for c in range(2):
            means, stds, counts = G.bin_stats_host(x, case24[0][:, c].astype(np.float64) * scale[c] + shift[c], centers)
            assert np.array_equal(counts, res[axis]["count"])
            assert np.allclose(means, res[axis]["mean"][c], rtol=1e-12, atol=1e-12, equal_nan=True)
            assert np.allclose(stds, res[axis]["std"][c], rtol=1e-10, atol=1e-12, equal_nan=True)


def _edge_case(G, nan_pixel):
    st = G.BinStats([G.Axis("k", 2, [0.0, 1.0, 2.0, 3.0], 1.0, 0.0)], 2, "cuda")      # edges -0.5 ... 3.5: exact
    meta = np.zeros((5, 4), dtype=np.float32)
    meta[:, 2] = [-0.5, 0.5, 3.5, -0.6, np.nan]
    t = np.zeros((5, 2, 8, 12), dtype=np.float32)
    t += np.arange(1, 6, dtype=np.float32)[:, None, None, None] + np.array([0.0, 100.0], dtype=np.float32)[None, :, None, None]
    t[:, :, 0, 0] += 1.0                                             # not constant: a std to compare
    if nan_pixel:
        t[1, 0, 3, 5] = np.nan
    st.update(torch.from_numpy(t).cuda(), torch.from_numpy(meta).cuda())
    return st.result(), t


def test_digitize_corner_cases_on_the_device(G):
    res, t = _edge_case(G, False)
    r = res["k"]
    assert r["count"].tolist() == [1, 1, 0, 0]                       # first edge: bin 0; on an edge: the upper bin; last edge, below, NaN: dropped
    for c in range(2):
        for b in range(2):
            p = t[b, c].astype(np.float64)
            assert abs(r["mean"][c, b] - p.mean()) <= 1e-13 * abs(p.mean()) and abs(r["std"][c, b] - p.std()) <= 1e-12
        assert np.isnan(r["mean"][c, 2:]).all() and np.isnan(r["std"][c, 2:]).all()
    assert int(r["nonfinite"].sum()) == 0


def test_a_nan_pixel_stays_in_its_bin(G):
    clean, _ = _edge_case(G, False)
    res, _ = _edge_case(G, True)
    r, c0 = res["k"], clean["k"]
    assert math.isnan(r["mean"][0, 1]) and math.isnan(r["std"][0, 1]) and r["nonfinite"][0, 1] == 1
    assert r["nonfinite"].sum() == 1 and r["count"].tolist() == [1, 1, 0, 0]
    for c, b in ((0, 0), (1, 0), (1, 1)):                            # the other entries: the bits of the clean run
        assert r["mean"][c, b] == c0["mean"][c, b] and r["std"][c, b] == c0["std"][c, b]


def test_the_references_float32_spelling_agrees(G, case24):
    """A semantic check, not a precision check: the script's own arithmetic (float32 un-normalisation per pixel, float32 np.mean /
    np.std, pairwise summation over <= 2.5e4 values ~ 1e-6) within 1e-4 of the bin's RMS."""
    want32 = restatement(G, *case24, dtype=np.float32)
    _, res = device_result(G, *case24)
    assert_close(res, want32, 1e-4, "BinStats vs the script's float32 arithmetic")


# --------------------------------------------------------------------------- #
# 8: a processed directory, and the command line
# --------------------------------------------------------------------------- #
def test_ground_truth_sensitivity_end_to_end(G, tmp_path):
    targets, meta = make_case(8, 1, 5)
    rng = np.random.default_rng(8)
    root = tmp_path / "processed"
    (root / "test").mkdir(parents=True)
    eye = np.eye(9, dtype=np.float32)
    for i in range(8):                                               # sorted file names = sample order
        a, b = rng.integers(0, 9, (32, 32)), rng.integers(0, 9, (32, 32))
        x = np.vstack([eye[a].transpose(2, 0, 1), rng.standard_normal((5, 32, 32)).astype(np.float32), eye[b].transpose(2, 0, 1)])
        np.savez_compressed(root / "test" / f"City_{i}_41.8990_12.4690_2019_08_to_2021_08.npz", input=x.astype(np.float32), target=targets[i],
                            metadata=meta[i], temperature_serie=rng.standard_normal(12).astype(np.float32))
    with open(root / "normalization_metrics.json", "w") as f:
        json.dump(METRICS, f)
    want = restatement(G, targets, meta)
    data = G.ground_truth_sensitivity(str(root), split="test", batch_size=3)
    assert set(data) == {"model_name", "model_type", "sweeps", "heatmaps"} and data["model_type"] == "dataset" and data["heatmaps"] == {}

    def as_result(d):
        return {axis: {k: np.array([d["sweeps"][axis]["channels"][ch][k] for ch in CHANNELS]) for k in ("mean", "std")}
                | {"count": want[axis]["count"]} for axis in ("latitude", "longitude")}

    assert_close(as_result(data), want, TOL, "ground_truth_sensitivity vs float64 restatement")
    stats = G.ground_truth_stats(str(root), "test", 8)
    assert np.array_equal(stats["latitude"]["count"], want["latitude"]["count"]) and int(stats["longitude"]["count"].sum()) == 7
    assert data["sweeps"]["latitude"]["x"] == G.LAT_RANGE.tolist() and data["sweeps"]["longitude"]["x"] == G.LON_RANGE.tolist()
    with pytest.raises(FileNotFoundError):
        G.ground_truth_sensitivity(str(root / "test"))

    # the same through the command line, in a fresh process
    out_dir = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.ground_truth", "--processed-dir", str(root), "--output-dir", out_dir, "--batch-size", "5"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    path = os.path.join(out_dir, "sensitivity_data_ground_truth.json")
    assert f"Saved Ground Truth sensitivity data to: {path}" in p.stdout
    back = json.load(open(path))
    assert set(back) == {"model_name", "model_type", "sweeps", "heatmaps"} and back["model_name"] == "Ground Truth (Dataset)"
    assert back["model_type"] == "dataset" and back["heatmaps"] == {} and set(back["sweeps"]) == {"latitude", "longitude"}
    for axis in ("latitude", "longitude"):
        sw = back["sweeps"][axis]
        assert set(sw) == {"x", "channels"} and len(sw["x"]) == 50 and list(sw["channels"]) == list(CHANNELS)
        for ch in CHANNELS:
            assert set(sw["channels"][ch]) == {"mean", "std"}
            for k in ("mean", "std"):                                # batches of 5 + 3 instead of 3 + 3 + 2: the same bits
                assert np.array_equal(sw["channels"][ch][k], data["sweeps"][axis]["channels"][ch][k], equal_nan=True)
