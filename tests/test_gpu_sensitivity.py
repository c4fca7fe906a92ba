"""GPU tests of ``mau_amd.sensitivity``: the U-Net++ metadata sweep (encoder column once at batch 1), the head-mean kernel
(``mau_head_mean``: 1x1 head + per-sample fp64 spatial mean in one launch), ``sweep_outputs`` / ``sweep_means`` for both model
types, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import unet_ref as R
from tests._helpers import mau, rel_err, rel_l2  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_net(mau, model_type, prec, seed=5, base_filters=8, **kw):
    torch.manual_seed(seed)
    return mau.UrbanPredictor(model_type, 23, 12, 16, 8, 16, 24, 2, base_filters=base_filters, **kw).cuda().set_precision(prec).eval()


def small_inputs(B=7, size=62, seed=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 23, size, size, generator=g).cuda(), torch.randn(1, 12, generator=g).cuda(), torch.randn(B, 8, generator=g).cuda()


def mean_bound(maps: torch.Tensor, scale=None) -> torch.Tensor:
    """|difference of two fp64 means of the same HW values, summed in different orders| <= HW * 2^-52 * mean|y| per entry:
    each order's rounding error is at most (HW - 1) * 2^-53 * sum|y| (the standard bound of recursive summation in any
    order); times |scale| when the mean is scaled."""
    HW = maps.shape[2] * maps.shape[3]
    b = HW * 2.0 ** -52 * maps.double().abs().mean((2, 3))
    return b if scale is None else b * torch.as_tensor(scale, dtype=torch.float64, device=b.device).abs()


# ---- 1. U-Net++ sweep == its own repeated-tile forward ------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_unetpp_sweep_equals_repeated_tile_forward(mau, prec):
    """sweep_outputs (x^{0..4,0} once at batch 1, the decoder nodes at batch B) == the reference's way (tile repeated B
    times), eval mode, bit for bit: per-sample results do not depend on the batch size."""
    net = small_net(mau, "unet++", prec)
    x, ts, md = small_inputs()
    with torch.no_grad():
        ref = net(x.expand(7, -1, -1, -1).contiguous(), ts.expand(7, -1).contiguous(), md)
    got = mau.sensitivity.sweep_outputs(net, x, ts, md)
    assert got.shape == ref.shape == (7, 2, 62, 62) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    assert torch.equal(mau.sensitivity.sweep_outputs(net, x, ts.expand(7, -1).contiguous(), md, chunk=3), ref)      # (B,T) series, chunks


def test_unetpp_sweep_through_row_buffers(mau):
    """base_filters=64 in bf16: the forward keeps the nodes of a row side by side in row buffers (virtual concat); the sweep
    broadcasts the encoder activations into slot 0 of the same buffers."""
    net = small_net(mau, "unet++", "bf16", seed=7, base_filters=64)
    x, ts, md = small_inputs(B=3, size=32, seed=8)
    with torch.no_grad():
        ref = net(x.expand(3, -1, -1, -1).contiguous(), ts.expand(3, -1).contiguous(), md)
    assert torch.equal(mau.sensitivity.sweep_outputs(net, x, ts, md), ref)


def test_unet_sweep_outputs_is_forward_metadata_sweep(mau):
    net = small_net(mau, "unet", "bf16", temporal_embeddings=False)
    x, ts, md = small_inputs()
    ref = net.forward_metadata_sweep(x, ts, md)
    assert torch.equal(mau.sensitivity.sweep_outputs(net, x, ts, md), ref)
    assert torch.equal(mau.sensitivity.sweep_outputs(net, x, ts, md, chunk=2), ref)


# ---- 2. U-Net++ sweep against the oracle at the production tile -----------------------------------------------
def test_unetpp_sweep_vs_oracle_250(mau):
    """250x250x23, 8 metadata features, B = 5, base_filters=16; running statistics warmed by one oracle training forward;
    against the ORACLE's repeated-tile eval forward.  fp32 rel_err <= 1e-3, bf16 rel_l2 <= 3e-2 (the bounds of
    test_metadata_sweep_vs_oracle_250)."""
    torch.manual_seed(60)
    net = mau.UrbanPredictor("unet++", 23, 12, 32, 8, 32, 24, 2, base_filters=16)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        R.forward("unet++", sd, torch.randn(4, 23, 62, 62, generator=g), torch.randn(4, 12, generator=g), torch.randn(4, 8, generator=g), True)
    B = 5
    x, ts, md = torch.randn(1, 23, 250, 250, generator=g), torch.randn(1, 12, generator=g), torch.randn(B, 8, generator=g)
    with torch.no_grad():
        ref = R.forward("unet++", sd, x.expand(B, -1, -1, -1), ts.expand(B, -1), md, False)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    for prec, metric, tol in (("fp32", rel_err, 1e-3), ("bf16", rel_l2, 3e-2)):
        net.set_precision(prec)
        got = mau.sensitivity.sweep_outputs(net, x.cuda(), ts.cuda(), md.cuda())
        assert got.shape == (B, 2, 250, 250)
        e = metric(got.cpu(), ref)
        print(f"unet++ sweep vs oracle 250 {prec}: {metric.__name__} {e:.2e}")
        assert e <= tol, (prec, e)


# ---- 3. mau_head_mean through ctypes against mau_head_fwd -----------------------------------------------------
@pytest.mark.parametrize("C", [64, 8])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_head_mean_kernel_vs_head_fwd(mau, dt, C):
    """means == mean over HW of the map mau_head_fwd writes.  The per-pixel values are the same bits (one shared device
    function), so only the order of the fp64 sum differs: |difference| <= HW * 2^-52 * mean|y| per entry (mean_bound)."""
    from mau_amd import functional as F_
    from mau_amd._lib import call, lib
    dev = torch.device("cuda")
    code, ld = F_.dtype_code(dt), F_.pad8(C)
    g = torch.Generator().manual_seed(100 + C)
    scale = torch.tensor([1.0, 8.25], dtype=torch.float64, device=dev)
    shift = torch.tensor([0.0, 14.5], dtype=torch.float64, device=dev)
    worst = 0.0
    for Co, tanh0 in ((2, 1), (1, 0)):
        w = (torch.randn(Co, C, generator=g) / C ** 0.5).cuda()
        b = torch.randn(Co, generator=g).cuda()
        for N in (1, 5):
            for H, W in ((62, 62), (250, 250), (33, 35)):
                a = torch.zeros(N, H, W, ld, dtype=dt, device=dev)
                a[..., :C] = torch.randn(N, H, W, C, generator=g).to(dt).cuda()
                out = torch.empty(N, Co, H, W, dtype=torch.float32, device=dev)
                call("mau_head_fwd", a.data_ptr(), ld, w.data_ptr(), b.data_ptr(), out.data_ptr(), tanh0, code, N, H * W, C, Co, F_._stream())
                ref = out.double().mean((2, 3))
                tickets = F_._tickets(dev)
                for sc, sh in ((None, None), (scale[:Co].contiguous(), shift[:Co].contiguous())):
                    means = torch.full((N, Co), float("nan"), dtype=torch.float64, device=dev)
                    ws = torch.empty(lib.mau_head_mean_ws_elems(N, H * W, Co), dtype=torch.float64, device=dev)
                    call("mau_head_mean", a.data_ptr(), ld, w.data_ptr(), b.data_ptr(), None if sc is None else sc.data_ptr(),
                         None if sh is None else sh.data_ptr(), means.data_ptr(), ws.data_ptr(), tickets.data_ptr(), tanh0, code,
                         N, H * W, C, Co, F_._stream())
                    want = ref if sc is None else ref * sc + sh
                    bound = mean_bound(out, sc)
                    diff = (means - want).abs()
                    worst = max(worst, float((diff / bound).max()))
                    assert bool((diff <= bound).all()), (Co, N, H, W, sc is not None, float((diff / bound).max()))
                    assert int(tickets.abs().sum()) == 0                    # the tickets are left zeroed
    print(f"head_mean C={C} {dt}: worst |difference| / bound = {worst:.3g}")


def test_head_mean_wide_head_and_many_samples(mau):
    """A head wider than 64 channels (weights from memory; mau_head_fwd's general kernel) and more samples than one launch has
    tickets for."""
    from mau_amd import functional as F_
    from mau_amd._lib import call, lib
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(9)
    for C, N, H, W in ((72, 3, 40, 33), (16, lib.mau_reduce_tickets_elems() + 6, 9, 7)):
        a = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16).cuda()
        w, b = (torch.randn(2, C, generator=g) / C ** 0.5).cuda(), torch.randn(2, generator=g).cuda()
        out = torch.empty(N, 2, H, W, dtype=torch.float32, device=dev)
        call("mau_head_fwd", a.data_ptr(), C, w.data_ptr(), b.data_ptr(), out.data_ptr(), 1, F_.MAU_BF16, N, H * W, C, 2, F_._stream())
        conv = mau.sensitivity.head_mean(a, C, w.view(2, C, 1, 1), b)
        assert bool(((conv - out.double().mean((2, 3))).abs() <= mean_bound(out)).all()), (C, N)


# ---- 4. determinism and independence ---------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["unet", "unet++"])
def test_sweep_means_bitwise_repeatable_and_independent_of_batch_and_chunk(mau, model_type):
    net = small_net(mau, model_type, "bf16")
    x, ts, md = small_inputs()
    S = mau.sensitivity
    sc, sh = [1.0, 8.25], [0.0, 14.5]
    m1 = S.sweep_means(net, x, ts, md, sc, sh)
    assert m1.shape == (7, 2) and m1.dtype == torch.float64 and m1.is_cuda
    assert torch.equal(m1, S.sweep_means(net, x, ts, md, sc, sh))                      # repeated call
    assert torch.equal(m1, S.sweep_means(net, x, ts, md, sc, sh, chunk=50))
    assert torch.equal(m1, S.sweep_means(net, x, ts, md, sc, sh, chunk=3))             # chunks of 3, 3, 1
    for n in range(7):
        assert torch.equal(m1[n:n + 1], S.sweep_means(net, x, ts, md[n:n + 1], sc, sh)), n      # row n alone, B = 1


# ---- 5. sweep_means against sweep_outputs -------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["unet", "unet++"])
def test_sweep_means_vs_sweep_outputs(mau, model_type):
    net = small_net(mau, model_type, "bf16")
    x, ts, md = small_inputs()
    maps = mau.sensitivity.sweep_outputs(net, x, ts, md)
    ref = maps.double().mean((2, 3))
    got = mau.sensitivity.sweep_means(net, x, ts, md)
    assert bool(((got - ref).abs() <= mean_bound(maps)).all()), float(((got - ref).abs() / mean_bound(maps)).max())
    sc = torch.tensor([1.0, 8.25], dtype=torch.float64)
    sh = torch.tensor([0.0, 14.5], dtype=torch.float64)
    got = mau.sensitivity.sweep_means(net, x, ts, md, scale=sc, shift=sh)
    assert bool(((got - (ref * sc.cuda() + sh.cuda())).abs() <= mean_bound(maps, sc.cuda())).all())


# ---- 6. error paths --------------------------------------------------------------------------------------
def test_sweep_error_paths(mau):
    S = mau.sensitivity
    x, ts, md = small_inputs()
    for model_type in ("unet", "unet++"):
        net = small_net(mau, model_type, "bf16")
        with pytest.raises(ValueError):
            S.sweep_outputs(net, x.expand(2, -1, -1, -1).contiguous(), ts, md)          # two tiles
        with pytest.raises(ValueError):
            S.sweep_means(net, x.expand(2, -1, -1, -1).contiguous(), ts, md)
        with pytest.raises(ValueError):
            S.sweep_means(net, x, ts, md, scale=[1.0, 2.0, 3.0])
        net.train()
        with pytest.raises(RuntimeError):
            S.sweep_outputs(net, x, ts, md)
        with pytest.raises(RuntimeError):
            S.sweep_means(net, x, ts, md)
    deep = small_net(mau, "unet++", "bf16", deep_supervision=True)
    with pytest.raises(ValueError):
        S.sweep_outputs(deep, x, ts, md)
    with pytest.raises(ValueError):
        S.sweep_means(deep, x, ts, md)
    with pytest.raises(NotImplementedError):                                            # the dispatcher's U-Net-only entry stays as it is
        small_net(mau, "unet++", "bf16").forward_metadata_sweep(x, ts, md)


# ---- 7. command line round trip ----------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["unet", "unet++"])
def test_cli_round_trip(mau, model_type, tmp_path):
    from mau_amd.checkpoint import save_checkpoint
    S = mau.sensitivity
    torch.manual_seed(21)
    flags = dict(temporal_embeddings=False, metadata_embeddings=True) if model_type == "unet" else {}
    net = mau.UrbanPredictor(model_type, 23, 12, 16, 8, 8, 32, 2, base_filters=8, **flags)
    hyper = {"temporal_dim": 16, "meta_dim": 8, "lstm_hidden": 32, "model_type": model_type,
             "temporal_embeddings": flags.get("temporal_embeddings", True), "metadata_embeddings": True}
    ckpt = str(tmp_path / "best.pth")
    save_checkpoint(ckpt, net, None, epoch=1, step=1, loss=0.5, hyperparameters=hyper, model_type=model_type, study_name="t",
                    trial_id=0, metadata_input_length=8)
    metrics = {"meta_mean": [20.0, 10.0, 3.0, 1.0], "meta_std": [15.0, 60.0, 2.0, 0.5], "temp_mean": 14.5, "temp_std": 8.25}
    mj = str(tmp_path / "normalization_metrics.json")
    json.dump(metrics, open(mj, "w"))
    out_dir = str(tmp_path / "out")
    env = dict(os.environ, MAU_QUIET="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mau_amd.sensitivity", "--checkpoint", ckpt, "--samples", "2", "--output-dir", out_dir,
                        "--precision", "bf16", "--heatmaps", "1", "--metrics-json", mj, "--tile", "32", "--seq-len", "12", "--seed", "33"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    name = ("metaemb" if model_type == "unet" else "emb") + ("++" if model_type == "unet++" else "")
    path = os.path.join(out_dir, f"sensitivity_data_{name}.json")
    assert os.path.exists(path), os.listdir(out_dir)
    d = json.load(open(path))
    assert d["model_name"] == name and d["model_type"] == model_type
    for key, x in (("latitude", np.linspace(-60, 70, 50)), ("longitude", np.linspace(-180, 180, 50))):
        assert d["sweeps"][key]["x"] == x.tolist()
        for ch in ("after_ndvi", "after_temp"):
            c = d["sweeps"][key]["channels"][ch]
            assert len(c["mean"]) == 50 and len(c["std"]) == 50 and np.isfinite(c["mean"]).all() and np.isfinite(c["std"]).all()
    assert list(d["heatmaps"]) == ["0"] and np.array(d["heatmaps"]["0"]["channels"]["after_temp"]["values"]).shape == (20, 20)
    # the same run driven by hand: same checkpoint, same seeds, same normalisation
    model = net.cuda().set_precision("bf16").eval()
    rep = S.SensitivityReport(name, model_type)
    gen = torch.Generator().manual_seed(33)
    for i in range(2):
        inputs, metadata, series, _len, t1, t2, _tgt = S.synthetic_tile(gen, 23, 32, 12, 8, 2, "cuda")
        rep.run_sample(model, inputs, series, metadata, t1, t2, metrics["meta_mean"], metrics["meta_std"], 8,
                       scale=[1.0, 8.25], shift=[0.0, 14.5], heatmap=i < 1, idx=i)
    assert json.loads(json.dumps(rep.export())) == d
