"""The training driver on a processed dataset (the folder layout, file naming and keys of the reference's
``process_and_save_subset``): ``GraphedTrainStep`` fed the packed ``Act`` batches of ``data.DeviceLoader``, a full ``train.run`` over
``train/`` and ``val/`` with a ragged last batch, ``validate()`` against separately computed means, and the refusal under a
process group.  Tiles are 23 x 48 x 40 with exact one-hot class planes; train/ holds 5, val/ 3; series of 24, 4 metadata features."""
import numpy as np
import pytest
import torch

from tests._helpers import mau  # noqa: F401

pytestmark = pytest.mark.gpu

H, W, N_TS = 48, 40, 24
CKPT_KEYS = {"epoch", "step", "model_state_dict", "optimizer_state_dict", "loss", "hyperparameters", "model_type", "study_name", "trial_id",
             "metadata_input_length"}
TERM_KEYS = {"total", "mse", "gradient", "pixel", "ssim"}


def write_tiles(folder, n, rng):
    folder.mkdir(parents=True)
    eye = np.eye(9, dtype=np.float32)
    for i in range(n):
        a, b = rng.integers(0, 9, (H, W)), rng.integers(0, 9, (H, W))
        x = np.vstack([eye[a].transpose(2, 0, 1), rng.standard_normal((5, H, W)).astype(np.float32), eye[b].transpose(2, 0, 1)])
        tgt = np.stack([np.tanh(rng.standard_normal((H, W))), rng.random((H, W))]).astype(np.float32)        # NDVI in (-1, 1), LST in [0, 1)
        np.savez_compressed(folder / f"City_{i}_41.8990_12.4690_2019_08_to_2021_08.npz", input=x.astype(np.float32), target=tgt,
                            metadata=rng.standard_normal(4).astype(np.float32), temperature_serie=rng.standard_normal(N_TS).astype(np.float32))


@pytest.fixture(scope="module")
def processed_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("processed")
    rng = np.random.default_rng(2024)
    write_tiles(root / "train", 5, rng)
    write_tiles(root / "val", 3, rng)
    return str(root)


@pytest.fixture()
def models_dir(tmp_path):
    from mau_amd.config import CONFIG
    old = CONFIG.MODELS_DIR
    CONFIG.MODELS_DIR = str(tmp_path)
    yield str(tmp_path)
    CONFIG.MODELS_DIR = old


def _small_net(mau, seed=31):
    torch.manual_seed(seed)
    return mau.UrbanPredictor("unet", 23, N_TS, 16, 8, 16, 24, 2, base_filters=16, temporal_embeddings=True,
                              metadata_embeddings=True).cuda().set_precision("bf16")


def _steps(mau, batches, graphed, fused_opt):
    net = _small_net(mau).train()
    opt = (mau.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3) if fused_opt
           else torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3, fused=True, capturable=True))
    crit = mau.compute_loss_mse_gradient
    step = mau.GraphedTrainStep(net, opt, crit, warmup=2) if graphed else None
    losses = []
    for x, md, ts, _len, t1, t2, tgt in batches:
        md = torch.cat([md, t1, t2], dim=1)
        if graphed and len(tgt) == 2:
            losses.append(step(x, ts, md, tgt).clone())
        elif graphed:                                               # the ragged batch: outside the graph, replay resumes afterwards
            assert step.matches(x, ts, md, tgt) == (step.graph is None)
            losses.append(step.eager_step(x, ts, md, tgt).clone())
        else:
            loss = crit(net(x, ts, md), tgt)["total"]
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach().clone())
    if graphed:
        assert step.graph is not None and step.calls == sum(1 for b in batches if len(b[6]) == 2)
        assert isinstance(step._in[0], mau.functional.Act) and step._in[0].C == 23 and not step._in[0].nchw
    net.eval()
    with torch.no_grad():
        ev = net(batches[0][0], batches[0][2], torch.cat([batches[0][1], batches[0][4], batches[0][5]], dim=1))
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, ev


@pytest.mark.parametrize("fused_opt", [False, True], ids=["torch-adamw", "pack-adamw"])
def test_graphed_train_step_takes_act_batches(mau, processed_dir, fused_opt):
    """Three passes over train/ in batches of 2, 2, 1 as the DeviceLoader packs them (``inputs`` is an ``Act``): warm-up, capture and
    replays on the full batches, the eager step on every ragged one -- bit-identical losses, parameters, buffers and a following eval
    output to the same nine steps launched one by one, for torch's optimizer and for the pack-writing one."""
    import mau_amd.functional  # noqa: F401
    loader = mau.data.create_dataloader("train", 2, shuffle=False, transform=mau.data.RandomFlip(3), processed_dir=processed_dir,
                                        device="cuda", dtype=torch.bfloat16)
    batches = [b for _ in range(3) for b in loader]
    assert [len(b[6]) for b in batches] == [2, 2, 1] * 3 and isinstance(batches[0][0], mau.functional.Act)
    torch.cuda.synchronize()
    a = _steps(mau, batches, False, fused_opt)
    b = _steps(mau, batches, True, fused_opt)
    for la, lb in zip(a[0], b[0]):
        assert torch.equal(la, lb), (a[0], b[0])
    assert float(a[0][0]) != float(a[0][-1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2])


def test_train_run_on_the_dataset(mau, processed_dir, models_dir):
    from mau_amd import train
    kw = dict(device="gpu", model_type="unet", temporal_embeddings=False, processed_dir=processed_dir, batch_size=2, epochs=2,
              precision="bf16")
    res = train.run(jobid="ds", **kw)
    assert res["step"] == 6                                         # two epochs of 2 + 2 + 1 tiles
    hist, terms = res["history"], res["val_terms"]
    assert len(hist) == 2 and all(len(h) == 2 and np.isfinite(h[0]) and np.isfinite(h[1]) for h in hist)
    assert len(terms) == 2 and all(set(d) == TERM_KEYS for d in terms)
    for e in range(2):                                              # the criterion is l1-gradient-ssim: both are terms[7]
        print("epoch", e, hist[e], terms[e])
        assert abs(terms[e]["total"] - hist[e][1]) <= 1e-6 * abs(hist[e][1])
        assert all(np.isfinite(v) for v in terms[e].values())
    assert res["best"] == min(h[1] for h in hist)
    path = res["checkpoint_path"]
    assert path is not None and path.endswith("urban-predictor-metaemb_trial_0_best_jobds.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == CKPT_KEYS and ck["model_type"] == "unet" and ck["metadata_input_length"] == 8 and ck["step"] in (3, 6)
    # graph and eager are bitwise equal, now across the ragged batch
    res2 = train.run(jobid="ds2", graph=False, **kw)
    assert res2["history"] == hist and res2["val_terms"] == terms and res2["step"] == 6


def test_validate_matches_separately_computed_means(mau, processed_dir):
    from mau_amd import losses as L, train
    net = _small_net(mau, seed=33).eval()
    loader = mau.data.create_dataloader("val", 2, shuffle=False, transform=None, processed_dir=processed_dir, device="cuda",
                                        dtype=torch.bfloat16)
    want = {k: 0.0 for k in ("mse", "gradient", "pixel", "ssim", "total", "mse_total", "mse_gradient_total")}
    n = 0
    with torch.no_grad():
        for x, md, ts, _len, t1, t2, tgt in loader:
            out = net(x, ts, torch.cat([md, t1, t2], dim=1))
            a, b = mau.compute_loss_mse_gradient(out, tgt), mau.compute_loss_l1_grad_ssim(out, tgt)
            s, _ = L.ssim_loss(out, tgt)
            vals = {"mse": a["mse"], "gradient": a["gradient"], "pixel": b["pixel"], "ssim": s, "total": b["total"],
                    "mse_total": mau.compute_loss_mse(out, tgt)["total"], "mse_gradient_total": a["total"]}
            for k, v in vals.items():
                want[k] += float(v) * len(tgt)
            n += len(tgt)
    assert n == 3
    want = {k: v / 3 for k, v in want.items()}

    def close(got, ref):
        return abs(got - ref) <= 1e-6 * abs(ref)

    other = lambda o, t: mau.compute_loss_l1_grad_ssim(o, t)         # a callable the driver does not know: called as it is
    for crit, key in ((mau.compute_loss_l1_grad_ssim, "total"), (mau.compute_loss_mse, "mse_total"),
                      (mau.compute_loss_mse_gradient, "mse_gradient_total"), (other, "total")):
        loss, terms = train.validate(net, loader, crit)
        print(key, loss, want[key], terms)
        assert net.training                                          # put back, as the reference does
        net.eval()
        assert close(loss, want[key]), (key, loss, want[key])
        assert set(terms) == TERM_KEYS
        for k in TERM_KEYS:
            assert close(terms[k], want[k]), (k, terms[k], want[k])
    # nothing counted: (inf, {})
    loss, terms = train.validate(net, [], mau.compute_loss_mse)
    assert loss == float("inf") and terms == {}


def test_processed_dir_is_refused_under_a_process_group(mau, processed_dir, monkeypatch):
    from mau_amd import train
    monkeypatch.setattr(train, "init_process_group_from_env", lambda: (0, 0, 2))
    with pytest.raises(NotImplementedError, match="more than one rank"):
        train.run(device="gpu", model_type="unet", temporal_embeddings=False, processed_dir=processed_dir, batch_size=2, epochs=1)
