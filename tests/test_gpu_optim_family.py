"""GPU tests of the optimizer family: ``mau_amd.SGD`` / ``mau_amd.Adam`` (csrc/optim.hip: the update of every convolution weight + both
weight packs in one launch, the rule a template parameter), the one-launch gradient norm (``mau_grad_norm_clip``) and gradient clipping
inside the fused update (``max_grad_norm``).  The yardstick is torch's own optimizer / ``clip_grad_norm_`` on the same device, fed
gradients from the same kernels; tolerances are those of ``test_gpu_model.py::test_fused_adamw_matches_torch_and_keeps_the_packs_fresh``."""
import ctypes
import math

import pytest
import torch

from tests._helpers import mau, rel_l2  # noqa: F401

pytestmark = pytest.mark.gpu

FLAGS = dict(temporal_embeddings=False, metadata_embeddings=True)


def _net(mau, prec, seed=100):
    torch.manual_seed(seed)
    return mau.UrbanPredictor("unet", 23, 10, 16, 8, 16, 24, 2, base_filters=16, **FLAGS).cuda().set_precision(prec).train()


def _batches(n, seed=101):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 23, 62, 50, generator=g).cuda(), torch.randn(2, 10, generator=g).cuda(), torch.randn(2, 8, generator=g).cuda(),
             torch.randn(2, 2, 62, 50, generator=g).cuda()) for _ in range(n)]


def _pair(mau, name, kw):
    """(torch optimizer class, mau class, keyword arguments of both)"""
    return (torch.optim.SGD, mau.SGD, kw) if name == "SGD" else (torch.optim.Adam, mau.Adam, kw)


CONFIGS = [("SGD", dict(lr=0.02, momentum=0.9)), ("SGD", dict(lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-2)),
           ("SGD", dict(lr=0.02, momentum=0.0)), ("Adam", dict(lr=2e-3, weight_decay=0.0)), ("Adam", dict(lr=2e-3, weight_decay=1e-2))]


def _step_one_close(net_t, net_m):
    for (k, p), (_, q) in zip(net_t.named_parameters(), net_m.named_parameters()):
        assert float((p - q).abs().max()) <= 1e-6 + 1e-5 * float(p.abs().max()), k


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("name,kw", CONFIGS, ids=["sgd-mom", "sgd-nesterov-wd", "sgd-plain", "adam", "adam-wd"])
def test_fused_sgd_and_adam_match_torch_and_keep_the_packs_fresh(mau, prec, name, kw):
    """Four steps on identical models: first loss bitwise equal, every parameter within 1e-6 + 1e-5 max|p| after the first step,
    later losses within 2e-3 (fp32) / 1e-2 (bf16) relative; after every step the packs the kernel wrote are a fresh re-pack (eval
    forward bitwise equal before and after mark_params_updated()).  SGD has no m / sqrt(v) amplification: in fp32 all parameters
    are also compared after the four steps, relative L2 1e-3 (the bound of test_packs_follow_the_optimizer_and_sgd_tracks_the_oracle).
    (Measured: 0.0 -- with torch's roundings the kernel's SGD is torch.optim.SGD bit for bit; with the momentum product contracted
    into an FMA the one-ulp difference grew to 9e-3 / 7e-2 on BatchNorm biases within the four steps, EXPERIMENTS.md.)"""
    tcls, mcls, kw = _pair(mau, name, kw)
    nets = [_net(mau, prec), _net(mau, prec)]
    opts = [tcls(nets[0].parameters(), **kw), mcls(nets[1].parameters(), **kw)]
    for step, (x, ts, md, tgt) in enumerate(_batches(4)):
        losses = []
        for net, opt in zip(nets, opts):
            loss = mau.compute_loss_mse(net(x, ts, md), tgt)["total"]
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(float(loss.detach()))
        net = nets[1].eval()
        with torch.no_grad():
            a = net(x, ts, md)
            mau.mark_params_updated()
            b = net(x, ts, md)
        net.train()
        assert torch.equal(a, b), step
        print(f"{name} {kw} {prec} step {step}: losses {losses}")
        assert losses[0] == losses[1] if step == 0 else abs(losses[0] - losses[1]) <= (2e-3 if prec == "fp32" else 1e-2) * abs(losses[0]), (step, losses)
        if step == 0:
            _step_one_close(nets[0], nets[1])
        pairs = list(zip(nets[0].named_parameters(), nets[1].named_parameters()))
        print(f"    parameters not bitwise equal to torch's after step {step}: {sum(not torch.equal(p, q) for (_, p), (_, q) in pairs)} of {len(pairs)}")
    assert all(math.isfinite(v) for v in losses)
    if name == "SGD" and prec == "fp32":
        errs = {k: rel_l2(q.detach().cpu(), p.detach().cpu()) for (k, p), (_, q) in pairs}
        worst = max(errs, key=errs.get)
        print(f"    SGD fp32, four steps: worst relative L2 {errs[worst]:.3e} ({worst})")
        for k, e in errs.items():
            assert e < 1e-3, (k, e)
    w = nets[1].model.conv2_0.conv1.weight
    assert w.grad is None and w._mau_grad_slot is not None


@pytest.mark.parametrize("name,kw", [("SGD", dict(lr=0.02, momentum=0.9)), ("Adam", dict(lr=2e-3, weight_decay=1e-2))], ids=["sgd", "adam"])
def test_state_dict_interchange_with_torch(mau, name, kw):
    """An optimizer_state_dict written by the torch class loads into the fused class and the other way round (also a torch state whose
    ``step`` lives on the host), and training goes on from it exactly as it does in the optimizer that wrote it."""
    tcls, mcls, kw = _pair(mau, name, kw)
    nets = [_net(mau, "fp32"), _net(mau, "fp32")]
    opts = [tcls(nets[0].parameters(), **kw), mcls(nets[1].parameters(), **kw)]
    batches = _batches(3)
    for x, ts, md, tgt in batches[:2]:
        for net, opt in zip(nets, opts):
            mau.compute_loss_mse(net(x, ts, md), tgt)["total"].backward()
            opt.step()
            opt.zero_grad()
    sd_t, sd_m = opts[0].state_dict(), opts[1].state_dict()
    assert sd_t["state"].keys() == sd_m["state"].keys()
    k0 = next(iter(sd_m["state"]))
    want = {"momentum_buffer"} if name == "SGD" else {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd_m["state"][k0].keys()) == want == set(sd_t["state"][k0].keys())
    assert {k for k in sd_m["param_groups"][0]} <= {k for k in sd_t["param_groups"][0]}
    if name == "Adam":
        assert float(sd_m["state"][k0]["step"]) == 2.0
        assert not sd_t["state"][k0]["step"].is_cuda         # torch's default Adam counts on the host: the fused class moves it
    # cross-load: the fused class continues from torch's state on torch's weights, torch from the fused state on the fused weights
    fresh_m = mcls(nets[0].parameters(), **kw)
    fresh_m.load_state_dict(sd_t)
    fresh_t = tcls(nets[1].parameters(), **kw)
    fresh_t.load_state_dict(sd_m)
    before = [{k: p.detach().clone() for k, p in net.named_parameters()} for net in nets]
    x, ts, md, tgt = batches[2]
    for net, opt in zip(nets, (fresh_m, fresh_t)):
        mau.compute_loss_mse(net(x, ts, md), tgt)["total"].backward()
        opt.step()
        opt.zero_grad()
    # both pairs took their third step from (nearly) the same state with the same rule: weights and moments stay together (the bounds
    # of the four-step comparisons: 1e-3 for SGD, 1e-2 for Adam's weights) -- moments restarted from zero would be far away
    tol = 1e-3 if name == "SGD" else 1e-2
    moved = 0.0
    for (k, p), (_, q) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert torch.isfinite(q).all() and torch.isfinite(p).all(), k
        if k.endswith("weight") and p.dim() == 4:
            assert rel_l2(q.detach().cpu(), p.detach().cpu()) < tol, k
            moved = max(moved, float((p - before[0][k]).abs().max()))
    assert moved > 0
    mom = "momentum_buffer" if name == "SGD" else "exp_avg"
    after_m, after_t = fresh_m.state_dict()["state"], fresh_t.state_dict()["state"]
    assert after_m.keys() == after_t.keys()
    for i, p in enumerate(nets[0].parameters()):
        if i in after_m and p.dim() == 4:
            assert rel_l2(after_m[i][mom].cpu(), after_t[i][mom].cpu()) < 1e-2, i
    if name == "Adam":
        assert float(fresh_m.state_dict()["state"][k0]["step"]) == 3.0 and float(fresh_t.state_dict()["state"][k0]["step"]) == 3.0
        assert fresh_m.state[next(iter(fresh_m.state))]["step"].is_cuda


def _norm_launch(segments, max_norm):
    from mau_amd import _lib
    lib = _lib.lib
    dev = segments[0].device
    host = ctypes.create_string_buffer(lib.mau_grad_norm_seg_bytes() * len(segments))
    nxt = ctypes.c_int(0)
    for i, s in enumerate(segments):
        _lib.call("mau_grad_norm_seg_fill", ctypes.addressof(host), i, s.data_ptr(), s.numel(), nxt.value, ctypes.addressof(nxt))
    table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
    ws = torch.full((nxt.value,), float("nan"), dtype=torch.float64, device=dev)
    tickets = torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    _lib.call("mau_grad_norm_clip", table.data_ptr(), len(segments), nxt.value, ws.data_ptr(), tickets.data_ptr(), max_norm, out.data_ptr(),
              out.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.clone(), tickets


def test_grad_norm_kernel(mau):
    """Segments of awkward lengths and alignments, values over a wide dynamic range: the norm equals the fp64 norm of the concatenation to
    one ulp of the fp32 result; two launches give the same bits; the tickets are left zeroed; a max_norm above the norm gives a
    coefficient of exactly 1, one below it max_norm / (norm + 1e-6); an Inf gradient gives a non-finite norm."""
    g = torch.Generator().manual_seed(7)
    base = torch.randn(3_300_000 + 5000, generator=g) * torch.exp(8 * torch.randn(3_300_000 + 5000, generator=g))     # ~ 1e-14 .. 1e14
    base = base.cuda()
    # lengths 1, 7, 4097 and a multi-million "arena", at element offsets 0, 1, 10, 4111 of one buffer: every 16-byte misalignment
    segs = [base[0:1], base[1:8], base[10:10 + 4097], base[4111:4111 + 3_300_001]]
    assert {s.data_ptr() % 16 for s in segs} == {0, 4, 8, 12}
    ref64 = torch.linalg.vector_norm(torch.cat([s.double() for s in segs]))
    ref32 = ref64.float()
    ulp = float(torch.nextafter(ref32, ref32 * 2) - ref32)
    out1, tk1 = _norm_launch(segs, 1e30)
    out2, tk2 = _norm_launch(segs, 1e30)
    print(f"norm kernel {float(out1[0])!r}  fp64 reference {float(ref64)!r}  ulp {ulp!r}")
    assert abs(float(out1[0]) - float(ref64)) <= ulp, (float(out1[0]), float(ref64), ulp)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    assert int(tk1.abs().sum()) == 0 and int(tk2.abs().sum()) == 0
    assert float(out1[1]) == 1.0                                                    # max_norm above the norm: no clipping, exactly
    small = [s * 1e-9 for s in segs[:3]]                                            # a norm of ordinary size, and one that clips
    n64 = float(torch.linalg.vector_norm(torch.cat([s.double() for s in small])))
    out3, _ = _norm_launch(small, n64 / 3)
    n32 = out3[0]
    assert abs(float(n32) - n64) <= float(torch.nextafter(n32, n32 * 2) - n32)
    want = (torch.tensor(n64 / 3, dtype=torch.float32, device=n32.device) / (n32 + 1e-6))
    assert abs(float(out3[1]) - float(want)) <= 1e-6 * float(want) and 0.3 < float(out3[1]) < 0.34
    bad = base.clone()
    bad[4111 + 1_234_567] = float("inf")
    out4, tk4 = _norm_launch([bad[0:1], bad[4111:4111 + 3_300_001]], 1.0)
    assert not torch.isfinite(out4[0]) and int(tk4.abs().sum()) == 0
    assert float(out4[1]) == 0.0                                                    # torch: max_norm / (inf + 1e-6) = 0
    bad[5] = float("nan")
    out5, _ = _norm_launch([bad[0:8]], 1.0)
    assert torch.isnan(out5[0]) and torch.isnan(out5[1])                            # (torch.clamp keeps a NaN coefficient)


def _one_clipped_step(mau, cls, kw, c, fused_clip, batch, prec="fp32"):
    net = _net(mau, prec)
    x, ts, md, tgt = batch
    mau.compute_loss_mse(net(x, ts, md), tgt)["total"].backward()
    if fused_clip:
        opt = cls(net.parameters(), max_grad_norm=c, **kw)
        opt.step()
        norm = opt.last_grad_norm.clone() if c > 0 else None
    else:
        opt = cls(net.parameters(), **kw)
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), c) if c > 0 else None
        opt.step()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    torch.cuda.synchronize()
    return net, norm, grads


@pytest.mark.parametrize("name,kw", [("SGD", dict(lr=0.02, momentum=0.9, weight_decay=1e-2)), ("Adam", dict(lr=2e-3, weight_decay=1e-2)),
                                     ("AdamW", dict(lr=2e-3, weight_decay=1e-2))], ids=["sgd", "adam", "adamw"])
def test_fused_clipping_matches_clip_grad_norm(mau, name, kw):
    """max_grad_norm=c inside the fused step against torch.nn.utils.clip_grad_norm_(parameters, c) followed by the same optimizer
    without it, identical nets and batch, c taken from a first measured norm: c = norm / 3 clips, c = 10 norm does not.
    ``last_grad_norm`` within 1e-6 relative of torch's norm (torch adds per-tensor fp32 norms, the kernel accumulates in fp64: they
    differ by fp32 rounding); parameters after the step within the one-step tolerance 1e-6 + 1e-5 max|p|; without clipping bitwise the
    step of the optimizer that has no max_grad_norm."""
    cls = {"SGD": mau.SGD, "Adam": mau.Adam, "AdamW": mau.AdamW}[name]
    batch = _batches(1)[0]
    _, norm0, _ = _one_clipped_step(mau, cls, kw, 1e30, False, batch)
    norm0 = float(norm0)
    assert norm0 > 0
    plain, _, _ = _one_clipped_step(mau, cls, kw, 0.0, True, batch)
    for c, clips in ((norm0 / 3, True), (10 * norm0, False)):
        ref, nt, gt = _one_clipped_step(mau, cls, kw, c, False, batch)
        got, nm, gm = _one_clipped_step(mau, cls, kw, c, True, batch)
        print(f"{name} c={c!r}: clip_grad_norm_ {float(nt)!r}  last_grad_norm {float(nm)!r}  rel {abs(float(nm) - float(nt)) / float(nt):.3e}")
        assert nm.dim() == 0 and nm.is_cuda
        assert abs(float(nm) - float(nt)) <= 1e-6 * float(nt), (float(nm), float(nt))
        _step_one_close(ref, got)
        # documented difference: the convolution weights' .grad keeps the unclipped gradient, the small parameters' are scaled
        k = "model.conv2_0.conv1.weight"
        if clips:
            assert rel_l2(gm[k].cpu() / 3, gt[k].cpu()) < 1e-3
            kb = "model.conv2_0.bn1.weight"
            assert rel_l2(gm[kb].cpu(), gt[kb].cpu()) < 1e-3
            moved = max(float((p - q).abs().max()) for p, q in zip(plain.parameters(), got.parameters()))
            assert moved > 0                                                      # (the clipped step IS another step)
        else:
            for (kk, p), (_, q) in zip(plain.named_parameters(), got.named_parameters()):
                assert torch.equal(p, q), kk


def _train_steps(mau, make_opt, steps, graphed, clip=0.0, prec="bf16", seed=60):
    torch.manual_seed(seed)
    net = mau.UrbanPredictor("unet", 6, 24, 16, 4, 16, 24, 2, base_filters=16, temporal_embeddings=True, metadata_embeddings=True).cuda().set_precision(prec).train()
    opt = make_opt(net.parameters())
    crit = mau.compute_loss_mse_gradient
    g = torch.Generator().manual_seed(seed + 1)
    step = mau.GraphedTrainStep(net, opt, crit, warmup=2, clip_grad_norm=clip) if graphed else None
    if not graphed and clip > 0:
        opt.max_grad_norm = clip
    losses, norms = [], []
    for _ in range(steps):
        x, ts, md = torch.randn(3, 6, 64, 48, generator=g).cuda(), torch.randn(3, 24, generator=g).cuda(), torch.randn(3, 4, generator=g).cuda()
        tgt = torch.randn(3, 2, 64, 48, generator=g).cuda()
        if graphed:
            losses.append(step(x, ts, md, tgt).clone())
        else:
            loss = crit(net(x, ts, md), tgt)["total"]
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach().clone())
        if opt.last_grad_norm is not None:
            norms.append(opt.last_grad_norm.clone())
    if graphed:
        from mau_amd import functional as F_
        assert step.graph is not None and step.calls == steps
        # the captured step holds no re-pack of its own: the optimizer wrote the packs of the weights the next forward reads
        assert step._self_packing is True and step.clip == 0.0
        assert step._groups and all(pg.fresh_after_step == F_._GENERATION[0] for pg in step._groups)
    net.eval()
    with torch.no_grad():
        ev = net(x, ts, md)
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, ev, norms


@pytest.mark.parametrize("which", ["sgd", "adam", "adamw-clip"])
def test_graphed_train_step_with_the_optimizer_family_matches_eager(mau, which):
    """GraphedTrainStep with mau.SGD, mau.Adam and mau.AdamW(max_grad_norm=c): six steps (two eager warm-ups, the capture, three
    replays) give bit for bit the losses, parameters, buffers and following eval output of the same steps run eagerly."""
    clip = 0.0
    if which == "sgd":
        make = lambda ps: mau.SGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-3)          # noqa: E731
    elif which == "adam":
        make = lambda ps: mau.Adam(ps, lr=1e-3, weight_decay=1e-3)                       # noqa: E731
    else:
        make = lambda ps: mau.AdamW(ps, lr=1e-3, weight_decay=1e-3)                      # noqa: E731
        probe = _train_steps(mau, lambda ps: mau.AdamW(ps, lr=1e-3, weight_decay=1e-3, max_grad_norm=1e30), 1, graphed=False)
        clip = float(probe[3][0]) / 3                                                    # a bound that clips the first steps at least
    a = _train_steps(mau, make, 6, graphed=False, clip=clip)
    b = _train_steps(mau, make, 6, graphed=True, clip=clip)
    for la, lb in zip(a[0], b[0]):
        assert torch.equal(la, lb), (a[0], b[0])
    assert float(a[0][0]) != float(a[0][5])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2])
    if clip > 0:
        assert len(a[3]) == 6 and len(b[3]) == 6
        for na, nb in zip(a[3], b[3]):
            assert torch.equal(na, nb) and torch.isfinite(na)
        assert float(a[3][0]) > clip                                                     # (it did clip)


@pytest.mark.parametrize("case", ["sgd", "clipping"])
def test_train_cli_constructs_the_fused_optimizers(mau, case, tmp_path, monkeypatch):
    """``mau_amd.train.run`` with ``optimizer: SGD`` and with ``gradient_clipping: 1``: two epochs of synthetic batches (eager warm-ups,
    capture, replays) end with finite train and validation losses on the fused classes; with clipping on, the optimizer clips (a
    finite ``last_grad_norm``) and ``torch.nn.utils.clip_grad_norm_`` is never called."""
    from mau_amd import train
    from mau_amd.config import CONFIG
    monkeypatch.setitem(CONFIG, "MODELS_DIR", str(tmp_path))
    monkeypatch.setitem(CONFIG.dataset, "image_shape_edge", 64)
    monkeypatch.setitem(CONFIG.training, "batch_size", 4)
    monkeypatch.setitem(CONFIG.training, "learning_rate", 1e-3)
    if case == "sgd":
        monkeypatch.setitem(CONFIG.training, "optimizer", "SGD")
    else:
        monkeypatch.setitem(CONFIG.training, "gradient_clipping", 1)

    def refuse(*a, **k):
        raise AssertionError("torch.nn.utils.clip_grad_norm_ was called: the fused optimizer clips")

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", refuse)
    res = train.run(device="gpu", temporal_embeddings=False, metadata_embeddings=True, model_type="unet", jobid="o", epochs=2,
                    steps_per_epoch=3, precision="bf16", val_batches=1)
    opt = res["optimizer"]
    assert type(opt) is (mau.SGD if case == "sgd" else mau.AdamW)
    assert len(res["history"]) == 2
    for tr, va in res["history"]:
        assert tr == tr and va == va and abs(tr) < float("inf") and abs(va) < float("inf"), res["history"]
    if case == "clipping":
        assert opt.max_grad_norm == 5.0
        assert opt.last_grad_norm is not None and bool(torch.isfinite(opt.last_grad_norm))
    else:
        assert opt.max_grad_norm == 0.0 and opt.last_grad_norm is None
        assert opt.param_groups[0]["momentum"] == CONFIG.training.momentum
