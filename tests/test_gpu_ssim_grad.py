"""``mau_ssim_loss_grad`` (csrc/ssim.hip) on the device, and its way up: ``functional.SSIMLoss``, ``compute_loss_l1_grad_ssim_trained``,
``GraphedTrainStep`` and ``train.run(ssim_gradient=True)``.

The kernel is compared, in ALL B*C*H*W elements, with the float64 closed form of ``tests/ssim_grad_ref.py``.  The bound is not a constant:
it is 4 x ``dev32``, the same measure (max |g - g64| / max |g64|) of float32 autograd of the torch spelling on the same input, computed
here on the CPU.  The kernel forms s2 - s0^2 from the same cancelling fp32 difference and sums the 121 taps separably, two roundings
per pass in another order: an error of the same kind that need not be the smaller one -- hence the factor 4.

Shapes (the smallest at which each thing can go wrong):
  (1,2,11,11)    a single map pixel              (1,2,12,27)    map 2x17: ragged tile in x
  (2,2,26,26)    map 16x16: one full map tile    (2,2,27,43)    map 17x33: seams in both axes, ragged last tiles, two images
  (1,2,384,384)  f = round(1.5) = 2              (1,2,385,391)  f = 2 with a dropped last row and column
  (1,2,640,640)  f = round(2.5) = 2 (half to even; a round-half-up would pool by 3)
  (2,3,20,20)    prep = 0, C != 2
"""
import pytest
import torch

from tests import ssim_grad_ref as R
from tests._helpers import _call, _stream, bits, mau, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

_IDS = ["x".join(map(str, s)) + ("" if p else "-noprep") for s, p in R.SHAPES]
_CACHE = {}


def _case(key):
    """(out, tgt, g64, dev32) of a case, computed once on the CPU and never changed"""
    if key not in _CACHE:
        if key == "flat":
            out, tgt, prep = *R.make_flat_inputs(21), True
        else:
            shape, prep = key
            out, tgt = R.make_inputs(shape, 20)
        g64 = R.ssim_grad_ref(out, tgt, prep)
        dev32 = R.rel_max(R.ssim_grad_autograd(out, tgt, prep, dtype=torch.float32), g64)
        _CACHE[key] = (out, tgt, g64, dev32)
    return _CACHE[key]


def _grad(out, tgt, prep=True, scale=1.0, fill=float("nan")):
    o, t = out.cuda().contiguous(), tgt.cuda().contiguous()
    B, C, H, W = o.shape
    d = torch.full_like(o, fill)
    _call("mau_ssim_loss_grad", o.data_ptr(), t.data_ptr(), d.data_ptr(), float(scale), int(prep), B, C, H, W, _stream())
    torch.cuda.synchronize()
    return d


def _check_against_float64(mau, key, prep, label):
    out, tgt, g64, dev32 = _case(key)
    d = _grad(out, tgt, prep)
    assert not torch.isnan(d).any(), "an element of dout was not written"
    err = R.rel_max(d, g64)
    print(f"{label}: err {err:.3e}  dev32 {dev32:.3e}  err/dev32 {err / dev32:.2f}")
    assert 0 < dev32 < 1e-3
    assert err <= 4 * dev32, (label, err, dev32)
    assert same_bits(_grad(out, tgt, prep, fill=0.0), d)             # determinism: same bits again, whatever dout held before
    return d


@pytest.mark.parametrize("shape,prep", R.SHAPES, ids=_IDS)
def test_gradient_against_float64(mau, shape, prep):
    d = _check_against_float64(mau, (shape, prep), prep, f"{shape} prep={int(prep)}")
    out = _case((shape, prep))[0]
    H, W = shape[2:]
    f = R.pool_factor(H, W)
    z = bits(d.cpu()) == 0                                            # the bit pattern of +0.0
    if prep:
        outside = (out[:, 1] < 0) | (out[:, 1] > 1)
        assert z[:, 1][outside].all()                                  # +0.0 where clamp() cut channel 1 off
        assert not z[:, 1, :H // f * f, :W // f * f][~outside[:, :H // f * f, :W // f * f]].any()
        if min(H, W) >= 26:
            assert outside.any() and (~outside).any()                  # (both branches occur)
    assert z[:, :, H // f * f:, :].all() and z[:, :, :, W // f * f:].all()     # +0.0 in what avg_pool2d drops
    assert not z[:, 0, :H // f * f, :W // f * f].any()
    if shape == (1, 2, 385, 391):
        assert z[:, :, 384:, :].numel() > 0 and z[:, :, :, 390:].numel() > 0


def test_gradient_on_flat_input(mau):
    """Variances tiny against c2, the cancellation at its worst (dev32 about 1.5e-4): the same rule."""
    _check_against_float64(mau, "flat", True, "flat (1, 2, 32, 32)")


def test_clamp_bounds_with_planted_values(mau):
    """Gradient reaches a channel-1 value ON a bound of the clamp (0.0, -0.0, 1.0); one ulp outside there is +0.0."""
    out, tgt = R.make_inputs((2, 2, 27, 43), 22)
    out[:, 1].clamp_(0.05, 0.95)
    one = torch.tensor(1.0)
    planted = {(0, 5, 5): 0.0, (0, 5, 30): 1.0, (1, 20, 5): float(torch.nextafter(0 * one, -one)), (1, 20, 30): float(torch.nextafter(one, 2 * one)),
               (0, 12, 4): -0.3, (1, 12, 12): 1.7, (1, 3, 14): -0.0}
    for (b, r, c), v in planted.items():
        out[b, 1, r, c] = v
    d = _grad(out, tgt).cpu()
    g64 = R.ssim_grad_ref(out, tgt)
    dev32 = R.rel_max(R.ssim_grad_autograd(out, tgt, dtype=torch.float32), g64)
    assert R.rel_max(d, g64) <= 4 * dev32
    for (b, r, c), v in planted.items():
        if 0.0 <= v <= 1.0:
            assert float(d[b, 1, r, c]) != 0.0 and float(g64[b, 1, r, c]) != 0.0, (b, r, c, v)
        else:
            assert int(bits(d)[b, 1, r, c]) == 0, (b, r, c, v)
    assert int((d[:, 1] == 0).sum()) == 4


def test_scale_is_the_last_factor(mau):
    """``scale = 0.5`` gives exactly half of ``scale = 1``: 2 d(0.5) == d(1) bit for bit, the zeros still +0.0."""
    out, tgt, g64, _ = _case(((2, 2, 27, 43), True))
    d1, dh, d4 = _grad(out, tgt), _grad(out, tgt, scale=0.5), _grad(out, tgt, scale=4.0)
    assert same_bits(2 * dh, d1) and same_bits(0.25 * d4, d1)
    assert float(d1.abs()[d1 != 0].min()) > 1e-30                         # (no subnormal that halving would round)
    assert int((bits(dh) == 0).sum()) == int((bits(d1) == 0).sum()) > 0
    d3 = _grad(out, tgt, scale=3.0)
    assert same_bits(d3, 3.0 * d1)


def test_refuses_what_ssim_loss_refuses(mau):
    from mau_amd._lib import MauError
    o = torch.zeros(1, 2, 8, 8, device="cuda")
    with pytest.raises(MauError, match="smaller than the 11x11 window"):
        _call("mau_ssim_loss_grad", o.data_ptr(), o.data_ptr(), o.data_ptr(), 1.0, 1, 1, 2, 8, 8, _stream())


def _cuda_inputs(shape, seed):
    out, tgt = R.make_inputs(shape, seed)
    return out.cuda(), tgt.cuda()


def test_trained_criterion_values_and_gradient(mau):
    """The same four values as ``compute_loss_l1_grad_ssim``, bit for bit; the gradient is d_l1 + 0.1 d_grad + 0.5 d_ssim, assembled here in
    float64 from ``L1GradientLoss`` and ``mau_ssim_loss_grad``, to the fp32 rounding of that sum: four roundings (fp32(0.1), its
    product, two additions; the product with 0.5 is exact), each at most 2^-24 of the sum of the terms' magnitudes."""
    from mau_amd.functional import L1GradientLoss
    from mau_amd.losses import ssim_loss
    out, tgt = _cuda_inputs((2, 2, 27, 43), 23)
    o = out.clone().requires_grad_(True)
    got = mau.compute_loss_l1_grad_ssim_trained(o, tgt)
    want = mau.compute_loss_l1_grad_ssim(out.clone().requires_grad_(True), tgt)
    assert list(got) == list(want) == ["total", "pixel", "gradient", "ssim"]
    for k in want:
        assert same_bits(got[k].detach(), want[k].detach()), k
    assert got["ssim"].requires_grad and not want["ssim"].requires_grad
    assert same_bits(ssim_loss(out, tgt, differentiable=True)[1], ssim_loss(out, tgt)[1])
    got["total"].backward(retain_graph=True)
    o1 = out.clone().requires_grad_(True)
    l1, gr = L1GradientLoss.apply(o1, tgt)
    d_l1 = torch.autograd.grad(l1, o1, retain_graph=True)[0].double()
    d_gr = torch.autograd.grad(gr, o1)[0].double()
    d_s = _grad(out, tgt).double()
    w_gr = float(torch.tensor(0.1, dtype=torch.float32))
    want_g = d_l1 + w_gr * d_gr + 0.5 * d_s
    tol = 4 * 2.0 ** -24 * (d_l1.abs() + w_gr * d_gr.abs() + 0.5 * d_s.abs())
    assert bool(((o.grad.double() - want_g).abs() <= tol).all())
    assert float((0.5 * d_s).abs().max()) > 100 * float(tol.max())        # (the SSIM part is far above that rounding: it is in there)
    # retain_graph: a second backward accumulates the same gradient again
    first = o.grad.clone()
    got["total"].backward()
    assert same_bits(o.grad, 2 * first)
    # no gradient asked for: value only, nothing saved
    with torch.no_grad():
        v = mau.compute_loss_l1_grad_ssim_trained(out, tgt)
    assert same_bits(v["total"], want["total"].detach()) and not v["total"].requires_grad


def _steps(mau, crit, graphed, n=5):
    """``n`` training steps of the smallest U-Net of tests/test_gpu_model.py's graphed-step tests, on a different batch each."""
    torch.manual_seed(5)
    net = mau.UrbanPredictor("unet", 6, 10, 8, 4, 8, 12, 2, base_filters=8, temporal_embeddings=False, metadata_embeddings=True).cuda().train()
    opt = mau.AdamW(net.parameters(), lr=1e-3)
    step = mau.GraphedTrainStep(net, opt, crit, warmup=2) if graphed else None
    g = torch.Generator().manual_seed(6)
    losses, first = [], None
    for _ in range(n):
        x, ts, md = torch.randn(2, 6, 32, 32, generator=g).cuda(), torch.randn(2, 10, generator=g).cuda(), torch.randn(2, 4, generator=g).cuda()
        tgt = torch.randn(2, 2, 32, 32, generator=g).cuda()
        if graphed:
            losses.append(step(x, ts, md, tgt).clone())
        else:
            loss = crit(net(x, ts, md), tgt)["total"]
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach().clone())
            del loss
        if first is None:
            first = {k: v.detach().clone() for k, v in net.state_dict().items()}
    if graphed:
        assert step.graph is not None and step.calls == n
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, first


def test_through_the_graphed_step(mau):
    """Two eager steps, a capture and two replays with the trained criterion: the losses and weights are the bits of the same five
    steps run eagerly; and after the FIRST step the weights differ from a run with the detached criterion -- the term trains."""
    a = _steps(mau, mau.compute_loss_l1_grad_ssim_trained, graphed=False)
    b = _steps(mau, mau.compute_loss_l1_grad_ssim_trained, graphed=True)
    for la, lb in zip(a[0], b[0]):
        assert torch.equal(la, lb), (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert all(bool(torch.isfinite(v).all()) for v in a[1].values() if v.is_floating_point())
    c = _steps(mau, mau.compute_loss_l1_grad_ssim, graphed=False, n=1)
    assert torch.equal(c[0][0], a[0][0])                                 # the same first loss: same weights, same batch, same value
    assert any(not torch.equal(a[2][k], c[2][k]) for k in a[2] if k.endswith("weight"))


def test_train_run_with_the_flag(mau, tmp_path, monkeypatch):
    from mau_amd import train
    from mau_amd.config import CONFIG
    monkeypatch.setitem(CONFIG, "MODELS_DIR", str(tmp_path))
    monkeypatch.setitem(CONFIG.dataset, "image_shape_edge", 64)
    monkeypatch.setitem(CONFIG.training, "batch_size", 2)
    monkeypatch.setitem(CONFIG.training, "loss", "l1-gradient-ssim")
    kw = dict(device="gpu", temporal_embeddings=False, metadata_embeddings=True, model_type="unet", epochs=1, steps_per_epoch=2,
              precision="bf16", val_batches=1)
    res = train.run(jobid="sg", ssim_gradient=True, **kw)
    assert res["step"] == 2 and len(res["history"]) == 1 and all(v == v and abs(v) < float("inf") for v in res["history"][0])
    assert set(res["val_terms"][0]) == {"total", "mse", "gradient", "pixel", "ssim"}
    ck = torch.load(res["checkpoint_path"], map_location="cpu", weights_only=False)
    assert ck["hyperparameters"]["ssim_gradient"] is True
    plain = train.run(jobid="pl", **kw)
    ck0 = torch.load(plain["checkpoint_path"], map_location="cpu", weights_only=False)
    assert "ssim_gradient" not in ck0["hyperparameters"]
    assert set(ck["hyperparameters"]) - set(ck0["hyperparameters"]) == {"ssim_gradient"}
    assert set(ck) == set(ck0)
    monkeypatch.setitem(CONFIG.training, "loss", "mse")
    with pytest.raises(ValueError, match="ssim-gradient"):
        train.run(jobid="no", ssim_gradient=True, **kw)
