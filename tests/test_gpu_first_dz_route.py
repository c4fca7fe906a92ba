"""The first layer's dz route through ``functional``: above ``_FIRST_DZ_FUSED_MIN_WORK`` pixels the weight-gradient kernel forms dz itself
(``mau_conv3x3_first_wgrad_bn``) and ``mau_bn_relu_bwd_apply`` is not launched for the layer.  The two routes must give the same bits
-- every parameter gradient and the loss of an eager step, every parameter after two steps of the captured step -- and at the default
threshold a small network launches exactly what it launched before the route existed."""
import pytest
import torch

from tests._helpers import first_difference, mau, patched, recorded_calls, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

NEVER = 2 ** 62
SIZE = (2, 6, 32, 48)


def _net(mau):
    torch.manual_seed(5)
    net = mau.UrbanPredictor("unet", 6, 10, 16, 4, 16, 24, 2, base_filters=64, temporal_embeddings=False, metadata_embeddings=True)
    return net.cuda().set_precision("bf16").train()


def _batch(seed=6):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = SIZE
    return (torch.randn(N, C, H, W, generator=g).cuda(), torch.randn(N, 10, generator=g).cuda(), torch.randn(N, 4, generator=g).cuda(),
            torch.randn(N, 2, H, W, generator=g).cuda())


def _eager_step(mau, min_work):
    """(loss, {name: grad}, recorded calls) of one training step of a fresh network; min_work None = the default threshold"""
    from mau_amd import functional as F_
    net, (x, ts, md, tgt) = _net(mau), _batch()
    hooks = {} if min_work is None else dict(_FIRST_DZ_FUSED_MIN_WORK=min_work)
    with patched(F_, **hooks), recorded_calls(mau) as rows:
        loss = mau.compute_loss_mse(net(x, ts, md), tgt)["total"]
        loss.backward()
        torch.cuda.synchronize()
    return loss.detach().cpu(), {n: p.grad.detach().cpu() for n, p in net.named_parameters() if p.grad is not None}, rows


@pytest.fixture(scope="module")
def steps(mau):
    return {k: _eager_step(mau, v) for k, v in (("fused", 0), ("two", NEVER), ("default", None))}


def _names(rows):
    return [r[0] for r in rows]


def test_gradients_and_loss_are_bit_equal(steps):
    (l1, g1, _), (l2, g2, _) = steps["fused"], steps["two"]
    assert same_bits(l1, l2)
    assert sorted(g1) == sorted(g2) and len(g1) > 20
    for n in g1:
        assert same_bits(g1[n], g2[n]), n


def test_the_fused_route_drops_one_apply_launch(steps):
    fused, two = _names(steps["fused"][2]), _names(steps["two"][2])
    assert fused.count("mau_conv3x3_first_wgrad_bn") == 1 and fused.count("mau_conv3x3_first_wgrad") == 0
    assert fused.count("mau_bn_relu_bwd_apply") == 12
    assert two.count("mau_conv3x3_first_wgrad_bn") == 0 and two.count("mau_conv3x3_first_wgrad") == 1
    assert two.count("mau_bn_relu_bwd_apply") == 13
    # nothing else moves: without the three names the two sequences are one
    moved = ("mau_conv3x3_first_wgrad_bn", "mau_conv3x3_first_wgrad", "mau_bn_relu_bwd_apply")
    assert [n for n in fused if n not in moved] == [n for n in two if n not in moved]
    # the fused call runs where the weight gradient ran: same position from the end, same stream
    rf = [r for r in steps["fused"][2] if r[0] == "mau_conv3x3_first_wgrad_bn"][0]
    rt = [r for r in steps["two"][2] if r[0] == "mau_conv3x3_first_wgrad"][0]
    assert rf[-1] == rt[-1] and rf[-8:] == rt[-8:]               # Cin, Cout, dtype, N, H, W, stream


def test_default_threshold_keeps_the_parent_route_at_this_size(steps):
    diff = first_difference(steps["default"][2], steps["two"][2], "default against never")
    assert diff is None, diff


def _graphed_params(mau, min_work):
    from mau_amd import functional as F_
    net, batch = _net(mau), _batch()
    with patched(F_, _FIRST_DZ_FUSED_MIN_WORK=min_work):
        opt = mau.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3)
        step = mau.GraphedTrainStep(net, opt, lambda o, t: mau.compute_loss_mse(o, t), warmup=1)
        losses = [step(*batch).clone() for _ in range(2)]        # one eager step, then the captured one
        torch.cuda.synchronize()
    assert step.graph is not None
    return [v.cpu() for v in losses], {n: p.detach().cpu() for n, p in net.named_parameters()}


def test_captured_step_is_bit_equal(mau):
    (l1, p1), (l2, p2) = _graphed_params(mau, 0), _graphed_params(mau, NEVER)
    assert all(same_bits(a, b) for a, b in zip(l1, l2))
    for n in p1:
        assert same_bits(p1[n], p2[n]), n
