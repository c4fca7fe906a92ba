"""The launch sequence of ``functional``: every call through ``functional.call`` of one training step, one eval forward and one
frozen eval forward, compared call for call with ``tests/golden/launch_trace.json`` -- recorded by
``tests/golden/make_launch_trace.py`` at the PARENT of a change that moves host code around without changing what is launched.

A call is recorded as ``[name, args...]``; ``_lib.PROTOTYPES[name]`` tells pointers from scalars:
  * a scalar verbatim (a float as ``float.hex``);
  * a pointer as 0 / 1 (null or not) -- addresses differ from run to run, whether an optional operand is passed does not;
  * the trailing stream as "main" (the stream current when the case started) or "side".
The real call still runs.  The SyncBN branch needs more than one GPU: tests/test_dist_gloo.py, tests/test_gpu_dist_rehearsal.py."""
import json
import os

import pytest
import torch

from tests._helpers import first_difference, mau, patched, recorded_calls  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")

# every hook of functional pinned to its default, so that a case's ``hooks`` are the only difference from the first case
DEFAULT_HOOKS = dict(_OVERLAP_WGRAD=2, _FUSED_REDUCE=True, _FUSED_BN=True, _FUSED_UP=True, _PACK_MULTI=True, _INFER_POOL_FUSED=True,
                     _FIRST_WGRAD=True, _DGRAD_FIRST=None, _EMB_FOLD=True, _EMB_FOLD_MIN_WORK=1 << 20)

UNET = dict(model_type="unet", base_filters=16, prec="bf16", size=(64, 48), emb_dims=(16, 16),
            flags=dict(temporal_embeddings=False, metadata_embeddings=True))
CASES = {
    # first-layer kernel, fused pool / head / upsample, mau_conv3x3_fwd_pool
    "unet_bf16": UNET,
    # pool windows that miss the last row / column, the second resize
    "unet_bf16_odd": dict(UNET, size=(62, 50)),
    # out_view row buffers, Fanout, dgrad_first, virtual concat, the embedding fold (64 + 64 embedding channels as in production, and
    # switched on at this size): the folded layers run on a DERIVED weight, whose gradient never takes the deferred join
    "unetpp_bf16": dict(model_type="unet++", base_filters=64, prec="bf16", size=(64, 64), emb_dims=(64, 64), flags={},
                        hooks=dict(_EMB_FOLD_MIN_WORK=0)),
    # ToNHWC, no first-layer kernel, materialised concat
    "unet_fp32": dict(UNET, base_filters=64, prec="fp32", size=(32, 32)),
    # unfused head, pool + skip and upsample backward
    "unet_bf16_unfused_bn": dict(UNET, hooks=dict(_FUSED_BN=False)),
    # the stream tag and the join placement
    "unet_bf16_overlap0": dict(UNET, hooks=dict(_OVERLAP_WGRAD=0)),
    "unet_bf16_overlap1": dict(UNET, hooks=dict(_OVERLAP_WGRAD=1)),
    "unet_bf16_overlap2": dict(UNET, hooks=dict(_OVERLAP_WGRAD=2)),
    # eval coefficients with a saved context, dbias = scale * dbeta
    "unet_bf16_eval_grad": dict(UNET, eval_grad=True),
}


def record_case(mau, case):
    """One fresh network: a training step (``eval_grad``: the same in eval mode), an eval no-grad forward, a frozen one."""
    from mau_amd import functional as F_
    torch.manual_seed(11)
    H, W = case["size"]
    g = torch.Generator().manual_seed(12)
    x, ts, md = torch.randn(2, 6, H, W, generator=g).cuda(), torch.randn(2, 10, generator=g).cuda(), torch.randn(2, 4, generator=g).cuda()
    tgt = torch.randn(2, 2, H, W, generator=g).cuda()
    tdim, mdim = case["emb_dims"]
    net = mau.UrbanPredictor(case["model_type"], 6, 10, tdim, 4, mdim, 24, 2, base_filters=case["base_filters"], **case["flags"])
    net = net.cuda().set_precision(case["prec"])
    torch.cuda.synchronize()
    with patched(F_, **dict(DEFAULT_HOOKS, **case.get("hooks", {}))), recorded_calls(mau) as rows:
        net.eval() if case.get("eval_grad") else net.train()
        mau.compute_loss_mse(net(x, ts, md), tgt)["total"].backward()
        net.eval()
        with torch.no_grad():
            net(x, ts, md)
            net.freeze_inference(True)
            net(x, ts, md)
        torch.cuda.synchronize()
    return rows


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert all(len(rows) > 50 for rows in golden["cases"].values())


@pytest.mark.parametrize("name", list(CASES))
def test_launch_trace_matches_the_recorded_one(mau, golden, name):
    diff = first_difference(record_case(mau, CASES[name]), golden["cases"][name], name)
    assert diff is None, diff
