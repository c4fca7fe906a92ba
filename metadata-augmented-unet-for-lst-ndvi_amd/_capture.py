"""What the captured sessions share (``GraphedInference``, ``ComparisonSession`` and, through ``_tile.TileSession``, ``ScenarioSession``,
``PlacementSession`` and ``RegionSession``): freezing a model, the warm-up and capture sequence, and the pinned staging buffer of a
host input.  The replay paths stay in the sessions."""
from __future__ import annotations

import numpy as np
import torch


def freeze(model: torch.nn.Module) -> torch.dtype:
    """Eval mode and ``freeze_inference(True)`` (packed weights and folded BatchNorm coefficients are computed once, outside the
    graph); returns the type the network computes in."""
    model.eval()
    if hasattr(model, "freeze_inference"):
        model.freeze_inference(True)
    return getattr(model, "model", model)._rt.dtype


def warm_up_and_capture(run, device, warmup: int):
    """``run()`` ``max(1, warmup)`` times on a fresh side stream, then once more into a hipGraph: (graph, what that call returned)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(max(1, warmup)):            # packs weights, sets kernel attributes, warms the allocator
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = run()
    return graph, out


class PinnedStage:
    """A pinned host buffer and the event of its last copy out: host inputs of a session travel through it."""

    def __init__(self, shape, dtype: torch.dtype):
        self.buf = torch.empty(shape, dtype=dtype).pin_memory()
        self.copied = torch.cuda.Event()

    def upload(self, src, dst: torch.Tensor) -> None:
        """``src`` (host tensor or numpy array) -> ``dst`` (device), non-blocking."""
        self.copied.synchronize()                  # the previous call's copy out of the pinned buffer has finished
        self.buf.copy_(src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src)))
        dst.copy_(self.buf, non_blocking=True)
        self.copied.record()
