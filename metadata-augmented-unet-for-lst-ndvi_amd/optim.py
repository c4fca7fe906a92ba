"""``mau_amd.AdamW`` / ``mau_amd.Adam`` / ``mau_amd.SGD``: the reference's three optimizers (src/train.py:209-216;
conf/config.yaml:41,48,52) with the update of every 3x3 convolution weight of a network and the re-pack of the updated weights into
the matrix-core layouts done by ONE kernel (``mau_opt_pack_step``, csrc/optim.hip; the update rule is a template parameter).

Same constructor arguments, same update rules, same ``state_dict`` layout as the torch class of the same name (``state[p] =
{'step', 'exp_avg', 'exp_avg_sq'}`` / ``{'momentum_buffer'}``: an ``optimizer_state_dict`` written here loads into the torch class
and vice versa).  What differs is the traffic: torch's fused AdamW streams p, g, m, v (28 bytes per parameter), then the forward of
the next step re-reads every weight twice to build its two packs; here a workgroup owns a 64 x 64 x 9 block of a layer, applies the
update and writes both packs from LDS (32 bytes per parameter, one launch: 0.37 -> 0.2 ms per step of the U-Net, measured for AdamW;
EXPERIMENTS.md has the figures of the other two).  The weight gradients are produced straight into a flat arena
(``functional.ConvBNReLU.backward`` writes the split-K sum into the parameter's ``_mau_grad_slot``; autograd adopts that view as
``p.grad``), so the kernel's table of addresses is built once.  All other parameters (BatchNorm, biases, encoders, head: 0.03 % of
the model) go through torch's multi-tensor kernels.  The step count lives on the device: the step is capturable into a
hipGraph (``train_graph.GraphedTrainStep``).

Gradient clipping (src/train.py:253-254) is part of the step: with ``max_grad_norm > 0`` one launch (``mau_grad_norm_clip``) takes the
global L2 norm of the gradients of ALL parameters of the optimizer and writes ``clip_grad_norm_``'s coefficient to device memory;
the fused kernel multiplies every gradient by it as it loads it, the small parameters' gradients are scaled by one multi-tensor
multiply.  ``optimizer.last_grad_norm`` is the 0-dim device tensor of the norm (what ``clip_grad_norm_`` returns).  One difference
from ``clip_grad_norm_`` + ``step()``: the convolution weights' ``.grad`` still holds the UNCLIPPED gradient after the step (the next
backward overwrites it; ``zero_grad`` is unaffected).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import functional as F_
from ._lib import MAU_OPT_ADAM, MAU_OPT_ADAMW, MAU_OPT_SGD, call, lib


def _device_table(host, dev) -> torch.Tensor:
    return torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)


class _PackOptimizer(torch.optim.Optimizer):
    """What the three classes share: the descriptor table of the fused launch, the gradient arena and its slots, the segment table of
    the norm kernel.  A subclass names its rule and state tensors and updates the small parameters (``_init_state``, ``_moments``,
    ``_hyper``, ``_step_rest``)."""
    RULE = -1

    def __init__(self, params, defaults, max_grad_norm: float = 0.0):
        if max_grad_norm < 0:
            raise ValueError(f"{type(self).__name__}: invalid max_grad_norm {max_grad_norm}")
        super().__init__(params, defaults)
        self.max_grad_norm = float(max_grad_norm)      # (an attribute, not a group option: the state_dict stays torch's)
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._tables = {}
        self._arena = None
        self._norm = None

    # ---- what a subclass provides ----
    def _init_state(self, p, group):
        raise NotImplementedError

    def _moments(self, group, st):
        """(m, v) tensors of the fused kernel's table row (None: the rule has no such tensor)."""
        raise NotImplementedError

    def _hyper(self, group):
        """(lr, beta1 or momentum, beta2, eps, weight_decay, nesterov) of the fused launch."""
        raise NotImplementedError

    def _step_rest(self, group, rest):
        raise NotImplementedError

    # ------------------------------------------------------------------ #
    def _conv_params(self, group) -> List[torch.Tensor]:
        return [p for p in group["params"] if p.is_cuda and p.dim() == 4 and p.shape[2:] == (3, 3) and p.dtype == torch.float32
                and getattr(p, "_mau_group", None) is not None and p.is_contiguous()]

    def _ensure_slots(self, convs):
        """Stable gradient addresses: every convolution weight gets a slot of a flat arena (unless dist.GradSync already gave it
        one); the backward writes the weight gradient there and autograd adopts the view as p.grad."""
        missing = [p for p in convs if getattr(p, "_mau_grad_slot", None) is None]
        if missing:
            self._arena = torch.zeros(sum(p.numel() for p in missing), dtype=torch.float32, device=missing[0].device)
            off = 0
            for p in missing:
                p._mau_grad_slot = self._arena[off:off + p.numel()].view_as(p)
                off += p.numel()

    def _table(self, group, convs, pg, code):
        moments = [self._moments(group, self.state[p]) for p in convs]
        st = pg._state.get(code) if pg is not None and code is not None else None
        key = (tuple(p.data_ptr() for p in convs), tuple(p._mau_grad_slot.data_ptr() for p in convs),
               tuple(None if m is None else m.data_ptr() for m, _ in moments), code, None if st is None else tuple(t.data_ptr() for t in st["wf"]))
        tb = self._tables.get(id(pg))
        if tb is None or tb["key"] != key:
            nbytes = lib.mau_adamw_pack_desc_bytes()
            host = ctypes.create_string_buffer(nbytes * len(convs))
            nxt = ctypes.c_int(0)
            index = {id(p): i for i, p in enumerate(pg.params)} if st is not None else {}
            for i, (p, (m, v)) in enumerate(zip(convs, moments)):
                j = index.get(id(p))
                wf = st["wf"][j].data_ptr() if j is not None else None
                wd = st["wd"][j].data_ptr() if j is not None else None
                call("mau_opt_pack_desc_fill", ctypes.addressof(host), i, p.data_ptr(), p._mau_grad_slot.data_ptr(),
                     None if m is None else m.data_ptr(), None if v is None else v.data_ptr(), wf, wd, p.shape[0], p.shape[1], nxt.value,
                     ctypes.addressof(nxt))
            tb = self._tables[id(pg)] = {"key": key, "table": _device_table(host, convs[0].device), "tiles": nxt.value, "packs": st is not None}
        return tb

    # ------------------------------------------------------------------ #
    def _clip_coef(self, fused, rest) -> torch.Tensor:
        """``mau_grad_norm_clip`` over the arena slots of the fused parameters and the gradients of all others; returns the device
        scalar ``min(1, max_grad_norm / (norm + 1e-6))``.  The small gradients are gathered into a flat buffer of this optimizer by
        one multi-tensor copy (unless they already sit in arena slots): the kernel's table holds addresses that never change, so
        the step stays capturable."""
        dev = (fused + rest)[0].device
        for p in rest:
            if not p.is_cuda or p.grad.dtype != torch.float32 or p.grad.device != dev:
                raise RuntimeError(f"{type(self).__name__}(max_grad_norm > 0) needs fp32 gradients on one HIP device")
        nm = self._norm
        rest_key = tuple(id(p) for p in rest)
        if nm is None or nm["rest_key"] != rest_key or nm["dev"] != dev:
            flat = torch.zeros(max(1, sum(p.numel() for p in rest)), dtype=torch.float32, device=dev)
            views, off = [], 0
            for p in rest:
                views.append(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
            nm = self._norm = {"rest_key": rest_key, "dev": dev, "flat": flat, "views": views, "key": None,
                               "tickets": torch.zeros(lib.mau_reduce_tickets_elems(), dtype=torch.int32, device=dev),
                               "out": torch.zeros(2, dtype=torch.float32, device=dev)}
        src = []
        for p, view in zip(rest, nm["views"]):
            slot = getattr(p, "_mau_grad_slot", None)
            if slot is not None and p.grad.is_contiguous() and p.grad.data_ptr() == slot.data_ptr():
                src.append(slot)                        # (under dist.GradSync every gradient lives in the arena already)
            else:
                src.append(view)
        gather = [(v, p.grad) for p, v, s in zip(rest, nm["views"], src) if s is v]
        if gather:
            torch._foreach_copy_([v for v, _ in gather], [g for _, g in gather])
        # contiguous runs of addresses become one segment each (the convolution arena: one)
        spans = sorted((t.data_ptr(), t.numel()) for t in [p._mau_grad_slot for p in fused] + src)
        key = tuple(spans)
        if nm["key"] != key:
            runs = []
            for ptr, n in spans:
                if runs and runs[-1][0] + 4 * runs[-1][1] == ptr:
                    runs[-1][1] += n
                else:
                    runs.append([ptr, n])
            host = ctypes.create_string_buffer(lib.mau_grad_norm_seg_bytes() * len(runs))
            nxt = ctypes.c_int(0)
            for i, (ptr, n) in enumerate(runs):
                call("mau_grad_norm_seg_fill", ctypes.addressof(host), i, ptr, n, nxt.value, ctypes.addressof(nxt))
            nm.update(key=key, table=_device_table(host, dev), nsegs=len(runs), blocks=nxt.value,
                      ws=torch.zeros(nxt.value, dtype=torch.float64, device=dev))
        out = nm["out"]
        call("mau_grad_norm_clip", nm["table"].data_ptr(), nm["nsegs"], nm["blocks"], nm["ws"].data_ptr(), nm["tickets"].data_ptr(),
             self.max_grad_norm, out.data_ptr(), out.data_ptr() + 4, F_._stream())
        self.last_grad_norm = out[0]
        return out[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        work = []
        for group in self.param_groups:
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            for p in live:
                if p.grad.is_sparse:
                    raise RuntimeError(f"{name} does not support sparse gradients")
                self._init_state(p, group)
            convs = [p for p in self._conv_params(group) if p.grad is not None]
            by_group = {}
            for p in convs:
                by_group.setdefault(id(p._mau_group), (p._mau_group, []))[1].append(p)
            for pg, ps in by_group.values():
                self._ensure_slots(ps)
                stray = [p for p in ps if p.grad.data_ptr() != p._mau_grad_slot.data_ptr()]
                if stray:                                   # (a gradient that did not come through the arena: accumulated, cloned ...)
                    torch._foreach_copy_([p._mau_grad_slot for p in stray], [p.grad for p in stray])
            fused_ids = {id(p) for p in convs}
            work.append((group, live, list(by_group.values()), [p for p in live if id(p) not in fused_ids]))
        if not work:
            return loss
        coef = None
        if self.max_grad_norm > 0:
            coef = self._clip_coef([p for _, _, bg, _ in work for _, ps in bg for p in ps], [p for _, _, _, rest in work for p in rest])
        for group, live, by_group, rest in work:
            self._count_step(live)
            lr, b1, b2, eps, wd, nesterov = self._hyper(group)
            for pg, ps in by_group:
                # the packs of the ONE precision the network has been run in ride along (several: the next forward re-packs)
                codes = list(pg._state.keys())
                code = codes[0] if len(codes) == 1 and len(ps) == len(pg.params) else None
                tb = self._table(group, ps, pg, code)
                step = self.state[ps[0]].get("step")
                call("mau_opt_pack_step", tb["table"].data_ptr(), len(ps), tb["tiles"], code if code is not None else F_.MAU_F32, self.RULE,
                     None if step is None else step.data_ptr(), None if coef is None else coef.data_ptr(), lr, b1, b2, eps, wd,
                     int(nesterov), F_._stream())
                if tb["packs"]:
                    pg.fresh_after_step = F_._GENERATION[0] + 1      # (the global step post-hook bumps the generation once, after this returns)
            if rest:
                if coef is not None:
                    torch._foreach_mul_([p.grad for p in rest], coef)
                self._step_rest(group, rest)
        return loss

    def _count_step(self, live):
        pass


class _AdamBase(_PackOptimizer):
    def __init__(self, params, lr, betas, eps, weight_decay, amsgrad, maximize, max_grad_norm):
        name = type(self).__name__
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError(f"{name}: invalid hyper-parameter")
        if amsgrad or maximize:
            raise ValueError(f"{name}: amsgrad / maximize are not implemented by the fused kernel (use the torch.optim class)")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), max_grad_norm)

    def _init_state(self, p, group):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)      # on the device: capturable
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not st["step"].is_cuda and p.is_cuda:                                  # a state_dict written by the torch class
            st["step"] = st["step"].to(p.device, dtype=torch.float32)
        return st

    def _moments(self, group, st):
        return st["exp_avg"], st["exp_avg_sq"]

    def _hyper(self, group):
        return float(group["lr"]), group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], False

    def _count_step(self, live):
        torch._foreach_add_([self.state[p]["step"] for p in live], 1.0)

    def _step_rest(self, group, rest):
        lr, b1, b2, eps, wd, _ = self._hyper(group)
        fn = torch._fused_adamw_ if self.RULE == MAU_OPT_ADAMW else torch._fused_adam_
        fn(rest, [p.grad for p in rest], [self.state[p]["exp_avg"] for p in rest], [self.state[p]["exp_avg_sq"] for p in rest], [],
           [self.state[p]["step"] for p in rest], lr=lr, beta1=b1, beta2=b2, weight_decay=wd, eps=eps, amsgrad=False, maximize=False)


class AdamW(_AdamBase):
    """``torch.optim.AdamW`` (src/train.py:213-214)."""
    RULE = MAU_OPT_ADAMW

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, amsgrad: bool = False,
                 maximize: bool = False, max_grad_norm: float = 0.0):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize, max_grad_norm)


class Adam(_AdamBase):
    """``torch.optim.Adam`` (src/train.py:211-212): ``weight_decay`` is an L2 term added to the gradient."""
    RULE = MAU_OPT_ADAM

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, amsgrad: bool = False,
                 maximize: bool = False, max_grad_norm: float = 0.0):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize, max_grad_norm)


class SGD(_PackOptimizer):
    """``torch.optim.SGD`` (src/train.py:209-210) with ``dampening == 0``.  ``momentum_buffer`` starts as zeros: ``buf = momentum *
    0 + g`` is torch's first-step rule ``buf = g`` when dampening is 0.  ``momentum == 0``: no buffer and no state."""
    RULE = MAU_OPT_SGD

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, maximize: bool = False, max_grad_norm: float = 0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("SGD: invalid hyper-parameter")
        if dampening != 0 or maximize:
            raise ValueError("SGD: dampening != 0 / maximize are not implemented by the fused kernel (use torch.optim.SGD)")
        if nesterov and momentum <= 0:
            raise ValueError("SGD: Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=bool(nesterov)),
                         max_grad_norm)

    def _init_state(self, p, group):
        st = self.state[p]
        if group["momentum"] != 0 and st.get("momentum_buffer") is None:       # (momentum 0: torch keeps no state either)
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _moments(self, group, st):
        return (st["momentum_buffer"] if group["momentum"] != 0 else None), None

    def _hyper(self, group):
        return float(group["lr"]), group["momentum"], 0.0, 0.0, group["weight_decay"], group["nesterov"]

    def _step_rest(self, group, rest):
        # torch's multi-tensor SGD, operation by operation (its fused single-launch form rounds differently from its default one)
        lr, mu, _, _, wd, nesterov = self._hyper(group)
        grads = [p.grad for p in rest]
        if wd != 0:
            grads = torch._foreach_add(grads, rest, alpha=wd)
        if mu != 0:
            bufs = [self.state[p]["momentum_buffer"] for p in rest]
            torch._foreach_mul_(bufs, mu)
            torch._foreach_add_(bufs, grads)
            grads = torch._foreach_add(grads, bufs, alpha=mu) if nesterov else bufs
        torch._foreach_add_(rest, grads, alpha=-lr)
