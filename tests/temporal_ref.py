"""Plain CPU references of the embedding branch's kernels (csrc/lstm.hip, the Linear and metadata-MLP kernels of csrc/head.hip), written
from the formulas; the extension is never imported here.

``lstm_ref`` is an explicit step loop over differentiable torch operators: in float64 it is the REFERENCE of tests/test_gpu_temporal.py,
in float32 the YARDSTICK -- what a plain fp32 evaluation of the same operation (libm nonlinearities, left-to-right sums) loses against
float64.  ``yardstick`` is the one normalisation every comparison there uses: max |a - ref| / max |ref| of one output tensor."""
import functools

import torch

GATE_ORDER = ("i", "f", "g", "o")                              # torch's row blocks of weight_ih / weight_hh / the biases


def lstm_ref(x, w_ih, w_hh, b_ih, b_hh, dtype):
    """nn.LSTM(input_size=1, hidden_size=H, batch_first=True) from h = c = 0 over x (B,T); w_ih (4H) or (4H,1), w_hh (4H,H), b_ih, b_hh
    (4H).  Returns the post-activation gates (B,T,4H) in the order i, f, g, o, the cells (B,T,H) and h_T (B,H), all in ``dtype`` and
    differentiable with respect to whichever arguments require a gradient."""
    x, w_ih, w_hh, b_ih, b_hh = (v.to(dtype) for v in (x, w_ih, w_hh, b_ih, b_hh))
    B, T = x.shape
    H = w_hh.shape[1]
    w_ih = w_ih.reshape(4 * H)
    h = torch.zeros((B, H), dtype=dtype)
    c = torch.zeros((B, H), dtype=dtype)
    gates, cells = [], []
    for t in range(T):
        pre = x[:, t, None] * w_ih[None, :] + b_ih + b_hh + h @ w_hh.t()
        i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
        g = torch.tanh(pre[:, 2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat([i, f, g, o], dim=1))
        cells.append(c)
    return torch.stack(gates, dim=1), torch.stack(cells, dim=1), h


def lstm_ref_all(x, w_ih, w_hh, b_ih, b_hh, dh_last, dtype):
    """Forward values and, for the incoming gradient ``dh_last`` (B,H), the four parameter gradients: a dict of detached ``dtype``
    tensors gates, cells, h_last, dw_ih (4H), dw_hh, db_ih, db_hh."""
    p = [v.detach().clone().to(dtype).requires_grad_(True) for v in (w_ih.reshape(-1), w_hh, b_ih, b_hh)]
    gates, cells, h = lstm_ref(x, *p, dtype)
    g = torch.autograd.grad(h, p, dh_last.to(dtype))
    return {"gates": gates.detach(), "cells": cells.detach(), "h_last": h.detach(), "dw_ih": g[0], "dw_hh": g[1], "db_ih": g[2], "db_hh": g[3]}


def lstm_dw_hh_of_steps(x, w_ih, w_hh, b_ih, b_hh, dh_last, b, t0, t1):
    """the share of sample ``b``'s steps [t0, t1) in dw_hh, float64: sum over those t of dpre_t (x) h_{t-1} -- every step multiplies h
    with its own copy of w_hh, the copies' gradients are the per-step terms"""
    f64 = torch.float64
    x, w_ih, w_hh, b_ih, b_hh, dh = (v.to(f64) for v in (x[b:b + 1], w_ih.reshape(-1), w_hh, b_ih, b_hh, dh_last[b:b + 1]))
    T, H = x.shape[1], w_hh.shape[1]
    copies = [w_hh.clone().requires_grad_(True) for _ in range(T)]
    h, c = torch.zeros((1, H), dtype=f64), torch.zeros((1, H), dtype=f64)
    for t in range(T):
        pre = x[:, t, None] * w_ih[None, :] + b_ih + b_hh + h @ copies[t].t()
        i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
        c = f * c + i * torch.tanh(pre[:, 2 * H:3 * H])
        h = o * torch.tanh(c)
    return sum(torch.autograd.grad(h, copies[t0:t1], dh))


def linear_ref(x, w, b, dout, dtype=torch.float64):
    """out = x w^T + b (b may be None) and the gradients of sum(out * dout): out (N,D), dx (N,F), dw (D,F), db (D)."""
    x, w, dout = x.to(dtype), w.to(dtype), dout.to(dtype)
    out = x @ w.t()
    if b is not None:
        out = out + b.to(dtype)
    return {"out": out, "dx": dout @ w, "dw": dout.t() @ x, "db": dout.sum(0)}


def meta_mlp_ref(md, w0, b0, w2, b2, demb, dtype=torch.float64):
    """Linear(F,Hd) -> ReLU -> Linear(Hd,D) and the gradients of sum(emb * demb); relu'(0) = 0 as in torch.  hidden (N,Hd) is the
    post-ReLU activation, dhidden (N,Hd) the gradient in front of the ReLU."""
    md, w0, b0, w2, b2, demb = (v.to(dtype) for v in (md, w0, b0, w2, b2, demb))
    pre = md @ w0.t() + b0
    hidden = pre.clamp_min(0)
    emb = hidden @ w2.t() + b2
    dhidden = (demb @ w2) * (pre > 0).to(dtype)
    return {"pre": pre, "hidden": hidden, "emb": emb, "dhidden": dhidden, "dw2": demb.t() @ hidden, "db2": demb.sum(0),
            "dw0": dhidden.t() @ md, "db0": dhidden.sum(0)}


def yardstick(ref64, val32):
    """max |val32 - ref64| / max |ref64| of one output tensor (0 / 0 = 0; x / 0 = inf)"""
    ref64, val32 = torch.as_tensor(ref64).double(), torch.as_tensor(val32).double()
    num, den = float((val32 - ref64).abs().max()), float(ref64.abs().max())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


# ---- the inputs of a case, shared by the host and the GPU tests -------------------------------------------------------------------------
def lstm_case(B, T, H, seed, x_scale=1.0, bias=None, forget_bias=None):
    """x (B,T) standard normal times ``x_scale``, weights and biases uniform in +-1/sqrt(H) (torch's initialisation; ``bias``: b_ih = +-bias
    with random signs and b_hh = 0 instead; ``forget_bias``: added to the forget gate's rows of b_ih, so that the cell state and its
    gradient persist over hundreds of steps), dh_last (B,H) standard normal -- float32 tensors from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    u = lambda *shape: (torch.rand(shape, generator=g) * 2 - 1) * k
    x = torch.randn((B, T), generator=g) * x_scale
    w_ih, w_hh, b_ih, b_hh = u(4 * H), u(4 * H, H), u(4 * H), u(4 * H)
    dh = torch.randn((B, H), generator=g)
    if bias is not None:
        b_ih = (torch.randint(0, 2, (4 * H,), generator=g).float() * 2 - 1) * bias
        b_hh = torch.zeros(4 * H)
    if forget_bias is not None:
        b_ih[H:2 * H] += forget_bias
    return {"x": x, "w_ih": w_ih, "w_hh": w_hh, "b_ih": b_ih, "b_hh": b_hh, "dh_last": dh}


LSTM_OUTPUTS = ("gates", "cells", "h_last", "dw_ih", "dw_hh", "db_ih", "db_hh")


@functools.lru_cache(maxsize=None)
def lstm_case_refs(B, T, H, seed, x_scale=1.0, bias=None, forget_bias=None):
    """(inputs, float64 reference, float32 yardstick values) of a case, computed once and shared"""
    c = lstm_case(B, T, H, seed, x_scale, bias, forget_bias)
    args = (c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["dh_last"])
    return c, lstm_ref_all(*args, torch.float64), lstm_ref_all(*args, torch.float32)
