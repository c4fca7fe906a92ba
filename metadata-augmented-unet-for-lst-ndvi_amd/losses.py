"""Mirror of the reference's criteria (src/utils/losses.py) on the HIP path.

* ``compute_loss_mse``            :27-39   F.mse_loss                                   -> HIP kernel
* ``gradient_loss``               :5-25    mean | |dy pred| - |dy tgt| | + same in x    -> HIP kernel
* ``compute_loss_mse_gradient``   :41-57   mse + 0.1 * gradient
* ``compute_loss_l1_grad_ssim``   :59-99   l1 + 0.1 * gradient + 0.5 * (1 - ssim)       (the yaml default, conf/config.yaml:42)
* ``compute_all_loss``            :101-115 every term above, value only                 -> ONE HIP launch (``mau_loss_terms``)
* ``compute_loss_l1_grad_ssim_trained``    the same values, SSIM attached to the graph   (opt-in, ``train --ssim-gradient``; not in the reference)

In the reference the SSIM values pass through ``torch.Tensor(ssim_vals)`` (:89-96), which detaches them: the SSIM
term changes the reported number, never the gradient.  ``compute_loss_l1_grad_ssim`` mirrors that and stays the default.  Whoever
wants the structural term to shape the forecast asks for it: ``ssim_loss(..., differentiable=True)`` and
``compute_loss_l1_grad_ssim_trained`` return the same values with ``d ssim / d outputs`` from one pixel-owned HIP launch
(``mau_ssim_loss_grad``, ``functional.SSIMLoss``), checked against a float64 closed form (``tests/ssim_grad_ref.py``).  ``piq`` (the SSIM provider) is not available in the
build environment, so the SSIM VALUE follows piq's published default algorithm (11x11 Gaussian, sigma 1.5,
k1 0.01, k2 0.03, average-pool downsampling by max(1, round(min(H, W)/256))): one fused HIP reduction
(``mau_ssim_loss``, csrc/ssim.hip), checked on the GPU against the torch-op spelling ``ssim_value_torch`` in ``tests/_helpers.py`` (test infrastructure, not product).
That scalar is **parity-unpinned** (no reference fixture can be generated without piq); everything that carries
gradient in the reference is pinned by fixture ``g9_losses.npz``.
"""
import torch

from .functional import L1GradientLoss, MSELoss, SSIMLoss, _require_cuda, _stream, _tickets
from ._lib import call, lib


def compute_loss_mse(outputs, targets):
    """Same return contract as the reference: {'total': loss, 'mse': loss} (src/utils/losses.py:34-39)."""
    mse = MSELoss.apply(outputs, targets)
    return {"total": mse, "mse": mse}


def gradient_loss(pred, target):
    """src/utils/losses.py:5-25."""
    _, g = L1GradientLoss.apply(pred, target)
    return {"gradient": g}


def compute_loss_mse_gradient(outputs, targets, lambda_grad=0.1):
    """src/utils/losses.py:41-57."""
    mse = MSELoss.apply(outputs, targets)
    _, g = L1GradientLoss.apply(outputs, targets)
    return {"total": mse + lambda_grad * g, "mse": mse, "gradient": g}


def ssim_loss(outputs, targets, differentiable=False):
    """1 - mean over the batch of piq.ssim(prepared outputs, prepared targets) (src/utils/losses.py:72-97) in one HIP
    reduction; the channel preparation (:72-84) happens while the tiles are loaded.  Value only (no gradient) as in the
    reference, unless ``differentiable``: then the same value, attached to ``outputs`` (``functional.SSIMLoss``).  Parity
    unpinned (module docstring).  Returns (loss scalar, per-image SSIM (B,))."""
    _require_cuda(outputs, "compute_loss_l1_grad_ssim")
    if differentiable:
        return SSIMLoss.apply(outputs, targets.detach())
    o = outputs.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    B, C, H, W = o.shape
    ws = torch.empty(lib.mau_ssim_ws_elems(B, C, H, W), dtype=torch.float64, device=o.device)
    per_image = torch.empty(B, dtype=torch.float32, device=o.device)
    loss = torch.empty(1, dtype=torch.float32, device=o.device)
    call("mau_ssim_loss", o.data_ptr(), t.data_ptr(), ws.data_ptr(), per_image.data_ptr(), loss.data_ptr(), 1, B, C, H, W, _stream())
    return loss.reshape(()), per_image


def compute_loss_l1_grad_ssim(outputs, targets, lambda_grad=0.1, lambda_ssim=0.5):
    """src/utils/losses.py:59-99 (same dict keys).  Gradient = d(l1 + lambda_grad*gradient); SSIM is value-only."""
    l1, g = L1GradientLoss.apply(outputs, targets)
    s, _ = ssim_loss(outputs, targets)                                                                     # :72-97
    total = l1 + lambda_grad * g + lambda_ssim * s
    return {"total": total, "pixel": l1, "gradient": g, "ssim": s}


def compute_loss_l1_grad_ssim_trained(outputs, targets, lambda_grad=0.1, lambda_ssim=0.5):
    """``compute_loss_l1_grad_ssim`` with the SSIM term attached to the graph: the same dict, the same values, and the gradient
    d(l1 + lambda_grad*gradient + lambda_ssim*ssim).  Not the reference's behaviour (it detaches the term): opt-in."""
    l1, g = L1GradientLoss.apply(outputs, targets)
    s, _ = ssim_loss(outputs, targets, differentiable=True)
    total = l1 + lambda_grad * g + lambda_ssim * s
    return {"total": total, "pixel": l1, "gradient": g, "ssim": s}


# index of every key of the reference's compute_all_loss dict in the ``terms`` of mau_loss_terms (include/mau_hip.h); 'total' is the
# l1-gradient-ssim total, because that dict is merged last (src/utils/losses.py:112-113)
ALL_LOSS_TERMS = {"total": 7, "mse": 0, "gradient": 4, "pixel": 1, "ssim": 5}
TERM_MSE_GRADIENT_TOTAL = 6


def loss_terms(outputs, targets, lambda_grad=0.1, lambda_ssim=0.5, acc=None):
    """Every loss term of the batch in ONE launch (``mau_loss_terms``, csrc/loss_terms.hip).  Returns (terms (8,) fp32, per-image
    SSIM (B,)); value only.  ``acc``: an 8-element float64 device tensor that additionally receives ``B * terms`` -- the sums of a
    validation pass stay on the device.  A batch the kernel has no SSIM for (not two channels, or smaller than the 11x11 window
    after pooling) raises ``ValueError`` before anything is launched."""
    _require_cuda(outputs, "compute_all_loss")
    o = outputs.detach().contiguous().float()
    t = targets.detach().contiguous().float()
    if o.dim() != 4 or o.shape != t.shape:
        raise ValueError(f"compute_all_loss: outputs {tuple(o.shape)} and targets {tuple(t.shape)} must be equal (B,C,H,W) shapes")
    B, C, H, W = o.shape
    n_ws = lib.mau_loss_terms_ws_elems(B, C, H, W)
    if C != 2 or n_ws == 0:
        raise ValueError(f"compute_all_loss: needs (B,2,H,W) maps of at least 11x11 pixels after SSIM pooling, got {tuple(o.shape)}")
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() < 8 or acc.device != o.device or not acc.is_contiguous()):
        raise ValueError("compute_all_loss: acc must be a contiguous float64 tensor of 8 elements on the outputs' device")
    ws = torch.empty(n_ws, dtype=torch.float64, device=o.device)
    terms = torch.empty(8, dtype=torch.float32, device=o.device)
    per_image = torch.empty(B, dtype=torch.float32, device=o.device)
    call("mau_loss_terms", o.data_ptr(), t.data_ptr(), ws.data_ptr(), _tickets(o.device).data_ptr(), terms.data_ptr(), per_image.data_ptr(),
         acc.data_ptr() if acc is not None else None, float(lambda_grad), float(lambda_ssim), B, C, H, W, _stream())
    return terms, per_image


def compute_all_loss(outputs, targets, lambda_grad=0.1, lambda_ssim=0.5, acc=None):
    """src/utils/losses.py:101-115: the dict of all loss components (total, mse, gradient, pixel, ssim), from one launch.  The values
    are 0-dim views of the kernel's ``terms`` and carry no gradient (this is what ``validate`` logs, never what is trained on)."""
    terms, _ = loss_terms(outputs, targets, lambda_grad, lambda_ssim, acc)
    return {k: terms[i] for k, i in ALL_LOSS_TERMS.items()}
