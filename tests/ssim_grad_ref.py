"""Host twin of ``mau_ssim_loss_grad``: d(1 - mean SSIM) / d out in closed form, in float64 on the CPU, and the differentiable torch
spelling of the same loss that autograd checks it against (``tests/_helpers.ssim_value_torch`` runs under ``no_grad``; ``ssim_loss_torch``
is that function's arithmetic, operation for operation, with the reference's channel preparation in front).

Notation: x, y the prepared, pooled planes; G the 11x11 Gaussian; s0..s4 = G*x, G*y, G*x^2, G*y^2, G*xy on the Ho x Wo map of valid
windows; sxx = s2 - s0^2, syy = s3 - s1^2, sxy = s4 - s0 s1; ld = s0^2 + s1^2 + c1, l = (2 s0 s1 + c1) / ld; cd = sxx + syy + c2,
cs = (2 sxy + c2) / cd; S = l cs.  Per map pixel
    a2 = dS/ds2 = -l cs / cd        a4 = dS/ds4 = 2 l / cd        a0 = dS/ds0 = cs (2 s1 - 2 s0 l) / ld - 2 s0 a2 - s1 a4
and per pooled pixel q
    dS/dx(q) = (G^T*a0)(q) + 2 x(q) (G^T*a2)(q) + y(q) (G^T*a4)(q)
with G^T* the transposed ("full") correlation.  Down to ``out``: times -1 / (B C Ho Wo); avg_pool2d's adjoint (1 / f^2 to every pixel of
the f x f cell, zero in the rows and columns it drops); the preparation's (channel 0: 0.5; channel 1: 1 on 0 <= out <= 1, else 0)."""
import torch
import torch.nn.functional as F

K, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def pool_factor(H, W):
    return max(1, round(min(H, W) / 256))


def window(dtype):
    c = torch.arange(K, dtype=dtype) - (K - 1) / 2.0
    g1 = torch.exp(-(c ** 2) / (2 * SIGMA ** 2))
    k = g1[:, None] * g1[None, :]
    return k / k.sum()


def prepare(v):
    """src/utils/losses.py:72-84: channel 0 -> (v + 1) / 2, channel 1 -> clamp(v, 0, 1)"""
    return torch.stack([(v[:, 0] + 1) / 2, torch.clamp(v[:, 1], 0, 1)], dim=1)


def ssim_loss_torch(out, tgt, prep=True):
    """1 - mean over images of ``ssim_value_torch(prepared out, prepared tgt)``, differentiable, in the dtype of ``out``."""
    x, y = (prepare(out), prepare(tgt)) if prep else (out, tgt)
    f = pool_factor(*x.shape[-2:])
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    C = x.shape[1]
    k = window(x.dtype)[None, None].repeat(C, 1, 1, 1)
    mu_x, mu_y = F.conv2d(x, k, groups=C), F.conv2d(y, k, groups=C)
    sxx = F.conv2d(x * x, k, groups=C) - mu_x ** 2
    syy = F.conv2d(y * y, k, groups=C) - mu_y ** 2
    sxy = F.conv2d(x * y, k, groups=C) - mu_x * mu_y
    c1, c2 = K1 ** 2, K2 ** 2
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ss = (2 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1) * cs
    return 1 - ss.mean(dim=(-1, -2)).mean(dim=1).mean()


def ssim_grad_autograd(out, tgt, prep=True, dtype=torch.float64):
    o = out.detach().to(dtype).clone().requires_grad_(True)
    ssim_loss_torch(o, tgt.detach().to(dtype), prep).backward()
    return o.grad


def ssim_grad_ref(out, tgt, prep=True, scale=1.0):
    """``scale * d ssim_loss / d out`` by the closed form of the module docstring, float64; (B, C, H, W)."""
    out, tgt = out.detach().double().cpu(), tgt.detach().double().cpu()
    B, C, H, W = out.shape
    if prep:
        assert C == 2, "the channel preparation is defined for (NDVI, temperature)"
    x, y = (prepare(out), prepare(tgt)) if prep else (out, tgt)
    f = pool_factor(H, W)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    Hd, Wd = x.shape[-2:]
    Ho, Wo = Hd - (K - 1), Wd - (K - 1)
    assert Ho > 0 and Wo > 0
    k = window(torch.float64)[None, None].repeat(C, 1, 1, 1)
    s0, s1 = F.conv2d(x, k, groups=C), F.conv2d(y, k, groups=C)
    s2, s3, s4 = F.conv2d(x * x, k, groups=C), F.conv2d(y * y, k, groups=C), F.conv2d(x * y, k, groups=C)
    c1, c2 = K1 ** 2, K2 ** 2
    sxx, syy, sxy = s2 - s0 * s0, s3 - s1 * s1, s4 - s0 * s1
    ld = s0 * s0 + s1 * s1 + c1
    l = (2 * s0 * s1 + c1) / ld
    cd = sxx + syy + c2
    cs = (2 * sxy + c2) / cd
    a2 = -l * cs / cd
    a4 = 2 * l / cd
    a0 = cs * (2 * s1 - 2 * s0 * l) / ld - 2 * s0 * a2 - s1 * a4
    full = lambda a: F.conv_transpose2d(a, k, groups=C)               # G^T*: map pixel p reaches q when 0 <= q - p <= 10
    dx = full(a0) + 2 * x * full(a2) + y * full(a4)                   # dS/dx on the pooled image
    dx = dx * (-1.0 / (B * C * Ho * Wo))
    d = torch.zeros(B, C, H, W, dtype=torch.float64)
    d[:, :, :Hd * f, :Wd * f] = dx.repeat_interleave(f, dim=2).repeat_interleave(f, dim=3) / (f * f)
    if prep:
        d[:, 0] *= 0.5
        inside = (out[:, 1] >= 0) & (out[:, 1] <= 1)                  # bounds inclusive, as torch.clamp's backward
        d[:, 1] = torch.where(inside, d[:, 1], torch.zeros_like(d[:, 1]))
    return scale * d


def make_inputs(shape, seed):
    """The inputs of the gradient tests: out[:, 0] = 0.5 N, out[:, 1] = 0.5 + 0.3 N (about 5 % outside the clamp), tgt = out + 0.2 N;
    channels beyond the second as the second."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    out = 0.5 + 0.3 * torch.randn(B, C, H, W, generator=g)
    out[:, 0] = 0.5 * torch.randn(B, H, W, generator=g)
    tgt = out + 0.2 * torch.randn(B, C, H, W, generator=g)
    return out, tgt


def make_flat_inputs(seed):
    """(1, 2, 32, 32): tgt constant (0 and 0.5), out = tgt + 1e-3 N -- variances tiny against c2, the cancellation at its worst."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.zeros(1, 2, 32, 32)
    tgt[:, 1] = 0.5
    return tgt + 1e-3 * torch.randn(1, 2, 32, 32, generator=g), tgt


def rel_max(a, ref):
    """max |a - ref| / max |ref|, in float64"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())


# (B, C, H, W), prep: the smallest shapes at which each thing can go wrong (tests/test_gpu_ssim_grad.py says which)
SHAPES = [((1, 2, 11, 11), True), ((1, 2, 12, 27), True), ((2, 2, 26, 26), True), ((2, 2, 27, 43), True), ((1, 2, 384, 384), True),
          ((1, 2, 385, 391), True), ((1, 2, 640, 640), True), ((2, 3, 20, 20), False)]
