"""Shared by tests/test_image_metrics_cpu.py and tests/test_image_metrics_gpu.py: the tests' OWN statement of the SSIM recipe in torch
(reflect pad, one 121-tap grouped conv2d -- the form the reference's torchmetrics call computes) at a chosen dtype, and the test
images.  Nothing here imports the package under test."""
import torch

# What a float64 evaluation of the recipe may be off by where variances and covariance cancel exactly (constant or identical images with
# values in [0, 1]): each of E[x^2] and mu^2 carries at most 121 roundings of 2^-53 on a value <= 1, the numerator holds 2 cov and the
# denominator var_p + var_t, and the nearest thing to compare them with is c2 = 9e-4.  About 6e-11.
F64_CANCELLATION = 4 * 121 * 2.0 ** -53 / 9e-4


def ssim_map_restated(preds, target, dtype, data_range=1.0):
    """[B,3,H,W] x 2 (on the CPU) -> the SSIM map per channel [B,3,H,W] computed entirely in `dtype`"""
    p, t = preds.to(dtype), target.to(dtype)
    i = torch.arange(11, dtype=dtype) - 5
    g = torch.exp(-((i / 1.5) ** 2) / 2)
    g = g / g.sum()
    kernel = (g.reshape(11, 1) @ g.reshape(1, 11)).reshape(1, 1, 11, 11).repeat(3, 1, 1, 1)
    p = torch.nn.functional.pad(p, (5, 5, 5, 5), mode="reflect")
    t = torch.nn.functional.pad(t, (5, 5, 5, 5), mode="reflect")
    stack = torch.cat([p, t, p * p, t * t, p * t], 0)
    out = torch.nn.functional.conv2d(stack, kernel, groups=3)
    mu_p, mu_t, e_pp, e_tt, e_pt = out.chunk(5, 0)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    var_p = (e_pp - mu_p * mu_p).clamp(min=0)
    var_t = (e_tt - mu_t * mu_t).clamp(min=0)
    cov = e_pt - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))


def restated(preds, target, mask=None, dtype=torch.float64):
    """What the reference's modules give, from the restatement at `dtype`: dict of ssim_map [B,H,W] (channel mean), ssim [B], psnr [B].
    mask: None or [B,H,W]."""
    smap = ssim_map_restated(preds, target, dtype).mean(1)
    p, t = preds.to(dtype), target.to(dtype)
    w = torch.ones_like(smap) if mask is None else mask.to(dtype)
    den = w.sum((1, 2))
    ssim = (smap * w).sum((1, 2)) / den
    mse = (((p - t) ** 2) * w[:, None]).sum((2, 3)) / den[:, None]
    return {"ssim_map": smap, "ssim": ssim, "psnr": (10 * torch.log10(1.0 / mse)).mean(-1)}


def make_images(H, W, B=2, seed=5):
    """target = clamp(base), pred = clamp(target + 0.05 randn): a smooth pattern, a product ramp and a flat 0.75 channel per image, the
    images different; the LAST image's flat channel is identical in pred and target.  float32 [B,3,H,W] on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    target = torch.empty(B, 3, H, W)
    for b in range(B):
        target[b, 0] = 0.5 + 0.45 * torch.sin(0.31 * xx + 0.7 * b) * torch.cos(0.19 * yy - 0.4 * b)
        target[b, 1] = (xx + b) / (W - 1 + b) * (yy / (H - 1))
        target[b, 2] = 0.75
    target = target.clamp(0, 1)
    pred = (target + 0.05 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    pred[B - 1, 2] = target[B - 1, 2]
    return pred, target
