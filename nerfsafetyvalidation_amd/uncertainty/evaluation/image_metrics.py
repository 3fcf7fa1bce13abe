"""Image metrics with masking (reference: uncertainty/evaluation/image_metrics.py): PSNRModule, SSIMModule and LPIPSModule with the
reference's signatures, over one shared function.

image_quality() returns everything both metrics need from ONE pass over the two images.  On a HIP device that pass is one
ngp_image_quality call (csrc/image_metrics.hip: window sums and the SSIM formula in double, fixed-order double sums, no
synchronisation); for tensors on the host it is the same recipe written with torch operators at the input's dtype.

The SSIM map is torchmetrics' structural_similarity_index_measure(..., data_range=1.0, return_full_image=True), which the reference
calls (image_metrics.py:119-121), stated here without that package: Gaussian window g (x) g, g[i] = exp(-(i / 1.5)^2 / 2) / sum for
i = -5..5; both images reflect-padded by 5; mu, var = max(E[x^2] - mu^2, 0) (clamped, as current torchmetrics), cov = E[pt] - mu_p mu_t
(not clamped); c1 = (0.01 range)^2, c2 = (0.03 range)^2; ssim = ((2 mu_p mu_t + c1)(2 cov + c2)) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)).

LPIPS is out of scope: its network weights are a download."""
from abc import abstractmethod

import torch
from torch import nn

from ... import _lib

_HALF_WINDOW = 5


def _window(dtype, device):
    i = torch.arange(-_HALF_WINDOW, _HALF_WINDOW + 1, dtype=dtype, device=device)
    g = torch.exp(-(i / 1.5) ** 2 / 2)
    return g / g.sum()


def _ssim_map_torch(preds, target, data_range):
    """[B,3,H,W] x 2 -> the per-channel SSIM map [B,3,H,W], torch operators at the inputs' dtype (the host path)"""
    g = _window(preds.dtype, preds.device)
    kernel = (g[:, None] * g[None, :]).expand(3, 1, -1, -1)
    pad = (_HALF_WINDOW,) * 4
    p = torch.nn.functional.pad(preds, pad, mode="reflect")
    t = torch.nn.functional.pad(target, pad, mode="reflect")
    mu_p, mu_t, e_pp, e_tt, e_pt = (torch.nn.functional.conv2d(x, kernel, groups=3) for x in (p, t, p * p, t * t, p * t))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    var_p = torch.clamp(e_pp - mu_p * mu_p, min=0.0)
    var_t = torch.clamp(e_tt - mu_t * mu_t, min=0.0)
    cov = e_pt - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))


def image_quality_stats(preds, target, mask=None, channels_last=False, return_map=False, data_range=1.0):
    """The sums of ngp_image_quality (include/ngp_hip.h) for a batch of three-channel frames.

    preds, target: [B,3,H,W], or [B,H,W,3] with channels_last (read in place either way); mask: None or weights broadcastable to
    [B,H,W] ([B,1,H,W] of the reference modules, [B,H,W,1], [B,H,W]).  Returns (stats, ssim_map): stats float64 [B,8] on the inputs'
    device -- [0] sum mask * ssim, [1] sum mask, [2:5] sum mask * err^2 per channel, [5] H * W -- and the channel-mean SSIM map
    [B,H,W] (None unless return_map).  Nothing is read back."""
    if preds.shape != target.shape or preds.dim() != 4 or preds.shape[-1 if channels_last else 1] != 3:
        raise ValueError(f"image_quality: expected two {'[B,H,W,3]' if channels_last else '[B,3,H,W]'} tensors, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if channels_last:
        preds, target = preds.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)      # views: the strides carry the layout
    B, _, H, W = preds.shape
    if H <= _HALF_WINDOW or W <= _HALF_WINDOW:
        raise ValueError(f"image_quality: the reflect pad of {_HALF_WINDOW} needs H, W > {_HALF_WINDOW} (got {H} x {W})")
    if not data_range > 0:
        raise ValueError("image_quality: data_range must be positive")
    if mask is not None:
        if mask.numel() != B * H * W:
            raise ValueError(f"image_quality: the mask has {mask.numel()} elements for {B} frames of {H} x {W}")
        mask = mask.reshape(B, H, W)

    if preds.is_cuda:
        preds, target = preds.detach(), target.detach()
        if preds.dtype != torch.float32:
            preds = preds.float()
        target = target.to(device=preds.device, dtype=torch.float32)
        if target.stride() != preds.stride():                                      # the kernel takes one set of strides for both
            preds, target = preds.contiguous(), target.contiguous()
        if mask is not None:
            mask = mask.detach().to(device=preds.device, dtype=torch.float32).contiguous()
        stats = torch.empty(B, 8, dtype=torch.float64, device=preds.device)
        work, wbytes = _lib.workspace("image_quality", B, H, W, device=preds.device)
        if work is None:              # a frame size the library refuses: a buffer all the same, so that its message names the reason
            work = torch.empty(8, dtype=torch.uint8, device=preds.device)
        ssim_map = torch.empty(B, H, W, dtype=torch.float32, device=preds.device) if return_map else None
        sb, sc, sy, sx = preds.stride()
        with torch.cuda.device(preds.device):
            _lib.call("image_quality", preds.data_ptr(), target.data_ptr(), mask, B, H, W, sb, sc, sy, sx, float(data_range), ssim_map,
                      stats, work, wbytes)
        return stats, ssim_map

    # host tensors: the same recipe with torch operators at the inputs' dtype
    if not preds.is_floating_point():
        preds = preds.float()
    target = target.to(preds.dtype)
    with torch.no_grad():
        ssim_map = _ssim_map_torch(preds, target, data_range).mean(1)
        weights = torch.ones_like(ssim_map) if mask is None else mask.to(preds.dtype)
        err = ((preds - target) ** 2 * weights[:, None]).sum((2, 3))
        stats = torch.zeros(B, 8, dtype=torch.float64)
        stats[:, 0] = (ssim_map * weights).sum((1, 2))
        stats[:, 1] = weights.sum((1, 2))
        stats[:, 2:5] = err
        stats[:, 5] = H * W
    return stats, (ssim_map if return_map else None)


def image_quality(preds, target, mask=None, channels_last=False, return_map=False, data_range=1.0):
    """PSNR and SSIM of a batch of frames from one pass (one ngp_image_quality launch on a HIP device), as a dict of tensors on the
    inputs' device, float64, without a synchronisation:
        ssim [B]     sum mask * map / sum mask, map = the SSIM map averaged over the channels   (image_metrics.py:119-135)
        psnr [B]     mean over the channels of 10 log10(1 / mse_c)                              (image_metrics.py:88-104)
        mse  [B,3]   sum mask * err^2 / sum mask per channel
        ssim_map [B,H,W]   only with return_map (float32 from the kernel, the inputs' dtype on the host)
    An all-zero mask gives the reference's 0 / 0: NaN."""
    stats, ssim_map = image_quality_stats(preds, target, mask, channels_last, return_map, data_range)
    mse = stats[:, 2:5] / stats[:, 1:2]
    out = {"ssim": stats[:, 0] / stats[:, 1], "psnr": (10 * torch.log10(1.0 / mse)).mean(-1), "mse": mse}
    if return_map:
        out["ssim_map"] = ssim_map
    return out


class ImageMetricModule(nn.Module):
    """Computes image metrics with masking capabilities.  preds and target are [bs,3,H,W] in [0, 1]; mask, when given, is [bs,1,H,W]
    (weights, not only 0 / 1) and restricts the metric to where it is non-zero.  Returns [bs] in preds' dtype."""

    def __init__(self):
        super().__init__()
        self.populate_modules()

    def populate_modules(self):
        """Populates the modules that will be used to compute the metric."""

    @abstractmethod
    def forward(self, preds, target, mask=None):
        """preds [bs,3,H,W], target [bs,3,H,W], mask [bs,1,H,W] or None -> [bs]"""


def _out_dtype(preds):
    return preds.dtype if preds.is_floating_point() else torch.float32


class PSNRModule(ImageMetricModule):
    """PSNR per channel from the masked MSE, then the mean over the three channels (image_metrics.py:79-104)."""

    def forward(self, preds, target, mask=None):
        return image_quality(preds, target, mask)["psnr"].to(_out_dtype(preds))


class SSIMModule(ImageMetricModule):
    """Channel mean of the SSIM map, then sum map * mask / sum mask (image_metrics.py:107-135)."""

    def forward(self, preds, target, mask=None):
        return image_quality(preds, target, mask)["ssim"].to(_out_dtype(preds))


class LPIPSModule(ImageMetricModule):
    """Not ported: LPIPS needs the pretrained weights of its feature network (torchmetrics downloads them), and there is no offline
    source for them."""

    def forward(self, preds, target, mask=None):
        raise NotImplementedError("LPIPSModule: the LPIPS network's pretrained weights are a download that this package does not ship; "
                                  "PSNRModule and SSIMModule are available")
