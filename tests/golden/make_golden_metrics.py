#!/usr/bin/env python3
"""Generates tests/golden/image_metrics.npz by running the REFERENCE's own PSNRModule and SSIMModule
(uncertainty/evaluation/image_metrics.py) on CPU in float64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

The reference module is imported from /root/reference unmodified.  Three packages it imports are not installed where this runs and
are replaced IN MEMORY by stand-ins: torchtyping (annotations only), torchmetrics.image.lpip (base class of the LPIPS wrapper, never
instantiated here) and torchmetrics.functional.  The stand-in for structural_similarity_index_measure is THIS script's float64
statement of the definition in include/ngp_hip.h (reflect pad 5, 11 x 11 Gaussian window of sigma 1.5 as one grouped convolution,
clamped variances, c1 = 0.01^2, c2 = 0.03^2).

What the fixture therefore pins is the reference's MASKING AND AVERAGING -- PSNR per channel from the masked MSE and then the channel
mean; the channel mean of the SSIM map and then sum(map * mask / sum(mask)) -- not the SSIM core, which torchmetrics would supply and
which is pinned by the closed forms and the float64 restatement in tests/test_image_metrics_*.py.  Nothing of the reference is copied:
the file holds the inputs (float32), the masks and the modules' float64 outputs, arrays only."""
import importlib.util
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, H, W = 2, 17, 23
SEED = 11


def ssim_full_image_f64(preds, target, data_range=1.0):
    """[B,3,H,W] -> the per-channel SSIM map [B,3,H,W], float64"""
    p, t = preds.double(), target.double()
    i = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-(i / 1.5) ** 2 / 2)
    g = g / g.sum()
    kernel = torch.outer(g, g).expand(3, 1, 11, 11)
    pp = torch.nn.functional.pad(p, (5, 5, 5, 5), mode="reflect")
    tp = torch.nn.functional.pad(t, (5, 5, 5, 5), mode="reflect")
    mu_p, mu_t, e_pp, e_tt, e_pt = (torch.nn.functional.conv2d(x, kernel, groups=3) for x in (pp, tp, pp * pp, tp * tp, pp * tp))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    var_p, var_t = torch.clamp(e_pp - mu_p ** 2, min=0.0), torch.clamp(e_tt - mu_t ** 2, min=0.0)
    cov = e_pt - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p ** 2 + mu_t ** 2 + c1) * (var_p + var_t + c2))


def _stand_ins():
    class _Subscriptable:
        def __class_getitem__(cls, item):
            return cls

    tt = types.ModuleType("torchtyping")
    tt.TensorType = _Subscriptable
    tm = types.ModuleType("torchmetrics")
    fn = types.ModuleType("torchmetrics.functional")
    seen = []

    def structural_similarity_index_measure(preds, target, reduction="none", data_range=1.0, return_full_image=False):
        assert reduction == "none" and data_range == 1.0 and return_full_image      # the one call the reference makes (:119-121)
        seen.append(tuple(preds.shape))
        full = ssim_full_image_f64(preds, target, data_range)
        return full.mean((1, 2, 3)), full

    fn.structural_similarity_index_measure = structural_similarity_index_measure
    image = types.ModuleType("torchmetrics.image")
    lpip = types.ModuleType("torchmetrics.image.lpip")
    lpip.LearnedPerceptualImagePatchSimilarity = type("LearnedPerceptualImagePatchSimilarity", (torch.nn.Module,), {})
    tm.functional, tm.image, image.lpip = fn, image, lpip
    mods = {"torchtyping": tt, "torchmetrics": tm, "torchmetrics.functional": fn, "torchmetrics.image": image, "torchmetrics.image.lpip": lpip}
    for name in mods:
        assert name not in sys.modules, f"{name} is installed: run the reference against it instead of the stand-in"
    sys.modules.update(mods)
    return seen


def main():
    seen = _stand_ins()
    spec = importlib.util.spec_from_file_location("ref_image_metrics", os.path.join(REF, "uncertainty", "evaluation", "image_metrics.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    gen = torch.Generator().manual_seed(SEED)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    target = torch.empty(B, 3, H, W)
    for b in range(B):
        target[b, 0] = 0.5 + 0.4 * torch.sin(0.37 * xx + 0.3 * b) * torch.cos(0.23 * yy)
        target[b, 1] = (xx / (W - 1)) * (yy / (H - 1))
        target[b, 2] = 0.75 - 0.25 * b
    target = target.clamp(0, 1)
    preds = (target + 0.05 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)
    mask_binary = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float()
    mask_weights = torch.rand(B, 1, H, W, generator=gen)
    assert mask_binary.sum((1, 2, 3)).min() > 0

    psnr, ssim = ref.PSNRModule(), ref.SSIMModule()
    out = {}
    p64, t64 = preds.double(), target.double()
    for tag, mask in (("none", None), ("binary", mask_binary.double()), ("weights", mask_weights.double())):
        out[f"psnr_{tag}"] = psnr(p64, t64, mask).numpy()
        out[f"ssim_{tag}"] = ssim(p64, t64, mask).numpy()
        assert out[f"psnr_{tag}"].dtype == np.float64 and out[f"psnr_{tag}"].shape == (B,) and np.isfinite(out[f"psnr_{tag}"]).all()
        assert out[f"ssim_{tag}"].dtype == np.float64 and out[f"ssim_{tag}"].shape == (B,)
    assert seen == [(B, 3, H, W)] * 3
    path = os.path.join(HERE, "image_metrics.npz")
    np.savez_compressed(path, preds=preds.numpy(), target=target.numpy(), mask_binary=mask_binary.numpy(), mask_weights=mask_weights.numpy(), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
