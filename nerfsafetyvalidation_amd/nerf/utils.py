"""Ray generation and the small helpers the render path uses (reference: nerf/utils.py:31-124,185-219).

get_rays keeps the reference's signature and result dict.  The full-frame branch (N <= 0) and
the explicit-pixel branch run in one HIP kernel (ngp_get_rays); random pixel selection
(N > 0) draws the indices with torch exactly as the reference does and feeds them to the same
kernel, so the Estimator's <=1024-pixel batches no longer build a full 800x800 ray grid."""
import os
import random

import numpy as np
import torch

from .. import _lib


def custom_meshgrid(*args):
    return torch.meshgrid(*args, indexing="ij")


def linear_to_srgb(x):
    """nerf/utils.py:42-44"""
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)


def srgb_to_linear(x):
    """nerf/utils.py:47-49"""
    return torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


class _RaysKernel(torch.autograd.Function):
    """ngp_get_rays with its vector-Jacobian product: the reference builds rays with differentiable torch ops
    (utils.py:103-111) and the Estimator / Planner differentiate through them with respect to the pose."""

    @staticmethod
    def forward(ctx, poses, intrinsics, H, W, inds):
        poses = poses.float().contiguous()
        B = poses.shape[0]
        fx, fy, cx, cy = [float(v) for v in intrinsics]
        n_pix = H * W if inds is None else inds.shape[0]
        rays_o = torch.empty(B, n_pix, 3, dtype=torch.float32, device=poses.device)
        rays_d = torch.empty(B, n_pix, 3, dtype=torch.float32, device=poses.device)
        _lib.call("get_rays", poses, B, fx, fy, cx, cy, H, W, inds, n_pix, rays_o, rays_d)
        ctx.geom = (B, fx, fy, cx, cy, H, W, n_pix)
        ctx.inds = inds
        return rays_o, rays_d

    @staticmethod
    def backward(ctx, grad_o, grad_d):
        B, fx, fy, cx, cy, H, W, n_pix = ctx.geom
        go = None if grad_o is None else grad_o.float().contiguous()
        gd = None if grad_d is None else grad_d.float().contiguous()
        ref = go if go is not None else gd
        grad_poses = torch.empty(B, 4, 4, dtype=torch.float32, device=ref.device)
        _lib.call("get_rays_backward", go, gd, B, fx, fy, cx, cy, H, W, ctx.inds, n_pix, grad_poses)
        return grad_poses, None, None, None, None


def _rays_torch(poses, intrinsics, H, W, inds):
    """the reference's own formulas (utils.py:69-71, 95-111), for poses on the HOST: a dataset served on a CPU device (NeRFDataset /
    Trainer bookkeeping without a GPU).  Nothing on a HIP device comes here."""
    fx, fy, cx, cy = intrinsics
    pix = torch.arange(H * W, device=poses.device) if inds is None else inds.long()
    i = (pix % W).float() + 0.5
    j = torch.div(pix, W, rounding_mode="floor").float() + 0.5
    zs = torch.ones_like(i)
    directions = torch.stack(((i - cx) / fx * zs, (j - cy) / fy * zs, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions.expand(poses.shape[0], -1, 3) @ poses[:, :3, :3].transpose(-1, -2)
    return poses[..., None, :3, 3].expand_as(rays_d), rays_d


def _rays_kernel(poses, intrinsics, H, W, inds):
    """poses [B,4,4] -> rays_o, rays_d [B, n_pix, 3] for pixel ids `inds` (int32 [n_pix], shared by all cameras) or all pixels."""
    if not poses.is_cuda:
        return _rays_torch(poses, intrinsics, H, W, inds)
    return _RaysKernel.apply(poses, intrinsics, H, W, inds)


def get_rays(poses, intrinsics, H, W, N=-1, error_map=None, inds=None):
    """poses [B,4,4] cam2world, intrinsics (fx,fy,cx,cy) -> {'rays_o','rays_d' [B,N,3], ('inds' [B,N])}.

    `inds` (extension): explicit flat pixel ids [n] shared by all cameras; generates only those rays.

    Runs with autocast disabled, as the reference's decorator does (nerf/utils.py:52).  A context manager per CALL, not the
    decorator: `@torch.autocast(...)` wraps every call in ONE shared context object whose saved `prev` state the threads of a frame
    pipeline overwrite for each other -- a thread inside its own autocast block then leaves get_rays with autocast switched off
    (found by scripts/fuzz_training.py: the viewer thread's next render raised in the FFMLP)."""
    with torch.autocast("cuda", enabled=False):
        return _get_rays(poses, intrinsics, H, W, N, error_map, inds)


def _get_rays(poses, intrinsics, H, W, N, error_map, inds):
    device = poses.device
    B = poses.shape[0]
    results = {}
    if inds is not None:
        inds32 = inds.to(device=device, dtype=torch.int32).contiguous().view(-1)
        rays_o, rays_d = _rays_kernel(poses, intrinsics, H, W, inds32)
        results["inds"] = inds32.long().expand([B, inds32.shape[0]])
    elif N > 0:
        N = min(N, H * W)
        if error_map is None:
            sel = torch.randint(0, H * W, size=[N], device=device)  # may duplicate (utils.py:77)
            rays_o, rays_d = _rays_kernel(poses, intrinsics, H, W, sel.int().contiguous())
            results["inds"] = sel.expand([B, N])
        else:
            # per-camera weighted sampling on the 128x128 error map (utils.py:81-93): pixel ids differ per camera
            inds_coarse = torch.multinomial(error_map.to(device), N, replacement=False)
            inds_x, inds_y = inds_coarse // 128, inds_coarse % 128
            sx, sy = H / 128, W / 128
            inds_x = (inds_x * sx + torch.rand(B, N, device=device) * sx).long().clamp(max=H - 1)
            inds_y = (inds_y * sy + torch.rand(B, N, device=device) * sy).long().clamp(max=W - 1)
            sel = inds_x * W + inds_y
            ro, rd = [], []
            for b in range(B):
                o, d = _rays_kernel(poses[b:b + 1], intrinsics, H, W, sel[b].int().contiguous())
                ro.append(o)
                rd.append(d)
            rays_o, rays_d = torch.cat(ro, 0), torch.cat(rd, 0)
            results["inds_coarse"] = inds_coarse
            results["inds"] = sel
    else:
        rays_o, rays_d = _rays_kernel(poses, intrinsics, H, W, None)
    results["rays_o"] = rays_o
    results["rays_d"] = rays_d
    return results


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


class PSNRMeter:
    """nerf/utils.py:185-219"""

    def __init__(self):
        self.V = 0
        self.N = 0

    def clear(self):
        self.V = 0
        self.N = 0

    def prepare_inputs(self, *inputs):
        outputs = []
        for inp in inputs:
            if torch.is_tensor(inp):
                inp = inp.detach().cpu().numpy()
            outputs.append(inp)
        return outputs

    def update(self, preds, truths):
        preds, truths = self.prepare_inputs(preds, truths)
        psnr = -10 * np.log10(np.mean((preds - truths) ** 2))
        self.V += psnr
        self.N += 1

    def measure(self):
        return self.V / self.N

    def report(self):
        return f"PSNR = {self.measure():.6f}"


class SSIMMeter:
    """Mean SSIM over the evaluated frames, next to PSNRMeter in a Trainer's metric list.  Every update is one pass over the two frames
    (uncertainty/evaluation/image_metrics.py::image_quality_stats: one ngp_image_quality launch on a HIP device) whose sums stay on the
    device; measure() is the one read-back.  The same pass yields the squared error, so measure_psnr() gives PSNRMeter's number
    (-10 log10 of the mean over all channels of an update, averaged over the updates) without the per-frame copy to the host."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.V = 0          # sum of the per-frame SSIM (a 0-dim float64 tensor after the first update)
        self.N = 0          # frames
        self.P = 0          # sum of the per-update PSNR
        self.U = 0          # updates

    def update(self, preds, truths):
        """preds, truths: [B,H,W,3] in [0, 1] (tensors or numpy arrays).  Whole frames only: SSIM has no meaning for the [B,N,3] ray
        batches of a training step, which raise."""
        from ..uncertainty.evaluation.image_metrics import image_quality_stats
        preds, truths = torch.as_tensor(preds), torch.as_tensor(truths)
        stats, _ = image_quality_stats(preds, truths.to(preds.device), channels_last=True)
        self.V = self.V + (stats[:, 0] / stats[:, 1]).sum()
        self.N += stats.shape[0]
        self.P = self.P - 10 * torch.log10(stats[:, 2:5].sum() / (3 * stats[:, 5].sum()))
        self.U += 1

    def measure(self):
        return float(self.V) / self.N

    def measure_psnr(self):
        return float(self.P) / self.U

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "SSIM"), self.measure(), global_step)

    def report(self):
        return f"SSIM = {self.measure():.6f}"
