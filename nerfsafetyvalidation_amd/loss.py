"""Training losses (reference: loss.py): `mape_loss`, `huber_loss`, the distortion regulariser `eff_distloss`, and depth supervision
`depth_loss` (not in the reference: its composite_rays_train returns no gradient for depth).

`eff_distloss` is the O(N) form of mip-NeRF 360's distortion loss.  Per ray, with Wpre_i = sum_{j<i} w_j, WMpre_i = sum_{j<i} w_j m_j:

    L_ray = 2 sum_i w_i (m_i Wpre_i - WMpre_i) + (1/3) sum_i interval_i w_i^2            loss = sum(L_ray) / number of rays

which equals sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 interval_i when m is non-decreasing along the ray.  Nothing here checks
the order: for an unsorted m the caller gets the expression above, which is also what the reference evaluates.  Differentiable in w
only (m and interval are sample positions; the reference returns no gradient for them either):

    dL_ray / dw_i = 2 (m_i (Wpre_i - Wsuf_i) + (WMsuf_i - WMpre_i)) + (2/3) interval_i w_i

On a HIP device the scans run in libngp_hip.so (csrc/distortion.hip: one wave per ray, no atomics, the same bits on every call);
on the CPU it is the torch `cumsum` form below.  The packed-sample form the occupancy-grid training path uses is
`raymarching.distortion_rays_train`.

`depth_loss` (DESIGN.md "Depth supervision").  Take one ray with weights w_i at ray distances t_i, a target z (a ray distance in
the units of t) and a per-ray scale (None = 1; the renderer passes 1 / (far - near), as it does for the distortion term).  The target
z has three cases:

  * z == 0, or NaN, or negative: no measurement.  L_ray = 0, and every gradient row of the ray is 0.
  * 0 < z < +inf: a surface at z.
        d = sum w_i t_i        A = sum_{t_i < z - margin} w_i        L_ray = a (scale (d - z))^2 + b A
  * z == +inf: known empty ray.  A = sum w_i, and L_ray = b A.

A is the opacity the ray has accumulated before the margin in front of the surface.  It is 1 - T there.  It is bounded by 1 and does
not depend on how densely the ray was sampled.  That is why it is linear in w and not a sum of w_i^2.  The derivative with respect
to the weights is

    g_i = dL_ray / dw_i = 2 a scale^2 (d - z) t_i + b [t_i < z - margin]

and the loss is sum(L_ray) / number of rays, over all rays and not over the valid ones.  a = weight_depth, b = weight_free.
Differentiable in w only.  On a HIP device it runs in libngp_hip.so (csrc/depth_loss.hip, the scans of the distortion kernels); on the
CPU it is the torch form below.  The packed-sample form with its exact chain to sigma is `raymarching.depth_rays_train`."""
import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from . import _lib

__all__ = ["mape_loss", "huber_loss", "eff_distloss", "depth_loss"]


def _reduce(loss, reduction):
    return loss.mean() if reduction == 'mean' else loss


def mape_loss(pred, target, reduction='mean'):
    """|pred - target| / (|target| + 0.01), its mean unless `reduction` is something else"""
    return _reduce((pred - target).abs() / (target.abs() + 1e-2), reduction)


def huber_loss(pred, target, delta=0.1, reduction='mean'):
    """r = |pred - target|:  r^2 / (2 delta) up to delta, r - delta / 2 beyond; its mean unless `reduction` is something else"""
    r = (pred - target).abs()
    return _reduce(torch.where(r > delta, r - 0.5 * delta, (0.5 / delta) * r * r), reduction)


def _prefix(x):
    """exclusive cumulative sum along the last axis"""
    total = x.cumsum(dim=-1)
    return torch.cat([torch.zeros_like(total[..., :1]), total[..., :-1]], dim=-1)


def _distloss_torch(w, m, interval):
    m = m.detach()
    interval = interval.detach() if torch.is_tensor(interval) else interval
    n_rays = max(w.numel() // max(w.shape[-1], 1), 1)
    wm = w * m
    pairs = 2 * w * (m * _prefix(w) - _prefix(wm))
    own = (1 / 3) * interval * w * w
    return (pairs.sum() + own.sum()) / n_rays


class _DistLossHIP(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, w, m, interval, interval_scalar):
        T = w.shape[-1]
        w2 = w.float().contiguous().view(-1, T)
        m2 = m.float().expand_as(w).contiguous().view(-1, T)
        iv = None if interval is None else interval.float().expand_as(w).contiguous().view(-1, T)
        B, dev = w2.shape[0], w2.device
        row = torch.arange(B, dtype=torch.int32, device=dev)
        rays = torch.stack([row, row * T, torch.full_like(row, T)], dim=1).contiguous()          # the dense layout as a ray table
        loss_rays = torch.zeros(B, dtype=torch.float32, device=dev)
        totals = torch.zeros(B, 2, dtype=torch.float32, device=dev)
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        ws, nbytes = _lib.workspace("distortion", B, device=dev)
        _lib.call("distortion_forward", w2, m2, iv, float(interval_scalar), rays, B * T, B, loss_rays, totals, loss, ws, nbytes)
        ctx.save_for_backward(w2, m2, iv, rays, totals)
        ctx.interval_scalar, ctx.shape = float(interval_scalar), w.shape
        return loss

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss):
        w2, m2, iv, rays, totals = ctx.saved_tensors
        B, T = w2.shape
        grad_w = torch.empty_like(w2)               # every row belongs to a ray and every sample is live: all of it is written
        _lib.call("distortion_backward", grad_loss.float().contiguous(), w2, m2, iv, ctx.interval_scalar, rays, totals, B * T, B, grad_w)
        return grad_w.view(ctx.shape), None, None, None


def eff_distloss(w, m, interval):
    """w, m [..., N] (weights and positions of the N samples of each ray), interval a number or a tensor that broadcasts to w ->
    scalar, the mean over the rays of L_ray (module docstring).  Differentiable in w."""
    if w.is_cuda and w.numel() > 0:
        if torch.is_tensor(interval):
            return _DistLossHIP.apply(w, m, interval, 0.0)
        return _DistLossHIP.apply(w, m, None, float(interval))
    return _distloss_torch(w, m, interval)


def _depth_loss_torch(w, t, target, margin, scale, weight_depth, weight_free):
    t = t.detach().expand_as(w)
    z = target.detach().to(w.dtype).reshape(w.shape[:-1])
    n_rays = max(z.numel(), 1)
    valid = z > 0                                               # (False for NaN)
    surface = valid & ~torch.isinf(z)
    front = (t < (z - margin).unsqueeze(-1)).to(w.dtype)       # +inf: every sample; NaN: none
    d, A = (w * t).sum(dim=-1), (w * front).sum(dim=-1)
    miss = d - torch.where(surface, z, torch.zeros_like(z))
    if scale is not None:
        miss = scale.detach().to(w.dtype).reshape(z.shape) * miss
    zero = torch.zeros_like(d)
    per_ray = weight_depth * torch.where(surface, miss * miss, zero) + weight_free * torch.where(valid, A, zero)
    return per_ray.sum() / n_rays


class _DepthLossHIP(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, w, t, target, scale, margin, weight_depth, weight_free):
        T = w.shape[-1]
        w2 = w.float().contiguous().view(-1, T)
        t2 = t.float().expand_as(w).contiguous().view(-1, T)
        B, dev = w2.shape[0], w2.device
        z = target.float().contiguous().view(-1)
        sc = None if scale is None else scale.float().expand(w.shape[:-1]).contiguous().view(-1)
        if z.numel() != B:
            raise RuntimeError("depth_loss: one target per ray")
        row = torch.arange(B, dtype=torch.int32, device=dev)
        rays = torch.stack([row, row * T, torch.full_like(row, T)], dim=1).contiguous()          # the dense layout as a ray table
        loss_rays = torch.zeros(B, dtype=torch.float32, device=dev)
        parts = torch.zeros(B, 2, dtype=torch.float32, device=dev)
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        ws, nbytes = _lib.workspace("depth_loss", B, device=dev)
        _lib.call("depth_loss_forward", w2, t2, rays, z, sc, margin, weight_depth, weight_free, B * T, B, loss_rays, parts, loss, ws,
                  nbytes)
        ctx.save_for_backward(w2, t2, rays, z, sc, parts)
        ctx.consts, ctx.shape = (margin, weight_depth, weight_free), w.shape
        return loss

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss):
        w2, t2, rays, z, sc, parts = ctx.saved_tensors
        B, T = w2.shape
        grad_w = torch.zeros_like(w2)               # the rows of a ray without a measurement are not written
        _lib.call("depth_loss_backward", grad_loss.float().contiguous(), w2, t2, rays, z, sc, *ctx.consts, parts, B * T, B, grad_w)
        return grad_w.view(ctx.shape), None, None, None, None, None, None


def depth_loss(w, t, target, margin, scale=None, weight_depth=1.0, weight_free=1.0):
    """w, t [..., T] (weights and ray distances of the T samples of each ray), target [...] (0 / NaN / negative: no measurement,
    +inf: known empty, else the surface's ray distance), scale [...] or None -> scalar, the mean over ALL rays of L_ray (module
    docstring).  Differentiable in w."""
    if w.is_cuda and w.numel() > 0:
        return _DepthLossHIP.apply(w, t, target, scale, float(margin), float(weight_depth), float(weight_free))
    return _depth_loss_torch(w, t, target, margin, scale, weight_depth, weight_free)
