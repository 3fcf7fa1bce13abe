"""Training losses (reference: loss.py): `mape_loss`, `huber_loss` and the distortion regulariser `eff_distloss`.

`eff_distloss` is the O(N) form of mip-NeRF 360's distortion loss.  Per ray, with Wpre_i = sum_{j<i} w_j, WMpre_i = sum_{j<i} w_j m_j:

    L_ray = 2 sum_i w_i (m_i Wpre_i - WMpre_i) + (1/3) sum_i interval_i w_i^2            loss = sum(L_ray) / number of rays

which equals sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 interval_i when m is non-decreasing along the ray.  Nothing here checks
the order: for an unsorted m the caller gets the expression above, which is also what the reference evaluates.  Differentiable in w
only (m and interval are sample positions; the reference returns no gradient for them either):

    dL_ray / dw_i = 2 (m_i (Wpre_i - Wsuf_i) + (WMsuf_i - WMpre_i)) + (2/3) interval_i w_i

On a HIP device the scans run in libngp_hip.so (csrc/distortion.hip: one wave per ray, no atomics, the same bits on every call);
on the CPU it is the torch `cumsum` form below.  The packed-sample form the occupancy-grid training path uses is
`raymarching.distortion_rays_train`."""
import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from . import _lib

__all__ = ["mape_loss", "huber_loss", "eff_distloss"]


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
        L = _lib.lib()
        nbytes = L.ngp_distortion_workspace(B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(L.ngp_distortion_forward(_lib.ptr(w2), _lib.ptr(m2), _lib.ptr(iv), float(interval_scalar), _lib.ptr(rays), B * T, B,
                                            _lib.ptr(loss_rays), _lib.ptr(totals), _lib.ptr(loss), _lib.ptr(ws), nbytes, _lib.stream()),
                   "distortion_forward")
        ctx.save_for_backward(w2, m2, iv, rays, totals)
        ctx.interval_scalar, ctx.shape = float(interval_scalar), w.shape
        return loss

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss):
        w2, m2, iv, rays, totals = ctx.saved_tensors
        B, T = w2.shape
        grad_w = torch.empty_like(w2)               # every row belongs to a ray and every sample is live: all of it is written
        _lib.check(_lib.lib().ngp_distortion_backward(_lib.ptr(grad_loss.float().contiguous()), _lib.ptr(w2), _lib.ptr(m2), _lib.ptr(iv),
                                                      ctx.interval_scalar, _lib.ptr(rays), _lib.ptr(totals), B * T, B, _lib.ptr(grad_w),
                                                      _lib.stream()), "distortion_backward")
        return grad_w.view(ctx.shape), None, None, None


def eff_distloss(w, m, interval):
    """w, m [..., N] (weights and positions of the N samples of each ray), interval a number or a tensor that broadcasts to w ->
    scalar, the mean over the rays of L_ray (module docstring).  Differentiable in w."""
    if w.is_cuda and w.numel() > 0:
        if torch.is_tensor(interval):
            return _DistLossHIP.apply(w, m, interval, 0.0)
        return _DistLossHIP.apply(w, m, None, float(interval))
    return _distloss_torch(w, m, interval)
