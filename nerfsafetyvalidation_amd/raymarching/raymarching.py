"""`raymarching` operator API on MI355X.

Same public names, argument order, defaults, output shapes and in-place behaviour
as the reference's raymarching/raymarching.py:19-362; the native calls go to
libngp_hip.so (include/ngp_hip.h) through ctypes on torch's current stream.

Deliberate, documented differences that are invisible to callers:
  * march_rays_train allocates ray slots by a prefix sum in ray order (a fixed
    member of the reference's atomicAdd permutation set);
  * march_rays' kernel zero-fills unused slots itself, so the wrapper allocates
    with torch.empty (the reference does torch.zeros + kernel, :328-330);
  * march_rays keeps derived copies of the occupancy bits (0.5 MB for 128^3 x 2),
    rebuilt when the bitfield tensor's version changes (ngp_march_rays_lin).
"""
import collections
import threading
import weakref

import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from .. import _lib

__all__ = ["near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "march_rays_train",
           "composite_rays_train", "distortion_rays_train", "depth_rays_train", "march_rays", "composite_rays"]

USE_OCCUPANCY_LIN = True        # march_rays keeps derived copies of the occupancy bits per bitfield version (False: the plain kernel, for A/B)

_fwd32 = custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd = custom_bwd(device_type="cuda")


def _dev(t):
    return t if t.is_cuda else t.cuda()


def _rays(rays_o, rays_d):
    return _dev(rays_o).contiguous().view(-1, 3), _dev(rays_d).contiguous().view(-1, 3)


# ---------------------------------------------------------------- utils
class _near_far_from_aabb(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, rays_o, rays_d, aabb, min_near=0.2):
        """raymarching.py:19-47.  rays_o/d [N,3], aabb [6] -> nears [N], fars [N]."""
        rays_o, rays_d = _rays(rays_o, rays_d)
        aabb = _dev(aabb).contiguous()
        N = rays_o.shape[0]
        nears = torch.empty(N, dtype=rays_o.dtype, device=rays_o.device)
        fars = torch.empty(N, dtype=rays_o.dtype, device=rays_o.device)
        _lib.call("near_far_from_aabb", rays_o, rays_d, aabb, N, min_near, nears, fars)
        return nears, fars


near_far_from_aabb = _near_far_from_aabb.apply


class _sph_from_ray(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, rays_o, rays_d, radius):
        """raymarching.py:52-79.  -> coords [N,2] in [-1,1]"""
        rays_o, rays_d = _rays(rays_o, rays_d)
        N = rays_o.shape[0]
        coords = torch.empty(N, 2, dtype=rays_o.dtype, device=rays_o.device)
        _lib.call("sph_from_ray", rays_o, rays_d, radius, N, coords)
        return coords


sph_from_ray = _sph_from_ray.apply


class _morton3D(Function):
    @staticmethod
    def forward(ctx, coords):
        """raymarching.py:84-102.  coords int32 [N,3] -> indices int32 [N]"""
        coords = _dev(coords).int().contiguous()
        N = coords.shape[0]
        indices = torch.empty(N, dtype=torch.int32, device=coords.device)
        _lib.call("morton3D", coords, N, indices)
        return indices


morton3D = _morton3D.apply


class _morton3D_invert(Function):
    @staticmethod
    def forward(ctx, indices):
        """raymarching.py:106-124.  indices int32 [N] -> coords int32 [N,3]"""
        indices = _dev(indices).int().contiguous()
        N = indices.shape[0]
        coords = torch.empty(N, 3, dtype=torch.int32, device=indices.device)
        _lib.call("morton3D_invert", indices, N, coords)
        return coords


morton3D_invert = _morton3D_invert.apply


class _packbits(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, grid, thresh, bitfield=None):
        """raymarching.py:129-154.  grid [C, H^3] -> bitfield uint8 [C*H^3/8]"""
        grid = _dev(grid).contiguous()
        C, H3 = grid.shape[0], grid.shape[1]
        N = C * H3 // 8
        wrote = () if bitfield is None else (bitfield,)
        if bitfield is None:
            bitfield = torch.empty(N, dtype=torch.uint8, device=grid.device)
        _lib.call("packbits", grid, N, thresh, bitfield, wrote=wrote)
        return bitfield


packbits = _packbits.apply


# ---------------------------------------------------------------- train
class _march_rays_train(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, step_counter=None, mean_count=-1,
                perturb=False, align=-1, force_all_rays=False, dt_gamma=0, max_steps=1024):
        """raymarching.py:161-228.  -> xyzs [M,3], dirs [M,3], deltas [M,2], rays int32 [N,3] (idx, offset, count)"""
        rays_o, rays_d = _rays(rays_o, rays_d)
        density_bitfield = _dev(density_bitfield).contiguous()
        N = rays_o.shape[0]
        M = N * max_steps
        if not force_all_rays and mean_count > 0:
            if align > 0:
                mean_count += align - mean_count % align
            M = mean_count
        dev, dt = rays_o.device, rays_o.dtype
        # unwritten rows must read as zero (rays past capacity are dropped, raymarching.cu:421)
        xyzs = torch.zeros(M, 3, dtype=dt, device=dev)
        dirs = torch.zeros(M, 3, dtype=dt, device=dev)
        deltas = torch.zeros(M, 2, dtype=dt, device=dev)
        rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
        wrote = () if step_counter is None else (step_counter,)
        if step_counter is None:
            step_counter = torch.zeros(2, dtype=torch.int32, device=dev)
        ws, ws_bytes = _lib.workspace("march_rays_train", N, device=dev)
        _lib.call("march_rays_train", rays_o, rays_d, density_bitfield, bound, dt_gamma, max_steps, N, C, H, M, nears.contiguous(),
                  fars.contiguous(), xyzs, dirs, deltas, rays, step_counter, int(perturb), ws, ws_bytes, wrote=wrote)
        if force_all_rays or mean_count <= 0:
            m = step_counter[0].item()  # D2H sync, as in the reference (:219)
            if align > 0:
                m += align - m % align  # F11: adds a full `align` when already aligned
            xyzs, dirs, deltas = xyzs[:m], dirs[:m], deltas[:m]
        return xyzs, dirs, deltas, rays


march_rays_train = _march_rays_train.apply


class _composite_rays_train(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, sigmas, rgbs, deltas, rays):
        """raymarching.py:233-262.  -> weights_sum [N], depth [N], image [N,3]; differentiable in sigmas, rgbs"""
        # the kernels are fp32 ("scalar_t should always be float in use", raymarching.cu:95)
        sigmas, rgbs, deltas = sigmas.float().contiguous(), rgbs.float().contiguous(), deltas.float().contiguous()
        rays = rays.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        weights_sum = torch.empty(N, dtype=sigmas.dtype, device=sigmas.device)
        depth = torch.empty(N, dtype=sigmas.dtype, device=sigmas.device)
        image = torch.empty(N, 3, dtype=sigmas.dtype, device=sigmas.device)
        _lib.call("composite_rays_train_forward", sigmas, rgbs, deltas, rays, M, N, weights_sum, depth, image)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image)
        ctx.dims = [M, N]
        return weights_sum, depth, image

    @staticmethod
    @_bwd
    def backward(ctx, grad_weights_sum, grad_depth, grad_image):
        # grad_depth is ignored, exactly as in the reference (:267)
        grad_weights_sum, grad_image = grad_weights_sum.contiguous(), grad_image.contiguous()
        sigmas, rgbs, deltas, rays, weights_sum, depth, image = ctx.saved_tensors
        M, N = ctx.dims
        grad_sigmas, grad_rgbs = torch.zeros_like(sigmas), torch.zeros_like(rgbs)
        _lib.call("composite_rays_train_backward", grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N,
                  grad_sigmas, grad_rgbs)
        return grad_sigmas, grad_rgbs, None, None


composite_rays_train = _composite_rays_train.apply


class _distortion_rays_train(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, sigmas, deltas, rays, scale):
        sigmas, deltas, rays = sigmas.float().contiguous(), deltas.float().contiguous(), rays.contiguous()
        scale = None if scale is None else scale.float().contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        loss_rays = torch.zeros(N, dtype=sigmas.dtype, device=sigmas.device)
        totals = torch.zeros(N, 2, dtype=sigmas.dtype, device=sigmas.device)
        loss = torch.zeros((), dtype=sigmas.dtype, device=sigmas.device)
        ws, ws_bytes = _lib.workspace("distortion", N, device=sigmas.device)
        _lib.call("distortion_train_forward", sigmas, deltas, rays, scale, M, N, loss_rays, totals, loss, ws, ws_bytes)
        ctx.save_for_backward(sigmas, deltas, rays, scale, totals)
        ctx.dims = [M, N]
        ctx.mark_non_differentiable(loss_rays)
        return loss, loss_rays

    @staticmethod
    @_bwd
    def backward(ctx, grad_loss, _grad_loss_rays):
        sigmas, deltas, rays, scale, totals = ctx.saved_tensors
        M, N = ctx.dims
        grad_sigmas = torch.zeros_like(sigmas)      # rows of dead samples, of dropped rays and of no ray read 0
        _lib.call("distortion_train_backward", grad_loss.float().contiguous(), sigmas, deltas, rays, scale, totals, M, N, grad_sigmas)
        return grad_sigmas, None, None, None


def distortion_rays_train(sigmas, deltas, rays, scale=None, return_rays=False):
    """The distortion regulariser (mip-NeRF 360) on march_rays_train's packed samples -> scalar, differentiable in sigmas.

    sigmas [M], deltas [M,2] = (dt, gap), rays int32 [N,3] = (index, offset, count), scale [N] per ray slot (None = 1; the renderer
    passes 1 / (far - near)).  Per ray, with alpha_i = 1 - exp(-sigma_i dt_i), T_{i+1} = T_i (1 - alpha_i), w_i = alpha_i T_i,
    m_i = scale * (gap_0 + ... + gap_i), delta_i = scale * dt_i:
        L_ray = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
    over the samples up to and including the first with T_{i+1} < 1e-4 (composite_rays_train's forward rule); rays with no samples or
    with offset + count >= M are dropped as composite_rays_train drops them.  The result is sum(L_ray) / N over ALL N rows of the table.

    The gradient is the exact derivative for every live sample, the one that stops the ray INCLUDED -- unlike
    composite_rays_train's backward, which writes no gradient for that sample.  Dead samples and dropped rays get 0.
    One HIP launch per direction plus the fixed-order mean: no atomics, the same bits on every call (csrc/distortion.hip).
    return_rays: also return L_ray per slot [N] (not differentiable)."""
    if rays.shape[0] == 0:
        loss, loss_rays = sigmas.float().sum() * 0, sigmas.new_zeros(0, dtype=torch.float32)
    else:
        loss, loss_rays = _distortion_rays_train.apply(sigmas, deltas, rays, scale)
    return (loss, loss_rays) if return_rays else loss


class _depth_rays_train(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, sigmas, deltas, rays, target, scale, margin, weight_depth, weight_free):
        sigmas, deltas, rays = sigmas.float().contiguous(), deltas.float().contiguous(), rays.contiguous()
        target = target.float().contiguous()
        scale = None if scale is None else scale.float().contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        if target.numel() != N or (scale is not None and scale.numel() != N):
            raise RuntimeError("depth_rays_train: target and scale hold one value per ray slot")
        loss_rays = torch.zeros(N, dtype=sigmas.dtype, device=sigmas.device)
        parts = torch.zeros(N, 2, dtype=sigmas.dtype, device=sigmas.device)
        loss = torch.zeros((), dtype=sigmas.dtype, device=sigmas.device)
        ws, nbytes = _lib.workspace("depth_loss", N, device=sigmas.device)
        _lib.call("depth_loss_train_forward", sigmas, deltas, rays, target, scale, margin, weight_depth, weight_free, M, N, loss_rays,
                  parts, loss, ws, nbytes)
        ctx.save_for_backward(sigmas, deltas, rays, target, scale, parts)
        ctx.dims, ctx.consts = [M, N], (margin, weight_depth, weight_free)
        ctx.mark_non_differentiable(loss_rays, parts)
        return loss, loss_rays, parts

    @staticmethod
    @_bwd
    def backward(ctx, grad_loss, _grad_loss_rays, _grad_parts):
        sigmas, deltas, rays, target, scale, parts = ctx.saved_tensors
        M, N = ctx.dims
        grad_sigmas = torch.zeros_like(sigmas)      # rows of dead samples, of rays that take no part and of no ray read 0
        _lib.call("depth_loss_train_backward", grad_loss.float().contiguous(), sigmas, deltas, rays, target, scale, *ctx.consts, parts, M,
                  N, grad_sigmas)
        return grad_sigmas, None, None, None, None, None, None, None


def depth_rays_train(sigmas, deltas, rays, target, margin, scale=None, weight_depth=1.0, weight_free=1.0, return_rays=False):
    """Depth supervision on march_rays_train's packed samples -> scalar, differentiable in sigmas (csrc/depth_loss.hip).

    sigmas [M], deltas [M,2] = (dt, gap), rays int32 [N,3] = (index, offset, count), target [N] and scale [N] per ray slot (scale
    None = 1; the renderer passes 1 / (far - near)).  The composite rule is distortion_rays_train's, and so are the stop
    (T_{i+1} < 1e-4, that sample included) and the drop rule (offset + count >= M); t_i = gap_0 + ... + gap_i.  With z = target[index],
    a = weight_depth, b = weight_free (`loss.py` has the same definitions for dense weights):
        z == 0, NaN or negative   no measurement: L_ray = 0, no gradient
        0 < z < +inf              d = sum w_i t_i,  A = sum_{t_i < z - margin} w_i,  L_ray = a (scale (d - z))^2 + b A
        z == +inf                 known empty ray: A = sum w_i,  L_ray = b A
    The result is sum(L_ray) / N over ALL N rows of the table.  The gradient is exact for every live sample, the one that stops the
    ray included.  No atomics: the same bits on every call and for every order of the table's rows.
    return_rays: also return L_ray [N] and parts [N,2] = (d, A) per slot (not differentiable)."""
    if rays.shape[0] == 0:
        loss = sigmas.float().sum() * 0
        loss_rays, parts = sigmas.new_zeros(0, dtype=torch.float32), sigmas.new_zeros(0, 2, dtype=torch.float32)
    else:
        loss, loss_rays, parts = _depth_rays_train.apply(sigmas, deltas, rays, target, scale, float(margin), float(weight_depth),
                                                         float(weight_free))
    return (loss, loss_rays, parts) if return_rays else loss


# ---------------------------------------------------------------- inference
# Derived copies of the occupancy bits for ngp_march_rays_lin (the reference's loop calls march_rays once per iteration, dozens of times per
# frame, with the same bitfield): built once per (bitfield TENSOR OBJECT, its version, stream) and dropped least-recently-used.  The entry
# holds a weak reference to the tensor: another tensor that happens to get a freed one's address (and version 0) is not mistaken for it.
# A stream's copy is written and read on that stream only, so no cross-stream ordering is needed.
_OCC_LIN = collections.OrderedDict()
_OCC_LIN_LOCK = threading.Lock()
_OCC_LIN_MAX = 8


def _occupancy_lin(density_bitfield, C, H):
    nbytes = _lib.lib().ngp_occupancy_lin_bytes(C, H)
    if not nbytes or not density_bitfield.is_cuda or density_bitfield.data_ptr() % 8 or density_bitfield.dtype != torch.uint8:
        return None
    stream = _lib.stream()
    key = (id(density_bitfield), int(stream or 0), C, H)
    with _OCC_LIN_LOCK:
        hit = _OCC_LIN.get(key)
        if hit is not None:
            ref, version, ptr, buf = hit
            if ref() is density_bitfield and version == density_bitfield._version and ptr == density_bitfield.data_ptr():
                _OCC_LIN.move_to_end(key)
                return buf
            del _OCC_LIN[key]
    buf = torch.empty(nbytes, dtype=torch.uint8, device=density_bitfield.device)      # (torch allocations are 512-byte aligned)
    _lib.call("build_occupancy_lin", density_bitfield, C, H, buf, nbytes, stream=stream)
    with _OCC_LIN_LOCK:
        _OCC_LIN[key] = (weakref.ref(density_bitfield), density_bitfield._version, density_bitfield.data_ptr(), buf)
        while len(_OCC_LIN) > _OCC_LIN_MAX:
            _OCC_LIN.popitem(last=False)
    return buf


class _march_rays(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, C, H, near, far,
                align=-1, perturb=False, dt_gamma=0, max_steps=1024):
        """raymarching.py:292-335.  -> xyzs, dirs, deltas of pad(n_alive*n_step) rows, slot = n*n_step"""
        rays_o, rays_d = _rays(rays_o, rays_d)
        M = n_alive * n_step
        if align > 0:
            M += align - (M % align)  # F11
        dev, dt = rays_o.device, rays_o.dtype
        xyzs = torch.empty(M, 3, dtype=dt, device=dev)
        dirs = torch.empty(M, 3, dtype=dt, device=dev)
        deltas = torch.empty(M, 2, dtype=dt, device=dev)
        occ = _occupancy_lin(density_bitfield, C, H) if USE_OCCUPANCY_LIN else None
        if occ is not None:
            _lib.call("march_rays_lin", n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H,
                      density_bitfield, near, far, xyzs, dirs, deltas, int(perturb), M, occ)
        else:
            _lib.call("march_rays", n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, density_bitfield,
                      near, far, xyzs, dirs, deltas, int(perturb), M)
        return xyzs, dirs, deltas


march_rays = _march_rays.apply


class _composite_rays(Function):
    @staticmethod
    @_fwd32
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image):
        """raymarching.py:340-359.  Updates rays_alive, rays_t, weights_sum, depth, image IN PLACE; returns ()."""
        sigmas, rgbs = sigmas.float().contiguous(), rgbs.float().contiguous()
        _lib.call("composite_rays", n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image,
                  wrote=(rays_alive, rays_t, weights_sum, depth, image))
        return tuple()


composite_rays = _composite_rays.apply
