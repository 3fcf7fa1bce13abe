"""The data side of Trainer.train_step / eval_step (reference: nerf/provider.py:311-316, nerf/utils.py:426-480).

Two forms of the same arithmetic:

  * the torch chain, written as the reference writes it (`reference_targets`, `reference_loss`): gather the pixels out of a float
    image tensor, sRGB -> linear, blend onto the background, MSELoss(reduction='none').mean(-1), the error-map scatter, mean.  It is
    the CPU path and the yardstick the kernels are tested against;
  * the HIP form (`training_targets`, `PhotometricLoss`): ngp_train_targets reads the chosen pixels straight out of the uint8 image
    store (a quarter of the reference's fp32 store) and ngp_photo_loss_forward / _backward are one autograd node each way.

`fused_targets` (module flag) selects the HIP form where it applies: a HIP device, one frame per batch, the criterion
MSELoss(reduction='none').  Everything else takes the torch chain.

Depth targets (DESIGN.md "Depth supervision") have the same two forms: `DepthStore` keeps a dataset's depth maps as 16-bit codes of
z-depth, `reference_depth_targets` turns the chosen pixels' codes into ray distances with torch operators, and
`training_depth_targets` (ngp_train_depth_targets) does the gather and the conversion in one launch."""
import numpy as np
import torch

from .. import _lib
from .utils import srgb_to_linear

fused_targets = True

_STORE_CODES = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}


def code_table(linear=False):
    """the 256 floats a uint8 code stands for: `image.astype(np.float32) / 255` (provider.py:221), through srgb_to_linear for the linear
    colour space (utils.py:430-431).  Host tensor."""
    table = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255)
    return srgb_to_linear(table) if linear else table


class ImageStore:
    """The dataset's frames as uint8 [n_img, H*W, C], resident on `data.device` (the HIP device when preloaded, the host otherwise).
    Indexing yields what the reference's `images` tensor holds -- float32 `code / 255`, bit for bit, in half where the reference keeps
    half (`opt.fp16 and opt.color_space != 'linear'`, provider.py:250-254) -- as [..., H, W, C] on the store's device."""

    def __init__(self, data, H, W, half=False):
        assert data.dtype == torch.uint8 and data.dim() == 3 and data.shape[1] == H * W and data.shape[2] in (3, 4)
        self.data, self.H, self.W, self.half = data.contiguous(), H, W, bool(half)
        self._tables = {}

    @property
    def shape(self):
        return torch.Size([self.data.shape[0], self.H, self.W, self.data.shape[2]])

    @property
    def dtype(self):
        return torch.float16 if self.half else torch.float32

    @property
    def device(self):
        return self.data.device

    def __len__(self):
        return self.data.shape[0]

    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def to(self, device):
        return ImageStore(self.data.to(device), self.H, self.W, self.half)

    def table(self, device, linear=False):
        key = (str(device), bool(linear))
        if key not in self._tables:
            self._tables[key] = code_table(linear).to(device)
        return self._tables[key]

    def __getitem__(self, index):
        codes = self.data[index]
        values = self.table(codes.device)[codes.long()]
        values = values.view(*codes.shape[:-2], self.H, self.W, codes.shape[-1])
        return values.half() if self.half else values

    def numpy(self):
        return self[torch.arange(len(self))].float().cpu().numpy()


class PixelBatch:
    """What `collate` hands over as `images` when the HIP form applies: the store, the frame and the chosen pixels instead of their
    gathered values.  `shape` is the shape of the tensor the reference would hold ([1, N, C] in training, [1, H, W, C] in evaluation) and
    `materialize()` builds exactly that tensor."""

    def __init__(self, store, frame, inds, device):
        self.store, self.frame, self.inds, self.device = store, int(frame), inds, device

    @property
    def shape(self):
        C = self.store.shape[-1]
        if self.inds is None:
            return torch.Size([1, self.store.H, self.store.W, C])
        return torch.Size([1, self.inds.shape[-1], C])

    def materialize(self):
        images = self.store[[self.frame]].to(self.device)
        if self.inds is None:
            return images
        C = images.shape[-1]
        return torch.gather(images.view(1, -1, C), 1, torch.stack(C * [self.inds], -1))


# ------------------------------------------------------------------------------------------------ depth maps
DEPTH_NONE, DEPTH_EMPTY = 0, 65535          # the two codes that are no distance: no measurement, known empty


def encode_depth(depth, integer_depth_scale):
    """float z-depth (any shape) -> uint16 codes: +inf -> 65535 (known empty), NaN or <= 0 -> 0 (no measurement), everything else
    round(z / integer_depth_scale) clipped to 1 .. 65534"""
    z = np.asarray(depth, dtype=np.float64)
    finite = np.isfinite(z) & (z > 0)
    codes = np.zeros(z.shape, dtype=np.uint16)
    codes[finite] = np.clip(np.rint(z[finite] / float(integer_depth_scale)), 1, 65534).astype(np.uint16)
    codes[np.isposinf(z)] = DEPTH_EMPTY
    return codes


class DepthStore:
    """The dataset's depth maps as 16-bit codes [n_img, H*W] (held as int16 bit patterns: torch indexes those on every device),
    resident on `data.device` like ImageStore.  A code k in 1 .. 65534 is the z-depth k * unit along the optical axis, in the units of
    the loaded poses (unit = integer_depth_scale * opt.scale); 0 is no measurement, 65535 known empty.  `intrinsics` (fx, fy, cx, cy)
    turn a pixel's z-depth into its ray distance."""

    def __init__(self, data, H, W, unit, intrinsics):
        assert data.dtype == torch.int16 and data.dim() == 2 and data.shape[1] == H * W
        self.data, self.H, self.W, self.unit = data.contiguous(), H, W, float(np.float32(unit))
        self.intrinsics = tuple(float(v) for v in intrinsics)

    @classmethod
    def from_codes(cls, codes, H, W, unit, intrinsics):
        """codes: uint16 numpy [n_img, H, W]"""
        codes = np.ascontiguousarray(codes, dtype=np.uint16).reshape(codes.shape[0], H * W)
        return cls(torch.from_numpy(codes.view(np.int16)), H, W, unit, intrinsics)

    @property
    def device(self):
        return self.data.device

    def __len__(self):
        return self.data.shape[0]

    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def to(self, device):
        return DepthStore(self.data.to(device), self.H, self.W, self.unit, self.intrinsics)

    def codes(self, index):
        """the codes of frames `index` as int32 [..., H*W] in 0 .. 65535"""
        return self.data[index].to(torch.int32) & 0xFFFF


def reference_depth_targets(codes, pix, W, intrinsics, unit):
    """codes int [..., N] of the pixels `pix` (flat ids, same shape) -> float32 ray distances, by torch operators:
    t = (code * unit) * |dir|, dir = ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1), the direction get_rays forms for the pixel before it
    normalises it; code 0 -> 0, code 65535 -> +inf."""
    fx, fy, cx, cy = intrinsics
    x = (((pix % W).float() + 0.5) - cx) / fx
    y = ((torch.div(pix, W, rounding_mode="floor").float() + 0.5) - cy) / fy
    t = (codes.float() * unit) * torch.sqrt((x * x + y * y) + 1.0)
    t = torch.where(codes == DEPTH_EMPTY, torch.full_like(t, float("inf")), t)
    return torch.where(codes == DEPTH_NONE, torch.zeros_like(t), t)


class DepthBatch:
    """What `collate` hands over as `depth` when the HIP form applies: the store, the frame and the chosen pixels.  `materialize()`
    builds the [1, N] tensor of ray distances the torch form gives."""

    def __init__(self, store, frame, inds, device):
        self.store, self.frame, self.inds, self.device = store, int(frame), inds, device

    @property
    def shape(self):
        return torch.Size([1, self.store.H * self.store.W if self.inds is None else self.inds.shape[-1]])

    def materialize(self):
        st = self.store
        codes = st.codes([self.frame]).to(self.device)
        pix = torch.arange(st.H * st.W, device=self.device)[None] if self.inds is None else self.inds.reshape(1, -1)
        return reference_depth_targets(torch.gather(codes, 1, pix), pix, st.W, st.intrinsics, st.unit)


def training_depth_targets(batch):
    """DepthBatch -> float32 [1, N] ray distances, one launch (ngp_train_depth_targets) straight from the 16-bit store"""
    st, device = batch.store, batch.device
    n_pix = st.H * st.W
    if st.data.device == device:
        data, base = st.data, batch.frame * n_pix
    else:
        data, base = st.data[batch.frame].to(device, non_blocking=True), 0
    inds = None if batch.inds is None else batch.inds.reshape(-1).contiguous()
    if inds is not None and inds.dtype != torch.int64:
        raise RuntimeError("pixel ids must be int64")
    N = n_pix if inds is None else int(inds.shape[0])
    if base + n_pix > data.numel():
        raise RuntimeError("the frame lies outside the depth store")
    out = torch.empty(N, dtype=torch.float32, device=device)
    fx, fy, cx, cy = st.intrinsics
    _lib.call("train_depth_targets", data, int(base), n_pix, st.W, inds, N, fx, fy, cx, cy, st.unit, out)
    return out.view(1, N)


# ------------------------------------------------------------------------------------------------ the torch chain (the reference's text)
def reference_targets(images, bg_color, color_space="srgb"):
    """images [B, N, 3/4] (or [B, H, W, 3/4]) -> gt_rgb (utils.py:430-444, :496-504).  Converts `images` in place, as the reference does."""
    C = images.shape[-1]
    if color_space == "linear":
        images[..., :3] = srgb_to_linear(images[..., :3])
    if C == 4:
        return images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
    return images


def reference_loss(criterion, pred_rgb, gt_rgb, error_map=None, index=None, inds_coarse=None):
    """utils.py:450-480: per-ray loss, the error-map update (in place on `error_map`), the mean"""
    loss = criterion(pred_rgb, gt_rgb).mean(-1)
    if len(loss.shape) == 3:
        loss = loss.mean(0)
    if error_map is not None:
        rows = error_map[index]
        error = loss.detach().to(rows.device)
        ema_error = 0.1 * rows.gather(1, inds_coarse) + 0.9 * error
        rows.scatter_(1, inds_coarse, ema_error)
        error_map[index] = rows
    return loss.mean()


# ------------------------------------------------------------------------------------------------ the HIP form
def gather_targets(store, frame_base, n_pix, inds, bg, table=None, round_half=False, n=None):
    """ngp_train_targets.  store: contiguous HIP tensor [..., C] (uint8 / f16 / f32); frame_base: first pixel of the frame in it;
    inds int64 [N] or None (pixels 0..n-1); bg float [N,3] or None (white); table float [256] or None -> gt float [N,3]"""
    if store.dtype not in _STORE_CODES:
        raise RuntimeError(f"image store of dtype {store.dtype}: uint8, float16 or float32")
    N = int(inds.shape[0]) if inds is not None else int(n_pix if n is None else n)
    if inds is not None and inds.dtype != torch.int64:
        raise RuntimeError("pixel ids must be int64")
    if bg is not None and (bg.dtype != torch.float32 or bg.numel() != N * 3):
        raise RuntimeError("the background is float32 [N,3]")
    if (frame_base + n_pix) * store.shape[-1] > store.numel():
        raise RuntimeError("the frame lies outside the image store")
    gt = torch.empty(N, 3, dtype=torch.float32, device=store.device)
    _lib.call("train_targets", store, _STORE_CODES[store.dtype], store.shape[-1], int(frame_base), int(n_pix), inds, N, bg, table,
              int(bool(round_half)), gt)
    return gt


def training_targets(batch, bg_color=None, color_space="srgb"):
    """PixelBatch -> gt_rgb float32 [1, N, 3] (training) or [1, H, W, 3] (evaluation, white background when bg_color is None or 1).
    bg_color: None / 1 (white) or a [1, N, 3] tensor (the random background, drawn by the caller as the reference draws it)."""
    store, device = batch.store, batch.device
    n_pix = store.H * store.W
    if store.data.device == device:
        data, base = store.data, batch.frame * n_pix
    else:
        data, base = store.data[batch.frame].to(device, non_blocking=True), 0       # one frame per step (provider.py:312)
    bg = None
    if torch.is_tensor(bg_color):
        bg = bg_color.reshape(-1, 3).float().contiguous()
    elif bg_color not in (None, 1):
        raise RuntimeError("training_targets: the background is white (None / 1) or a per-ray tensor")
    linear = color_space == "linear"
    inds = None if batch.inds is None else batch.inds.reshape(-1).contiguous()
    gt = gather_targets(data, base, n_pix, inds, bg, store.table(device, True) if linear else None, store.half)
    return gt.view(1, -1, 3) if inds is not None else gt.view(1, store.H, store.W, 3)


def photo_loss_forward(pred, gt, error_row=None, inds_coarse=None):
    """pred [..., 3] (f32 / f16), gt float32 of the same shape -> (per_ray float32 [N], mean 0-dim); updates error_row in place"""
    N = pred.numel() // 3
    dev = pred.device
    per_ray = torch.empty(N, dtype=torch.float32, device=dev)
    mean = torch.empty((), dtype=torch.float32, device=dev)
    work, nbytes = _lib.workspace("photo_loss", N, device=dev)
    if error_row is not None:
        if error_row.dtype != torch.float32 or inds_coarse is None or inds_coarse.dtype != torch.int64 or inds_coarse.numel() != N:
            raise RuntimeError("the error-map row is float32 and inds_coarse int64 [N]")
        inds_coarse = inds_coarse.reshape(-1).contiguous()
    _lib.call("photo_loss_forward", pred, _lib.dtype_code(pred), gt, N, per_ray, mean, error_row,
              0 if error_row is None else error_row.numel(), inds_coarse if error_row is not None else None, work, nbytes,
              wrote=() if error_row is None else (error_row,))
    return per_ray, mean


def photo_loss_backward(pred, gt, g):
    """grad_pred = g * 2 (pred - gt) / (3 N), g a 0-dim float32 tensor on the device"""
    grad = torch.empty_like(pred)
    _lib.call("photo_loss_backward", pred, _lib.dtype_code(pred), gt, pred.numel() // 3, g, grad)
    return grad


class PhotometricLoss(torch.autograd.Function):
    """criterion(pred, gt).mean(-1) -> error-map update -> .mean() of train_step as one node each way"""

    @staticmethod
    def forward(ctx, pred, gt, error_row, inds_coarse):
        pred, gt = pred.contiguous(), gt.contiguous()
        if gt.dtype != torch.float32 or gt.shape != pred.shape:
            raise RuntimeError("PhotometricLoss: gt is float32 of pred's shape")
        _, mean = photo_loss_forward(pred, gt, error_row, inds_coarse)
        ctx.save_for_backward(pred, gt)
        return mean

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        return photo_loss_backward(pred, gt, g.float().contiguous()), None, None, None


def photometric_loss(pred, gt, error_row=None, inds_coarse=None):
    return PhotometricLoss.apply(pred, gt, error_row, inds_coarse)


def is_plain_mse(criterion):
    return type(criterion) is torch.nn.MSELoss and criterion.reduction == "none"
