"""Keypoints and the interest mask of the reference's state estimator (nav/estimator_helpers.py:10-35 find_POI, :95-107), on the GPU.

find_POI ran OpenCV's SIFT on the frame; here SIFT's detection stage with cv2.SIFT_create()'s defaults is the HIP kernel chain of
csrc/features.hip (ngp_sift_interest_mask).  The estimator consumes only the integer keypoint positions and the dilated mask built
from them, so orientations and descriptors are not computed.  nav/sift_numpy.py restates the kernels in float32 numpy; the tests
hold the two equal bit for bit.  OpenCV's own keypoints are not the yardstick ("The state estimator")."""
import numpy as np
import torch

from .. import _lib


def _frame(img_rgb, device):
    """uint8 [H,W,3] (numpy or torch) -> contiguous uint8 tensor on the GPU"""
    t = img_rgb if torch.is_tensor(img_rgb) else torch.from_numpy(np.ascontiguousarray(img_rgb))
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"features: a uint8 [H, W, 3] frame (got {tuple(t.shape)} {t.dtype})")
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device).contiguous()


def sift_interest_mask(img_rgb, kernel_size=5, dil_iter=3, device=None, return_pyramid=False):
    """-> dict(points, mask: uint8 [W, H] on the GPU, indexed [x, y] as the reference's interest_regions; count: int32 [1] on the GPU,
    the number of accepted keypoints before deduplication) and, with return_pyramid, 'pyramid': per octave the float32 Gaussian
    [6, rows, cols] and DoG [5, rows, cols] layers (views into the workspace)."""
    rgb = _frame(img_rgb, device)
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    lib = _lib.lib()
    ws, ws_bytes = _lib.workspace("sift", H, W, device=rgb.device)
    if ws is None:
        raise ValueError(f"features: unsupported frame size {H} x {W} (each side in [8, 16384], 20 H W < 2^32)")
    points = torch.empty(W, H, dtype=torch.uint8, device=rgb.device)
    mask = torch.empty(W, H, dtype=torch.uint8, device=rgb.device)
    count = torch.empty(1, dtype=torch.int32, device=rgb.device)
    _lib.call("sift_interest_mask", rgb, H, W, int(kernel_size), int(dil_iter), points, mask, count, ws, ws_bytes)
    out = {"points": points, "mask": mask, "count": count}
    if return_pyramid:
        pyr = []
        rows, cols = 2 * H, 2 * W
        for o in range(lib.ngp_sift_octaves(H, W)):
            off = lib.ngp_sift_layer_offset(H, W, o, 0)
            plane = rows * cols
            layers = ws[off:off + 11 * plane * 4].view(torch.float32).view(11, rows, cols)
            pyr.append((layers[:6], layers[6:]))
            rows, cols = rows // 2, cols // 2
        out["pyramid"] = pyr
        out["workspace"] = ws
    return out


def find_POI(img_rgb, render=False):
    """estimator_helpers.py:10-35: -> (xy int64 [n, 2] -- the distinct truncated keypoint positions (x, y), sorted; the reference's
    set has no order -- and extras {'features': None}).  No keypoint: xy has shape (0,), as np.array([]) in the reference."""
    pts = sift_interest_mask(img_rgb, dil_iter=0)["points"]
    xy = torch.nonzero(pts).cpu().numpy().astype(np.int64)
    if xy.shape[0] == 0:
        xy = np.zeros((0,), np.int64)
    return xy, {"features": None}


def interest_mask(img_rgb, kernel_size, dil_iter):
    """the dilated interest mask of estimate_relative_pose (:101-106): bool [W, H] on the GPU, indexed [x, y], and the keypoint count"""
    out = sift_interest_mask(img_rgb, kernel_size, dil_iter)
    return out["mask"].bool(), int(out["count"].item())
