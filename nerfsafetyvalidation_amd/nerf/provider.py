"""Posed-image datasets (reference: nerf/provider.py:19-27, 57-91, 94-332): the instant-ngp `transforms*.json` formats, read into
camera poses, intrinsics and an image store, and served to the Trainer one frame per step.

What differs from the reference, and why:
  * images are decoded with PIL (8-bit RGB / RGBA; anything else is refused).  `downscale != 1` resizes with PIL's box filter, which
    may differ from cv2.INTER_AREA in the last bit of a pixel;
  * the images stay uint8 (`targets.ImageStore`, [n_img, H*W, C]): a quarter of the reference's fp32 tensor.  Indexing `images`
    yields the reference's values (`code / 255` in float32, bit for bit; half where the reference holds half);
  * on a HIP device `collate` hands the Trainer the chosen pixel ids (`targets.PixelBatch`) instead of their gathered values, and
    ngp_train_targets reads them out of the store (`targets.fused_targets = False`, a CPU device or B > 1: the reference's gather);
  * `rand_pose >= 0` (CLIP-guided training) is not ported;
  * depth supervision (not in the reference): frames may name a 16-bit `depth_path` with a top-level `integer_depth_scale`
    (Instant-NGP's keys).  The maps are read only when `opt.lambda_depth > 0 or opt.lambda_free > 0`, kept as codes
    (`targets.DepthStore`), and `collate` adds `depth`: the chosen pixels' ray distances (DESIGN.md "Depth supervision")."""
import glob
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import targets
from .targets import DepthBatch, DepthStore, ImageStore, PixelBatch
from .utils import get_rays


def nerf_matrix_to_ngp(pose, scale=0.33, offset=[0, 0, 0]):
    """provider.py:19-27 (for the fox dataset, 0.33 scales the camera radius to about 2)"""
    new_pose = np.array([
        [pose[1, 0], -pose[1, 1], -pose[1, 2], pose[1, 3] * scale + offset[0]],
        [pose[2, 0], -pose[2, 1], -pose[2, 2], pose[2, 3] * scale + offset[1]],
        [pose[0, 0], -pose[0, 1], -pose[0, 2], pose[0, 3] * scale + offset[2]],
        [0, 0, 0, 1],
    ], dtype=np.float32)
    return new_pose


def ngp_matrix_to_nerf(pose, scale=0.33, offset=[0, 0, 0]):
    """inverse of nerf_matrix_to_ngp (exact for scale = 1, offset = 0: only signs and rows move)"""
    return np.array([
        [pose[2, 0], -pose[2, 1], -pose[2, 2], (pose[2, 3] - offset[2]) / scale],
        [pose[0, 0], -pose[0, 1], -pose[0, 2], (pose[0, 3] - offset[0]) / scale],
        [pose[1, 0], -pose[1, 1], -pose[1, 2], (pose[1, 3] - offset[1]) / scale],
        [0, 0, 0, 1],
    ], dtype=np.float32)


def rand_poses(size, device, radius=1, theta_range=[np.pi / 3, 2 * np.pi / 3], phi_range=[0, 2 * np.pi]):
    """random poses of an orbit camera, [size, 4, 4] (provider.py:57-91); the look-at is scene.look_at_poses"""
    from ..scene import look_at_poses
    thetas = torch.rand(size, device=device) * (theta_range[1] - theta_range[0]) + theta_range[0]
    phis = torch.rand(size, device=device) * (phi_range[1] - phi_range[0]) + phi_range[0]
    centers = torch.stack([radius * torch.sin(thetas) * torch.sin(phis), radius * torch.cos(thetas), radius * torch.sin(thetas) * torch.cos(phis)], dim=-1)
    return torch.from_numpy(look_at_poses(centers.double().cpu().numpy()).astype(np.float32)).to(device)


def read_image(path):
    """uint8 [H, W, 3/4] (RGB order) of an 8-bit RGB / RGBA file"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise ValueError(f"{path}: image mode {im.mode!r}; only 8-bit RGB and RGBA images are supported")
        return np.array(im, dtype=np.uint8)


def read_depth(path):
    """uint16 [H, W] codes of a 16-bit greyscale file"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B", "I"):
            raise ValueError(f"{path}: image mode {im.mode!r}; depth maps are 16-bit greyscale")
        codes = np.array(im)
    if codes.ndim != 2 or codes.min() < 0 or codes.max() > 65535:
        raise ValueError(f"{path}: depth maps are 16-bit greyscale")
    return codes.astype(np.uint16)


def _resize_box(image, W, H):
    from PIL import Image
    return np.array(Image.fromarray(image).resize((W, H), Image.BOX), dtype=np.uint8)


class NeRFDataset:
    def __init__(self, opt, device, type='train', downscale=1, n_test=10):
        super().__init__()
        self.opt = opt
        self.device = torch.device(device)
        self.type = type  # train, val, test
        self.downscale = downscale
        self.root_path = opt.path
        self.preload = opt.preload  # keep the image store on the device
        self.scale = opt.scale  # camera radius scale to make sure cameras are inside the bounding box
        self.offset = opt.offset  # camera offset
        self.bound = opt.bound
        self.fp16 = opt.fp16

        self.training = self.type in ['train', 'all', 'trainval']
        self.num_rays = self.opt.num_rays if self.training else -1

        # depth maps are read only for the depth terms: with both weights 0 a dataset that has them loads exactly as one without
        self.with_depth = getattr(opt, "lambda_depth", 0) > 0 or getattr(opt, "lambda_free", 0) > 0

        self.rand_pose = opt.rand_pose
        if self.rand_pose >= 0:
            raise NotImplementedError("rand_pose >= 0 (CLIP-guided training on random poses) is not ported")

        # auto-detect transforms.json and split mode
        if os.path.exists(os.path.join(self.root_path, 'transforms.json')):
            self.mode = 'colmap'  # manually split, use view-interpolation for test
        elif os.path.exists(os.path.join(self.root_path, 'transforms_train.json')):
            self.mode = 'blender'  # provided split
        else:
            raise NotImplementedError(f'[NeRFDataset] Cannot find transforms*.json under {self.root_path}')

        if self.mode == 'colmap':
            with open(os.path.join(self.root_path, 'transforms.json'), 'r') as f:
                transform = json.load(f)
        else:
            if type == 'all':  # every split (train / val / test), as instant-ngp does
                transform = None
                for transform_path in glob.glob(os.path.join(self.root_path, '*.json')):
                    with open(transform_path, 'r') as f:
                        tmp_transform = json.load(f)
                        if transform is None:
                            transform = tmp_transform
                        else:
                            transform['frames'].extend(tmp_transform['frames'])
            elif type == 'trainval':
                with open(os.path.join(self.root_path, 'transforms_train.json'), 'r') as f:
                    transform = json.load(f)
                with open(os.path.join(self.root_path, 'transforms_val.json'), 'r') as f:
                    transform_val = json.load(f)
                transform['frames'].extend(transform_val['frames'])
            else:
                with open(os.path.join(self.root_path, f'transforms_{type}.json'), 'r') as f:
                    transform = json.load(f)

        if 'h' in transform and 'w' in transform:
            self.H = int(transform['h']) // downscale
            self.W = int(transform['w']) // downscale
        else:
            self.H = self.W = None  # read from the first image

        frames = transform["frames"]

        if self.mode == 'colmap' and type == 'test':
            # two random poses and a sweep between them (slerp with a sine easing)
            from scipy.spatial.transform import Rotation, Slerp
            f0, f1 = np.random.choice(frames, 2, replace=False)
            pose0 = nerf_matrix_to_ngp(np.array(f0['transform_matrix'], dtype=np.float32), scale=self.scale, offset=self.offset)
            pose1 = nerf_matrix_to_ngp(np.array(f1['transform_matrix'], dtype=np.float32), scale=self.scale, offset=self.offset)
            rots = Rotation.from_matrix(np.stack([pose0[:3, :3], pose1[:3, :3]]))
            slerp = Slerp([0, 1], rots)

            self.poses = []
            images = None
            for i in range(n_test + 1):
                ratio = np.sin(((i / n_test) - 0.5) * np.pi) * 0.5 + 0.5
                pose = np.eye(4, dtype=np.float32)
                pose[:3, :3] = slerp(ratio).as_matrix()
                pose[:3, 3] = (1 - ratio) * pose0[:3, 3] + ratio * pose1[:3, 3]
                self.poses.append(pose)
        else:
            if self.mode == 'colmap':  # the first frame is the validation set
                if type == 'train':
                    frames = frames[1:]
                elif type == 'val':
                    frames = frames[:1]

            self.poses = []
            images = []
            depth_maps = []
            for f in frames:
                f_path = os.path.join(self.root_path, f['file_path'])
                if self.mode == 'blender' and '.' not in os.path.basename(f_path):
                    f_path += '.png'
                if not os.path.exists(f_path):  # (the fox dataset lists files it does not have)
                    continue

                pose = np.array(f['transform_matrix'], dtype=np.float32)
                pose = nerf_matrix_to_ngp(pose, scale=self.scale, offset=self.offset)

                image = read_image(f_path)
                if self.H is None or self.W is None:
                    self.H = image.shape[0] // downscale
                    self.W = image.shape[1] // downscale
                if image.shape[0] != self.H or image.shape[1] != self.W:
                    image = _resize_box(image, self.W, self.H)

                self.poses.append(pose)
                images.append(image)

                if self.with_depth:
                    if 'depth_path' not in f:
                        depth_maps.append(None)      # (an all-zero map: no measurement anywhere)
                        continue
                    if downscale != 1:
                        raise NotImplementedError("depth maps together with downscale != 1 are not supported")
                    codes = read_depth(os.path.join(self.root_path, f['depth_path']))
                    if codes.shape != (self.H, self.W):
                        raise ValueError(f"{f['depth_path']}: depth map of {codes.shape[1]} x {codes.shape[0]}, image of {self.W} x {self.H}")
                    depth_maps.append(codes)

        self.poses = torch.from_numpy(np.stack(self.poses, axis=0))  # [N, 4, 4]
        self.images = None
        if images is not None:
            codes = torch.from_numpy(np.stack(images, axis=0))  # [N, H, W, C] uint8
            half = bool(self.preload and self.fp16 and self.opt.color_space != 'linear')    # where the reference holds half
            self.images = ImageStore(codes.view(codes.shape[0], self.H * self.W, codes.shape[-1]), self.H, self.W, half=half)

        self.radius = self.poses[:, :3, 3].norm(dim=-1).mean(0).item()

        if self.training and self.opt.error_map:
            self.error_map = torch.ones([self.images.shape[0], 128 * 128], dtype=torch.float)
        else:
            self.error_map = None

        if self.preload:
            self.poses = self.poses.to(self.device)
            if self.images is not None:
                self.images = self.images.to(self.device)
            if self.error_map is not None:
                self.error_map = self.error_map.to(self.device)

        # intrinsics: focal lengths, then fields of view, else an error
        if 'fl_x' in transform or 'fl_y' in transform:
            fl_x = (transform['fl_x'] if 'fl_x' in transform else transform['fl_y']) / downscale
            fl_y = (transform['fl_y'] if 'fl_y' in transform else transform['fl_x']) / downscale
        elif 'camera_angle_x' in transform or 'camera_angle_y' in transform:
            fl_x = self.W / (2 * np.tan(transform['camera_angle_x'] / 2)) if 'camera_angle_x' in transform else None
            fl_y = self.H / (2 * np.tan(transform['camera_angle_y'] / 2)) if 'camera_angle_y' in transform else None
            if fl_x is None: fl_x = fl_y
            if fl_y is None: fl_y = fl_x
        else:
            raise RuntimeError('Failed to load focal length, please check the transforms.json!')

        cx = (transform['cx'] / downscale) if 'cx' in transform else (self.W / 2)
        cy = (transform['cy'] / downscale) if 'cy' in transform else (self.H / 2)

        self.intrinsics = np.array([fl_x, fl_y, cx, cy])

        self.depths = None
        if self.with_depth and images is not None:
            if any(m is not None for m in depth_maps) and 'integer_depth_scale' not in transform:
                raise RuntimeError("frames name a depth_path but the transforms file has no integer_depth_scale")
            codes = np.stack([np.zeros((self.H, self.W), dtype=np.uint16) if m is None else m for m in depth_maps], axis=0)
            self.depths = DepthStore.from_codes(codes, self.H, self.W, float(transform.get('integer_depth_scale', 1.0)) * self.scale, self.intrinsics)
            if self.preload:
                self.depths = self.depths.to(self.device)

    def collate(self, index):
        B = len(index)  # a list of length 1
        poses = self.poses[index].to(self.device)  # [B, 4, 4]
        error_map = None if self.error_map is None else self.error_map[index]
        rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays, error_map)

        results = {
            'H': self.H,
            'W': self.W,
            'rays_o': rays['rays_o'],
            'rays_d': rays['rays_d'],
        }

        if self.images is not None:
            if targets.fused_targets and self.device.type == 'cuda' and B == 1:
                results['images'] = PixelBatch(self.images, index[0], rays['inds'] if self.training else None, self.device)
            else:
                images = self.images[index].to(self.device)  # [B, H, W, 3/4]
                if self.training:
                    C = images.shape[-1]
                    images = torch.gather(images.view(B, -1, C), 1, torch.stack(C * [rays['inds']], -1))  # [B, N, 3/4]
                results['images'] = images

        if self.depths is not None:      # ray distances of the same pixels (0: no measurement, +inf: known empty)
            if targets.fused_targets and self.device.type == 'cuda' and B == 1:
                results['depth'] = DepthBatch(self.depths, index[0], rays['inds'] if self.training else None, self.device)
            else:
                codes = self.depths.codes(index).to(self.device)  # [B, H*W]
                pix = rays['inds'] if self.training else torch.arange(self.H * self.W, device=self.device).expand(B, -1)
                results['depth'] = targets.reference_depth_targets(torch.gather(codes, 1, pix), pix, self.W, self.depths.intrinsics, self.depths.unit)

        if error_map is not None:  # the trainer needs these to update the error map
            results['index'] = index
            results['inds_coarse'] = rays['inds_coarse']

        return results

    def dataloader(self):
        size = len(self.poses)
        loader = DataLoader(list(range(size)), batch_size=1, collate_fn=self.collate, shuffle=self.training, num_workers=0)
        loader._data = self  # the trainer reads error_map and poses through the loader
        loader.has_gt = self.images is not None
        return loader


def write_blender_dataset(path, poses_ngp, images_uint8, camera_angle_x, split, scale=1.0, offset=(0, 0, 0), depths=None, integer_depth_scale=None):
    """Write `transforms_<split>.json` and `<split>/r_<i>.png` under `path` so that NeRFDataset(opt.scale = scale, opt.offset = offset)
    reads back `poses_ngp` [n,4,4] (this package's camera convention; exactly for scale = 1, offset = 0) and `images_uint8`
    [n,H,W,3/4].

    depths: float [n,H,W] z-depth along the optical axis, in the units of the WRITTEN poses (np.inf: known empty, NaN or <= 0: no
    measurement), written as 16-bit greyscale `<split>/r_<i>_depth.png` of codes round(z / integer_depth_scale) (targets.encode_depth)
    with Instant-NGP's keys: `depth_path` per frame, `integer_depth_scale` at the top level (default: the largest finite depth / 65534)."""
    from PIL import Image
    os.makedirs(os.path.join(path, split), exist_ok=True)
    top = {"camera_angle_x": float(camera_angle_x)}
    if depths is not None:
        depths = np.asarray(depths, dtype=np.float64)
        if depths.ndim != 3 or depths.shape[0] != len(images_uint8) or depths.shape[1:] != np.asarray(images_uint8[0]).shape[:2]:
            raise ValueError("depths are float [n, H, W], one map per image")
        if integer_depth_scale is None:
            finite = depths[np.isfinite(depths) & (depths > 0)]
            integer_depth_scale = float(finite.max()) / 65534 if finite.size else 1.0
        top["integer_depth_scale"] = float(integer_depth_scale)
    frames = []
    for i, (pose, image) in enumerate(zip(np.asarray(poses_ngp, dtype=np.float32), np.asarray(images_uint8))):
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[-1] not in (3, 4):
            raise ValueError("images are uint8 [H, W, 3] or [H, W, 4]")
        Image.fromarray(np.ascontiguousarray(image)).save(os.path.join(path, split, f"r_{i}.png"))
        nerf = ngp_matrix_to_nerf(pose, scale=scale, offset=list(offset))
        frame = {"file_path": f"./{split}/r_{i}", "transform_matrix": [[float(v) for v in row] for row in nerf]}
        if depths is not None:
            codes = targets.encode_depth(depths[i], integer_depth_scale)
            Image.fromarray(codes).save(       # (uint16 -> mode I;16)
                os.path.join(path, split, f"r_{i}_depth.png"))
            frame["depth_path"] = f"./{split}/r_{i}_depth.png"
        frames.append(frame)
    with open(os.path.join(path, f"transforms_{split}.json"), "w") as f:
        json.dump({**top, "frames": frames}, f, indent=1)
    return path
