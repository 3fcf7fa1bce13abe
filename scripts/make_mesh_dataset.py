#!/usr/bin/env python3
"""Render frames of a triangle mesh (world.MeshWorld) into a blender-format folder that NeRFDataset / main_nerf read, so that one mesh
can be the world a NeRF is trained on, validated against (rollout's `world`) and collision-checked against:

    python scripts/make_mesh_dataset.py OUT [--size 200] [--train 100] [--val 2] [--test 4] [--ply PATH] [--device cuda:0] [--depth]

The mesh is scene.henge_mesh() (the synthetic scene, in the NeRF's axes) or, with --ply, any mesh mesh.write_ply wrote (vertex colours
when it has them).  The cameras are scene.orbit_poses.  The frames are RGBA: the headlight-shaded colour, alpha 1 on a hit and 0 on a
miss.  --depth also writes the world's depth per pixel for depth-supervised training (16-bit `r_<i>_depth.png`, Instant-NGP's
`depth_path` / `integer_depth_scale`): the cast's ray distance divided by the length of the pixel's unnormalised direction, which is
the z-depth along the optical axis, and +inf (known empty) on a miss.  Read it back with `--scale 1 --offset 0 0 0 --bound 2`.  --device cpu renders through the package's numpy path."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerfsafetyvalidation_amd.mesh import read_ply
from nerfsafetyvalidation_amd.nerf.provider import write_blender_dataset
from nerfsafetyvalidation_amd.scene import CAMERA_ANGLE_X, henge_mesh, intrinsics, orbit_poses
from nerfsafetyvalidation_amd.world import MeshWorld


def render_frames(world, poses, size, depth=False):
    """-> uint8 [n, size, size, 4] (and, with depth, float64 [n, size, size] z-depth, +inf on a miss)"""
    K = intrinsics(size, size)
    fx, fy, cx, cy = [float(v) for v in K]
    x = (np.arange(size, dtype=np.float64) + 0.5 - cx) / fx
    y = (np.arange(size, dtype=np.float64) + 0.5 - cy) / fy
    length = np.sqrt(x[None, :] ** 2 + y[:, None] ** 2 + 1.0)          # |dir| of get_rays' direction before it is normalised
    frames, depths = [], []
    for pose in poses:
        out = world.render(torch.from_numpy(pose), K, size, size, bg_color=0.0)
        alpha = (out["prim"] >= 0).to(torch.uint8) * 255
        frames.append(torch.cat([out["image_u8"], alpha[..., None]], -1).cpu().numpy())
        if depth:
            depths.append(out["depth"].double().cpu().numpy() / length)
    return (np.stack(frames), np.stack(depths)) if depth else np.stack(frames)


def make(out, size=200, n_train=100, n_val=2, n_test=4, ply=None, device="cuda:0", resolution=64, depth=False):
    dev = torch.device(device)
    vertices, faces, colors = read_ply(ply) if ply else henge_mesh(resolution)
    world = MeshWorld(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev), None if colors is None else torch.from_numpy(colors).to(dev))
    poses = orbit_poses()
    n_all = len(poses)
    train = [int(v) for v in np.linspace(0, n_all, n_train, endpoint=False)]
    rest = [v for v in range(n_all) if v not in set(train)] or list(range(n_all))
    pick = lambda n, shift: [rest[(shift + i * max(1, len(rest) // max(1, n))) % len(rest)] for i in range(n)]
    for split, views in (("train", train), ("val", pick(n_val, 0)), ("test", pick(n_test, 1))):
        if depth:
            frames, depths = render_frames(world, poses[views], size, depth=True)
            write_blender_dataset(out, poses[views], frames, CAMERA_ANGLE_X, split, depths=depths)
        else:
            write_blender_dataset(out, poses[views], render_frames(world, poses[views], size), CAMERA_ANGLE_X, split)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--val", type=int, default=2)
    ap.add_argument("--test", type=int, default=4)
    ap.add_argument("--ply", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--depth", action="store_true", help="also write the world's depth maps (depth-supervised training)")
    a = ap.parse_args()
    make(a.out, a.size, a.train, a.val, a.test, a.ply, a.device, depth=a.depth)
    print(f"wrote {a.train} train / {a.val} val / {a.test} test views of {a.size}x{a.size} to {a.out}")
