#!/usr/bin/env python3
"""Render teacher frames of the synthetic scene's network into a blender-format folder that NeRFDataset / main_nerf read:

    python scripts/make_synthetic_dataset.py OUT [--size 200] [--train 100] [--val 2] [--test 4] [--rgba]

`--rgba` stores the opacity as an alpha channel (straight colours, as the nerf_synthetic files do): the frame is rendered on black
and on white, alpha = 1 - (white - black), colour = black / alpha.  Read it back with `--scale 1 --offset 0 0 0 --bound 2`."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerfsafetyvalidation_amd.nerf.provider import write_blender_dataset
from nerfsafetyvalidation_amd.nerf.utils import get_rays
from nerfsafetyvalidation_amd.scene import CAMERA_ANGLE_X, StonehengeScene


def render_frames(sc, teacher, views, rgba, device):
    poses = torch.from_numpy(sc.poses).to(device)
    frames = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for v in views:
            r = get_rays(poses[v:v + 1], sc.intrinsics, sc.H, sc.W)
            white = teacher.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False)["image"].float()[0]
            if rgba:
                black = teacher.render(r["rays_o"], r["rays_d"], staged=True, bg_color=0, perturb=False)["image"].float()[0]
                alpha = (1 - (white - black).mean(-1, keepdim=True)).clamp(0, 1)
                colour = torch.where(alpha > 0, black / alpha.clamp(min=1e-6), torch.zeros_like(black))
                image = torch.cat([colour, alpha], -1)
            else:
                image = white
            frames.append((image.clamp(0, 1) * 255).round().to(torch.uint8).view(sc.H, sc.W, -1).cpu().numpy())
    return np.stack(frames)


def make(out, size=200, n_train=100, n_val=2, n_test=4, rgba=False, device="cuda:0"):
    dev = torch.device(device)
    sc = StonehengeScene(H=size, W=size, bound=2)
    teacher = sc.build_model(dev)
    n_all = len(sc.poses)
    train = [int(v) for v in np.linspace(0, n_all, n_train, endpoint=False)]
    rest = [v for v in range(n_all) if v not in set(train)] or list(range(n_all))
    pick = lambda n, shift: [rest[(shift + i * max(1, len(rest) // max(1, n))) % len(rest)] for i in range(n)]
    for split, views in (("train", train), ("val", pick(n_val, 0)), ("test", pick(n_test, 1))):
        write_blender_dataset(out, sc.poses[views], render_frames(sc, teacher, views, rgba, dev), CAMERA_ANGLE_X, split)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--val", type=int, default=2)
    ap.add_argument("--test", type=int, default=4)
    ap.add_argument("--rgba", action="store_true")
    a = ap.parse_args()
    make(a.out, a.size, a.train, a.val, a.test, a.rgba)
    print(f"wrote {a.train} train / {a.val} val / {a.test} test views of {a.size}x{a.size} to {a.out}")
