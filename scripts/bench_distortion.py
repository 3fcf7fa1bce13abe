#!/usr/bin/env python3
"""The distortion regulariser on the MI355X: (1) forward + backward of the HIP node (raymarching.distortion_rays_train) against the
same computation as torch operators on the same GPU -- gather the packed samples to dense [N, longest ray], cumprod / cumsum, autograd --
on a training batch (4096 rays) and on a full 800 x 800 frame (640 k rays) of the trained student; (2) Trainer steps/s with
--lambda_distort 0 and 1e-3, alternated in one process (bench_trainer.py's set-up).  Appends the lines to profiles/distortion_bench.jsonl.

    python scripts/bench_distortion.py [--size 800] [--views 100] [--out profiles/distortion_bench.jsonl]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

import make_synthetic_dataset
from nerfsafetyvalidation_amd import raymarching
from nerfsafetyvalidation_amd.nerf.provider import NeRFDataset
from nerfsafetyvalidation_amd.nerf.trainer import Trainer
from nerfsafetyvalidation_amd.nerf.utils import get_rays
from nerfsafetyvalidation_amd.optim import Adam
from nerfsafetyvalidation_amd.scene import StonehengeScene


def torch_chain(sigmas, deltas, scale_rows, rows, inside, n_rays):
    """the operator's definition with torch operators on dense [N, T] (rows / inside: the gather plan, built once outside the timing)"""
    sg, dt, gap = sigmas[rows] * inside, deltas[rows, 0] * inside, deltas[rows, 1] * inside
    alpha = 1 - torch.exp(-sg * dt)
    T = torch.cumprod(1 - alpha, dim=1)
    T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], dim=1)
    w = alpha * T * (T >= 1e-4) * inside                       # T_i >= 1e-4: no earlier sample took the ray below the threshold
    m, delta = scale_rows * torch.cumsum(gap, dim=1), scale_rows * dt
    wm = w * m
    W, WM = torch.cumsum(w, dim=1) - w, torch.cumsum(wm, dim=1) - wm
    return ((2 * w * (m * W - WM)).sum() + ((1 / 3) * delta * w * w).sum()) / n_rays


def gather_plan(rays, M):
    index, offset, count = rays[:, 0].long(), rays[:, 1].long(), rays[:, 2].long()
    count = torch.where(offset + count >= M, torch.zeros_like(count), count)
    steps = torch.arange(int(count.max()), device=rays.device)[None, :]
    inside = steps < count[:, None]
    return (offset[:, None] + steps).clamp(max=M - 1), inside, index


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def operator_line(model, origins, directions, mean_count, reps, what):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        nears, fars = raymarching.near_far_from_aabb(origins, directions, model.aabb_train, model.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=origins.device)
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(origins, directions, model.bound, model.density_bitfield, model.cascade,
                                                                model.grid_size, nears, fars, counter, mean_count, False, 128, False, 0, 1024)
        used = int(counter[0].item())
        sigmas = torch.zeros(xyzs.shape[0], dtype=torch.float32, device=origins.device)
        for at in range(0, min(used, xyzs.shape[0]), 1 << 24):          # the network in slices: a full frame is hundreds of millions of samples
            end = min(at + (1 << 24), used, xyzs.shape[0])
            sigmas[at:end] = (model.density_scale * model(xyzs[at:end], dirs[at:end])[0]).float()
        del xyzs, dirs
    scale = 1 / (fars - nears)
    M, N = sigmas.shape[0], rays.shape[0]
    rows, inside, index = gather_plan(rays, M)
    scale_rows = torch.where(inside.any(dim=1), scale[index], torch.zeros_like(scale))[:, None]      # (a ray that misses the box: 1 / 0, and no samples)
    res = {}

    def hip():
        s = sigmas.detach().requires_grad_(True)
        loss = raymarching.distortion_rays_train(s, deltas, rays, scale)
        loss.backward()
        res["hip"] = (loss.detach(), s.grad)

    def chain():
        s = sigmas.detach().requires_grad_(True)
        loss = torch_chain(s, deltas, scale_rows, rows, inside, N)
        loss.backward()
        res["torch"] = (loss.detach(), s.grad)

    t_hip, t_torch = [], []
    for _ in range(3):                       # alternated
        t_hip.append(round(time_ms(hip, reps), 4))
        t_torch.append(round(time_ms(chain, max(reps // 10, 2)), 4))
    gmax = float(res["torch"][1].abs().max())
    return {"bench": "distortion_operator", "what": what, "rays": N, "samples": used, "rows": M, "longest_ray": int(rays[:, 2].max().item()),
            "hip_fwd_bwd_ms": t_hip, "torch_dense_fwd_bwd_ms": t_torch,
            # what the HIP node has to move: sigma 4 + deltas 8 bytes per sample once forward, twice backward (rays over 64 samples: three
            # times), 4 bytes of gradient; rows of dead samples are zero-filled by a memset of the whole gradient
            "hip_algorithmic_bytes": int(used * (12 + 2 * 12 + 4) + M * 4),
            "loss_hip": float(res["hip"][0]), "loss_torch": float(res["torch"][0]),
            "grad_max_abs_diff_over_max": float((res["hip"][1] - res["torch"][1]).abs().max()) / gmax if gmax > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        make_synthetic_dataset.make(root, a.size, a.views, 1, 1, rgba=True)
        opt = SimpleNamespace(path=root, preload=True, scale=1.0, offset=[0, 0, 0], bound=2, fp16=True, num_rays=a.rays, rand_pose=-1, error_map=False,
                              color_space="srgb", update_extra_interval=16, iters=30000, cuda_ray=True, dt_gamma=0, max_steps=1024, lambda_distort=0)
        loader = NeRFDataset(opt, dev, type="train").dataloader()
    sc = StonehengeScene(H=a.size, W=a.size, bound=2)
    student = sc.build_model(dev, table_seed=1)
    student.encoder.reset_parameters()
    student.reset_extra_state()
    trainer = Trainer("ngp", opt, student, device=dev, workspace=None, criterion=torch.nn.MSELoss(reduction="none"), fp16=True, ema_decay=0.95,
                      optimizer=lambda m: Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15),
                      lr_scheduler=lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda it: 0.1 ** min(it / opt.iters, 1)),
                      scheduler_update_every_step=True, mute=True, use_tensorboardX=False)
    student.mark_untrained_grid(loader._data.poses, loader._data.intrinsics)
    for lam in (0, 1e-3, 0):                             # warm-up of both forms: the occupancy grid's 16 full sweeps are over after 256 steps
        opt.lambda_distort = lam
        trainer.epoch += 1
        trainer.train_one_epoch(loader)
    rates = {0: [], 1e-3: []}
    for _ in range(a.rounds):
        for lam in (0, 1e-3):
            opt.lambda_distort = lam
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.epoch += 1
            trainer.train_one_epoch(loader)
            torch.cuda.synchronize()
            rates[lam].append(round(len(loader) / (time.perf_counter() - t0), 1))
    lines = [{"bench": "distortion_trainer", "size": a.size, "views": a.views, "rays": a.rays, "steps_per_s_lambda_0": rates[0],
              "steps_per_s_lambda_1e-3": rates[1e-3], "final_epoch_loss": trainer.stats["loss"][-1], "mean_count": int(student.mean_count),
              "device": torch.cuda.get_device_name(0)}]

    student.train()
    poses = torch.from_numpy(sc.poses).to(dev)
    frame = get_rays(poses[3:4], sc.intrinsics, a.size, a.size)
    o, d = frame["rays_o"].view(-1, 3).contiguous(), frame["rays_d"].view(-1, 3).contiguous()
    pick = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(0))[:a.rays].to(dev)
    lines.append(operator_line(student, o[pick].contiguous(), d[pick].contiguous(), int(student.mean_count), 200, f"training batch, {a.rays} rays"))
    per_ray = max(int(student.mean_count) // a.rays, 1)
    lines.append(operator_line(student, o, d, 2 * per_ray * o.shape[0], 20, f"full {a.size} x {a.size} frame"))
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
