#!/usr/bin/env python3
"""Depth supervision on the MI355X: (1) forward + backward of the HIP node (raymarching.depth_rays_train) against the same computation
as torch operators on the same GPU -- gather the packed samples to dense [N, longest ray], cumprod / cumsum, autograd -- on a training
batch (4096 rays) of a student trained on the mesh world's frames; (2) Trainer steps/s with both weights 0 (the path of the commit before
the term existed: the depth maps are not even read) and with --lambda_depth / --lambda_free on, alternated in one process over
`--rounds` rounds so that the run-to-run spread shows; (3) the fused target gather (ngp_train_depth_targets) against the torch form.
Appends the lines to profiles/depth_loss_bench.jsonl.

    python scripts/bench_depth_loss.py [--size 400] [--views 50] [--rounds 4] [--out profiles/depth_loss_bench.jsonl]"""
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

import make_mesh_dataset
from bench_distortion import gather_plan, time_ms
from nerfsafetyvalidation_amd import raymarching
from nerfsafetyvalidation_amd.nerf import targets
from nerfsafetyvalidation_amd.nerf.provider import NeRFDataset
from nerfsafetyvalidation_amd.nerf.trainer import Trainer
from nerfsafetyvalidation_amd.optim import Adam
from nerfsafetyvalidation_amd.scene import StonehengeScene

MARGIN, A, B = 0.02, 0.1, 0.01


def torch_chain(sigmas, deltas, z_rows, scale_rows, rows, inside, n_rays):
    """the operator's definition with torch operators on dense [N, T] (rows / inside: the gather plan, built once outside the timing)"""
    sg, dt, gap = sigmas[rows] * inside, deltas[rows, 0] * inside, deltas[rows, 1] * inside
    alpha = 1 - torch.exp(-sg * dt)
    T = torch.cumprod(1 - alpha, dim=1)
    T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], dim=1)
    w = alpha * T * (T >= 1e-4) * inside
    t = torch.cumsum(gap, dim=1)
    valid = z_rows > 0
    surface = valid & torch.isfinite(z_rows)
    d = (w * t).sum(dim=1, keepdim=True)
    front = (w * (t < z_rows - MARGIN)).sum(dim=1, keepdim=True)
    miss = torch.where(surface, scale_rows * (d - torch.where(surface, z_rows, torch.zeros_like(z_rows))), torch.zeros_like(d))
    return (A * (miss * miss).sum() + B * torch.where(valid, front, torch.zeros_like(front)).sum()) / n_rays


def operator_line(model, batch, depth, mean_count, reps):
    origins, directions = batch["rays_o"].view(-1, 3).contiguous(), batch["rays_d"].view(-1, 3).contiguous()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        nears, fars = raymarching.near_far_from_aabb(origins, directions, model.aabb_train, model.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=origins.device)
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(origins, directions, model.bound, model.density_bitfield, model.cascade,
                                                                model.grid_size, nears, fars, counter, mean_count, False, 128, False, 0, 1024)
        used = int(counter[0].item())
        sigmas = (model.density_scale * model(xyzs, dirs)[0]).float()
    scale = 1 / (fars - nears)
    target = model.march_depth_target(depth.view(-1), nears)
    M, N = sigmas.shape[0], rays.shape[0]
    rows, inside, index = gather_plan(rays, M)
    any_row = inside.any(dim=1)
    scale_rows = torch.where(any_row, scale[index], torch.zeros_like(scale))[:, None]
    z_rows = torch.where(any_row, target[index], torch.zeros_like(target))[:, None]
    res = {}

    def hip():
        s = sigmas.detach().requires_grad_(True)
        loss = raymarching.depth_rays_train(s, deltas, rays, target, MARGIN, scale, A, B)
        loss.backward()
        res["hip"] = (loss.detach(), s.grad)

    def chain():
        s = sigmas.detach().requires_grad_(True)
        loss = torch_chain(s, deltas, z_rows, scale_rows, rows, inside, N)
        loss.backward()
        res["torch"] = (loss.detach(), s.grad)

    t_hip, t_torch = [], []
    for _ in range(3):                       # alternated
        t_hip.append(round(time_ms(hip, reps), 4))
        t_torch.append(round(time_ms(chain, max(reps // 10, 2)), 4))
    gmax = float(res["torch"][1].abs().max())
    return {"bench": "depth_loss_operator", "what": f"training batch, {N} rays", "rays": N, "samples": used, "rows": M,
            "longest_ray": int(rays[:, 2].max().item()), "surface_rays": int((torch.isfinite(target) & (target > 0)).sum()),
            "empty_rays": int(torch.isinf(target).sum()), "hip_fwd_bwd_ms": t_hip, "torch_dense_fwd_bwd_ms": t_torch,
            # what the HIP node has to move: sigma 4 + deltas 8 bytes per sample once forward and once backward, 4 bytes of gradient;
            # rows of dead samples are zero-filled by a memset of the whole gradient
            "hip_algorithmic_bytes": int(used * (12 + 12 + 4) + M * 4),
            "loss_hip": float(res["hip"][0]), "loss_torch": float(res["torch"][0]),
            "grad_max_abs_diff_over_max": float((res["hip"][1] - res["torch"][1]).abs().max()) / gmax if gmax > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = dict(preload=True, scale=1.0, offset=[0, 0, 0], bound=2, fp16=True, num_rays=a.rays, rand_pose=-1, error_map=False, color_space="srgb",
                update_extra_interval=16, iters=30000, cuda_ray=True, dt_gamma=0, max_steps=1024, depth_margin=MARGIN)
    with tempfile.TemporaryDirectory() as root:
        make_mesh_dataset.make(root, a.size, a.views, 1, 1, device="cuda:0", depth=True)
        opt_off = SimpleNamespace(path=root, lambda_depth=0, lambda_free=0, **base)
        opt_on = SimpleNamespace(path=root, lambda_depth=A, lambda_free=B, **base)
        loaders = {"off": NeRFDataset(opt_off, dev, type="train").dataloader(), "on": NeRFDataset(opt_on, dev, type="train").dataloader()}
    assert loaders["off"]._data.depths is None and loaders["on"]._data.depths is not None
    sc = StonehengeScene(H=a.size, W=a.size, bound=2)
    student = sc.build_model(dev, table_seed=1)
    student.encoder.reset_parameters()
    student.reset_extra_state()
    opt = SimpleNamespace(**vars(opt_off))
    trainer = Trainer("ngp", opt, student, device=dev, workspace=None, criterion=torch.nn.MSELoss(reduction="none"), fp16=True, ema_decay=0.95,
                      optimizer=lambda m: Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15),
                      lr_scheduler=lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda it: 0.1 ** min(it / opt.iters, 1)),
                      scheduler_update_every_step=True, mute=True, use_tensorboardX=False)
    student.mark_untrained_grid(loaders["on"]._data.poses, loaders["on"]._data.intrinsics)

    def epoch(which):
        opt.lambda_depth, opt.lambda_free = (A, B) if which == "on" else (0, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.epoch += 1
        trainer.train_one_epoch(loaders[which])
        torch.cuda.synchronize()
        return round(len(loaders[which]) / (time.perf_counter() - t0), 1)

    warm = max(1, -(-256 // a.views))            # the occupancy grid's 16 full sweeps are over after 256 steps
    for _ in range(warm):
        epoch("off")
    epoch("on")
    rates = {"off": [], "on": []}
    for _ in range(a.rounds):
        for which in ("off", "on"):
            rates[which].append(epoch(which))
    lines = [{"bench": "depth_loss_trainer", "size": a.size, "views": a.views, "rays": a.rays, "lambda_depth": A, "lambda_free": B, "margin": MARGIN,
              "steps_per_s_off": rates["off"], "steps_per_s_on": rates["on"], "final_epoch_loss": trainer.stats["loss"][-1],
              "last_loss_depth": float(trainer.last_loss_depth.detach()), "last_loss_depth_parts": [float(v) for v in trainer.last_loss_depth_parts],
              "mean_count": int(student.mean_count), "device": torch.cuda.get_device_name(0)}]

    student.train()
    batch = next(iter(loaders["on"]))
    depth = targets.training_depth_targets(batch["depth"])
    lines.append(operator_line(student, batch, depth, int(student.mean_count), 200))
    t_fused = [round(time_ms(lambda: targets.training_depth_targets(batch["depth"]), 500), 4) for _ in range(3)]
    t_torch = [round(time_ms(lambda: batch["depth"].materialize(), 500), 4) for _ in range(3)]
    lines.append({"bench": "depth_targets", "rays": int(depth.numel()), "fused_ms": t_fused, "torch_ms": t_torch,
                  "max_abs_diff": float((torch.nan_to_num(depth, posinf=0.0) - torch.nan_to_num(batch["depth"].materialize(), posinf=0.0)).abs().max())})
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
