#!/usr/bin/env python3
"""Timings of the trajectory planner (nav.Planner) on one GPU, one JSON line each:

  learn_update   ms per learn_update (250 epochs, envConfig.json): the collision term as the torch composition (validate.py's
                 density_fn on the world points: the fused per-point density) or as the collision kernel (ngp_planner_collision),
                 each eagerly or replayed from a captured graph (capture included).  The kernel pair is not captured (nav/quad_plot.py:
                 its capture crashes hipGraph instantiation), so its graphed form is reported as unavailable.
  init           ms for a_star_init + learn_init (1000 epochs), the planner's default (graphed)
  rollout_step   ms per rollout step (64 x 64 frame, 64 samples per ray, the render under run_rollout's default fp16 autocast) with
                 the planner (default: graphed epochs) and without it (the hover stand-in)

The network is tests/golden/planner.npz's (the planner fixture: a third of the A* cells occupied).

    python scripts/bench_planner_rollout.py [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def network(f, device):
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    net = NeRFNetwork(encoding="hashgrid", bound=int(f["bound"]), cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1)
    g = torch.Generator().manual_seed(int(f["table_seed"]))
    net.encoder.embeddings.data.copy_(torch.rand(net.encoder.embeddings.shape, generator=g) - 0.5)
    for i, l in enumerate(net.sigma_net):
        l.weight.data.copy_(torch.from_numpy(f[f"sigma{i}"]))
    for i, l in enumerate(net.color_net):
        l.weight.data.copy_(torch.from_numpy(f[f"color{i}"]))
    net = net.to(device).eval()
    net.requires_grad_(False)
    return net


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import nav
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd import scene as SC
    device = torch.device("cuda:0")
    f = np.load(os.path.join(ROOT, "tests", "golden", "planner.npz"), allow_pickle=False)
    net = network(f, device)
    rot = torch.tensor(RO.PLANNER_ROT, device=device)
    cfg = RO.planner_config(device)
    base = nav.Planner(cfg["start_state"], cfg["end_state"], cfg, nav.density_query(net, rot))
    base.a_star_init(generator=torch.Generator().manual_seed(0))
    S = base.calc_everything()[0].shape[0]

    for kernel in (False, True):
        for graphs in (False, True):
            name = f"{'collision_kernel' if kernel else 'composition'}_{'graphed' if graphs else 'eager'}"
            if kernel and graphs:
                print(json.dumps({"bench": "planner_learn_update", "form": name, "available": False,
                                  "reason": "the collision kernel pair is not captured; a graphed epoch uses the composition"}), flush=True)
                continue
            times = []
            for _ in range(args.repeats):
                p = RO.copy_plan(base)
                p.use_graphs, p.fused_collision = graphs, kernel
                times.append(timed(lambda: p.learn_update(0)))
            print(json.dumps({"bench": "planner_learn_update", "form": name, "epochs": cfg["epochs_update"], "states": S,
                              "body_points": int(base.robot_body.shape[0]), "ms": round(min(times), 3),
                              "ms_per_epoch": round(min(times) / cfg["epochs_update"], 4), "all_ms": [round(t, 3) for t in times]}), flush=True)

    def init():
        p = nav.Planner(cfg["start_state"], cfg["end_state"], cfg, nav.density_query(net, rot))
        p.a_star_init(generator=torch.Generator().manual_seed(0))
        p.learn_init()
    t_init = min(timed(init) for _ in range(2))
    print(json.dumps({"bench": "planner_init", "form": "default_graphed", "epochs_init": cfg["epochs_init"], "ms": round(t_init, 3)}), flush=True)

    H = W = 64
    kw = dict(num_steps=64, upsample_steps=0, max_ray_batch=4096)
    steps = 4
    plan0 = RO.initial_plan(net, cfg, 0)
    for with_planner in (False, True):
        times = []
        for _ in range(2):
            sim = RO.RolloutSimulator(net, SC.intrinsics(H, W), H, W, steps, seed=0, render_kwargs=kw,
                                      planner_cfg=cfg if with_planner else None, initial_plan=plan0 if with_planner else None)
            with torch.autocast("cuda", dtype=torch.float16):       # as run_rollout(autocast=True), its default
                times.append(timed(lambda: sim.run(0)) / steps)
        print(json.dumps({"bench": "rollout_step", "planner": with_planner, "frame": [H, W], "samples_per_ray": 64, "steps": steps,
                          "autocast": "fp16 render, fp32 plan", "ms_per_step": round(min(times), 3)}), flush=True)


if __name__ == "__main__":
    main()
