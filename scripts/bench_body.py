#!/usr/bin/env python3
"""Timings of the body collision test (csrc/body.hip; world.MeshWorld.box_overlap, collision.box_cells) on one GPU, one JSON line each,
also written to profiles/body_bench.jsonl:

  boxes_mesh    the body boxes of seeded trajectories (hover flights from ENV's start towards its end under the rollout's noise,
                4 interpolated poses per step) against scene.henge_mesh(R)'s triangles, exact; ms between stream events, median,
                min and max of the repeats after a warm-up; the same for 4 boxes per call (launch-bound: reported as such)
  boxes_cells   the same boxes against the world's occupancy map over collision.reference_box(); and 4 boxes per call
  numpy         the numpy paths (the rule's definition) on a subsample large enough to time, host clock, and that they agree
  rollout_step  run_rollout with body=BodyBox.planner() next to the same run with body=None (the default path), host clock around a
                synchronise, per simulated step -- and with exact=True
  verdicts      the share of colliding simulations of one seeded rollout with the body (cells, exact) and without it

    python scripts/bench_body.py [--mesh 256] [--boxes 100000] [--repeats 20] [--out profiles/body_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_raycast import event_ms  # noqa: E402


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def trajectory_states(n_boxes, steps=10, n_interp=4, seed=0, noise_scale=1.0):
    """n_boxes interpolated states [n, 6] (xyz, rotation vector) of seeded hover flights, rollout.drone_dynamics batched on the host"""
    from nerfsafetyvalidation_amd import rollout as RO
    sims = -(-n_boxes // (steps * n_interp))
    gen = torch.Generator().manual_seed(seed)
    state = RO.initial_state(steps).repeat(sims, 1)
    std = torch.tensor(RO.ENV["mpc_noise_std"]) * noise_scale
    hover = torch.tensor([RO.ENV["mass"] * RO.ENV["g"], 0.0, 0.0, 0.0]).repeat(sims, 1)
    hist = [state.numpy().astype(np.float64)]
    for _ in range(steps):
        state = RO.drone_dynamics(state, hover, RO.ENV["T_final"] / steps) + torch.normal(torch.zeros(sims, 12), std.repeat(sims, 1), generator=gen)
        hist.append(state.numpy().astype(np.float64))
    hist = np.stack(hist)                                              # [steps + 1, sims, 12]
    w = (np.arange(1, n_interp + 1) / n_interp)[None, :, None, None]
    poses = hist[:-1, None] * (1 - w) + hist[1:, None] * w             # [steps, n_interp, sims, 12]
    poses = poses.transpose(2, 0, 1, 3).reshape(-1, 12)[:n_boxes]
    return np.concatenate([poses[:, 0:3], poses[:, 6:9]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd import world as WO
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh
    if not torch.cuda.is_available():
        raise SystemExit("bench_body.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    body = CO.BodyBox.planner()
    v, f, c = henge_mesh(args.mesh)
    world = WO.MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device))
    grid = CO.reference_box()
    occ = world.occupancy(grid)
    boxes_host = CO.body_boxes(trajectory_states(args.boxes), body)
    boxes = torch.from_numpy(boxes_host).to(device)
    four = boxes[:4].contiguous()
    N = int(boxes.shape[0])

    prim = world.box_overlap(boxes)["prim"]
    emit({"bench": "boxes_mesh", "boxes": N, "triangles": world.n_faces, "grid": list(world.dims), "pairs": world.pairs,
          "hit_share": round(float((prim >= 0).float().mean()), 4), "all": spread(event_ms(lambda: world.box_overlap(boxes), args.repeats)),
          "four_per_call_launch_bound": spread(event_ms(lambda: world.box_overlap(four), args.repeats))})
    cell = CO.box_cells(boxes, occ, grid)
    emit({"bench": "boxes_cells", "boxes": N, "map": list(grid.shape), "occupied_cells": int(occ.sum()),
          "hit_share": round(float((cell >= 0).float().mean()), 4), "all": spread(event_ms(lambda: CO.box_cells(boxes, occ, grid), args.repeats)),
          "four_per_call_launch_bound": spread(event_ms(lambda: CO.box_cells(four, occ, grid), args.repeats))})

    # the numpy paths on a subsample: the brute force over all triangles is what defines the result, not a competitor
    n_mesh, n_cells = 16, 4000
    vw, faces = WO.vertices_to_world(v, CO.PLANNER_ROT), f
    t0 = time.perf_counter()
    ref_prim = WO.box_overlap_numpy(boxes_host[:n_mesh], vw, faces)["prim"]
    mesh_s = time.perf_counter() - t0
    occ_host = occ.cpu().numpy()
    t0 = time.perf_counter()
    ref_cell = CO.box_cells_numpy(boxes_host[:n_cells], occ_host, grid)
    cells_s = time.perf_counter() - t0
    emit({"bench": "numpy", "mesh_boxes": n_mesh, "mesh_ms_per_box": round(mesh_s * 1e3 / n_mesh, 3), "cells_boxes": n_cells,
          "cells_ms_per_box": round(cells_s * 1e3 / n_cells, 4), "same_prim": bool(np.array_equal(ref_prim, prim[:n_mesh].cpu().numpy())),
          "same_cell": bool(np.array_equal(ref_cell, cell[:n_cells].cpu().numpy()))})

    # a rollout step with the body on, against the default path
    H = W = 64
    n_sims, steps = 16, 6
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device)
    small = WO.MeshWorld(*[torch.from_numpy(a).to(device) for a in henge_mesh(64)])
    field = CO.SignedDistanceField.from_mesh(small)

    def timed(**kw):
        out_ms, rows = [], None
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows, _ = RO.run_rollout(model, sc.intrinsics, H, W, n_sims, steps, seed=1, sdf=field, world=small, in_flight=1, **kw)
            torch.cuda.synchronize()
            out_ms.append((time.perf_counter() - t0) * 1e3 / max(1, rows.shape[0]))
        return rows, out_ms[1:]                        # (the first call warms up)

    plain_ms, cells_ms, exact_ms = timed()[1], timed(body=body)[1], timed(body=body, exact=True)[1]
    emit({"bench": "rollout_step", "size": H, "simulations": n_sims, "steps": steps, "ms_per_step_body_none": spread(plain_ms),
          "ms_per_step_body_cells": spread(cells_ms), "ms_per_step_body_exact": spread(exact_ms)})
    many = 64

    def ever(**kw):
        rows, _ = RO.run_rollout(model, sc.intrinsics, H, W, many, steps, seed=1, sdf=field, world=small, in_flight=1, **kw)
        return round(float(np.mean([rows[rows[:, 0] == s][-1, -1] for s in range(many)])), 4)

    emit({"bench": "verdicts", "simulations": many, "steps": steps, "seed": 1, "colliding_share_centre_point": ever(),
          "colliding_share_body_cells": ever(body=body), "colliding_share_body_exact": ever(body=body, exact=True)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
