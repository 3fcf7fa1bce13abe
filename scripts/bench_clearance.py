#!/usr/bin/env python3
"""Timings of the body clearance (csrc/clearance.hip; world.MeshWorld.box_clearance, collision.box_cells_clearance) on one GPU, one
JSON line each, also written to profiles/clearance_bench.jsonl:

  clearance_mesh   bench_body.py's trajectory boxes against scene.henge_mesh(R)'s triangles at max_distance 0.1 / 0.25 / 1.0 m; ms
                   between stream events, median, min and max of the repeats after a warm-up; the same for 4 boxes per call; next
                   to them the verdict alone (box_overlap) on the same boxes
  clearance_cells  the same boxes against the world's occupancy map over collision.reference_box(); and 4 boxes per call
  numpy            the numpy paths (the rule's definition) on a subsample, host clock per box, and that they agree bit for bit
  rollout_step     run_rollout with body=BodyBox.planner() alone next to the same run with clearance=0.25, host clock around a
                   synchronise, per simulated step -- against the map and with exact=True

    python scripts/bench_clearance.py [--mesh 256] [--boxes 100000] [--repeats 20] [--out profiles/clearance_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_body import spread, trajectory_states  # noqa: E402
from bench_raycast import event_ms  # noqa: E402

MAX_DISTANCES = (0.1, 0.25, 1.0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd import world as WO
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh
    if not torch.cuda.is_available():
        raise SystemExit("bench_clearance.py measures on a GPU; none is available")
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

    def shares(out):
        hit = out["hit"] >= 0
        return {"hit_share": round(float(hit.float().mean()), 4), "accepted_gap_share": round(float((~hit & torch.isfinite(out["distance"])).float().mean()), 4)}

    emit({"bench": "verdict_alone", "boxes": N, "mesh": spread(event_ms(lambda: world.box_overlap(boxes), args.repeats)),
          "cells": spread(event_ms(lambda: CO.box_cells(boxes, occ, grid), args.repeats))})
    for D in MAX_DISTANCES:
        out = world.box_clearance(boxes, D)
        emit({"bench": "clearance_mesh", "max_distance": D, "boxes": N, "triangles": world.n_faces, "grid": list(world.dims), "pairs": world.pairs,
              **shares(out), "all": spread(event_ms(lambda: world.box_clearance(boxes, D), args.repeats)),
              "four_per_call": spread(event_ms(lambda: world.box_clearance(four, D), args.repeats))})
    for D in MAX_DISTANCES:
        out = CO.box_cells_clearance(boxes, occ, grid, D)
        emit({"bench": "clearance_cells", "max_distance": D, "boxes": N, "map": list(grid.shape), "occupied_cells": int(occ.sum()), **shares(out),
              "all": spread(event_ms(lambda: CO.box_cells_clearance(boxes, occ, grid, D), args.repeats)),
              "four_per_call": spread(event_ms(lambda: CO.box_cells_clearance(four, occ, grid, D), args.repeats))})

    # the numpy paths on a subsample: they define the result
    D = 0.25
    n_mesh, n_cells = 8, 64
    vw = WO.vertices_to_world(v, CO.PLANNER_ROT)
    t0 = time.perf_counter()
    ref = WO.box_clearance_numpy(boxes_host[:n_mesh], vw, f, D)
    mesh_s = time.perf_counter() - t0
    got = world.box_clearance(boxes[:n_mesh], D)
    same_mesh = bool(np.array_equal(bits(ref["distance"]), bits(got["distance"].cpu().numpy())) and np.array_equal(ref["prim"], got["prim"].cpu().numpy()))
    occ_host = occ.cpu().numpy()
    t0 = time.perf_counter()
    ref = CO.box_cells_clearance_numpy(boxes_host[:n_cells], occ_host, grid, D)
    cells_s = time.perf_counter() - t0
    got = CO.box_cells_clearance(boxes[:n_cells], occ, grid, D)
    same_cells = bool(np.array_equal(bits(ref["distance"]), bits(got["distance"].cpu().numpy())) and np.array_equal(ref["cell"], got["cell"].cpu().numpy()))
    emit({"bench": "numpy", "max_distance": D, "mesh_boxes": n_mesh, "mesh_ms_per_box": round(mesh_s * 1e3 / n_mesh, 3), "cells_boxes": n_cells,
          "cells_ms_per_box": round(cells_s * 1e3 / n_cells, 3), "same_mesh": same_mesh, "same_cells": same_cells})

    # a rollout step with the body alone and with its clearance
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
            rows, _ = RO.run_rollout(model, sc.intrinsics, H, W, n_sims, steps, seed=1, sdf=field, world=small, in_flight=1, body=body, **kw)
            torch.cuda.synchronize()
            out_ms.append((time.perf_counter() - t0) * 1e3 / max(1, rows.shape[0]))
        return rows, out_ms[1:]                        # (the first call warms up)

    cells_rows, cells_ms = timed()
    gap_rows, gap_ms = timed(clearance=D)
    exact_ms, exact_gap_ms = timed(exact=True)[1], timed(exact=True, clearance=D)[1]
    emit({"bench": "rollout_step", "size": H, "simulations": n_sims, "steps": steps, "clearance": D, "ms_per_step_body_cells": spread(cells_ms),
          "ms_per_step_clearance_cells": spread(gap_ms), "ms_per_step_body_exact": spread(exact_ms), "ms_per_step_clearance_exact": spread(exact_gap_ms),
          "same_verdicts": bool(np.array_equal(cells_rows[:, 22:], gap_rows[:, 22:])), "smallest_value_centre": round(float(cells_rows[:, 14].min()), 4),
          "smallest_value_clearance": round(float(gap_rows[:, 14].min()), 4)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
