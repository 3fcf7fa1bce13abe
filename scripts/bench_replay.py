#!/usr/bin/env python3
"""Timings of the failure replay (nerfsafetyvalidation_amd/replay.py, world.MeshWorld.render_scene, csrc/overlay.hip) on one GPU, one
JSON line each, also written to profiles/replay_bench.jsonl:

  scene         an 800 x 800 MeshWorld.render_scene of scene.henge_mesh(64) with the primitives of a 12-step planned trajectory
                (replay.failure_primitives of synthetic plans: the initial plan and 12 replans of 12 points each, 12 cubes), next to
                MeshWorld.render alone, the two alternating in one loop; ms between stream events, median and min of the repeats
  overlay_cast  the overlay cast alone (those rays, those primitives, the mesh's t as the far limit) with 8 x 8 pixel tiles and
                row-major, next to the same rule as chunked torch operators on the same GPU, and whether the two agree in every bit
                of t; the useful arithmetic per second from a count of the rule's operations
  replay        a whole run_replay of a small Monte-Carlo run (the synthetic scene's network at 64 x 64, hover stand-in, sdf="world"
                built once outside the timed region): host clock around a synchronise, without and with the views

    python scripts/bench_replay.py [--size 800] [--repeats 30] [--out profiles/replay_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_raycast import alternating_ms, event_ms, stats  # noqa: E402

# the rule's floating-point operations per (ray, primitive), counted from csrc/overlay.hip: a capsule (three re-centrings, the body's
# two cross products and quadratic, two caps of 43 each) about 180, a box (one re-centring, three slabs of 10) about 48
FLOP_CAPSULE, FLOP_BOX = 180, 48


def torch_overlay(o, d, prims, t_max, chunk_pairs=1 << 24):
    """world.overlay_terms + the acceptance as torch operators on the device (float32, one operator per operation) -> t, prim"""
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    P = prims.shape[0]
    kind, r = prims[None, :, 0], prims[None, :, 7]
    a, b = [prims[None, :, 1 + k] for k in range(3)], [prims[None, :, 4 + k] for k in range(3)]
    inf = torch.tensor(float("inf"), device=o.device)
    ts, ps = [], []
    step = max(1, chunk_pairs // max(1, P))
    for i in range(0, o.shape[0], step):
        oc, dc = [o[i:i + step, k, None] for k in range(3)], [d[i:i + step, k, None] for k in range(3)]
        dd = dot(dc, dc)
        inv_dd = 1.0 / dd

        def centred(c):
            t0 = dot(dc, [c[k] - oc[k] for k in range(3)]) * inv_dd
            return t0, [(oc[k] + t0 * dc[k]) - c[k] for k in range(3)]

        m = [(a[k] + b[k]) * 0.5 for k in range(3)]
        t0, qm = centred(m)
        ba = [b[k] - a[k] for k in range(3)]
        oa = [qm[k] + (m[k] - a[k]) for k in range(3)]
        baba, rr = dot(ba, ba), r * r
        u, w = cross(ba, dc), cross(ba, oa)
        A, B = dot(u, u), dot(u, w)
        C = dot(w, w) - rr * baba
        h = B * B - A * C
        tp = (-B - torch.sqrt(h)) / A
        y = dot(ba, oa) + tp * dot(ba, dc)
        t = torch.where((A > 0) & (h >= 0) & (y > 0) & (y < baba), t0 + tp, inf)
        for c in (a, b):
            t0, p = centred(c)
            Bs = dot(dc, p)
            hs = Bs * Bs - dd * (dot(p, p) - rr)
            tc = t0 + (-Bs - torch.sqrt(hs)) / dd
            t = torch.where((hs >= 0) & (tc < t), tc, t)
        t0, pb = centred(a)
        t_near, t_far = torch.full_like(t, -float("inf")), torch.full_like(t, float("inf"))
        miss = torch.zeros_like(t, dtype=torch.bool)
        for k in range(3):
            still = (dc[k] == 0).expand_as(t)
            miss = miss | (still & (pb[k].abs() > b[k]))
            inv = 1.0 / dc[k]
            t1, t2 = (-b[k] - pb[k]) * inv, (b[k] - pb[k]) * inv
            lo = torch.fmin(t1, t2)
            t_near = torch.where(~still & (lo > t_near), lo, t_near)
            t_far = torch.where(~still, torch.fmin(t_far, torch.fmax(t1, t2)), t_far)
        tb = torch.where(~miss & (t_near <= t_far), t0 + t_near, inf)
        t = torch.where(kind == 0, t, tb)
        ok = (t > 0) & (t < t_max[i:i + step, None])
        tm = torch.where(ok, t, inf)
        best, prim = tm.min(1)                     # (ties: torch's min reports one of the closest; only t is compared)
        ts.append(best)
        ps.append(torch.where(torch.isinf(best), torch.full_like(prim, -1), prim))
    return torch.cat(ts), torch.cat(ps)


def synthetic_plans(steps=12, points=12, seed=0):
    """the plans of a `steps`-step planned flight from ENV's start to its end: the initial plan a bowed line, every replan the rest of
    the previous one bent a little -> (plans: 1 + steps arrays [points, 3], rows: `steps` replay rows at the plan's way points)"""
    from nerfsafetyvalidation_amd import replay as RP
    from nerfsafetyvalidation_amd import rollout as RO
    rng = np.random.default_rng(seed)
    start, end = np.array(RO.ENV["start_pos"]), np.array(RO.ENV["end_pos"])
    s = np.linspace(0, 1, points)[:, None]
    plan = start + (end - start) * s + np.array([0.0, 0.0, 0.15]) * np.sin(np.pi * s)
    plans, rows = [plan], np.zeros((steps, RP.REPLAY_ROW_WIDTH))
    for k in range(steps):
        here = plans[-1][0] + (plans[-1][-1] - plans[-1][0]) / (steps - k + 1) + rng.normal(0, 0.01, 3)
        plans.append(here + (end - here) * s + np.array([0.0, 0.0, 0.15 * (1 - k / steps)]) * np.sin(np.pi * s) + rng.normal(0, 0.004, (points, 3)))
        rows[k, 1], rows[k, 15:18] = k, here
    rows[-1, 20] = rows[:, 21] = 1
    return plans, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import replay as RP
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh
    from nerfsafetyvalidation_amd.world import MeshWorld, overlay_prims
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    S = args.size
    v, f, c = henge_mesh(64)
    world = MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device))
    plans, rows = synthetic_plans()
    tubes, boxes = RP.failure_primitives(rows, plans)
    prims, colors = overlay_prims(tubes, boxes)
    n_capsules, n_boxes = int((prims[:, 0] == 0).sum()), int((prims[:, 0] == 1).sum())
    pose, K = RP.overview_camera(S, S)

    scene_ms, render_ms = alternating_ms([lambda: world.render_scene(pose, K, S, S, tubes=tubes, boxes=boxes), lambda: world.render(pose, K, S, S)],
                                         args.repeats)
    out = world.render_scene(pose, K, S, S, tubes=tubes, boxes=boxes)
    emit({"bench": "scene", "size": S, "rays": S * S, "triangles": world.n_faces, "primitives": int(prims.shape[0]), "capsules": n_capsules,
          "boxes": n_boxes, "overlay_pixels": int((out["overlay_prim"] >= 0).sum()), "mesh_pixels": int((out["prim"] >= 0).sum()),
          "render_scene": stats(scene_ms), "render": stats(render_ms),
          "scene_over_render": round(statistics.median(scene_ms) / statistics.median(render_ms), 3)})

    rays = get_rays(torch.from_numpy(pose).to(device)[None], K, S, S)
    o, d = rays["rays_o"].reshape(-1, 3).contiguous(), rays["rays_d"].reshape(-1, 3).contiguous()
    far = world.cast(o, d, frame_width=S)["t"]
    q = torch.from_numpy(prims).to(device)
    tiled, rowmajor, mesh_cast = alternating_ms([lambda: world.cast_overlay(o, d, prims, t_max=far, frame_width=S),
                                                 lambda: world.cast_overlay(o, d, prims, t_max=far), lambda: world.cast(o, d, frame_width=S)], args.repeats)
    brute = event_ms(lambda: torch_overlay(o, d, q, far), 3, warmup=1)
    bt, _ = torch_overlay(o, d, q, far)
    got = world.cast_overlay(o, d, prims, t_max=far, frame_width=S)
    flop = float(S * S) * (n_capsules * FLOP_CAPSULE + n_boxes * FLOP_BOX)
    emit({"bench": "overlay_cast", "size": S, "rays": S * S, "primitives": int(prims.shape[0]), "cast_tiles": stats(tiled), "cast_row_major": stats(rowmajor),
          "mesh_cast_tiles": stats(mesh_cast), "overlay_over_mesh_cast": round(statistics.median(tiled) / statistics.median(mesh_cast), 3),
          "torch_operators": stats(brute), "torch_over_kernel": round(statistics.median(brute) / statistics.median(tiled), 1),
          "same_t_bits": bool(torch.equal(bt.view(torch.int32), got["t"].view(torch.int32))),
          "rays_with_other_t_bits": int((bt.view(torch.int32) != got["t"].view(torch.int32)).sum()),
          "largest_t_difference": float(torch.nan_to_num(bt - got["t"], nan=0.0, posinf=0.0, neginf=0.0).abs().max()),
          "rule_gflop": round(flop / 1e9, 2), "rule_tflops_tiles": round(flop / statistics.median(tiled) / 1e9, 2)})

    # a whole replay of a small Monte-Carlo run
    H = W = 64
    n_sims, steps = 6, 6
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device)
    nerf_sdf = CO.SignedDistanceField.from_occupancy(CO.occupancy_from_fn(CO.henge_fn, CO.reference_box()), CO.reference_box())
    stress, _ = RO.run_rollout(model, sc.intrinsics, H, W, n_sims, steps, seed=1, sdf=nerf_sdf)
    t0 = time.perf_counter()
    truth = CO.SignedDistanceField.from_mesh(world)
    torch.cuda.synchronize()
    field_ms = (time.perf_counter() - t0) * 1e3

    def timed(**kw):
        out_ms = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = RP.run_replay(stress, None, sc.intrinsics, H, W, world=world, sdf=truth, seed=1, steps=steps, **kw)
            torch.cuda.synchronize()
            out_ms.append((time.perf_counter() - t0) * 1e3)
        return res, out_ms[1:]                         # (the first call warms up)

    res, plain_ms = timed()
    with tempfile.TemporaryDirectory() as tmp:
        _, views_ms = timed(views=tmp)
    emit({"bench": "replay", "size": H, "simulations": n_sims, "recorded_steps": int(stress.shape[0]), "replayed_steps": int(res.rows.shape[0]),
          "step_matrix_tn_fn_fp_tp": res.confusion_matrix("step").reshape(-1).tolist(), "traj_matrix_tn_fn_fp_tp": res.confusion_matrix("traj").reshape(-1).tolist(),
          "world_field_ms": round(field_ms, 2), "run_replay": stats(plain_ms), "run_replay_with_views": stats(views_ms),
          "ms_per_replayed_step": round(statistics.median(plain_ms) / max(1, res.rows.shape[0]), 3)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
