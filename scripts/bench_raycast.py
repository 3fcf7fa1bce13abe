#!/usr/bin/env python3
"""Timings of the ground-truth camera (nerfsafetyvalidation_amd/world.py, csrc/raycast.hip) on one GPU, one JSON line each, also
written to profiles/raycast_bench.jsonl.  One 800 x 800 frame of scene.henge_mesh at two mesh resolutions; per mesh:

  build        ms of MeshWorld(...) on device tensors (pack, count, scan, emit, sort, start table; host clock around a synchronise,
               median of the repeats), the triangle count, the grid dimensions, the pairs and the mean pairs per cell
  frame        ms of cast + shade and of the cast alone, between stream events, median and min of the repeats, with frame_width
               (8 x 8 pixel tiles per wave) and without (row-major), the two alternating in one loop; whether both give the same bits
  layout       the cast reading triangles through the index list (what MeshWorld builds) against a copy of the triangle rows laid out
               in pair order, alternating
  brute_force  the same rule as chunked torch operators on the same GPU, on every `--stride`-th pixel of the frame in both
               directions (the full frame against 10^5 triangles is minutes of elementwise kernels), next to the grid cast of the same
               rays, and whether the two agree
  nerf_frame   the model's own render of that frame (the synthetic scene's network, occupancy-grid renderer under autocast, as the
               rollout renders it), for scale
and once: `slips`, the background pixels of six 256 x 256 frames (a cube map) seen from a point inside the closed ground slab of the
mesh -- every such ray must hit, a miss is a ray that slipped between two triangles at a shared edge (a recorded figure).

    python scripts/bench_raycast.py [--size 800] [--resolutions 64 128] [--repeats 30] [--stride 8] [--out profiles/raycast_bench.jsonl]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn, repeats, warmup=3):
    """ms of fn() between two events on the current stream, per repeat"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternating_ms(fns, repeats, warmup=3):
    """the same for several variants, one after the other inside every round -> one list per variant"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "repeats": len(ms)}


def torch_brute_force(o, d, tri, chunk_pairs=1 << 25):
    """world.cast_numpy's rule as torch operators on the device (float32, one operator per operation): -> t, prim"""
    F = tri.shape[0]
    v0, e1, e2 = [[tri[None, :, k + j] for j in range(3)] for k in (0, 4, 8)]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    ts, prims = [], []
    inf = torch.tensor(float("inf"), device=o.device)
    for i in range(0, o.shape[0], max(1, chunk_pairs // F)):
        oc = [o[i:i + max(1, chunk_pairs // F), k, None] for k in range(3)]
        dc = [d[i:i + max(1, chunk_pairs // F), k, None] for k in range(3)]
        p = cross(dc, e2)
        det = dot(e1, p)
        inv = 1.0 / det
        s = [oc[k] - v0[k] for k in range(3)]
        u = dot(s, p) * inv
        q = cross(s, e1)
        v = dot(dc, q) * inv
        t = dot(e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        tm = torch.where(ok, t, inf)
        best, prim = tm.min(1)                     # (ties: torch's min reports one of the closest; only t is compared below)
        ts.append(best)
        prims.append(torch.where(torch.isinf(best), torch.full_like(prim, -1), prim))
    return torch.cat(ts), torch.cat(prims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh, look_at_poses
    from nerfsafetyvalidation_amd.world import MeshWorld
    device = torch.device("cuda:0")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    S = args.size
    sc = StonehengeScene(H=S, W=S, bound=2)
    pose = torch.from_numpy(sc.poses[47]).to(device)
    rays = get_rays(pose[None], sc.intrinsics, S, S)
    o, d = rays["rays_o"].reshape(-1, 3).contiguous(), rays["rays_d"].reshape(-1, 3).contiguous()
    sub = (torch.arange(0, S, args.stride, device=device)[:, None] * S + torch.arange(0, S, args.stride, device=device)[None, :]).reshape(-1)
    o_sub, d_sub = o[sub].contiguous(), d[sub].contiguous()
    frame_ms = {}

    for R in args.resolutions:
        t0 = time.perf_counter()
        v, f, c = henge_mesh(R)
        mesh_s = time.perf_counter() - t0
        tv, tf, tc = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device)
        MeshWorld(tv, tf, tc)
        build = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            world = MeshWorld(tv, tf, tc)
            torch.cuda.synchronize()
            build.append((time.perf_counter() - t0) * 1e3)
        emit({"bench": "build", "mesh_resolution": R, "triangles": world.n_faces, "vertices": world.n_vertices, "grid": list(world.dims),
              "pairs": world.pairs, "mean_pairs_per_cell": round(world.mean_pairs_per_cell, 3), "henge_mesh_host_s": round(mesh_s, 2),
              **stats(build)})

        def frame(width):
            hit = world.cast(o, d, frame_width=width)
            return hit, world.shade(d, hit)

        tiled, rowmajor, cast_tiled, cast_rowmajor = alternating_ms(
            [lambda: frame(S), lambda: frame(None), lambda: world.cast(o, d, frame_width=S), lambda: world.cast(o, d)], args.repeats)
        (hit_a, img_a), (hit_b, img_b) = frame(S), frame(None)
        same = all(torch.equal(hit_a[k].view(torch.int32), hit_b[k].view(torch.int32)) for k in hit_a) and torch.equal(img_a[0], img_b[0])
        frame_ms[R] = statistics.median(tiled)
        emit({"bench": "frame", "mesh_resolution": R, "size": S, "rays": S * S, "hit_fraction": round(float((hit_a["prim"] >= 0).float().mean()), 4),
              "cast_shade_tiles": stats(tiled), "cast_shade_row_major": stats(rowmajor), "cast_tiles": stats(cast_tiled),
              "cast_row_major": stats(cast_rowmajor), "row_major_over_tiles": round(statistics.median(rowmajor) / statistics.median(tiled), 3),
              "same_bits": bool(same), "mrays_per_s_cast_shade_tiles": round(S * S / statistics.median(tiled) / 1e3, 1)})

        # the other triangle layout: a copy of the triangle rows in pair order (48 bytes per pair, a cell's triangles contiguous)
        # read through an identity index list -- the same kernel, the memory pattern of a cast that needs no indirection
        ordered = copy.copy(world)
        ordered.tri_data = world.tri_data[world.pair_tri.long()].contiguous()
        ordered.pair_tri = torch.arange(world.pairs, dtype=torch.int32, device=device)
        ordered.n_faces = world.pairs
        by_index, by_pair = alternating_ms([lambda: world.cast(o, d, frame_width=S), lambda: ordered.cast(o, d, frame_width=S)], args.repeats)
        same_t = torch.equal(world.cast(o, d, frame_width=S)["t"], ordered.cast(o, d, frame_width=S)["t"])
        emit({"bench": "layout", "mesh_resolution": R, "cast_index_list": stats(by_index), "cast_pair_order_copy": stats(by_pair),
              "pair_order_over_index": round(statistics.median(by_pair) / statistics.median(by_index), 3), "same_t": bool(same_t),
              "index_list_bytes": 4 * world.pairs + 48 * world.n_faces, "pair_order_bytes": 52 * world.pairs})

        brute = event_ms(lambda: torch_brute_force(o_sub, d_sub, world.tri_data), 3, warmup=1)
        grid_sub = event_ms(lambda: world.cast(o_sub, d_sub), args.repeats)
        bt, _ = torch_brute_force(o_sub, d_sub, world.tri_data)
        agree = bool(torch.equal(bt, world.cast(o_sub, d_sub)["t"]))
        emit({"bench": "brute_force", "mesh_resolution": R, "rays": int(sub.numel()), "stride": args.stride, "triangles": world.n_faces,
              "torch_brute_force": stats(brute), "grid_cast_same_rays": stats(grid_sub),
              "brute_over_grid": round(statistics.median(brute) / statistics.median(grid_sub), 1), "same_t": agree})

    model = sc.build_model(device)

    def nerf_frame():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1, perturb=False, frame_width=S)["image"]

    nerf = event_ms(nerf_frame, 10)
    emit({"bench": "nerf_frame", "size": S, **stats(nerf),
          "nerf_over_world_frame": {str(R): round(statistics.median(nerf) / ms, 2) for R, ms in frame_ms.items()}})

    # rays that slip between triangles: from inside the closed ground slab every ray must hit
    v, f, c = henge_mesh(args.resolutions[0])
    world = MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device))
    eye = np.array([0.1, -0.33, 0.1])
    n, total, missed = 256, 0, 0
    K = np.array([n / 2, n / 2, n / 2, n / 2], np.float64)            # a 90 degree field of view: six frames tile the sphere
    for centre in np.concatenate([np.eye(3), -np.eye(3)]) + np.array([1e-3, 2e-3, -1e-3]):
        cam = look_at_poses(centre[None])[0]                            # at `centre` looking at 0: turn it round
        cam[:3, 3] = eye
        prim = world.render(torch.from_numpy(cam).float(), K, n, n)["prim"]
        total += prim.numel()
        missed += int((prim < 0).sum())
    emit({"bench": "slips", "mesh_resolution": args.resolutions[0], "eye": eye.tolist(), "rays": total, "background_pixels": missed})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
