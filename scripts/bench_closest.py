#!/usr/bin/env python3
"""Timings of the closest-point query and the surface-error report (nerfsafetyvalidation_amd/world.py MeshWorld.closest,
mesh.surface_error, csrc/closest.hip) on one GPU, one JSON line each, also written to profiles/closest_bench.jsonl.

Workload: the `--resolution`^3 isosurface of the synthetic Stonehenge model (bench_mesh.py's: the 95th percentile of the field as
the threshold, scaled to the model's bounds) against scene.henge_mesh(`--resolution`), both directions, max_distance = `--cells`
lattice cells.  The two surfaces have nothing to do with each other (the synthetic table is noise): most points are misses, which is
what max_distance is for; the henge mesh against itself moved by half a cell is the all-hits case.

  build        ms of MeshWorld(...) for both meshes, triangles, grid, pairs
  closest      per direction: ms of MeshWorld.closest between stream events (median, min, max of the repeats) in the points' own
               order and with the coherent sort, the two alternating in one loop; the same for the points shuffled; whether all
               give the same bits; hits; (point, triangle) pairs tested per point (mean, median, max) against F for brute force
  brute_force  the same rule as chunked torch operators on the same GPU on a subsample of the points (all of them would be 10^13
               pairs), next to the kernel on the same points, and whether the two agree
  numpy        world.closest_numpy on a smaller subsample (host clock), and whether it agrees with the kernel bit for bit
  stats        ngp_distance_stats on the accuracy distances against the same figures from torch operators
  surface_error  the whole report, host clock around a synchronise

    python scripts/bench_closest.py [--resolution 256] [--cells 3] [--repeats 10] [--out profiles/closest_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def alternating_ms(fns, repeats, warmup=2):
    """ms of each fn() between two events on the current stream, the variants one after the other inside every round"""
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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def torch_brute_force(p, tri, max_distance, chunk_pairs=1 << 24):
    """world.closest_numpy's rule as torch operators on the device (float32, one operator per operation): p [N,3], tri [F,3,3] ->
    distance [N] (+inf on a miss), prim [N]"""
    F = tri.shape[0]
    v0, v1, v2 = [[tri[None, :, j, k] for k in range(3)] for j in range(3)]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    inf, zero, one = [torch.tensor(x, device=p.device) for x in (float("inf"), 0.0, 1.0)]
    e1, e2 = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
    e12 = [v2[k] - v1[k] for k in range(3)]
    n = cross(e1, e2)
    nn = dot(n, n)
    lo = [torch.minimum(v0[k], torch.minimum(v1[k], v2[k])) for k in range(3)]
    hi = [torch.maximum(v0[k], torch.maximum(v1[k], v2[k])) for k in range(3)]
    rows = max(1, chunk_pairs // F)
    ds, prims = [], []
    for i in range(0, p.shape[0], rows):
        pc = [p[i:i + rows, k, None] for k in range(3)]
        s = [pc[k] - v0[k] for k in range(3)]
        sn = dot(s, n)
        b, c = dot(cross(s, e2), n) / nn, dot(cross(e1, s), n) / nn
        inside = (nn > 0) & (b >= 0) & (c >= 0) & (b + c <= 1)
        g = [torch.maximum(torch.maximum(lo[k] - pc[k], pc[k] - hi[k]), zero) for k in range(3)]
        box2, plane2 = dot(g, g), (sn * sn) / nn
        d2 = torch.where(inside, torch.where(plane2 >= box2, plane2, box2), inf)
        s1 = [pc[k] - v1[k] for k in range(3)]
        for ap, ab in ((s, e1), (s, e2), (s1, e12)):
            den = dot(ab, ab)
            t = torch.where(den == 0, zero, dot(ap, ab) / den)
            t = torch.where(t >= 0, t, zero)
            t = torch.where(t <= 1, t, one)
            r = [ap[k] - t * ab[k] for k in range(3)]
            sd = dot(r, r)
            d2 = torch.where(sd < d2, sd, d2)
        best, prim = d2.min(1)                       # (ties: torch's min reports one of the closest; only the distance is compared)
        dist = best.sqrt()
        hit = dist <= max_distance
        ds.append(torch.where(hit, dist, inf))
        prims.append(torch.where(hit, prim, torch.full_like(prim, -1)))
    return torch.cat(ds), torch.cat(prims)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--cells", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--brute-points", type=int, default=1024)
    ap.add_argument("--brute-pairs", type=float, default=2e9)
    ap.add_argument("--numpy-pairs", type=float, default=6e7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import mesh as M
    from nerfsafetyvalidation_amd import world as W
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh
    device = torch.device("cuda:0")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    R = args.resolution
    model = StonehengeScene(H=32, W=32, bound=2).build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    model.eval()
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]

    def query(pts):
        with torch.no_grad():
            return model.density(pts.to(device))["sigma"]

    u = M.extract_fields(lo, hi, R, query)
    sample = u.flatten()[torch.randperm(u.numel(), device=device, generator=torch.Generator(device).manual_seed(0))[:1 << 20]]
    thr = float(torch.quantile(sample, 0.95))
    iv, ifc = M.isosurface(u, thr)
    del u
    iv = (iv / (R - 1.0) * (hi - lo)[None] + lo[None]).to(torch.float32).contiguous()
    hv, hf, _ = henge_mesh(R)
    hv, hf = torch.from_numpy(hv).to(device), torch.from_numpy(hf).to(device)
    cell = float((hi - lo).max()) / (R - 1.0)
    md = args.cells * cell

    worlds = {}
    for name, (v, f) in (("isosurface", (iv, ifc)), ("henge", (hv, hf))):
        W.MeshWorld(v, f)
        build = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            worlds[name] = W.MeshWorld(v, f)
            torch.cuda.synchronize()
            build.append((time.perf_counter() - t0) * 1e3)
        w = worlds[name]
        emit({"bench": "build", "mesh": name, "resolution": R, "vertices": w.n_vertices, "triangles": w.n_faces, "grid": list(w.dims),
              "pairs": w.pairs, "mean_pairs_per_cell": round(w.mean_pairs_per_cell, 3), **stats(build)})

    def same_bits(a, b):
        return bool(torch.equal(a["distance"].view(torch.int32), b["distance"].view(torch.int32)) and torch.equal(a["prim"], b["prim"]))

    gen = torch.Generator(device).manual_seed(1)
    cases = (("accuracy", "isosurface vertices -> henge", iv, worlds["henge"], md),
             ("completeness", "henge vertices -> isosurface", hv, worlds["isosurface"], md),
             ("shifted", "henge vertices + half a cell -> henge", hv + 0.5 * cell, worlds["henge"], md))
    distances = {}
    for tag, what, pts, world, limit in cases:
        pts = pts.contiguous()
        shuffled = pts[torch.randperm(pts.shape[0], device=device, generator=gen)].contiguous()
        plain, coherent, s_plain, s_coherent = alternating_ms(
            [lambda: world.closest(pts, limit, coherent=False), lambda: world.closest(pts, limit, coherent=True),
             lambda: world.closest(shuffled, limit, coherent=False), lambda: world.closest(shuffled, limit, coherent=True)], args.repeats)
        a, b = world.closest(pts, limit, coherent=False, tested=True), world.closest(pts, limit, coherent=True)
        c, d = world.closest(shuffled, limit, coherent=False), world.closest(shuffled, limit, coherent=True)
        tested = a["tested"].to(torch.float64)
        distances[tag] = a["distance"]
        N = pts.shape[0]
        emit({"bench": "closest", "direction": tag, "what": what, "points": N, "triangles": world.n_faces, "max_distance": round(limit, 6),
              "max_distance_cells": args.cells, "hits": int((a["prim"] >= 0).sum()),
              "own_order": stats(plain), "own_order_coherent_sort": stats(coherent), "shuffled": stats(s_plain),
              "shuffled_coherent_sort": stats(s_coherent), "same_bits": same_bits(a, b) and same_bits(c, d),
              "mpoints_per_s_own_order": round(N / statistics.median(plain) / 1e3, 2),
              "pairs_tested_per_point": {"mean": round(float(tested.mean()), 2), "median": float(tested.median()), "max": int(tested.max())},
              "brute_force_pairs_per_point": world.n_faces})

        n_brute = int(min(args.brute_points, max(64, args.brute_pairs // world.n_faces)))
        sub = pts[torch.randperm(N, device=device, generator=gen)[:n_brute]].contiguous()
        tri = world.vertices[world.faces.long()]
        brute, kernel = alternating_ms([lambda: torch_brute_force(sub, tri, limit), lambda: world.closest(sub, limit, coherent=False)], 3, warmup=1)
        bd, _ = torch_brute_force(sub, tri, limit)
        kd = world.closest(sub, limit, coherent=False)
        finite = torch.isfinite(bd) & torch.isfinite(kd["distance"])
        emit({"bench": "brute_force", "direction": tag, "points": int(sub.shape[0]), "triangles": world.n_faces, "torch_brute_force": stats(brute),
              "kernel_same_points": stats(kernel), "brute_over_kernel": round(statistics.median(brute) / statistics.median(kernel), 1),
              "same_distance_bits": bool(torch.equal(bd.view(torch.int32), kd["distance"].view(torch.int32))),
              "max_abs_difference": float((bd[finite] - kd["distance"][finite]).abs().max()) if bool(finite.any()) else 0.0,
              "hits": int(finite.sum())})
        del tri

        n_np = max(1, min(64, int(args.numpy_pairs // world.n_faces)))
        small = sub[:n_np]
        vn, fn = world.vertices.cpu().numpy(), world.faces.cpu().numpy()
        t0 = time.perf_counter()
        want = W.closest_numpy(small.cpu().numpy(), vn, fn, limit)
        host_s = time.perf_counter() - t0
        got = world.closest(small, limit)
        emit({"bench": "numpy", "direction": tag, "points": n_np, "triangles": world.n_faces, "closest_numpy_s": round(host_s, 3),
              "numpy_us_per_point": round(host_s / n_np * 1e6, 1),
              "same_bits": bool(np.array_equal(want["distance"].view(np.int32), got["distance"].cpu().numpy().view(np.int32))
                                and np.array_equal(want["prim"], got["prim"].cpu().numpy()))})

    th = (cell, 2 * cell, md)
    dist = distances["accuracy"]

    def torch_stats():
        fin = torch.isfinite(dist)
        x = torch.where(fin, dist, torch.zeros_like(dist)).double()
        return fin.sum(), x.sum(), (x * x).sum(), x.max(), [(fin & (dist <= t)).sum() for t in th]

    kernel, eager = alternating_ms([lambda: M.distance_stats(dist, th), torch_stats], args.repeats)
    ks, ts = M.distance_stats(dist, th), torch_stats()
    emit({"bench": "stats", "n": int(dist.shape[0]), "ngp_distance_stats_with_host_read": stats(kernel), "torch_operators_no_host_read": stats(eager),
          "finite": ks["finite"], "sum": ks["sum"], "torch_sum": float(ts[1]), "same_counts": ks["finite"] == int(ts[0]) and
          list(ks["within"]) == [int(c) for c in ts[4]], "same_bits_split_in_three": ks == M.distance_stats(dist, th, splits=(dist.shape[0] // 7 | 1, dist.shape[0] // 2 | 1))})

    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        err = M.surface_error(iv, ifc, worlds["henge"], thresholds=th, max_distance=md)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    emit({"bench": "surface_error", "what": "isosurface against henge, vertices, the given mesh's world built inside", **stats(times),
          "accuracy": {"n": err.accuracy.n, "misses": err.accuracy.misses, "mean": err.accuracy.mean, "max": err.accuracy.max},
          "completeness": {"n": err.completeness.n, "misses": err.completeness.misses, "mean": err.completeness.mean, "max": err.completeness.max},
          "f_score": {str(round(t, 5)): round(v, 6) for t, v in err.f_score.items()}, "hausdorff": err.hausdorff, "margin_0.5": err.margin(0.5)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
