#!/usr/bin/env python3
"""Timings of mesh.simplify (csrc/simplify.hip) on one GPU, one JSON line per cell size, also written to
profiles/simplify_bench.jsonl.  The mesh is the resolution^3 isosurface of the synthetic Stonehenge scene's fp32 model at the 95th
percentile of its field (bench_mesh.py's setting), in index units; it is simplified at cell = 2, 4 and 8 with origin (0, 0, 0).

  V, F, V_out, F_out   input and output sizes
  hip_ms               the whole simplify() call (its sorts, scans and the one host read included): stream events around `inner`
                       calls in a row, after a warm-up, the median of `repeats` such rounds divided by `inner`; all_hip_ms the rounds
  stage_ms             per entry point, device events through ngp_prof_* (the torch plumbing between them is the rest of hip_ms)
  numpy_s              the numpy path (the definition) on the same mesh, one host thread, once; identical: same bits as the HIP path
  surface_error_ms     mesh.surface_error of the full and of the simplified mesh, scaled to the model's bounds, against
                       scene.henge_mesh(resolution) (bench_closest.py's report: vertices both ways, truncated at three lattice steps,
                       the given mesh's MeshWorld built inside), host clock around the call with a synchronise on each side, best of
                       `repeats`
  world_ms             MeshWorld construction + one 800 x 800 cast from outside the box, full and simplified, the same way
  f_score_at_two_steps the report's F-score at two lattice steps, full and simplified (what the coarser surface costs against the true world)
  moved_max_cells      the largest distance of a simplified vertex from the full surface, in cells (at most sqrt(3))

    python scripts/bench_simplify.py [--resolution 256] [--repeats 5] [--inner 3] [--no-numpy] [--out profiles/simplify_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STAGES = ("keys", "corners", "accumulate", "faces", "emit")


def event_ms(fn, repeats, inner):
    """median over `repeats` rounds of (stream-event time of `inner` calls in a row) / inner, after one warm-up round"""
    for _ in range(inner):
        out = fn()
    rounds = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            out = fn()
        stop.record()
        stop.synchronize()
        rounds.append(start.elapsed_time(stop) / inner)
    return statistics.median(rounds), rounds, out


def host_ms(fn, repeats):
    """best of `repeats` host-clock timings with a device synchronise on each side, after one warm-up call"""
    out = fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), out


def prof_ms(lib, name):
    ms, launches = ctypes.c_double(0), ctypes.c_uint64(0)
    if lib.ngp_prof_read(name.encode(), ctypes.byref(ms), ctypes.byref(launches), None) != 0 or launches.value == 0:
        return None
    return ms.value / launches.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import _lib
    from nerfsafetyvalidation_amd import mesh as M
    from nerfsafetyvalidation_amd.scene import StonehengeScene, henge_mesh
    from nerfsafetyvalidation_amd.world import MeshWorld
    device = torch.device("cuda:0")
    lib = _lib.lib()
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
    v, f = M.isosurface(u, thr)
    del u
    V, F = int(v.shape[0]), int(f.shape[0])
    vn, fn = v.cpu().numpy(), f.cpu().numpy()

    # downstream, in the bounds' units: the report against the true world's mesh, and a world of the mesh's own with one frame cast
    step = float((hi - lo).max()) / (R - 1.0)

    def scaled(vv):
        return (vv / (R - 1.0) * (hi - lo)[None] + lo[None]).to(torch.float32).contiguous()

    hv, hf, _ = henge_mesh(R)
    henge = MeshWorld(torch.from_numpy(hv).to(device), torch.from_numpy(hf).to(device))
    centre = (lo + hi) / 2.0
    eye = centre + torch.tensor([1.1, 0.9, 0.7], device=device) * (hi - lo)
    ii, jj = torch.meshgrid(torch.linspace(-0.5, 0.5, 800, device=device), torch.linspace(-0.5, 0.5, 800, device=device), indexing="ij")
    fwd = torch.nn.functional.normalize(centre - eye, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], device=device)), dim=0)
    up = torch.linalg.cross(right, fwd)
    rays_d = torch.nn.functional.normalize(fwd + jj[..., None] * right - ii[..., None] * up, dim=-1).reshape(-1, 3).contiguous()
    rays_o = eye.expand_as(rays_d).contiguous()

    def world_and_cast(vv, ff):
        w = MeshWorld(vv, ff)
        return w, w.cast(rays_o, rays_d, frame_width=800)

    def error_of(vv, ff):
        return M.surface_error(vv, ff, henge, thresholds=(step, 2.0 * step), max_distance=3.0 * step)

    full_v = scaled(v)
    full_error_ms, full_err = host_ms(lambda: error_of(full_v, f), args.repeats)
    full_world_ms, (full_world, full_hit) = host_ms(lambda: world_and_cast(full_v, f), args.repeats)
    lines = []
    for cell in (2, 4, 8):
        run = lambda: M.simplify(v, f, cell, origin=(0.0, 0.0, 0.0))
        ms, rounds, (sv, sf, _) = event_ms(run, args.repeats, args.inner)
        lib.ngp_prof_enable(1)
        lib.ngp_prof_reset()
        for _ in range(args.inner):
            run()
        torch.cuda.synchronize()
        stage = {k: prof_ms(lib, "simplify_" + k) for k in STAGES}
        lib.ngp_prof_enable(0)
        line = {"bench": "simplify", "resolution": R, "threshold": round(thr, 5), "cell": cell, "V": V, "F": F, "V_out": int(sv.shape[0]),
                "F_out": int(sf.shape[0]), "hip_ms": round(ms, 3), "all_hip_ms": [round(t, 3) for t in rounds], "inner": args.inner,
                "stage_ms": {k: None if s is None else round(s, 4) for k, s in stage.items()}}
        if not args.no_numpy:
            t = time.perf_counter()
            nv, nf, _ = M.simplify(vn, fn, cell, origin=(0.0, 0.0, 0.0))
            line["numpy_s"] = round(time.perf_counter() - t, 2)
            line["identical"] = bool(np.array_equal(nf, sf.cpu().numpy()) and np.array_equal(nv.view(np.uint32), sv.cpu().numpy().view(np.uint32)))
            del nv, nf
        out_v = scaled(sv)
        err_ms, err = host_ms(lambda: error_of(out_v, sf), args.repeats)
        world_ms, (_, hit) = host_ms(lambda: world_and_cast(out_v, sf), args.repeats)
        line["surface_error_ms"] = {"full": round(full_error_ms, 2), "simplified": round(err_ms, 2)}
        line["world_ms"] = {"full": round(full_world_ms, 2), "simplified": round(world_ms, 2)}
        line["moved_max_cells"] = round(float(full_world.closest(out_v, 4.0 * cell * step)["distance"].max()) / (cell * step), 3)
        line["f_score_at_two_steps"] = {"full": round(full_err.f_score[2.0 * step], 4), "simplified": round(err.f_score[2.0 * step], 4)}
        line["pixels_hit"] = {"full": int(torch.isfinite(full_hit["t"]).sum()), "simplified": int(torch.isfinite(hit["t"]).sum())}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for d in lines:
            fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
