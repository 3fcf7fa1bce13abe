#!/usr/bin/env python3
"""Timings of the mesh export (nerfsafetyvalidation_amd/mesh.py) on one GPU, one JSON line each, also written to
profiles/mesh_bench.jsonl:

  field        ms for extract_fields: model.density on the resolution^3 lattice of model.aabb_infer (S = 128 chunks)
  isosurface   ms of the three kernel stages (count = k_iso_flags + k_iso_count, scan = k_iso_scan, emit = k_iso_emit; device
               events through ngp_prof_*), ms of the whole isosurface() call on the host clock (workspace, the host read of V and F,
               the output allocation included), V and F, and next to each stage the time its compulsory traffic would take at the HBM
               rate DESIGN.md uses (8.0 TB/s):
                 count  4 N field + 1 N flags written + 1 N flags read + 6 N (mask, count, two uint16 prefixes) + N / 16 block totals
                 scan   N / 8 (block totals read and written)
                 emit   4 N field + 6 N (mask, count, prefixes) + N / 16 + 12 V + 12 F
  cpu_path     s of the numpy path on the same field (one host thread), and whether the two meshes are identical
  save_mesh    s of the whole call, the float64 scaling and the binary PLY included

The network is the synthetic Stonehenge scene's (scene.StonehengeScene.build_model), fp32.  Its random table has no surface at the
reference's default threshold, so the threshold is the 95th percentile of the field (5 % of the lattice inside), as bench_sdf.py
chooses its map threshold.

    python scripts/bench_mesh.py [--resolution 256] [--repeats 3] [--out profiles/mesh_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, repeats):
    """best of `repeats` host-clock timings around fn() with a device synchronise on each side, after one warm-up call"""
    out = fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), ts, out


def prof_ms(lib, name):
    ms, launches = ctypes.c_double(0), ctypes.c_uint64(0)
    if lib.ngp_prof_read(name.encode(), ctypes.byref(ms), ctypes.byref(launches), None) != 0 or launches.value == 0:
        return None
    return ms.value / launches.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import _lib
    from nerfsafetyvalidation_amd import mesh as M
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    device = torch.device("cuda:0")
    lib = _lib.lib()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    R = args.resolution
    model = StonehengeScene(H=32, W=32, bound=2).build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    model.eval()
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]

    def query(pts):
        with torch.no_grad():
            return model.density(pts.to(device))["sigma"]

    ms, all_ms, u = timed(lambda: M.extract_fields(lo, hi, R, query), args.repeats)
    emit({"bench": "field", "resolution": R, "ms": round(ms, 3), "all_ms": [round(t, 3) for t in all_ms],
          "points_per_s": round(R ** 3 / ms * 1e3)})
    sample = u.flatten()[torch.randperm(u.numel(), device=device)[:1 << 20]]
    thr = float(torch.quantile(sample, 0.95))

    ms, all_ms, (v, f) = timed(lambda: M.isosurface(u, thr), args.repeats)
    lib.ngp_prof_enable(1)
    lib.ngp_prof_reset()
    for _ in range(args.repeats):
        M.isosurface(u, thr)
    torch.cuda.synchronize()
    stage = {k: prof_ms(lib, "isosurface_" + k) for k in ("count", "scan", "emit")}
    lib.ngp_prof_enable(0)
    N, V, F = R ** 3, int(v.shape[0]), int(f.shape[0])
    floor_bytes = {"count": 12 * N + N // 16, "scan": N // 8, "emit": 10 * N + N // 16 + 12 * V + 12 * F}
    emit({"bench": "isosurface", "resolution": R, "threshold": round(thr, 5), "inside_fraction": round(float((u > thr).float().mean()), 5),
          "V": V, "F": F, "call_ms": round(ms, 3), "all_call_ms": [round(t, 3) for t in all_ms],
          "stage_ms": {k: None if s is None else round(s, 4) for k, s in stage.items()},
          "floor_bytes": floor_bytes, "floor_ms_at_8TBps": {k: round(b / HBM_BYTES_PER_S * 1e3, 4) for k, b in floor_bytes.items()},
          "workspace_bytes": int(lib.ngp_isosurface_workspace(R, R, R))})

    un = u.cpu().numpy()
    t = time.perf_counter()
    cv, cf = M.isosurface(un, thr)
    cpu_s = time.perf_counter() - t
    emit({"bench": "cpu_path", "resolution": R, "s": round(cpu_s, 2), "gpu_call_ms": round(ms, 3), "ratio": round(cpu_s * 1e3 / ms, 1),
          "identical": bool(np.array_equal(cf, f.cpu().numpy()) and np.array_equal(cv.view(np.uint32), v.cpu().numpy().view(np.uint32)))})
    del cv, cf, un

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "meshes", "henge.ply")
        torch.cuda.synchronize()
        t = time.perf_counter()
        verts, tris = M.save_mesh(model, path, resolution=R, threshold=thr)
        s = time.perf_counter() - t
        emit({"bench": "save_mesh", "resolution": R, "s": round(s, 2), "V": int(len(verts)), "F": int(len(tris)),
              "ply_bytes": os.path.getsize(path)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for d in lines:
            fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
