#!/usr/bin/env python3
"""Timings of the connected-component labelling (nerfsafetyvalidation_amd/collision.py, csrc/components.hip) on one GPU, one JSON
line each, also written to profiles/components_bench.jsonl:

  label          per lattice (NerfSimulator's box 96 x 92 x 24, and 256^3), input (the synthetic model's thresholded density; random
                 fills at 10 / 30 / 60 %) and connectivity (6, 14, 18, 26): ms of collision.label_components (the call: workspace,
                 six launches, the host read of n) and of collision.component_table (followed by a synchronise), host clock around
                 a device synchronise; the per-stage device times (HIP events around each stage: tile, seams, flatten, rank = scan +
                 rank + relabel, stats); scipy.ndimage.label on the host INCLUDING the device-to-host copy of the map; the
                 package's numpy path (reference box: every line; 256^3: the 30 % fill under 26 only, it takes many seconds).
                 Every timing: median, minimum and maximum of --repeats runs after --warmup unrecorded ones.
  remove         a whole collision.remove_floaters(min_cells=.., grounded=..) on both lattices, model input
  save_mesh      mesh.save_mesh(min_points=64) against mesh.save_mesh() at 256^3, seconds

The model is the synthetic Stonehenge scene's; its random table has no surface, so the threshold is the 95th percentile of the
densities (about 5 % occupied, in many small pieces: close to the worst a floater filter meets).

    python scripts/bench_components.py [--repeats 10] [--warmup 2] [--out profiles/components_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STAGES = ("cc_tile", "cc_seams", "cc_flatten", "cc_rank", "cc_stats")


def spread(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}


def timed(fn, repeats, warmup, sync=True):
    """ms of fn(): host clock, a device synchronise on each side"""
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return spread(ts), out


def prof_ms(lib, name):
    ms, launches = ctypes.c_double(0), ctypes.c_uint64(0)
    if lib.ngp_prof_read(name.encode(), ctypes.byref(ms), ctypes.byref(launches), None) != 0 or launches.value == 0:
        return None
    return round(ms.value / launches.value, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.jsonl"))
    args = ap.parse_args()
    from scipy import ndimage
    from nerfsafetyvalidation_amd import _lib
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import mesh as M
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    device = torch.device("cuda:0")
    lib = _lib.lib()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    model = StonehengeScene(H=32, W=32, bound=2).build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    model.eval()

    def query(pts):
        with torch.no_grad():
            return model.density(pts.to(device))["sigma"]

    def thresholded(u):
        sample = u.flatten()[torch.randperm(u.numel(), device=device)[:1 << 20]]
        return u > float(torch.quantile(sample, 0.95))

    with torch.no_grad():
        box_density = CO.cell_max_density(model, CO.reference_box())
    lattices = {"96x92x24": thresholded(box_density), "256x256x256": thresholded(M.extract_fields(model.aabb_infer[:3], model.aabb_infer[3:], 256, query))}

    structures = {}
    for c in CO.CONNECTIVITIES:
        s = np.zeros((3, 3, 3), bool)
        s[1, 1, 1] = True
        for dx, dy, dz in CO.connectivity_offsets(c):
            s[1 + dx, 1 + dy, 1 + dz] = True
        structures[c] = s

    for lattice, model_occ in lattices.items():
        shape = tuple(model_occ.shape)
        inputs = {"model": model_occ}
        for fill, seed in ((0.1, 1), (0.3, 2), (0.6, 3)):
            inputs[f"fill{int(fill * 100)}"] = torch.from_numpy(np.random.default_rng(seed).random(shape) < fill).to(device)
        for name, occ in inputs.items():
            for c in CO.CONNECTIVITIES:
                label_ms, (labels, n) = timed(lambda: CO.label_components(occ, c), args.repeats, args.warmup)
                table_ms, table = timed(lambda: CO.component_table(labels, n, occ), args.repeats, args.warmup)
                lib.ngp_prof_enable(1)
                lib.ngp_prof_reset()
                for _ in range(args.repeats):
                    CO.component_table(*CO.label_components(occ, c))
                torch.cuda.synchronize()
                stage = {k[3:]: prof_ms(lib, k) for k in STAGES}
                lib.ngp_prof_enable(0)

                def scipy_run():
                    return ndimage.label(occ.cpu().numpy(), structures[c])
                scipy_ms, (want, n_want) = timed(scipy_run, args.cpu_repeats, 1)
                line = {"bench": "label", "lattice": lattice, "input": name, "connectivity": c, "occupied_fraction": round(float(occ.float().mean()), 4),
                        "components": n, "largest_cells": int(table.cells.max()) if n else 0, "label_call_ms": label_ms, "table_call_ms": table_ms,
                        "stage_ms": stage, "scipy_with_copy_ms": scipy_ms, "equal_to_scipy": bool(n == n_want and np.array_equal(labels.cpu().numpy(), want)),
                        "workspace_bytes": int(lib.ngp_label_components_workspace(*shape))}
                if lattice == "96x92x24" or (name == "fill30" and c == 26):
                    occ_np = occ.cpu().numpy()
                    line["numpy_path_ms"], _ = timed(lambda: CO.label_components_numpy(occ_np, c), args.cpu_repeats if lattice == "96x92x24" else 1,
                                                    1 if lattice == "96x92x24" else 0, sync=False)
                emit(line)
                del want, labels, table

        min_cells = 8
        for kw in (dict(min_cells=min_cells), dict(grounded=(2, "lo")), dict(min_cells=min_cells, grounded=(2, "lo"))):
            ms, (cleaned, report) = timed(lambda: CO.remove_floaters(model_occ, **kw), args.repeats, args.warmup)
            emit({"bench": "remove", "lattice": lattice, "input": "model", "connectivity": 26, "keywords": {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()},
                  "call_ms": ms, "components": report["n"], "kept": report["kept"]["count"], "dropped": report["dropped"]["count"],
                  "cells_before": int(model_occ.sum()), "cells_after": int(cleaned.sum())})

    thr = float(torch.quantile(M.extract_fields(model.aabb_infer[:3], model.aabb_infer[3:], 64, query).flatten(), 0.95))
    with tempfile.TemporaryDirectory() as tmp:
        result = {}
        for min_points in (0, 64, 0, 64):          # alternating
            path = os.path.join(tmp, f"m{min_points}.ply")
            torch.cuda.synchronize()
            t = time.perf_counter()
            verts, tris = M.save_mesh(model, path, resolution=256, threshold=thr, min_points=min_points)
            result.setdefault(min_points, []).append((round(time.perf_counter() - t, 3), int(len(verts)), int(len(tris))))
        emit({"bench": "save_mesh", "resolution": 256, "threshold": round(thr, 4),
              "plain": {"s": [r[0] for r in result[0]], "V": result[0][0][1], "F": result[0][0][2]},
              "min_points_64": {"s": [r[0] for r in result[64]], "V": result[64][0][1], "F": result[64][0][2]}})

    out.close()


if __name__ == "__main__":
    main()
