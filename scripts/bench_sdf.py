#!/usr/bin/env python3
"""Timings of the collision field (nerfsafetyvalidation_amd/collision.py) on one GPU, one JSON line each, also written to
profiles/sdf_bench.jsonl:

  map_build      ms for occupancy_from_density + SignedDistanceField.from_occupancy (density, threshold, EDT, float64 sqrt on
                 the host) over NerfSimulator's box (2.4 x 2.3 x 0.6 m) at 40 and 160 cells/m, 2^3 samples per cell, for the
                 fp32 nn.Linear network (outside autocast) and the fp16 FFMLP network (under autocast)
  cell_density   ngp_cell_max_density density evaluations/s against ngp_network_density points/s on the same points (the
                 latter's points precomputed, one launch per sub-sample; the time excludes forming them)
  edt            ngp_edt_sq ms on the henge map at both sizes, against scipy.ndimage.distance_transform_edt on the host's CPUs
  rollout_step   ms per rollout step (32 x 32 frame, 32 samples per ray, fp16 autocast) with and without the field

The network is the synthetic Stonehenge scene's (scene.StonehengeScene.build_model).  Its random table has no surface, so the map
threshold is the 95th percentile of each network's 40 cells/m cell densities (about 5 % of the cells occupied); the line reports
the occupied fraction.  scipy's transform runs on one thread.

    python scripts/bench_sdf.py [--repeats 3] [--out profiles/sdf_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    device = torch.device("cuda:0")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    sc = StonehengeScene(H=32, W=32, bound=2)
    models = [("f32_linear", sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False), False),
              ("f16_ffmlp", sc.build_model(device, cuda_ray=False), True)]
    s = 2
    boxes = {g: CO.GridBox.from_range((-1.4, -1.3, -0.1), (1.0, 1.0, 0.5), g) for g in (40, 160)}
    thresh = {}
    for name, model, ac in models:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=ac):
            thresh[name] = float(torch.quantile(CO.cell_max_density(model, boxes[40], s).flatten(), 0.95))

    for g, box in boxes.items():
        cells = int(np.prod(box.shape))
        for name, model, ac in models:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                def build():
                    return CO.SignedDistanceField.from_occupancy(CO.occupancy_from_density(model, box, thresh[name], s), box)
                ms, all_ms, sdf = timed(build, args.repeats)
                emit({"bench": "map_build", "network": name, "cells_per_m": g, "shape": list(box.shape), "samples_per_axis": s,
                      "thresh": round(thresh[name], 4), "ms": round(ms, 3), "all_ms": [round(t, 3) for t in all_ms],
                      "occupied_fraction": round(float((sdf.values == 0).mean()), 5)})
                fm = model.fused_model()
                ms_cell, _, sig = timed(lambda: fm.cell_max_density(box.start, box.granularity, box.shape, s, CO.PLANNER_ROT), args.repeats)
                pts = [CO.to_nerf(box.sample_points(a, b, c, s, device), CO.PLANNER_ROT).reshape(-1, 3).contiguous()
                       for a in range(s) for b in range(s) for c in range(s)]

                def per_point():
                    return torch.stack([fm.network_density(p) for p in pts]).amax(0)
                ms_pt, _, want = timed(per_point, args.repeats)
                n_eval = cells * s ** 3
                emit({"bench": "cell_density", "network": name, "cells_per_m": g, "evaluations": n_eval,
                      "cell_max_density_ms": round(ms_cell, 3), "cell_max_density_eval_per_s": round(n_eval / ms_cell * 1e3),
                      "network_density_ms": round(ms_pt, 3), "network_density_points_per_s": round(n_eval / ms_pt * 1e3),
                      "ratio": round(ms_pt / ms_cell, 3), "bit_identical": bool(torch.equal(sig, want.reshape(box.shape)))})
                del pts

    try:
        import scipy.ndimage as nd
    except ImportError:
        nd = None
    for g, box in boxes.items():
        occ = CO.occupancy_from_fn(CO.henge_fn, box, 2)
        occ_dev = occ.to(device)
        ms, all_ms, d2 = timed(lambda: CO.edt_sq(occ_dev), args.repeats)
        line = {"bench": "edt", "cells_per_m": g, "shape": list(box.shape), "gpu_ms": round(ms, 3), "all_ms": [round(t, 3) for t in all_ms]}
        if nd is not None:
            occ_np = occ.numpy()
            t = time.perf_counter()
            want = nd.distance_transform_edt(~occ_np)
            line["scipy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            line["equal_to_scipy"] = bool(np.array_equal(np.sqrt(d2.cpu().numpy().astype(np.float64)), want))
        emit(line)

    H = W = 32
    kw = dict(num_steps=32, upsample_steps=0, max_ray_batch=1024)
    model = models[1][1]
    sdf = CO.SignedDistanceField.from_occupancy(CO.occupancy_from_fn(CO.henge_fn, boxes[40], 2), boxes[40])
    steps = 6
    for with_sdf in (False, True):
        def one():
            sim = RO.RolloutSimulator(model, sc.intrinsics, H, W, steps, seed=0, render_kwargs=kw, sdf=sdf if with_sdf else None)
            with torch.autocast("cuda", dtype=torch.float16):
                return sim.run(0)
        ms, all_ms, rows = timed(one, args.repeats)
        emit({"bench": "rollout_step", "sdf": with_sdf, "frame": [H, W], "samples_per_ray": 32, "steps_run": int(rows.shape[0]),
              "ms_per_step": round(ms / rows.shape[0], 3)})

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for d in lines:
            fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
