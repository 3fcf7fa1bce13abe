#!/usr/bin/env python3
"""Throughput of one Cross Entropy Method population (cem.run_cem, kmax = 1) next to run_rollout on the same model, frame size, step
count, signed distance field and `in_flight`, on one GPU.  A population is `m` independent simulations run through the same
concurrent machinery as the Monte-Carlo rollout, so the two are expected to agree to within the spread between machines; the run
records both and gates nothing.  Appends ONE JSON line to profiles/cem_bench.jsonl (and prints it).

The model is the synthetic Stonehenge scene's fp32 network (nerf/network.py backbone, no autocast: the arithmetic validate.py's rollout
runs), rendered through `run` with --samples uniform samples per ray; a simulation that collides ends early, so frames/s counts the
frames really rendered.

    python scripts/bench_cem.py [--size 256] [--samples 128] [--steps 12] [--m 24] [--in-flight 6] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--m", type=int, default=24)
    ap.add_argument("--in-flight", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cem_bench.jsonl"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import collision as CO
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    device = torch.device("cuda:0")
    H = W = args.size
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    sdf = CO.SignedDistanceField.from_occupancy(CO.occupancy_from_fn(CO.henge_fn, CO.reference_box()), CO.reference_box())
    kw = dict(num_steps=args.samples, upsample_steps=0, max_ray_batch=4096)
    common = dict(seed=0, sdf=sdf, in_flight=args.in_flight, render_kwargs=kw, autocast=False)

    def cem(m):
        rows, _, counters = CE.run_cem(model, sc.intrinsics, H, W, args.steps, m=m, m_elite=max(2, m // 2), kmax=1, **common)
        return rows, counters

    def mc(m):
        return RO.run_rollout(model, sc.intrinsics, H, W, m, args.steps, **common)

    def once(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rows, counters = fn(args.m)
        torch.cuda.synchronize()
        return time.perf_counter() - t, counters, rows.shape[0]

    def summary(runs):
        dt, counters, n_rows = min(runs, key=lambda r: r[0])
        return {"seconds": round(dt, 4), "all_seconds": [round(r[0], 4) for r in runs], "simulations": counters["simulations"], "rows": n_rows,
                "frames": counters["frames"], "simulations_per_s": round(counters["simulations"] / dt, 3),
                "frames_per_s": round(counters["frames"] / dt, 2)}

    cem(min(args.m, args.in_flight))                        # warm-up: kernels loaded, the fp32 snapshot and the streams' workspaces built
    mc(min(args.m, args.in_flight))
    runs = {"cem": [], "monte_carlo": []}
    for _ in range(args.repeats):                           # interleaved, so that a drift of the machine falls on both alike
        runs["cem"].append(once(cem))
        runs["monte_carlo"].append(once(mc))
    prop = torch.cuda.get_device_properties(0)
    line = {"bench": "cem_population", "gpu": torch.cuda.get_device_name(0), "arch": prop.gcnArchName, "compute_units": prop.multi_processor_count,
            "frame": [H, W], "samples_per_ray": args.samples,
            "steps": args.steps, "m": args.m, "in_flight": args.in_flight, "dtype": "f32 (no autocast)", "repeats": args.repeats,
            "cem": summary(runs["cem"]), "monte_carlo": summary(runs["monte_carlo"])}
    line["cem_over_monte_carlo_frames_per_s"] = round(line["cem"]["frames_per_s"] / line["monte_carlo"]["frames_per_s"], 4)
    text = json.dumps(line)
    with open(args.out, "a") as fh:
        fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
