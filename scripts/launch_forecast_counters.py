#!/usr/bin/env python3
"""Schedule counters of the fused render loop per frame, one frame at a time (one context): launches, rolled-back launches, network
samples discarded with them, launches sized by the saturation forecast -- for the bench frame (bound 2, the 20 views
bench.py times after a warm-up of 5) and the Lego-like setting (bound 1, cameras at r = 3.2, the views of bench_lego_like.py).
One JSON line per setting and word of NGP_SCHED_* switches (profiles/launch_forecast.jsonl).

  launch_forecast_counters.py [size] [--flags 0,1]          counters (a tree without the counters reports launches and roll-backs)
  NGP_TRACE_SCHEDULE=1 launch_forecast_counters.py ... 2> trace.txt ;  launch_forecast_counters.py --trace trace.txt
      where the roll-backs happen: per rolled-back launch its q, planned K, headroom, the guess and the deaths before the violation
"""
import json, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise_trace(path):
    plans = [json.loads(m.group(1)) for m in re.finditer(r"\[ngp\] plan (\{.*\})", open(path).read())]
    bad = [p for p in plans if p["rolled_back"]]
    rows = []
    for p in bad:
        # the first violating iteration j: n_alive - deaths before j <= n_alive - headroom - 1
        cum, j_bad = 0, None
        for j, d in enumerate(p["deaths"][:-1]):
            cum += d
            if cum > p["headroom"]:
                j_bad = j + 1
                break
        rows.append({"q": p["q"], "K": p["K"], "K_rate": p["K_rate"], "n_alive": p["n_alive"], "headroom": p["headroom"],
                     "guess_per_iteration": p["rate"], "forecast": p["forecast"], "deaths": p["deaths"], "exhausted": p["exhausted"],
                     "first_bad_iteration": j_bad,
                     # q = 8 has no crossing (n_step is clamped): such a launch fails only because the last ray died inside it and the
                     # last iteration has to run on its own (the caller wants its tensors)
                     "at_n_step_crossing": j_bad is not None and p["q"] < 8, "by_own_last_rule": j_bad is not None and p["q"] == 8,
                     "deaths_before_violation_over_headroom": round(cum / max(p["headroom"], 1), 2) if j_bad else None})
    by_q = {}
    for r in rows:
        by_q[str(r["q"])] = by_q.get(str(r["q"]), 0) + 1
    print(json.dumps({"trace": os.path.basename(path), "multi_iteration_launches": len(plans), "rolled_back": len(bad),
                      "rolled_back_by_q": by_q, "rolled_back_at_an_n_step_crossing": sum(r["at_n_step_crossing"] for r in rows),
                      "rolled_back_by_the_own_last_rule": sum(r["by_own_last_rule"] for r in rows),
                      "rolled_back_launches": rows}))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return summarise_trace(sys.argv[2])
    import torch
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    size = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 800
    flag_words = [int(f) for f in sys.argv[sys.argv.index("--flags") + 1].split(",")] if "--flags" in sys.argv else [0]
    dev = torch.device("cuda:0")
    settings = (("bench_frame", 2, 1.5, list(range(5, 25))), ("lego_like", 1, 3.2, [v * 7 % 200 for v in range(3, 23)]))
    for name, bound, radius, views in settings:
        sc = StonehengeScene(H=size, W=size, bound=bound, radius=radius)
        model = sc.build_model(dev)
        poses = torch.from_numpy(sc.poses).to(dev)
        for flags in flag_words:
            tot, sched_tot = {}, {}
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                def frame(v):
                    r = get_rays(poses[v:v + 1], sc.intrinsics, size, size)
                    return model.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, frame_width=size)
                fm0 = model.fused_model()
                if hasattr(fm0, "schedule_flags"):
                    fm0.schedule_flags = flags
                for v in range(3):
                    frame(v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for v in views:
                    frame(v)
                    for k, x in model.last_render_stats.items():
                        tot[k] = tot.get(k, 0) + x
                    fm = model.fused_model()
                    if hasattr(fm, "schedule_stats"):
                        for k, x in fm.schedule_stats().items():
                            sched_tot[k] = sched_tot.get(k, 0) + x
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            n = len(views)
            out = {"setting": name, "frame": f"{size}x{size}", "schedule_flags": flags, "frames": n,
                   "launches_per_frame": round(tot["launches"] / n, 2), "rolled_back_per_frame": round(tot["replayed"] / n, 3),
                   "network_samples_per_frame": round(tot["samples_marched"] / n), "reference_iterations_per_frame": round(tot["iterations"] / n, 1),
                   "ms_per_frame_with_counter_reads": round(dt / n * 1e3, 3)}
            if sched_tot:
                out.update({"discarded_samples_per_frame": round(sched_tot["discarded_samples"] / n), 
                            "forecast_sized_launches_per_frame": round(sched_tot["forecast_sized"] / n, 2),
                            "multi_iteration_launches_per_frame": round(sched_tot["multi_iteration_launches"] / n, 2)})
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
