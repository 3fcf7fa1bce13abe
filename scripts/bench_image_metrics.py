#!/usr/bin/env python3
"""Times the image-quality pass and appends the rows to profiles/image_metrics_bench.jsonl.

One 800 x 800 frame ([1,800,800,3], the Trainer's layout), median of 20 calls after 3 warm-ups, each call between two stream events:
  * one_launch       image_quality_stats: ngp_image_quality (main + final kernel) and the allocation of its outputs
  * torch_operators  the same recipe as torch operators on the same GPU, float32 (reflect pad, grouped 11 x 11 conv2d of the five
                     images, the elementwise SSIM formula, the channel mean and the sums): what the reference's torchmetrics call runs
A 200-frame evaluation loop (the frames already on the device, as eval_step leaves them), wall time including the final read-back:
  * psnr_meter           PSNRMeter alone: the copy of both frames to the host per frame
  * psnr_and_ssim_meter  [PSNRMeter, SSIMMeter], what --ssim runs
  * ssim_meter_both      SSIMMeter alone, measure() and measure_psnr()

    python scripts/bench_image_metrics.py [--hw 800] [--frames 200] [--out profiles/image_metrics_bench.jsonl] [--tag NAME]

Needs a GPU.  --tag names the library build in the rows (e.g. a float-sums variant selected with NGP_HIP_LIB)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfsafetyvalidation_amd.nerf.utils import PSNRMeter, SSIMMeter  # noqa: E402
from nerfsafetyvalidation_amd.uncertainty.evaluation import image_metrics as IM  # noqa: E402


def torch_operators(pred, target):
    """[1,H,W,3] x 2 -> (sum of the channel-mean SSIM map, squared error per channel), torch operators only"""
    p, t = pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)
    smap = IM._ssim_map_torch(p, t, 1.0).mean(1)
    return smap.sum((1, 2)), ((p - t) ** 2).sum((2, 3))


def event_ms(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def loop_seconds(meters, pred, target, frames, finish):
    for m in meters:
        m.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        for m in meters:
            m.update(pred, target)
    values = finish(meters)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_bench.jsonl"))
    ap.add_argument("--tag", default="double_sums")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_metrics.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    H = W = a.hw
    gen = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    target = torch.stack([0.5 + 0.45 * torch.sin(0.031 * xx) * torch.cos(0.019 * yy), xx / (W - 1) * yy / (H - 1), torch.full((H, W), 0.75)], -1)[None]
    pred = (target + 0.05 * torch.randn(target.shape, generator=gen)).clamp(0, 1).to(dev)
    target = target.clamp(0, 1).to(dev)

    base = {"bench": "image_metrics", "H": H, "W": W, "build": a.tag}
    rows = []
    stats, _ = IM.image_quality_stats(pred, target, channels_last=True)
    s_sum, err = torch_operators(pred, target)
    torch.cuda.synchronize()
    rows.append({**base, "what": "agreement", "ssim_one_launch": (stats[0, 0] / stats[0, 1]).item(), "ssim_torch_float32": s_sum.item() / (H * W),
                 "sq_err_rel_diff": ((stats[0, 2:5] - err[0].double()).abs() / stats[0, 2:5]).max().item()})
    for name, fn in (("one_launch", lambda: IM.image_quality_stats(pred, target, channels_last=True)),
                     ("one_launch_with_map", lambda: IM.image_quality_stats(pred, target, channels_last=True, return_map=True)),
                     ("torch_operators", lambda: torch_operators(pred, target))):
        med, lo, hi = event_ms(fn)
        rows.append({**base, "what": "frame", "arm": name, "ms_median": med, "ms_min": lo, "ms_max": hi, "reps": 20, "warmup": 3})
        print(rows[-1], flush=True)
    arms = (("psnr_meter", [PSNRMeter()], lambda ms: {"psnr": float(ms[0].measure())}),
            ("psnr_and_ssim_meter", [PSNRMeter(), SSIMMeter()], lambda ms: {"psnr": float(ms[0].measure()), "ssim": ms[1].measure()}),
            ("ssim_meter_both", [SSIMMeter()], lambda ms: {"ssim": ms[0].measure(), "psnr": ms[0].measure_psnr()}))
    for name, meters, finish in arms:
        loop_seconds(meters, pred, target, 3, finish)
        runs = [loop_seconds(meters, pred, target, a.frames, finish) for _ in range(3)]
        secs = sorted(r[0] for r in runs)
        rows.append({**base, "what": "evaluation_loop", "arm": name, "frames": a.frames, "seconds_median": secs[1], "seconds_min": secs[0],
                     "seconds_max": secs[2], "ms_per_frame": secs[1] / a.frames * 1e3, **runs[0][1]})
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
