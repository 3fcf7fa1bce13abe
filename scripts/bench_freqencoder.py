#!/usr/bin/env python3
"""The frequency encoder on the MI355X: forward and forward + backward of the HIP operator (freqencoder.freq_encode) against the same
encoding written as torch operators with autograd on the same GPU, three alternated repeats per arm, at

    D = 3, degree 6 on 4 M rows     (the samples of a training batch)
    D = 3, degree 4 on 33 M rows    (one 4096-ray chunk of `run` at 512 samples x 16 chunks)

and the share of the HBM roofline the HIP operator reaches: its algorithmic bytes -- forward 4 (D + C) per row, backward 4 (C + 2 D)
per row -- over its time, against the 6.29 TB/s a float4 copy measures on this chip (8.0 TB/s on the data sheet).  Appends the lines to
profiles/freqencoder_bench.jsonl.

    python scripts/bench_freqencoder.py [--out profiles/freqencoder_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerfsafetyvalidation_amd.freqencoder import freq_encode

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def torch_encode(x, degree):
    return torch.cat([x] + [fn(x * 2.0 ** f) for f in range(degree) for fn in (torch.sin, torch.cos)], dim=-1)


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def shape_lines(rows, D, degree, reps, what, dev):
    C = D + 2 * D * degree
    g = torch.Generator(device=dev).manual_seed(rows % 1000 + degree)
    x = torch.rand(rows, D, device=dev, generator=g) * 4 - 2
    grad = torch.randn(rows, C, device=dev, generator=g)
    res = {}

    def forward(encode, key):
        def run():
            with torch.no_grad():
                res[key] = encode(x)
        return run

    def both(encode, key):
        def run():
            xg = x.detach().requires_grad_(True)
            encode(xg).backward(grad)
            res[key] = xg.grad
        return run

    hip = lambda t: freq_encode(t, degree, C)
    chain = lambda t: torch_encode(t, degree)
    lines = []
    for mode, make, nbytes in (("forward", forward, 4 * (D + C) * rows), ("forward+backward", both, 4 * (D + C) * rows + 4 * (C + 2 * D) * rows)):
        t_hip, t_torch = [], []
        for _ in range(3):                                    # alternated
            t_hip.append(round(time_ms(make(hip, "hip"), reps), 4))
            t_torch.append(round(time_ms(make(chain, "torch"), max(reps // 20, 3)), 4))
        best = min(t_hip) * 1e-3
        scale = float(res["torch"].abs().max())
        lines.append({"bench": "freqencoder", "what": what, "mode": mode, "rows": rows, "D": D, "degree": degree, "C": C,
                      "hip_ms": t_hip, "torch_ms": t_torch, "hip_algorithmic_bytes": nbytes,
                      "hip_TB_per_s": round(nbytes / best / 1e12, 3),
                      "hip_share_of_measured_hbm_6.29TBs": round(nbytes / best / HBM_MEASURED, 3),
                      "hip_share_of_spec_hbm_8TBs": round(nbytes / best / HBM_SPEC, 3),
                      "max_abs_diff_hip_torch_over_max": float((res["hip"] - res["torch"]).abs().max()) / scale,
                      "device": torch.cuda.get_device_name(0)})
        res.clear()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freqencoder_bench.jsonl"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the row counts (a rehearsal: 0.001)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_freqencoder.py needs an MI355X: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    lines = []
    lines += shape_lines(int((4 << 20) * a.scale), 3, 6, 400, "training batch: 4 M samples, degree 6", dev)
    lines += shape_lines(int((4096 * 512 * 16) * a.scale), 3, 4, 60, "run chunk: 4096 rays x 512 samples x 16, degree 4", dev)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
