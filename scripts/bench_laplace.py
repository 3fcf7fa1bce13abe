#!/usr/bin/env python3
"""Times the Bayesian-Laplace fit on an 800 x 800 frame (n = 640 000 points) and appends the rows to profiles/laplace_bench.jsonl:
the sigma-fit kernel per evaluation (loss only; loss + full gradient; bytes/s on the features), whole fits through the fused path
(default and likelihood_gradient=True, LM in closed form and with the reference's dense host arithmetic), and the same default fit
through the package's torch path on the GPU (re-encode + autograd every step: what the reference executes) as the baseline.

    python scripts/bench_laplace.py [--hw 800] [--n-steps 1000] [--out profiles/laplace_bench.jsonl]

Needs a GPU; kernel times are device events over `--iters` launches after a warm-up, fit times a host clock around a synchronise."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nerfsafetyvalidation_amd import scene as SC  # noqa: E402
from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork  # noqa: E402
from nerfsafetyvalidation_amd.nerf.utils import get_rays  # noqa: E402
from nerfsafetyvalidation_amd.uncertainty.quantification import bayesian_laplace as BL  # noqa: E402


class TorchPath(BL.BayesianLaplace):
    def uses_fused_path(self, X):
        return False


def kernel_ms(feat, y, theta, mode, iters):
    for _ in range(5):
        BL.sigma_fit_eval(feat, y, theta, 0.0, 1.0, mode)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        BL.sigma_fit_eval(feat, y, theta, 0.0, 1.0, mode)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def fit_seconds(cls, model, X, y, theta, pert, n_steps, **kw):
    lg = kw.pop("likelihood_gradient", False)
    bl = cls(model, 0.0, 1.0, 0.01, likelihood_gradient=lg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bl.fit(X, y, theta_init=theta, perturbations=pert, n_steps=n_steps, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr, rmv = bl.covariance_summary()
    return dt, {"lm_iterations": len(bl.hessian.branches), "trace": tr, "rmv": rmv, "min_loss": bl.min_loss, "fused": bool(bl.fused)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--n-steps", type=int, default=1000)
    ap.add_argument("--torch-steps", type=int, default=100, help="steps per perturbation of the torch-path baseline (scaled to --n-steps in the row)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_laplace.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, density_scale=48.0, min_near=0.2, density_thresh=0.01, bg_radius=-1)
    g = torch.Generator().manual_seed(0)
    model.encoder.embeddings.data.copy_((torch.rand(model.encoder.embeddings.shape, generator=g) - 0.5).half().float())
    model = model.eval().to(dev)
    H = W = a.hw
    pose = torch.from_numpy(SC.orbit_poses()[33:34].copy()).float().to(dev)
    rays = get_rays(pose, SC.intrinsics(H, W), H, W)
    with torch.no_grad():
        out = model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1.0, perturb=False, num_steps=32, upsample_steps=0)
    X = (rays["rays_o"].reshape(-1, 3) + rays["rays_d"].reshape(-1, 3)).unsqueeze(-2).float()
    y = out["aggregated_density"].reshape(-1).float().contiguous()
    n = X.shape[0]
    gen = torch.Generator(device=dev).manual_seed(3)
    theta = torch.randn(3072, device=dev, generator=gen)
    pert = torch.randn((3,) + tuple(X.shape), device=dev, generator=gen) * 0.3
    probe = BL.BayesianLaplace(model, 0.0, 1.0, 0.01)
    feat = probe._encode(X)
    rows = []
    base = {"bench": "laplace", "n": n, "H": H, "W": W}
    ms0, ms2 = kernel_ms(feat, y, theta, BL.MODE_LOSS, a.iters), kernel_ms(feat, y, theta, BL.MODE_FULL_GRAD, a.iters)
    fbytes = feat.numel() * 4 + y.numel() * 4
    rows.append({**base, "what": "kernel", "ms_loss": ms0, "ms_loss_full_grad": ms2, "feature_bytes": fbytes,
                 "loss_bytes_per_s": fbytes / (ms0 * 1e-3), "grad_bytes_per_s": fbytes / (ms2 * 1e-3), "iters": a.iters,
                 "note": "sigma_fit main + reduce kernel, device events; the gradient pass reads the features twice (second read from cache)"})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(3):
        probe._encode(X[None].add(pert)[p])
    torch.cuda.synchronize()
    rows.append({**base, "what": "encode_3_perturbations", "seconds": time.perf_counter() - t0})
    for name, cls, kw in (("fused_default_closed_form_lm", BL.BayesianLaplace, dict(lm_solver="closed_form")),
                          ("fused_default_dense_lm", BL.BayesianLaplace, dict()),
                          ("fused_likelihood_gradient_closed_form_lm", BL.BayesianLaplace, dict(likelihood_gradient=True, lm_solver="closed_form"))):
        fit_seconds(cls, model, X, y, theta, pert, 10, lm_max_iter=2, **dict(kw))          # warm-up of every launch shape
        dt, info = fit_seconds(cls, model, X, y, theta, pert, a.n_steps, **dict(kw))
        rows.append({**base, "what": "fit", "path": name, "n_steps": a.n_steps, "seconds": dt, **info})
        print(rows[-1], flush=True)
    fit_seconds(TorchPath, model, X, y, theta, pert, 3, lm_max_iter=2, lm_solver="closed_form")
    dt, info = fit_seconds(TorchPath, model, X, y, theta, pert, a.torch_steps, lm_solver="closed_form")
    rows.append({**base, "what": "fit", "path": "torch_default_closed_form_lm", "n_steps": a.torch_steps, "seconds": dt,
                 "seconds_scaled_to_n_steps": dt * a.n_steps / a.torch_steps, **info})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
