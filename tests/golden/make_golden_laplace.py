#!/usr/bin/env python3
"""Generates tests/golden/laplace.npz by running the REFERENCE's own Bayesian-Laplace code on CPU: uncertain.uncertainty("Bayesian
Laplace Approximation", ...) and, inside it, BayesianLaplace.fit and hessian/methods.levenberg_marquardt.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_laplace.py

The network is make_golden._ref_network(2, False, 48.0) (the reference's NeRFNetwork over the CPU oracle shims, table seed 0); the
frame is orbit view 33 at 16 x 16 (256 points), rendered as validate.py's render_fn on 32 uniform samples; lr = 0.01.
Patched IN MEMORY only, nothing of the reference is copied or changed:
  * Tensor.cuda() returns the tensor, torch.randn(..., device='cuda') draws on the CPU, uncertain.H = uncertain.W = 16;
  * the network's own parameters do not require a gradient (the reference's loss.backward() would otherwise also accumulate the
    48 MB table gradient 3000 times; no recorded value depends on it);
  * stdout is discarded.
The whole run is made on ONE host thread (hessian.methods.single_thread_lapack: a setting of the process, not of the reference): the
reference's float32 solve / inverse are round-off dominated and their results depend on the LAPACK thread count otherwise.
Spies record what the reference computed: the draws, every loss of the 3 x 1000 steps, theta at the probe steps, and LM's calls of
the objective and of torch.linalg.solve.  SEED = 3 is the first seed tried; the conditions asserted at the end hold for it (LAPLACE_SEED overrides it, LAPLACE_DRY=1 only
reports).  The report also shows how far the reference's float32 solve / inverse are from their closed forms."""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (shims, sys.path of the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfsafetyvalidation_amd import scene as SC  # noqa: E402

H = W = 16
VIEW = 33
LR = 0.01
SEED = int(os.environ.get("LAPLACE_SEED", "3"))
PROBES = (0, 1, 99, 100, 500, 999)
RENDER = dict(staged=True, bg_color=1.0, perturb=False, num_steps=32, upsample_steps=0)


def loss_f64(theta, feat, y):
    th = theta.astype(np.float64)
    W1, W2 = th[:2048].reshape(64, 32), th[2048:].reshape(16, 64)
    h0 = np.maximum(feat.astype(np.float64) @ W1.T, 0) @ W2[0]
    return 0.5 * np.sum(th ** 2) + 0.5 * np.sum((y.astype(np.float64).reshape(-1) - np.exp(h0)) ** 2)


def main():
    import matplotlib
    matplotlib.use("Agg")
    import uncertain as U
    import uncertainty.quantification.bayesian_laplace as BLM

    net = MG._ref_network(2, False, 48.0)
    net.requires_grad_(False)
    intr = SC.intrinsics(H, W)
    pose = torch.from_numpy(SC.orbit_poses()[VIEW:VIEW + 1].copy()).float()
    rays = MG.ref_get_rays(pose, intr, H, W)
    with torch.no_grad():
        out = net.render(rays["rays_o"], rays["rays_d"], **RENDER)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}

    rec = {"randn_like": [], "randn": [], "fit": [], "lm": []}
    real_cuda, real_randn, real_randn_like, real_solve = torch.Tensor.cuda, torch.randn, torch.randn_like, torch.linalg.solve
    real_nlp, real_wrap = BLM.BayesianLaplace.negative_log_posterior, BLM.BayesianLaplace.negative_log_posterior_hessian_wrapper

    def randn(*a, **k):
        k.pop("device", None)
        t = real_randn(*a, **k)
        rec["randn"].append(t.clone())
        return t

    def randn_like(t, **k):
        r = real_randn_like(t, **k)
        rec["randn_like"].append(r.detach().clone())
        return r

    in_lm = [False]

    def nlp(self, theta, X, y):
        v = real_nlp(self, theta, X, y)
        if not in_lm[0]:
            k = len(rec["fit"]) % 1000
            rec["fit"].append((float(v), theta.detach().clone().numpy() if k in PROBES else None, X.detach().clone() if k == 0 else None))
        return v

    def wrap(self, xt):
        in_lm[0] = True
        v = real_wrap(self, xt)
        rec["lm"].append(("func", xt.detach().clone().numpy(), float(v)))
        return v

    def solve(A, b):
        try:
            r = real_solve(A, b)
        except RuntimeError:
            rec["lm"].append(("solve_err", None, None))
            raise
        rec["lm"].append(("solve", (-b).detach().clone().numpy(), None))
        return r

    from nerfsafetyvalidation_amd.uncertainty.quantification.hessian.methods import single_thread_lapack
    torch.manual_seed(SEED)
    with single_thread_lapack(), contextlib.redirect_stdout(io.StringIO()):
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.randn, torch.randn_like, torch.linalg.solve = randn, randn_like, solve
        BLM.BayesianLaplace.negative_log_posterior, BLM.BayesianLaplace.negative_log_posterior_hessian_wrapper = nlp, wrap
        U.H = U.W = H
        got = {}
        real_fit = BLM.BayesianLaplace.fit

        def fit(self, X, y):
            r = real_fit(self, X, y)
            got["mean"], got["X"], got["y"] = np.array(self.posterior_mean, np.float32), np.asarray(X), np.asarray(y)
            return r

        BLM.BayesianLaplace.fit = fit
        try:
            trace, rmv = U.uncertainty("Bayesian Laplace Approximation", rendered_output=(out, rays["rays_o"], rays["rays_d"]),
                                       model_to_use=net, lr=LR)
        finally:
            torch.Tensor.cuda, torch.randn, torch.randn_like, torch.linalg.solve = real_cuda, real_randn, real_randn_like, real_solve
            BLM.BayesianLaplace.negative_log_posterior, BLM.BayesianLaplace.negative_log_posterior_hessian_wrapper = real_nlp, real_wrap
            BLM.BayesianLaplace.fit = real_fit
    for k, v in net.state_dict().items():
        assert torch.equal(v, state0[k]), f"the reference left {k} changed"

    theta_init, pert = rec["randn_like"][0].numpy(), (rec["randn"][0] * 0.3).numpy()      # (:64-65: randn * perturbation_scale)
    X, y = got["X"].astype(np.float32), got["y"].astype(np.float32)
    assert len(rec["fit"]) == 3000 and pert.shape == (3,) + X.shape
    hist = np.array([v for v, _, _ in rec["fit"]], np.float32).reshape(3, 1000)
    assert np.isfinite(hist).all(), "a loss is not finite: change SEED"
    # the reference's selection (:79-81): running minimum over all steps, minTheta aliases the LAST perturbation that improved it
    run_min, chosen = np.inf, -1
    for p in range(3):
        for k in range(1000):
            if hist[p, k] < run_min:
                run_min, chosen = hist[p, k], p
    best = hist.min(1)
    order = np.sort(best)
    assert (order[1] - order[0]) / abs(order[0]) > 1e-3, f"winner not separated from the runner-up ({order[:2]}): change SEED"
    with torch.no_grad():
        feat_X = net.encoder(torch.from_numpy(X), bound=net.bound).reshape(-1, 32).numpy()
        feat_p = np.stack([net.encoder(torch.from_numpy(X[None] + pert)[p], bound=net.bound).reshape(-1, 32).numpy() for p in range(3)])
        for p in range(3):
            assert torch.equal(rec["fit"][1000 * p][2], torch.from_numpy(X)[None].add(torch.from_numpy(pert))[p])
    probe_theta = np.stack([[rec["fit"][1000 * p + k][1] for k in PROBES] for p in range(3)])
    probe_ref = np.array([[hist[p, k] for k in PROBES] for p in range(3)], np.float64)
    probe_f64 = np.array([[loss_f64(probe_theta[p, i], feat_p[p], y) for i in range(len(PROBES))] for p in range(3)])
    loss_err_ref = float(np.max(np.abs(probe_ref - probe_f64) / np.abs(probe_f64)))

    # ---- LM: parse the event log into iterations
    ev = rec["lm"]
    assert not any(e[0] == "solve_err" for e in ev), "torch.linalg.solve raised: the closed form has no such branch; change SEED"
    branches, lambdas, f_new, f_x0, i, lm, x_final, g_final = [], [], [], [], 0, 0.01, got["mean"], None
    while i < len(ev):
        assert ev[i][0] == "func" and ev[i + 1][0] == "solve"
        g_final = ev[i + 1][1]
        if i + 3 >= len(ev):
            break                                      # allclose(dx, 0): the loop ended here
        assert ev[i + 2][0] == "func" and ev[i + 3][0] == "func"
        x_final, fn, f0 = ev[i + 2][1], ev[i + 2][2], ev[i + 3][2]
        better = fn < f0
        assert abs(fn - f0) / abs(f0) > 1e-3 or not np.isfinite(fn), f"LM comparison {len(branches)} not separated ({fn} vs {f0}): change SEED"
        lm = lm / 10 if better else lm * 10
        branches.append(better)
        lambdas.append(lm)
        f_new.append(fn)
        f_x0.append(f0)
        i += 4
    # float64 replay of the closed form dx = -g / (lambda + g.g) along the reference's branch decisions
    x64, lam = got["mean"].astype(np.float64), 0.01
    for b in branches:
        g = x64.copy()
        x64 = x64 - g / (lam + g @ g)
        lam = lam / 10 if b else lam * 10
    lm_x_err_ref = float(np.max(np.abs(x_final.astype(np.float64) - x64)) / np.max(np.abs(x64)))
    g64 = g_final.astype(np.float64)
    diag = np.maximum(0, (1 - g64 * g64 / (0.01 + g64 @ g64)) / 0.01)
    print(f"seed {SEED}: chosen {chosen}, best {best}, loss_err_ref {loss_err_ref:.3e}, LM iterations {len(branches)} "
          f"(better: {sum(branches)}), lm_x_err_ref {lm_x_err_ref:.3e}, trace {trace!r} rmv {rmv!r}; closed form trace {diag.mean()!r} "
          f"rmv {np.sqrt(diag.mean()) / diag.size!r}")
    if os.environ.get("LAPLACE_DRY"):                  # seed search: report only
        return
    MG.save("laplace.npz", seed=SEED, lr=LR, H=H, W=W, view=VIEW, num_steps=RENDER["num_steps"], bound=2, density_scale=48.0, table_seed=0,
            theta_init=theta_init, perturbations=pert, X=X, y=y, feat_X=feat_X, feat_p=feat_p, loss_history=hist, chosen=chosen,
            posterior_mean=got["mean"], probe_steps=np.array(PROBES), probe_theta=probe_theta, probe_ref=probe_ref, probe_f64=probe_f64,
            loss_err_ref=loss_err_ref, lm_branches=np.array(branches, bool), lm_lambdas=np.array(lambdas, np.float64),
            lm_f_new=np.array(f_new, np.float64), lm_f_x0=np.array(f_x0, np.float64), lm_x=x_final, lm_g=g_final, lm_x_f64=x64,
            lm_x_err_ref=lm_x_err_ref, trace=np.float64(trace), rmv=np.float64(rmv), **MG._weights(net))


if __name__ == "__main__":
    main()
