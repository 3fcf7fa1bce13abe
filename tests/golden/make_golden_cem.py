#!/usr/bin/env python3
"""Generates tests/golden/cem.npz by running the REFERENCE's own CrossEntropyMethod.optimize()
(validation/stresstests/CrossEntropyMethod.py:49-305, with validation/distributions/SeedableMultivariateNormal.py) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cem.py

The simulator is make_golden.py::gen_rollout's stub of NerfSimulator: step() keeps the reference's Agent.step (drone dynamics + noise)
with a hover action and reward() is the reference's own; sigma is a fixed function of the state; the collision value is the analytic
distance |pos - C| - R to a sphere (float64 of the float32 position) and collided = value < 0.  p and q are validate.py:31-38's, the
seed is the default CPU generator's (validate.py:35); steps = 4, m = 6, m_elite = 3, kmax = 3.
Patched IN MEMORY only, nothing of the reference is copied or changed: Tensor.cuda() returns the tensor; `seaborn` is a stub module;
runBlenderOnFailure is a no-op; compute_best_solution is stubbed (it cannot run against NerfSimulator: it unpacks three of step()'s
five values); plt.savefig is discarded; the working directory is a temporary one with results/.  A spy around
SeedableMultivariateNormal records the means and covariances of every refit and the noises of every q.sample().
Stored: the CSV rows, the per-population means and covariance diagonals, every simulation's whole noise trajectory, risks and elite
indices (np.argsort as :215), the generator seed, the stub's coefficients.
The sphere: the first one tried, C = end_pos + (0.3, 0, 0) with R = 0.29, fails a condition asserted at the end (the weights of
population 1's step 2 are so uneven that torch.cov's 1 - sum(w^2) rounds to nothing and the reference clamps the variance), so the
sphere was moved: C = the nominal position after step 3 + (0, 0, 0.3), R = 0.29 -- 70 of the 72 possible rows, one collision in each
of populations 0 and 1, no message (CEM_C / CEM_R override it, CEM_DRY=1 only reports)."""
import contextlib
import csv
import io
import os
import sys
import tempfile
import types
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (shims, sys.path of the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerfsafetyvalidation_amd import rollout as RO  # noqa: E402

STEPS, M, M_ELITE, KMAX = 4, 6, 3, 3
SIGMA = (0.02, 0.4, 0.3)
C = [float(v) for v in os.environ["CEM_C"].split(",")] if "CEM_C" in os.environ else [-0.0375, -0.614, 0.5875]
R = float(os.environ.get("CEM_R", "0.29"))


def main():
    import matplotlib
    matplotlib.use("Agg")
    sns = types.ModuleType("seaborn")
    sns.histplot = lambda *a, **k: None
    sys.modules.setdefault("seaborn", sns)
    import matplotlib.pyplot as plt
    import validation.stresstests.CrossEntropyMethod as CEM
    import validation.distributions.SeedableMultivariateNormal as SMN
    from nav.agent_helpers import Agent
    from validation.simulators.NerfSimulator import NerfSimulator

    x0 = RO.initial_state(STEPS)
    centre = np.asarray(C, np.float64)

    class Sim(NerfSimulator):
        def __init__(self):
            self.uq_method = "Gaussian Approximation"

        def reset(self):
            eye = torch.eye(3)
            self.agent = SimpleNamespace(dt=RO.ENV["T_final"] / STEPS, g=RO.ENV["g"], mass=RO.ENV["mass"], I=eye, invI=torch.inverse(eye),
                                         x=x0.clone(), data={}, states_history=[], iter=0)
            self.agent.drone_dynamics = lambda s_, a_: Agent.drone_dynamics(self.agent, s_, a_)
            self.agent.get_img = lambda data: np.zeros((2, 2, 3), np.uint8)

        def step(self, disturbance):
            action = torch.tensor([RO.ENV["mass"] * RO.ENV["g"], 0.0, 0.0, 0.0])
            _, true_state, _ = Agent.step(self.agent, action, noise=disturbance)
            value = float(np.linalg.norm(np.asarray(true_state[:3], np.float64) - centre) - R)
            sigma = SIGMA[0] + SIGMA[1] * abs(float(true_state[0])) + SIGMA[2] * abs(float(true_state[7]))
            return value < 0, value, true_state[:3], sigma, None

    fits, draws = [], []

    class Spy(SMN.SeedableMultivariateNormal):
        def __init__(self, means, covs, noise_seed=None):
            super().__init__(means, covs, noise_seed)
            fits.append((np.stack([np.asarray(m_, np.float32) for m_ in means]), np.stack([np.asarray(c, np.float32) for c in covs])))

        def sample(self, simulationNumber):
            out = super().sample(simulationNumber)
            draws.append(np.stack([o.numpy() for o in out]))
            return out

        def compute_best_solution(self, simulator):
            return None, None, None

    real_cuda, real_savefig, real_smn, real_blender = torch.Tensor.cuda, plt.savefig, CEM.SeedableMultivariateNormal, CEM.runBlenderOnFailure
    mean = torch.tensor(RO.ENV["mpc_noise_mean"], dtype=torch.float32)
    std = torch.tensor(RO.ENV["mpc_noise_std"], dtype=torch.float32)
    cov = torch.stack([torch.square(torch.diag(std))] * STEPS)                       # validate.py:32
    gen = torch.Generator()                                                          # validate.py:35 (on the CPU here)
    seed = gen.initial_seed()
    cwd, log = os.getcwd(), io.StringIO()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "results", "pltpaths"))
        os.chdir(tmp)
        torch.Tensor.cuda = lambda self, *a, **k: self
        plt.savefig = lambda *a, **k: None
        CEM.SeedableMultivariateNormal, CEM.runBlenderOnFailure = Spy, lambda *a, **k: None
        try:
            with contextlib.redirect_stdout(log):
                q = Spy([mean] * STEPS, cov, noise_seed=gen)
                p = Spy([mean] * STEPS, cov, noise_seed=gen)
                cem = CEM.CrossEntropyMethod(Sim(), q, p, M, M_ELITE, KMAX, gen, None, None, 0, 0)
                cem.optimize()
            with open(os.path.join(tmp, "results", f"collisionValuesCEM_m{M}melite{M_ELITE}k{KMAX}.csv")) as fh:
                rows = [[float(v) if v not in ("True", "False") else float(v == "True") for v in r] for r in csv.reader(fh)]
        finally:
            os.chdir(cwd)
            torch.Tensor.cuda, plt.savefig = real_cuda, real_savefig
            CEM.SeedableMultivariateNormal, CEM.runBlenderOnFailure = real_smn, real_blender
            plt.close("all")
    rows = np.asarray(rows, np.float64)
    out = log.getvalue()
    assert len(fits) == 2 + KMAX and len(draws) == KMAX * M
    noises = np.stack(draws).reshape(KMAX, M, STEPS, 12)
    means = np.stack([f[0] for f in fits[2:]])                                       # [KMAX, STEPS, 12]: q after population k
    cov_diags = np.stack([np.diagonal(f[1], axis1=-2, axis2=-1) for f in fits[2:]])
    for f in fits[2:]:
        assert np.array_equal(f[1], np.stack([np.diag(np.diag(c)) for c in f[1]]))   # diagonal only (:243-249)
    ever = np.array([[rows[(rows[:, 0] == k) & (rows[:, 1] == s)][-1, 26] for s in range(M)] for k in range(KMAX)])
    risks = np.array([[rows[(rows[:, 0] == k) & (rows[:, 1] == s)][:, 17].min() for s in range(M)] for k in range(KMAX)])
    elite = np.stack([np.argsort(r_)[:M_ELITE] for r_ in risks])
    gaps = []
    for r_ in risks:
        s_ = np.sort(r_)
        gaps.append((s_[M_ELITE] - s_[M_ELITE - 1]) / (s_[-1] - s_[0]))
    print(f"C {C} R {R}: {rows.shape[0]} of {KMAX * M * STEPS} rows, collided per population {ever.sum(1)}, elite {elite.tolist()}, "
          f"elite-boundary gaps / range {np.round(gaps, 4)}")
    said = [line[:120] for line in out.splitlines() if any(word in line for word in ("Clamping", "Exiting", "Negative/zero weights"))]
    if os.environ.get("CEM_DRY"):
        print(f"messages: {said}")
        return
    assert not said, f"the reference printed {said}: move the sphere"
    assert ever.any() and not ever.all(), "every simulation (or none) collided: move the sphere"
    assert min(gaps) >= 1e-3, "an elite boundary is not separated: move the sphere"
    MG.save("cem.npz", rows=rows, means=means, cov_diags=cov_diags, noises=noises, risks=risks, elite_indices=elite, steps=STEPS, m=M,
            m_elite=M_ELITE, kmax=KMAX, generator_seed=np.int64(seed), sigma_coeffs=np.array(SIGMA), centre=centre, radius=np.float64(R))


if __name__ == "__main__":
    main()
