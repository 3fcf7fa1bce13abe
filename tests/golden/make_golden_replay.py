#!/usr/bin/env python3
"""Generates tests/golden/replay.npz by running the REFERENCE's own replay_MC() and replay_CEM()
(validation/utils/replay/replay_MC.py, replay_CEM.py) on CPU, each on a results/*.csv that the reference's own stress loop wrote
(MonteCarlo.validate() as make_golden.py::gen_rollout runs it, CrossEntropyMethod.optimize() as make_golden_cem.py runs it).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_replay.py

Two worlds: the stress loops judge collisions against an analytic sphere A ("the NeRF's world"), the replays against another sphere B
("the true world").  In both, the simulator is the stub of the other generators: step() keeps the reference's Agent.step (drone
dynamics + noise) with a hover action; the collision value is |pos - C| - R (float64 of the float32 position) and collided =
value < 0; the stress stub's sigma is make_golden_cem.py's fixed function of the state.  The replays' BlenderSimulator is that stub
with sphere B and three return values (BlenderSimulator.step's).
Patched IN MEMORY only, nothing of the reference is copied or changed: `seaborn` is a stub module (histplot, heatmap), `gym` is
make_golden.py's, Tensor.cuda() returns the tensor, runBlenderOnFailure is a no-op in the stress loops and a spy that records
(n_sim, step, populationNum) in the replays, plt.savefig and plt.show are discarded, compute_best_solution is stubbed as in
make_golden_cem.py; the working directory is a temporary one with results/ (the replays find their csv there and write
results/replays/collisionValuesReplay.csv and counts.pkl).
Stored per replay (prefix mc_ / cem_): the input CSV rows, collisionValuesReplay.csv's rows, the eight counts in counts.pkl's order
(tp, tn, fp, fn per step, then per trajectory), the spy's calls (population -1: none); and steps, the simulation counts, the seed of
the CEM generator and of the Monte-Carlo generator, the stub's sigma coefficients and the two spheres.
The spheres: A is make_golden_cem.py's centre (the nominal position after step 3 + (0, 0, 0.3)) with R = 0.33, so that about half of
the stress loops' simulations collide; B = (-0.098, -0.6, 0.595), R = 0.335 -- moved mostly across the flight direction, so that each
world has a region the other lacks.  A first try (B = A moved by (0.012, -0.008, 0.004), equal radii; m = 6) left the false-positive
and false-negative cells empty; a random search over B (shifts of 0.03, radii 0.30 .. 0.34) with m = 10, m_elite = 5 found this pair.
The conditions asserted at the end decide whether a pair of spheres will do
(REPLAY_A / REPLAY_B = "cx,cy,cz,r" override them, REPLAY_DRY=1 only reports): all four per-step cells non-zero in both replays, at
least three per-trajectory cells non-zero in the Monte-Carlo replay, and a replayed simulation that collides before its last recorded
step (the "remaining steps are false negatives" rule)."""
import contextlib
import csv
import io
import os
import pickle
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

STEPS, N_SIMS = 4, 16
M, M_ELITE, KMAX = 10, 5, 3
SIGMA = (0.02, 0.4, 0.3)


def _sphere(name, default):
    v = [float(x) for x in os.environ[name].split(",")] if name in os.environ else default
    return np.asarray(v[:3], np.float64), float(v[3])


A = _sphere("REPLAY_A", [-0.0375, -0.614, 0.5875, 0.33])
B = _sphere("REPLAY_B", [-0.098, -0.6, 0.595, 0.335])


def _rows(path):
    with open(path) as fh:
        return np.asarray([[float(v) if v not in ("True", "False") else float(v == "True") for v in r] for r in csv.reader(fh)], np.float64)


def main():
    import matplotlib
    matplotlib.use("Agg")
    sns = types.ModuleType("seaborn")
    sns.histplot = lambda *a, **k: None
    sns.heatmap = lambda *a, **k: None
    sys.modules.setdefault("seaborn", sns)
    import matplotlib.pyplot as plt
    import validation.stresstests.CrossEntropyMethod as CEM
    import validation.stresstests.MonteCarlo as MC
    import validation.distributions.SeedableMultivariateNormal as SMN
    import validation.utils.replay.replay_CEM as RCEM
    import validation.utils.replay.replay_MC as RMC
    from nav.agent_helpers import Agent
    from validation.simulators.NerfSimulator import NerfSimulator

    x0 = RO.initial_state(STEPS)

    def fresh_agent(owner):
        eye = torch.eye(3)
        owner.agent = SimpleNamespace(dt=RO.ENV["T_final"] / STEPS, g=RO.ENV["g"], mass=RO.ENV["mass"], I=eye, invI=torch.inverse(eye),
                                      x=x0.clone(), data={}, states_history=[], iter=0)
        owner.agent.drone_dynamics = lambda s_, a_: Agent.drone_dynamics(owner.agent, s_, a_)
        owner.agent.get_img = lambda data: np.zeros((2, 2, 3), np.uint8)

    def hover_step(owner, disturbance, sphere):
        action = torch.tensor([RO.ENV["mass"] * RO.ENV["g"], 0.0, 0.0, 0.0])
        _, true_state, _ = Agent.step(owner.agent, action, noise=disturbance)
        value = float(np.linalg.norm(np.asarray(true_state[:3], np.float64) - sphere[0]) - sphere[1])
        return value < 0, value, true_state

    class Stress(NerfSimulator):                                 # the NeRF's world: sphere A
        def __init__(self):
            self.uq_method = "Gaussian Approximation"

        def reset(self):
            fresh_agent(self)

        def step(self, disturbance):
            collided, value, st = hover_step(self, disturbance, A)
            return collided, value, st[:3], SIGMA[0] + SIGMA[1] * abs(float(st[0])) + SIGMA[2] * abs(float(st[7])), None

    class Truth:                                                 # BlenderSimulator's stand-in, the true world: sphere B
        def __init__(self, *args, **kwargs):
            pass

        def reset(self):
            fresh_agent(self)

        def step(self, disturbance):
            collided, value, st = hover_step(self, disturbance, B)
            return collided, value, st[:3]

    class Q(SMN.SeedableMultivariateNormal):
        def compute_best_solution(self, simulator):
            return None, None, None

    calls = []

    def spy(blend_file, workspace, n_sim, step, outputSimulationList, populationNum=None):
        calls.append((int(n_sim), int(step), -1 if populationNum is None else int(populationNum)))

    mean = torch.tensor(RO.ENV["mpc_noise_mean"], dtype=torch.float32)
    std = torch.tensor(RO.ENV["mpc_noise_std"], dtype=torch.float32)
    keep = dict(cuda=torch.Tensor.cuda, savefig=plt.savefig, show=plt.show, smn=CEM.SeedableMultivariateNormal, cem_blender=CEM.runBlenderOnFailure,
                mc_blender=MC.runBlenderOnFailure, rmc=(RMC.BlenderSimulator, RMC.runBlenderOnFailure),
                rcem=(RCEM.BlenderSimulator, RCEM.runBlenderOnFailure))
    cwd, log, out = os.getcwd(), io.StringIO(), {}
    torch.Tensor.cuda = lambda self, *a, **k: self
    plt.savefig = plt.show = lambda *a, **k: None
    CEM.SeedableMultivariateNormal, CEM.runBlenderOnFailure, MC.runBlenderOnFailure = Q, (lambda *a, **k: None), (lambda *a, **k: None)
    RMC.BlenderSimulator, RMC.runBlenderOnFailure, RCEM.BlenderSimulator, RCEM.runBlenderOnFailure = Truth, spy, Truth, spy
    try:
        for kind in ("mc", "cem"):
            with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(log):
                os.makedirs(os.path.join(tmp, "results", "pltpaths"))
                os.chdir(tmp)
                del calls[:]
                if kind == "mc":
                    mc = MC.MonteCarlo(Stress(), N_SIMS, STEPS, mean, std, None, None, 0)
                    out["mc_seed"] = mc.noise_seed.initial_seed()
                    mc.validate()
                    RMC.replay_MC(None, None, mean, std, None, None, None, None, None, None, None, None, None, None, 0, 0)
                else:
                    gen = torch.Generator()
                    out["cem_seed"] = gen.initial_seed()
                    cov = torch.stack([torch.square(torch.diag(std))] * STEPS)
                    q, p = Q([mean] * STEPS, cov, noise_seed=gen), Q([mean] * STEPS, cov, noise_seed=gen)
                    CEM.CrossEntropyMethod(Stress(), q, p, M, M_ELITE, KMAX, gen, None, None, 0, 0).optimize()
                    RCEM.replay_CEM(None, None, mean, std, None, None, None, None, None, None, None, None, None, None, 0, 0, 0)
                stress = [f for f in os.listdir("results") if f.lower().endswith(".csv")]
                assert len(stress) == 1
                out[kind + "_input"] = _rows(os.path.join("results", stress[0]))
                out[kind + "_replay"] = _rows(os.path.join("results", "replays", "collisionValuesReplay.csv"))
                with open("counts.pkl", "rb") as fh:
                    out[kind + "_counts"] = np.asarray([int(c) for c in pickle.load(fh)], np.int64)
                out[kind + "_calls"] = np.asarray(calls, np.int64).reshape(-1, 3)
                os.chdir(cwd)
    finally:
        os.chdir(cwd)
        torch.Tensor.cuda, plt.savefig, plt.show = keep["cuda"], keep["savefig"], keep["show"]
        CEM.SeedableMultivariateNormal, CEM.runBlenderOnFailure, MC.runBlenderOnFailure = keep["smn"], keep["cem_blender"], keep["mc_blender"]
        (RMC.BlenderSimulator, RMC.runBlenderOnFailure), (RCEM.BlenderSimulator, RCEM.runBlenderOnFailure) = keep["rmc"], keep["rcem"]
        plt.close("all")
    early = {}
    for kind, sim_col in (("mc", 0), ("cem", 1)):
        inp, rep, c = out[kind + "_input"], out[kind + "_replay"], out[kind + "_counts"]
        early[kind] = int(inp.shape[0] - rep.shape[0])          # recorded steps the replay never reached: it collided before them
        print(f"{kind}: {inp.shape} input rows, {rep.shape} replay rows, counts (tp, tn, fp, fn) step {c[:4].tolist()} traj {c[4:].tolist()}, "
              f"{len(out[kind + '_calls'])} view calls, {early[kind]} recorded steps after a replay collision")
    if os.environ.get("REPLAY_DRY"):
        return out, early
    for kind in ("mc", "cem"):
        c = out[kind + "_counts"]
        assert (c[:4] > 0).all(), f"{kind}: a per-step cell is empty: move the spheres"
        assert c[:4].sum() == out[kind + "_input"].shape[0]      # every recorded step is counted once (the remaining ones as fn)
    assert (out["mc_counts"][4:] > 0).sum() >= 3, "mc: fewer than three per-trajectory cells: move the spheres"
    assert early["mc"] > 0 or early["cem"] > 0, "no replayed simulation collides before its last recorded step: move the spheres"
    assert out["mc_input"].shape[1] == 24 and out["cem_input"].shape[1] == 27 and out["mc_replay"].shape[1] == 22 and out["cem_replay"].shape[1] == 23
    MG.save("replay.npz", steps=STEPS, n_simulations=N_SIMS, m=M, m_elite=M_ELITE, kmax=KMAX, mc_seed=np.int64(out["mc_seed"]), cem_seed=np.int64(out["cem_seed"]),
            sigma_coeffs=np.array(SIGMA), centre_a=A[0], radius_a=np.float64(A[1]), centre_b=B[0], radius_b=np.float64(B[1]),
            **{k: v for k, v in out.items() if not k.endswith("_seed")})


if __name__ == "__main__":
    main()
