"""The Cross Entropy Method stress test (validate.py:28-46: envConfig.json's stress_test == "Cross Entropy Method") around the same
simulation step as the Monte-Carlo rollout (rollout.RolloutSimulator).

What the reference runs (validation/stresstests/CrossEntropyMethod.py:49-305, validation/distributions/SeedableMultivariateNormal.py):

    p = q = one N(noise mean, diag(std^2)) per step                    validate.py:31-38
    for k in start_k .. kmax-1:                                        CrossEntropyMethod.py:66
        for simulation in 0 .. m-1:                                    :79
            noises = q.sample(simulation)      manual_seed(seed + simulation), one draw per step       :82, SeedableMultivariateNormal.py:19-22
            per step: NerfSimulator.step(noise); the row holds the reward of the PREVIOUS step (:112), then
                reward   = simulator.reward(p_step.log_prob(noise), sigma, trace)                      :114-115
                adjusted = value - reward * 0.01 * value                                               :118-122
                log p, log q of the noise, their running sums, collided                                :129-143
            risk = min over the steps of `adjusted`; the first collision ends the simulation           :149-166
        elite = the m_elite lowest risks                                                                :215
        per step i: w = exp(log p_i(x) - log q_i(x) - logsumexp), mean = w @ x, cov = diag(clamp(diag(cov(x, aweights=w))))   :224-251
        q = SeedableMultivariateNormal(means, covs, seed); a ValueError (e.g. a zero variance) ends the loop with the old q    :264-271

Quirks kept: every population draws with the SAME seeds (seed + simulation), only q changes; the reward that adjusts a step's value is
the one computed FROM that step (the row's reward column is the previous one); only the diagonal of the refitted covariance is kept.

All of a CEM step that touches the GPU is the rollout's own path (the renders, the UQ, the planner, the SDF); the refit is `steps`
twelve-dimensional Gaussians on m_elite samples and runs on the host.  A population is a set of independent simulations, so it runs
like run_rollout's: sharded over ranks (dist.shard_range), `in_flight` at a time on streams (pipeline.FramePipeline), ONE
gather_views of the padded rows per population; every rank then computes the same refit from the same rows (elite noises are
re-drawn from q, which is deterministic given the simulation number), so no other collective is needed.

Not ported: the plots and seaborn histograms, the Blender call, the TOY_PROBLEM branch, and `start_iter` (in the reference it skips
simulations in EVERY population, not only the resumed one).  The reference's compute_best_solution cannot run against NerfSimulator
(SeedableMultivariateNormal.py:36 unpacks three of step()'s five values); best_solution() here is what it evidently means
(DESIGN.md)."""
import contextlib

import numpy as np
import torch
from torch.distributions import MultivariateNormal

from . import rollout as RO
from .dist import shard_range

CEM_ROW_WIDTH = 27   # CrossEntropyMethod.py:173-189: population, simulation, step, noise x12, reward applied, uncertainty, adjusted sdf
#                      value, xyz, step log p, step log q, cumulative log p, cumulative log q, collided (+ ever collided)
COV_MAX = 0.1        # :245-247
MIN_WEIGHT = 1e-8    # :237


class SeedableMultivariateNormal:
    """SeedableMultivariateNormal.py:13-22: one MultivariateNormal per step (float32, on the host) and a seed; simulation `sim` draws
    its `steps` noises in step order from a generator seeded seed + sim.  The reference seeds the GLOBAL generator
    (torch.manual_seed(seed + sim); [d.sample() ...]); the values here are the same, drawn from a generator of this call's own, so
    that simulations on several host threads do not disturb each other (or anyone else's global state)."""

    def __init__(self, means, covs, seed):
        self.means = [torch.as_tensor(m_, dtype=torch.float32).cpu() for m_ in means]
        self.covs = [torch.as_tensor(c, dtype=torch.float32).cpu() for c in covs]
        self.noise_seed = int(seed)
        self.distributions = [MultivariateNormal(m_, c) for m_, c in zip(self.means, self.covs)]    # ValueError: not positive definite

    def __len__(self):
        return len(self.distributions)

    def sample(self, sim):
        """-> list of `steps` tensors [12].  MultivariateNormal.rsample restated with a generator: loc + scale_tril @ eps,
        eps = empty(shape).normal_() (torch/distributions/multivariate_normal.py, utils._standard_normal; _unbroadcasted_scale_tril is
        the distribution's own Cholesky factor, a private attribute as of torch 2.10 -- tests/test_cem_cpu.py holds the draws against
        d.sample())"""
        gen = torch.Generator().manual_seed(self.noise_seed + int(sim))
        out = []
        for d in self.distributions:
            eps = torch.empty(d.loc.shape, dtype=d.loc.dtype).normal_(generator=gen)
            out.append(d.loc + torch.matmul(d._unbroadcasted_scale_tril, eps.unsqueeze(-1)).squeeze(-1))
        return out

    def log_prob(self, step, x):
        """torch.distributions' float32 log-density of step `step` at x [..., 12] (CrossEntropyMethod.py:114,129-130,226)"""
        return self.distributions[step].log_prob(torch.as_tensor(x, dtype=torch.float32))


def target_distribution(steps, seed):
    """validate.py:31-38: ENV's noise mean and diag(std^2) at every step"""
    mean = torch.tensor(RO.ENV["mpc_noise_mean"], dtype=torch.float32)
    cov = torch.square(torch.diag(torch.tensor(RO.ENV["mpc_noise_std"], dtype=torch.float32)))
    return SeedableMultivariateNormal([mean] * steps, [cov] * steps, seed)


def _logsumexp(a):
    """scipy.special.logsumexp (CrossEntropyMethod.py:229) for a 1-D float32 tensor: log(sum(exp(a - max))) + max"""
    a_max = a.max()
    return torch.log(torch.exp(a - a_max).sum()) + a_max


def refit(elite_samples, p, q):
    """CrossEntropyMethod.py:221-251 per step.  elite_samples [m_elite, steps, 12] float32 -> (means: list of [12], covs: list of
    [12, 12] diagonal, info: {"weights_clamped": bool [steps], "cov_clamped": bool [steps]})"""
    x_all = torch.as_tensor(elite_samples, dtype=torch.float32)
    steps = x_all.shape[1]
    means, covs = [], []
    info = {"weights_clamped": np.zeros(steps, bool), "cov_clamped": np.zeros(steps, bool)}
    for i in range(steps):
        x = x_all[:, i]
        log_w = p.log_prob(i, x) - q.log_prob(i, x)
        w = torch.exp(log_w - _logsumexp(log_w))
        if torch.any(w <= 0):                                    # :235-237
            info["weights_clamped"][i] = True
            w = torch.clamp(w, min=MIN_WEIGHT)
        mean = w @ x                                             # :240
        diag = torch.cov(x.T, aweights=w).diag()                 # :241-244
        if (diag > COV_MAX).any() or (diag < 0).any():           # :245-247
            info["cov_clamped"][i] = True
            diag = torch.clamp(diag, 0, COV_MAX)
        means.append(mean)
        covs.append(torch.diag(diag))
    return means, covs, info


class CEMSimulator(RO.RolloutSimulator):
    """One simulation of a CEM population (CrossEntropyMethod.py:79-166): RolloutSimulator's step with the noise drawn from q and the
    CEM row.  The collision flag is the simulator's own; the reward only adjusts the value that ranks the simulation."""

    def __init__(self, *args, p=None, q=None, population=0, **kwargs):
        super().__init__(*args, **kwargs)
        self.p, self.q, self.population = p, q, population

    def begin(self, sim):
        self._noises = self.q.sample(sim)                        # :82
        self._reward = 0.0
        self._cum_p = torch.zeros((), dtype=torch.float32)       # (:132-133: float32 running sums)
        self._cum_q = torch.zeros((), dtype=torch.float32)
        self.raw_values = []

    def draw_noise(self, sim, k):
        return self._noises[k]

    def write_row(self, sim, k, noise, value, where, sigma_d, collided):
        applied = self._reward                                   # :112: the reward of the previous step, 0 at step 0
        p_step, q_step = self.p.log_prob(k, noise), self.q.log_prob(k, noise)
        self._reward = self.reward(float(p_step), sigma_d)       # :114-115
        self.raw_values.append(value)
        adjusted = value - self._reward * (0.01 * value)         # :118-122
        self._cum_p = self._cum_p + p_step
        self._cum_q = self._cum_q + q_step
        return [self.population, sim, k, *noise.tolist(), applied, sigma_d, adjusted, *where.tolist(), p_step.item(), q_step.item(),
                self._cum_p.item(), self._cum_q.item(), float(collided)]


def simulation_risks(rows, population, m):
    """CrossEntropyMethod.py:166: per simulation of `population`, the smallest adjusted value of its steps -> float64 [m]"""
    pop = rows[rows[:, 0] == population]
    return np.array([pop[pop[:, 1] == s][:, 17].min() for s in range(m)], np.float64)


def select_elite(risks, m_elite):
    """:215: the m_elite lowest risks; ties go to the lower simulation number"""
    return np.argsort(risks, kind="stable")[:m_elite]


def failure_probability(rows):
    """The importance-sampling estimate the cumulative log p / log q and "ever collided" columns exist for.  Per population: the mean
    over its simulations of 1[ever collided] * exp(sum log p - sum log q) (the sums at the simulation's last row), float64.
    -> {"populations": [..], "per_population": [..], "pooled": the same mean over all simulations of all populations,
        "collisions": [..] per population, "mean_steps_to_collision": [..] per population, NaN without a collision (the two figures
        CrossEntropyMethod.py:170-171 prints: the collision step's number, averaged)}"""
    rows = np.asarray(rows, np.float64)
    pops = np.unique(rows[:, 0])
    per_pop, collisions, mean_steps, terms_all = [], [], [], []
    for k in pops:
        pop = rows[rows[:, 0] == k]
        terms, steps_to = [], []
        for s in np.unique(pop[:, 1]):
            last = pop[pop[:, 1] == s][-1]
            hit = last[26] != 0
            terms.append(np.exp(last[23] - last[24]) if hit else 0.0)
            if hit:
                steps_to.append(last[2])
        per_pop.append(float(np.mean(terms)))
        collisions.append(len(steps_to))
        mean_steps.append(float(np.mean(steps_to)) if steps_to else float("nan"))
        terms_all.extend(terms)
    return {"populations": [int(k) for k in pops], "per_population": per_pop, "pooled": float(np.mean(terms_all)),
            "collisions": collisions, "mean_steps_to_collision": mean_steps}


def _lowest_value_step(q, simulator, sim):
    simulator.q = q
    rows = simulator.run(sim)
    best = int(np.argmin(np.asarray(simulator.raw_values[:rows.shape[0]], np.float64)))
    return q.means[best], q.covs[best], float(simulator.raw_values[best])


def best_solution(q, simulator, sim):
    """What SeedableMultivariateNormal.compute_best_solution (:24-45) evidently means: ONE more simulation with noises from `q`, here
    seeded as simulation `sim` (run_cem: seed + m), on `simulator` (a CEMSimulator) -> (mean, cov, value) of the step with the lowest
    RAW sdf value (the first such step; a collision ends the simulation, :43)."""
    return _lowest_value_step(q, simulator, sim)


def run_cem(model, intrinsics, H, W, steps, m=10, m_elite=5, kmax=5, seed=0, q=None, start_k=0, sdf=None, best_solution=False, rank=0,
            world_size=1, group=None, in_flight=3, render_kwargs=None, autocast=True, gather=True, renders_per_step=2, planner_cfg=None,
            estimator_cfg=None, uq_method=RO.UQ_GAUSSIAN, uq_kwargs=None, world=None, body=None, exact=False, clearance=None):
    """CrossEntropyMethod.optimize() with every population run like run_rollout's simulations.  m, m_elite, kmax: validate.py:39's
    10, 5, 5.  q: the proposal to start from (default: the target p); with start_k it is the reference's `--k` resume.  sdf: a
    collision.SignedDistanceField, REQUIRED (the analytic 0 / 9999 stand-in gives CEM nothing to rank), or "world": the ground-truth
    field of `world`'s mesh (SignedDistanceField.from_mesh over reference_box(), built once here; a ValueError without world=).  The other keywords are
    run_rollout's (world: the world.MeshWorld every simulation's sensor looks at, or None; body / exact: the collision.BodyBox the collisions are judged with, or None; clearance: None, or the cap D of the body's gap that then is the value `adjusted`, the risk and the elite are built from); the refit needs every rank's rows, so gather=False is only accepted on one rank.
    Returns (rows [total, CEM_ROW_WIDTH] float64 in (population, simulation, step) order, result, this rank's counters).  result:
    means / covs / q (the final proposal), population_scores / elite_scores (the two series the reference plots, :209,220),
    elite_indices, refit_info and the refitted population_means / population_covs per population, stopped_early (None, or the population whose refit gave no valid q -- the
    reference's ValueError branch, :264-271; q is then the last valid one), and with best_solution=True best_solution's triple
    (simulation number m, i.e. seeded seed + m; every rank runs it, it is one simulation and deterministic)."""
    from .collision import check_body, check_clearance, resolve_sdf
    sdf = resolve_sdf(sdf, world, "run_cem")
    check_body(body, exact, sdf, world, "run_cem")
    check_clearance(clearance, body, "run_cem")
    if sdf is None:
        raise ValueError("run_cem: sdf is required (the analytic stand-in's 0 / 9999 gives the Cross Entropy Method nothing to rank)")
    if not 0 < m_elite <= m:
        raise ValueError(f"run_cem: m_elite {m_elite} must be in 1..m ({m})")
    if world_size > 1 and not gather:
        raise ValueError("run_cem: every rank refits from all rows; gather=False needs world_size == 1")
    device = next(model.parameters()).device
    p = target_distribution(steps, seed)
    q = p if q is None else q
    if len(q) != steps:
        raise ValueError(f"run_cem: q has {len(q)} steps, the simulation {steps}")
    lo, hi = shard_range(m, rank, world_size)
    sims = list(range(lo, hi))
    counters = {"frames": 0, "simulations": 0, "steps": 0}
    plan0 = RO.initial_plan(model, planner_cfg, seed) if planner_cfg is not None and sims else None

    def make(population, q_k):
        return CEMSimulator(model, intrinsics, H, W, steps, seed=seed, render_kwargs=render_kwargs, renders_per_step=renders_per_step,
                            planner_cfg=planner_cfg, initial_plan=plan0, sdf=sdf, estimator_cfg=estimator_cfg, uq_method=uq_method,
                            uq_kwargs=uq_kwargs, world=world, body=body, exact=exact, clearance=clearance, p=p, q=q_k,
                            population=population)

    result = {"population_scores": [], "elite_scores": [], "elite_indices": [], "refit_info": [], "population_means": [],
              "population_covs": [], "stopped_early": None}
    all_rows = []
    pipe = RO.simulation_pipeline(sims, in_flight, device)      # one pool of threads and streams for all populations
    with pipe if pipe is not None else contextlib.nullcontext():
        for k in range(start_k, kmax):
            def one(sim, k=k, q_k=q):
                sim_obj = make(k, q_k)
                with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                    rows = sim_obj.run(sim)
                return rows, sim_obj.frames

            results = RO.run_simulations(one, sims, in_flight, device, pipe)
            counters["simulations"] += len(sims)
            for rows, frames in results:
                counters["frames"] += frames
                counters["steps"] += rows.shape[0]
            rows_k = RO.gather_rows(results, m, steps, CEM_ROW_WIDTH, world_size, group, device, gather)
            all_rows.append(rows_k)
            # ---- from here on every rank computes the same thing from the same rows
            risks = simulation_risks(rows_k, k, m)
            elite = select_elite(risks, m_elite)
            result["population_scores"].append(float(risks.mean()))
            result["elite_scores"].append(float(risks[elite].mean()))
            result["elite_indices"].append(elite.copy())
            elite_samples = torch.stack([torch.stack(q.sample(int(s))) for s in elite])      # (:216: whole trajectories, drawn again)
            means, covs, info = refit(elite_samples, p, q)
            result["refit_info"].append(info)
            result["population_means"].append(means)
            result["population_covs"].append(covs)
            try:
                q = SeedableMultivariateNormal(means, covs, seed)
            except (ValueError, torch.linalg.LinAlgError):
                result["stopped_early"] = k
                break
    result.update(means=q.means, covs=q.covs, q=q)
    if best_solution:
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            result["best_solution"] = _lowest_value_step(q, make(kmax, q), m)
    rows = np.concatenate(all_rows, 0) if all_rows else np.zeros((0, CEM_ROW_WIDTH), np.float64)
    return rows, result, counters
