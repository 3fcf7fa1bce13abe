"""The Cross Entropy Method stress test (nerfsafetyvalidation_amd/cem.py) on CPU: its rows, elite selection and refits against what the
reference's own CrossEntropyMethod.optimize() wrote (tests/golden/cem.npz, made by make_golden_cem.py), `refit` against a float64
restatement on hand-built elites, the seedable distribution, the sharded run over two gloo ranks and the importance-sampling estimate.
No rendering here (that is test_cem_gpu.py): observe and collision are overridden with the fixture's stand-ins."""
import os
import socket
import threading

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = float(np.finfo(np.float32).eps)


class _FakeModel:
    def parameters(self):
        return iter([torch.zeros(1)])


_state = {}


def _sim_class():
    """the fixture's stub: sigma a function of the state, the collision value the distance to a sphere, evaluated at the state itself"""
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import rollout as RO
    z = np.load(os.path.join(G, "cem.npz"))
    a, b, c = [float(v) for v in z["sigma_coeffs"]]
    centre, radius = z["centre"].astype(np.float64), float(z["radius"])

    class Sim(CE.CEMSimulator):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.n_interp = 1                                  # the stub looks at the new state only

        def observe(self, pose):
            st = _state["state"]
            return a + b * abs(float(st[0])) + c * abs(float(st[7]))

        def collision(self, xyz):
            v = float(np.linalg.norm(np.asarray(xyz, np.float64) - centre) - radius)
            return v < 0, v

    return CE, RO, Sim, z


class _patched:
    """CE.CEMSimulator = Sim, and RO.camera_pose hands the state it was called with to Sim.observe (as test_rollout.py does)"""

    def __init__(self, CE, RO, Sim):
        self.CE, self.RO, self.Sim = CE, RO, Sim

    def __enter__(self):
        self.keep = (self.CE.CEMSimulator, self.RO.camera_pose)
        orig = self.RO.camera_pose

        def spy(state):
            _state["state"] = state
            return orig(state)

        self.CE.CEMSimulator, self.RO.camera_pose = self.Sim, spy

    def __exit__(self, *exc):
        self.CE.CEMSimulator, self.RO.camera_pose = self.keep
        return False


def refit_f64(x, mean_p, var_p, mean_q, var_q):
    """CrossEntropyMethod.py:224-251 for ONE step in float64, diagonal Gaussians: x [n, 12] -> (mean [12], variance [12] after the
    clamp, weights clamped?, variance clamped?).  A weight counts as <= 0 when it is in float32, where the reference computes it."""
    x, mean_p, var_p, mean_q, var_q = [np.asarray(v, np.float64) for v in (x, mean_p, var_p, mean_q, var_q)]

    def logpdf(mu, var):
        return (-0.5 * (x - mu) ** 2 / var - 0.5 * np.log(2 * np.pi * var)).sum(1)

    lw = logpdf(mean_p, var_p) - logpdf(mean_q, var_q)
    lw = lw - (np.log(np.exp(lw - lw.max()).sum()) + lw.max())
    w = np.exp(lw)
    w_clamped = bool((w.astype(np.float32) <= 0).any())
    if w_clamped:
        w = np.maximum(w, 1e-8)
    mean = w @ x
    avg = (w[:, None] * x).sum(0) / w.sum()                    # torch.cov with aweights, correction = 1
    var = (w[:, None] * (x - avg) ** 2).sum(0) / (w.sum() - (w * w).sum() / w.sum())
    v_clamped = bool((var > 0.1).any() or (var < 0).any())
    if v_clamped:
        var = np.clip(var, 0, 0.1)
    return mean, var, w_clamped, v_clamped


def _target(CE, RO, steps, seed=0):
    return CE.target_distribution(steps, seed), np.asarray(RO.ENV["mpc_noise_mean"], np.float64), np.asarray(RO.ENV["mpc_noise_std"], np.float64) ** 2


@pytest.fixture(scope="module")
def cem_run():
    """ONE run of the port on the fixture's configuration, shared by the tests below (not modified by them)"""
    CE, RO, Sim, z = _sim_class()
    steps, m, m_elite, kmax = [int(z[k]) for k in ("steps", "m", "m_elite", "kmax")]
    with _patched(CE, RO, Sim):
        rows, result, counters = CE.run_cem(_FakeModel(), None, 8, 8, steps, m=m, m_elite=m_elite, kmax=kmax, seed=int(z["generator_seed"]),
                                            sdf=object(), in_flight=1, autocast=False, best_solution=True)
    return CE, RO, z, rows, result, counters


def test_population_0_and_every_exact_column_match_the_reference(cem_run):
    CE, RO, z, rows, result, counters = cem_run
    want = z["rows"]
    assert rows.shape == want.shape and rows.shape[1] == CE.CEM_ROW_WIDTH == 27
    np.testing.assert_array_equal(rows[:, :3], want[:, :3])                       # population, simulation, step: every population
    np.testing.assert_array_equal(rows[:, 25:], want[:, 25:])                     # collided, ever collided
    np.testing.assert_array_equal(np.stack(result["elite_indices"]), z["elite_indices"])
    assert result["stopped_early"] is None and counters == {"frames": 0, "simulations": 3 * 6, "steps": rows.shape[0]}
    assert rows.shape[0] < 3 * 6 * 4 and 0 < rows[:, 26].sum()                    # a collision cut a simulation short
    p0 = want[:, 0] == 0
    got, ref = rows[p0], want[p0]
    np.testing.assert_allclose(got[:, 3:15], ref[:, 3:15], rtol=0, atol=2e-7)     # noise
    np.testing.assert_allclose(got[:, 18:21], ref[:, 18:21], rtol=0, atol=1e-6)   # position
    np.testing.assert_allclose(got[:, 21:25], ref[:, 21:25], rtol=1e-6, atol=1e-4)  # step / cumulative log p, log q
    np.testing.assert_allclose(got[:, 15:18], ref[:, 15:18], rtol=1e-5, atol=1e-5)  # reward applied, sigma, adjusted value
    assert (got[got[:, 2] == 0][:, 15] == 0).all()                                # no reward before the first step
    np.testing.assert_array_equal(got[:, 21:23][:, 0], got[:, 21:23][:, 1])       # q == p in population 0
    # the two series the reference plots
    risks = z["risks"]
    np.testing.assert_allclose(result["population_scores"], risks.mean(1), rtol=1e-5)
    np.testing.assert_allclose(result["elite_scores"], [risks[k][z["elite_indices"][k]].mean() for k in range(3)], rtol=1e-5)


def test_refits_and_later_populations_within_the_reference_s_own_error(cem_run):
    """The refit formulas in float64 on the fixture's elites are the yardstick.  Both the port's `refit` on the reference's own elites
    and q, and the q that run_cem itself reached after every population (result["population_means"] / ["population_covs"]), may be
    at most 4 x as far from float64 as the reference itself, whose distance is floored at float32 epsilon x the largest elite
    magnitude (4: another summation order over m_elite terms).
    Measured, populations 0 / 1 / 2: means -- reference 1.6e-9 / 3.3e-8 / 4.5e-8 from float64 (floor 6.1e-9 / 9.3e-9 / 1.1e-8), the port
    and the run 1.6e-9 / 3.3e-8 / 4.5e-8; variances -- reference 8.9e-11 / 1.2e-8 / 2.2e-7 (the weighted covariance divides by
    1 - sum(w^2), which uneven weights bring close to 0), the port and the run the same: the host refit gives the reference's numbers.
    Rows of populations 1 and 2: the log-probability columns 21-24 keep population 0's bound.  The other columns get population 0's
    bound plus the reference's OWN refit error carried through the draw, element by element: noise[d] = mean[d] + sd[d] * eps[d] with
    the row's eps, so 4 x (|mean - f64|[d] + |var - f64|[d] / (2 sd[d]) * |eps[d]|) (no floor), at most 1.7e-8 / 7.4e-7 here; the state adds these
    up over the steps so far with the dynamics' gains over T = 2 s (position: 1 from a position noise, T velocity, g T^2 / 2 angle,
    g T^3 / 6 rate; angle: 1 and T), at most 1.2e-6 / 3.9e-5 for the position; sigma = a + b |x| + c |angle_y|, the reward is 1-Lipschitz in log p - 36 sigma, the
    value in the position (times sqrt 3), the adjustment multiplies by (1 - 0.01 reward): at most 3.6e-6 / 1.2e-4 for the adjusted value.
    Measured differences there: noise 1.8e-9 / 2.5e-9, position 4.5e-8 / 4.1e-8, adjusted value 2.4e-8 / 2.0e-8, columns 21-24 0."""
    CE, RO, z, rows, result, counters = cem_run
    steps, kmax, m = int(z["steps"]), int(z["kmax"]), int(z["m"])
    p, mean_p, var_p = _target(CE, RO, steps)
    sa, sb, sc_ = [float(v) for v in z["sigma_coeffs"]]
    T, g = RO.ENV["T_final"], RO.ENV["g"]
    gain_pos = np.repeat([1.0, T, g * T ** 2 / 2, g * T ** 3 / 6], 3)          # noise dimension -> position, over the whole flight
    gain_rot = np.repeat([0.0, 0.0, 1.0, T], 3)                                # noise dimension -> rotation vector
    q_ref = p
    for k in range(kmax):
        elites = z["noises"][k][z["elite_indices"][k]]                            # [m_elite, steps, 12] float32
        mean_q = [mean_p] * steps if k == 0 else z["means"][k - 1]
        var_q = [var_p] * steps if k == 0 else z["cov_diags"][k - 1]
        f64 = [refit_f64(elites[:, i], mean_p, var_p, mean_q[i], var_q[i]) for i in range(steps)]
        m64, v64 = np.stack([f[0] for f in f64]), np.stack([f[1] for f in f64])
        assert not any(f[2] or f[3] for f in f64)
        means, covs, info = CE.refit(torch.from_numpy(elites), p, q_ref)
        assert not info["weights_clamped"].any() and not info["cov_clamped"].any()
        floor = EPS32 * float(np.abs(elites).max())
        err_m, err_v = np.abs(z["means"][k] - m64), np.abs(z["cov_diags"][k] - v64)          # the reference's own distance, per element
        d_ref_m, d_ref_v = max(float(err_m.max()), floor), max(float(err_v.max()), floor)
        for name, ms, cs in (("port's refit", means, covs), ("run's q", result["population_means"][k], result["population_covs"][k])):
            got_m, got_v = torch.stack(ms).numpy().astype(np.float64), torch.stack([c.diag() for c in cs]).numpy().astype(np.float64)
            for c in cs:
                assert torch.equal(c, torch.diag(c.diag()))                       # diagonal only
            d_m, d_v = float(np.abs(got_m - m64).max()), float(np.abs(got_v - v64).max())
            print(f"population {k}, {name}: mean distance from float64 {d_m:.2e} (reference {err_m.max():.2e}, floor {floor:.2e}); "
                  f"variance {d_v:.2e} (reference {err_v.max():.2e})")
            assert d_m <= 4 * d_ref_m and d_v <= 4 * d_ref_v, (name, k)
        if k + 1 < kmax:
            # ---- rows of the run's own population k + 1, drawn from its own q after population k
            sel = z["rows"][:, 0] == k + 1
            got, ref = rows[sel], z["rows"][sel]
            np.testing.assert_allclose(got[:, 21:25], ref[:, 21:25], rtol=1e-6, atol=1e-4)   # log p, log q, their sums: population 0's bound
            step = ref[:, 2].astype(int)
            sd = np.sqrt(z["cov_diags"][k].astype(np.float64))
            eps = (ref[:, 3:15] - z["means"][k][step]) / sd[step]
            c_noise = 4 * (err_m[step] + err_v[step] / (2 * sd[step]) * np.abs(eps))          # [rows, 12], the carried part
            c_pos, c_rot = np.zeros(len(ref)), np.zeros(len(ref))
            for i in range(len(ref)):                                              # summed over the simulation's steps so far
                mine = (ref[:, 1] == ref[i, 1]) & (ref[:, 2] <= ref[i, 2])
                c_pos[i], c_rot[i] = (c_noise[mine] * gain_pos).sum(), (c_noise[mine] * gain_rot).sum()
            c_sigma = sb * c_pos + sc_ * c_rot
            c_reward = (np.abs(ref[:, 3:15]) / var_p * c_noise).sum(1) + 36 * c_sigma          # of the reward computed FROM the row
            c_applied = np.array([c_reward[(ref[:, 1] == r[1]) & (ref[:, 2] == r[2] - 1)].sum() for r in ref])   # the previous row's
            raw = np.abs(ref[:, 17]) / 0.64                                                    # reward in [-72, 36]: 0.64 <= 1 - 0.01 reward <= 1.72
            c_adj = 1.72 * np.sqrt(3) * c_pos + 0.01 * raw * c_reward
            print(f"population {k + 1} rows: noise {np.abs(got[:, 3:15] - ref[:, 3:15]).max():.2e} (carried <= {c_noise.max():.2e}), position "
                  f"{np.abs(got[:, 18:21] - ref[:, 18:21]).max():.2e} (carried <= {c_pos.max():.2e}), adjusted value "
                  f"{np.abs(got[:, 17] - ref[:, 17]).max():.2e} (carried <= {c_adj.max():.2e}), columns 21-24 {np.abs(got[:, 21:25] - ref[:, 21:25]).max():.2e}")
            assert (np.abs(got[:, 3:15] - ref[:, 3:15]) <= 2e-7 + c_noise).all()
            assert (np.abs(got[:, 18:21] - ref[:, 18:21]) <= 1e-6 + c_pos[:, None]).all()
            for col, carried in ((15, c_applied), (16, c_sigma), (17, c_adj)):
                assert (np.abs(got[:, col] - ref[:, col]) <= 1e-5 + 1e-5 * np.abs(ref[:, col]) + carried).all(), col
        q_ref = CE.SeedableMultivariateNormal(list(torch.from_numpy(z["means"][k])), [torch.diag(d) for d in torch.from_numpy(z["cov_diags"][k])], 0)
    assert all(torch.equal(a, b) for a, b in zip(result["means"] + result["covs"], result["population_means"][-1] + result["population_covs"][-1]))
    # the estimate the p / q columns exist for, on the run's rows and on the reference's
    mine, want = CE.failure_probability(rows), CE.failure_probability(z["rows"])
    assert mine["populations"] == want["populations"] and mine["collisions"] == want["collisions"]
    assert mine["mean_steps_to_collision"][:2] == want["mean_steps_to_collision"][:2]
    # (each cumulative sum within 1e-6 x ~150 + 1e-4, their difference within 5e-4, so exp of it within 1e-3 relative)
    np.testing.assert_allclose(mine["per_population"], want["per_population"], rtol=1e-3, atol=0)
    np.testing.assert_allclose(mine["pooled"], want["pooled"], rtol=1e-3, atol=0)
    assert want["pooled"] > 0


def test_best_solution_is_one_more_simulation_seeded_after_the_population(cem_run):
    """run_cem(best_solution=True): simulation number m (seeded seed + m) drawn from the final q, replayed here through the dynamics and
    the stub's sphere: the step with the lowest RAW value, its mean and covariance, and that raw value (not the adjusted one)"""
    CE, RO, z, rows, result, _ = cem_run
    steps, m = int(z["steps"]), int(z["m"])
    q = result["q"]
    assert q.noise_seed == int(z["generator_seed"])
    noises = q.sample(m)
    state, raw = RO.initial_state(steps), []
    for k in range(steps):
        state = RO.drone_dynamics(state, torch.tensor([RO.ENV["mass"] * RO.ENV["g"], 0.0, 0.0, 0.0]), RO.ENV["T_final"] / steps) + noises[k]
        raw.append(float(np.linalg.norm(state[:3].numpy().astype(np.float64) - z["centre"]) - float(z["radius"])))
        if raw[-1] < 0:
            break
    best = int(np.argmin(raw))
    mean, cov, value = result["best_solution"]
    assert value == raw[best] and torch.equal(mean, q.means[best]) and torch.equal(cov, q.covs[best])
    assert len(set(raw)) == len(raw) and not torch.equal(q.means[best], q.means[(best + 1) % steps])   # the choice is a choice


def _elites(seed, n, steps):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, steps, 12, generator=g) * 0.02


def _check_refit(CE, elites, p, q, mean_p, var_p, mean_q, var_q):
    means, covs, info = CE.refit(elites, p, q)
    for i in range(elites.shape[1]):
        m64, v64, wc, vc = refit_f64(elites[:, i].numpy(), mean_p, var_p, mean_q[i], var_q[i])
        np.testing.assert_allclose(means[i].numpy(), m64, rtol=2e-5, atol=1e-8)
        np.testing.assert_allclose(covs[i].diag().numpy(), v64, rtol=2e-4, atol=1e-10)
        assert bool(info["weights_clamped"][i]) == wc and bool(info["cov_clamped"][i]) == vc
    return means, covs, info


def test_refit_clamps_a_variance_above_the_limit():
    CE, RO, _, _ = _sim_class()
    p, mean_p, var_p = _target(CE, RO, 2)
    x = _elites(1, 4, 2)
    x[:, 1, 5] = torch.tensor([-1.0, 1.0, -1.0, 1.0])          # variance 4/3 > 0.1 at step 1, dimension 5
    means, covs, info = _check_refit(CE, x, p, p, mean_p, var_p, [mean_p] * 2, [var_p] * 2)
    assert list(info["cov_clamped"]) == [False, True] and not info["weights_clamped"].any()
    assert float(covs[1][5, 5]) == np.float32(0.1) and float(covs[0].diag().max()) < 0.1


def test_refit_clamps_weights_that_underflow():
    CE, RO, _, _ = _sim_class()
    p, mean_p, var_p = _target(CE, RO, 1)
    mean_q = mean_p.copy()
    mean_q[0] = 0.2                                            # log p - log q = (0.04 - 0.4 x0) / 0.0008: 50 at x0 = 0, -100 at 0.3
    q = CE.SeedableMultivariateNormal([torch.from_numpy(mean_q).float()], [torch.diag(torch.from_numpy(var_p).float())], 0)
    x = _elites(2, 3, 1)
    x[:, 0, 0] = torch.tensor([0.0, 0.001, 0.3])
    means, covs, info = _check_refit(CE, x, p, q, mean_p, var_p, [mean_q], [var_p])
    assert info["weights_clamped"][0] and not info["cov_clamped"][0]
    # the clamped sample carries exactly 1e-8: mean = w01 @ x01 + 1e-8 * x2
    lw = torch.tensor([(0.04 - 0.4 * 0.0) / 0.0008, (0.04 - 0.4 * 0.001) / 0.0008], dtype=torch.float64)
    w01 = torch.softmax(lw, 0).numpy()
    np.testing.assert_allclose(float(means[0][0]), w01[1] * 0.001 + 1e-8 * 0.3, rtol=1e-4)


def test_zero_variance_stops_run_cem_with_the_previous_q():
    CE, RO, Sim, z = _sim_class()
    p, mean_p, var_p = _target(CE, RO, 2)
    x = _elites(3, 3, 2)
    x[:, 0, 3] = 0.0
    _, covs, info = CE.refit(x, p, p)
    assert float(covs[0][3, 3]) == 0.0 and not info["cov_clamped"].any()     # 0 is inside [0, 0.1]: no clamp, but no distribution either
    with pytest.raises(ValueError):
        CE.SeedableMultivariateNormal([torch.zeros(12)] * 2, covs, 0)

    class ZeroColumn(CE.SeedableMultivariateNormal):
        def sample(self, sim):
            out = super().sample(sim)
            out[1][3] = 0.0
            return out

    q0 = ZeroColumn([p.means[0]] * 3, [p.covs[0]] * 3, 7)
    with _patched(CE, RO, Sim):
        rows, result, _ = CE.run_cem(_FakeModel(), None, 8, 8, 3, m=4, m_elite=2, kmax=3, seed=7, q=q0, sdf=object(), in_flight=1, autocast=False)
    assert result["stopped_early"] == 0 and result["q"] is q0
    assert set(rows[:, 0]) == {0.0} and len(result["elite_indices"]) == 1 and len(result["refit_info"]) == 1
    assert all(torch.equal(a, b) for a, b in zip(result["means"], q0.means))


def test_resume_from_a_passed_in_proposal(cem_run):
    """q and start_k: the reference's --k resume -- populations 1.. of a run restarted from q_1 are those of the whole run"""
    CE, RO, z, rows, result, _ = cem_run
    _, _, Sim, _ = _sim_class()
    steps, m, m_elite, kmax, seed = [int(z[k]) for k in ("steps", "m", "m_elite", "kmax", "generator_seed")]
    with _patched(CE, RO, Sim):
        _, first, _ = CE.run_cem(_FakeModel(), None, 8, 8, steps, m=m, m_elite=m_elite, kmax=1, seed=seed, sdf=object(), in_flight=1, autocast=False)
        rows2, second, _ = CE.run_cem(_FakeModel(), None, 8, 8, steps, m=m, m_elite=m_elite, kmax=kmax, seed=seed, q=first["q"], start_k=1,
                                      sdf=object(), in_flight=1, autocast=False)
    np.testing.assert_array_equal(rows2, rows[rows[:, 0] >= 1])
    assert all(torch.equal(a, b) for a, b in zip(second["means"] + second["covs"], result["means"] + result["covs"]))


def test_sample_is_the_reference_s_draw_and_leaves_the_global_generator_alone():
    CE, RO, _, _ = _sim_class()
    g = torch.Generator().manual_seed(4)
    steps, seed = 5, 1234
    means = [torch.randn(12, generator=g) * 0.01 for _ in range(steps)]
    covs = [torch.diag(torch.rand(12, generator=g) * 1e-3 + 1e-5) for _ in range(steps)]
    q = CE.SeedableMultivariateNormal(means, covs, seed)
    with torch.random.fork_rng():                              # SeedableMultivariateNormal.py:19-22 as written
        want = []
        for sim in range(6):
            torch.manual_seed(seed + sim)
            want.append(torch.stack([d.sample() for d in q.distributions]))
    before = torch.get_rng_state()
    serial = [torch.stack(q.sample(sim)) for sim in range(6)]
    assert all(torch.equal(a, b) for a, b in zip(serial, want))
    got = {}

    def work(tid):
        got[tid] = [[torch.stack(q.sample(sim)) for sim in range(6)] for _ in range(20)]

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert all(torch.equal(a, b) for t in range(2) for rep in got[t] for a, b in zip(rep, want))
    assert torch.equal(torch.get_rng_state(), before)
    lp = q.log_prob(2, want[0][2])
    assert lp.dtype == torch.float32 and torch.equal(lp, q.distributions[2].log_prob(want[0][2]))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, m, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        CE, RO, Sim, z = _sim_class()

        class CpuSim(Sim):
            def observe(self, pose):
                return 0.05 + 0.2 * abs(float(pose[0, 3]))

        CE.CEMSimulator, keep = CpuSim, CE.CEMSimulator
        try:
            rows, result, counters = CE.run_cem(_FakeModel(), None, 8, 8, int(z["steps"]), m=m, m_elite=2, kmax=2, seed=int(z["generator_seed"]),
                                                sdf=object(), rank=rank, world_size=world, in_flight=1, autocast=False)
        finally:
            CE.CEMSimulator = keep
        ret[rank] = (rows, torch.stack(result["means"]).numpy(), torch.stack(result["covs"]).numpy(), counters)
    finally:
        dist.destroy_process_group()


def test_cem_shards_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    m, world = 7, 2                                        # 4 + 3 simulations; the fixture's sphere stops simulation 5
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), m, ret), nprocs=world, join=True)
    ret1 = mgr.dict()
    mp.spawn(_worker, args=(1, _free_port(), m, ret1), nprocs=1, join=True)
    rows, means, covs, c = ret1[0]
    for r in range(world):
        np.testing.assert_array_equal(ret[r][0], rows)
        np.testing.assert_array_equal(ret[r][1], means)
        np.testing.assert_array_equal(ret[r][2], covs)
    assert ret[0][3]["simulations"] + ret[1][3]["simulations"] == c["simulations"] == 2 * m
    assert ret[0][3]["steps"] + ret[1][3]["steps"] == c["steps"] == rows.shape[0]
    assert rows[:, 26].any() and not rows[:, 26].all()                            # ragged: some simulation collided
    assert [tuple(r) for r in rows[:, :3]] == sorted(tuple(r) for r in rows[:, :3])   # (population, simulation, step) order


def test_failure_probability_on_a_hand_written_table():
    from nerfsafetyvalidation_amd import cem as CE
    rows = np.zeros((7, CE.CEM_ROW_WIDTH))
    #            sim step cum p  cum q  collided ever
    table = [(0, 0, -0.5, -1.0, 0, 1), (0, 1, -1.0, -2.0, 1, 1),                   # collided at step 1: exp(-1 + 2) = e
             (1, 0, -4.0, -3.0, 0, 0),                                            # never collided: 0
             (2, 0, -1.0, -1.0, 0, 1), (2, 1, -2.0, -2.0, 0, 1), (2, 2, -3.0, -2.5, 1, 1)]   # step 2: exp(-0.5)
    for r, (sim, step, cp, cq, hit, ever) in zip(rows, table):
        r[1], r[2], r[23], r[24], r[25], r[26] = sim, step, cp, cq, hit, ever
    rows[6, 0], rows[6, 1], rows[6, 23], rows[6, 24], rows[6, 25], rows[6, 26] = 1, 0, -2.0, -4.0, 1, 1    # population 1: one simulation, e^2
    out = CE.failure_probability(rows)
    assert out["populations"] == [0, 1] and out["collisions"] == [2, 1]
    np.testing.assert_allclose(out["per_population"], [(np.e + 0 + np.exp(-0.5)) / 3, np.exp(2.0)], rtol=1e-15)
    np.testing.assert_allclose(out["pooled"], (np.e + 0 + np.exp(-0.5) + np.exp(2.0)) / 4, rtol=1e-15)
    assert out["mean_steps_to_collision"] == [1.5, 0.0]
    none = CE.failure_probability(rows[2:3])
    assert none["per_population"] == [0.0] and none["collisions"] == [0] and np.isnan(none["mean_steps_to_collision"][0])


def test_run_validation_dispatches_both_stress_tests(monkeypatch):
    import nerfsafetyvalidation_amd as pkg
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import rollout as RO
    calls = []
    monkeypatch.setattr(RO, "run_rollout", lambda *a, **k: calls.append(("mc", a, k)) or "mc")
    monkeypatch.setattr(CE, "run_cem", lambda *a, **k: calls.append(("cem", a, k)) or "cem")
    assert RO.run_validation("Monte Carlo", 1, 2, n=3) == "mc" and RO.run_validation("Cross Entropy Method", 4, m=5) == "cem"
    assert calls == [("mc", (1, 2), {"n": 3}), ("cem", (4,), {"m": 5})]
    with pytest.raises(ValueError, match="Unrecognized stress test"):
        RO.run_validation("Importance Sampling")
    assert (RO.STRESS_MONTE_CARLO, RO.STRESS_CEM) == ("Monte Carlo", "Cross Entropy Method")
    assert pkg.cem is CE and pkg.rollout is RO


def test_run_cem_needs_a_signed_distance_field():
    from nerfsafetyvalidation_amd import cem as CE
    with pytest.raises(ValueError, match="sdf is required"):
        CE.run_cem(_FakeModel(), None, 8, 8, 3, sdf=None)
    with pytest.raises(ValueError, match="sdf is required"):
        CE.run_cem(_FakeModel(), None, 8, 8, 3)
