"""The Cross Entropy Method stress test (nerfsafetyvalidation_amd/cem.py) on the GPU: populations of 32 x 32 frames through the fp32
network's `run` (no autocast) with the Gaussian-approximation UQ and the signed distance field built by the GPU distance transform.
The render and UQ path itself is held against the oracle by test_rollout_gpu.py; here every CEM row is tied to that path (its sigma is
the plain RolloutSimulator.observe of the row's own state, bit for bit) and to the refit (its noise is the draw from the q rebuilt
from the previous population's rows), and the rows must not depend on how many simulations are in flight."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 32
STEPS, M, M_ELITE, KMAX, SEED = 3, 4, 2, 2, 11
KW = dict(num_steps=32, upsample_steps=0, max_ray_batch=1024)


@pytest.fixture(scope="module")
def sdf(device):
    from nerfsafetyvalidation_amd import collision as CO
    return CO.SignedDistanceField.from_occupancy(CO.occupancy_from_fn(CO.henge_fn, CO.reference_box()), CO.reference_box())


@pytest.fixture(scope="module")
def runs(device, sdf):
    """the same CEM run with 1 and with 3 simulations in flight (shared, not modified)"""
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    out = [CE.run_cem(model, sc.intrinsics, H, W, STEPS, m=M, m_elite=M_ELITE, kmax=KMAX, seed=SEED, sdf=sdf, in_flight=n, render_kwargs=KW,
                      autocast=False) for n in (1, 3)]
    return sc, model, out


def test_rows_and_proposal_do_not_depend_on_in_flight(runs):
    from nerfsafetyvalidation_amd import cem as CE
    _, _, ((rows1, res1, c1), (rows3, res3, c3)) = runs
    assert rows1.shape[1] == CE.CEM_ROW_WIDTH and 0 < rows1.shape[0] <= KMAX * M * STEPS
    np.testing.assert_array_equal(rows1, rows3)
    for a, b in zip(res1["means"] + res1["covs"], res3["means"] + res3["covs"]):
        assert torch.equal(a, b)
    assert [list(e) for e in res1["elite_indices"]] == [list(e) for e in res3["elite_indices"]]
    for c in (c1, c3):
        assert c == {"frames": 2 * rows1.shape[0], "simulations": KMAX * M, "steps": rows1.shape[0]}
    assert set(rows1[:, 0]) == set(range(KMAX)) and np.isfinite(rows1).all()
    assert len(set(rows1[:, 17])) > M                                              # the field gives CEM distances to rank, not 0 / 9999


def test_every_row_s_noise_is_the_refitted_draw_and_its_sigma_the_plain_observe(runs, sdf):
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import rollout as RO
    sc, model, ((rows, res, _), _) = runs
    p = CE.target_distribution(STEPS, SEED)
    plain = RO.RolloutSimulator(model, sc.intrinsics, H, W, STEPS, seed=SEED, render_kwargs=KW, sdf=sdf)
    hover = torch.tensor([RO.ENV["mass"] * RO.ENV["g"], 0.0, 0.0, 0.0])
    q = p
    for k in range(KMAX):
        pop = rows[rows[:, 0] == k]
        for sim in range(M):
            mine = pop[pop[:, 1] == sim]
            want = torch.stack(q.sample(sim)).numpy()
            assert 1 <= mine.shape[0] <= STEPS and list(mine[:, 2]) == list(range(mine.shape[0]))
            np.testing.assert_array_equal(mine[:, 3:15], want[:mine.shape[0]].astype(np.float64))
            state, cum_p, cum_q, reward = RO.initial_state(STEPS), np.float32(0), np.float32(0), 0.0
            for r in mine:
                noise = torch.from_numpy(r[3:15].astype(np.float32))
                state = RO.drone_dynamics(state, hover, RO.ENV["T_final"] / STEPS) + noise
                with torch.autocast("cuda", enabled=False):
                    sigma = plain.observe(RO.camera_pose(state))
                assert r[16] == sigma, (k, sim, r[2], r[16], sigma)
                lp, lq = float(p.log_prob(int(r[2]), noise)), float(q.log_prob(int(r[2]), noise))
                cum_p, cum_q = np.float32(cum_p + np.float32(lp)), np.float32(cum_q + np.float32(lq))     # float32 running sums
                assert r[15] == reward and list(r[21:25]) == [lp, lq, float(cum_p), float(cum_q)]
                reward = RO.reward_fn(lp, sigma)
                collided, value = sdf.lookup(r[18:21])                             # the simulator's own flag, on the raw value
                assert r[25] == float(collided)
                if not collided:                                                   # the last interpolated point is the state itself
                    np.testing.assert_array_equal(r[18:21], state[:3].numpy().astype(np.float64))
                if value is not None:
                    assert r[17] == value - reward * (0.01 * value)
            assert mine[:-1, 25].sum() == 0 and (mine[:, 26] == mine[-1, 25]).all()                # the first collision ends the simulation
        # q_{k+1} from population k's rows through refit
        risks = CE.simulation_risks(rows, k, M)
        elite = CE.select_elite(risks, M_ELITE)
        assert list(elite) == list(res["elite_indices"][k])
        means, covs, _ = CE.refit(torch.stack([torch.stack(q.sample(int(s))) for s in elite]), p, q)
        q = CE.SeedableMultivariateNormal(means, covs, SEED)
    assert all(torch.equal(a, b) for a, b in zip(q.means + q.covs, res["means"] + res["covs"]))


def test_cem_run_cuda_path_and_dedupe(device, sdf):
    """the occupancy-grid renderer (--cuda_ray) under autocast: renders_per_step = 1 gives the same rows with half the frames"""
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=48, W=48, bound=2)
    model = sc.build_model(device, cuda_ray=True)
    rows2, res2, c2 = CE.run_cem(model, sc.intrinsics, 48, 48, 2, m=3, m_elite=2, kmax=2, seed=3, sdf=sdf, in_flight=1)
    rows1, res1, c1 = CE.run_cem(model, sc.intrinsics, 48, 48, 2, m=3, m_elite=2, kmax=2, seed=3, sdf=sdf, in_flight=3, renders_per_step=1)
    assert c2["frames"] == 2 * c1["frames"] == 2 * rows1.shape[0]
    np.testing.assert_array_equal(rows1, rows2)
    assert np.isfinite(rows1[:, 16]).all() and np.isfinite(rows1[:, 17]).all()
    assert all(torch.equal(a, b) for a, b in zip(res1["means"] + res1["covs"], res2["means"] + res2["covs"]))


def test_cem_with_the_laplace_method(device, sdf):
    """uq_method = 'Bayesian Laplace Approximation' at 16 x 16: the uncertainty column holds the root mean variance, the reward (the next
    row's column 15, and what adjusts this row's value) is reward_fn_laplace of torch's float32 log p, the rmv and the trace"""
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=16, W=16, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    seen = {}

    class Spy(CE.CEMSimulator):
        def uncertainty_laplace(self, out, rays):
            got = super().uncertainty_laplace(out, rays)
            self._uq.append(got)
            return got

        def run(self, sim):
            self._uq = []
            rows = super().run(sim)
            seen[sim] = (self._uq, list(self.raw_values))
            return rows

    CE.CEMSimulator, keep = Spy, CE.CEMSimulator
    try:
        rows, res, c = CE.run_cem(model, sc.intrinsics, 16, 16, 2, m=2, m_elite=2, kmax=1, seed=2, sdf=sdf, in_flight=1, autocast=False,
                                  render_kwargs=dict(num_steps=32, upsample_steps=0), uq_method=RO.UQ_LAPLACE,
                                  uq_kwargs=dict(n_steps=20, lm_solver="closed_form"))
    finally:
        CE.CEMSimulator = keep
    assert c["frames"] == 2 * rows.shape[0] and len(seen) == 2
    for sim in range(2):
        mine = rows[rows[:, 1] == sim]
        uq, raw = seen[sim]
        assert len(uq) == len(raw) == mine.shape[0] >= 1
        reward = 0.0
        for r, (trace, rmv), value in zip(mine, uq, raw):
            assert np.isfinite(trace) and np.isfinite(rmv) and rmv > 0
            assert r[16] == rmv and r[15] == reward
            reward = RO.reward_fn_laplace(r[21], rmv, trace)
            assert reward == float(np.clip(r[21] - 36 * rmv * trace * 3, -72, 36))
            assert r[17] == value - reward * (0.01 * value)
