"""The trajectory planner (nerfsafetyvalidation_amd.nav) against tests/golden/planner.npz, which the reference's own
nav/quad_plot.py and nav/quad_helpers.py wrote (tests/golden/make_golden_planner.py).  CPU tensors only: A*, the differential
flatness of calc_everything, body_to_world and update_state need no network."""
import os

import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import nav

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(G, "planner.npz"), allow_pickle=False)


def _cfg(f, density_fn=None):
    start, end = torch.from_numpy(f["start_state"]), torch.from_numpy(f["end_state"])
    cfg = {"T_final": 2.0, "steps": 12, "lr": 0.001, "epochs_init": int(f["epochs_init"]), "fade_out_epoch": 0, "fade_out_sharpness": 10,
           "epochs_update": int(f["epochs_update"]), "start_state": start, "end_state": end, "I": torch.eye(3), "g": 10.0, "mass": 1.0,
           "body": f["body"], "nbins": [int(v) for v in f["nbins"]]}
    return nav.Planner(start, end, cfg, density_fn)


def test_astar_matches_the_reference_paths(fx):
    for i in range(4):
        occ, start, goal = fx[f"astar{i}_occ"], tuple(int(v) for v in fx[f"astar{i}_start"]), tuple(int(v) for v in fx[f"astar{i}_goal"])
        want = fx[f"astar{i}_path"]
        if want.shape[0] == 0:
            with pytest.raises(ValueError):
                nav.astar(torch.from_numpy(occ), start, goal)
            continue
        assert np.array_equal(np.asarray(nav.astar(torch.from_numpy(occ), start, goal)), want)
        assert np.array_equal(np.asarray(nav.astar(occ, start, goal)), want)          # a numpy grid gives the same path
    # the planner's own 20^3 grid
    path = nav.astar(torch.from_numpy(fx["occupied"]), tuple(int(v) for v in fx["astar_start"]), tuple(int(v) for v in fx["astar_goal"]))
    assert np.array_equal(np.asarray(path), fx["path"])


def test_astar_raises_where_the_reference_raises(fx):
    occ = fx["astar0_occ"].copy()
    occ[0, 0, 0] = True
    with pytest.raises(AssertionError):
        nav.astar(occ, (0, 0, 0), (7, 7, 7))
    occ = fx["astar0_occ"].copy()
    occ[7, 7, 7] = True
    with pytest.raises(AssertionError):
        nav.astar(occ, (0, 0, 0), (7, 7, 7))


def test_smoothing_draw_comes_from_the_given_generator(fx):
    g = torch.Generator().manual_seed(int(fx["smooth_seed"]))
    draw = torch.normal(mean=0, std=0.001 * torch.ones(fx["smoothing_draw"].shape), generator=g)
    assert np.array_equal(draw.numpy(), fx["smoothing_draw"])


def test_calc_everything_and_body_to_world_match_the_reference(fx):
    p = _cfg(fx)
    p.states = torch.from_numpy(fx["states_astar"]).clone().requires_grad_(True)
    names = ["pos", "vel", "accel", "rot_matrix", "omega", "angular_accel", "actions"]
    for n, v in zip(names, p.calc_everything()):
        want = fx[f"ce_{n}"]
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(v.detach().numpy() - want).max())
        assert err <= 1e-6 * scale, f"{n}: max |d| = {err:.3e} (scale {scale:.3g})"
    world = p.body_to_world(p.robot_body).detach().numpy()
    assert np.abs(world - fx["body_world"]).max() <= 1e-6
    assert np.array_equal(p.get_next_action().detach().numpy(), fx["ce_actions"][0])


def test_update_state_matches_the_reference(fx):
    p = _cfg(fx)
    p.states = torch.from_numpy(fx["states_init"]).clone().requires_grad_(True)
    p.initial_accel = torch.from_numpy(fx["accel_init"]).clone().requires_grad_(True)
    measured = torch.from_numpy(fx["measured_state"])
    p.update_state(measured)
    assert p.start_state is measured
    assert np.array_equal(p.states.detach().numpy(), fx["states_upd0"])
    assert np.abs(p.initial_accel.detach().numpy() - fx["accel_upd0"]).max() <= 1e-6 * np.abs(fx["accel_upd0"]).max()
    assert p.states.requires_grad and p.initial_accel.requires_grad and p.states.grad_fn is None


class _OperatorsOnly(torch.nn.Module):
    """a CPU model without a fused form: density() is a torch function of the points"""

    def __init__(self):
        super().__init__()
        self.fused = True

    def density(self, x):
        return {"sigma": torch.exp(-(x ** 2).sum(-1)), "geo_feat": x}

    def fused_model(self):
        return None


def test_density_query_without_a_fused_model_is_the_torch_composition(fx):
    model = _OperatorsOnly()
    rot = torch.from_numpy(fx["rot"])
    q = nav.density_query(model, rot)
    x = torch.rand(3, 7, 3)
    assert torch.equal(q(x), model.density(x.reshape((-1, 3)) @ rot)["sigma"].reshape(x.shape[:-1]))
    p = _cfg(fx, q)
    pos, _, _, rot_matrix = p.calc_everything()[:4]
    assert q.collision(rot_matrix, pos, p.robot_body) is None
    # the planner's cost through the query equals its cost through the plain reference lambda
    lam = lambda x: model.density(x.reshape((-1, 3)) @ rot)["sigma"].reshape(x.shape[:-1])   # noqa: E731
    p2 = _cfg(fx, lam)
    c1, c2 = p.total_cost(), p2.total_cost()
    assert torch.equal(c1, c2)
    c1.backward()
    c2.backward()
    assert torch.equal(p.states.grad, p2.states.grad) and torch.equal(p.initial_accel.grad, p2.initial_accel.grad)
