#!/usr/bin/env python3
"""Generates tests/golden/planner.npz by running the REFERENCE's own trajectory planner (nav/quad_plot.py, nav/quad_helpers.py) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_planner.py

The density_fn is validate.py:283-288's closure `model.density(x.reshape((-1, 3)) @ rot)['sigma']` over the reference's
NeRFNetwork on the CPU oracle (make_golden.py's shims), built like make_golden.gen_density_grad's fp32 network (weight seed 5,
table seed 3, full fp32 table draws) with one change: row 0 of the sigma net's output layer is replaced by -18 * |row 0|, so that
sigma = exp(h0) <= 1 and a third of the 20^3 A* cells are occupied (the unchanged network has sigma ~ 1 everywhere: every cell would
be occupied and A* would refuse the start).  Two things differ from validate.py and are patched IN MEMORY only:
  * torch.optim.Adam(..., capturable=True) needs a GPU; the fixture's Adam runs with capturable=False (the same update, with the
    bias corrections in float64 on the host instead of fp32 on the device: differences at the last bits of a step);
  * the per-epoch prints and the JSON dumps are not triggered (no `basefolder`; stdout discarded while the planner runs).
The smoothing noise of a_star_init is drawn from torch's global generator seeded with SMOOTH_SEED right before the call (the
only random draw in it), so a caller passing torch.Generator().manual_seed(SMOOTH_SEED) reproduces it.
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (shims, sys.path of the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nav.quad_helpers as QH  # noqa: E402
import nav.quad_plot as QP  # noqa: E402
from nav.math_utils import vec_to_rot_matrix  # noqa: E402

SMOOTH_SEED = 11
OCC_SCALE = 18.0
EPOCHS_INIT, EPOCHS_UPDATE = 20, 10


class _AdamCPU(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, capturable=False, **kw):
        super().__init__(params, lr=lr, capturable=False, **kw)


def planner_network():
    torch.manual_seed(5)
    net = MG.RefNetwork(encoding="hashgrid", bound=2, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1)
    g = torch.Generator().manual_seed(3)
    net.encoder.embeddings.data.copy_(torch.rand(net.encoder.embeddings.shape, generator=g) - 0.5)
    net = net.eval()
    net.requires_grad_(False)
    w = net.sigma_net[-1].weight
    w[0] = -OCC_SCALE * w[0].abs()
    return net


def planner_cfg():
    """validate.py:205-256 with envConfig.json's values (fewer epochs)"""
    start_R = vec_to_rot_matrix(torch.tensor([0.0, 0.0, 0.0]))
    end_R = vec_to_rot_matrix(torch.tensor([0.0, 0.0, 0.0]))
    rates = torch.zeros(3)
    start_state = torch.cat([torch.tensor([-0.75, -0.235, 0.25]), rates, start_R.reshape(-1), rates], dim=0)
    end_state = torch.cat([torch.tensor([0.2, -0.74, 0.3]), rates, end_R.reshape(-1), rates], dim=0)
    cfg = {"T_final": 2.0, "steps": 12, "lr": 0.001, "epochs_init": EPOCHS_INIT, "fade_out_epoch": 0, "fade_out_sharpness": 10,
           "epochs_update": EPOCHS_UPDATE, "start_state": start_state, "end_state": end_state,
           "I": torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1]]).float(), "g": 10.0, "mass": 1.0,
           "body": np.array([[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]), "nbins": [10, 10, 5]}
    return start_state, end_state, cfg


def astar_cases():
    out = {}
    rng = np.random.default_rng(7)
    for i, (shape, frac) in enumerate([((8, 8, 8), 0.25), ((12, 10, 6), 0.3), ((6, 6, 6), 0.2), ((6, 6, 6), 0.0)]):
        occ = rng.random(shape) < frac
        start, goal = (0, 0, 0), tuple(s - 1 for s in shape)
        occ[start] = occ[goal] = False
        if i == 3:                                   # a wall across the grid: no path
            occ[:, 3, :] = True
        try:
            path = np.asarray(QH.astar(torch.from_numpy(occ), start, goal), np.int32)
        except ValueError:
            path = np.zeros((0, 3), np.int32)
        out[f"astar{i}_occ"], out[f"astar{i}_start"], out[f"astar{i}_goal"], out[f"astar{i}_path"] = occ, start, goal, path
    return out


def main():
    torch.optim.Adam = _AdamCPU
    net = planner_network()
    rot = torch.tensor([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]])
    density_fn = lambda x: net.density(x.reshape((-1, 3)) @ rot)["sigma"].reshape(x.shape[:-1])   # noqa: E731  (validate.py:288)
    start_state, end_state, cfg = planner_cfg()
    rec = {}

    # what a_star_init sees: the occupancy grid, and its one random draw
    real_astar, real_normal = QP.astar, torch.normal

    def spy_astar(occupied, start, goal):
        rec["occupied"] = occupied.numpy().copy()
        rec["astar_start"], rec["astar_goal"] = np.asarray(start, np.int32), np.asarray(goal, np.int32)
        path = real_astar(occupied, start, goal)
        rec["path"] = np.asarray(path, np.int32)
        return path

    def spy_normal(*a, **k):
        r = real_normal(*a, **k)
        rec["smoothing_draw"] = r.numpy().copy()
        return r

    traj = QP.Planner(start_state, end_state, cfg, density_fn)
    with contextlib.redirect_stdout(io.StringIO()):
        QP.astar, torch.normal = spy_astar, spy_normal
        torch.manual_seed(SMOOTH_SEED)
        traj.a_star_init()
        QP.astar, torch.normal = real_astar, real_normal
    rec["states_astar"] = traj.states.detach().numpy().copy()
    names = ["pos", "vel", "accel", "rot_matrix", "omega", "angular_accel", "actions"]
    for n, v in zip(names, traj.calc_everything()):
        rec[f"ce_{n}"] = v.detach().numpy().copy()
    rec["body_world"] = traj.body_to_world(traj.robot_body).detach().numpy().copy()
    cost = traj.total_cost()
    cost.backward()
    rec["cost0"] = float(cost)
    rec["grad_states0"], rec["grad_accel0"] = traj.states.grad.numpy().copy(), traj.initial_accel.grad.numpy().copy()
    traj.states.grad = None
    traj.initial_accel.grad = None

    with contextlib.redirect_stdout(io.StringIO()):
        traj.learn_init()
    rec["states_init"], rec["accel_init"] = traj.states.detach().numpy().copy(), traj.initial_accel.detach().numpy().copy()
    rec["actions_init"] = traj.get_actions().detach().numpy().copy()

    # one MPC step: a measured state near the plan's next one, then the replan
    full = traj.get_full_states().detach()
    g = torch.Generator().manual_seed(13)
    measured = full[1] + 0.01 * torch.randn(18, generator=g) * torch.tensor([1.0] * 6 + [0.0] * 9 + [1.0] * 3)
    rec["measured_state"] = measured.numpy().copy()
    traj.update_state(measured)
    rec["states_upd0"], rec["accel_upd0"] = traj.states.detach().numpy().copy(), traj.initial_accel.detach().numpy().copy()
    with contextlib.redirect_stdout(io.StringIO()):
        traj.learn_update(0)
    rec["states_upd"], rec["accel_upd"] = traj.states.detach().numpy().copy(), traj.initial_accel.detach().numpy().copy()
    rec["actions_upd"] = traj.get_actions().detach().numpy().copy()

    rec.update(astar_cases())
    MG.save("planner.npz", bound=2, table_seed=3, occ_scale=OCC_SCALE, smooth_seed=SMOOTH_SEED, epochs_init=EPOCHS_INIT,
            epochs_update=EPOCHS_UPDATE, rot=rot.numpy(), start_state=start_state.numpy(), end_state=end_state.numpy(),
            body=cfg["body"], nbins=np.asarray(cfg["nbins"]), **MG._weights(net), **rec)


if __name__ == "__main__":
    main()
