#!/usr/bin/env python3
"""Generates tests/golden/estimator.npz by running the REFERENCE's own state estimator (nav/estimator_helpers.py Estimator) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_estimator.py

The network is make_golden.gen_run_grad's, its colour net's output layer scaled by COLOR_GAIN so the frames have texture (the reference's NeRFNetwork over the CPU oracle shims of make_golden.py, table seed 0),
rendered as validate.py:290-291's render_fn / get_rays_fn on a 32 x 32 frame (num_steps 32, no upsampling).  Three estimate_state
calls on one Estimator: two with keypoints (the second starts from the first's sig) and one with none (the failure branch).
Patched IN MEMORY only, nothing of the reference is copied or changed:
  * cv2.SIFT_create().detect returns a given keypoint list (recorded as a fixture input: there is no OpenCV here), and cv2.dilate is
    the numpy restatement of its box dilation (nav/sift_numpy.dilate, itself tested against brute force);
  * torch.optim.Adam runs with capturable=False (needs a GPU otherwise; the same update with the bias corrections on the host);
  * Tensor.cuda() returns the tensor (the sensor image stays on the CPU);
  * basefolder is a temporary directory (the per-step JSON the reference writes is discarded); stdout is discarded.
Before the run the shims' encoder backwards are checked to stay opaque to autograd as the CUDA extension's are: the input
gradient of the grid and SH encoders carries no graph, so the fixture's Hessian is the reference's."""
import contextlib
import io
import os
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (shims, sys.path of the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nav.estimator_helpers as EH  # noqa: E402
from nav.agent_helpers import Agent  # noqa: E402
from nav.math_utils import nerf_matrix_to_ngp_torch, rot_x, vec_to_rot_matrix  # noqa: E402
from nerfsafetyvalidation_amd.nav import sift_numpy as S  # noqa: E402
from nerfsafetyvalidation_amd import scene as SC  # noqa: E402

H = W = 32
SEED = 21
DT = 2.0 / 12
N_ITER, BATCH = 10, 64
COLOR_GAIN = 8.0
RENDER = dict(staged=True, bg_color=1.0, perturb=False, num_steps=32, upsample_steps=0)


class _AdamCPU(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, capturable=False, **kw):
        super().__init__(params, lr=lr, capturable=False, **kw)


def check_opaque(net):
    """the oracle shims return input gradients without a graph, as the CUDA extensions do"""
    x = torch.rand(64, 3) - 0.5
    for enc, inp in ((net.encoder, x), (net.encoder_dir, x / x.norm(dim=-1, keepdim=True))):
        inp = inp.clone().requires_grad_(True)
        g, = torch.autograd.grad(enc(inp).float().square().sum(), inp, create_graph=True)
        assert not g.requires_grad, f"{type(enc).__name__}: the input gradient carries a graph"


def start_state():
    """a state whose camera (measurement_fn's pose) is orbit view 33 with its x axis mirrored (the orbit poses are left-handed), so
    that the frame sees the scene; small velocities"""
    from scipy.spatial.transform import Rotation
    from nerfsafetyvalidation_amd import rollout as RO
    P = torch.from_numpy(SC.orbit_poses()[33].copy()).float()
    flip = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    neg = torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    R = RO.rot_x(np.pi / 2).T @ flip.T @ P[:3, :3] @ neg @ torch.diag(torch.tensor([-1.0, 1.0, 1.0]))
    s = torch.zeros(12)
    s[:3] = flip.T @ P[:3, 3]
    s[3:6] = torch.tensor([0.05, -0.02, 0.0])
    s[6:9] = torch.tensor(Rotation.from_matrix(R.numpy().astype(np.float64)).as_rotvec(), dtype=torch.float32)
    return s


def main():
    net = MG._ref_network(2, False, 48.0)
    with torch.no_grad():
        net.color_net[-1].weight.mul_(COLOR_GAIN)      # contrast: the unchanged network renders an almost uniform grey
    check_opaque(net)
    intr = SC.intrinsics(H, W)
    get_rays_fn = lambda pose: MG.ref_get_rays(pose, intr, H, W)                  # noqa: E731  (validate.py:291)
    render_fn = lambda o, d: net.render(o, d, **RENDER)                          # noqa: E731  (validate.py:290)
    eye = torch.eye(3)
    agent = SimpleNamespace(dt=DT, g=10.0, mass=1.0, I=eye, invI=torch.inverse(eye))
    agent.drone_dynamics = lambda s_, a_: Agent.drone_dynamics(agent, s_, a_)

    start = start_state()
    actions = [torch.tensor([10.3, 0.01, -0.02, 0.0]), torch.tensor([9.8, 0.0, 0.01, 0.02]), torch.tensor([10.0, 0.0, 0.0, 0.0])]
    keypoints = [np.array([[10.3, 12.7], [20.9, 8.1], [15.5, 25.2], [10.9, 12.2]], np.float32),
                 np.array([[5.2, 6.8], [26.4, 19.9], [16.1, 16.6]], np.float32),
                 np.zeros((0, 2), np.float32)]
    # the sensor images: renders of states near the propagated ones (render_from_pose of the body pose), quantised as
    # NerfSimulator.py:102-106
    offsets = [5 * torch.tensor([0.01, -0.005, 0.004, 0, 0, 0, 0.01, 0.0, -0.008, 0, 0, 0]),
               5 * torch.tensor([-0.006, 0.008, 0.0, 0, 0, 0, -0.004, 0.006, 0.0, 0, 0, 0]), torch.zeros(12)]
    x = start.clone()
    images = []
    filt = SimpleNamespace(get_rays=get_rays_fn, render_fn=render_fn)
    for a, off in zip(actions, offsets):
        x = agent.drone_dynamics(x, a)
        s = x + off
        pose = torch.eye(4)
        pose[:3, :3] = vec_to_rot_matrix(s[6:9])
        pose[:3, 3] = s[:3]
        with torch.no_grad():
            img = torch.squeeze(EH.Estimator.render_from_pose(filt, pose)).numpy().reshape(H, W, -1).copy()
        img *= 255
        images.append(img.astype(np.uint8))

    rec = {"sig_prop": [], "hessian": []}
    det_calls = iter(keypoints)
    EH.cv2.SIFT_create = lambda *a, **k: SimpleNamespace(
        detect=lambda img, m: [SimpleNamespace(pt=(float(p[0]), float(p[1]))) for p in next(det_calls)])
    EH.cv2.dilate = lambda m, k, iterations=1: S.dilate(m, k.shape[0], iterations)
    real_hess, real_erp, real_cuda = torch.autograd.functional.hessian, EH.Estimator.estimate_relative_pose, torch.Tensor.cuda

    def spy_hess(*a, **k):
        h = real_hess(*a, **k)
        rec["hessian"].append(h.detach().numpy().copy())
        return h

    def spy_erp(self, img, start_state, sig, obs_img_pose=None):
        rec["sig_prop"].append(sig.detach().numpy().copy())
        return real_erp(self, img, start_state, sig, obs_img_pose=obs_img_pose)

    cfg = {"batch_size": BATCH, "kernel_size": 5, "dil_iter": 3, "lrate": 1e-3, "N_iter": N_ITER, "render_viz": False,
           "show_rate": [20, 100], "sig0": torch.eye(12), "Q": torch.eye(12)}
    out = {k: [] for k in ("state", "sig", "losses", "states", "batch", "success")}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        (Path(tmp) / "estimator_data").mkdir()
        torch.optim.Adam, torch.autograd.functional.hessian, EH.Estimator.estimate_relative_pose = _AdamCPU, spy_hess, spy_erp
        torch.Tensor.cuda = lambda self, *a, **k: self
        try:
            np.random.seed(SEED)                                  # seed_everything(seed) of NerfSimulator.reset
            est = EH.Estimator(cfg, agent, start.clone(), get_rays_fn=get_rays_fn, render_fn=render_fn)
            est.basefolder = Path(tmp)
            for img, a in zip(images, actions):
                n_hess = len(rec["hessian"])
                xt = est.estimate_state(img, None, a)
                out["state"].append(xt.numpy().copy())
                out["sig"].append(est.sig.detach().numpy().copy())
                out["losses"].append(np.asarray(est.losses, np.float64).reshape(-1))
                out["states"].append(np.asarray(est.states, np.float32).reshape(-1, 12))
                out["batch"].append(np.asarray(est.batch).copy())
                out["success"].append(len(rec["hessian"]) > n_hess)
        finally:
            torch.optim.Adam, torch.autograd.functional.hessian = _AdamCPU.__mro__[1], real_hess
            EH.Estimator.estimate_relative_pose, torch.Tensor.cuda = real_erp, real_cuda
    # G = dL_rgb/dpose of measurement_fn's pose at each estimate on its last batch (the reference's own first-order gradient): with
    # it, inverse(sig) + inverse(sig)^T + d^2/ds^2 <G, pose(s)> reproduces the recorded Hessians (tests/test_estimator_cpu.py)
    grads = []
    for i in range(2):
        b, xt = out["batch"][i], torch.from_numpy(out["state"][i])
        pose = torch.eye(4)
        rot = rot_x(torch.tensor(np.pi / 2)) @ vec_to_rot_matrix(xt[6:9])[:3, :3]
        pr, tr = nerf_matrix_to_ngp_torch(rot, xt[:3])
        pose[:3, :3], pose[:3, 3] = pr, tr
        pose.requires_grad_(True)
        rays = get_rays_fn(pose.reshape((1, 4, 4)))
        ro = rays["rays_o"].reshape((H, W, -1))[b[:, 0], b[:, 1]]
        rd = rays["rays_d"].reshape((H, W, -1))[b[:, 0], b[:, 1]]
        rgb = render_fn(ro.reshape((1, -1, 3)), rd.reshape((1, -1, 3)))["image"].reshape((-1, 3))
        target = torch.tensor((images[i] / 255.).astype(np.float32))[b[:, 0], b[:, 1]]
        g, = torch.autograd.grad(torch.nn.functional.mse_loss(rgb, target), pose)
        grads.append(g.numpy().copy())
    assert out["success"] == [True, True, False]
    assert all(im.std() > 5 for im in images[:2]), "the sensor frames should see the scene"
    arrays = {}
    for i in range(3):
        arrays[f"image{i}"], arrays[f"action{i}"], arrays[f"keypoints{i}"] = images[i], actions[i].numpy(), keypoints[i]
        arrays[f"state{i}"], arrays[f"sig{i}"], arrays[f"sig_prop{i}"] = out["state"][i], out["sig"][i], rec["sig_prop"][i]
        arrays[f"losses{i}"], arrays[f"states{i}"] = out["losses"][i], out["states"][i]
    for i in range(2):
        arrays[f"hessian{i}"], arrays[f"batch{i}"], arrays[f"grad_pose{i}"] = rec["hessian"][i], out["batch"][i], grads[i]
    MG.save("estimator.npz", color_gain=COLOR_GAIN, bound=2, density_scale=48.0, table_seed=0, H=H, W=W, seed=SEED, dt=DT, n_iter=N_ITER, batch_size=BATCH,
            num_steps=RENDER["num_steps"], start_state=start.numpy(), **MG._weights(net), **arrays)


if __name__ == "__main__":
    main()
