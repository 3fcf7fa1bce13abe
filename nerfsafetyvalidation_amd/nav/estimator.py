"""The reference's NeRF state estimator (nav/estimator_helpers.py:37-311 Estimator): the same class, method names and arithmetic
order, in fp32 outside autocast.

    estimate_state      propagate with the agent's dynamics, A = jacobian of the dynamics, sig_prop = A sig A^T + Q,
                        estimate_relative_pose, then sig = inverse(Hessian of measurement_fn at the estimate)
    estimate_relative_pose   keypoints and the dilated interest mask (nav/features.py: HIP), N_iter Adam steps on
                        measurement_fn over min(batch_size, n) interest pixels drawn without replacement per step
    measurement_fn      mahalanobis(state, start, sig) + MSE of the rendered pixels against the sensor image / 255

Two choices differ in form, not in value:
  * the pixel draws come from the estimator's own np.random.RandomState(seed): the stream NerfSimulator.reset's
    seed_everything(seed) gives the reference's global generator (the estimator is the only consumer of np.random in a step), without
    sharing one generator between simulations that run on several threads;
  * the Hessian.  The reference takes torch.autograd.functional.hessian of measurement_fn.  Its grid and SH encoders return their
    input gradients from an extension call that carries no graph, so the second derivative only sees where the state enters the
    rays differentiably: rays_o = t and rays_d = dirs R^T are linear in the pose, the sample positions o + d z piecewise linear.  The
    reference's matrix is therefore exactly  inverse(sig) + inverse(sig)^T + d^2/ds^2 <G, pose(s)>  with G = dL_rgb/dpose at the
    estimate held constant (one first-order backward through ngp_get_rays_backward) and pose(s) the twice-differentiable pose
    construction of measurement_fn; only the rotation block [6:9, 6:9] gets a render term ("The state estimator").
    Double-differentiating this package's own autograd nodes would NOT give that matrix (their backwards are kernel launches).

No JSON is written and nothing is printed or plotted: the history is kept on the object (losses, states, covariance,
state_estimate, action)."""
import numpy as np
import torch

from ..rollout import rot_x, vec_to_rot_matrix
from .features import sift_interest_mask

_FLIP_YZ = [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
_NEG_YZ = [[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]]


def mahalanobis(u, v, cov):
    """math_utils.py:17-19"""
    delta = u - v
    return delta @ torch.inverse(cov) @ delta


def state_to_pose(state):
    """measurement_fn's camera pose (estimator_helpers.py:205-216): rot_x(pi/2) @ R(state[6:9]), then nerf_matrix_to_ngp_torch, as a
    4x4 on the state's device; differentiable (twice) in the state"""
    dev = state.device
    R = vec_to_rot_matrix(state[6:9])
    rot = rot_x(np.pi / 2).to(dev) @ R[:3, :3]
    flip, neg = torch.tensor(_FLIP_YZ, device=dev), torch.tensor(_NEG_YZ, device=dev)
    pose, trans = flip @ rot @ neg, flip @ state[:3]
    top = torch.cat([pose, trans[:, None]], dim=1)
    return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)], dim=0)


def interest_pixels(mask_xy):
    """coords[interest_regions] of estimate_relative_pose (:100-107) for a mask indexed [x, y]: the (row, col) = (y, x) pairs in the
    mask's C order (x major) -- the order np.random.choice's indices refer to"""
    return np.ascontiguousarray(np.argwhere(mask_xy)[:, ::-1])


class Estimator:
    """estimator_helpers.py:37-311.  agent: an object with drone_dynamics(state [12], action [4]) -> [12].  get_rays_fn(pose [1,4,4],
    inds) -> {'rays_o', 'rays_d'} for the flat pixel ids `inds` (row * W + col); render_fn(rays_o, rays_d) -> {'image'}.
    seed: the pixel draws' np.random.RandomState."""

    def __init__(self, filter_cfg, agent, start_state, filter=True, get_rays_fn=None, render_fn=None, seed=0) -> None:
        self.batch_size = filter_cfg["batch_size"]
        self.kernel_size = filter_cfg["kernel_size"]
        self.dil_iter = filter_cfg["dil_iter"]
        self.lrate = filter_cfg["lrate"]
        self.agent = agent
        self.is_filter = filter
        self.xt = start_state
        self.sig = filter_cfg["sig0"]
        self.Q = filter_cfg["Q"]
        self.iter = filter_cfg["N_iter"]
        self.get_rays = get_rays_fn
        self.render_fn = render_fn
        self.rng = np.random.RandomState(seed)
        self.losses = None
        self.covariance = None
        self.state_estimate = None
        self.states = None
        self.action = None
        self.hessian = None
        self.keypoints = None
        self.iteration = 0

    def estimate_relative_pose(self, sensor_image, start_state, sig, obs_img_pose=None):
        """:77-189 -> (state [12], success).  sensor_image: uint8 [H, W, 3] (numpy or torch)."""
        if not self.is_filter:
            raise NotImplementedError("Estimator: filter=False is not implemented (as in the reference)")
        mask_xy, self.keypoints = self.interest_regions(sensor_image)
        if self.keypoints == 0:                        # :88-95: feature detection failed
            self.losses = []
            self.states = []
            return start_state.clone().detach(), False
        dev = start_state.device
        img = sensor_image.cpu().numpy() if torch.is_tensor(sensor_image) else np.asarray(sensor_image)
        target = torch.tensor((np.array(img) / 255.).astype(np.float32), device=dev)
        region = interest_pixels(mask_xy)

        optimized_state = start_state.clone().detach() + 1e-6
        optimized_state.requires_grad_(True)
        optimizer = torch.optim.Adam(params=[optimized_state], lr=self.lrate, betas=(0.9, 0.999), capturable=optimized_state.is_cuda)
        losses, states = [], []
        batch = None
        for _ in range(self.iter):
            optimizer.zero_grad()
            rand_inds = self.rng.choice(region.shape[0], size=min(self.batch_size, region.shape[0]), replace=False)
            batch = region[rand_inds]
            loss = self.measurement_fn(optimized_state, start_state, sig, target, batch)
            losses.append(loss.item())
            states.append(optimized_state.clone().cpu().detach().numpy().tolist())
            # loss.backward() restricted to the state: a map that still requires grad collects nothing (several simulations may
            # share one model on several threads)
            optimized_state.grad, = torch.autograd.grad(loss, [optimized_state])
            optimizer.step()
        self.target = target
        self.batch = batch
        self.losses = losses
        self.states = states
        return optimized_state.clone().detach(), True

    def interest_regions(self, sensor_image):
        """find_POI + the dilated mask (:84-106) on the GPU (nav/features.py) -> (bool [W, H] numpy, indexed [x, y]; keypoint count)"""
        det = sift_interest_mask(sensor_image, self.kernel_size, self.dil_iter)
        return det["mask"].cpu().numpy().astype(bool), int(det["count"].item())

    def _render_loss(self, pose, target, batch):
        """MSE of the rendered batch pixels for a 4x4 pose"""
        H, W, _ = target.shape
        b = torch.as_tensor(np.ascontiguousarray(batch), device=target.device)
        rays = self.get_rays(pose.reshape((1, 4, 4)), b[:, 0] * W + b[:, 1])
        output = self.render_fn(rays["rays_o"].reshape((1, -1, 3)), rays["rays_d"].reshape((1, -1, 3)))
        rgb = output["image"].reshape((-1, 3)).float()
        return torch.nn.functional.mse_loss(rgb, target[b[:, 0], b[:, 1]])

    def measurement_fn(self, state, start_state, sig, target, batch):
        """:191-225: mahalanobis(state, start_state, sig) + MSE of the rendered batch pixels"""
        loss_dyn = mahalanobis(state, start_state, sig)
        loss_rgb = self._render_loss(state_to_pose(state), target, batch)
        return loss_rgb + loss_dyn

    def measurement_hessian(self, state, sig):
        """the reference's hessian(measurement_fn) at `state` (see the module docstring): inverse(sig) + inverse(sig)^T, plus
        d^2/ds^2 <G, pose(s)> with G = dL_rgb/dpose at `state` on the last batch"""
        state = state.detach()
        pose = state_to_pose(state).detach().requires_grad_(True)
        loss_rgb = self._render_loss(pose, self.target, self.batch)
        G, = torch.autograd.grad(loss_rgb, pose)
        G = G.detach()
        render = torch.autograd.functional.hessian(lambda s: (G * state_to_pose(s)).sum(), state)
        inv = torch.inverse(sig)
        return (inv + inv.T) + render

    def render_from_pose(self, pose):
        """:227-244: the full frame of a body pose (4x4)"""
        rot = rot_x(np.pi / 2).to(pose.device) @ pose[:3, :3]
        flip, neg = torch.tensor(_FLIP_YZ, device=pose.device), torch.tensor(_NEG_YZ, device=pose.device)
        new_pose = torch.eye(4, device=pose.device)
        new_pose[:3, :3] = flip @ rot @ neg
        new_pose[:3, 3] = flip @ pose[:3, 3]
        rays = self.get_rays(new_pose.reshape((1, 4, 4)), None)
        return torch.squeeze(self.render_fn(rays["rays_o"], rays["rays_d"])["image"])

    def render_for_uncertainty(self, pose):
        """:246-262 -> (render output, rays_o, rays_d) without grad"""
        rot = rot_x(np.pi / 2).to(pose.device) @ pose[:3, :3]
        flip, neg = torch.tensor(_FLIP_YZ, device=pose.device), torch.tensor(_NEG_YZ, device=pose.device)
        new_pose = torch.eye(4, device=pose.device)
        new_pose[:3, :3] = flip @ rot @ neg
        new_pose[:3, 3] = flip @ pose[:3, 3]
        rays = self.get_rays(new_pose.reshape((1, 4, 4)), None)
        with torch.no_grad():
            output = self.render_fn(rays["rays_o"], rays["rays_d"])
        return output, rays["rays_o"], rays["rays_d"]

    def estimate_state(self, sensor_img, obs_img_pose, action):
        """:264-311 -> the state estimate [12].  self.success: whether the relative-pose fit ran (False: no keypoint; the estimate is
        the propagated state and sig keeps its previous value)."""
        with torch.autocast("cuda", enabled=False):
            self.xt = self.agent.drone_dynamics(self.xt, action)
            self.action = action.detach().cpu().numpy().tolist()
            A = torch.autograd.functional.jacobian(lambda x: self.agent.drone_dynamics(x, action), self.xt)
            A = A.to(self.sig.device)
            sig_prop = A @ self.sig @ A.T + self.Q
            xt, success_flag = self.estimate_relative_pose(sensor_img, self.xt.clone().detach().to(self.sig.device), sig_prop,
                                                           obs_img_pose=obs_img_pose)
            if self.is_filter is True and success_flag is True:
                hess = self.measurement_hessian(xt, sig_prop)
                self.hessian = hess
                self.sig = torch.inverse(hess)
        self.success = success_flag
        self.xt = xt.to(self.xt.device)
        self.covariance = self.sig.clone().cpu().detach().numpy().tolist()
        self.state_estimate = self.xt.clone().cpu().detach().numpy().tolist()
        self.iteration += 1
        return self.xt.clone().detach()


def estimator_config(device, **overrides):
    """envConfig.json's estimator_cfg (dil_iter 3, kernel 5, batch 1024, lrate 1e-3, N_iter 100) with validate.py:170-171,269-270's
    sig0 = Q = I_12 on `device`.  `overrides` replace entries."""
    cfg = {"dil_iter": 3, "kernel_size": 5, "batch_size": 1024, "lrate": 1e-3, "N_iter": 100,
           "sig0": torch.eye(12, dtype=torch.float32, device=device), "Q": torch.eye(12, dtype=torch.float32, device=device)}
    cfg.update(overrides)
    return cfg


__all__ = ["Estimator", "estimator_config", "interest_pixels", "mahalanobis", "state_to_pose"]
