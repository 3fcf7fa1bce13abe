"""The Monte-Carlo stress-test rollout as a render workload (BASELINE configs[4]; SURVEY.md section 8d "Rollout config 5").

What `validate.py` runs per simulation step (validation/stresstests/MonteCarlo.py:38-116 around
validation/simulators/NerfSimulator.py:66-157), reduced to the part that is this repo's path:

    noise ~ N(mean, std + 0.01 * std * reward)              MonteCarlo.py:49-53   (12-D disturbance, envConfig.json:45-46)
    state  = drone_dynamics(state, action) + noise          nav/agent_helpers.py:43-56,102-148
    pose   = camera pose of the state in the NeRF's frame   agent_helpers.py:58-77 -> nav/estimator_helpers.py:227-237
    render #1 = render_fn(get_rays_fn(pose))                NerfSimulator.py:102   (filter.render_from_pose)
    render #2 = the same frame again, no_grad               NerfSimulator.py:110   (filter.render_for_uncertainty)
    sigma_d   = GaussianApproximationDensityUncertainty(rgbs, sigmas, image of render #2).optimize()     uncertain.py:78-91
    reward    = clip(loglik(noise) - 36 * sigma_d, -72, 36) NerfSimulator.py:159-181
    one CSV row                                             MonteCarlo.py:58-116

Not here (out of scope): the SIFT / iNeRF state estimator unless it is asked for (below).  Its place is taken by a
fixed, documented stand-in so that the rollout still produces every column of the reference's CSV.  The ground-truth image of the
reference's second simulator (BlenderSimulator.py:82,102: Agent.get_img, a Blender subprocess) is opt-in without Blender (`world`, a
world.MeshWorld: a HIP ray caster looking at a triangle mesh): every step the world's frame of the true pose, quantised to uint8, is
kept as `world_image` and, with the estimator, is the sensor image in the place of render #1 -- so the NeRF's model error enters the
rollout.  The NeRF renders and the step's uncertainty run as without it.  The signed distance field is opt-in (`sdf`, a collision.SignedDistanceField: built on the GPU from the NeRF's
density, or the reference's own `sdf.npy` through from_array): each interpolated state is looked up as NerfSimulator.py:131-147
does -- the value starts at 9999, a point outside the field keeps the previous value, the first collision ends the check.
Without it (`sdf=None`, the default) the stand-in looks the four interpolated states up in the analytic occupancy of the
synthetic scene (scene_collision: 0 inside, 9999 outside).  The A* + Adam planner (nav.Planner) is opt-in (`planner_cfg`, built by planner_config()):
    reset      Planner + a_star_init + learn_init under seed_everything(seed) (NerfSimulator.py:182-214), computed ONCE per rollout
               and copied into every simulation -- the stand-in for the reference's on-disk `cached/` plans;
    each step  action = get_next_action() (NerfSimulator.py:82); after dynamics and noise update_state(state_est) and
               learn_update(k) (:126-129), where state_est is the TRUE noisy state as an 18-vector (:120) -- the stand-in for the
               estimator.  The simulation starts at rest in start_pos (validate.py:224-233) and steps by the plan's dt.
The reference's NeRF state estimator (nav.Estimator) is opt-in on top of the planner (`estimator_cfg`, built by
nav.estimator_config()): each simulation builds a fresh Estimator at the true start state; every step render #1's image, quantised
as NerfSimulator.py:102-106 does (* 255, astype(uint8)), is the sensor image of estimate_state (:120), and the planner replans from
the estimate instead of the true state.  The per-step estimates, covariances and success flags are kept on the simulator.
Without it (`planner_cfg=None`, the default) the planner's action is hover thrust (zero torque) with the straight-line velocity
from `start_pos` to `end_pos` as the initial condition (the path the A* initialisation approximates).

Simulations are independent given their seed -- the reference's own CEM draws with `manual_seed(noise_seed + simulationNumber)`
(validation/distributions/SeedableMultivariateNormal.py:19-22) -- so they shard over ranks with no data-path collective; the rows are
gathered once at the end (dist.gather_views).  Within a rank several simulations advance concurrently, each on its own host thread
and HIP stream (pipeline.FramePipeline): a simulation's steps are sequential (the reward feeds the next step's noise), the
simulations are not.  The Cross Entropy Method stress test (cem.py) runs its populations through the same step (RolloutSimulator.run
with another noise source and row writer) and the same machinery (run_simulations, gather_rows); run_validation picks between the two.
"""
import math

import numpy as np
import torch

from .dist import gather_views, shard_range
from .scene import henge_occupancy

# envConfig.json (reference repo root): the values the rollout depends on
ENV = {
    "mpc_noise_mean": [0.0] * 12,                                                                      # :45
    "mpc_noise_std": [2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2, 2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2],         # :46
    "mass": 1.0, "g": 10.0, "I": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],                  # :23-25
    "start_pos": [-0.75, -0.235, 0.25], "end_pos": [0.2, -0.74, 0.3], "start_R": [0.0, 0.0, 0.0],      # :32-35
    "T_final": 2.0,                                                                                    # :37
}
# envConfig.json's agent_cfg / planner_cfg values the planner adds (validate.py:169-256)
PLANNER_ENV = {
    "body_lims": [[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]], "body_nbins": [10, 10, 5],                          # :17-22
    "end_R": [0.0, 0.0, 0.0], "steps": 12, "planner_lr": 0.001, "epochs_init": 1000, "fade_out_epoch": 0,            # :36-45
    "fade_out_sharpness": 10, "epochs_update": 250,
}
PLANNER_ROT = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]    # validate.py:283: Blender -> NeRF axes of density_fn
ROW_WIDTH = 24   # MonteCarlo.py:95-116: sim, step, noise x12, sdf value, xyz, step loglik, cumulative loglik, reward, sigma, collided (+ ever collided)
PENALTY = 36.0   # NerfSimulator.py:171
UQ_GAUSSIAN, UQ_LAPLACE = "Gaussian Approximation", "Bayesian Laplace Approximation"     # envConfig.json's uq_method
NUM_PERTURBATIONS = 3   # NerfSimulator.py:172


# ------------------------------------------------------------------ SO(3) helpers (nav/math_utils.py), float32 on the host
def rot_x(phi):
    """math_utils.py:12-15 (cos / sin of the float32 angle, as torch.cos(torch.tensor(phi)) gives them)"""
    p = torch.tensor(phi, dtype=torch.float32)
    c, s = float(torch.cos(p)), float(torch.sin(p))
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=torch.float32)


def skew(v):
    """math_utils.py:167-178 (and :92-102): vector [...,3] -> skew-symmetric [...,3,3]"""
    S = torch.zeros(*v.shape[:-1], 3, 3, dtype=v.dtype, device=v.device)
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def vec_to_rot_matrix(rot_vec):
    """Rodrigues (math_utils.py:151-165): axis = v / (1e-10 + |v|)"""
    angle = torch.linalg.vector_norm(rot_vec, dim=-1, keepdim=True)
    S = skew(rot_vec / (1e-10 + angle))
    angle = angle[..., None]
    return torch.eye(3, dtype=rot_vec.dtype, device=rot_vec.device) + torch.sin(angle) * S + (1 - torch.cos(angle)) * (S @ S)


def rot_matrix_to_vec(R, eps=1e-7):
    """math_utils.py:104-149: angle from the trace through the clamped arccos, axis from the antisymmetric part"""
    x = (torch.diagonal(R, dim1=-2, dim2=-1).sum(-1) - 1) / 2
    slope = float(np.arccos(1 - eps) / eps)
    good = x.abs() <= 1 - eps
    sign = torch.sign(x)
    angle = torch.where(good, torch.acos(x.clamp(-1 + eps, 1 - eps)),
                        torch.acos(sign * (1 - eps)) - slope * sign * (x.abs() - 1 + eps))[..., None]
    vec = 1 / (2 * torch.sin(angle + 1e-10)) * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0],
                                                             R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    vec = torch.where(angle == 0, torch.zeros_like(vec), vec)
    return angle * vec


# ------------------------------------------------------------------ drone dynamics (nav/agent_helpers.py:102-148)
def drone_dynamics(state, action, dt, mass=ENV["mass"], g=ENV["g"], inertia=None):
    """state [...,12] = pos, vel (world), rotation vector, body rates; action [...,4] = thrust, torque -> next state [...,12].
    One explicit Euler step; the rotation advances by the exponential map of omega * dt."""
    inertia = torch.tensor(ENV["I"], dtype=torch.float32) if inertia is None else inertia
    inv_inertia = torch.inverse(inertia)
    pos, v, omega = state[..., 0:3], state[..., 3:6], state[..., 9:12]
    R = vec_to_rot_matrix(state[..., 6:9])
    thrust = torch.zeros_like(pos)
    thrust[..., 2] = action[..., 0]
    dv = (torch.tensor([0.0, 0.0, -mass * g]) + (R @ thrust[..., None])[..., 0]) / mass
    Iw = (inertia @ omega[..., None])[..., 0]
    domega = (inv_inertia @ (action[..., 1:4] - torch.linalg.cross(omega, Iw))[..., None])[..., 0]
    angle = omega * dt
    theta = torch.linalg.vector_norm(angle, dim=-1, keepdim=True)
    K = skew(angle / torch.where(theta == 0, torch.ones_like(theta), theta))
    th = theta[..., None]
    exp_i = torch.eye(3) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)        # = I for theta == 0, as :130-131
    nxt = torch.empty_like(state)
    nxt[..., 0:3] = pos + v * dt
    nxt[..., 3:6] = v + dv * dt
    nxt[..., 6:9] = rot_matrix_to_vec(R @ exp_i)
    nxt[..., 9:12] = omega + domega * dt
    return nxt


_FLIP_YZ = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
_NEG_YZ = torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])


def camera_pose(state):
    """The cam2world matrix NerfSimulator renders for a drone state, in the NeRF's frame: agent_helpers.py:58-61,75 build the
    body-frame pose (rot_x(pi/2) @ R, then rot_x(-pi/2) @ that), estimator_helpers.py:227-237 turn it into the camera
    (rot_x(pi/2) @ .) and math_utils.py:19-31 (nerf_matrix_to_ngp_torch) into the ngp axes."""
    R = vec_to_rot_matrix(state[..., 6:9])
    body = rot_x(-math.pi / 2) @ (rot_x(math.pi / 2) @ R)
    rot = rot_x(math.pi / 2) @ body
    pose = torch.eye(4).repeat(*state.shape[:-1], 1, 1)
    pose[..., :3, :3] = _FLIP_YZ @ rot @ _NEG_YZ
    pose[..., :3, 3] = (_FLIP_YZ @ state[..., 0:3, None])[..., 0]
    return pose


def trajectory_log_likelihood(noise, mean, std):
    """MonteCarlo.py:30-36: sum of log(clip(N(noise; mean, std), 1e-8, 1e8)), float64 as scipy.stats.norm.pdf"""
    noise, mean, std = [np.asarray(a, np.float64) for a in (noise, mean, std)]
    pdf = np.exp(-0.5 * ((noise - mean) / std) ** 2) / (std * math.sqrt(2 * math.pi))
    return float(np.log(np.clip(pdf, 1e-8, 1e8)).sum())


def reward_fn(likelihood, sigma_d_opt):
    """NerfSimulator.py:159-181, uq_method == 'Gaussian Approximation'"""
    return float(np.clip(likelihood - PENALTY * sigma_d_opt, -PENALTY * 2, PENALTY))


def reward_fn_laplace(likelihood, rmv, trace):
    """NerfSimulator.py:177-179, uq_method == 'Bayesian Laplace Approximation': step() unpacks uncertainty()'s (trace, rmv) as
    `trace, sigma` and returns `sigma, trace` (:110,148), so sigma_d_opt is the root mean variance and `trace` the trace"""
    return float(np.clip(likelihood - PENALTY * rmv * trace * NUM_PERTURBATIONS, -PENALTY * 2, PENALTY))


def scene_collision(state_xyz):
    """Stand-in for the sdf.npy lookup of NerfSimulator.py:131-155: is the (drone-frame) position inside the analytic occupancy
    of the synthetic scene (scene.henge_occupancy, in the NeRF's axes)?  Returns (collided, value) with value 0 inside, 9999 free."""
    ngp = (_FLIP_YZ.numpy().astype(np.float64) @ np.asarray(state_xyz, np.float64))
    inside = bool(henge_occupancy(np.float64(ngp[0]), np.float64(ngp[1]), np.float64(ngp[2])))
    return inside, (0.0 if inside else 9999.0)


def initial_state(n_steps):
    """12-vector start state (validate.py:228-241 with start_R = 0, zero rates) with the straight-line velocity towards end_pos"""
    s = torch.zeros(12)
    start, end = torch.tensor(ENV["start_pos"]), torch.tensor(ENV["end_pos"])
    s[0:3] = start
    s[3:6] = (end - start) / ENV["T_final"]
    s[6:9] = torch.tensor(ENV["start_R"])
    return s


def planner_config(device, **overrides):
    """validate.py:224-256's planner_cfg from ENV / PLANNER_ENV: start and end 18-vectors (zero rates, R from vec_to_rot_matrix)
    on `device`, and the scalars.  `overrides` replace entries (e.g. epochs_init, epochs_update)."""
    rates = torch.zeros(3)
    start_R = vec_to_rot_matrix(torch.tensor(ENV["start_R"]))
    end_R = vec_to_rot_matrix(torch.tensor(PLANNER_ENV["end_R"]))
    start_state = torch.cat([torch.tensor(ENV["start_pos"]).float(), rates, start_R.reshape(-1), rates], dim=0)
    end_state = torch.cat([torch.tensor(ENV["end_pos"]).float(), rates, end_R.reshape(-1), rates], dim=0)
    cfg = {"T_final": ENV["T_final"], "steps": PLANNER_ENV["steps"], "lr": PLANNER_ENV["planner_lr"],
           "epochs_init": PLANNER_ENV["epochs_init"], "fade_out_epoch": PLANNER_ENV["fade_out_epoch"],
           "fade_out_sharpness": PLANNER_ENV["fade_out_sharpness"], "epochs_update": PLANNER_ENV["epochs_update"],
           "start_state": start_state.to(device), "end_state": end_state.to(device),
           "I": torch.tensor(ENV["I"]).float().to(device), "g": ENV["g"], "mass": ENV["mass"],
           "body": np.array(PLANNER_ENV["body_lims"]), "nbins": PLANNER_ENV["body_nbins"]}
    cfg.update(overrides)
    return cfg


def initial_plan(model, planner_cfg, seed):
    """NerfSimulator.reset's planner (NerfSimulator.py:188-214): seed_everything(seed), Planner, a_star_init, learn_init -- fp32
    outside autocast, density_fn = validate.py:288's query of `model` (nav.density_query)"""
    from .nav import Planner, density_query
    from .nerf.utils import seed_everything
    device = planner_cfg["start_state"].device
    seed_everything(seed)
    with torch.autocast("cuda", enabled=False):
        plan = Planner(planner_cfg["start_state"], planner_cfg["end_state"], planner_cfg,
                       density_query(model, torch.tensor(PLANNER_ROT, device=device)))
        plan.a_star_init()
        plan.learn_init()
    return plan


def copy_plan(plan):
    """an independent planner continuing from `plan` (its own states and initial acceleration; the rest is read-only)"""
    import copy
    p = copy.copy(plan)
    p.states = plan.states.detach().clone().requires_grad_(True)
    p.initial_accel = plan.initial_accel.detach().clone().requires_grad_(True)
    return p


class RolloutSimulator:
    """One simulation = `steps` calls of step(); mirrors NerfSimulator.step's use of the renderer (two full-frame renders and the
    Gaussian-approximation UQ per step) and MonteCarlo.validate's bookkeeping."""

    def __init__(self, model, intrinsics, H, W, steps, seed=0, render_kwargs=None, num_interpolated_points=4, renders_per_step=2,
                 planner_cfg=None, initial_plan=None, sdf=None, estimator_cfg=None, uq_method=UQ_GAUSSIAN, uq_kwargs=None, world=None,
                 body=None, exact=False, clearance=None):
        """planner_cfg: None (the hover stand-in) or planner_config()'s dict: the reference's planner steers the drone.
        initial_plan: the plan after reset when the caller has computed it already (run_rollout: once per rollout).
        sdf: None (the analytic stand-in, scene_collision), a collision.SignedDistanceField the collision check looks up, or "world":
        the ground-truth field of `world`'s mesh over reference_box() (SignedDistanceField.from_mesh; needs world=).
        estimator_cfg: None (the planner replans from the true state) or nav.estimator_config()'s dict: the reference's estimator
        turns render #1 of every step into the state the planner replans from (needs planner_cfg).
        uq_method: envConfig.json's key.  The default, 'Gaussian Approximation', is the path described above.  'Bayesian Laplace
        Approximation': uncertain.uncertainty on render #2 and its rays (NerfSimulator.py:110), the row's uncertainty column holds the
        root mean variance and the reward is reward_fn_laplace.  uq_kwargs: its keywords (lr -- the reference passes filter.lrate,
        1e-3 -- and BayesianLaplace.fit's, e.g. n_steps, likelihood_gradient, lm_solver).
        world: None (the NeRF is its own world: render #1 is the sensor image), or a world.MeshWorld: the true world
        (BlenderSimulator.py:82,102).  Every step its frame of the true pose is kept as self.world_image (uint8 [H,W,3] numpy) and,
        with estimator_cfg, is the estimator's sensor image; shared and read-only between simulations.
        body: None (the reference's verdict: the centre point's field value, today's rows byte for byte, nothing new launched), or a
        collision.BodyBox (BodyBox.planner(): the planner's body_lims): the collided column carries the verdict of that box at the
        step's interpolated poses, by world.py's body rule -- exact=False against the occupied cells of `sdf` (any field: a NeRF-density
        one or sdf="world"), exact=True against the triangles of `world` (needs world=).  Columns 14 and 15:18 stay the centre's field
        value and position; self.body_hits keeps, per step, the `cell` (or `prim`) of each interpolated pose (int32 [n_interp], -1:
        free).  The analytic stand-in (sdf=None) has no map: a body with it is a ValueError.
        clearance: None (column 14 stays the centre's field value; nothing new launched), or a finite length D > 0 in metres (needs
        body=): the step's n_interp boxes go through ONE clearance call (world.py's clearance rule; against the same geometry as the
        verdict) in the place of the overlap call.  The verdict is its `hit`, so the collided column is what body= alone gives; column
        14 -- and through it the Cross Entropy Method's adjusted value and risk -- is the smallest min(distance, D) over the poses the
        walk visits (up to and including the first hit): 0.0 on a collision, D in open space.  self.body_clearance keeps, per step,
        the distances of the interpolated poses (float64 [n_interp], +inf beyond D)."""
        self.world, self.world_image = world, None
        from .collision import check_body, check_clearance, resolve_sdf
        sdf = resolve_sdf(sdf, world, "RolloutSimulator")
        check_body(body, exact, sdf, world, "RolloutSimulator")
        self.body, self.exact, self.body_hits = body, bool(exact), []
        self.clearance, self.body_clearance = check_clearance(clearance, body, "RolloutSimulator"), []
        if uq_method not in (UQ_GAUSSIAN, UQ_LAPLACE):
            raise ValueError(f"Unrecognized uncertainty quantification method {uq_method}")
        self.uq_method, self.uq_kwargs, self.last_trace = uq_method, dict(uq_kwargs or {}), None
        from .nerf.utils import get_rays
        from .uncertainty.quantification.gaussian_approximation_density_uncertainty import GaussianApproximationDensityUncertainty
        self.model, self.intrinsics, self.H, self.W, self.steps, self.seed = model, intrinsics, H, W, steps, seed
        self.device = next(model.parameters()).device if model is not None else None
        # frame_width: scheduling hint of this build's renderer (the rays are whole row-major frames); results do not depend on it
        self.render_kwargs = dict(staged=True, bg_color=1.0, perturb=False, frame_width=W)
        self.render_kwargs.update(render_kwargs or {})
        self.n_interp = num_interpolated_points
        self.renders_per_step = renders_per_step
        self.dt = ENV["T_final"] / steps                       # NerfSimulator.py:40
        self.planner_cfg, self._initial_plan, self.planner = planner_cfg, initial_plan, None
        self.sdf = sdf
        self.estimator_cfg, self.estimator = estimator_cfg, None
        if estimator_cfg is not None and planner_cfg is None:
            raise ValueError("RolloutSimulator: estimator_cfg needs planner_cfg (the estimate is what the planner replans from)")
        if planner_cfg is not None:
            self.dt = planner_cfg["T_final"] / planner_cfg["steps"]   # agent_cfg['dt'] (NerfSimulator.py:36)
        self.mean = torch.tensor(ENV["mpc_noise_mean"], dtype=torch.float32)
        self.std = torch.tensor(ENV["mpc_noise_std"], dtype=torch.float32)
        self._get_rays, self._UQ = get_rays, GaussianApproximationDensityUncertainty
        self.frames = 0
        self.samples = 0

    def render(self, pose):
        rays = self._get_rays(pose.reshape(1, 4, 4).to(self.device), self.intrinsics, self.H, self.W)
        out = self.model.render(rays["rays_o"], rays["rays_d"], **self.render_kwargs)
        self.frames += 1
        self.last_rays = rays
        return out

    def uncertainty_laplace(self, out, rays):
        """uncertain.py:181-231 on a render and its rays -> (trace, rmv)"""
        from .uncertain import LAPLACE, uncertainty
        kw = dict(self.uq_kwargs)
        lr = kw.pop("lr", (self.estimator_cfg or {}).get("lrate", 1e-3))
        return uncertainty(LAPLACE, rendered_output=(out, rays["rays_o"], rays["rays_d"]), model_to_use=self.model, lr=lr, **kw)

    def reward(self, loglik, sigma_d):
        """NerfSimulator.reward (:159-181) for this simulator's uq_method"""
        if self.uq_method == UQ_LAPLACE:
            return reward_fn_laplace(loglik, sigma_d, self.last_trace)
        return reward_fn(loglik, sigma_d)

    def uncertainty(self, out):
        """uncertain.py:78-91: c = rgbs, d = sigmas, r = image of the render"""
        c, d = out["rgbs"], out["sigmas"]
        if c.dim() == 2:            # run_cuda's last-iteration tensors [M,3] / [M]: one sample per row
            c = c[:, None, :]
        uq = self._UQ(c, d.reshape(-1), out["image"])
        mu, sigma = uq.optimize()
        return float(mu), float(sigma), uq.stats

    # ---- the four places where the reference talks to something outside the path; tests override them ------------------------
    def make_generator(self, sim):
        """SeedableMultivariateNormal.py:19-22: seed + simulation number (simulations are independent and shardable)"""
        return torch.Generator().manual_seed(self.seed + sim)

    def action(self, k, state):
        """Planner.get_next_action (nav/quad_plot.py:211-214, NerfSimulator.py:82) with a planner; else the stand-in: hover thrust,
        zero torque"""
        if self.planner is not None:
            with torch.no_grad(), torch.autocast("cuda", enabled=False):      # the plan is fp32 (the render may run under autocast)
                return self.planner.get_next_action().detach().cpu()
        return torch.tensor([ENV["mass"] * ENV["g"], 0.0, 0.0, 0.0])

    def reset_planner(self):
        """NerfSimulator.reset's planner (a copy of the rollout's initial plan), or None without planner_cfg"""
        if self.planner_cfg is None:
            self.planner = None
            return
        if self._initial_plan is None:
            self._initial_plan = initial_plan(self.model, self.planner_cfg, self.seed)
        self.planner = copy_plan(self._initial_plan)

    def replan(self, k, state):
        """NerfSimulator.py:120-129: the state estimate as an 18-vector (stand-in: the true noisy state), update_state, learn_update"""
        if self.planner is None:
            return
        if self.estimator is not None:
            state = self.estimate(k, state)
        dev = self.planner.device
        s = state.to(dev)
        state_est = torch.cat([s[:6], vec_to_rot_matrix(s[6:9]).reshape(-1), s[9:]], dim=-1)
        with torch.autocast("cuda", enabled=False):
            self.planner.update_state(state_est)
            self.planner.learn_update(k)

    def reset_estimator(self, sim, start_state):
        """NerfSimulator.reset's Estimator (:196-197) at the true start state, drawing its pixels from seed + simulation number"""
        self.estimates, self.covariances, self.estimate_success = [], [], []
        if self.estimator_cfg is None:
            self.estimator = None
            return
        from .nav.estimator import Estimator
        from .nerf.utils import get_rays
        kw = {k: v for k, v in self.render_kwargs.items() if k != "frame_width"}   # (sparse pixels: no frame to schedule by)
        dev, dt = self.device, self.dt

        class _Agent:
            @staticmethod
            def drone_dynamics(x, action):
                return drone_dynamics(x, action, dt)

        self.estimator = Estimator(self.estimator_cfg, _Agent(), start_state.clone(), seed=self.seed + sim,
                                   get_rays_fn=lambda pose, inds: get_rays(pose.to(dev), self.intrinsics, self.H, self.W, inds=inds),
                                   render_fn=lambda o, d: self.model.render(o, d, **kw))

    def estimate(self, k, state):
        """NerfSimulator.py:120: estimate_state on the quantised render #1 of this step -> the 12-vector the planner replans from"""
        est = self.estimator.estimate_state(self.sensor_image, self.poses[-1], self.actions[-1]).cpu()
        self.estimates.append(est.numpy().copy())
        self.covariances.append(np.asarray(self.estimator.covariance, np.float32))
        self.estimate_success.append(bool(self.estimator.success))
        return est

    def observe(self, pose):
        """NerfSimulator.py:100-110: the NeRF render of the true pose, the same frame again for the UQ -> sigma_d_opt.  With the
        estimator, render #1's image quantised as :102-106 (* 255, astype(uint8)) becomes self.sensor_image -- or, with a world, the
        world's frame of the pose (BlenderSimulator.py:82,102)."""
        with torch.no_grad():
            if self.world is not None:
                self.world_image = self.world.render(pose, self.intrinsics, self.H, self.W)["image_u8"].cpu().numpy()
                if self.estimator is not None:
                    self.sensor_image = self.world_image
            out = None
            for i in range(self.renders_per_step):
                out = self.render(pose)
                if i == 0 and self.estimator is not None and self.world is None:
                    img = torch.squeeze(out["image"]).float().cpu().numpy().reshape((self.H, self.W, -1))
                    img *= 255
                    self.sensor_image = img.astype(np.uint8)
            if self.uq_method == UQ_LAPLACE:
                self.last_trace, rmv = self.uncertainty_laplace(out, self.last_rays)
                return rmv
            return self.uncertainty(out)[1]

    def judge_body(self, states):
        """the body's verdict at interpolated states [n, 6] (xyz, rotation vector) -> int32 [n] numpy: the overlapped triangle
        (exact) or occupied cell of each pose, -1 where the body is free; one call, on the simulator's device"""
        from .collision import body_boxes
        boxes = body_boxes(states, self.body)
        if self.exact:
            hits = self.world.box_overlap(boxes)["prim"]
        else:
            device = self.device if self.device is not None else getattr(self.world, "device", None)
            hits = self.sdf.box_overlap(boxes, device=device if device is not None and device.type == "cuda" else None)
        return np.asarray(hits.cpu().numpy() if isinstance(hits, torch.Tensor) else hits, np.int32)

    def measure_body(self, states):
        """the body's clearance at interpolated states [n, 6] (xyz, rotation vector), capped at self.clearance -> {"distance" float64
        [n] (0 on a hit, +inf beyond the cap), "hit" int32 [n]: judge_body's answer} numpy; one call, on the simulator's device"""
        from .collision import body_boxes
        boxes = body_boxes(states, self.body)
        if self.exact:
            out = self.world.box_clearance(boxes, self.clearance)
        else:
            device = self.device if self.device is not None else getattr(self.world, "device", None)
            out = self.sdf.box_clearance(boxes, self.clearance, device=device if device is not None and device.type == "cuda" else None)
        host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a                          # noqa: E731
        return {"distance": np.asarray(host(out["distance"]), np.float64), "hit": np.asarray(host(out["hit"]), np.int32)}

    def collision(self, xyz):
        """-> (collided, value): the SDF lookup (value None: outside the field, keep the previous value) or the analytic stand-in"""
        if self.sdf is not None:
            return self.sdf.lookup(xyz)
        return scene_collision(xyz)

    # ---- the two places where the stress tests differ (cem.CEMSimulator overrides them): where a step's noise comes from and what
    # ---- a step writes
    def begin(self, sim):
        """start simulation `sim`'s noise source and bookkeeping (MonteCarlo.py:41-47)"""
        self._gen = self.make_generator(sim)
        self._reward, self._cumulative = 0.0, 0.0

    def draw_noise(self, sim, k):
        """MonteCarlo.py:49-53: the std widened by the previous step's reward"""
        std = self.std + (0.01 * self.std) * self._reward
        return torch.normal(self.mean, std, generator=self._gen)

    def write_row(self, sim, k, noise, value, where, sigma_d, collided):
        """MonteCarlo.py:58-116: one CSV row; the reward it computes applies to the NEXT step (:81-83)"""
        loglik = trajectory_log_likelihood(noise.numpy(), self.mean.numpy(), self.std.numpy())
        self._cumulative += loglik
        row = [sim, k, *noise.tolist(), value, *where.tolist(), loglik, self._cumulative, self._reward, sigma_d, float(collided)]
        self._reward = self.reward(loglik, sigma_d)
        return row

    def run(self, sim):
        """-> rows [n_steps_run, row width] float64 (a collision ends the simulation, MonteCarlo.py:88-93); the last column,
        "ever collided", is added once the simulation is over (MonteCarlo.py:112)"""
        self.begin(sim)
        self.reset_planner()
        state = initial_state(self.steps)
        if self.planner is not None:                           # at rest in start_pos (validate.py:224-233, NerfSimulator.py:30-33)
            state[3:6] = 0.0
        self.reset_estimator(sim, state)
        history = [state.numpy().astype(np.float64)]
        rows = []
        self.poses, self.actions, self.body_hits, self.body_clearance = [], [], [], []
        for k in range(self.steps):
            noise = self.draw_noise(sim, k)
            action = self.action(k, state)
            self.actions.append(action)
            state = drone_dynamics(state, action, self.dt) + noise          # agent_helpers.py:47-56
            history.append(state.numpy().astype(np.float64))
            pose = camera_pose(state)
            self.poses.append(pose)
            sigma_d = self.observe(pose)
            self.replan(k, state)
            # linear interpolation of the true states, last `n_interp` points checked (NerfSimulator.py:92-97,131-155)
            hist = np.stack(history)
            x = np.arange(hist.shape[0])
            xn = np.linspace(0, hist.shape[0] - 1, hist.shape[0] * self.n_interp)
            interp = np.stack([np.interp(xn, x, hist[:, i]) for i in range(3)], -1)[-self.n_interp:]
            hits, gaps, gap = None, None, self.clearance
            if self.body is not None:                          # the same np.interp rule on the rotation vector: one judgement of all poses
                turn = np.stack([np.interp(xn, x, hist[:, i]) for i in range(6, 9)], -1)[-self.n_interp:]
                if self.clearance is None:
                    hits = self.judge_body(np.concatenate([interp, turn], -1))
                else:                                          # one clearance call in the overlap call's place: its hit is the verdict
                    measured = self.measure_body(np.concatenate([interp, turn], -1))
                    hits, gaps = measured["hit"], measured["distance"]
                    self.body_clearance.append(gaps)
                self.body_hits.append(hits)
            collided, value, where = False, 9999.0, interp[-1]
            for i, p in enumerate(interp):
                collided, v = self.collision(p)
                if v is not None:                              # None: NerfSimulator.py:145's IndexError branch keeps the value
                    value = v
                if hits is not None:                           # the body's verdict; value and position stay the centre's
                    collided = bool(hits[i] >= 0)
                if gaps is not None:                           # the body's gap at the poses the walk visits, capped
                    gap = min(gap, float(min(gaps[i], self.clearance)))
                where = p
                if collided:
                    break
            if gaps is not None:
                value = gap
            rows.append(self.write_row(sim, k, noise, value, where, sigma_d, collided))
            if collided:
                break
        rows = np.asarray(rows, np.float64)
        return np.concatenate([rows, np.full((rows.shape[0], 1), float(rows[:, -1].any()))], 1)   # "ever collided", MonteCarlo.py:112


def simulation_pipeline(sims, in_flight, device):
    """the pipeline.FramePipeline run_simulations runs `sims` on (a context manager), or None when they run one after the other"""
    if in_flight > 1 and len(sims) > 1:
        from .pipeline import FramePipeline
        return FramePipeline(None, in_flight=in_flight, device=device)
    return None


def run_simulations(one, sims, in_flight, device, pipe=None):
    """one(sim) -> (rows, frames) for every simulation of `sims`, `in_flight` at a time, each on its own host thread and HIP stream
    (pipeline.FramePipeline) -> the results in `sims` order.  pipe: a simulation_pipeline() the caller keeps open over several calls
    (cem.run_cem: one for all populations); without it one is opened for this call."""
    if pipe is None:
        pipe = simulation_pipeline(sims, in_flight, device)
        if pipe is not None:
            with pipe:
                return run_simulations(one, sims, in_flight, device, pipe)
        return [one(s) for s in sims]
    futures = [pipe.submit_fn(one, s) for s in sims]
    return [f.result()[0] for f in futures]


def gather_rows(results, n_simulations, steps, width, world_size=1, group=None, device=None, gather=True):
    """this rank's (rows, frames) results -> every simulation's rows [total, width] in simulation order with ONE collective.  Ragged
    (a collision ends a simulation early): every simulation is padded to `steps` rows with NaN for the gather."""
    local = np.full((len(results), steps, width), np.nan, np.float64)
    for i, (rows, _) in enumerate(results):
        local[i, :rows.shape[0]] = rows
    if gather and world_size > 1:
        import torch.distributed as dist
        t = torch.from_numpy(local)
        if dist.get_backend(group) == "nccl":
            t = t.to(device)
        allr = gather_views(t, n_simulations, group).cpu().numpy()
    else:
        allr = local
    flat = allr.reshape(-1, width)
    return flat[~np.isnan(flat[:, 0])]


def run_rollout(model, intrinsics, H, W, n_simulations, steps, seed=0, rank=0, world_size=1, group=None, in_flight=3,
                render_kwargs=None, autocast=True, gather=True, renders_per_step=2, planner_cfg=None, sdf=None, estimator_cfg=None,
                uq_method=UQ_GAUSSIAN, uq_kwargs=None, world=None, body=None, exact=False, clearance=None):
    """Monte-Carlo rollout sharded over ranks.  Returns (rows [total, ROW_WIDTH] float64 in simulation order -- every rank's when
    `gather`, else this rank's -- and a dict of this rank's counters).  planner_cfg: None, or planner_config()'s dict (the
    reference's planner steers every simulation; its initial plan is computed once here).  sdf: None (the analytic stand-in) or
    a collision.SignedDistanceField every simulation's collision check looks up, or "world": the ground-truth field of `world`'s mesh
    (SignedDistanceField.from_mesh over reference_box(), built once here; a ValueError without world=).  estimator_cfg: None, or nav.estimator_config()'s
    dict (with planner_cfg: every simulation's planner replans from the reference's NeRF state estimate; eager estimator steps).
    uq_method / uq_kwargs: RolloutSimulator's (the default is the Gaussian approximation, rows unchanged).  world: None, or the
    world.MeshWorld every simulation's sensor looks at (RolloutSimulator's `world`; shared, read-only).  body / exact: None (the
    centre point's verdict, the rows as they always were) or the collision.BodyBox every simulation's collisions are judged with
    (RolloutSimulator's `body`: against sdf's occupied cells, or with exact=True against world's triangles).  clearance: None, or
    a finite length D > 0 (needs body=): column 14 is the body's gap to the nearest obstacle, capped at D (RolloutSimulator's
    `clearance`), not the centre's field value."""
    from .collision import check_body, check_clearance, resolve_sdf
    sdf = resolve_sdf(sdf, world, "run_rollout")
    check_body(body, exact, sdf, world, "run_rollout")
    check_clearance(clearance, body, "run_rollout")
    device = next(model.parameters()).device
    lo, hi = shard_range(n_simulations, rank, world_size)
    sims = list(range(lo, hi))
    counters = {"frames": 0, "simulations": len(sims), "steps": 0}
    plan0 = initial_plan(model, planner_cfg, seed) if planner_cfg is not None and sims else None

    def one(sim):
        sim_obj = RolloutSimulator(model, intrinsics, H, W, steps, seed=seed, render_kwargs=render_kwargs, renders_per_step=renders_per_step,
                                   planner_cfg=planner_cfg, initial_plan=plan0, sdf=sdf, estimator_cfg=estimator_cfg,
                                   uq_method=uq_method, uq_kwargs=uq_kwargs, world=world, body=body, exact=exact,
                                   clearance=clearance)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            rows = sim_obj.run(sim)
        return rows, sim_obj.frames

    results = run_simulations(one, sims, in_flight, device)
    for rows, frames in results:
        counters["frames"] += frames
        counters["steps"] += rows.shape[0]
    return gather_rows(results, n_simulations, steps, ROW_WIDTH, world_size, group, device, gather), counters


STRESS_MONTE_CARLO, STRESS_CEM = "Monte Carlo", "Cross Entropy Method"     # envConfig.json's stress_test


SIM_NERF, SIM_BLENDER = "NerfSimulator", "BlenderSimulator"               # envConfig.json's simulator


def run_validation(stress_test, *args, simulator=SIM_NERF, **kwargs):
    """validate.py:23-49: envConfig.json's `stress_test` picks the loop -- 'Monte Carlo' -> run_rollout(*args, **kwargs),
    'Cross Entropy Method' -> cem.run_cem(*args, **kwargs); anything else is an error (the reference prints and exits).  `simulator`
    is envConfig.json's key of that name: 'NerfSimulator' (the default: the NeRF is its own world) or 'BlenderSimulator' (the sensor
    looks at the true world: needs world=, a world.MeshWorld); anything else is an error.  With world=, sdf="world" judges the
    collisions of either loop against the mesh's own field, not against the NeRF's; body= (a collision.BodyBox) judges them for the
    drone's body box instead of its centre point (exact=True: against the mesh's triangles), and clearance=D scores them with the
    body's gap to the nearest obstacle instead of the centre's field value."""
    if simulator not in (SIM_NERF, SIM_BLENDER):
        raise ValueError(f"Unrecognized simulator {simulator}")
    if simulator == SIM_BLENDER and kwargs.get("world") is None:
        raise ValueError("run_validation: simulator 'BlenderSimulator' needs world= (a world.MeshWorld: the true world its camera looks at)")
    if stress_test == STRESS_MONTE_CARLO:
        return run_rollout(*args, **kwargs)
    if stress_test == STRESS_CEM:
        from . import cem
        return cem.run_cem(*args, **kwargs)
    raise ValueError(f"Unrecognized stress test {stress_test}")
