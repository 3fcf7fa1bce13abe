"""The trajectory planner of nav/quad_plot.py:10-308: A* initial path, then Adam on the flat states of a quadrotor trajectory
against control effort and the NeRF's density along the drone's body (differential flatness: positions and yaw determine
velocities, rotations, rates and the actions).

Same constructor, attribute names, methods and arithmetic order as the reference, on the device of `start_state` (the reference
sets torch's default tensor type to cuda, validate.py:112), fp32 and outside autocast.  Differences, none of which changes a value:
  * what only writes files or plots is left out: save_poses, save_costs, save_progress, plot, the `basefolder` JSON dumps, the
    prints of a_star_init and get_actions and the per-epoch `print(it, loss)` -- that print is also a host read per epoch;
  * `a_star_init(generator=None)` draws its smoothing noise from `generator` (default: torch's global one, as the reference);
  * next_rotation of the start state is computed once per start state instead of once per calc_everything (its `theta == 0`
    test is a host read), and the constants of calc_everything are built once;
  * get_state_cost takes the world points from the calc_everything it has already run (the reference runs it a second time
    inside body_to_world, to the same values) and drops the unused `point_vels`;
  * with a `density_query` callable whose model has a fused form, the collision term mean_b density_fn(...) ** 2 is ONE HIP
    launch each way (ngp_planner_collision); any other density_fn takes the reference's torch composition;
  * the fused branch computes mean_b(sigma^2) * distance where the reference computes mean_b(sigma^2 * distance): the same
    value up to fp32 rounding (one product per state instead of one per body point), the one change of arithmetic order;
  * with fade_out_epoch <= 0 (envConfig.json: 0, the epoch-dependent mask is dead) and the plan on a GPU, the epochs of
    learn_init / learn_update are replayed from ONE captured HIP graph per call (graphs.GraphedStep): the gradients live in
    preallocated .grad tensors zeroed in place, the pattern of scripts/bench_planner_graph.py.  GraphedStep runs the epoch for
    real while it warms up, so the plan, the initial acceleration and the Adam state are snapshotted before and restored
    after: the plan after N graphed epochs equals the plan after N eager epochs of the same collision path bit for bit.
    cfg['graphs'] = False (or any other fade_out_epoch) runs them eagerly;
  * a captured epoch evaluates the collision term through the composition (density_fn on the world points, i.e. the fused
    per-point density of nerf/network.py), not through ngp_planner_collision: capturing the kernel pair crashes hipGraph
    instantiation (torch.cuda.graph's capture_end) on ROCm 7 / torch 2.10, with .backward() into preallocated gradients as with
    torch.autograd.grad, while the per-point density kernels capture fine; the cause is not found yet.  Eager epochs use the
    kernel pair (cfg['fused_collision'] = False: the composition there too).
"""
import threading

import torch

from .math_utils import rot_matrix_to_vec
from .quad_helpers import astar, next_rotation


_CAPTURE_LOCK = threading.Lock()


class DensityQuery:
    """validate.py:288's density_fn, `model.density(x.reshape((-1, 3)) @ rot)['sigma'].reshape(x.shape[:-1])`, as an object
    the Planner recognises: `collision` evaluates the planner's collision term through the fused HIP kernels when they apply."""

    def __init__(self, model, rot):
        self.model = model
        self.rot = rot

    def __call__(self, x):
        return self.model.density(x.reshape((-1, 3)) @ self.rot)["sigma"].reshape(x.shape[:-1])

    def fused_model(self, body=None):
        """the model's FusedModel when the fused collision term applies: a GPU model with a fused form, `fused` not switched off,
        and nothing but the plan requiring a gradient (map, rot and body frozen); else None"""
        m = self.model
        if not self.rot.is_cuda or not getattr(m, "fused", False) or not hasattr(m, "fused_model"):
            return None
        if self.rot.requires_grad or (body is not None and body.requires_grad):
            return None
        if any(p.requires_grad for p in m.parameters()):
            return None
        return m.fused_model()

    def collision(self, rot_matrix, pos, body):
        """mean_b self(rot_matrix @ body.T + pos[..., None]) ** 2 -> [S] (quad_plot.py:216-241), or None when the fused form does
        not apply (the caller then runs the torch composition)"""
        fm = self.fused_model(body)
        if fm is None:
            return None
        from .._fused import PlannerCollision
        return PlannerCollision.apply(fm, rot_matrix, pos, body, self.rot)


def density_query(model, rot):
    """validate.py:288's density_fn for `model` and the axis permutation `rot` [3,3]; the Planner takes the fused collision kernel
    with it (DensityQuery)"""
    return DensityQuery(model, rot)


class Planner:
    def __init__(self, start_state, end_state, cfg, density_fn):
        self.nerf = density_fn
        self.device = start_state.device
        dev = self.device

        self.cfg                = cfg
        self.T_final            = cfg['T_final']
        self.steps              = cfg['steps']
        self.lr                 = cfg['lr']
        self.epochs_init        = cfg['epochs_init']
        self.epochs_update      = cfg['epochs_update']
        self.fade_out_epoch     = cfg['fade_out_epoch']
        self.fade_out_sharpness = cfg['fade_out_sharpness']
        self.mass               = cfg['mass']
        self.J                  = cfg['I']
        self.g                  = torch.tensor([0., 0., -cfg['g']], device=dev)
        self.body_extent        = cfg['body']
        self.body_nbins         = cfg['nbins']
        # extension: replay the epochs from a captured HIP graph where possible (the plan is the same either way)
        self.use_graphs         = bool(cfg.get('graphs', True))
        # extension: the fused collision kernel for a density_query density_fn in EAGER epochs (captured epochs use the composition)
        self.fused_collision    = bool(cfg.get('fused_collision', True))
        self._capturing         = False

        self.CHURCH = False

        self.dt = self.T_final / self.steps

        self.start_state = start_state
        self.end_state   = end_state
        self._ez = torch.tensor([0, 0, 1.0], device=dev)
        self._next_R, self._next_R_of = None, None

        slider = torch.linspace(0, 1, self.steps, device=dev)[1:-1, None]

        states = (1-slider) * self.full_to_reduced_state(start_state) + \
                    slider  * self.full_to_reduced_state(end_state)

        self.states = states.clone().detach().requires_grad_(True)
        self.initial_accel = torch.tensor([cfg['g'], cfg['g']], device=dev).requires_grad_(True)

        # the shape of the robot body point cloud
        lin = lambda i: torch.linspace(self.body_extent[i, 0], self.body_extent[i, 1], self.body_nbins[i], device=dev)   # noqa: E731
        body = torch.stack(torch.meshgrid(lin(0), lin(1), lin(2), indexing="ij"), dim=-1)
        self.robot_body = body.reshape(-1, 3)

        if self.CHURCH:
            self.robot_body = self.robot_body/2

        self.epoch = 0

    def full_to_reduced_state(self, state):
        pos = state[:3]
        R = state[6:15].reshape((3,3))

        x,y,_ = R @ torch.tensor([1.0, 0, 0], device=state.device)
        angle = torch.atan2(y, x)

        return torch.cat([pos, angle.reshape(1)], dim=-1).detach()

    def a_star_init(self, generator=None):
        """A* through the NeRF's occupancy on a 20^3 grid of [-1, 1]^3, then a smoothed path as the initial states.  The smoothing
        noise comes from `generator` (drawn on its device, then moved to the plan's); None = torch's global generator on the plan's
        device, as the reference."""
        dev = self.device
        side = 100 # grid size

        if self.CHURCH:
            x_linspace = torch.linspace(-2,-1, side, device=dev)
            y_linspace = torch.linspace(-1,0, side, device=dev)
            z_linspace = torch.linspace(0,1, side, device=dev)

            coods = torch.stack(torch.meshgrid(x_linspace, y_linspace, z_linspace, indexing="ij"), dim=-1)
        else:
            linspace = torch.linspace(-1,1, side, device=dev) # extent of the grid
            # side, side, side, 3
            coods = torch.stack(torch.meshgrid(linspace, linspace, linspace, indexing="ij"), dim=-1)

        kernel_size = 5 # 100/5 = 20. scene size of 2 gives a box size of 2/20 = 0.1 = drone size
        output = self.nerf(coods)
        maxpool = torch.nn.MaxPool3d(kernel_size = kernel_size)

        # 20, 20, 20
        occupied = maxpool(output[None,None,...])[0,0,...] > 0.3

        grid_size = side//kernel_size

        # convert to index coordinates
        start_grid_float = grid_size*(self.start_state[:3] + 1)/2
        end_grid_float   = grid_size*(self.end_state  [:3] + 1)/2
        start = tuple(int(start_grid_float[i]) for i in range(3) )
        end =   tuple(int(end_grid_float[i]  ) for i in range(3) )

        path = astar(occupied, start, end)
        self.astar_path = path

        # convert from index coordinates
        squares =  2* (torch.tensor( path, dtype=torch.float, device=dev)/grid_size) -1

        # adding yaw
        states = torch.cat( [squares, torch.zeros( (squares.shape[0], 1), device=dev) ], dim=-1)

        # prevents weird zero derivative issues
        if generator is None:
            randomness = torch.normal(mean= 0, std=0.001*torch.ones(states.shape, device=dev) )
        else:
            randomness = torch.normal(mean=0, std=0.001*torch.ones(states.shape, device=generator.device), generator=generator).to(dev)
        states += randomness

        # smooth path (diagram of which states are averaged)
        # 1 2 3 4 5 6 7
        # 1 1 2 3 4 5 6
        # 2 3 4 5 6 7 7
        prev_smooth = torch.cat([states[0,None, :], states[:-1,:]],        dim=0)
        next_smooth = torch.cat([states[1:,:],      states[-1,None, :], ], dim=0)
        states = (prev_smooth + next_smooth + states)/3

        self.states = states.clone().detach().requires_grad_(True)

    def params(self):
        return [self.initial_accel, self.states]

    def _start_next_R(self, start_R, start_omega):
        """next_rotation of the start state, once per start state (it reads theta == 0 back to the host)"""
        if self._next_R_of is not self.start_state:
            self._next_R = next_rotation(start_R, start_omega, self.dt)
            self._next_R_of = self.start_state
        return self._next_R

    def calc_everything(self):

        start_pos   = self.start_state[None, 0:3]
        start_v     = self.start_state[None, 3:6]
        start_R     = self.start_state[6:15].reshape((1, 3, 3))
        start_omega = self.start_state[None, 15:]

        end_pos   = self.end_state[None, 0:3]
        end_v     = self.end_state[None, 3:6]
        end_R     = self.end_state[6:15].reshape((1, 3, 3))
        end_omega = self.end_state[None, 15:]

        next_R = self._start_next_R(start_R, start_omega)

        # start, next, decision_states, last, end

        start_accel = start_R @ self._ez * self.initial_accel[0] + self.g
        next_accel = next_R @ self._ez * self.initial_accel[1] + self.g

        next_vel = start_v + start_accel * self.dt
        after_next_vel = next_vel + next_accel * self.dt

        next_pos = start_pos + start_v * self.dt
        after_next_pos = next_pos + next_vel * self.dt
        after2_next_pos = after_next_pos + after_next_vel * self.dt

        # position 2 and 3 are unused - but the attached rotations are
        current_pos = torch.cat( [start_pos, next_pos, after_next_pos, after2_next_pos, self.states[2:, :3], end_pos], dim=0)

        prev_pos = current_pos[:-1, :]
        next_pos = current_pos[1: , :]

        current_vel = (next_pos - prev_pos)/self.dt
        current_vel = torch.cat( [ current_vel, end_v], dim=0)

        prev_vel = current_vel[:-1, :]
        next_vel = current_vel[1: , :]

        current_accel = (next_vel - prev_vel)/self.dt - self.g

        # duplicate last acceleration - it is not used for anything (there is no action at the last state)
        current_accel = torch.cat( [ current_accel, current_accel[-1,None,:] ], dim=0)

        accel_mag     = torch.norm(current_accel, dim=-1, keepdim=True)

        # needs to be pointing in direction of acceleration
        z_axis_body = current_accel/accel_mag

        # remove states with rotations already constrained
        z_axis_body = z_axis_body[2:-1, :]

        z_angle = self.states[:,3]

        in_plane_heading = torch.stack( [torch.sin(z_angle), -torch.cos(z_angle), torch.zeros_like(z_angle)], dim=-1)

        x_axis_body = torch.cross(z_axis_body, in_plane_heading, dim=-1)
        x_axis_body = x_axis_body/torch.norm(x_axis_body, dim=-1, keepdim=True)
        y_axis_body = torch.cross(z_axis_body, x_axis_body, dim=-1)

        # S, 3, 3 # assembled manually from basis vectors
        rot_matrix = torch.stack( [x_axis_body, y_axis_body, z_axis_body], dim=-1)

        rot_matrix = torch.cat( [start_R, next_R, rot_matrix, end_R], dim=0)

        current_omega = rot_matrix_to_vec( rot_matrix[1:, ...] @ rot_matrix[:-1, ...].swapdims(-1,-2) ) / self.dt
        current_omega = torch.cat( [ current_omega, end_omega], dim=0)

        prev_omega = current_omega[:-1, :]
        next_omega = current_omega[1:, :]

        angular_accel = (next_omega - prev_omega)/self.dt
        # duplicate last angular acceleration - it is not used for anything (there is no action at the last state)
        angular_accel = torch.cat( [ angular_accel, angular_accel[-1,None,:] ], dim=0)

        # S, 3    3,3      S, 3, 1
        torques = (self.J @ angular_accel[...,None])[...,0]
        actions =  torch.cat([ accel_mag*self.mass, torques ], dim=-1)

        return current_pos, current_vel, current_accel, rot_matrix, current_omega, angular_accel, actions

    def get_full_states(self):
        pos, vel, accel, rot_matrix, omega, angular_accel, actions = self.calc_everything()
        return torch.cat( [pos, vel, rot_matrix.reshape(-1, 9), omega], dim=-1 )

    def get_actions(self):
        pos, vel, accel, rot_matrix, omega, angular_accel, actions = self.calc_everything()
        return actions

    def get_next_action(self):
        actions = self.get_actions()
        # fz, tx, ty, tz
        return actions[0, :]

    @staticmethod
    def _to_world(rot_matrix, pos, points):
        # S, 3, P    =    S,3,3       3,P       S, 3, _
        world_points =  rot_matrix @ points.T + pos[..., None]
        return world_points.swapdims(-1,-2)

    def body_to_world(self, points):
        pos, vel, accel, rot_matrix, omega, angular_accel, actions = self.calc_everything()
        return self._to_world(rot_matrix, pos, points)

    def get_state_cost(self):
        pos, vel, accel, rot_matrix, omega, angular_accel, actions = self.calc_everything()

        fz = actions[:, 0]
        torques = torch.norm(actions[:, 1:], dim=-1)

        # S
        distance = torch.sum( vel**2 + 1e-5, dim = -1)**0.5

        use_kernel = isinstance(self.nerf, DensityQuery) and self.fused_collision and not self._capturing
        collision = self.nerf.collision(rot_matrix, pos, self.robot_body) if use_kernel else None
        if collision is not None:
            # S = mean_b density (one launch each way), times distance
            colision_prob = collision * distance
        else:
            # S, B
            density = self.nerf( self._to_world(rot_matrix, pos, self.robot_body) )**2

            # multiplied by distance to prevent it from just speed tunnelling
            # S =   S,B * S,_
            colision_prob = torch.mean(density * distance[:,None], dim = -1)

        if self.epoch < self.fade_out_epoch:
            t = torch.linspace(0,1, colision_prob.shape[0], device=colision_prob.device)
            position = self.epoch/self.fade_out_epoch
            mask = torch.sigmoid(self.fade_out_sharpness * (position - t))
            colision_prob = colision_prob * mask

        # cost function shaping
        return 1000*fz**2 + 0.01*torques**4 + colision_prob * 1e6, colision_prob*1e6

    def total_cost(self):
        total_cost, colision_loss  = self.get_state_cost()
        return torch.mean(total_cost)

    # ---- optimisation -----------------------------------------------------------------------------------------------------
    def _epoch(self, opt, it):
        opt.zero_grad()
        self.epoch = it
        loss = self.total_cost()
        loss.backward()
        opt.step()
        return loss

    def graphable(self):
        """whether the epochs replay from a captured graph: enabled, the plan on a GPU, no epoch-dependent fade-out mask"""
        return self.use_graphs and self.states.is_cuda and self.fade_out_epoch <= 0

    def _run_epochs(self, opt, n):
        if n <= 0:
            return
        if not self.graphable():
            for it in range(n):
                self._epoch(opt, it)
            return
        from ..graphs import GraphedStep
        params = self.params()
        saved = [p.detach().clone() for p in params]
        saved_state = {p: ({k: v.clone() for k, v in opt.state[p].items() if isinstance(v, torch.Tensor)} if p in opt.state else None)
                       for p in params}
        for p in params:
            p.grad = torch.zeros_like(p)

        def epoch():
            for p in params:
                p.grad.zero_()
            loss = self.total_cost()
            loss.backward()
            opt.step()
            return loss

        # one capture at a time in the process; other threads (simulations in flight) may keep launching meanwhile
        # the collision kernel pair stays out of the graph (see the module docstring): warm-up and capture take the composition
        self._capturing = True
        try:
            with _CAPTURE_LOCK:
                step = GraphedStep(epoch, (), device=self.device, capture_error_mode="thread_local")
        finally:
            self._capturing = False
        # the warm-up ran real epochs: put the plan and the optimiser back where they were
        with torch.no_grad():
            for p, v in zip(params, saved):
                p.copy_(v)
            for p in params:
                before = saved_state[p]
                for k, v in opt.state[p].items():
                    if isinstance(v, torch.Tensor):
                        if before is None:
                            v.zero_()          # = what a fresh Adam creates on its first step: step 0, zero moments
                        else:
                            v.copy_(before[k])
        for _ in range(n):
            step()
        self.epoch = n - 1
        del step

    def learn_init(self):
        opt = torch.optim.Adam(self.params(), lr=self.lr, capturable=True)
        self._run_epochs(opt, self.epochs_init)

    def learn_update(self, iteration):
        opt = torch.optim.Adam(self.params(), lr=self.lr, capturable=True)
        self._run_epochs(opt, self.epochs_update)

    def update_state(self, measured_state):
        pos, vel, accel, rot_matrix, omega, angular_accel, actions = self.calc_everything()

        self.start_state = measured_state
        self.states = self.states[1:, :].detach().requires_grad_(True)
        self.initial_accel = actions[1:3, 0].detach().requires_grad_(True)
