"""Failure replay: the disturbances a stress test recorded, fed to the TRUE world (DESIGN.md "Failure replay").

The reference's pipeline has three stages: a stress test (rollout.run_rollout, cem.run_cem) searches for disturbance sequences that
crash the drone in the NeRF; validation/utils/replay/replay_MC.py / replay_CEM.py feed exactly those disturbances to the
BlenderSimulator -- the true world's camera and the true world's collision field; and the replay counts, per step and per trajectory,
how often the NeRF's verdict and the true world's agree.  The two confusion matrices are its product.  Every replayed trajectory is
also handed to Blender (runBlenderOnFailure -> validation/utils/viz_failures_blend.py) to be drawn into the scene.  This module is
that second and third stage without Blender: the world is a world.MeshWorld, its collision field SignedDistanceField.from_mesh, and
the drawing is MeshWorld.render_scene (csrc/overlay.hip).

    ReplaySimulator(RolloutSimulator)       one replayed simulation: recorded noise, the world as the only sensor, the replay row
    run_replay(rows, model, ...)            replay_MC / replay_CEM -> ReplayResult (rows, counts, views)
    ReplayCounts / ConfusionCounts          tp, tn, fp, fn per step and per trajectory; replaces the reference's counts.pkl
    failure_view(world, sim_rows, plans)    the picture of one replayed simulation (failure_primitives: viz_failures_blend.py's geometry)
    read_results_csv / write_replay_csv     the reference's results/*.csv in, collisionValuesReplay.csv out

The counting (replay_MC.py:105-128), kept exactly, with `world` the replay's verdict and `nerf` the recorded one:
    per step         tp += world and nerf;  fn += world and not nerf;  fp += not world and nerf;  tn += not world and not nerf
    THE QUIRK        a collision in the world ends the replayed simulation, and ALL its remaining recorded steps are added to fn,
                     whatever the NeRF said on them (:112-118).  It is the reference's bookkeeping and is not "fixed" here.
    per trajectory   the same four cells from "ever collided" in the replay against the recorded last column of the simulation's
                     last row
A step the NeRF flagged after the world's collision is therefore a false negative, and a recorded simulation is never longer than its
first NeRF collision, so in practice the remaining steps are those the NeRF called free.

Not ported: the seaborn heat map (ReplayResult.confusion_matrix is its data), the .blend output (the view is a PNG), counts.pkl
(pass `counts=` to continue) and sharding over ranks.
"""
import csv
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import rollout as RO
from .collision import PLANNER_ROT, SDF_WORLD, check_body, reference_box, resolve_sdf, to_nerf

REPLAY_ROW_WIDTH = 22       # replay_MC.py:81-103,134: sim, step, noise x12, collision value, xyz, step loglik, cumulative loglik, collided (+ ever collided)
REPLAY_CEM_ROW_WIDTH = 23   # replay_CEM.py:142: the population in front
TUBE_RADIUS = 0.02          # blenderUtils.py:22 / viz_failures_blend.py:29: bevel_depth
CUBE_HALF = 0.0125          # viz_failures_blend.py:55: add_cube's scale of a size-2 cube
PATH_RADIUS = CUBE_HALF / 2 # the flown path's tube (no counterpart in the reference): thinner than the cubes it threads, so that they show
# failure_view's colours
COLOR_INITIAL_PLAN = (0.10, 0.30, 0.90)                    # blue
COLOR_REPLAN_FIRST, COLOR_REPLAN_LAST = (1.00, 0.85, 0.10), (0.90, 0.15, 0.10)     # yellow at time step 0 -> red at the last
COLOR_FLOWN_PATH = (0.10, 0.65, 0.20)                      # green
COLOR_CUBE = (0.10, 0.10, 0.10)                            # near black
COLOR_CUBE_COLLIDED = (0.90, 0.10, 0.80)                   # magenta


@dataclass
class ConfusionCounts:
    """one confusion matrix's cells; the world is the truth, the NeRF the prediction"""
    tp: int = 0
    tn: int = 0
    fp: int = 0
    fn: int = 0

    def add(self, world, nerf):
        world, nerf = bool(world), bool(nerf)
        self.tp += int(world and nerf)
        self.fn += int(world and not nerf)
        self.fp += int(not world and nerf)
        self.tn += int(not world and not nerf)

    @property
    def total(self):
        return self.tp + self.tn + self.fp + self.fn

    def matrix(self):
        """the reference's layout (replay_MC.py:153): [[tn, fn], [fp, tp]] -- rows: NeRF False / True, columns: world False / True"""
        return np.array([[self.tn, self.fn], [self.fp, self.tp]], dtype=np.int64)


@dataclass
class ReplayCounts:
    """the eight counts of a replay (the content of the reference's counts.pkl): per step and per trajectory"""
    step: ConfusionCounts = field(default_factory=ConfusionCounts)
    traj: ConfusionCounts = field(default_factory=ConfusionCounts)

    def copy(self):
        return ReplayCounts(ConfusionCounts(**vars(self.step)), ConfusionCounts(**vars(self.traj)))


def count_simulation(counts, world_flags, nerf_step_flags, nerf_ever):
    """replay_MC.py:105-128 for one simulation: world_flags, the replay's step verdicts (as many as it ran: a collision ends it);
    nerf_step_flags, the recorded step verdicts (all recorded steps); nerf_ever, the recorded trajectory verdict.  Adds to `counts`."""
    ever = False
    for k, w in enumerate(world_flags):
        counts.step.add(w, nerf_step_flags[k])
        if w:
            ever = True
            counts.step.fn += len(nerf_step_flags) - k - 1          # the quirk: the remaining steps, whatever the NeRF said
            break
    counts.traj.add(ever, nerf_ever)
    return ever


def replay_log_likelihood(noise, mean, std):
    """replay_MC.py:144-148 (trajectoryLikelihood): the sum of log N(noise; mean, std), float64.  The replay's copy of the function has
    NO clip of the densities, unlike MonteCarlo.py:33 -- it is rollout.trajectory_log_likelihood wherever every density lies in 1e-8 ..
    1e8, and differs from it on the far-out noise a refitted CEM proposal draws (the reference's own replay rows show it)."""
    noise, mean, std = [np.asarray(a, np.float64) for a in (noise, mean, std)]
    with np.errstate(divide="ignore"):
        return float((-0.5 * ((noise - mean) / std) ** 2 - np.log(std * np.sqrt(2 * np.pi))).sum())


class ReplaySimulator(RO.RolloutSimulator):
    """One replayed simulation (replay_MC.py:70-103 around BlenderSimulator.step): RolloutSimulator's step with the RECORDED noise,
    the world's frame as the only observation and the replay row.  noises: float32 [n, 12], the recorded rows' noise columns -- the
    simulation has exactly n steps (a collision in the replay ends it earlier).  steps: the STRESS run's step count (its dt).
    population: None (Monte Carlo) or the CEM population the row starts with.  With planner_cfg, self.plans holds the plan's
    positions (Planner.get_full_states()[:, :3], numpy [S, 3], the planner's world frame) after reset and after every replan."""

    def __init__(self, *args, noises=None, population=None, **kwargs):
        super().__init__(*args, **kwargs)
        if self.world is None:
            raise ValueError("ReplaySimulator: world= is required (the true world the recorded disturbances are replayed in)")
        self.noises = torch.from_numpy(np.ascontiguousarray(noises, np.float32).reshape(-1, 12))
        self.steps = int(self.noises.shape[0])               # (dt keeps the stress run's steps: set by the base class above)
        self.population = population
        self.plans = []

    def begin(self, sim):
        self._cumulative = 0.0

    def draw_noise(self, sim, k):
        return self.noises[k]

    def observe(self, pose):
        """BlenderSimulator.step's sensing (:82,102): the world's frame of the true pose, the estimator's sensor image when there is
        one.  No NeRF render for an uncertainty and no UQ (BlenderSimulator.step has none) -> NaN for the unused sigma."""
        with torch.no_grad():
            self.world_image = self.world.render(pose, self.intrinsics, self.H, self.W)["image_u8"].cpu().numpy()
        if self.estimator is not None:
            self.sensor_image = self.world_image
        return float("nan")

    def _keep_plan(self):
        if self.planner is not None:
            with torch.no_grad(), torch.autocast("cuda", enabled=False):
                self.plans.append(self.planner.get_full_states()[:, :3].detach().cpu().numpy().copy())

    def reset_planner(self):
        super().reset_planner()
        self.plans = []
        self._keep_plan()

    def replan(self, k, state):
        super().replan(k, state)
        self._keep_plan()

    def write_row(self, sim, k, noise, value, where, sigma_d, collided):
        """replay_MC.py:81-103: the log-likelihood against the unwidened mean / std (replay_log_likelihood)"""
        loglik = replay_log_likelihood(noise.numpy(), self.mean.numpy(), self.std.numpy())
        self._cumulative += loglik
        return [sim, k, *noise.tolist(), value, *where.tolist(), loglik, self._cumulative, float(collided)]

    def run(self, sim):
        rows = super().run(sim)
        if self.population is not None:                      # replay_CEM.py:142
            rows = np.concatenate([np.full((rows.shape[0], 1), float(self.population)), rows], 1)
        return rows


@dataclass
class ReplayResult:
    """rows: float64 [total, REPLAY_ROW_WIDTH or REPLAY_CEM_ROW_WIDTH] in (population,) simulation order; counts: ReplayCounts
    (including what `counts=` brought in); views: the PNG paths run_replay(views=dir) wrote, one per simulation (else empty);
    view_calls: (simulation, step, population or None) per replayed simulation, in order -- runBlenderOnFailure's arguments;
    plans: per replayed simulation ReplaySimulator.plans (empty lists without a planner)."""
    rows: np.ndarray
    counts: ReplayCounts
    views: list = field(default_factory=list)
    view_calls: list = field(default_factory=list)
    plans: list = field(default_factory=list)

    def _cells(self, kind):
        if kind not in ("step", "traj"):
            raise ValueError(f"ReplayResult: kind is 'step' or 'traj' (got {kind!r})")
        return getattr(self.counts, kind)

    def confusion_matrix(self, kind):
        """[[tn, fn], [fp, tp]] (rows: NeRF False / True; columns: world False / True): createConfusionMatrix's array"""
        return self._cells(kind).matrix()

    def labels(self, kind):
        """(y_true, y_pred): 0 / 1 vectors expanded from the counts, the world as truth; order tp, fn, fp, tn"""
        c = self._cells(kind)
        y_true = np.repeat([1, 1, 0, 0], [c.tp, c.fn, c.fp, c.tn])
        y_pred = np.repeat([1, 0, 1, 0], [c.tp, c.fn, c.fp, c.tn])
        return y_true, y_pred

    def scores(self, kind):
        """accuracy, precision, recall and F1 of the matrix (uncertainty/evaluation/metrics.py; an empty denominator is numpy's NaN)"""
        from .uncertainty.evaluation import metrics as M
        y_true, y_pred = self.labels(kind)
        return {"accuracy": M.calculate_accuracy(y_true, y_pred), "precision": M.calculate_precision(y_true, y_pred),
                "recall": M.calculate_recall(y_true, y_pred), "f1": M.calculate_f1_score(y_true, y_pred)}


def group_rows(rows):
    """a stress test's rows -> (cem, {population or None: {simulation: (noises float32 [n,12], step flags bool [n], ever collided
    bool)}}), simulations and populations in order of first appearance.  Width ROW_WIDTH (run_rollout): noise columns 2:14; width
    cem.CEM_ROW_WIDTH (run_cem): population first, noise columns 3:15; the NeRF's verdicts are the last two columns (replay_*.py:57/63).
    The noise is the columns cast to float32 (replay_MC.py:52)."""
    from .cem import CEM_ROW_WIDTH
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 2 or rows.shape[1] not in (RO.ROW_WIDTH, CEM_ROW_WIDTH):
        raise ValueError(f"run_replay: rows are run_rollout's (width {RO.ROW_WIDTH}) or run_cem's (width {CEM_ROW_WIDTH}), got shape {rows.shape}")
    cem = rows.shape[1] == CEM_ROW_WIDTH
    off = 1 if cem else 0
    data = {}
    for r in rows:
        pop = int(r[0]) if cem else None
        sims = data.setdefault(pop, {})
        sims.setdefault(int(r[off]), []).append(r)
    out = {}
    for pop, sims in data.items():
        out[pop] = {}
        for s, rs in sims.items():
            rs = np.stack(rs)
            out[pop][s] = (rs[:, 2 + off:14 + off].astype(np.float32), rs[:, -2] != 0, bool(rs[-1, -1] != 0))
    return cem, out


def run_replay(rows, model, intrinsics, H, W, *, world, sdf=SDF_WORLD, seed=0, planner_cfg=None, estimator_cfg=None, render_kwargs=None,
               in_flight=3, autocast=True, start=0, start_k=0, counts=None, views=None, steps=None, body=None, exact=False):
    """replay_MC / replay_CEM: every recorded simulation of `rows` again, with its recorded noise, in the true world -> ReplayResult.

    rows: run_rollout's array (width ROW_WIDTH) or run_cem's (width CEM_ROW_WIDTH); any other width is a ValueError.
    world: the world.MeshWorld the sensor looks at, REQUIRED.  sdf: "world" (the default: the mesh's own field,
    SignedDistanceField.from_mesh over reference_box(), built once here through collision.resolve_sdf), or a
    collision.SignedDistanceField -- e.g. the reference's sdf.npy through from_array -- or None (the analytic stand-in).
    model: the NeRF the planner and the estimator use; may be None when neither is asked for: then the NeRF renders nothing.
    seed, planner_cfg and estimator_cfg MUST BE THOSE OF THE STRESS RUN, so that the world is the only thing that differs between the
    two runs.  With planner_cfg the initial plan is computed once per replay and copied into every simulation, as run_rollout does.
    steps: the stress run's `steps` (what its dt was made from); default: planner_cfg's, else the largest number of recorded rows of a
    simulation (right whenever one simulation ran to its end).
    The simulations are independent and run through rollout.run_simulations, `in_flight` at a time, each on its own stream; one rank.
    start / start_k: the reference's start_iter / start_k -- simulations start.., populations start_k.. (by position: range(start,
    number of simulations), as the reference indexes them).  Its quirk is kept: `start` skips the first simulations of EVERY
    population (replay_CEM.py:77), not only of the resumed one.
    counts: a ReplayCounts to continue from (it is not modified); it replaces the reference's counts.pkl, no pickle file is written.
    views: None, or a directory: one PNG per replayed simulation -- also those that did not collide, as replay_MC.py:119-121 -- named
    failure_{sim}_{step}.png, with {population}_ in front of {sim} for CEM rows (viz_failures_blend.py:108-111); step is the
    colliding step, or the last one; the picture is failure_view's default overview at the frame size H x W.  The counting follows the module docstring, quirk included.
    body / exact: None, or the collision.BodyBox the replay's verdicts are judged with (RolloutSimulator's `body`: against the field's
    occupied cells, or with exact=True against the world's triangles).  It applies to both verdicts of a confusion matrix: the world's
    is judged here; the NeRF's is the recorded one, so `rows` must come from a stress run with the SAME body (like seed, planner_cfg
    and estimator_cfg) for the matrices to compare like with like."""
    from .world import MeshWorld
    cem, data = group_rows(rows)
    if world is None:
        raise ValueError("run_replay: world= is required (a world.MeshWorld: the true world the recorded disturbances are replayed in)")
    if isinstance(sdf, str) and sdf == SDF_WORLD and not isinstance(world, MeshWorld):
        raise ValueError(f"run_replay: sdf={SDF_WORLD!r} needs a world.MeshWorld (the mesh the ground-truth field is built from)")
    if model is None and (planner_cfg is not None or estimator_cfg is not None):
        raise ValueError("run_replay: the planner and the estimator need the NeRF (model=)")
    sdf = resolve_sdf(sdf, world, "run_replay")
    check_body(body, exact, sdf, world, "run_replay")
    device = next(model.parameters()).device if model is not None else getattr(world, "device", torch.device("cpu"))

    def by_position(table, first, what):
        for i in range(first, len(table)):                   # the reference's range(start, len(...)) over keys it assumes are 0..n-1
            if i not in table:
                raise ValueError(f"run_replay: {what} {i} is not among the recorded {sorted(k for k in table)} (the reference indexes by position)")
            yield i

    if cem:
        tasks = [(k, s) for k in by_position(data, int(start_k), "population") for s in by_position(data[k], int(start), "simulation")]
    else:
        tasks = [(None, s) for s in by_position(data.get(None, {}), int(start), "simulation")]
    if steps is None:
        steps = planner_cfg["steps"] if planner_cfg is not None else max([len(data[k][s][0]) for k, s in tasks], default=1)
    plan0 = RO.initial_plan(model, planner_cfg, seed) if planner_cfg is not None and tasks else None

    def one(task):
        pop, s = task
        sim = ReplaySimulator(model, intrinsics, H, W, int(steps), seed=seed, render_kwargs=render_kwargs, planner_cfg=planner_cfg,
                              initial_plan=plan0, sdf=sdf, estimator_cfg=estimator_cfg, world=world, body=body, exact=exact, noises=data[pop][s][0],
                              population=pop)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast and device.type == "cuda"):
            out = sim.run(s)
        return (out, sim.plans), sim.frames

    results = RO.run_simulations(one, tasks, in_flight if device.type == "cuda" else 1, device)
    total = (counts or ReplayCounts()).copy()
    result = ReplayResult(rows=np.zeros((0, REPLAY_CEM_ROW_WIDTH if cem else REPLAY_ROW_WIDTH)), counts=total)
    all_rows = []
    if views is not None:
        os.makedirs(views, exist_ok=True)
    for (pop, s), ((sim_rows, plans), _) in zip(tasks, results):
        _, nerf_steps, nerf_ever = data[pop][s]
        count_simulation(total, sim_rows[:, -2] != 0, nerf_steps, nerf_ever)
        step = int(sim_rows[-1, 2 if cem else 1])            # the colliding step, or the last one (replay_MC.py:116,121)
        result.view_calls.append((s, step, pop))
        result.plans.append(plans)
        all_rows.append(sim_rows)
        if views is not None:
            from PIL import Image
            name = f"failure_{s}_{step}.png" if pop is None else f"failure_{pop}_{s}_{step}.png"
            image = failure_view(world, sim_rows, plans or None, H=H, W=W)["image_u8"]
            Image.fromarray(np.ascontiguousarray(image.cpu().numpy() if isinstance(image, torch.Tensor) else image)).save(os.path.join(views, name))
            result.views.append(os.path.join(views, name))
    if all_rows:
        result.rows = np.concatenate(all_rows, 0)
    return result


# ------------------------------------------------------------------------------------------------------------- the failure view
def _row_layout(width):
    """-> (first position column, step-collided column) of a replay row (22 / 23 wide) or a stress row (24 / 27: viz_failures_blend.py:99)"""
    from .cem import CEM_ROW_WIDTH
    if width in (REPLAY_ROW_WIDTH, RO.ROW_WIDTH):
        return 15, width - 2
    if width == REPLAY_CEM_ROW_WIDTH:
        return 16, width - 2
    if width == CEM_ROW_WIDTH:
        return 18, width - 2
    raise ValueError(f"failure_view: rows of width {width} are neither replay rows nor a stress test's")


def overview_camera(H, W):
    """the default camera of failure_view: it looks at the centre of collision.reference_box() (turned into the NeRF's axes) from
    above and beside it -- the direction (0.55, 0.7, 0.45) in the NeRF's axes, whose y is the world's up -- at 1.6 times the box's
    half diagonal, through scene.look_at_poses; focal length = W (a 53 degree field of view) -> (pose [4,4] float32, intrinsics)"""
    from .scene import look_at_poses
    box = reference_box()
    lo = np.asarray(box.start, np.float64)
    hi = lo + np.asarray(box.shape, np.float64) / box.granularity
    centre = to_nerf(torch.from_numpy((lo + hi) / 2)[None], PLANNER_ROT)[0].numpy()
    direction = np.array([0.55, 0.7, 0.45])
    pose = look_at_poses((direction / np.linalg.norm(direction) * 1.6 * np.linalg.norm(hi - lo) / 2)[None])[0]
    pose[:3, 3] += centre
    return pose.astype(np.float32), np.array([float(W), float(W), W / 2.0, H / 2.0])


def failure_primitives(sim_rows, plans=None):
    """viz_failures_blend.py's geometry of one simulation in the mesh's axes -> (tubes, boxes) as MeshWorld.render_scene takes them.
    sim_rows: the simulation's rows (replay rows, or a stress test's); plans: ReplaySimulator.plans, or None without a planner.
    The initial plan and the latest plan of every time step are tubes of radius 0.02 (bevel_depth), every step's recorded position a
    cube of half extent 0.0125 (add_cube's scale); without a planner the flown path itself (start position, then the recorded
    positions) is the tube -- of radius 0.00625, half the cubes' half extent: it threads the cubes, and a 0.02 tube would swallow them.
    Positions are in the planner's world frame and go through collision.to_nerf(., PLANNER_ROT) into the mesh's axes."""
    sim_rows = np.asarray(sim_rows, np.float64)
    if sim_rows.ndim != 2 or sim_rows.shape[0] == 0:
        raise ValueError("failure_view: the rows of one simulation, at least one")
    first, flag = _row_layout(sim_rows.shape[1])
    nerf = lambda p: to_nerf(torch.as_tensor(np.asarray(p, np.float32)).reshape(-1, 3), PLANNER_ROT).numpy()
    positions = nerf(sim_rows[:, first:first + 3])
    collided = sim_rows[:, flag] != 0
    tubes = []
    if plans:
        tubes.append((nerf(plans[0]), TUBE_RADIUS, COLOR_INITIAL_PLAN))
        n = len(plans) - 1
        for i, plan in enumerate(plans[1:]):
            w = i / (n - 1) if n > 1 else 0.0
            rgb = tuple((1 - w) * a + w * b for a, b in zip(COLOR_REPLAN_FIRST, COLOR_REPLAN_LAST))
            tubes.append((nerf(plan), TUBE_RADIUS, rgb))
    else:
        tubes.append((np.concatenate([nerf(RO.ENV["start_pos"]), positions]), PATH_RADIUS, COLOR_FLOWN_PATH))
    boxes = []
    for mask, rgb in ((~collided, COLOR_CUBE), (collided, COLOR_CUBE_COLLIDED)):
        if mask.any():
            boxes.append((positions[mask], (CUBE_HALF,) * 3, rgb))
    return tubes, boxes


def failure_view(world, sim_rows, plans=None, pose=None, intrinsics=None, H=400, W=400):
    """The picture of one replayed simulation in the true world, in the place of runBlenderOnFailure -> viz_failures_blend.py ->
    MeshWorld.render_scene's dict (image, image_u8, depth, prim, overlay_prim) of failure_primitives(sim_rows, plans).
    Colours: the initial plan blue (0.10, 0.30, 0.90); the replans from yellow (1.00, 0.85, 0.10) at time step 0 to red (0.90, 0.15,
    0.10) at the last, linearly; the flown path green (0.10, 0.65, 0.20); the cubes near black (0.10, 0.10, 0.10), the cube of a
    colliding step magenta (0.90, 0.10, 0.80).
    pose / intrinsics: the camera (cam2world, (fx, fy, cx, cy)); default overview_camera(H, W), an overview of reference_box()."""
    tubes, boxes = failure_primitives(sim_rows, plans)
    if pose is None or intrinsics is None:
        cam, K = overview_camera(H, W)
        pose = cam if pose is None else pose
        intrinsics = K if intrinsics is None else intrinsics
    return world.render_scene(pose, intrinsics, H, W, tubes=tubes, boxes=boxes)


# ------------------------------------------------------------------------------------------------------------- CSV in and out
def _cell(text):
    t = text.strip()
    if t.upper() == "TRUE":                                  # (compared case-insensitively, as replay_MC.py:106)
        return 1.0
    if t.upper() == "FALSE":
        return 0.0
    return float(t)


def read_results_csv(path):
    """the reference's results/*.csv (MonteCarlo.py / CrossEntropyMethod.py write booleans as True / False) or one with numeric flags
    -> float64 [rows, width]; every row must have the same width"""
    with open(path, newline="") as fh:
        rows = [[_cell(v) for v in r] for r in csv.reader(fh) if r]
    if not rows:
        return np.zeros((0, 0), np.float64)
    if len({len(r) for r in rows}) != 1:
        raise ValueError(f"read_results_csv: {path} has rows of different widths")
    return np.asarray(rows, np.float64)


def write_replay_csv(result, path):
    """collisionValuesReplay.csv's columns (replay_MC.py:130-135): the integer columns as integers, the two flags as True / False,
    every other value as repr(float) -- read_results_csv gives result.rows back exactly"""
    rows = result.rows if isinstance(result, ReplayResult) else np.asarray(result, np.float64)
    ints = 3 if rows.shape[1] == REPLAY_CEM_ROW_WIDTH else 2
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        for r in rows:
            w.writerow([int(v) for v in r[:ints]] + [repr(float(v)) for v in r[ints:-2]] + [bool(r[-2]), bool(r[-1])])
