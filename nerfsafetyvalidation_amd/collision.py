"""The rollout's signed distance field (validation/simulators/NerfSimulator.py:55-61,131-147), built from the NeRF on the GPU.

The reference builds its collision field offline in two steps: validation/utils/createCollisionMap.py marks, in Blender, the
1/40 m cells of a box that hold a mesh vertex, and validation/utils/createSDF.py turns that map into
`scipy.ndimage.distance_transform_edt(~map) / 40`, the distance in metres from every cell to the nearest occupied one.  A user of
this project has a trained NeRF, not a Blender scene, so the map comes from the model's own density instead:

    occupancy_from_density   max sigma over s^3 points of every cell > thresh    ngp_cell_max_density (HIP)
    occupancy_from_points    createCollisionMap.py:43-53 for any point cloud      numpy
    occupancy_from_fn        a host-side analytic scene (the synthetic henge)     numpy
    occupancy_from_mesh      every cell a triangle of the world's mesh touches    ngp_voxelize_* (HIP); numpy for a CPU world
    SignedDistanceField.from_occupancy   exact squared EDT in integers            ngp_edt_sq (HIP), then sqrt in float64 / granularity

`occupancy_from_mesh` (world.MeshWorld.occupancy, a conservative surface voxelisation) is the ground truth: the reference's map comes
from the scene's mesh too, and a model must not mark its own homework.  `SignedDistanceField.from_mesh` is the field of that map, what
`sdf="world"` resolves to in rollout.run_rollout / cem.run_cem; `map_agreement` scores a NeRF-density map against it.

`from_occupancy` reproduces createSDF.py bit for bit: scipy also takes the float64 square root of an exact integer sum of squares.
`lookup` is NerfSimulator's host check of one point; `query` the same index rule as a batched device gather.

Boxes: NerfSimulator looks values up with its own constants (`reference_box()`, shape (96, 92, 24)) while createCollisionMap.py
builds the map over a different box (`collision_map_box()`, shape (72, 96, 56)).  The reference therefore indexes a (72, 96, 56)
field with the start and granularity of the other box; `SignedDistanceField.from_array(sdf, reference_box())` reproduces that
("The collision field").
"""
import numpy as np
import torch

from . import _lib
from .scene import henge_occupancy

PLANNER_ROT = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]    # rollout.PLANNER_ROT: world (Blender) -> NeRF axes


class GridBox:
    """An axis-aligned box of cubic cells: `start` [3] (metres, world frame), `granularity` (cells per metre), `shape` (X, Y, Z)."""

    def __init__(self, start, granularity, shape):
        self.start = tuple(float(v) for v in start)
        self.granularity = float(granularity)
        self.shape = tuple(int(n) for n in shape)
        if len(self.start) != 3 or len(self.shape) != 3:
            raise ValueError("GridBox: start and shape have three entries")

    @classmethod
    def from_range(cls, start, end, granularity):
        """the reference's box definition: shape[d] = worldToIndex(end[d], start[d], granularity)"""
        return cls(start, granularity, cls(start, granularity, (0, 0, 0)).world_to_index(end))

    def world_to_index(self, w):
        """validation/utils/blenderUtils.py:15-16 per axis: int(np.floor((w - start) * granularity)) in float64"""
        return tuple(int(np.floor((float(w[d]) - self.start[d]) * self.granularity)) for d in range(3))

    def indices(self, points):
        """world_to_index of points [..., 3] (float64 arithmetic) -> int64 [..., 3]"""
        p = np.asarray(points, np.float64)
        return np.stack([np.floor((p[..., d] - self.start[d]) * self.granularity) for d in range(3)], -1).astype(np.int64)

    def sample_points(self, a, b, c, samples_per_axis, device="cpu"):
        """world points [X, Y, Z, 3] float32 of sub-sample (a, b, c) of every cell, in ngp_cell_max_density's arithmetic:
        start + (cell + (sub + 0.5) / s) / granularity, each operation one fp32 IEEE rounding (the divisors are tensors: torch divides
        by a host scalar through its reciprocal)"""
        f32 = dict(dtype=torch.float32, device=device)
        s = torch.tensor([float(samples_per_axis)], **f32)
        g = torch.tensor([self.granularity], **f32)
        axes = []
        for d, sub in enumerate((a, b, c)):
            cell = torch.arange(self.shape[d], **f32)
            off = (torch.tensor([float(sub)], **f32) + 0.5) / s
            axes.append(torch.tensor([self.start[d]], **f32) + (cell + off) / g)
        gx, gy, gz = torch.meshgrid(*axes, indexing="ij")
        return torch.stack([gx, gy, gz], -1)

    def __eq__(self, other):
        return isinstance(other, GridBox) and (self.start, self.granularity, self.shape) == (other.start, other.granularity, other.shape)

    def __repr__(self):
        return f"GridBox(start={self.start}, granularity={self.granularity}, shape={self.shape})"


def reference_box():
    """NerfSimulator's lookup constants (NerfSimulator.py:55-61): START (-1.4, -1.3, -0.1), END (1, 1, 0.5), 40 cells/m"""
    return GridBox.from_range((-1.4, -1.3, -0.1), (1.0, 1.0, 0.5), 40)


def collision_map_box():
    """the box createCollisionMap.py:18-23 builds its map over: START (-1.2, -1.2, -0.22), END (0.6, 1.2, 1.2), 40 cells/m"""
    return GridBox.from_range((-1.2, -1.2, -0.22), (0.6, 1.2, 1.2), 40)


def to_nerf(points, rot):
    """world points [..., 3] -> the NeRF's axes as plan_point / ngp_cell_max_density form them: x[j] = (w0 r0j + w1 r1j) + w2 r2j"""
    r = torch.as_tensor(rot, dtype=points.dtype).to(points.device).reshape(3, 3)
    return points[..., 0:1] * r[0] + points[..., 1:2] * r[1] + points[..., 2:3] * r[2]


# ------------------------------------------------------------------ occupancy sources: bool [X, Y, Z]
def cell_max_density(model, box, samples_per_axis=2, rot=PLANNER_ROT, chunk_points=1 << 22):
    """the largest raw sigma over samples_per_axis^3 points of every cell of `box` -> float32 [X, Y, Z] on the model's device.
    Through ngp_cell_max_density when the model has a fused form in the current autocast context (fp32 network outside autocast,
    fp16 under it; each sigma bit-identical to ngp_network_density's on the same point).  Otherwise chunked
    `model.density(x @ rot)` on the same fp32 points: not bit-identical (the model's own kernels or operators evaluate it)."""
    s = int(samples_per_axis)
    if s < 1:
        raise ValueError("samples_per_axis must be >= 1")
    device = next(model.parameters()).device
    fm = model.fused_model() if getattr(model, "fused", False) and hasattr(model, "fused_model") and device.type == "cuda" else None
    if fm is not None:
        return fm.cell_max_density(box.start, box.granularity, box.shape, s, rot)
    out = None
    with torch.no_grad():
        for a in range(s):
            for b in range(s):
                for c in range(s):
                    x = to_nerf(box.sample_points(a, b, c, s, device), rot).reshape(-1, 3)
                    sig = torch.cat([model.density(x[i:i + chunk_points])["sigma"].float() for i in range(0, x.shape[0], chunk_points)])
                    sig = sig.reshape(box.shape)
                    out = sig if out is None else torch.maximum(out, sig)
    return out


def occupancy_from_density(model, box, thresh, samples_per_axis=2, rot=PLANNER_ROT):
    """cell occupied <=> its largest sigma > thresh (strict, as packbits, raymarching.cu:286-288).  `thresh` is required: sigma
    scales differ from model to model."""
    return cell_max_density(model, box, samples_per_axis, rot) > float(thresh)


def occupancy_from_points(points, box):
    """createCollisionMap.py:43-53 for a point cloud [N, 3] (world frame): every point floors to its cell; points outside the box are
    dropped -> bool [X, Y, Z] (CPU)"""
    occ = np.zeros(box.shape, dtype=bool)
    idx = box.indices(np.asarray(points, np.float64).reshape(-1, 3))
    idx = idx[np.all((idx >= 0) & (idx < np.asarray(box.shape)), axis=1)]
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    return torch.from_numpy(occ)


def occupancy_from_fn(fn, box, samples_per_axis=2):
    """a host-side analytic scene: fn(x, y, z) -> bool on float64 world coordinates; a cell is occupied when any of its
    samples_per_axis^3 points (placed as in ngp_cell_max_density, in float64) is -> bool [X, Y, Z] (CPU)"""
    s = int(samples_per_axis)
    axes = [[box.start[d] + (np.arange(box.shape[d], dtype=np.float64) + (sub + 0.5) / s) / box.granularity for sub in range(s)]
            for d in range(3)]
    occ = np.zeros(box.shape, dtype=bool)
    for xa in axes[0]:
        for ya in axes[1]:
            for za in axes[2]:
                occ |= np.broadcast_to(np.asarray(fn(xa[:, None, None], ya[None, :, None], za[None, None, :]), dtype=bool), box.shape)
    return torch.from_numpy(occ)


def occupancy_from_mesh(world, box, rot=PLANNER_ROT):
    """the true world's map: every cell of `box` that a triangle of `world` (a world.MeshWorld) touches, by world.py's voxelisation
    rule -> bool [X, Y, Z] on the world's device (HIP for a mesh on the GPU, numpy for a CPU world; the same map).  A superset of
    occupancy_from_points on the mesh's vertices: no holes where a triangle is larger than a cell.  rot: a signed permutation."""
    return world.occupancy(box, rot)


def map_agreement(pred, truth):
    """how well a predicted map (a NeRF-density map) matches the truth map (occupancy_from_mesh): two bool maps of one shape (tensors
    or arrays) -> {"tp", "fp", "fn", "tn"} (ints: occupied in both, in pred only, in truth only, in neither) and "iou" = tp / (tp + fp
    + fn), "precision" = tp / (tp + fp), "recall" = tp / (tp + fn) (floats; 1.0 where the denominator is 0: nothing to get wrong)"""
    p, t = torch.as_tensor(pred).bool(), torch.as_tensor(truth).bool()
    if p.shape != t.shape:
        raise ValueError(f"map_agreement: maps of one shape (got {tuple(p.shape)} and {tuple(t.shape)})")
    t = t.to(p.device)
    tp, fp, fn = [int(v) for v in torch.stack([(p & t).sum(), (p & ~t).sum(), (~p & t).sum()]).cpu()]
    ratio = lambda a, b: a / b if b else 1.0                          # noqa: E731
    return {"tp": tp, "fp": fp, "fn": fn, "tn": int(p.numel()) - tp - fp - fn, "iou": ratio(tp, tp + fp + fn),
            "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn)}


def henge_fn(x, y, z):
    """the synthetic scene in the world (drone) frame: scene.henge_occupancy in the NeRF's axes, mapped as rollout.scene_collision
    does (_FLIP_YZ: NeRF = (y, z, x))"""
    return henge_occupancy(y, z, x)


# ------------------------------------------------------------------ the distance transform
def edt_sq(occ):
    """exact squared distance, in cells, from every cell to the nearest occupied one (ngp_edt_sq): bool [X, Y, Z] -> int32 [X, Y, Z]
    on the GPU (the map's device, or the current one for a host map); _lib.NGP_EDT_INF everywhere when no cell is occupied"""
    if occ.dim() != 3:
        raise ValueError("edt_sq: a 3-D map")
    dev = occ.device if occ.is_cuda else torch.device("cuda", torch.cuda.current_device())
    m = occ.to(dev, torch.uint8).contiguous()
    X, Y, Z = m.shape
    lib = _lib.lib()
    d2 = torch.empty(X, Y, Z, dtype=torch.int32, device=dev)
    ws_bytes = lib.ngp_edt_sq_workspace(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ngp_edt_sq(_lib.ptr(m), X, Y, Z, _lib.ptr(d2), _lib.ptr(ws), ws_bytes, _lib.stream()), "edt_sq")
    return d2


class SignedDistanceField:
    """Distances in metres [X, Y, Z] float64 (host) on `box`: its start and granularity place the cells; the index range is the
    array's own shape, as numpy's indexing of the reference's `self.sdf` has it."""

    def __init__(self, values, box):
        self.values = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        if self.values.ndim != 3:
            raise ValueError("SignedDistanceField: a 3-D array")
        self.box = GridBox(box.start, box.granularity, self.values.shape)
        self._collide_below = 1 / self.box.granularity        # NerfSimulator.py:143: within one cell of the surface
        self._dev = {}

    @classmethod
    def from_occupancy(cls, occ, box):
        """createSDF.py:13-32 on the GPU: sqrt(float64(d2)) / granularity; +inf everywhere for a map with no occupied cell (scipy
        measures from a phantom background outside the array there)"""
        if tuple(occ.shape) != box.shape:
            raise ValueError(f"map shape {tuple(occ.shape)} != box shape {box.shape}")
        d2 = edt_sq(occ).cpu().numpy()
        vals = np.sqrt(d2.astype(np.float64)) / box.granularity
        vals[d2 == _lib.NGP_EDT_INF] = np.inf
        return cls(vals, box)

    @classmethod
    def from_mesh(cls, world, box=None, rot=PLANNER_ROT):
        """the ground-truth field: from_occupancy of occupancy_from_mesh(world, box, rot) (box: default reference_box(), the box
        NerfSimulator looks values up in).  A HIP world's map goes to ngp_edt_sq on its device without a host round trip; a CPU
        world's (numpy) map is moved to the current HIP device, as from_occupancy does with any host map -- without one this raises."""
        box = reference_box() if box is None else box
        if world.device.type != "cuda" and not torch.cuda.is_available():
            raise RuntimeError("SignedDistanceField.from_mesh: the distance transform (ngp_edt_sq) is a HIP kernel and no HIP device is "
                               "available; world.occupancy(box) alone runs on the CPU")
        return cls.from_occupancy(occupancy_from_mesh(world, box, rot), box)

    @classmethod
    def from_array(cls, sdf, box=None):
        """a field as the reference stores it (`sdf.npy`), as-is; looked up with `box`'s start and granularity (default: NerfSimulator's
        constants, reference_box())"""
        return cls(sdf, reference_box() if box is None else box)

    def save(self, path):
        """float64 [X, Y, Z] in .npy format, as createSDF.py's sdf.npy"""
        np.save(path, self.values)

    def lookup(self, xyz):
        """NerfSimulator.py:131-147 for one world point -> (collided, value): indices in [-n, n) are valid (negative ones wrap, as numpy
        indexing does) and collided = value < 1 / granularity; anything else is the IndexError branch -> (False, None): not collided,
        the caller keeps its previous value"""
        idx = self.box.world_to_index(xyz)
        if any(not (-n <= i < n) for i, n in zip(idx, self.values.shape)):
            return False, None
        value = float(self.values[idx])
        return value < self._collide_below, value

    def _device_values(self, device):
        v = self._dev.get(device)
        if v is None:
            v = self._dev[device] = torch.from_numpy(self.values).to(device)
        return v

    def query(self, points):
        """lookup's index rule for a batch: points [..., 3] tensor -> (values [...] float64, NaN where out of range; in_range [...] bool),
        on the points' device (float64 index arithmetic)"""
        p = points.to(torch.float64)
        start = torch.tensor(self.box.start, dtype=torch.float64, device=p.device)
        idx = torch.floor((p - start) * self.box.granularity).long()
        n = torch.tensor(self.values.shape, dtype=torch.long, device=p.device)
        ok = ((idx >= -n) & (idx < n)).all(-1)
        idx = torch.where(ok[..., None], torch.where(idx < 0, idx + n, idx), torch.zeros_like(idx))
        vals = self._device_values(p.device)[idx[..., 0], idx[..., 1], idx[..., 2]]
        return torch.where(ok, vals, torch.full_like(vals, float("nan"))), ok


SDF_WORLD = "world"


def resolve_sdf(sdf, world, who):
    """the `sdf` keyword of the rollout entry points: None and a SignedDistanceField pass through; "world" is the ground-truth field
    of `world` (a world.MeshWorld) over reference_box(), SignedDistanceField.from_mesh -- built here, once per run"""
    if not isinstance(sdf, str):
        return sdf
    if sdf != SDF_WORLD:
        raise ValueError(f"{who}: sdf is None, a collision.SignedDistanceField or {SDF_WORLD!r} (got {sdf!r})")
    if world is None:
        raise ValueError(f"{who}: sdf={SDF_WORLD!r} needs world= (a world.MeshWorld: the mesh the ground-truth field is built from)")
    return SignedDistanceField.from_mesh(world, reference_box())
