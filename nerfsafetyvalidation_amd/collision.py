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

The drone's body ("Body collision"; the rule is world.py's docstring, "The body rule"): `lookup` judges the drone's centre
point -- a collision only when the centre lies in an occupied cell.  Opt-in, the simulators judge the planner's body box instead:

    BodyBox(lims, margin=0)        the planner's body_lims as half extents and an offset; BodyBox.planner()
    body_boxes(states, body)       drone states -> the box table [..., 15]; the rule's one rotation (Rodrigues, numpy float64)
    box_cells(boxes, occupied, box)   per box the lowest occupied cell it overlaps     ngp_box_cells_overlap (HIP); box_cells_numpy
    SignedDistanceField.occupied / .box_overlap(boxes)   the field's own map (values == 0) and the test against it

and, with clearance=, score a step by the gap between that box and the nearest obstacle instead of the centre's field value (DESIGN.md,
"Body clearance"; world.py's docstring, "The clearance rule"):

    box_cells_clearance(boxes, occupied, box, max_distance)   per box the distance to the nearest occupied cell, that cell and the
                                                              verdict's cell             ngp_box_cells_clearance (HIP); box_cells_clearance_numpy
    box_cell_distance2(boxes, centre, s)                      the rule's squared distance per (box, cell) pair
    SignedDistanceField.box_clearance(boxes, max_distance)    the same against the field's own map
    trajectory_clearance(states, body, world= / sdf=, exact=, max_distance=)   re-score recorded poses [n, 6] in one call

Connected components ("Connected components"): what tells a floater -- a blob of density attached to nothing, a phantom
obstacle in the field above -- from an obstacle.

    label_components     the labelling rule below                                      ngp_label_components (HIP); numpy on the CPU
    component_table      cells, bounding box and overlap with a truth map per label    ngp_component_stats (HIP); numpy on the CPU
    remove_floaters      drop components by size, rank or contact with the ground
    floater_report       phantom components of a predicted map, missed ones of the truth

The labelling rule.  Input: `occupied` [X, Y, Z] in C order, non-zero = occupied, X * Y * Z < 2^31, every dimension >= 1.  Two
occupied cells are neighbours when their index offset is one of the connectivity's: for 6, 18 and 26 the offsets of {-1,0,1}^3 \\ 0
with at most 1, 2 or 3 non-zero entries; for 14, +- the seven mesh.EDGE_OFFSETS ({0,1}^3 \\ 0), the lattice edges of the isosurface's
Kuhn split -- the connectivity under which two inside lattice points share a marching-tetrahedra edge.  A component is a class of
the transitive closure.  Output: `labels` int32 [X, Y, Z], 0 on empty cells and 1 + rank elsewhere, the components ranked by the
smallest C-order linear index of their cells; `n`, their number.  This is scipy.ndimage.label(occupied, structure) for
generate_binary_structure(3, 1 | 2 | 3) (6, 18, 26) or the 14-offset mask, numbering and dtype included -- a function of the input
alone, the same on every call and on both paths.
"""
import dataclasses

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


def occupancy_from_density(model, box, thresh, samples_per_axis=2, rot=PLANNER_ROT, min_cells=0, connectivity=26, grounded=None):
    """cell occupied <=> its largest sigma > thresh (strict, as packbits, raymarching.cu:286-288).  `thresh` is required: sigma
    scales differ from model to model.  min_cells / connectivity / grounded: handed to remove_floaters, which then takes the
    floaters out of the map (the defaults leave it as it is, and label nothing)."""
    occ = cell_max_density(model, box, samples_per_axis, rot) > float(thresh)
    if min_cells == 0 and grounded is None:
        return occ
    return remove_floaters(occ, connectivity=connectivity, min_cells=min_cells, grounded=grounded)[0]


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


# ------------------------------------------------------------------ connected components
CONNECTIVITIES = (6, 14, 18, 26)
KUHN_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))     # = mesh.EDGE_OFFSETS (mesh imports this module)
_STAGES = {-1: "tile", -2: "seams", -3: "flatten"}                  # ngp_label_components' n_components when a loop reached its bound


def connectivity_offsets(connectivity):
    """the neighbour offsets of a connectivity, both directions -> a list of (dx, dy, dz)"""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity is one of {CONNECTIVITIES} (got {connectivity!r})")
    if connectivity == 14:
        return [o for o in KUHN_OFFSETS] + [tuple(-v for v in o) for o in KUHN_OFFSETS]
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 0 < (dx != 0) + (dy != 0) + (dz != 0) <= most]


def _check_map(occ, who):
    if len(occ.shape) != 3:
        raise ValueError(f"{who}: a 3-D map (got shape {tuple(occ.shape)})")
    if min(occ.shape) < 1 or int(np.prod(occ.shape, dtype=np.int64)) >= 2 ** 31:
        raise ValueError(f"{who}: every dimension >= 1 and X * Y * Z < 2^31 (got shape {tuple(occ.shape)})")


def label_components_numpy(occ, connectivity=26):
    """the labelling rule (module docstring) in numpy: array [X, Y, Z], non-zero = occupied -> (labels int32 [X, Y, Z], n).
    The occupied cells, numbered in C order, are the nodes and every forward offset contributes its pairs of occupied cells as edges;
    then rounds of hooking (the larger root of an edge's two ends under the smaller one, np.minimum.at) and pointer jumping to a
    fixed point.  A path of k cells costs about log2(k) jumps, not k sweeps.  A component's root is its first cell in C order, so the
    roots' order is the ranking."""
    occ = np.asarray(occ)
    _check_map(occ, "label_components")
    forward = [o for o in connectivity_offsets(connectivity) if o > (0, 0, 0)]
    inside = np.ascontiguousarray(occ != 0)
    X, Y, Z = inside.shape
    cells = np.flatnonzero(inside)
    labels = np.zeros(inside.shape, dtype=np.int32)
    if cells.size == 0:
        return labels, 0
    node = np.full(inside.size, -1, dtype=np.int64)
    node[cells] = np.arange(cells.size)
    node = node.reshape(inside.shape)
    us, vs = [], []
    for dx, dy, dz in forward:          # dx >= 0; the lower end a and the upper end b = a + offset
        a = (slice(0, X - dx), slice(max(0, -dy), Y - max(0, dy)), slice(max(0, -dz), Z - max(0, dz)))
        b = (slice(dx, X), slice(max(0, dy), Y + min(0, dy)), slice(max(0, dz), Z + min(0, dz)))
        both = inside[a] & inside[b]
        us.append(node[a][both])
        vs.append(node[b][both])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(cells.size)
    while u.size:
        pu, pv = parent[u], parent[v]
        differ = pu != pv
        if not differ.any():
            break
        u, v, pu, pv = u[differ], v[differ], pu[differ], pv[differ]
        np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))          # parent is flat here: both are roots
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
    roots = parent == np.arange(cells.size)
    rank = np.cumsum(roots)
    labels.reshape(-1)[cells] = rank[parent]
    return labels, int(rank[-1])


def _label_components_hip(occ, connectivity):
    m = (occ != 0).to(torch.uint8).contiguous()
    X, Y, Z = m.shape
    with torch.cuda.device(m.device):
        labels = torch.empty(X, Y, Z, dtype=torch.int32, device=m.device)
        n_dev = torch.empty(1, dtype=torch.int32, device=m.device)
        ws, ws_bytes = _lib.workspace("label_components", X, Y, Z, device=m.device)
        _lib.call("label_components", m, X, Y, Z, connectivity, labels, n_dev, ws, ws_bytes)
        n = int(n_dev.item())          # the call's one host read
    if n < 0:
        raise RuntimeError(f"label_components: a device loop reached its bound in stage '{_STAGES.get(n, n)}'; the labels are not valid")
    return labels, n


def label_components(occ, connectivity=26):
    """the labelling rule (module docstring) -> (labels int32 [X, Y, Z], n: int).  A CUDA tensor goes through ngp_label_components on
    the current stream and the labels stay on its device (one host read, of n); a CPU tensor or a numpy array goes through
    label_components_numpy and the same kind comes back.  Any dtype (non-zero = occupied) and any strides."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"label_components: connectivity is one of {CONNECTIVITIES} (got {connectivity!r})")
    _check_map(occ, "label_components")
    if isinstance(occ, torch.Tensor):
        if occ.is_cuda:
            return _label_components_hip(occ.detach(), connectivity)
        labels, n = label_components_numpy(occ.detach().numpy(), connectivity)
        return torch.from_numpy(labels), n
    return label_components_numpy(occ, connectivity)


@dataclasses.dataclass
class ComponentTable:
    """per component (row c: label c + 1): `cells` int64 [n] the number of cells, `lo` / `hi` int32 [n, 3] the inclusive index
    bounding box, `overlap` int64 [n] the number of its cells a truth map marks (None without one).  Tensors on the labels' device,
    or numpy arrays for numpy labels."""
    cells: object
    lo: object
    hi: object
    overlap: object


def component_table_numpy(labels, n, truth=None):
    """component_table in numpy -> ComponentTable of arrays"""
    labels = np.asarray(labels)
    flat = labels.reshape(-1)
    cells = np.bincount(flat, minlength=n + 1)[1:n + 1].astype(np.int64)
    lo, hi = np.full((n, 3), np.iinfo(np.int32).max, dtype=np.int32), np.full((n, 3), -1, dtype=np.int32)
    where = np.flatnonzero(flat)
    which = flat[where] - 1
    for d, coord in enumerate(np.unravel_index(where, labels.shape)):
        np.minimum.at(lo[:, d], which, coord.astype(np.int32))
        np.maximum.at(hi[:, d], which, coord.astype(np.int32))
    overlap = None
    if truth is not None:
        marked = np.asarray(truth).reshape(-1)[where] != 0
        overlap = np.bincount(which[marked], minlength=n).astype(np.int64)
    return ComponentTable(cells, lo, hi, overlap)


def component_table(labels, n, truth=None):
    """labels int32 [X, Y, Z] of n components (label_components' pair), truth: a map of the same shape or None -> ComponentTable.
    CUDA labels go through ngp_component_stats on the current stream and everything stays on the device (no host read); anything
    else through numpy.  The values are the same."""
    n = int(n)
    if n < 0 or len(labels.shape) != 3:
        raise ValueError(f"component_table: labels [X, Y, Z] and n >= 0 (got shape {tuple(labels.shape)}, n = {n})")
    if truth is not None and tuple(truth.shape) != tuple(labels.shape):
        raise ValueError(f"component_table: truth has the labels' shape (got {tuple(truth.shape)} and {tuple(labels.shape)})")
    if not isinstance(labels, torch.Tensor):
        return component_table_numpy(labels, n, None if truth is None else (truth.cpu().numpy() if isinstance(truth, torch.Tensor) else truth))
    if not labels.is_cuda:
        t = component_table_numpy(labels.numpy(), n, None if truth is None else torch.as_tensor(truth).cpu().numpy())
        return ComponentTable(*[None if a is None else torch.from_numpy(a) for a in (t.cells, t.lo, t.hi, t.overlap)])
    dev = labels.device
    lab = labels.detach().to(torch.int32).contiguous()
    marks = None if truth is None else (torch.as_tensor(truth).to(dev) != 0).to(torch.uint8).contiguous()
    X, Y, Z = lab.shape
    with torch.cuda.device(dev):
        cells = torch.empty(n, dtype=torch.int64, device=dev)
        lo, hi = torch.empty(n, 3, dtype=torch.int32, device=dev), torch.empty(n, 3, dtype=torch.int32, device=dev)
        overlap = None if truth is None else torch.empty(n, dtype=torch.int64, device=dev)
        _lib.call("component_stats", lab, X, Y, Z, n, marks, cells, lo, hi, overlap)
    return ComponentTable(cells, lo, hi, overlap)


def _table_to_host(table):
    """a ComponentTable as numpy arrays, with ONE device-to-host copy when it lives on a device"""
    if not isinstance(table.cells, torch.Tensor):
        return table
    n = table.cells.shape[0]
    cols = [table.cells.reshape(n, 1), table.lo.to(torch.int64), table.hi.to(torch.int64)]
    if table.overlap is not None:
        cols.append(table.overlap.reshape(n, 1))
    packed = torch.cat(cols, 1).cpu().numpy()
    return ComponentTable(packed[:, 0].copy(), packed[:, 1:4].astype(np.int32), packed[:, 4:7].astype(np.int32),
                          None if table.overlap is None else packed[:, 7].copy())


def _listing(table, pick):
    """the report of the components `pick` (bool [n], host) of a host table"""
    idx = np.flatnonzero(pick)
    return {"count": int(idx.size), "labels": [int(i) + 1 for i in idx], "cells": [int(c) for c in table.cells[idx]],
            "lo": [tuple(int(v) for v in row) for row in table.lo[idx]], "hi": [tuple(int(v) for v in row) for row in table.hi[idx]]}


def _select_cells(labels, pick):
    """bool [X, Y, Z]: the cells whose component `pick` (bool [n], host) selects, of the labels' kind"""
    lut = np.concatenate([[False], np.asarray(pick, dtype=bool)])
    if isinstance(labels, torch.Tensor):
        return torch.from_numpy(lut).to(labels.device)[labels.long()]
    return lut[labels]


def remove_floaters(occ, *, connectivity=26, min_cells=0, keep_largest=None, grounded=None):
    """occ [X, Y, Z] (tensor on any device, or numpy; non-zero = occupied) -> (cleaned, report).  A component (label_components with
    `connectivity`) is KEPT iff all of: it has at least min_cells cells; it is among the keep_largest largest (ties: the lower label
    first; None: no limit); with grounded = (axis, "lo" | "hi"), its bounding box reaches the first ("lo") or last ("hi") layer of
    that axis -- a floater is what is attached to nothing.  cleaned: the map without the dropped components, of the input's kind,
    dtype and device (the input itself when nothing is dropped).  report: {"n", "kept": {...}, "dropped": {...}}, each with
    "count", "labels", "cells", "lo", "hi" (the inclusive index boxes).  One host read of n and one of the table."""
    if len(occ.shape) != 3:
        raise ValueError(f"remove_floaters: a 3-D map (got shape {tuple(occ.shape)})")
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"remove_floaters: connectivity is one of {CONNECTIVITIES} (got {connectivity!r})")
    if int(min_cells) != min_cells or min_cells < 0:
        raise ValueError(f"remove_floaters: min_cells is an integer >= 0 (got {min_cells!r})")
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
        raise ValueError(f"remove_floaters: keep_largest is None or an integer >= 1 (got {keep_largest!r})")
    if grounded is not None:
        if not (isinstance(grounded, (tuple, list)) and len(grounded) == 2 and grounded[0] in (0, 1, 2) and grounded[1] in ("lo", "hi")):
            raise ValueError(f"remove_floaters: grounded is None or (axis in 0..2, 'lo' | 'hi') (got {grounded!r})")
    labels, n = label_components(occ, connectivity)
    table = _table_to_host(component_table(labels, n))
    keep = table.cells >= int(min_cells)
    if keep_largest is not None:
        order = np.lexsort((np.arange(n), -table.cells))          # by size, largest first; ties by label
        among = np.zeros(n, dtype=bool)
        among[order[:int(keep_largest)]] = True
        keep &= among
    if grounded is not None:
        axis, side = grounded
        keep &= (table.lo[:, axis] == 0) if side == "lo" else (table.hi[:, axis] == occ.shape[axis] - 1)
    report = {"n": n, "kept": _listing(table, keep), "dropped": _listing(table, ~keep)}
    if keep.all():
        return occ, report
    kept_cells = _select_cells(labels, keep)
    if isinstance(occ, torch.Tensor):
        return torch.where(kept_cells, occ, torch.zeros_like(occ)), report
    return np.where(kept_cells, occ, np.zeros_like(occ)), report


def floater_report(pred, truth, connectivity=26):
    """a predicted map (a NeRF-density map) against the truth map (occupancy_from_mesh), component by component ->
    {"phantom": the components of pred without a single cell in truth (obstacles that do not exist: floaters),
     "missed": the components of truth without a single cell in pred (whole obstacles the model does not see),
     "pred_components", "truth_components": the two counts, "agreement": map_agreement(pred, truth)};
    phantom and missed as remove_floaters' listings ("count", "labels", "cells", "lo", "hi").  Runs where pred lives."""
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError(f"floater_report: maps of one shape (got {tuple(pred.shape)} and {tuple(truth.shape)})")
    if isinstance(pred, torch.Tensor):
        truth = torch.as_tensor(truth).to(pred.device)
    else:
        truth = truth.cpu().numpy() if isinstance(truth, torch.Tensor) else np.asarray(truth)
    out = {}
    for key, (a, b) in (("phantom", (pred, truth)), ("missed", (truth, pred))):
        labels, n = label_components(a, connectivity)
        table = _table_to_host(component_table(labels, n, b))
        out[key] = _listing(table, table.overlap == 0)
        out["pred_components" if key == "phantom" else "truth_components"] = n
    out["agreement"] = map_agreement(pred, truth)
    return out


# ------------------------------------------------------------------ the distance transform
def edt_sq(occ):
    """exact squared distance, in cells, from every cell to the nearest occupied one (ngp_edt_sq): bool [X, Y, Z] -> int32 [X, Y, Z]
    on the GPU (the map's device, or the current one for a host map); _lib.NGP_EDT_INF everywhere when no cell is occupied"""
    if occ.dim() != 3:
        raise ValueError("edt_sq: a 3-D map")
    dev = occ.device if occ.is_cuda else torch.device("cuda", torch.cuda.current_device())
    m = occ.to(dev, torch.uint8).contiguous()
    X, Y, Z = m.shape
    d2 = torch.empty(X, Y, Z, dtype=torch.int32, device=dev)
    ws, ws_bytes = _lib.workspace("edt_sq", X, Y, Z, device=dev)
    _lib.call("edt_sq", m, X, Y, Z, d2, ws, ws_bytes)
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

    @property
    def occupied(self):
        """the map the field was made from, bool [X, Y, Z] (host): values == 0 -- all-false for a field with no occupied cell"""
        occ = self._dev.get("occupied")
        if occ is None:
            occ = self._dev["occupied"] = np.ascontiguousarray(self.values == 0)
        return occ

    def _device_occupied(self, device):
        device = torch.device(device)
        m = self._dev.get(("occupied", device))
        if m is None:
            m = self._dev[("occupied", device)] = torch.from_numpy(self.occupied).to(device)
        return m

    def box_overlap(self, boxes, device=None):
        """body boxes float64 [N,15] (world.py's box table; collision.body_boxes) against the field's occupied cells by the body rule
        -> `cell` int32 [N]: the lowest C-order linear index of an occupied cell each box overlaps, -1 without one.  device: where the
        test runs -- None: where the boxes are (numpy boxes: the host, box_cells_numpy, an array comes back); a HIP device: csrc/body.hip
        on the current stream against a cached device copy of the map, the result a tensor there."""
        if device is None:
            device = boxes.device if isinstance(boxes, torch.Tensor) else "cpu"
        device = torch.device(device)
        if device.type != "cuda":
            cell = box_cells_numpy(boxes, self.occupied, self.box)
            return torch.from_numpy(cell) if isinstance(boxes, torch.Tensor) else cell
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return box_cells(boxes, self._device_occupied(device), self.box)

    def box_clearance(self, boxes, max_distance, device=None):
        """body boxes float64 [N,15] against the field's occupied cells by the clearance rule -> {"distance" float64 [N], "cell" int32
        [N], "hit" int32 [N]} (hit: box_overlap's cell).  device: box_overlap's rule -- None: where the boxes are (numpy boxes: the
        host, box_cells_clearance_numpy, arrays come back); a HIP device: csrc/clearance.hip on the current stream against the cached
        device copy of the map, the results tensors there."""
        if device is None:
            device = boxes.device if isinstance(boxes, torch.Tensor) else "cpu"
        device = torch.device(device)
        if device.type != "cuda":
            out = box_cells_clearance_numpy(boxes, self.occupied, self.box, max_distance)
            return {k: torch.from_numpy(v) for k, v in out.items()} if isinstance(boxes, torch.Tensor) else out
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return box_cells_clearance(boxes, self._device_occupied(device), self.box, max_distance)

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


# ------------------------------------------------------------------ the drone's body (world.py's docstring, "The body rule")
_BODY_CHUNK_PAIRS = 1 << 18                         # (box, candidate cell) pairs per chunk of box_cells_numpy
ORTHONORMAL_TOL = 1e-6                              # body_boxes refuses an R with max |R^T R - I| above this


class BodyBox:
    """The drone's body as the planner has it (envConfig.json's body_lims): lims [[x0, x1], [y0, y1], [z0, z1]] in the body frame,
    metres.  half = (hi - lo) / 2 + margin, offset = (hi + lo) / 2 (float64 [3] each); margin >= 0 inflates every half extent."""

    def __init__(self, lims, margin=0.0):
        lims = np.asarray(lims, np.float64)
        if lims.shape != (3, 2) or not np.isfinite(lims).all() or (lims[:, 1] < lims[:, 0]).any():
            raise ValueError(f"BodyBox: lims are [[x0, x1], [y0, y1], [z0, z1]] with lo <= hi (got {lims.tolist()})")
        if not (float(margin) >= 0.0 and np.isfinite(margin)):
            raise ValueError(f"BodyBox: margin is a finite length >= 0 (got {margin!r})")
        self.lims, self.margin = lims, float(margin)
        self.half = (lims[:, 1] - lims[:, 0]) / 2 + self.margin
        self.offset = (lims[:, 1] + lims[:, 0]) / 2

    @classmethod
    def planner(cls, margin=0.0):
        """the box the planner plans with: rollout.PLANNER_ENV["body_lims"], +-5 x +-5 x +-2 cm"""
        from .rollout import PLANNER_ENV
        return cls(PLANNER_ENV["body_lims"], margin)

    def __repr__(self):
        return f"BodyBox(lims={self.lims.tolist()}, margin={self.margin})"


def rodrigues(rot_vec):
    """rotation vectors float64 [..., 3] -> R [..., 3, 3] = I + sin(t) K + (1 - cos(t)) K K, t = |v|, K the skew matrix of v / t (the
    identity for t == 0), numpy float64.  The body rule's only rotation: no kernel computes one."""
    v = np.asarray(rot_vec, np.float64)
    t = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]
    with np.errstate(all="ignore"):
        k = np.where(t > 0, v / np.where(t > 0, t, 1.0), 0.0)
    K = np.zeros(v.shape[:-1] + (3, 3), np.float64)
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    t = t[..., None]
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def body_boxes(states, body):
    """drone states -> the body rule's box table float64 [..., 15] (numpy).  states [..., 12] (rollout's: xyz 0:3, rotation vector
    6:9), [..., 6] (xyz, rotation vector) or [..., 18] (the planner's: xyz 0:3, R row-major 6:15, used as given).  R = rodrigues of
    the rotation vector, the centre xyz + R offset, the half extents body.half.  ValueError when max |R^T R - I| > ORTHONORMAL_TOL
    (or is not a number)."""
    s = np.asarray(states.detach().cpu().numpy() if isinstance(states, torch.Tensor) else states, np.float64)
    if s.ndim < 1 or s.shape[-1] not in (6, 12, 18):
        raise ValueError(f"body_boxes: states are [..., 12], [..., 6] (xyz, rotation vector) or [..., 18] (with R), got {s.shape}")
    if s.shape[-1] == 18:
        R = s[..., 6:15].reshape(s.shape[:-1] + (3, 3))
    else:
        R = rodrigues(s[..., 6:9] if s.shape[-1] == 12 else s[..., 3:6])
    if R.size:
        err = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max()
        if not err <= ORTHONORMAL_TOL:
            raise ValueError(f"body_boxes: R is not a rotation, max |R^T R - I| = {err} > {ORTHONORMAL_TOL}")
    out = np.empty(s.shape[:-1] + (15,), np.float64)
    out[..., 0:3] = s[..., 0:3] + (R @ body.offset[:, None])[..., 0]
    out[..., 3:12] = R.reshape(s.shape[:-1] + (9,))
    out[..., 12:15] = body.half
    return out


def box_cell_overlap(boxes, centre, s):
    """the body rule's box-cell test for M (box, cell) pairs: boxes float64 [M,15], centre float64 [M,3] the cells' centres (world),
    s their half-width -> bool [M]"""
    from . import world as WO
    with np.errstate(all="ignore"):
        c, R, h, valid = WO.box_parts(boxes)
        t = WO.box_frame(c, R, centre)
        A = np.abs(R)
        sep = ~valid
        for a in range(3):
            sep = sep | (np.abs(t[a]) > h[:, a] + s * ((A[:, 0, a] + A[:, 1, a]) + A[:, 2, a]))
        for i in range(3):
            q = (R[:, i, 0] * t[0] + R[:, i, 1] * t[1]) + R[:, i, 2] * t[2]
            sep = sep | (np.abs(q) > ((h[:, 0] * A[:, i, 0] + h[:, 1] * A[:, i, 1]) + h[:, 2] * A[:, i, 2]) + s)
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            for a in range(3):
                b, cc = (a + 1) % 3, (a + 2) % 3
                p = R[:, i, b] * t[cc] - R[:, i, cc] * t[b]
                r = (h[:, b] * A[:, i, cc] + h[:, cc] * A[:, i, b]) + s * (A[:, j, a] + A[:, k, a])
                sep = sep | (np.abs(p) > r)
    return ~sep


def box_candidates(boxes, box, reach=0.0):
    """the candidate cells of every body box in the map's GridBox: per axis floor((c_a - E_a - start_a) g) - 1 .. floor((c_a + E_a -
    start_a) g) + 1 clipped to the map -> (lo int64 [N,3], n int64 [N,3]): the first cell and the number of cells (0: none; an
    invalid row has none); a NaN bound takes the whole axis.  reach: the clearance rule's max_distance, E_a + reach in E_a's place"""
    from . import world as WO
    c, R, h, valid = WO.box_parts(boxes)
    start, g, top = np.asarray(box.start, np.float64), np.float64(box.granularity), np.asarray(box.shape, np.float64) - 1.0
    with np.errstate(all="ignore"):
        E = WO.box_extent(R, h) + np.float64(reach)
        l = np.floor(((c - E) - start) * g) - 1.0
        u = np.floor(((c + E) - start) * g) + 1.0
        some = ~((u < 0.0) | (l > top)).any(1) & valid
        first = np.where(l >= 1.0, np.minimum(l, top), 0.0)
        last = np.where(u <= top - 1.0, np.maximum(u, 0.0), top)
    first, last = np.nan_to_num(first).astype(np.int64), np.nan_to_num(last).astype(np.int64)
    return first, np.where(some[:, None], np.maximum(last - first + 1, 0), 0)


def box_cells_numpy(boxes, occupied, box, all_cells=False):
    """the body rule's box-cells test in numpy, chunked over (box, candidate cell) pairs: boxes float64 [N,15], occupied [X,Y,Z]
    (non-zero = occupied), box the map's GridBox (its start and granularity; the index range is the array's) -> int32 [N]: the lowest
    C-order linear index of an occupied cell the box overlaps, -1 without one.  all_cells: every cell of the map is every box's
    candidate (brute force, for small maps: the candidates change no result)"""
    from . import world as WO
    b = WO.check_boxes(boxes, "box_cells_numpy")
    occ = np.ascontiguousarray(np.asarray(occupied) != 0)
    _check_map(occ, "box_cells_numpy")
    box = GridBox(box.start, box.granularity, occ.shape)
    WO.check_voxel_box(box)
    N = b.shape[0]
    none = np.iinfo(np.int64).max
    best = np.full(N, none, np.int64)
    if N == 0:
        return np.full(0, -1, np.int32)
    shape = np.asarray(occ.shape, np.int64)
    start, g = np.asarray(box.start, np.float64), np.float64(box.granularity)
    s = np.float64(0.5) / g
    if all_cells:
        lo, n = np.zeros((N, 3), np.int64), np.tile(shape, (N, 1))
    else:
        lo, n = box_candidates(b, box)
    counts = n.prod(1)
    ends = np.cumsum(counts)
    flat = occ.reshape(-1)
    for p0 in range(0, int(ends[-1]), _BODY_CHUNK_PAIRS):
        pair = np.arange(p0, min(int(ends[-1]), p0 + _BODY_CHUNK_PAIRS), dtype=np.int64)
        i = np.searchsorted(ends, pair, side="right")                              # the first box with ends[i] > pair
        j = pair - (ends[i] - counts[i])
        nyz, nz = n[i, 1] * n[i, 2], n[i, 2]
        ijk = np.stack([lo[i, 0] + j // nyz, lo[i, 1] + (j % nyz) // nz, lo[i, 2] + j % nz], 1)
        cell = (ijk[:, 0] * shape[1] + ijk[:, 1]) * shape[2] + ijk[:, 2]
        keep = flat[cell]                                                          # only an occupied cell can be the answer
        i, ijk, cell = i[keep], ijk[keep], cell[keep]
        centre = start + (ijk.astype(np.float64) + 0.5) / g
        hit = box_cell_overlap(b[i], centre, s)
        np.minimum.at(best, i[hit], cell[hit])
    return np.where(best == none, -1, best).astype(np.int32)


def box_cells(boxes, occupied, box):
    """the free function that dispatches: boxes [N,15] (float64; tensor or numpy), occupied [X,Y,Z] (a map: bool or uint8, non-zero =
    occupied), box the map's GridBox -> int32 [N] by the body rule.  A map on a HIP device goes through ngp_box_cells_overlap on the
    current stream and the result stays there (no host read); a host map through box_cells_numpy (a tensor comes back for a tensor
    map, an array for an array)."""
    from . import world as WO
    if not (isinstance(occupied, torch.Tensor) and occupied.is_cuda):
        host = occupied.detach().numpy() if isinstance(occupied, torch.Tensor) else occupied
        cell = box_cells_numpy(boxes, host, box)
        return torch.from_numpy(cell) if isinstance(occupied, torch.Tensor) else cell
    _check_map(occupied, "box_cells")
    dev = occupied.device
    m = occupied.detach()
    m = (m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).to(torch.uint8)).contiguous()
    grid = GridBox(box.start, box.granularity, tuple(m.shape))
    WO.check_voxel_box(grid)
    b = boxes.detach() if isinstance(boxes, torch.Tensor) else torch.from_numpy(WO.check_boxes(boxes, "box_cells"))
    if b.dim() != 2 or b.shape[1] != 15:
        raise ValueError(f"box_cells: the box table is [N,15] (centre, R row-major, half extents), got {tuple(b.shape)}")
    b = b.to(dev, torch.float64).contiguous()
    N = b.shape[0]
    if N >= 2 ** 31:
        raise ValueError("box_cells: N must be < 2^31")
    cell = torch.empty(N, dtype=torch.int32, device=dev)
    if N:
        import ctypes
        with torch.cuda.device(dev):
            _lib.call("box_cells_overlap", m, ctypes.byref(WO._voxel_box_struct(grid, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])), b, N, cell)
    return cell


# ------------------------------------------------------------------ the body's clearance (world.py's docstring, "The clearance rule")
def _box_cell_terms(boxes, centre, s):
    """-> (d2 float64 [M] by the clearance rule's box-cell part, +inf for an invalid row; overlap bool [M] by the body rule)"""
    from . import world as WO
    inf = np.float64(np.inf)
    with np.errstate(all="ignore"):
        c, R, h, valid = WO.box_parts(boxes)
        over = box_cell_overlap(boxes, centre, s)
        hh = [h[:, a] for a in range(3)]
        best = np.full(boxes.shape[0], inf)
        for m in range(8):                                                         # the cell's corners against the box
            x = np.stack([centre[:, i] + (s if (m >> i) & 1 else -s) for i in range(3)], 1)
            best = WO._take_smaller(best, WO.clamp_gap2(WO.box_frame(c, R, x), hh))
        for m in range(8):                                                         # the box's corners against the cell
            o = [hh[a] if (m >> a) & 1 else -hh[a] for a in range(3)]
            y = [(c[:, i] + ((R[:, i, 0] * o[0] + R[:, i, 1] * o[1]) + R[:, i, 2] * o[2])) - centre[:, i] for i in range(3)]
            best = WO._take_smaller(best, WO.clamp_gap2(y, [s, s, s]))
        for i in range(3):                                                         # the cell's edges against the box's edges
            j, k = (i + 1) % 3, (i + 2) % 3
            for m in range(4):
                x0 = np.empty_like(centre)
                x0[:, i], x0[:, j], x0[:, k] = centre[:, i] - s, centre[:, j] + (s if m & 1 else -s), centre[:, k] + (s if m & 2 else -s)
                x1 = x0.copy()
                x1[:, i] = centre[:, i] + s
                q0, q1 = WO.box_frame(c, R, x0), WO.box_frame(c, R, x1)
                best = WO.box_edges_segment_d2(hh, q0, [q1[a] - q0[a] for a in range(3)], best)
    return np.where(valid, np.where(over, 0.0, best), inf), over & valid


def box_cell_distance2(boxes, centre, s):
    """the clearance rule's squared distance for M (box, cell) pairs: boxes float64 [M,15], centre float64 [M,3] the cells' centres
    (world), s their half-width -> float64 [M]: 0 where the body rule says overlap, else the smallest of the 160 candidates; +inf
    for an invalid row"""
    return _box_cell_terms(np.ascontiguousarray(boxes, np.float64), np.asarray(centre, np.float64), np.float64(s))[0]


def _cell_skip(boxes, centre, s, limit2):
    """the rule's lower-bound skip for (box, cell) pairs: True where the cell's bounds in the box's frame prove d2 > limit2"""
    from . import world as WO
    with np.errstate(all="ignore"):
        c, R, h, _ = WO.box_parts(boxes)
        t = WO.box_frame(c, R, centre)
        A = np.abs(R)
        rho = [s * ((A[:, 0, a] + A[:, 1, a]) + A[:, 2, a]) for a in range(3)]
        lb2, m = WO.frame_gap2([t[a] - rho[a] for a in range(3)], [t[a] + rho[a] for a in range(3)], [h[:, a] for a in range(3)])
        return lb2 > limit2 + WO.CLEARANCE_SKIP * (limit2 + m * m)


def box_cells_clearance_numpy(boxes, occupied, box, max_distance, all_cells=False):
    """the clearance rule against a map in numpy, chunked over (box, candidate cell) pairs: box_cells_numpy's arguments and
    max_distance (a length > 0 or +inf) -> {"distance" float64 [N] (+inf: no occupied cell within max_distance), "cell" int32 [N]
    (-1), "hit" int32 [N]: box_cells_numpy's cell}.  all_cells: every cell of the map is every box's candidate."""
    from . import world as WO
    max_distance = WO.check_max_distance(max_distance, "box_cells_clearance_numpy")
    b = WO.check_boxes(boxes, "box_cells_clearance_numpy")
    occ = np.ascontiguousarray(np.asarray(occupied) != 0)
    _check_map(occ, "box_cells_clearance_numpy")
    box = GridBox(box.start, box.granularity, occ.shape)
    WO.check_voxel_box(box)
    N = b.shape[0]
    inf, none = np.float64(np.inf), np.iinfo(np.int64).max
    best, arg, hit = np.full(N, inf), np.full(N, none, np.int64), np.full(N, none, np.int64)
    out = {"distance": np.full(N, inf), "cell": np.full(N, -1, np.int32), "hit": np.full(N, -1, np.int32)}
    if N == 0:
        return out
    shape = np.asarray(occ.shape, np.int64)
    start, g = np.asarray(box.start, np.float64), np.float64(box.granularity)
    s = np.float64(0.5) / g
    limit2 = np.float64(max_distance) * np.float64(max_distance)
    if all_cells:
        lo, n = np.zeros((N, 3), np.int64), np.tile(shape, (N, 1))
        n = np.where(WO.box_parts(b)[3][:, None], n, 0)
    else:
        lo, n = box_candidates(b, box, max_distance)
    counts = n.prod(1)
    ends = np.cumsum(counts)
    flat = occ.reshape(-1)
    for p0 in range(0, int(ends[-1]), _BODY_CHUNK_PAIRS):
        pair = np.arange(p0, min(int(ends[-1]), p0 + _BODY_CHUNK_PAIRS), dtype=np.int64)
        i = np.searchsorted(ends, pair, side="right")
        j = pair - (ends[i] - counts[i])
        nyz, nz = n[i, 1] * n[i, 2], n[i, 2]
        ijk = np.stack([lo[i, 0] + j // nyz, lo[i, 1] + (j % nyz) // nz, lo[i, 2] + j % nz], 1)
        cell = (ijk[:, 0] * shape[1] + ijk[:, 1]) * shape[2] + ijk[:, 2]
        keep = flat[cell]
        i, ijk, cell = i[keep], ijk[keep], cell[keep]
        centre = start + (ijk.astype(np.float64) + 0.5) / g
        keep = ~_cell_skip(b[i], centre, s, limit2)
        i, cell, centre = i[keep], cell[keep], centre[keep]
        d2, over = _box_cell_terms(b[i], centre, s)
        np.minimum.at(hit, i[over], cell[over])
        order = np.lexsort((cell, d2, i))                                          # per box: the smallest d2, then the lowest cell
        i, cell, d2 = i[order], cell[order], d2[order]
        head = np.r_[True, i[1:] != i[:-1]] if i.size else np.zeros(0, bool)
        i, cell, d2 = i[head], cell[head], d2[head]
        better = (d2 < best[i]) | ((d2 == best[i]) & (cell < arg[i]))
        best[i[better]], arg[i[better]] = d2[better], cell[better]
    with np.errstate(all="ignore"):
        distance = np.sqrt(best)
        ok = (best < inf) & (distance <= max_distance)
    hit = np.where(hit == none, -1, hit)
    out["distance"] = np.where(ok, distance, inf)
    out["cell"] = np.where(hit >= 0, hit, np.where(ok, arg, -1)).astype(np.int32)
    out["hit"] = hit.astype(np.int32)
    return out


def _clearance_boxes(boxes, dev, who):
    from . import world as WO
    b = boxes.detach() if isinstance(boxes, torch.Tensor) else torch.from_numpy(WO.check_boxes(boxes, who))
    if b.dim() != 2 or b.shape[1] != 15:
        raise ValueError(f"{who}: the box table is [N,15] (centre, R row-major, half extents), got {tuple(b.shape)}")
    if b.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: N must be < 2^31")
    return b.to(dev, torch.float64).contiguous()


def box_cells_clearance(boxes, occupied, box, max_distance):
    """the free function that dispatches, as box_cells does: -> {"distance" float64 [N], "cell" int32 [N], "hit" int32 [N]} by the
    clearance rule.  A map on a HIP device goes through ngp_box_cells_clearance on the current stream and the results stay there; a
    host map through box_cells_clearance_numpy (tensors come back for a tensor map, arrays for an array)."""
    from . import world as WO
    max_distance = WO.check_max_distance(max_distance, "box_cells_clearance")
    if not (isinstance(occupied, torch.Tensor) and occupied.is_cuda):
        host = occupied.detach().numpy() if isinstance(occupied, torch.Tensor) else occupied
        out = box_cells_clearance_numpy(boxes, host, box, max_distance)
        return {k: torch.from_numpy(v) for k, v in out.items()} if isinstance(occupied, torch.Tensor) else out
    _check_map(occupied, "box_cells_clearance")
    dev = occupied.device
    m = occupied.detach()
    m = (m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).to(torch.uint8)).contiguous()
    grid = GridBox(box.start, box.granularity, tuple(m.shape))
    WO.check_voxel_box(grid)
    b = _clearance_boxes(boxes, dev, "box_cells_clearance")
    N = b.shape[0]
    out = {"distance": torch.empty(N, dtype=torch.float64, device=dev), "cell": torch.empty(N, dtype=torch.int32, device=dev),
           "hit": torch.empty(N, dtype=torch.int32, device=dev)}
    if N:
        import ctypes
        with torch.cuda.device(dev):
            _lib.call("box_cells_clearance", m, ctypes.byref(WO._voxel_box_struct(grid, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])), b, N,
                      max_distance, out["distance"], out["cell"], out["hit"])
    return out


def trajectory_clearance(states, body, *, world=None, sdf=None, exact=False, max_distance):
    """re-score recorded poses: interpolated drone states [n, 6] (xyz, rotation vector; body_boxes' other layouts too), body a BodyBox
    -> the clearance rule's dict for the n body boxes, in one call: exact=False against the occupied cells of `sdf` (a
    SignedDistanceField; on `world`'s device when that is a HIP world) -> {"distance", "cell", "hit"}; exact=True against `world`'s
    triangles -> {"distance", "prim", "hit"}"""
    if not isinstance(body, BodyBox):
        raise ValueError(f"trajectory_clearance: body is a collision.BodyBox (got {type(body).__name__})")
    boxes = body_boxes(states, body)
    boxes = boxes.reshape(-1, 15)
    if exact:
        if world is None:
            raise ValueError("trajectory_clearance: exact=True measures against the world's triangles and needs world= (a world.MeshWorld)")
        return world.box_clearance(boxes, max_distance)
    if not isinstance(sdf, SignedDistanceField):
        raise ValueError("trajectory_clearance: sdf= is a collision.SignedDistanceField (or exact=True with world=)")
    device = getattr(world, "device", None)
    return sdf.box_clearance(boxes, max_distance, device=device if device is not None and device.type == "cuda" else None)


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


def check_body(body, exact, sdf, world, who):
    """the `body` / `exact` keywords of the rollout entry points against the resolved `sdf` and `world`: None passes (with exact
    unset); a BodyBox needs a map -- the analytic stand-in (sdf=None) has none -- and exact=True needs world="""
    if body is None:
        if exact:
            raise ValueError(f"{who}: exact=True selects the body's test and needs body= (a collision.BodyBox)")
        return
    if not isinstance(body, BodyBox):
        raise ValueError(f"{who}: body is None or a collision.BodyBox (got {type(body).__name__})")
    if exact and world is None:
        raise ValueError(f"{who}: exact=True tests the body against the world's triangles and needs world= (a world.MeshWorld)")
    if sdf is None:
        raise ValueError(f"{who}: body= needs sdf= (a collision.SignedDistanceField or {SDF_WORLD!r}): the analytic stand-in has no map "
                         "of occupied cells, and no field for the centre's value")


def check_clearance(clearance, body, who):
    """the `clearance` keyword of the rollout entry points: None passes; otherwise a finite length > 0 (the cap D of the step's
    value), which needs body= -> None or the float"""
    if clearance is None:
        return None
    d = float(clearance)
    if not (d > 0.0 and np.isfinite(d)):
        raise ValueError(f"{who}: clearance is None or a finite length > 0 in metres (got {clearance!r})")
    if body is None:
        raise ValueError(f"{who}: clearance= measures the gap between the body and the obstacles and needs body= (a collision.BodyBox)")
    return d
