"""Shared inputs of the body-clearance tests (test_clearance_cpu.py, test_clearance_gpu.py): hand triangles around body_cases.HAND_BOX
with dyadic coordinates and exact answers, and per mesh and map the max_distance values and the numpy references.  Everything is
built once per process and must not be modified by a test.

The hand box is, in the world, x in [0.75, 1.25], y in [1.5, 2.5], z in [0.375, 0.625] (body_cases)."""
import functools

import numpy as np

import body_cases as BC
import raycast_cases as RC
import voxelize_cases as VC
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import world as WO

INF = float("inf")
N = 256                                             # the first N boxes of body_cases.mesh_boxes / map_boxes

# name -> (triangle, the exact SQUARED distance to the hand box)
HAND = {
    # in the plane x = 4.25, covering the box's shadow (y + z <= 5 holds all of it): face to face
    "a parallel face at gap 3": ([[4.25, 0.0, 0.0], [4.25, 5.0, 0.0], [4.25, 0.0, 5.0]], 9.0),
    # its first vertex looks at the middle of the face x = 1.25 from half a metre
    "a vertex over a face": ([[1.75, 2.0, 0.5], [3.0, 1.75, 0.5], [3.0, 2.25, 0.5]], 0.25),
    # in the vertical plane 3 x + 4 y = 18.75, one metre along (0.6, 0.8, 0) from the box's edge x = 1.25, y = 2.5; the foot of each of
    # that edge's corners lies in the triangle's interior: n = (72, 96, 0), n . n = 14400, (s . n)^2 = 14400
    "a corner over the interior": ([[6.25, 0.0, -4.0], [-1.75, 6.0, -4.0], [2.25, 3.0, 8.0]], 1.0),
    # its first edge, (3.25, 3, 0.625) -> (1.25, 1, 2.625) along (1, 1, -1), passes (2.25, 2, 1.625): (1, 0, 1) away from the point
    # (1.25, 2, 0.625) of the box's edge x = 1.25, z = 0.625, and (1, 0, 1) is perpendicular to both edges: d2 = 2
    "edge to edge": ([[3.25, 3.0, 0.625], [1.25, 1.0, 2.625], [10.0, 2.0, 10.0]], 2.0),
}
MAX_DISTANCE_FAR = 1.0                              # "a parallel face at gap 3" and LARGE_AROUND are beyond it
# the plane x + y + z = 12.375 of body_cases' large triangles, moved 8 along x: the triangle's bounds hold the box, its plane is
# 8 / sqrt(3) away
LARGE_AROUND = [list(BC.CORNER + 64 * np.array(d) + np.array([8.0, 0.0, 0.0])) for d in ((1, -1, 0), (-1, 0, 1), (0, 1, -1))]


def triangle(tri):
    """-> float64 [1,3,3], exact in float32"""
    t = np.asarray(tri, np.float64)
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    return t[None]


# ---- max_distance per mesh: (D, a smaller one, a third); by the numpy reference D leaves at least MIN_SHARE of the N boxes in each of
# the three outcomes: hit, an accepted gap, beyond max_distance.  +inf runs on the two small meshes (the brute force over henge's 8 328
# faces without a bound takes the CPU 20 s).
MIN_SHARE = 0.10
MESH_MAX_DISTANCE = {"cube": (0.054, 0.02, INF), "henge": (0.2, 0.08, 0.5), "soup": (0.082, 0.03, INF)}
# per map of voxelize_cases: (the mesh whose map shows all three outcomes, D, a smaller one, a larger one: another reach of the
# candidate range and of the skip).  No mesh shows all three in "hand" (5 x 4 x 3 cells: HAND_HIT_SHARE of the boxes hit, whatever
# the mesh) nor in "miss" (an empty map: every box is beyond any max_distance); the tests assert exactly that there instead.
MAP_MAX_DISTANCE = {"hand": (None, 0.05, 0.02, 0.2), "around": ("henge", 0.35, 0.1, 0.6), "slab": ("cube", 0.33, 0.1, 0.6),
                    "cut": ("henge", 0.15, 0.05, 0.3), "miss": (None, 0.25, 0.1, 1.0), "odd": ("soup", 0.043, 0.015, 0.1),
                    "field": ("henge", 0.143, 0.05, 0.3)}
HAND_HIT_SHARE = 0.9


@functools.lru_cache(maxsize=None)
def mesh_clearance(name, rot, max_distance):
    """box_clearance_numpy of the first N of body_cases.mesh_boxes(name, rot): computed once, shared, read-only"""
    _, f, _ = RC.mesh(name)
    out = WO.box_clearance_numpy(BC.mesh_boxes(name, rot)[:N], VC.world_vertices(name, rot), f, max_distance)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def map_clearance(mesh, box, max_distance):
    """box_cells_clearance_numpy of the first N of body_cases.map_boxes(box) and its last four (the box that holds the map, the far
    one, the NaN row, the negative extent) on voxelize_cases' map of `mesh`: computed once, shared, read-only"""
    out = CO.box_cells_clearance_numpy(map_boxes(box), VC.reference(mesh, box), VC.BOXES[box], max_distance)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def map_boxes(box):
    b = np.concatenate([BC.map_boxes(box)[:N], BC.map_boxes(box)[-4:]])
    b.setflags(write=False)
    return b


def shares(out, key):
    """-> the shares of (hit, an accepted gap, beyond max_distance) among a result's boxes"""
    hit = out["hit"] >= 0
    gap = ~hit & np.isfinite(out["distance"])
    assert np.array_equal(out[key] >= 0, hit | gap)
    return float(hit.mean()), float(gap.mean()), float((~hit & ~gap).mean())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)
