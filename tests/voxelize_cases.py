"""Shared boxes and numpy references of the voxeliser tests (test_voxelize_cpu.py, test_voxelize_gpu.py): the meshes are
raycast_cases' (cube, henge, soup -- soup holds the zero-area and the duplicate faces); everything is built once per process and
must not be modified by a test.

Boxes (world frame).  The dyadic ones have start and granularity that are sums of a few powers of two, so the float64 cell geometry
is exact and hand answers are unambiguous; `odd` has test_collision_gpu's granularity and shape and nothing exact about it (the centres'
division rounds).  With PLANNER_ROT the unit-box meshes lie in the world's unit box too (a permutation of the axes).
"""
import functools

import raycast_cases as RC
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import world as WO

IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
ROTS = {"planner": CO.PLANNER_ROT, "identity": IDENTITY}

BOXES = {
    "hand": CO.GridBox((-0.5, -0.25, 0.0), 4, (5, 4, 3)),             # the hand tests' box: 0.25 m cells, cuts the unit box
    "around": CO.GridBox((-0.125, -0.125, -0.125), 8, (10, 10, 10)),  # holds the unit box with a cell to spare
    "slab": CO.GridBox((-1.0, -0.5, -0.25), 8, (16, 7, 3)),           # three different sizes, none a multiple of another
    "cut": CO.GridBox((0.25, -0.25, -0.125), 16, (12, 9, 10)),        # cuts every mesh
    "miss": CO.GridBox((5.0, 5.0, 5.0), 4, (3, 4, 5)),                # holds no mesh
    "odd": CO.GridBox((0.21, -0.11, -0.07), 37.3, (11, 9, 7)),
    "field": CO.GridBox((-1.0, -1.0, -0.5), 16, (32, 32, 12)),        # holds the henge: the distance field and the ray check
}
SMALL = ("hand", "around", "slab")                                    # few enough cells for the brute force over all of them


def world_vertices(name, rot):
    v, _, _ = RC.mesh(name)
    return WO.vertices_to_world(v, ROTS[rot])


@functools.lru_cache(maxsize=None)
def reference(name, box, rot="planner"):
    """voxelize_numpy's map of mesh `name` in BOXES[box]: computed once, shared, read-only"""
    _, f, _ = RC.mesh(name)
    occ = WO.voxelize_numpy(world_vertices(name, rot), f, BOXES[box])
    occ.setflags(write=False)
    return occ
