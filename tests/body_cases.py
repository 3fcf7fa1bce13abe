"""Shared inputs of the body-collision tests (test_body_cpu.py, test_body_gpu.py): hand cases with dyadic coordinates, whose answers
are written down here by hand, and seeded box tables for the meshes of raycast_cases and the maps of voxelize_cases.  Everything is
built once per process and must not be modified by a test.

The hand box.  c = (1, 2, 0.5), h = (0.5, 0.25, 0.125), R a quarter turn about z: the box's x axis is the world's y, its y axis the
world's -x.  In the world it is therefore the axis-aligned box x in [0.75, 1.25], y in [1.5, 2.5], z in [0.375, 0.625]; every
coordinate below is a short sum of powers of two, so float32 holds the vertices and float64 evaluates the rule without rounding.
OFF = 2^-20 is the "one dyadic step": the touching triangles moved by it along +x no longer touch."""
import functools

import numpy as np

import raycast_cases as RC
import voxelize_cases as VC
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import world as WO

f32 = np.float32
OFF = 2.0 ** -20
QUARTER_Z = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
HAND_BOX = np.array([1.0, 2.0, 0.5] + [v for row in QUARTER_Z for v in row] + [0.5, 0.25, 0.125], np.float64)
CORNER = np.array([1.25, 2.5, 0.625])          # the box's (+x, +y, +z) corner in the world
CENTRE = np.array([1.0, 2.0, 0.5])


def _shift(tri, dx):
    return [[p[0] + dx, p[1], p[2]] for p in tri]


_FACE = [[1.25, 2.0, 0.5], [2.0, 1.75, 0.5], [2.0, 2.25, 0.5]]                      # a vertex on the face x = 1.25, the rest beyond it
_EDGE = [[1.5, 2.25, 0.5], [1.0, 2.75, 0.5], [1.5, 2.75, 0.5]]                      # its first edge crosses the box's edge x = 1.25, y = 2.5 at
#                                                                                    (1.25, 2.5): x + y >= 3.75 on the triangle, <= 3.75 on the box
_CORNER = [list(CORNER + 0.5 * np.array(d)) for d in ((1, -1, 0), (-1, 0, 1), (0, 1, -1))]      # in the plane x + y + z = 4.375 around the
#                                                                                    corner, its centroid: only the normal axis decides
_LARGE_TOUCH = [list(CORNER + 64 * np.array(d)) for d in ((1, -1, 0), (-1, 0, 1), (0, 1, -1))]  # the same plane, vertices 64 away
_LARGE_THROUGH = [list(CENTRE + 64 * np.array(d)) for d in ((1, -1, 0), (-1, 0, 1), (0, 1, -1))]  # through the centre: the box lies in
#                                                                                    the triangle's interior region, far from every edge
# name -> (triangle [3 vertices][3], overlaps the hand box)
HAND = {
    "touches a face": (_FACE, True),
    "off the face": (_shift(_FACE, OFF), False),
    "touches an edge": (_EDGE, True),
    "off the edge": (_shift(_EDGE, OFF), False),
    "touches a corner": (_CORNER, True),
    "off the corner": (_shift(_CORNER, OFF), False),
    "large, touches the corner through its interior": (_LARGE_TOUCH, True),
    "large, off the corner": (_shift(_LARGE_TOUCH, 2.0 ** -10), False),             # (float32 at 64 resolves 2^-17)
    "large, the box in its interior region": (_LARGE_THROUGH, True),
    "wholly inside the box": ([[1.0, 2.0, 0.5], [1.125, 2.125, 0.5], [1.0, 2.125, 0.5625]], True),
    "zero area: a segment through the box": ([[0.0, 2.0, 0.5], [2.0, 2.0, 0.5], [2.0, 2.0, 0.5]], True),
    "zero area: a point in the box": ([[1.0, 2.0, 0.5]] * 3, True),
    "zero area: a point on the box's face": ([[1.25, 2.0, 0.5]] * 3, True),
    "zero area: a segment beside the box": ([[1.25 + OFF, 1.0, 0.5], [1.25 + OFF, 3.0, 0.5], [1.25 + OFF, 3.0, 0.5]], False),
    "zero area: a point off the face": ([[1.25 + OFF, 2.0, 0.5]] * 3, False),
    "far away": ([[5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [5.0, 6.0, 5.0]], False),
}


def hand_triangle(name):
    """-> (vertices float32 [3,3], faces int32 [1,3]) of one hand case; the float32 copy is exact"""
    tri = np.asarray(HAND[name][0], np.float64)
    v = tri.astype(f32)
    assert np.array_equal(v.astype(np.float64), tri), name
    return v, np.array([[0, 1, 2]], np.int32)


@functools.lru_cache(maxsize=None)
def hand_mesh():
    """every hand triangle in one mesh, in HAND's order, then the first one again (a duplicate at a higher index) -> (vertices, faces)"""
    v = np.concatenate([hand_triangle(n)[0] for n in HAND] + [hand_triangle(next(iter(HAND)))[0]])
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    v.setflags(write=False)
    return v, f


def hand_boxes():
    """-> (boxes float64 [5,15], the prim each has in hand_mesh()): the hand box (face 0 touches it: the lowest index wins over its
    duplicate, the last face); the hand box with a NaN, with an infinite centre and with a negative half extent (-1 each); and the hand
    box moved 8 along -x, which only the segment through y = 2, z = 0.5 (x in [0, 2]) could reach -- it ends at x = 0: -1"""
    names = list(HAND)
    b = np.tile(HAND_BOX, (5, 1))
    b[1, 7] = np.nan
    b[2, 0] = np.inf
    b[3, 13] = -0.25
    b[4, 0] -= 8.0
    return b, np.array([0, -1, -1, -1, -1], np.int32), names


# ---- seeded boxes for a mesh: centres drawn around the mesh's world bounds, rotations from a normal rotation vector
def random_boxes(lo, hi, n, seed, half=(0.05, 0.05, 0.02), spread=0.15):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    centres = rng.uniform(lo - spread * ext, hi + spread * ext, (n, 3))
    states = np.concatenate([centres, rng.normal(0.0, 1.0, (n, 3))], 1)
    body = CO.BodyBox([[-h, h] for h in half])
    return CO.body_boxes(states, body)


MESH_HALF = {"cube": (0.06, 0.05, 0.03), "henge": (0.12, 0.12, 0.05), "soup": (0.06, 0.05, 0.03)}    # so that about a third of the boxes hit
HIT_SHARE = (0.25, 0.45)                            # the tests assert the share of mesh_reference's hits lies in here
N_BOXES = 1000


@functools.lru_cache(maxsize=None)
def mesh_boxes(name, rot):
    """1 000 seeded boxes around mesh `name` in the world frame of VC.ROTS[rot], with a NaN row and a negative-extent row among them"""
    vw = VC.world_vertices(name, rot).astype(np.float64)
    b = random_boxes(vw.min(0), vw.max(0), N_BOXES, 7 + len(name), MESH_HALF[name])
    b[17, 4] = np.nan
    b[400, 12] = -1e-3
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def mesh_reference(name, rot):
    """box_overlap_numpy's prim of mesh_boxes(name, rot): computed once, shared, read-only"""
    _, f, _ = RC.mesh(name)
    prim = WO.box_overlap_numpy(mesh_boxes(name, rot), VC.world_vertices(name, rot), f)["prim"]
    prim.setflags(write=False)
    return prim


@functools.lru_cache(maxsize=None)
def map_boxes(box):
    """1 000 seeded boxes around map VC.BOXES[box] (some straddle its faces), then one that contains the whole map, one far outside
    it, a NaN row and a negative-extent row; the half extents are two and a half, one and a half and one cell"""
    B = VC.BOXES[box]
    lo = np.asarray(B.start)
    hi = lo + np.asarray(B.shape) / B.granularity
    cellw = 1.0 / B.granularity
    b = random_boxes(lo, hi, N_BOXES, 11 + len(box), (2.5 * cellw, 1.5 * cellw, cellw), spread=0.1)
    whole = np.concatenate([(lo + hi) / 2, np.eye(3).reshape(-1), (hi - lo)])
    far = np.concatenate([hi + 10.0, np.eye(3).reshape(-1), [cellw] * 3])
    bad = np.tile(whole, (2, 1))
    bad[0, 1], bad[1, 14] = np.nan, -cellw
    b = np.concatenate([b, whole[None], far[None], bad])
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def map_reference(mesh, box):
    """box_cells_numpy's cell of map_boxes(box) on voxelize_cases' map of `mesh`: computed once, shared, read-only"""
    cell = CO.box_cells_numpy(map_boxes(box), VC.reference(mesh, box), VC.BOXES[box])
    cell.setflags(write=False)
    return cell
