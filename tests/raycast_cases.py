"""Shared meshes and rays of the ray-caster tests (test_raycast_cpu.py, test_raycast_gpu.py, test_world_gpu.py): the smallest that can
still go wrong.  Everything is built once per process and must not be modified by a test.

Meshes (name -> vertices float32 [V,3], faces int32 [F,3], colors float32 [V,3] or None):
    cube    the unit cube, 12 triangles: face k (x=0, x=1, y=0, y=1, z=0, z=1) is triangles 2k, 2k + 1, split along the diagonal from
            its (0, 0) corner to its (1, 1) corner -- the shared edge
    henge   scene.henge_mesh(24), a few thousand triangles
    soup    500 seeded triangles in the unit box: 478 random, ten zero-area (an edge from v0 is zero), ten exact duplicates of earlier
            ones (the same vertex indices, at higher face indices) and two that span the box
Rays per mesh (float32 [N,3] pairs; `sections` names slices of them):
    three 48 x 48 pinhole frames (from outside the box, from inside it, from a point in the plane of one of its faces looking along
    it) and about 256 hand-built rays: axis-parallel (through points on the face diagonals, edges and corners), lying in the
    cell-boundary planes of the automatic and of the (4,4,4) grid, through grid vertices, starting on the boundary, starting far away
    (50 box sizes: the grid walk; 5000: past the walk's reach), pointing away, through edge midpoints and vertices of the first faces,
    with a NaN or an infinite component, with a zero direction.
"""
import functools

import numpy as np

from nerfsafetyvalidation_amd import scene as SC
from nerfsafetyvalidation_amd import world as WO

f32 = np.float32
FRAME = 48
RESOLUTIONS = ((1, 1, 1), (4, 4, 4), (16, 7, 3), None)
N_TAILS = (1, 63, 64, 65)
ZERO_AREA = range(478, 488)
DUPLICATES = range(488, 498)        # face 488 + i repeats face DUPLICATE_OF[i]
DUPLICATE_OF = tuple(range(7, 457, 45))
LARGE = (498, 499)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], f32)       # vertex index = 4x + 2y + z
    idx = lambda x, y, z: 4 * x + 2 * y + z
    faces = []
    for axis in range(3):
        for side in (0, 1):
            def corner(a, b):
                p = [0, 0, 0]
                p[axis] = side
                p[(axis + 1) % 3], p[(axis + 2) % 3] = a, b
                return idx(*p)
            faces += [[corner(0, 0), corner(1, 0), corner(1, 1)], [corner(0, 0), corner(1, 1), corner(0, 1)]]
    return v, np.array(faces, np.int32), None


def soup():
    rng = np.random.default_rng(20240611)
    verts, faces = [], []
    for _ in range(478):
        c = rng.uniform(0.1, 0.9, 3)
        tri = c + rng.uniform(-0.12, 0.12, (3, 3))
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts += list(np.clip(tri, 0, 1))
    for i in range(10):                                   # zero area: e1 = 0, e2 = 0, or both
        a, b = rng.uniform(0.2, 0.8, 3), rng.uniform(0.2, 0.8, 3)
        n = len(verts)
        verts += [a, b]
        faces.append([[n, n, n + 1], [n, n + 1, n], [n, n, n]][i % 3])
    for src in DUPLICATE_OF:
        faces.append(list(faces[src]))
    n = len(verts)
    verts += [[0, 0, 0.4], [1, 0, 0.45], [0.5, 1, 0.5], [0.3, 0, 0], [0.35, 1, 0.5], [0.3, 0, 1]]
    faces += [[n, n + 1, n + 2], [n + 3, n + 4, n + 5]]
    v = np.asarray(verts, f32)
    colors = rng.uniform(0, 1, v.shape).astype(f32)
    return v, np.asarray(faces, np.int32), colors


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "cube":
        return cube()
    if name == "soup":
        return soup()
    if name == "henge":
        return SC.henge_mesh(24)
    raise KeyError(name)


MESHES = ("cube", "henge", "soup")


def pinhole(origin, forward, up, H=FRAME, W=FRAME, angle=1.0):
    """unit-direction rays of an H x W pinhole camera, row-major, pixel centres -> (o, d) float32 [H W, 3]"""
    fwd = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    fl = W / (2 * np.tan(angle / 2))
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = ((i.reshape(-1, 1) - W / 2) / fl) * right + ((j.reshape(-1, 1) - H / 2) / fl) * down + fwd
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.asarray(origin, f32), (H * W, 1)), d.astype(f32)


def _hand_rays(v, faces):
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext, mid = hi - lo, (lo + hi) / 2
    size = float(ext.max())
    o, d, tags = [], [], []

    def add(tag, org, direction):
        o.append(np.asarray(org, np.float64))
        d.append(np.asarray(direction, np.float64))
        tags.append(tag)

    # axis-parallel: through points (a, a) of the other two axes -- on the face diagonals, the box's edges and corners
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for frac in (0.0, 0.25, 0.5, 0.75, 1.0, 0.3, 0.77, 0.123):
            for sign in (1.0, -1.0):
                p = np.zeros(3)
                p[b], p[c] = lo[b] + frac * ext[b], lo[c] + frac * ext[c]
                p[a] = lo[a] - 0.5 * size if sign > 0 else hi[a] + 0.5 * size
                e = np.zeros(3)
                e[a] = sign
                add("axis", p, e)
    # in the cell-boundary planes of two grids: one coordinate exactly on a plane, no motion along that axis
    for res in (None, (4, 4, 4)):
        g = WO.grid_params(v.min(0), v.max(0), len(faces), res)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for k in sorted({0, 1, int(g["n"][a]) // 2, int(g["n"][a])}):
                p, e = np.zeros(3), np.zeros(3)
                p[a] = f32(g["lo"][a] + f32(k) * g["cell"][a])
                p[b], p[c] = lo[b] - 0.4 * size, mid[c] + 0.11 * ext[c]
                e[b], e[c] = 1.0, 0.07
                add("plane", p, e)
        # through grid vertices, from outside
        n = g["n"]
        for k in range(20):
            cell = np.array([(5 * k + 1) % (n[0] + 1), (3 * k + 2) % (n[1] + 1), (7 * k) % (n[2] + 1)])
            target = (g["lo"] + cell.astype(f32) * g["cell"]).astype(np.float64)
            org = mid + size * np.array([1.3, 0.9, -1.1]) * (1 if k % 2 else -1)
            add("vertex", org, target - org)
    # starting on the bounding box, pointing in
    for a in range(3):
        for side in (0, 1):
            for k in range(4):
                p = lo + ext * np.array([0.21 + 0.17 * k, 0.63 - 0.13 * k, 0.35 + 0.11 * k])
                p[a] = lo[a] if side == 0 else hi[a]
                e = mid - p + 0.05 * size
                add("boundary", p, e)
    # far away (the grid walk at 50 box sizes, every triangle at 5000), aimed into the box
    for k in range(32):
        w = np.array([np.cos(1.0 + 2.4 * k), np.sin(0.3 + 1.7 * k), np.cos(2.0 + 0.9 * k)])
        w /= np.linalg.norm(w)
        dist = 5000.0 if k % 4 == 3 else 50.0
        target = lo + ext * np.array([(0.37 * k) % 1, (0.61 * k) % 1, (0.83 * k) % 1])
        org = target + w * dist * size
        add("far", org, -w if k % 2 else (target - org))
    # pointing away from the mesh
    for k in range(24):
        w = np.array([np.cos(0.7 * k), np.sin(1.1 * k), np.cos(1.9 * k + 1)])
        org = mid + (0.8 + 0.2 * (k % 3)) * size * w / np.linalg.norm(w)
        add("away", org, org - mid)
    # through the edge midpoints and the first vertex of the first faces (shared edges and vertices)
    for k in range(12):
        tri = v[faces[k % len(faces)]].astype(np.float64)
        org = mid + size * np.array([0.9, 1.7, -1.3])
        for target in (tri[0], (tri[0] + tri[1]) / 2, (tri[1] + tri[2]) / 2, (tri[0] + tri[2]) / 2):
            add("shared", org, target - org)
    # not rays at all: misses before any loop
    for k in range(4):
        p, e = mid + size * np.array([0.0, 0.0, -2.0]), np.array([0.01 * k, 0.02, 1.0])
        if k % 2:
            p[k % 3] = np.nan
        else:
            e[k % 3] = np.nan
        add("nan", p, e)
    add("nan", mid + [np.inf, 0, 0], [-1.0, 0, 0])
    add("nan", mid - [0, 0, 2 * size], [0, np.inf, 1.0])
    for k in range(4):
        add("zero", mid if k % 2 else lo - size, [0.0, -0.0, 0.0])
    return np.asarray(o).astype(f32), np.asarray(d).astype(f32), tags


@functools.lru_cache(maxsize=None)
def rays(name):
    """-> (rays_o, rays_d float32 [N,3], sections: name -> slice, tags of the hand rays)"""
    v, faces, _ = mesh(name)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext, mid = hi - lo, (lo + hi) / 2
    size = float(ext.max())
    frames = [pinhole(mid + size * np.array([1.1, 0.8, -1.4]), -np.array([1.1, 0.8, -1.4]), [0.0, 1.0, 0.0]),
              pinhole(mid + ext * np.array([0.05, 0.1, -0.03]), [0.6, -0.3, 0.74], [0.0, 1.0, 0.0], angle=1.6),
              pinhole([mid[0] - 0.9 * ext[0], hi[1], mid[2] + 0.1 * ext[2]], [1.0, 0.0, -0.05], [0.0, 1.0, 0.0], angle=0.9)]
    ho, hd, tags = _hand_rays(v, faces)
    o = np.concatenate([f[0] for f in frames] + [ho])
    d = np.concatenate([f[1] for f in frames] + [hd])
    n = FRAME * FRAME
    sections = {"outside": slice(0, n), "inside": slice(n, 2 * n), "grazing": slice(2 * n, 3 * n), "hand": slice(3 * n, 3 * n + len(ho))}
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d, sections, tuple(tags)


@functools.lru_cache(maxsize=None)
def tri_data(name):
    v, faces, _ = mesh(name)
    t = WO.pack_triangles(v, faces)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference(name):
    """the numpy path's result on all of rays(name): computed once, shared, read-only"""
    o, d, _, _ = rays(name)
    out = WO.cast_numpy(o, d, tri_data(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
