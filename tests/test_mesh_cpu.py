"""mesh.py's numpy path (the package's CPU path of isosurface) and the export chain around it: no GPU.

Analytic fields on index coordinates; every bound below is derived in its test, none is taken from what the code gives."""
import os
import struct

import numpy as np
import pytest
import torch

import mesh_fields as MF
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import mesh as M


def _mesh(u, thr=0.0):
    v, f = M.isosurface(u, thr)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v, f


# ------------------------------------------------------------------ closed surfaces
@pytest.mark.parametrize("field,euler", [(MF.sphere, 2), (MF.two_spheres, 4), (MF.torus, 0)])
def test_closed_surfaces(field, euler):
    v, f = _mesh(field())
    MF.assert_closed(v, f, euler)


def test_sphere_accuracy():
    """|u| is a distance (|grad u| = 1) and a lattice edge is at most sqrt(3) long, so both of a crossing edge's ends are within
    sqrt(3) of the sphere and the field's second derivative along the edge is at most the curvature 1 / (r0 - sqrt(3)) there.  Linear
    interpolation over a length h <= sqrt(3) is then off by at most h^2 / 8 * curvature = 3 / (8 (r0 - sqrt(3))) in u, i.e. in
    distance; 1e-4 covers the fp32 roundings (2^-23 * 20)."""
    c, r0 = 9.3, 6.0
    v, _ = _mesh(MF.sphere(centre=(c, c, c), radius=r0))
    err = np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r0)
    print("sphere: max | |v - c| - r0 | =", err.max())
    assert err.max() <= 3 / (8 * (r0 - np.sqrt(3))) + 1e-4


# ------------------------------------------------------------------ plane
def _clip_plane_box(n, d, hi):
    """area of {x in [0, hi]^3 : n.x = d} in float64: a large square in the plane, clipped by the six half-spaces"""
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    o, s = n * d, 10.0 * hi
    poly = [o + s * (i * a + j * b) for i, j in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    for axis in range(3):
        for sign, bound in ((1.0, 0.0), (-1.0, -hi)):       # keep sign * x[axis] >= bound
            out = []
            for k in range(len(poly)):
                p, q = poly[k], poly[(k + 1) % len(poly)]
                fp, fq = sign * p[axis] - bound, sign * q[axis] - bound
                if fp >= 0:
                    out.append(p)
                if (fp >= 0) != (fq >= 0):
                    out.append(p + (q - p) * (fp / (fp - fq)))
            poly = out
    poly = np.array(poly)
    return 0.5 * abs(np.dot(n, sum(np.cross(poly[k], poly[(k + 1) % len(poly)]) for k in range(len(poly)))))


def test_plane():
    """u = n.x + c with |n| = 1 is linear, so interpolation is exact up to rounding: the stored u is off by 2^-24 |u| <= 2^-24 sqrt(3) R,
    t by a few 2^-24 (times an edge of length <= sqrt(3)), the coordinate by 2^-24 R: within 8 R 2^-23 together.  The triangles tile
    the plane's cut through the box, so their areas add up to the polygon's."""
    R = 12
    n = np.array([0.31, -0.52, 0.79])
    n /= np.linalg.norm(n)
    thr = 0.25
    c = thr - float(n @ np.array([5.3, 6.1, 4.9]))          # the plane n.x + c = thr passes through (5.3, 6.1, 4.9)
    u = (MF.lattice((R, R, R)) @ n + c).astype(np.float32)
    v, f = _mesh(u, thr)
    v64 = v.astype(np.float64)
    resid = np.abs(v64 @ n + c - thr)
    print("plane: max distance", resid.max(), "bound", 8 * R * 2.0 ** -23)
    assert resid.max() <= 8 * R * 2.0 ** -23
    tri = v64[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    want = _clip_plane_box(n, thr - c, R - 1.0)
    print("plane: area", area, "polygon", want)
    assert abs(area - want) <= 1e-4 * want
    # normals point from inside (u > thr) to outside: against the gradient
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (normals @ n < 0).all()


# ------------------------------------------------------------------ open surfaces, coverage
def test_open_surface_on_a_random_field():
    shape = (17, 13, 9)
    u = MF.random_field(shape, 17)
    v, f = _mesh(u)
    owners, types = M.vertex_edges(u, 0.0)
    assert len(owners) == len(v)
    assert MF.assert_open_only_at_the_boundary(shape, owners, types, f, M.EDGE_OFFSETS) > 0


def test_all_256_corner_configurations():
    u = MF.random_field(MF.ALL_CONFIG_SHAPE, MF.ALL_CONFIG_SEED)
    assert max(u.shape) <= 17
    assert len(np.unique(MF.corner_configurations(u, 0.0))) == 256
    v, f = _mesh(u)
    owners, types = M.vertex_edges(u, 0.0)
    MF.assert_open_only_at_the_boundary(u.shape, owners, types, f, M.EDGE_OFFSETS)
    # every vertex on its own lattice edge, between the ends, and every end pair straddles the threshold
    off = np.asarray(M.EDGE_OFFSETS)[types]
    assert ((v >= owners) & (v <= owners + off)).all()
    ua = u[tuple(owners.T)]
    ub = u[tuple((owners + off).T)]
    assert ((ua > 0) != (ub > 0)).all()
    # welded: as many vertices as crossing edges, no two on one edge
    assert len(np.unique(np.concatenate([owners, types[:, None]], 1), axis=0)) == len(v)
    # the mesh of -u is the same surface turned inside out: the same vertices (negating both operands of a subtraction or a
    # division changes no bit), the same triangles as vertex sets, every directed edge reversed
    v2, f2 = _mesh(-u, 0.0)
    assert np.array_equal(v2, v)
    rows = lambda a: set(map(tuple, np.asarray(a).tolist()))       # noqa: E731
    assert rows(np.sort(f2, axis=1)) == rows(np.sort(f, axis=1))
    directed = lambda a: rows(np.concatenate([a[:, [0, 1]], a[:, [1, 2]], a[:, [2, 0]]]))      # noqa: E731
    assert directed(f2) == directed(f[:, ::-1])


# ------------------------------------------------------------------ corner cases
@pytest.mark.parametrize("corner", range(8))
def test_one_corner_inside(corner):
    """a single cell: the corner's edges in the Kuhn split go to the corners whose offset code contains or is contained in its own --
    all 7 for (0,0,0) and (1,1,1), 4 for the others; it lies in 6 or 2 of the tetrahedra, one triangle each"""
    u = np.zeros((2, 2, 2), dtype=np.float32)
    c = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
    u[tuple(c)] = 1.0
    v, f = _mesh(u, 0.5)
    assert (len(v), len(f)) == ((7, 6) if corner in (0, 7) else (4, 2))
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    tri = v.astype(np.float64)[f]
    normals = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", normals, tri.mean(1) - c) > 0).all()        # away from the inside corner
    # u is 1 at the corner and 0 at the other end: every vertex is the midpoint of its edge
    assert np.array_equal(np.abs(v - c).max(1), np.full(len(v), 0.5, dtype=np.float32))


def test_thin_lattice():
    shape = (2, 5, 3)
    u = MF.random_field(shape, 3)
    v, f = _mesh(u)
    owners, types = M.vertex_edges(u, 0.0)
    assert len(v) == len(owners) > 0
    MF.assert_open_only_at_the_boundary(shape, owners, types, f, M.EDGE_OFFSETS)


def test_empty_surfaces_and_strictness():
    for u in (np.full((3, 4, 5), -1.0, np.float32), np.full((3, 4, 5), 1.0, np.float32), np.zeros((3, 4, 5), np.float32)):
        v, f = _mesh(u, 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    # a value equal to the threshold is outside: one point above it among points AT it is a closed surface through its neighbours
    u = np.full((3, 3, 3), 2.0, np.float32)
    u[1, 1, 1] = 3.0
    v, f = _mesh(u, 2.0)
    MF.assert_closed(v, f, 2)
    assert np.array_equal(np.abs(v - 1.0).max(1), np.ones(len(v), dtype=np.float32))     # t = 1: on the outside neighbour itself
    vt, ft = M.isosurface(torch.from_numpy(u), 2.0)
    assert isinstance(vt, torch.Tensor) and np.array_equal(vt.numpy(), v) and np.array_equal(ft.numpy(), f)


def test_nan_is_outside_and_inf_raises():
    u = MF.sphere()
    w = u.copy()
    hole = (5, 9, 9)
    assert u[hole] > 0
    w[hole] = np.nan
    low = u.copy()
    low[hole] = -1.0
    v, f = _mesh(w)
    v_low, f_low = _mesh(low)
    assert np.array_equal(f, f_low) and v.shape == v_low.shape
    for bad in (np.inf, -np.inf):
        w[hole] = bad
        with pytest.raises(ValueError):
            M.isosurface(w, 0.0)
    with pytest.raises(ValueError):
        M.isosurface(np.zeros((1, 4, 4), np.float32), 0.0)


def test_non_contiguous_input():
    u = MF.random_field((6, 7, 8), 5)
    v, f = _mesh(u)
    v2, f2 = _mesh(np.asfortranarray(u))
    v3, f3 = _mesh(u.transpose(2, 1, 0).copy().transpose(2, 1, 0))
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and np.array_equal(v, v3) and np.array_equal(f, f3)


# ------------------------------------------------------------------ export and chain
def _query(pts):
    # products and sums only: each is one IEEE operation per element however the batch is cut
    return pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 2] - 0.3 * pts[:, 0]


def test_extract_fields_crosses_chunk_edges():
    lo, hi = torch.tensor([-1.0, -0.5, 0.25]), torch.tensor([1.5, 2.0, 0.75])
    calls = []

    def q(pts):
        calls.append(pts.shape)
        return _query(pts)
    u = M.extract_fields(lo, hi, 5, q, S=2)
    assert u.dtype == torch.float32 and u.shape == (5, 5, 5) and len(calls) == 27 and max(c[0] for c in calls) == 8
    axes = [torch.linspace(float(lo[d]), float(hi[d]), 5) for d in range(3)]
    g = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(u, _query(g).reshape(5, 5, 5))


def test_extract_geometry_scales_like_the_reference():
    lo, hi = torch.tensor([-1.0, -0.5, 0.25]), torch.tensor([1.5, 2.0, 0.75])
    R = 9
    verts, tris = M.extract_geometry(lo, hi, R, 0.1, _query)
    v, f = M.isosurface(M.extract_fields(lo, hi, R, _query), 0.1)
    assert verts.dtype == np.float64 and tris.dtype == np.int32 and len(verts) > 0
    b_min, b_max = lo.numpy(), hi.numpy()
    want = v.numpy().astype(np.float64) / (R - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    assert np.array_equal(verts, want) and np.array_equal(tris, f.numpy())


class _Blob(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("aabb_infer", torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.5, 2.0]))

    def density(self, x):
        return {"sigma": 20.0 * torch.exp(-((x - torch.tensor([0.1, 0.2, 0.4])) ** 2).sum(-1) * 3.0)}


def test_save_mesh_ply_round_trip(tmp_path):
    path = os.path.join(tmp_path, "meshes", "blob.ply")
    verts, tris = M.save_mesh(_Blob(), path, resolution=24, threshold=10)
    MF.assert_closed(verts, tris, 2)
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert [ln for ln in lines if ln.startswith("property")] == ["property float x", "property float y", "property float z",
                                                                "property list uchar int vertex_indices"]
    assert (nv, nf) == (len(verts), len(tris)) and len(body) == 12 * nv + 13 * nf
    got_v = np.array(struct.unpack(f"<{3 * nv}f", body[:12 * nv])).reshape(nv, 3)
    assert np.array_equal(got_v.astype(np.float32), verts.astype(np.float32))
    for k in (0, nf // 2, nf - 1):
        rec = struct.unpack("<Biii", body[12 * nv + 13 * k:12 * nv + 13 * (k + 1)])
        assert rec[0] == 3 and list(rec[1:]) == list(tris[k])


def test_mesh_to_world_inverts_to_nerf():
    w = torch.from_numpy(np.random.default_rng(1).standard_normal((50, 3))).float()
    assert torch.equal(M.mesh_to_world(CO.to_nerf(w, CO.PLANNER_ROT)), w)
    assert np.array_equal(M.mesh_to_world(CO.to_nerf(w, CO.PLANNER_ROT).numpy()), w.numpy().astype(np.float64))
    assert M.mesh_to_world(np.array([[1.0, 2.0, 3.0]])).tolist() == [[3.0, 1.0, 2.0]]       # NeRF (x, y, z) = world (y, z, x)


def test_sphere_mesh_marks_the_cells_that_hold_a_vertex():
    """createCollisionMap.py's rule on the mesh: mesh -> world frame -> occupancy_from_points"""
    v, _ = _mesh(MF.sphere())
    nerf = v.astype(np.float64) / 19.0 * 1.2 - 0.6          # the lattice over [-0.6, 0.6]^3 in the NeRF's axes
    world = M.mesh_to_world(nerf)
    box = CO.GridBox((-0.7, -0.7, -0.7), 10, (14, 14, 14))
    occ = CO.occupancy_from_points(world, box).numpy()
    cells = np.floor((world - np.array(box.start)) * box.granularity).astype(np.int64)
    assert ((cells >= 0) & (cells < 14)).all()
    want = np.zeros(box.shape, dtype=bool)
    want[tuple(cells.T)] = True
    assert np.array_equal(occ, want) and 0 < occ.sum() < occ.size
    assert world[:, 0] == pytest.approx(nerf[:, 2]) and world[:, 1] == pytest.approx(nerf[:, 0])
