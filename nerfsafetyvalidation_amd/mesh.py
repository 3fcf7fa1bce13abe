"""The NeRF's density as a triangle mesh: Trainer.save_mesh -> extract_geometry -> extract_fields of the reference
(nerf/utils.py:152-182, 533-551), with the field-to-surface step (mcubes there) as HIP kernels.

    extract_fields     the density on a resolution^3 lattice, S^3 points per query, kept on the device the values come from
    isosurface         lattice -> (vertices [V,3] float32 in index units, faces [F,3] int32)
                         CUDA tensor: ngp_isosurface_count / ngp_isosurface_emit (csrc/mesh.hip)
                         CPU tensor / numpy array: the same rule and order in numpy (the package's CPU path)
    extract_geometry   extract_fields + isosurface + the reference's scaling to the bounds
    save_mesh          extract_geometry of model.density over model.aabb_infer, written as a binary PLY
    write_ply/read_ply the binary PLY (optionally with uchar vertex colours) and its reader
    mesh_to_world      NeRF axes -> the world frame of collision.py's boxes (the inverse of collision.to_nerf)

The rule (DESIGN.md "Mesh export"): marching tetrahedra on the Kuhn split.  A lattice point is inside iff u > threshold (strict;
NaN is outside).  Every cell is cut into the six tetrahedra around its (0,0,0)-(1,1,1) diagonal -- for the permutation (a, b, c) of
the axes, in lexicographic order, tetrahedron k is {corner, +e_a, +e_a+e_b, +(1,1,1)} -- the same cut on both sides of every cell
face, so the surface has no cracks and no ambiguous case.  Their edges are the 7 lattice edges with an offset in {0,1}^3 \\ 0, owned
by the lower end: EDGE_OFFSETS, type 0..6.  An edge whose ends differ carries one vertex, t = (thr - ua) / (ub - ua),
v = pa + t * (pb - pa) with a the owner, in fp32 with one rounding per operation.  Vertices are ordered by (owner in C order, edge
type), faces by (cell in C order, tetrahedron, triangle); triangle normals (right-hand rule) point from inside to outside.

With collision.py the mesh feeds the reference's createCollisionMap.py -> createSDF.py chain:
    occ = collision.occupancy_from_points(mesh_to_world(vertices), box); SignedDistanceField.from_occupancy(occ, box)
"""
import itertools
import os
import struct

import numpy as np
import torch

from . import _lib
from .collision import PLANNER_ROT

# edge type -> lattice offset (dx, dy, dz): 3 axis edges, 3 face diagonals, the body diagonal
EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# tetrahedron k of a cell: corner, +e_a, +e_a+e_b, +(1,1,1) for the k-th permutation (a, b, c) in lexicographic order
TET_PERMUTATIONS = tuple(itertools.permutations(range(3)))


def _code(offset):
    """corner offset -> 3-bit code (bit 0 = x, bit 1 = y, bit 2 = z)"""
    return offset[0] | (offset[1] << 1) | (offset[2] << 2)


def _offset(code):
    return (code & 1, (code >> 1) & 1, (code >> 2) & 1)


_TYPE_OF_CODE = {_code(o): t for t, o in enumerate(EDGE_OFFSETS)}


def _derive_tables():
    """The 16-case table of every tetrahedron, derived from the geometry (as csrc/mesh.hip's make_iso_tables derives its own copy):
    the tetrahedron's corners at their lattice offsets, crossings at edge midpoints, every triangle turned so that its normal has a
    positive component along (centroid of the outside corners) - (centroid of the inside corners).
    -> tets [6][4] corner codes, ntri [16], tris [6][16] lists of triangles of three (owner corner code, edge type)"""
    tets, tris = [], []
    ntri = [{0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(c).count("1")] for c in range(16)]
    for a, b, _ in TET_PERMUTATIONS:
        codes = [0, 1 << a, (1 << a) | (1 << b), 7]
        P = np.array([_offset(c) for c in codes], dtype=np.int64)
        per_case = []
        for case in range(16):
            inside = [i for i in range(4) if (case >> i) & 1]
            outside = [i for i in range(4) if not (case >> i) & 1]
            if len(inside) in (0, 4):
                per_case.append([])
                continue
            if len(inside) == 1:
                cut = [[(inside[0], o) for o in outside]]
            elif len(inside) == 3:
                cut = [[(outside[0], i) for i in inside]]
            else:       # the quad (i0 o0) (i0 o1) (i1 o1) (i1 o0), cut along (i0 o0)-(i1 o1)
                (i0, i1), (o0, o1) = inside, outside
                cut = [[(i0, o0), (i0, o1), (i1, o1)], [(i0, o0), (i1, o1), (i1, o0)]]
            direction = len(inside) * P[outside].sum(0) - len(outside) * P[inside].sum(0)
            out = []
            for tri in cut:
                m = [P[i] + P[j] for i, j in tri]
                if np.dot(np.cross(m[1] - m[0], m[2] - m[0]), direction) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                # the corner codes form a chain under inclusion: an edge's lower end is the AND of its ends
                out.append([(codes[i] & codes[j], _TYPE_OF_CODE[codes[i] ^ codes[j]]) for i, j in tri])
            per_case.append(out)
        tets.append(codes)
        tris.append(per_case)
    return tets, ntri, tris


_TETS, _NTRI, _TRIS = _derive_tables()
_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _as_field(u):
    u = np.ascontiguousarray(u, dtype=np.float32)
    if u.ndim != 3 or min(u.shape) < 2:
        raise ValueError(f"isosurface: a 3-D lattice with at least 2 points per axis (got shape {u.shape})")
    if u.size >= 2 ** 31:
        raise ValueError(f"isosurface: X * Y * Z must be < 2^31 (got {u.size})")
    if np.isinf(u).any():
        raise ValueError("isosurface: the field holds +-inf")
    return u


def _edge_masks(inside):
    """bool [X,Y,Z] -> uint8 [X,Y,Z]: bit t set where the point owns a type-t edge whose ends differ"""
    X, Y, Z = inside.shape
    mask = np.zeros(inside.shape, dtype=np.uint8)
    for t, (dx, dy, dz) in enumerate(EDGE_OFFSETS):
        a = inside[:X - dx, :Y - dy, :Z - dz]
        b = inside[dx:, dy:, dz:]
        mask[:X - dx, :Y - dy, :Z - dz] |= (a != b).astype(np.uint8) << t
    return mask


def vertex_edges(u, threshold):
    """the lattice edge of every vertex, in the mesh's vertex order: (owner [V,3] int64 lattice coordinates, edge type [V] int64);
    the edge's other end is owner + EDGE_OFFSETS[type]"""
    u = _as_field(u.detach().cpu().numpy() if isinstance(u, torch.Tensor) else u)
    mask = _edge_masks(u > np.float32(threshold)).reshape(-1)
    owners = np.flatnonzero(mask)
    bits = (mask[owners, None] >> np.arange(7)) & 1
    k, t = np.nonzero(bits)            # row-major: owner in C order, then type
    return np.stack(np.unravel_index(owners[k], u.shape), -1).astype(np.int64), t.astype(np.int64)


def _isosurface_numpy(u, threshold):
    u = _as_field(u)
    thr = np.float32(threshold)
    X, Y, Z = u.shape
    inside = u > thr
    mask = _edge_masks(inside).reshape(-1)
    voff = np.cumsum(_POPCOUNT8[mask]) - _POPCOUNT8[mask]          # exclusive scan, int64
    V = int(_POPCOUNT8[mask].sum())
    if V >= 2 ** 31:
        raise ValueError(f"isosurface: {V} vertices do not fit int32 indices")
    uf = u.reshape(-1)
    strides = (Y * Z, Z, 1)
    vertices = np.empty((V, 3), dtype=np.float32)
    for t, off in enumerate(EDGE_OFFSETS):
        owner = np.flatnonzero((mask >> t) & 1)
        if owner.size == 0:
            continue
        ua = uf[owner]
        ub = uf[owner + off[0] * strides[0] + off[1] * strides[1] + off[2] * strides[2]]
        with np.errstate(all="ignore"):
            s = (thr - ua) / (ub - ua)                              # float32 throughout
            ids = voff[owner] + _POPCOUNT8[mask[owner] & ((1 << t) - 1)]
            pa = np.unravel_index(owner, u.shape)
            for d in range(3):
                vertices[ids, d] = pa[d].astype(np.float32) + s * np.float32(off[d])

    # faces: the corner configuration of every cell, then per tetrahedron and case
    cfg = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.uint8)
    for code in range(8):
        dx, dy, dz = _offset(code)
        cfg |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.uint8) << code
    cfg = cfg.reshape(-1)
    active = np.flatnonzero((cfg != 0) & (cfg != 255))              # cells in C order
    cfg = cfg[active].astype(np.int64)
    cx, cy, cz = np.unravel_index(active, (X - 1, Y - 1, Z - 1))
    corner = (cx * Y + cy) * Z + cz                                 # the cell's low corner as a lattice point
    ntri = np.asarray(_NTRI, dtype=np.int64)
    cases = [sum(((cfg >> code) & 1) << i for i, code in enumerate(tet)) for tet in _TETS]
    per_tet = np.stack([ntri[c] for c in cases], 0) if active.size else np.zeros((6, 0), dtype=np.int64)
    per_cell = per_tet.sum(0)
    F = int(per_cell.sum())
    if F >= 2 ** 31:
        raise ValueError(f"isosurface: {F} faces do not fit int32 indices")
    foff = np.cumsum(per_cell) - per_cell
    faces = np.empty((F, 3), dtype=np.int32)
    for k in range(6):
        for case in range(1, 15):
            sel = np.flatnonzero(cases[k] == case)
            if sel.size == 0:
                continue
            base = foff[sel] + per_tet[:k, sel].sum(0)
            for j, tri in enumerate(_TRIS[k][case]):
                for i, (code, t) in enumerate(tri):
                    o = _offset(code)
                    owner = corner[sel] + o[0] * strides[0] + o[1] * strides[1] + o[2] * strides[2]
                    faces[base + j, i] = voff[owner] + _POPCOUNT8[mask[owner] & ((1 << t) - 1)]
    return vertices, faces


def _isosurface_hip(u, threshold):
    u = u.detach()
    if u.dim() != 3 or min(u.shape) < 2:
        raise ValueError(f"isosurface: a 3-D lattice with at least 2 points per axis (got shape {tuple(u.shape)})")
    if u.numel() >= 2 ** 31:
        raise ValueError(f"isosurface: X * Y * Z must be < 2^31 (got {u.numel()})")
    u = u.to(torch.float32).contiguous()
    X, Y, Z = u.shape
    lib = _lib.lib()
    with torch.cuda.device(u.device):
        ws_bytes = lib.ngp_isosurface_workspace(X, Y, Z)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device)
        state = torch.empty(3, dtype=torch.int64, device=u.device)      # V, F, any(+-inf): one host read for all three
        state[2] = torch.isinf(u).any()
        _lib.check(lib.ngp_isosurface_count(_lib.ptr(u), X, Y, Z, float(threshold), _lib.ptr(ws), ws_bytes, _lib.ptr(state), _lib.stream()),
                   "isosurface_count")
        V, F, bad = (int(v) for v in state.tolist())
        if bad:
            raise ValueError("isosurface: the field holds +-inf")
        if V >= 2 ** 31 or F >= 2 ** 31:
            raise ValueError(f"isosurface: {V} vertices / {F} faces do not fit int32 indices")
        vertices = torch.empty(V, 3, dtype=torch.float32, device=u.device)
        faces = torch.empty(F, 3, dtype=torch.int32, device=u.device)
        if V or F:
            _lib.check(lib.ngp_isosurface_emit(_lib.ptr(u), X, Y, Z, float(threshold), _lib.ptr(ws), ws_bytes, V, F, _lib.ptr(vertices),
                                               _lib.ptr(faces), _lib.stream()), "isosurface_emit")
    return vertices, faces


def isosurface(u, threshold):
    """u [X,Y,Z] -> (vertices [V,3] float32 in index units, faces [F,3] int32); (0,3) arrays for an empty surface.  A CUDA tensor goes
    through the HIP kernels on the current stream (tensors back, on u's device, one host read of the sizes between count and emit); a
    CPU tensor or a numpy array through numpy (tensors back for a tensor, arrays for an array).  A non-contiguous or non-float32 input
    is copied first.  ValueError for +-inf in the field."""
    if isinstance(u, torch.Tensor):
        if u.is_cuda:
            return _isosurface_hip(u, threshold)
        v, f = _isosurface_numpy(u.detach().numpy(), threshold)
        return torch.from_numpy(v), torch.from_numpy(f)
    return _isosurface_numpy(np.asarray(u), threshold)


def extract_fields(bound_min, bound_max, resolution, query_func, S=128):
    """query_func on the resolution^3 lattice of torch.linspace(bound_min[d], bound_max[d], resolution) per axis, at most S^3 points
    [n, 3] per call (the reference's chunking, nerf/utils.py:152-167) -> float32 [R,R,R] tensor on the device query_func answers on"""
    axes = [torch.linspace(float(bound_min[d]), float(bound_max[d]), resolution).split(S) for d in range(3)]
    u = None
    with torch.no_grad():
        x0 = 0
        for xs in axes[0]:
            y0 = 0
            for ys in axes[1]:
                z0 = 0
                for zs in axes[2]:
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                    val = query_func(pts).detach().reshape(len(xs), len(ys), len(zs)).to(torch.float32)
                    if u is None:
                        u = torch.zeros(resolution, resolution, resolution, dtype=torch.float32, device=val.device)
                    u[x0:x0 + len(xs), y0:y0 + len(ys), z0:z0 + len(zs)] = val
                    z0 += len(zs)
                y0 += len(ys)
            x0 += len(xs)
    return u


def _bounds(b):
    """the bounds as numpy in their own dtype (float32 for model.aabb_infer): the reference subtracts them before it promotes"""
    return (b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64))[:3]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """-> (vertices [V,3] float64 numpy in the bounds' units, triangles [F,3] int32 numpy): the isosurface of extract_fields, scaled as
    nerf/utils.py:181 scales mcubes' vertices: v / (resolution - 1) * (b_max - b_min) + b_min"""
    u = extract_fields(bound_min, bound_max, resolution, query_func)
    v, f = isosurface(u, threshold)
    b_min, b_max = _bounds(bound_min), _bounds(bound_max)
    vertices = v.cpu().numpy().astype(np.float64) / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    return vertices, f.cpu().numpy()


def _ply_colors(colors, n):
    """vertex colours [V,3] as uint8: uint8 as it is, floats in [0, 1] as round(c * 255)"""
    c = np.asarray(colors)
    if c.shape != (n, 3):
        raise ValueError(f"write_ply: colors [V,3] (got {c.shape} for {n} vertices)")
    if c.dtype == np.uint8:
        return c
    return np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_ply(path, vertices, triangles, colors=None):
    """binary little-endian PLY: `float x y z` per vertex (and `uchar red green blue` with colors: uint8, or floats in [0, 1] stored as
    round(c * 255)), `list uchar int vertex_indices` per face.  Without colors the file is what it has always been."""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    rgb = "" if colors is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n{rgb}"
              f"element face {t.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    if colors is None:
        vertex_bytes = v.tobytes()
    else:
        vrec = np.empty(v.shape[0], dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
        vrec["p"], vrec["c"] = v, _ply_colors(colors, v.shape[0])
        vertex_bytes = vrec.tobytes()
    rec = np.empty(t.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"] = 3
    rec["i"] = t
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vertex_bytes)
        fh.write(rec.tobytes())


def read_ply(path):
    """what write_ply writes -> (vertices float32 [V,3], triangles int32 [F,3], colors uint8 [V,3] or None).  Binary little-endian,
    vertex properties `float x y z` and optionally `uchar red green blue`, triangles as `list uchar int vertex_indices`; anything
    else is a ValueError."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} is not a PLY file")
    lines = [ln.split() for ln in blob[:end].decode("ascii").split("\n")[1:] if ln.strip() and not ln.startswith("comment")]
    if not lines or lines[0] != ["format", "binary_little_endian", "1.0"]:
        raise ValueError("read_ply: only binary_little_endian 1.0")
    elements = []
    for ln in lines[1:]:
        if ln[0] == "element":
            elements.append((ln[1], int(ln[2]), []))
        elif ln[0] == "property" and elements:
            elements[-1][2].append(tuple(ln[1:]))
        else:
            raise ValueError(f"read_ply: unexpected header line {' '.join(ln)}")
    xyz = [("float", "x"), ("float", "y"), ("float", "z")]
    rgb = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    if [e[0] for e in elements] != ["vertex", "face"] or elements[0][2] not in (xyz, xyz + rgb) or \
            elements[1][2] != [("list", "uchar", "int", "vertex_indices")]:
        raise ValueError("read_ply: expected `float x y z [uchar red green blue]` vertices and `list uchar int vertex_indices` faces")
    n_v, n_f, colored = elements[0][1], elements[1][1], elements[0][2] == xyz + rgb
    vtype = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (3,))] if colored else []))
    ftype = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    body = blob[end + len(b"end_header\n"):]
    if len(body) != n_v * vtype.itemsize + n_f * ftype.itemsize:
        raise ValueError("read_ply: the body's size does not match the header (only triangles are read)")
    vrec = np.frombuffer(body, dtype=vtype, count=n_v)
    frec = np.frombuffer(body, dtype=ftype, count=n_f, offset=n_v * vtype.itemsize)
    if n_f and (frec["n"] != 3).any():
        raise ValueError("read_ply: a face is not a triangle")
    return vrec["p"].astype(np.float32), frec["i"].astype(np.int32), (vrec["c"].copy() if colored else None)


def save_mesh(model, save_path, resolution=256, threshold=10, fp16=False):
    """Trainer.save_mesh (nerf/utils.py:533-553): the isosurface sigma = threshold of model.density over model.aabb_infer on a
    resolution^3 lattice, written to save_path as a binary PLY -> (vertices float64 [V,3], triangles int32 [F,3])"""
    directory = os.path.dirname(save_path)
    if directory:
        os.makedirs(directory, exist_ok=True)
    device = model.aabb_infer.device

    def query_func(pts):
        with torch.no_grad(), torch.autocast(device.type, dtype=torch.float16 if device.type == "cuda" else torch.bfloat16, enabled=fp16):
            return model.density(pts.to(device))["sigma"]

    vertices, triangles = extract_geometry(model.aabb_infer[:3], model.aabb_infer[3:], resolution, threshold, query_func)
    write_ply(save_path, vertices, triangles)
    return vertices, triangles


def mesh_to_world(vertices, rot=PLANNER_ROT):
    """NeRF-frame points [..., 3] -> the world (planner) frame: the inverse of collision.to_nerf, x = w @ rot, for an orthonormal rot
    (w = x @ rot^T).  numpy in -> float64 numpy out; tensor in -> tensor out."""
    if isinstance(vertices, torch.Tensor):
        r = torch.as_tensor(rot, dtype=vertices.dtype).to(vertices.device).reshape(3, 3)
        return vertices[..., 0:1] * r[:, 0] + vertices[..., 1:2] * r[:, 1] + vertices[..., 2:3] * r[:, 2]
    r = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    return np.asarray(vertices, dtype=np.float64) @ r.T
