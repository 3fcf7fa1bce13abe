"""The NeRF's density as a triangle mesh: Trainer.save_mesh -> extract_geometry -> extract_fields of the reference
(nerf/utils.py:152-182, 533-551), with the field-to-surface step (mcubes there) as HIP kernels.

    extract_fields     the density on a resolution^3 lattice, S^3 points per query, kept on the device the values come from
    isosurface         lattice -> (vertices [V,3] float32 in index units, faces [F,3] int32)
                         CUDA tensor: ngp_isosurface_count / ngp_isosurface_emit (csrc/mesh.hip)
                         CPU tensor / numpy array: the same rule and order in numpy (the package's CPU path)
    simplify           a mesh made coarser by vertex clustering: one vertex per cubic cell, placed by the incident faces' plane quadrics
                         CUDA tensors: ngp_simplify_* (csrc/simplify.hip); CPU tensors / numpy arrays: the numpy path that defines it
    extract_geometry   extract_fields + isosurface (+ simplify with simplify_cell > 0) + the reference's scaling to the bounds
    save_mesh          extract_geometry of model.density over model.aabb_infer, written as a binary PLY
    write_ply/read_ply the binary PLY (optionally with uchar vertex colours) and its reader
    mesh_to_world      NeRF axes -> the world frame of collision.py's boxes (the inverse of collision.to_nerf)
    surface_error      how far the mesh is from the true world's (world.MeshWorld): accuracy, completeness, F-score, Hausdorff,
                         and the collision margin a planner needs (DESIGN.md "Surface error")
    sample_surface     area-weighted surface samples, deterministic for a seed
    distance_stats     count, sum, sum of squares, maximum and counts within thresholds of a distance array, in double, in one
                         fixed order (csrc/closest.hip ngp_distance_stats on a HIP device, the same order in numpy on the CPU)
    error_colors       per-vertex distances -> uint8 colours for write_ply

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
import ctypes
import dataclasses
import itertools
import math
import os
import struct

import numpy as np
import torch

from . import _lib
from .collision import PLANNER_ROT, component_table, label_components, to_nerf

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
    with torch.cuda.device(u.device):
        ws, ws_bytes = _lib.workspace("isosurface", X, Y, Z, device=u.device)
        state = torch.empty(3, dtype=torch.int64, device=u.device)      # V, F, any(+-inf): one host read for all three
        state[2] = torch.isinf(u).any()
        _lib.call("isosurface_count", u, X, Y, Z, float(threshold), ws, ws_bytes, state)
        V, F, bad = (int(v) for v in state.tolist())
        if bad:
            raise ValueError("isosurface: the field holds +-inf")
        if V >= 2 ** 31 or F >= 2 ** 31:
            raise ValueError(f"isosurface: {V} vertices / {F} faces do not fit int32 indices")
        vertices = torch.empty(V, 3, dtype=torch.float32, device=u.device)
        faces = torch.empty(F, 3, dtype=torch.int32, device=u.device)
        if V or F:
            _lib.call("isosurface_emit", u, X, Y, Z, float(threshold), ws, ws_bytes, V, F, vertices, faces)
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


# ------------------------------------------------------------------------------------------------------------- simplification
SIMPLIFY_LAMBDA = 1e-3                              # the regularisation towards the mean, as a share of trace(Q_A)
SIMPLIFY_MAX_INDEX = 1 << 21                        # cell indices per axis: three of them make one int64 key
_PLACEMENTS = {"quadric": 0, "mean": 1}


def _grouped_sum(values, start, count):
    """THE summation order of simplify (csrc/simplify.hip follows it): values float64 [N], sorted by cluster, cluster c owning the rows
    start[c] .. start[c] + count[c] -> float64 [C].  A cluster's rows are cut into groups of 64 consecutive ranks (the last padded
    with +0); a group is summed by the xor butterfly (_fold64); the cluster's sum is 0 + group 0 + group 1 + ... in that order."""
    C = count.shape[0]
    groups = -(-count // 64)
    gstart = np.cumsum(groups) - groups
    cluster = np.repeat(np.arange(C), count)
    padded = np.zeros(int(groups.sum()) * 64, dtype=np.float64)
    padded[gstart[cluster] * 64 + (np.arange(values.shape[0]) - start[cluster])] = values
    partial = _fold64(padded.reshape(-1, 64), np.add)
    acc = np.zeros(C, dtype=np.float64)
    for j in range(int(groups.max()) if C else 0):
        sel = np.flatnonzero(groups > j)
        acc[sel] = acc[sel] + partial[gstart[sel] + j]
    return acc


def _simplify_args(n_vertices, n_faces, cell, origin, placement):
    if placement not in _PLACEMENTS:
        raise ValueError(f"simplify: placement is 'quadric' or 'mean' (got {placement!r})")
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"simplify: cell > 0 and finite (got {cell})")
    if n_vertices >= 2 ** 31 or 3 * n_faces >= 2 ** 31:
        raise ValueError(f"simplify: V < 2^31 and 3 F < 2^31 (got {n_vertices} vertices, {n_faces} faces)")
    if origin is not None:
        origin = [float(o) for o in origin]
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"simplify: origin is three finite numbers (got {origin})")
    return cell, origin


_SIMPLIFY_ERRORS = {1: "a vertex is not finite, lies below `origin` or has a cell index >= 2^21", 2: "a face index is outside [0, V)"}


def _simplify_numpy(vertices, faces, cell, origin=None, placement="quadric"):
    """The definition of simplify (its docstring), in IEEE double on the float32 inputs with one rounding per written operation."""
    v32 = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = v32.shape[0], faces.shape[0]
    cell, origin = _simplify_args(V, F, cell, origin, placement)
    if origin is None:
        origin = [float(a) for a in v32.min(0)] if V else [0.0, 0.0, 0.0]
    o = np.asarray(origin, dtype=np.float64)
    v = v32.astype(np.float64)
    with np.errstate(all="ignore"):
        idx = np.floor((v - o[None, :]) / cell)
        if not ((idx >= 0.0) & (idx < float(SIMPLIFY_MAX_INDEX))).all():          # (false for NaN)
            raise ValueError("simplify: " + _SIMPLIFY_ERRORS[1])
    if ((faces < 0) | (faces >= V)).any():
        raise ValueError("simplify: " + _SIMPLIFY_ERRORS[2])
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.full(V, -1, np.int32))
    if V == 0 or F == 0:
        return empty

    # clusters: the distinct cells in ascending (ix, iy, iz); a cluster's vertices in ascending index
    ii = idx.astype(np.int64)
    keys = (ii[:, 0] << 42) | (ii[:, 1] << 21) | ii[:, 2]
    ukeys, cluster, vcount = np.unique(keys, return_inverse=True, return_counts=True)
    cluster = cluster.reshape(-1)
    C = ukeys.shape[0]
    vorder = np.argsort(cluster, kind="stable")
    vstart = np.cumsum(vcount) - vcount
    ci = np.stack([ukeys >> 42, (ukeys >> 21) & (SIMPLIFY_MAX_INDEX - 1), ukeys & (SIMPLIFY_MAX_INDEX - 1)], -1).astype(np.float64)
    pc = o[None, :] + (ci + 0.5) * cell

    # the mean of every cluster's vertices, relative to the cell's centre
    rel = v[vorder] - pc[cluster[vorder]]
    m = np.stack([_grouped_sum(rel[:, a], vstart, vcount) for a in range(3)], -1) / vcount.astype(np.float64)[:, None]

    # the plane quadrics of the corners of every cluster, corners in ascending 3 f + k
    ccluster = cluster[faces.reshape(-1)]
    corder = np.argsort(ccluster, kind="stable")
    ccount = np.bincount(ccluster, minlength=C)
    cstart = np.cumsum(ccount) - ccount
    fa = faces[corder // 3]
    pa, pb, pcn = v[fa[:, 0]], v[fa[:, 1]], v[fa[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = pb - pa, pcn - pa
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        r = pa - pc[ccluster[corder]]
        d = -((nx * r[:, 0] + ny * r[:, 1]) + nz * r[:, 2])
        del fa, pa, pb, pcn, e1, e2, r
        qxx, qxy, qxz, qyy, qyz, qzz, bx, by, bz = (_grouped_sum(t, cstart, ccount) for t in
                                                    (nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, d * nx, d * ny, d * nz))
        # (Q_A + mu I) x = mu m - q_b by Cramer's rule, every cofactor written out
        t = (qxx + qyy) + qzz
        mu = SIMPLIFY_LAMBDA * t
        a, b, c, dd, e, f = qxx + mu, qxy, qxz, qyy + mu, qyz, qzz + mu
        r0, r1, r2 = mu * m[:, 0] - bx, mu * m[:, 1] - by, mu * m[:, 2] - bz
        c00, c01, c02 = dd * f - e * e, c * e - b * f, b * e - c * dd
        c11, c12, c22 = a * f - c * c, b * c - a * e, a * dd - b * b
        det = (a * c00 + b * c01) + c * c02
        x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], -1)
        half = cell / 2.0
        ok = (np.abs(x) <= half).all(1) & (t != 0.0)                # (false for a NaN or an infinity in x)
        if _PLACEMENTS[placement] == 1:
            ok[:] = False
        x = np.where(ok[:, None], x, m)
        x = np.minimum(np.maximum(x, -half), half)
        rep = (pc + x).astype(np.float32)
    single = vcount == 1
    rep[single] = v32[vorder[vstart[single]]]

    # faces: survivors in input order and rotation; clusters no survivor references are dropped
    fc = cluster[faces]
    keep = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    if not keep.any():
        return empty
    referenced = np.zeros(C, dtype=bool)
    referenced[fc[keep].reshape(-1)] = True
    new_id = (np.cumsum(referenced) - 1).astype(np.int32)
    return rep[referenced], new_id[fc[keep]], np.where(referenced[cluster], new_id[cluster], np.int32(-1)).astype(np.int32)


def _simplify_hip(vertices, faces, cell, origin, placement):
    device = vertices.device
    v = vertices.detach().to(torch.float32).reshape(-1, 3).contiguous()
    f = faces.detach().to(device, torch.int32).reshape(-1, 3).contiguous()
    V, F = v.shape[0], f.shape[0]
    cell, origin = _simplify_args(V, F, cell, origin, placement)
    with torch.cuda.device(device):
        empty = lambda: (torch.zeros(0, 3, dtype=torch.float32, device=device), torch.zeros(0, 3, dtype=torch.int32, device=device),
                         torch.full((V,), -1, dtype=torch.int32, device=device))
        if V == 0 and F == 0:
            return empty()
        if origin is None:
            origin = v.min(0).values.tolist() if V else [0.0, 0.0, 0.0]      # (a host read of its own; pass origin to avoid it)
        o = (ctypes.c_double * 3)(*origin)
        state = torch.zeros(3, dtype=torch.int64, device=device)              # V', F', the error word: one host read for all three
        err = state[2:].view(torch.int32)
        keys = torch.empty(V, dtype=torch.int64, device=device)
        _lib.call("simplify_keys", v, V, f, F, o, cell, keys, err)
        if V == 0 or F == 0:
            code = int(state[2].item()) & 0xFFFFFFFF
            if code:
                raise ValueError("simplify: " + _SIMPLIFY_ERRORS[code])
            return empty()
        # plumbing: every list sorted by cluster (stable: ascending index within one), the clusters' first rows
        skeys, vorder = torch.sort(keys, stable=True)
        rank = torch.zeros(V, dtype=torch.int64, device=device)
        rank[1:] = torch.cumsum(skeys[1:] != skeys[:-1], 0)
        vcluster = torch.empty(V, dtype=torch.int32, device=device)
        vcluster[vorder] = rank.to(torch.int32)
        ids = torch.arange(V + 1, dtype=torch.int64, device=device)
        vstart = torch.searchsorted(rank, ids)                                # (V for the ids past the last cluster)
        ccluster = torch.empty(3 * F, dtype=torch.int32, device=device)
        _lib.call("simplify_corners", f, F, V, vcluster, ccluster)
        csorted, corder = torch.sort(ccluster, stable=True)
        cstart = torch.searchsorted(csorted.to(torch.int64), ids)
        rep = torch.empty(V, 3, dtype=torch.float32, device=device)           # (one row per cluster; there are at most V)
        _lib.call("simplify_accumulate", v, V, f, F, o, cell, _PLACEMENTS[placement], skeys, vorder, vstart, corder, cstart, rep)
        keep = torch.empty(F, dtype=torch.int32, device=device)
        referenced = torch.empty(V, dtype=torch.int32, device=device)
        _lib.call("simplify_faces", ccluster, F, V, keep, referenced)
        keep_scan, ref_scan = torch.cumsum(keep, 0), torch.cumsum(referenced, 0)         # inclusive, int64
        state[0], state[1] = ref_scan[-1], keep_scan[-1]
        n_v, n_f, code = (int(s) for s in state.tolist())
        if code & 0xFFFFFFFF:
            raise ValueError("simplify: " + _SIMPLIFY_ERRORS[code & 0xFFFFFFFF])
        out_v = torch.empty(n_v, 3, dtype=torch.float32, device=device)
        out_f = torch.empty(n_f, 3, dtype=torch.int32, device=device)
        vertex_map = torch.empty(V, dtype=torch.int32, device=device)
        _lib.call("simplify_emit", V, F, vcluster, ccluster, rep, keep, keep_scan, referenced, ref_scan, n_v, n_f, out_v, out_f, vertex_map)
    return out_v, out_f, vertex_map


def simplify(vertices, faces, cell, *, origin=None, placement="quadric"):
    """Vertex clustering with quadric-optimal representatives (Rossignac-Borrel cells, Lindstrom's placement; DESIGN.md "Mesh
    simplification"): vertices float32 [V,3], faces int32 [F,3] -> (vertices float32 [V',3], faces int32 [F',3], vertex_map int32 [V]:
    the output vertex of every input vertex, or -1).  CUDA tensors go through csrc/simplify.hip on the current stream (tensors back; one
    host read, of V', F' and the error word, plus one of the minimum when origin is None); CPU tensors and numpy arrays through
    _simplify_numpy, which defines the result -- the HIP path gives the same bits.  All arithmetic is IEEE double on the float32 inputs.

    1. vertex -> cell i_a = floor((v_a - o_a) / cell), o = origin (default: the per-axis float32 minimum); a coordinate on a cell face
       belongs to the upper cell.  ValueError for cell <= 0, a non-finite coordinate, a vertex below origin, an index >= 2^21, a face
       index outside [0, V), an unknown placement.
    2. clusters = the distinct cells in ascending (ix, iy, iz); p_c = o + (i + 1/2) cell.
    3. per cluster, relative to p_c: m = the mean of its vertices (ascending index); over every corner 3 f + k (ascending) whose vertex
       lies in it, with A, B, C the face's vertices: n = (B - A) x (C - A), d = -n . (A - p_c), Q_A += n n^T, q_b += d n.  Every sum
       in _grouped_sum's order.
    4. t = trace Q_A, mu = SIMPLIFY_LAMBDA t, x solves (Q_A + mu I) x = mu m - q_b (Cramer's rule); x = m instead for
       placement="mean", t == 0, or an x that is not finite or leaves the cell (some |x_a| > cell / 2); x clamped to +- cell / 2; the
       vertex is float32(p_c + x).  A cluster of ONE vertex keeps that vertex bit for bit.
    5. a face survives iff its three clusters differ; survivors keep order and rotation; duplicates stay (a closed surface stays closed).
    6. clusters without a surviving face are dropped, the rest renumbered in order."""
    if isinstance(vertices, torch.Tensor):
        if vertices.is_cuda:
            return _simplify_hip(vertices, torch.as_tensor(faces), cell, origin, placement)
        out = _simplify_numpy(vertices.detach().numpy(), torch.as_tensor(faces).detach().cpu().numpy(), cell, origin, placement)
        return tuple(torch.from_numpy(a) for a in out)
    return _simplify_numpy(np.asarray(vertices), faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces),
                           cell, origin, placement)


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


def drop_small_components(u, threshold, min_points):
    """u [X,Y,Z] with the floaters taken out before the surface is cut: the inside points (u > threshold, strict, NaN outside, as
    isosurface has it) that belong to a 14-connected component (collision.label_components; +- EDGE_OFFSETS, the Kuhn split's own
    edges) of fewer than min_points points are set to `threshold`, which is outside; nothing else changes.  No kept inside point
    shares a lattice edge with a changed one, so the kept surface keeps every vertex bit for bit, and its order.  Runs where u lives
    (HIP for a CUDA tensor: one host read, of the number of components); the same kind comes back, u itself for min_points <= 1."""
    if int(min_points) != min_points or min_points < 0:
        raise ValueError(f"drop_small_components: min_points is an integer >= 0 (got {min_points!r})")
    if min_points <= 1:
        return u
    is_tensor = isinstance(u, torch.Tensor)
    thr = np.float32(threshold)
    inside = (u.to(torch.float32) > float(thr)) if is_tensor else (np.asarray(u, dtype=np.float32) > thr)       # isosurface's own test
    labels, n = label_components(inside, 14)
    cells = component_table(labels, n).cells
    if is_tensor:
        small = torch.cat([torch.zeros(1, dtype=torch.bool, device=u.device), cells < int(min_points)])[labels.long()]
        return torch.where(small, torch.full_like(u, float(thr)), u)
    small = np.concatenate([[False], cells < int(min_points)])[labels]
    return np.where(small, np.asarray(thr, dtype=u.dtype), u)


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, min_points=0, simplify_cell=0):
    """-> (vertices [V,3] float64 numpy in the bounds' units, triangles [F,3] int32 numpy): the isosurface of extract_fields, scaled as
    nerf/utils.py:181 scales mcubes' vertices: v / (resolution - 1) * (b_max - b_min) + b_min.  min_points: drop_small_components
    first (0: the field as it is).  simplify_cell > 0: simplify(..., cell=simplify_cell, origin=(0, 0, 0)) on the surface in index
    units, before the scaling -- the cell is in lattice steps and the result does not depend on where the bounds lie (0: the surface
    as it is cut)."""
    if not simplify_cell >= 0:
        raise ValueError(f"extract_geometry: simplify_cell >= 0 (got {simplify_cell!r})")
    u = drop_small_components(extract_fields(bound_min, bound_max, resolution, query_func), threshold, min_points)
    v, f = isosurface(u, threshold)
    if simplify_cell > 0:
        v, f, _ = simplify(v, f, simplify_cell, origin=(0.0, 0.0, 0.0))
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


def save_mesh(model, save_path, resolution=256, threshold=10, fp16=False, min_points=0, simplify_cell=0):
    """Trainer.save_mesh (nerf/utils.py:533-553): the isosurface sigma = threshold of model.density over model.aabb_infer on a
    resolution^3 lattice, written to save_path as a binary PLY -> (vertices float64 [V,3], triangles int32 [F,3]).  min_points:
    components of fewer inside lattice points are left out (drop_small_components; 0: none).  simplify_cell: the side, in lattice
    steps, of the cells `simplify` clusters the surface's vertices in (0: no simplification, the file it has always been)."""
    directory = os.path.dirname(save_path)
    if directory:
        os.makedirs(directory, exist_ok=True)
    device = model.aabb_infer.device

    def query_func(pts):
        with torch.no_grad(), torch.autocast(device.type, dtype=torch.float16 if device.type == "cuda" else torch.bfloat16, enabled=fp16):
            return model.density(pts.to(device))["sigma"]

    vertices, triangles = extract_geometry(model.aabb_infer[:3], model.aabb_infer[3:], resolution, threshold, query_func, min_points,
                                           simplify_cell)
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


# ------------------------------------------------------------------------------------------------------------- surface error
MAX_THRESHOLDS = 8                                  # NGP_DISTANCE_STATS_MAX_THRESHOLDS
MISS_COLOR = (255, 0, 255)                          # error_colors: a point without surface within max_distance
ERROR_RAMP = ((0, 160, 0), (255, 255, 0), (255, 0, 0))      # error_colors: distance 0, vmax / 2, vmax and beyond


def _check_thresholds(thresholds):
    th = [float(t) for t in thresholds]
    if len(th) > MAX_THRESHOLDS or any(t != t for t in th):
        raise ValueError(f"distance_stats: at most {MAX_THRESHOLDS} thresholds, none NaN (got {th})")
    return th


def _fold64(a, op):
    """the xor butterfly of 64 lanes as lane 0 sees it: offsets 32, 16, .. 1 over the last axis"""
    for off in (32, 16, 8, 4, 2, 1):
        a = op(a[..., :off], a[..., off:2 * off])
    return a[..., 0]


def distance_stats_numpy(distance, thresholds=()):
    """ngp_distance_stats in numpy, the same order and so the same bits: element i sits in lane i % 64 of group i / 64; a group's 64
    contributions (a non-finite or absent element contributes nothing) by the butterfly, in double; lane l adds the groups l,
    l + 64, ... in that order; the butterfly over the lanes.  -> the dict distance_stats documents"""
    th = _check_thresholds(thresholds)
    d = np.ascontiguousarray(distance, np.float32).reshape(-1)
    n = d.shape[0]
    rows = 64 * max(1, -(-n // 4096))                                   # groups, padded to whole rounds of the 64 lanes
    x = np.full(rows * 64, np.inf, np.float32)
    x[:n] = d
    x = x.reshape(rows, 64)
    finite = x < np.float32(np.inf)                                       # (false for NaN)
    v = np.where(finite, x, np.float32(0)).astype(np.float64)
    terms = [finite.astype(np.float64), v, v * v, v] + [(finite & (x <= np.float32(t))).astype(np.float64) for t in th]
    out = []
    for q, t in enumerate(terms):
        op = np.maximum if q == 3 else np.add
        groups = _fold64(t, op).reshape(-1, 64)
        acc = np.zeros(64, np.float64)
        for row in groups:
            acc = op(acc, row)
        out.append(float(_fold64(acc, op)))
    return {"n": n, "finite": int(out[0]), "sum": out[1], "sum_sq": out[2], "max": out[3], "within": tuple(int(c) for c in out[4:])}


def distance_stats(distance, thresholds=(), splits=()):
    """distance: float32 [N], a tensor (a HIP device: ngp_distance_stats on the current stream; the CPU: distance_stats_numpy) or
    a numpy array -> {"n": N, "finite": the number of finite entries, "sum", "sum_sq", "max": of those, in double (max 0 without
    any), "within": the number of finite entries <= each threshold}.  splits: indices at which the array is handed to the kernel in
    separate launches; the result does not depend on them."""
    th = _check_thresholds(thresholds)
    if not isinstance(distance, torch.Tensor) or distance.device.type != "cuda":
        return distance_stats_numpy(distance.detach().numpy() if isinstance(distance, torch.Tensor) else distance, th)
    d = distance.detach().to(torch.float32).reshape(-1).contiguous()
    n, lib = d.shape[0], _lib.lib()
    cuts = [0] + sorted(int(c) for c in splits) + [n]
    if cuts[1] < 0 or cuts[-2] > n:
        raise ValueError(f"distance_stats: splits lie in 0 .. {n}")
    th_c = (ctypes.c_float * max(1, len(th)))(*th)
    with torch.cuda.device(d.device):
        state = torch.empty(lib.ngp_distance_stats_state_bytes(), dtype=torch.uint8, device=d.device)
        stats = torch.empty(16, dtype=torch.float64, device=d.device)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b - a >= 2 ** 31:
                raise ValueError("distance_stats: fewer than 2^31 distances per launch; pass splits")
            ws, nbytes = _lib.workspace("distance_stats", b - a, device=d.device)
            _lib.call("distance_stats", d[a:b] if b > a else None, b - a, a, th_c, len(th), state, stats, ws, nbytes)
    out = stats.cpu().tolist()
    return {"n": n, "finite": int(out[0]), "sum": out[1], "sum_sq": out[2], "max": out[3], "within": tuple(int(c) for c in out[4:4 + len(th)])}


def sample_surface(vertices, faces, n, seed=0):
    """n points of the surface, area-weighted: float32 [n,3] on the vertices' device (numpy in, numpy out).  Deterministic for a
    seed, and the same on every device: the draw and its arithmetic run on the host in float64 -- three uniform draws per point
    (u, r1, r2 [n] each, in this order) from torch.Generator().manual_seed(seed); the face is the first whose cumulative area (in
    face order) exceeds u * the total, the point (1 - sqrt(r1)) v0 + sqrt(r1) (1 - r2) v1 + sqrt(r1) r2 v2, rounded to float32."""
    as_numpy = not isinstance(vertices, torch.Tensor)
    v = torch.as_tensor(np.asarray(vertices) if as_numpy else vertices.detach())
    f = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces.detach())
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0 or int(n) < 0:
        raise ValueError(f"sample_surface: vertices [V,3], faces [F,3], n >= 0 (got {tuple(v.shape)}, {tuple(f.shape)}, {n})")
    tri = v.to("cpu", torch.float32)[f.to("cpu").long()].to(torch.float64)
    area = torch.linalg.vector_norm(torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), dim=1)
    cdf = torch.cumsum(area, 0)
    if not float(cdf[-1]) > 0:
        raise ValueError("sample_surface: the mesh has no area")
    gen = torch.Generator().manual_seed(int(seed))
    u, r1, r2 = [torch.rand(int(n), generator=gen, dtype=torch.float64) for _ in range(3)]
    face = torch.searchsorted(cdf, u * cdf[-1], right=True).clamp_max(f.shape[0] - 1)
    su = r1.sqrt()
    t = tri[face]
    p = ((1.0 - su)[:, None] * t[:, 0] + (su * (1.0 - r2))[:, None] * t[:, 1] + (su * r2)[:, None] * t[:, 2]).to(torch.float32)
    return p.numpy() if as_numpy else p.to(v.device)


@dataclasses.dataclass
class DirectionError:
    """one direction of surface_error: n points, `misses` of them without surface within max_distance (or not finite); mean, rms and
    max of the others' distances; within[tau] the number of points with distance <= tau; `distances` float32 [n] on the world's
    device (+inf: a miss); `stats` the raw sums they come from (distance_stats' dict)"""
    n: int
    misses: int
    mean: float
    rms: float
    max: float
    within: dict
    distances: torch.Tensor
    stats: dict


def _direction(distances, thresholds):
    st = distance_stats(distances, thresholds)
    k = st["finite"]
    return DirectionError(st["n"], st["n"] - k, st["sum"] / k if k else math.nan, math.sqrt(st["sum_sq"] / k) if k else math.nan, st["max"],
                          dict(zip(thresholds, st["within"])), distances, st)


@dataclasses.dataclass
class SurfaceError:
    """accuracy: the given mesh's points against the world; completeness: the world's points against the given mesh.
    precision[tau] = accuracy.within[tau] / accuracy.n, recall[tau] the same of completeness (a miss is not within),
    f_score[tau] = 2 p r / (p + r) (0 when both are); hausdorff: the larger of the two maxima, max_distance when a point missed."""
    accuracy: DirectionError
    completeness: DirectionError
    thresholds: tuple
    max_distance: float
    precision: dict
    recall: dict
    f_score: dict
    hausdorff: float

    def margin(self, q):
        """the q-quantile (nearest rank: the smallest distance with a share >= q of the points at or below it, numpy's
        `inverted_cdf`) of the completeness distances: the collision radius within which a share q of the true surface has surface
        of the given mesh.  +inf when the quantile falls among the misses."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"SurfaceError.margin: q in [0, 1] (got {q})")
        d = np.sort(self.completeness.distances.detach().cpu().numpy().reshape(-1))
        if d.size == 0:
            return math.nan
        return float(d[min(d.size - 1, max(0, int(math.ceil(d.size * q - 1.0))))])


def surface_error(vertices, faces, world, *, thresholds, max_distance, samples=None, seed=0, frame="nerf"):
    """the distance between the surface of a mesh (vertices [V,3], faces [F,3]; the NeRF's axes, or frame="world": the planner's
    frame, turned by collision.to_nerf like MeshWorld's) and the surface of `world` (a world.MeshWorld), both ways -> SurfaceError.
    The points of a direction are the mesh's vertices, or with samples=n that many area-weighted surface samples (sample_surface
    with `seed` for the given mesh, seed + 1 for the world).  max_distance truncates the search (world.MeshWorld.closest): a point
    without surface within it is a miss.  Everything runs on the world's device: closest-point queries and statistics in HIP on a
    HIP device, their numpy forms on the CPU."""
    from .world import MeshWorld
    if frame not in ("nerf", "world"):
        raise ValueError(f"surface_error: frame is 'nerf' or 'world' (got {frame!r})")
    th = tuple(_check_thresholds(thresholds))
    max_distance = float(max_distance)
    if max_distance != max_distance:
        raise ValueError("surface_error: max_distance is NaN")
    v = torch.as_tensor(np.asarray(vertices) if not isinstance(vertices, torch.Tensor) else vertices.detach()).to(world.device, torch.float32)
    f = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces.detach()).to(world.device)
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"surface_error: vertices [V,3] (got {tuple(v.shape)})")
    if frame == "world":
        v = to_nerf(v, PLANNER_ROT)
    given = MeshWorld(v, f)
    if samples is None:
        from_given, from_world = given.vertices, world.vertices
    else:
        from_given = sample_surface(given.vertices, given.faces, samples, seed)
        from_world = sample_surface(world.vertices, world.faces, samples, seed + 1)
    accuracy = _direction(world.closest(from_given, max_distance)["distance"], th)
    completeness = _direction(given.closest(from_world, max_distance)["distance"], th)
    precision = {t: accuracy.within[t] / accuracy.n if accuracy.n else math.nan for t in th}
    recall = {t: completeness.within[t] / completeness.n if completeness.n else math.nan for t in th}
    f_score = {t: 2.0 * precision[t] * recall[t] / (precision[t] + recall[t]) if precision[t] + recall[t] > 0 else 0.0 for t in th}
    hausdorff = max_distance if accuracy.misses or completeness.misses else max(accuracy.max, completeness.max)
    return SurfaceError(accuracy, completeness, th, max_distance, precision, recall, f_score, hausdorff)


def error_colors(distance, vmax):
    """distances [N] (tensor or numpy) -> uint8 [N,3] for write_ply: ERROR_RAMP, linear between its three colours at 0, vmax / 2 and
    vmax (beyond: the last), rounded to nearest; a non-finite distance (a miss) is MISS_COLOR"""
    if not float(vmax) > 0:
        raise ValueError("error_colors: vmax > 0")
    d = np.asarray(distance.detach().cpu().numpy() if isinstance(distance, torch.Tensor) else distance, np.float64).reshape(-1)
    ok = np.isfinite(d)
    t = np.clip(np.where(ok, d, 0.0) / float(vmax), 0.0, 1.0) * 2.0
    ramp = np.asarray(ERROR_RAMP, np.float64)
    k = np.minimum(t.astype(np.int64), 1)
    w = (t - k)[:, None]
    rgb = np.rint(ramp[k] * (1.0 - w) + ramp[k + 1] * w).astype(np.uint8)
    rgb[~ok] = MISS_COLOR
    return rgb
