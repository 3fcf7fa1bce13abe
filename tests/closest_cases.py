"""Shared meshes, query points and references of the closest-point tests (test_closest_cpu.py, test_closest_gpu.py).  The meshes are
raycast_cases' (cube, henge, soup).  Everything is built once per process and must not be modified by a test.

Points per mesh (float32 [N,3], about 2 000; `sections` names slices of them):
    vertex     up to 200 of the vertices the faces use (evenly spread over their list)
    midpoint   the three edge midpoints of up to 100 faces (evenly spread over the face list)
    centroid   the centroids of the same faces
    centre     the centre of the bounding box (on the cube: the same distance to all 12 faces)
    duplicate  (soup) centroid and two inner points of every face that a later face repeats: the tie goes to the lower index
    zero_area  (soup) the centroid of every zero-area face
    near       600 points within 0.05 extents of the surface: a random point of a random face plus a random offset
    outside    500 points of the bounding box enlarged by 0.7 extents on every side
    far        one point beyond the grid's reach (every triangle is tested)
    broken     points with a NaN, a +inf or a -inf component: misses
HAND are the sections whose closest triangle is not in doubt between float32 and float64.
"""
import functools
import math

import numpy as np
import torch

import raycast_cases as RC
from nerfsafetyvalidation_amd import world as WO

f32 = np.float32
MESHES = RC.MESHES
RESOLUTIONS = RC.RESOLUTIONS
N_TAILS = RC.N_TAILS
HAND = ("vertex", "centroid", "duplicate")
mesh = RC.mesh
bits = RC.bits


def scale(name):
    """the mesh's scale S of grid_params, and its largest extent"""
    v = mesh(name)[0]
    ext = float((v.max(0) - v.min(0)).max())
    return max(ext, float(np.abs(v).max())), ext


@functools.lru_cache(maxsize=None)
def points(name):
    """-> (points float32 [N,3], sections: name -> slice)"""
    v, faces, _ = mesh(name)
    rng = np.random.default_rng({"cube": 11, "henge": 12, "soup": 13}[name])
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    parts = []
    used = np.unique(faces)                                           # (soup holds vertices that no face uses: not surface)
    parts.append(("vertex", v[used[np.unique(np.linspace(0, len(used) - 1, min(len(used), 200)).astype(np.int64))]]))
    some = faces[np.unique(np.linspace(0, len(faces) - 1, min(len(faces), 100)).astype(np.int64))]
    tri = v[some].astype(np.float64)
    parts.append(("midpoint", np.concatenate([(tri[:, 0] + tri[:, 1]) / 2, (tri[:, 0] + tri[:, 2]) / 2, (tri[:, 1] + tri[:, 2]) / 2])))
    parts.append(("centroid", tri.mean(1)))
    parts.append(("centre", ((lo + hi) / 2)[None]))
    if name == "soup":
        t = v[faces[list(RC.DUPLICATES)]].astype(np.float64)
        parts.append(("duplicate", np.concatenate([t.mean(1), 0.6 * t[:, 0] + 0.3 * t[:, 1] + 0.1 * t[:, 2], 0.2 * t[:, 0] + 0.2 * t[:, 1] + 0.6 * t[:, 2]])))
        parts.append(("zero_area", v[faces[list(RC.ZERO_AREA)]].astype(np.float64).mean(1)))
    pick = rng.integers(0, len(faces), 600)
    w = rng.dirichlet((1.0, 1.0, 1.0), 600)
    on = (v[faces[pick]].astype(np.float64) * w[:, :, None]).sum(1)
    off = rng.normal(size=(600, 3))
    off *= (rng.uniform(0, 0.05 * ext, 600) / np.linalg.norm(off, axis=1))[:, None]
    off[:100] = 0.0                                                   # the first hundred lie on the surface
    parts.append(("near", on + off))
    parts.append(("outside", rng.uniform(lo - 0.7 * ext, hi + 0.7 * ext, (500, 3))))
    reach = float(WO.grid_params(v.min(0), v.max(0), len(faces))["reach"])
    parts.append(("far", np.array([[1.5 * reach, (lo[1] + hi[1]) / 2, lo[2]]])))
    mid = (lo + hi) / 2
    broken = np.tile(mid, (6, 1))
    broken[0, 0], broken[1, 1], broken[2, 2] = np.nan, np.inf, -np.inf
    broken[3] = np.nan
    broken[4, 0], broken[4, 2] = np.inf, np.nan
    broken[5, 1] = -np.inf
    parts.append(("broken", broken))
    sections, at = {}, 0
    for tag, a in parts:
        sections[tag] = slice(at, at + len(a))
        at += len(a)
    p = np.concatenate([np.asarray(a, np.float64) for _, a in parts]).astype(f32)
    p.setflags(write=False)
    return p, sections


@functools.lru_cache(maxsize=None)
def reference(name):
    """closest_numpy (the rule, float32, max_distance = +inf) on points(name): computed once, shared, read-only"""
    v, faces, _ = mesh(name)
    out = WO.closest_numpy(points(name)[0], v, faces)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference64(name):
    """the same formulas in float64 on the same float32 inputs"""
    v, faces, _ = mesh(name)
    out = WO.closest_numpy(points(name)[0], v, faces, dtype=np.float64)
    for a in out.values():
        a.setflags(write=False)
    return out


def truncated(ref, max_distance):
    """the rule's result for a finite max_distance from its result for +inf: acceptance is the last step of the rule"""
    keep = ref["distance"] <= f32(max_distance)
    return {"distance": np.where(keep, ref["distance"], f32(np.inf)), "prim": np.where(keep, ref["prim"], -1).astype(np.int32),
            "point": np.where(keep[:, None], ref["point"], f32(np.nan))}


def same(got, want):
    """prim equal; distance and point bit for bit, NaN positions equal (NaN payloads are not compared)"""
    g = {k: np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a) for k, a in got.items()}
    assert g["prim"].dtype == np.int32 and g["distance"].dtype == f32 and g["point"].dtype == f32
    assert np.array_equal(g["prim"].reshape(-1), want["prim"].reshape(-1))
    assert np.array_equal(bits(g["distance"]).reshape(-1), bits(want["distance"]).reshape(-1))
    gp, wp = g["point"].reshape(-1, 3), want["point"].reshape(-1, 3)
    assert np.array_equal(np.isnan(gp), np.isnan(wp))
    assert np.array_equal(bits(np.nan_to_num(gp)), bits(np.nan_to_num(wp)))


# ---- the two cubes of the surface-error tests: half-widths 1 and 1 + DELTA, every face a K x K lattice of quads
DELTA = 0.0625
CUBE_K = 8


@functools.lru_cache(maxsize=None)
def lattice_cube(half, k=CUBE_K):
    """an axis-aligned cube of half-width `half` centred on the origin, each face k x k quads of two triangles: (vertices float32
    [V,3], faces int32 [F,3]); the eight corners are among the vertices"""
    t = np.linspace(-half, half, k + 1)
    verts, faces = [], []
    for axis in range(3):
        for side in (-half, half):
            base = len(verts)
            for a in t:
                for b in t:
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, a, b
                    verts.append(p)
            for i in range(k):
                for j in range(k):
                    q = base + i * (k + 1) + j
                    faces += [[q, q + k + 1, q + k + 2], [q, q + k + 2, q + 1]]
    v, f = np.asarray(verts, f32), np.asarray(faces, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


# ---- tolerances, the surface-error cases and the statistics' references
# measured max |d32 - d64| / S over the point sets of closest_cases: cube 1.04e-7, henge 1.59e-6, soup 3.90e-6 -- the one point
# beyond the grid's reach, 96 S away, sets the last two; without it 1.04e-7, 1.15e-7, 8.3e-8.  Relative to max(S, d): 1.06e-7.
MEASURED_OVER_S = 3.90e-6
MEASURED_RELATIVE = 1.06e-7
TOL_OVER_S = 4 * MEASURED_OVER_S
TOL_RELATIVE = 4 * MEASURED_RELATIVE


def stats_bound(n):
    """relative bound of a sum of ngp_distance_stats' order against the exact sum of the same non-negative terms: every term passes
    6 + ceil(groups / 64) + 6 double additions (the group's butterfly, its lane's groups in turn, the lanes' butterfly), each with a
    relative error of at most 2^-53, and nothing cancels: (12 + ceil(ceil(n / 64) / 64)) 2^-53, first order"""
    return (12 + math.ceil(math.ceil(n / 64) / 64)) * 2.0 ** -53 * 1.01


def exact_stats(d, thresholds):
    """float64 evaluation with exactly rounded sums (math.fsum)"""
    d = np.asarray(d, f32).reshape(-1)
    fin = d[np.isfinite(d)].astype(np.float64)
    return {"n": d.size, "finite": fin.size, "sum": math.fsum(fin), "sum_sq": math.fsum(fin * fin), "max": float(fin.max()) if fin.size else 0.0,
            "within": tuple(int((fin <= np.float64(f32(t))).sum()) for t in thresholds)}


def check_stats(got, want):
    assert got["n"] == want["n"] and got["finite"] == want["finite"] and got["within"] == want["within"] and got["max"] == want["max"]
    bound = stats_bound(want["n"])
    for key in ("sum", "sum_sq"):
        print(key, got[key], want[key], "bound", bound * want[key])
        assert abs(got[key] - want[key]) <= bound * want[key]


THRESHOLDS = (1.01 * DELTA, 1.5 * DELTA, 0.25)


def two_cubes(device=None):
    (v1, f1), (v2, f2) = lattice_cube(1.0), lattice_cube(1.0 + DELTA)
    if device is None:
        return v1, f1, WO.MeshWorld(v2, f2)
    return torch.from_numpy(v1.copy()).to(device), torch.from_numpy(f1.copy()).to(device), \
        WO.MeshWorld(torch.from_numpy(v2.copy()).to(device), torch.from_numpy(f2.copy()).to(device))


def check_two_cubes(err):
    """cube of half-width 1 against cube of half-width 1 + delta: every distance in [delta, delta sqrt 3], the Hausdorff distance
    delta sqrt 3 at the outer cube's corners; tolerance: test_closest_numpy_against_float64's, S = 1 + delta"""
    tol = TOL_RELATIVE * (1.0 + DELTA)
    for side in (err.accuracy, err.completeness):
        d = side.distances.detach().cpu().numpy()
        assert side.misses == 0 and side.n == d.size == 6 * (CUBE_K + 1) ** 2
        assert (d >= DELTA - tol).all() and (d <= DELTA * math.sqrt(3) + tol).all()
        check_stats(side.stats, exact_stats(d, THRESHOLDS))
        assert side.mean == side.stats["sum"] / side.n and side.rms == math.sqrt(side.stats["sum_sq"] / side.n) and side.max == side.stats["max"]
        assert tuple(side.within[t] for t in THRESHOLDS) == side.stats["within"]
    assert abs(err.accuracy.max - DELTA) <= tol                        # the inner cube's vertices all see a face straight ahead
    assert abs(err.hausdorff - DELTA * math.sqrt(3)) <= tol and err.hausdorff == err.completeness.max
    dc = err.completeness.distances.detach().cpu().numpy()
    corner = np.abs(np.asarray(lattice_cube(1.0 + DELTA)[0])).min(1) == f32(1.0 + DELTA)
    assert corner.sum() == 24 and (np.abs(dc[corner] - DELTA * math.sqrt(3)) <= tol).all()
    assert err.precision[THRESHOLDS[0]] == 1.0 and err.recall[THRESHOLDS[2]] == 1.0
    for t in THRESHOLDS:
        p, r = err.precision[t], err.recall[t]
        assert r == float((dc <= f32(t)).sum()) / dc.size and err.f_score[t] == 2 * p * r / (p + r)
    assert 0 < err.recall[THRESHOLDS[0]] < err.recall[THRESHOLDS[1]] < 1.0
    for q in (0.0, 0.3, 0.5, 0.9, 0.95, 0.99, 1.0):
        assert err.margin(q) == float(np.quantile(dc, q, method="inverted_cdf"))


def stats_arrays():
    """hand-built distance arrays with +inf entries: N in (1, 63, 64, 65, 4097) and an empty one"""
    rng = np.random.default_rng(5)
    out = {}
    for n in (0, 1, 63, 64, 65, 4097):
        d = (rng.uniform(0, 1, n) ** 4 * 3).astype(f32)
        d[rng.uniform(0, 1, n) < 0.1] = np.inf
        if n >= 63:
            d[5], d[62] = 0.0, 0.25
        out[n] = d
    out["inf"] = np.full(70, np.inf, f32)
    return out


STATS_THRESHOLDS = (0.0, 0.25, 0.5, 1.0, 2.9, 3.5)
