"""The overlay cast's shared cases (tests/test_overlay_cpu.py, tests/test_overlay_gpu.py): a fixed set of primitives, two 40 x 56
frames, float64 geometry that does not use the rule's closed forms, and the numpy path's result, computed once and read-only."""
import functools

import numpy as np

import raycast_cases as RC
from nerfsafetyvalidation_amd import world as WO

f32 = np.float32
H, W = 40, 56
RADIUS, HALF = 0.02, 0.0125
VIEW = np.array([0.3, 0.2, -1.0]) / np.linalg.norm([0.3, 0.2, -1.0])       # the cameras sit at VIEW * distance and look at the origin
CLOSE, FAR = 0.5, 4.0
MARGIN = 1e-4                                                              # test_world_gpu.py's silhouette margin for the cube

POLYLINE = np.array([[-0.20, -0.10, 0.02], [-0.12, 0.06, -0.03], [-0.02, -0.05, 0.04], [0.06, 0.08, -0.02], [0.15, -0.04, 0.03],
                     [0.21, 0.07, 0.00]], f32)
SPHERE = np.array([0.05, -0.10, -0.02], f32)                               # the degenerate capsule, a == b
ALONG = np.array([-0.10, -0.02, 0.0])                                      # a capsule along the view direction, through this point
CUBES = np.array([[0.12, 0.10, -0.05],                                     # in the open
                  [-0.14, -0.11, 0.01],                                    # in the open
                  POLYLINE[2] - 0.08 * VIEW], f32)                         # behind the tube's joint at POLYLINE[2], seen from the cameras
# prims 0..4 the polyline, 5 the sphere, 6 the capsule along the view, 7..9 the cubes
N_TUBE = 7


@functools.lru_cache(None)
def prims():
    along = np.stack([ALONG + 0.06 * VIEW, ALONG - 0.06 * VIEW]).astype(f32)
    q, _ = WO.overlay_prims(tubes=[(POLYLINE, RADIUS, (1, 0, 0)), (SPHERE[None], 0.03, (0, 1, 0)), (along, RADIUS, (0, 0, 1))],
                            boxes=[(CUBES, (HALF, HALF, HALF), (1, 1, 0))])
    q.setflags(write=False)
    return q


COLORS = np.concatenate([np.tile([[0.9, 0.2, 0.1]], (5, 1)), [[0.1, 0.8, 0.2]], [[0.2, 0.3, 0.9]], np.tile([[0.9, 0.8, 0.1]], (3, 1))]).astype(f32)


@functools.lru_cache(None)
def frame(which):
    """-> (o, d) float32 [H W, 3] (unit d), read-only: "close" from CLOSE, "far" from FAR with a field of view that keeps the scene's size
    in pixels"""
    dist = CLOSE if which == "close" else FAR
    o, d = RC.pinhole(VIEW * dist, -VIEW, [0.0, 1.0, 0.0], H=H, W=W, angle=2 * np.arctan(0.27 / dist))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


# ---- float64 geometry: signed distances, nothing of the rule's algebra
def sdf_each(x, q=None):
    """signed distance of the points x [..., P, 3] (float64), point p of a row to primitive p -> [..., P]: |x - segment| - r, or the
    box's signed distance"""
    q = np.asarray(prims() if q is None else q, np.float64)
    x = np.asarray(x, np.float64)
    a, b, r = q[:, 1:4], q[:, 4:7], q[:, 7]
    ba = b - a
    baba = (ba * ba).sum(-1)
    s = np.clip(((x - a) * ba).sum(-1) / np.where(baba > 0, baba, 1.0), 0.0, 1.0)
    cap = np.linalg.norm(x - (a + s[..., None] * ba), axis=-1) - r
    e = np.abs(x - a) - b
    box = np.linalg.norm(np.maximum(e, 0.0), axis=-1) + np.minimum(e.max(-1), 0.0)
    return np.where(q[:, 0] == 0, cap, box)


def sdf(points, q=None):
    """signed distance of points [..., 3] to every primitive -> [..., P]"""
    P = (prims() if q is None else q).shape[0]
    x = np.asarray(points, np.float64)
    return sdf_each(np.broadcast_to(x[..., None, :], x.shape[:-1] + (P, 3)), q)


def ray_clearance(o, d, q=None, reach=8.0, iters=64):
    """the smallest signed distance along every ray (t in [0, reach]) to every primitive -> [N, P] float64: golden-section search on
    the distance along the ray, which is convex in t (the primitives are convex); 0.618^64 of the reach is left of the bracket"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    P = (prims() if q is None else q).shape[0]
    lo, hi = np.zeros((o.shape[0], P)), np.full((o.shape[0], P), float(reach))
    g = (np.sqrt(5.0) - 1) / 2
    at = lambda t: sdf_each(o[:, None, :] + t[..., None] * d[:, None, :], q)
    for _ in range(iters):
        m1, m2 = hi - g * (hi - lo), lo + g * (hi - lo)
        left = at(m1) < at(m2)
        hi, lo = np.where(left, m2, hi), np.where(left, lo, m1)
    return at((lo + hi) / 2)


@functools.lru_cache(None)
def clearance(which):
    """ray_clearance of frame(which) against prims(): computed once, shared, read-only"""
    o, d = frame(which)
    c = ray_clearance(o, d, reach=2 * (CLOSE if which == "close" else FAR))
    c.setflags(write=False)
    return c


@functools.lru_cache(None)
def reference(which):
    """the numpy path's result on frame(which) against prims(): computed once, shared, read-only"""
    o, d = frame(which)
    out = WO.cast_overlay_numpy(o, d, prims())
    for a in out.values():
        a.setflags(write=False)
    return out


def straddling_prims(P, seed=3):
    """P unique primitives (capsules and boxes, alternating) in the cameras' view; record 255 and record 256 (the last of an LDS chunk
    and the first of the next), where they exist, sit in front of all others so that rays hit exactly them"""
    rng = np.random.default_rng(seed + P)
    c = rng.uniform(-0.2, 0.2, (P, 3))
    q = np.zeros((P, 8), f32)
    q[:, 0] = np.arange(P) % 2
    q[:, 1:4] = c
    q[:, 4:7] = np.where(q[:, 0:1] == 0, c + rng.uniform(-0.05, 0.05, (P, 3)), rng.uniform(0.005, 0.02, (P, 3)))
    q[:, 7] = np.where(q[:, 0] == 0, rng.uniform(0.008, 0.02, P), 1.0)
    right = np.cross(VIEW, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, VIEW)
    for i, (x, y) in ((255, (-0.06, 0.0)), (256, (0.06, 0.0)), (511, (0.0, 0.045)), (512, (0.0, -0.045))):
        if i < P:
            centre = VIEW * 0.3 + right * x + up * y
            q[i, 1:4] = centre
            q[i, 4:7] = centre + [0.0, 0.02, 0.0] if q[i, 0] == 0 else [0.015, 0.015, 0.015]
            q[i, 7] = 0.015 if q[i, 0] == 0 else 1.0
    return q


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
