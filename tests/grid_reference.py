"""The multiresolution grid encoder restated in plain NumPy float64, independently of oracle/: the level geometry, the corner entries
and weights of every point, the forward interpolation, and the table-gradient scatter with a per-entry error bound.

Method.  Only what decides WHICH entries a point touches is done in the kernels' own precision; everything else is float64.
  * level scale     exp2f(l * S) * H - 1 in fp32, exp2f from the host's libm through ctypes (fill_levels evaluates exactly this on the
                    host); resolution = ceil(scale) + 1.
  * position        the kernels form fmaf(x, scale, 0.5 or 0): ONE rounding.  x * scale + offset is evaluated in float64 (a 48-bit
                    product plus 0.5: exact for every x >= 2^-5 / scale and for x = 0) and rounded once to float32.  floor and the
                    fraction come from that value (the fraction is exact in fp32); the weights are float64 products of the fractions.
  * entry           the stride loop over the dimensions in 32-bit wrap-around arithmetic, the three-prime xor hash when the level
                    does not fit and the grid type is `hash`, then the modulo -- for both grid types, align_corners and D = 2, 3.
  * scatter         per level, from E[B, 2^D] (entry) and W[B, 2^D] (weight) and a gradient g[B, C], with np.bincount:
                    want = sum w * g, A = sum |w * g|, k = number of contributions of in-range points whose gradient is not zero
                    in every channel (the kernels emit nothing for the others).

The bound of the comparison.  For every entry e and channel:  |got - want| <= R(k_e) * u * A_e + R(k_e) * tiny,  u the unit roundoff
of the table type.  R counts the roundings that a legitimate route of csrc/gridencoder.hip can put on an entry with k contributions:

  fp16 tables, R = 3k + 2, u = 2^-11, tiny = 2^-14.  Read off the code:
    - counted per event, as the issue does: each of the k contributions is rounded to half at most once when it becomes a record of
      the binned first pass (to_half2) or part of a flushed partial sum (k); an entry sees at most k atomics, because every atomic
      carries at least one contribution of its own -- a run, a record, a flushed slice --, and each rounds its operand
      (__float2half_rn in table_add) and the running sum (2k); all the fp32 work before that -- the 2D roundings of the weight,
      w * g, at most six additions of a segmented sum, the int64 -> float conversions of the fixed-point sums: below
      16 * 2^-24 A = 2^-9 u A -- and a record that the bin reduce sums and converts once more take the last 2.
    - counted per contribution, which is tighter: the longest route is merge -> record (one half rounding of the partial sum it is
      in) -> exact fixed-point reduce -> flush (a second one) -> m <= k atomics that round a running sum holding it: k + 2 half
      roundings, + 1 for the fp32 work = k + 3 <= 3k + 2 for every k >= 1.  The difference pays for the second-order terms:
      (1 + u)^(k + 3) - 1 <= (3k + 2) u up to k = 3800 (only level 0 of the dense input has fuller entries; it accumulates in LDS
      and issues one atomic per workgroup, m <= 256).
    The 3k + 2 of the issue therefore holds on every route and is kept as stated.  R * tiny covers an atomic unit that flushes
    subnormal halves (operand and result of each of the <= k atomics) and the fixed-point units 2^-24, 2^-26 and 2^-30 (half a
    unit per addition, k additions).
  fp32 tables, R = 2k + 6, u = 2^-24, tiny = 2^-126.  2D <= 6 roundings on the way to w * g (D for 1 - f, D - 1 for the products, one
    for the multiply), and the k contributions are joined by at most k fp32 additions (segmented sums, LDS float atomics, table
    atomics: a tree with k leaves); the other k is room for second order.  No fixed point and no halves on this route, so `tiny` is
    the smallest normal float (a float atomic may flush a denormal), not the 2^-14 the fp16 routes need: stricter than asked.

No term is fitted to a kernel's output.  An entry with k = 0 must read back as zero bits; the converse is not required (sums cancel).

What the bound sees: one lost, doubled or misfiled contribution c is certain to fail when |c| > 2 * bound at its entry (the rest of
the entry's error is at most bound).  detectable_share() is the share of contributions for which that holds, from the reference alone.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_PRIMES = (1, 2654435761, 805459861)
UNIT = {np.dtype(np.float16): 2.0 ** -11, np.dtype(np.float32): 2.0 ** -24}
TINY = {np.dtype(np.float16): 2.0 ** -14, np.dtype(np.float32): 2.0 ** -126}


@functools.lru_cache(maxsize=None)
def _exp2f():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.exp2f.restype = ctypes.c_float
    libm.exp2f.argtypes = [ctypes.c_float]
    return libm.exp2f


def level_table(D, L, log2_hashmap_size, desired_resolution=2048, H=16, align_corners=False):
    """(offsets int32 [L + 1], per_level_scale): entries per level = min(2^log2_hashmap_size, (resolution [+ 1])^D) rounded up to 8"""
    pls = np.exp2(np.log2(desired_resolution / H) / (L - 1))
    offsets = [0]
    for l in range(L):
        r = int(np.ceil(H * pls ** l))
        n = min(2 ** log2_hashmap_size, (r if align_corners else r + 1) ** D)
        offsets.append(offsets[-1] + (n + 7) // 8 * 8)
    return np.array(offsets, np.int32), pls


def level_geometry(L, per_level_scale, H=16):
    """(scale float32[L], resolution int[L]): exp2f(l * S) * H - 1 with every operation in fp32, S = log2(per_level_scale) as a C float"""
    S = np.float32(np.log2(per_level_scale))
    scale = np.empty(L, np.float32)
    for l in range(L):
        e = np.float32(_exp2f()(float(np.float32(l) * S)))
        scale[l] = np.float32(e * np.float32(H)) - np.float32(1.0)
    return scale, [int(np.ceil(s)) + 1 for s in scale]


def _entry(pc, size, res, gridtype, align_corners):
    """pc uint64 [n, D] grid coordinates -> entry index in the level (uint32 wrap-around arithmetic)"""
    D = pc.shape[1]
    step = res if align_corners else res + 1
    stride, index = 1, np.zeros(pc.shape[0], np.uint64)
    for d in range(D):
        if stride <= size:
            index = (index + pc[:, d] * np.uint64(stride)) & _M32
            stride = (stride * step) & 0xFFFFFFFF
    if gridtype == 0 and stride > size:
        index = np.zeros(pc.shape[0], np.uint64)
        for d in range(D):
            index ^= (pc[:, d] * np.uint64(_PRIMES[d])) & _M32
    return index % np.uint64(size)


def corners(x, offsets, per_level_scale, H=16, gridtype=0, align_corners=False):
    """x float32 [B, D] -> E int32 [L, B, 2^D] (entry within its level), W float64 [L, B, 2^D], inb bool [B] (every coordinate in [0, 1]).
    Rows of points outside the range hold entry 0 with weight 0."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] in (2, 3)
    B, D = x.shape
    L = len(offsets) - 1
    scale, res = level_geometry(L, per_level_scale, H)
    inb = ~((x < 0) | (x > 1)).any(axis=1)
    xd = np.where(inb[:, None], x, np.float32(0)).astype(np.float64)
    E = np.zeros((L, B, 1 << D), np.int32)
    W = np.zeros((L, B, 1 << D), np.float64)
    for l in range(L):
        size = int(offsets[l + 1]) - int(offsets[l])
        p = (xd * float(scale[l]) + (0.0 if align_corners else 0.5)).astype(np.float32)      # one rounding, as fmaf
        pg = np.floor(p)
        fr = (p - pg).astype(np.float64)                                                      # exact in fp32
        pg = pg.astype(np.uint64)
        for idx in range(1 << D):
            w = np.ones(B, np.float64)
            pc = pg.copy()
            for d in range(D):
                hi = (idx >> d) & 1
                w *= fr[:, d] if hi else 1.0 - fr[:, d]
                pc[:, d] += np.uint64(hi)
            E[l, :, idx] = _entry(pc, size, res[l], gridtype, align_corners).astype(np.int32)
            W[l, :, idx] = w
        E[l, ~inb] = 0
        W[l, ~inb] = 0.0
    return E, W, inb


def forward(x, emb, offsets, per_level_scale, H=16, gridtype=0, align_corners=False):
    """the interpolated features, float64 [B, L * C] (zero for points outside [0, 1])"""
    E, W, _ = corners(x, offsets, per_level_scale, H, gridtype, align_corners)
    L, B, _ = E.shape
    emb = np.asarray(emb, np.float64)
    out = np.zeros((B, L, emb.shape[1]))
    for l in range(L):
        out[:, l] = (W[l][:, :, None] * emb[int(offsets[l]) + E[l]]).sum(axis=1)
    return out.reshape(B, -1)


def live_points(inb, g):
    """the points that contribute: in range and with a gradient that is not zero in every channel.  g [B, C]"""
    return inb & (np.asarray(g) != 0).any(axis=1)


def scatter(E, W, inb, g, size):
    """one level: E, W [B, 2^D], g [B, C] -> want float64 [size, C], A float64 [size, C], k int64 [size]"""
    g = np.asarray(g, np.float64)
    live = live_points(inb, g)
    e = E[live].ravel()
    w = W[live]
    C = g.shape[1]
    want, A = np.zeros((size, C)), np.zeros((size, C))
    for c in range(C):
        v = (w * g[live, c][:, None]).ravel()
        want[:, c] = np.bincount(e, v, minlength=size)
        A[:, c] = np.bincount(e, np.abs(v), minlength=size)
    return want, A, np.bincount(e, minlength=size)


def rounding_count(k, dtype):
    """R(k) of the module docstring"""
    k = np.asarray(k, np.float64)
    return 3.0 * k + 2.0 if np.dtype(dtype) == np.float16 else 2.0 * k + 6.0


def bound(A, k, dtype):
    """R(k) u A + R(k) tiny per entry and channel.  A [size, C], k [size]"""
    R = rounding_count(k, dtype)[:, None]
    return R * UNIT[np.dtype(dtype)] * A + R * TINY[np.dtype(dtype)]


def compare(got, want, A, k, dtype):
    """-> (worst error / bound, entries that exceed it, untouched entries that are not zero bits).  Every entry takes part."""
    got = np.asarray(got)
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / bound(A, k, dtype)
    bits = got.view(np.uint16 if got.dtype == np.float16 else np.uint32)
    stray = np.flatnonzero((k == 0) & (bits != 0).any(axis=1))
    bad = np.flatnonzero(~(ratio <= 1.0).all(axis=1))           # (a NaN fails)
    return float(ratio.max(initial=0.0)) if not np.isnan(ratio).any() else float("nan"), bad, stray


def detectable_share(E, W, inb, g, A, k, dtype):
    """share of a level's contributions c with |c| > 2 * bound at their entry in at least one channel (A, k from scatter())"""
    g = np.asarray(g, np.float64)
    bd = bound(A, k, dtype)
    live = live_points(inb, g)
    e, w = E[live], W[live]
    c = np.abs(w[:, :, None] * g[live][:, None, :])
    seen = (c > 2.0 * bd[e]).any(axis=2)
    return float(seen.mean()) if seen.size else 0.0


def expected(E, W, inb, g, offsets, dtype=None):
    """all levels: g [L, B, C] -> want [n, C], A [n, C], k [n] over the whole table (n = offsets[-1]) and, with a dtype, the
    detectable share of every level"""
    L = len(offsets) - 1
    n, C = int(offsets[-1]), g.shape[2]
    want, A, k = np.zeros((n, C)), np.zeros((n, C)), np.zeros(n, np.int64)
    shares = []
    for l in range(L):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        want[lo:hi], A[lo:hi], k[lo:hi] = scatter(E[l], W[l], inb, g[l], hi - lo)
        if dtype is not None:
            shares.append(detectable_share(E[l], W[l], inb, g[l], A[lo:hi], k[lo:hi], dtype))
    return want, A, k, shares


def compare_levels(got, want, A, k, offsets, dtype):
    """compare() per level -> list of (worst ratio, failing entries, stray entries), entry numbers within the level"""
    return [compare(got[lo:hi], want[lo:hi], A[lo:hi], k[lo:hi], dtype)
            for lo, hi in zip(map(int, offsets[:-1]), map(int, offsets[1:]))]


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs the CPU and GPU tests share
# ---------------------------------------------------------------------------------------------------------------------------------
def ray_points(n_rays, T, D, seed, t_max=0.35):
    """n_rays x T samples in ray order: o ~ U(0.3, 0.7), unit directions, t in [0, t_max] -> float32 [n_rays * T, D]
    (the far ends of some rays leave [0, 1])"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.3, 0.7, (n_rays, 1, D))
    d = rng.normal(size=(n_rays, 1, D))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (o + d * np.linspace(0, t_max, T).reshape(1, T, 1)).reshape(-1, D).astype(np.float32)


def dense_gradient(B, L, C, seed, dtype=np.float16):
    """N(0, 1) rounded to `dtype` on every sample, level-major [L, B, C]"""
    return np.random.default_rng(seed).normal(size=(L, B, C)).astype(np.float32).astype(dtype)


NERF_RAYS, NERF_SAMPLES, NERF_LEVELS, NERF_FEATURES, NERF_LOG2_T = 640, 256, 16, 2, 19
# name -> (one run per this many samples, seed, shortest and longest run)
NERF_KINDS = {"dense": (None, 1, None), "bursts400": (400, 2, (1, 5)), "bursts4000": (4000, 3, (1, 5)), "runs4000": (4000, 4, (6, 16))}


def nerf_points():
    """the 163 840 ray-ordered points of the NeRF-shaped cases (D = 3, L = 16, T = 2^19, C = 2)"""
    return ray_points(NERF_RAYS, NERF_SAMPLES, 3, seed=101)


def nerf_gradient(kind):
    """fp16 [16, 163840, 2]: N(0, 1) on every sample (`dense`), on isolated runs of 1 to 5 samples (`bursts400`, `bursts4000`) or of
    6 to 16 samples (`runs4000`: same-cell chains long enough for every round of the kernels' segmented sums)"""
    B = NERF_RAYS * NERF_SAMPLES
    every, seed, lengths = NERF_KINDS[kind]
    if every is None:
        return dense_gradient(B, NERF_LEVELS, NERF_FEATURES, seed)
    return burst_gradient(B, NERF_LEVELS, NERF_FEATURES, B // every, seed, lengths=lengths)


def burst_gradient(B, L, C, n_runs, seed, dtype=np.float16, lengths=(1, 5)):
    """N(0, 1) on n_runs runs of lengths[0] to lengths[1] consecutive samples, zero elsewhere (zero on both sides of a run: run heads
    and tails).  Runs start at multiples of 8, so the longer ones also cross the 16-lane rows the kernels merge in."""
    rng = np.random.default_rng(seed)
    on = np.zeros(B, bool)
    gap = 8 * (2 + lengths[1] // 8)                              # runs never touch
    start = rng.choice(B // gap, n_runs, replace=False) * gap
    if lengths[1] > 8:
        start += 8 * rng.integers(0, 2, n_runs)
    for s, n in zip(start, rng.integers(lengths[0], lengths[1] + 1, n_runs)):
        on[s:s + n] = True
    g = rng.normal(size=(L, B, C)).astype(np.float32).astype(dtype)
    g[:, ~on] = 0
    return g
