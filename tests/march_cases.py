"""Hand-built occupancy grids, bounds and rays for the occupancy march (test_march_cases_cpu.py, test_march_gpu.py), and the CPU
oracle's answers on them.  numpy and the project's own oracle only; everything is built once per process (lru_cache) and must not be
modified by a test.

A configuration is (bound, C, H, max_steps, dt_gamma, perturb).  Per configuration:

  grids(C, H)       four bool grids occ[C, x, y, z] and their bitfields (pack: bit level * H^3 + morton3D(x, y, z), LSB first in a byte)
      random        30 % of the cells, independent per level
      blocks        a 3-D checkerboard of 4x4x4 blocks (its phase alternates with the level): the coarse bits and the block jump
      corners       only (0,0,0), (H-1,H-1,H-1) and one cell next to the centre, on every level
      shell         the cells whose centre lies at a radius in (0.55, 0.7) of the level's cube

  rays(bound, H)    2048 rays: four families of 512, each 496 rays and then 16 that miss the box (near = far = FLT_MAX)
      inside        origins uniform in +-0.9 bound, random unit directions
      outside       from 2.2 bound away, aimed at a point in +-0.5
      axis          direction exactly +-e_k with the next component +0.0 or -0.0; the other two origin components on the level-0 cell
                    lattice j * 2 / H - 1, j in [0, H]; the origin 1.25 bound out along the axis
      diagonal      direction (+-1, +-1, +-1) / sqrt(3) through a lattice corner point, starting 1.5 bound (per axis) before it; two in
                    five along the cube's main diagonal (the only ones that meet the `corners` grid's corner cells)
    nears / fars are the oracle's near_far_from_aabb with min_near = 0.05.
"""
import collections
import functools

import numpy as np

from oracle import oracle as O

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
MIN_NEAR = 0.05
FAMILIES = ("inside", "outside", "axis", "diagonal")
PER_FAMILY, MISSES = 512, 16
N_RAYS = PER_FAMILY * len(FAMILIES)
GRIDS = ("random", "blocks", "corners", "shell")

Config = collections.namedtuple("Config", "bound C H max_steps dt_gamma perturb")
CONFIGS = (
    Config(1.0, 1, 128, 1024, 0.0, 0),           # one cascade, derived copies
    Config(2.0, 2, 128, 1024, 1.0 / 128, 0),     # exactly at the coarse cap; cone steps
    Config(4.0, 3, 128, 512, 0.0, 0),            # above the cap: plain kernels; many rays fill the budget
    Config(8.0, 4, 64, 1024, 0.0, 0),            # copies, budget filled inside lattice windows
    Config(16.0, 5, 64, 1024, 1.0 / 256, 1),     # five levels, cone steps, jitter
    Config(1.5, 2, 64, 256, 0.0, 0),             # non-power-of-two bound
    Config(3.0, 3, 32, 128, 0.0, 1),             # non-power-of-two bound, jitter
    Config(1.0, 1, 16, 64, 0.0, 0),              # smallest single cascade with copies; words of the linear copy span two rows
    Config(8.0, 8, 8, 128, 0.0, 0),              # H = 8 has copies only at C = 8
    Config(1.0, 1, 8, 64, 0.0, 0),               # 512 cells, not a multiple of 4096: no copies
    Config(2.0, 2, 64, 1100, 0.0, 0),            # max_steps > 1024: no (t, dt) trace
)


def config_id(cfg):
    return "b%g_C%d_H%d_s%d_g%g_p%d" % (cfg.bound, cfg.C, cfg.H, cfg.max_steps, cfg.dt_gamma, cfg.perturb)


def bits(a):
    """uint32 view of a float32 array (bit-exact comparisons, NaN included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------------------- bitfields
def is_pow2(H):
    return H >= 1 and (H & (H - 1)) == 0


def expand_bits(v):
    """bit i of v (v < 1024) -> bit 3 i"""
    v = np.asarray(v, np.uint32)
    out = np.zeros_like(v)
    for i in range(10):
        out |= ((v >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i)
    return out


def morton3D(x, y, z):
    return expand_bits(x) | (expand_bits(y) << np.uint32(1)) | (expand_bits(z) << np.uint32(2))


def cell_bit_index(C, H):
    """uint32 [C, H, H, H]: bit index of cell (level, x, y, z) in the bitfield"""
    if not is_pow2(H):
        raise ValueError("grid size %d is not a power of two: morton3D(x, y, z) would exceed H^3" % H)
    i = np.arange(H, dtype=np.uint32)
    m = morton3D(i[:, None, None], i[None, :, None], i[None, None, :])
    return (np.arange(C, dtype=np.uint32) * np.uint32(H ** 3))[:, None, None, None] + m[None]


def pack(occ):
    """occ bool [C, H, H, H] indexed (level, x, y, z) -> uint8 [C * H^3 / 8]"""
    occ = np.asarray(occ, bool)
    C, H = occ.shape[0], occ.shape[1]
    assert occ.shape == (C, H, H, H)
    idx = cell_bit_index(C, H)
    if (C * H ** 3) % 8:
        raise ValueError("C * H^3 = %d cells do not fill whole bytes" % (C * H ** 3))
    flat = np.zeros(C * H ** 3, np.uint8)
    flat[idx.ravel()] = occ.ravel()
    return np.packbits(flat, bitorder="little")


def unpack(bitfield, C, H):
    """the inverse of pack"""
    flat = np.unpackbits(np.asarray(bitfield, np.uint8), bitorder="little")
    return flat[cell_bit_index(C, H)].astype(bool)


def _occ(name, C, H):
    rng = np.random.default_rng(1000 * C + H)
    i = np.arange(H)
    X, Y, Z = np.meshgrid(i, i, i, indexing="ij")
    occ = np.zeros((C, H, H, H), bool)
    for level in range(C):
        if name == "random":
            occ[level] = rng.random((H, H, H)) < 0.3
        elif name == "blocks":
            occ[level] = (((X >> 2) + (Y >> 2) + (Z >> 2) + level) & 1) == 0
        elif name == "corners":
            occ[level, 0, 0, 0] = occ[level, H - 1, H - 1, H - 1] = True
            occ[level, H // 2, H // 2 - 1, H // 2] = True
        elif name == "shell":
            c = (i + 0.5) * 2.0 / H - 1.0
            r = np.sqrt(c[X] ** 2 + c[Y] ** 2 + c[Z] ** 2)
            occ[level] = (r > 0.55) & (r < 0.7)
        else:
            raise KeyError(name)
    return occ


@functools.lru_cache(maxsize=None)
def grid(name, C, H):
    """-> (occ bool [C,H,H,H], bitfield uint8 [C H^3 / 8]), read-only"""
    occ = _occ(name, C, H)
    bf = pack(occ)
    occ.setflags(write=False)
    bf.setflags(write=False)
    return occ, bf


def corner_cells(C, H):
    """the eight cube corners of every level: (level, x, y, z)"""
    return [(l, x, y, z) for l in range(C) for x in (0, H - 1) for y in (0, H - 1) for z in (0, H - 1)]


def single_bit(C, H, cell):
    occ = np.zeros((C, H, H, H), bool)
    occ[cell] = True
    return occ, pack(occ)


# ---------------------------------------------------------------------------------------------------------------- derived copies
def ceil256(n):
    return (n + 255) // 256 * 256


def lin_bytes(C, H):
    """ngp_occupancy_lin_bytes by its documented rule: H a power of two >= 8, 1 <= C <= 8, whole 4096-cell units, the x-fastest copy
    within 1 MiB and the 4x4x4-block bits within 8 KiB"""
    cells = C * H ** 3
    if not (1 <= C <= 8 and 8 <= H <= 1024 and is_pow2(H)) or cells % 4096 or cells // 8 > (1 << 20) or cells // 512 > 8192:
        return 0
    return ceil256(cells // 8) + cells // 512


def lin_reference(occ):
    """-> (linear copy, coarse copy) as uint8 arrays: bit (level, z, y, x) x-fastest, and one bit per 4x4x4 block (level, bz, by, bx)"""
    C, H = occ.shape[0], occ.shape[1]
    lin = np.packbits(np.ascontiguousarray(occ.transpose(0, 3, 2, 1)).ravel().astype(np.uint8), bitorder="little")
    B = H // 4
    blocks = occ.reshape(C, B, 4, B, 4, B, 4).any(axis=(2, 4, 6))                  # (level, bx, by, bz)
    coarse = np.packbits(np.ascontiguousarray(blocks.transpose(0, 3, 2, 1)).ravel().astype(np.uint8), bitorder="little")
    return lin, coarse


# ---------------------------------------------------------------------------------------------------------------- rays
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _family(name, rng, bound, H, n, n_miss):
    lattice = lambda size: (rng.integers(0, H + 1, size=size) * (2.0 / H) - 1.0)      # noqa: E731  (exact in float32: H a power of two)
    m = n + n_miss
    if name == "inside":
        o = rng.uniform(-0.9 * bound, 0.9 * bound, (m, 3))
        d = _unit(rng, m)
    elif name == "outside":
        o = 2.2 * bound * _unit(rng, m)
        d = rng.uniform(-0.5, 0.5, (m, 3)) - o
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
    elif name == "axis":
        k = rng.integers(0, 3, m)
        sgn = rng.choice([-1.0, 1.0], m)
        o = lattice((m, 3))
        o[np.arange(m), k] = -sgn * 1.25 * bound
        d = np.zeros((m, 3))
        d[np.arange(m), k] = sgn
        d[np.arange(m), (k + 1) % 3] = rng.choice([-0.0, 0.0], m)
    elif name == "diagonal":
        s = rng.choice([-1.0, 1.0], (m, 3))
        p = lattice((m, 3))
        main = np.arange(m) < 2 * n // 5          # two in five run along the cube's main diagonal, through the corner cells of every level
        s[main] = s[main, :1]
        p[main] = p[main, :1]
        o = p - s * 1.5 * bound
        d = s / np.sqrt(3.0)
    else:
        raise KeyError(name)
    if n_miss:
        # the misses: the x slab and the y slab are met at disjoint times (near_far_from_aabb's first test)
        r = slice(n, m)
        if name in ("inside", "outside"):
            o[r, 0] = rng.uniform(-0.5, 0.5, n_miss) * bound
            o[r, 1] = 2.0 * bound
            dd = np.stack([rng.choice([-1.0, 1.0], n_miss), rng.uniform(0.02, 0.2, n_miss), rng.uniform(-0.3, 0.3, n_miss)], -1)
            d[r] = dd / np.linalg.norm(dd, axis=-1, keepdims=True)
        elif name == "axis":
            o[r] = lattice((n_miss, 3))
            o[r, 1] = 2.0 * bound
            d[r] = 0.0
            d[r, 0] = rng.choice([-1.0, 1.0], n_miss)
            d[r, 2] = rng.choice([-0.0, 0.0], n_miss)
        else:
            o[r, 0] = lattice(n_miss) - 3.0 * bound * s[r, 0]
            o[r, 1] = lattice(n_miss) + 1.5 * bound * s[r, 1]
    return o.astype(f32), d.astype(f32)


Rays = collections.namedtuple("Rays", "rays_o rays_d nears fars family miss")


@functools.lru_cache(maxsize=None)
def rays(bound, H):
    """-> Rays: rays_o, rays_d float32 [2048,3], nears, fars float32 [2048], family: name -> slice, miss bool [2048]; read-only"""
    rng = np.random.default_rng(int(round(bound * 2)) * 4096 + H)
    os_, ds, family = [], [], {}
    miss = np.zeros(N_RAYS, bool)
    for i, name in enumerate(FAMILIES):
        o, d = _family(name, rng, bound, H, PER_FAMILY - MISSES, MISSES)
        os_.append(o)
        ds.append(d)
        family[name] = slice(i * PER_FAMILY, (i + 1) * PER_FAMILY)
        miss[(i + 1) * PER_FAMILY - MISSES:(i + 1) * PER_FAMILY] = True
    rays_o, rays_d = np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds))
    aabb = np.array([-bound] * 3 + [bound] * 3, f32)
    nears, fars = np.empty(N_RAYS, f32), np.empty(N_RAYS, f32)
    O.near_far_from_aabb(rays_o, rays_d, aabb, N_RAYS, MIN_NEAR, nears, fars)
    for a in (rays_o, rays_d, nears, fars, miss):
        a.setflags(write=False)
    return Rays(rays_o, rays_d, nears, fars, family, miss)


def subset(r, index):
    """the rays `index` selects (contiguous copies), as (rays_o, rays_d, nears, fars)"""
    return tuple(np.ascontiguousarray(a[index]) for a in (r.rays_o, r.rays_d, r.nears, r.fars))


# ---------------------------------------------------------------------------------------------------------------- the oracle's marches
Train = collections.namedtuple("Train", "xyzs dirs deltas rays counter")


def oracle_train(cfg, bitfield, rays_o, rays_d, nears, fars):
    """O.march_rays_train with M = N * max_steps rows (no ray is dropped), the outputs cut to the samples taken"""
    N = rays_o.shape[0]
    M = N * cfg.max_steps
    xyzs, dirs, deltas = np.zeros((M, 3), f32), np.zeros((M, 3), f32), np.zeros((M, 2), f32)
    table, counter = np.zeros((N, 3), np.int32), np.zeros(2, np.int32)
    O.march_rays_train(rays_o, rays_d, bitfield, cfg.bound, cfg.dt_gamma, cfg.max_steps, N, cfg.C, cfg.H, M, nears, fars, xyzs, dirs, deltas,
                       table, counter, cfg.perturb)
    m = int(counter[0])
    return Train(xyzs[:m].copy(), dirs[:m].copy(), deltas[:m].copy(), table, counter)


@functools.lru_cache(maxsize=4)      # (up to 60 MB each)
def train_reference(ci, grid_name):
    """the oracle's march_rays_train of configuration CONFIGS[ci] on all 2048 rays; read-only"""
    cfg = CONFIGS[ci]
    r = rays(cfg.bound, cfg.H)
    out = oracle_train(cfg, grid(grid_name, cfg.C, cfg.H)[1], r.rays_o, r.rays_d, r.nears, r.fars)
    for a in out:
        a.setflags(write=False)
    return out


def padded(m, align=128):
    """the wrapper's row count (adds a full `align` when already aligned, as the reference does)"""
    return m + align - m % align


def oracle_march(cfg, bitfield, r, alive, rays_t, n_step, align=128):
    """O.march_rays on the rays `alive` from `rays_t`, into zeroed buffers of padded(n_alive * n_step) rows -> xyzs, dirs, deltas"""
    n_alive = alive.shape[0]
    M = padded(n_alive * n_step, align)
    xyzs, dirs, deltas = np.zeros((M, 3), f32), np.zeros((M, 3), f32), np.zeros((M, 2), f32)
    O.march_rays(n_alive, n_step, alive, rays_t, r.rays_o, r.rays_d, cfg.bound, cfg.dt_gamma, cfg.max_steps, cfg.C, cfg.H, bitfield, r.nears,
                 r.fars, xyzs, dirs, deltas, cfg.perturb)
    return xyzs, dirs, deltas


def oracle_advance(alive, rays_t, deltas, n_step):
    """O.composite_rays with zero density: rays_t moves past the samples taken; a ray that took fewer than n_step is finished.
    -> (the rays still alive, compacted as the render loop compacts them; the new rays_t)"""
    n_alive = alive.shape[0]
    alive, rays_t = alive.copy(), rays_t.copy()
    rows = n_alive * n_step
    N = rays_t.shape[0]
    sig, rgb = np.zeros(rows, f32), np.zeros((rows, 3), f32)
    ws, dp, im = np.zeros(N, f32), np.zeros(N, f32), np.zeros((N, 3), f32)
    O.composite_rays(n_alive, n_step, alive, rays_t, sig, rgb, np.ascontiguousarray(deltas[:rows]), ws, dp, im)
    return np.ascontiguousarray(alive[alive >= 0]), rays_t


# ---------------------------------------------------------------------------------------------------------------- coverage statistics
def samples_per_ray(train):
    """int [N]: the count of ray n (the table's rows are in ray order)"""
    assert np.array_equal(train.rays[:, 0], np.arange(train.rays.shape[0]))
    return train.rays[:, 2]


def boundary_crossings(cfg, occ, r, train):
    """bool [N]: rays with a sample in the top cascade (max norm >= 2^(C-2)) whose next lattice point, one step on, lies in the SAME
    top-level cell, has max norm < 2^(C-2) and falls in an EMPTY cell of the level below -- where a march that takes the occupied
    top-level cell's exit for the end of the run of samples goes wrong.  Only a non-power-of-two bound puts the cube surface of the
    level below inside a top-level cell.  (float64 positions: a statistic of the cases, not a reference for the kernels.)"""
    C, H = cfg.C, cfg.H
    assert C >= 2
    inner = float(2 ** (C - 2))
    idx = np.repeat(train.rays[:, 0], train.rays[:, 2])
    p = train.xyzs.astype(np.float64)
    q = p + train.deltas[:, :1].astype(np.float64) * r.rays_d[idx].astype(np.float64)
    top = lambda v: np.clip(np.floor((v / cfg.bound + 1.0) * (0.5 * H)), 0, H - 1).astype(np.int64)      # noqa: E731
    low = np.clip(np.floor((q / inner + 1.0) * (0.5 * H)), 0, H - 1).astype(np.int64)
    hit = (np.abs(p).max(-1) >= inner) & (np.abs(q).max(-1) < inner) & (top(p) == top(q)).all(-1)
    if C >= 3:
        hit &= np.abs(q).max(-1) >= inner / 2          # (else the point belongs to a still lower level)
    hit &= ~occ[C - 2, low[:, 0], low[:, 1], low[:, 2]]
    out = np.zeros(train.rays.shape[0], bool)
    out[idx[hit]] = True
    return out
