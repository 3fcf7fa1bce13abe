"""Fields and mesh checks shared by tests/test_mesh_cpu.py and tests/test_mesh_gpu.py (index coordinates, float32 lattices)."""
import numpy as np

ALL_CONFIG_SHAPE, ALL_CONFIG_SEED = (17, 17, 17), 0      # every one of the 256 corner configurations occurs (asserted on the CPU)


def lattice(shape):
    """[X,Y,Z,3] float64 index coordinates"""
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)


def sphere(shape=(20, 20, 20), centre=(9.3, 9.3, 9.3), radius=6.0):
    return (radius - np.linalg.norm(lattice(shape) - np.asarray(centre), axis=-1)).astype(np.float32)


def two_spheres(shape=(20, 20, 20)):
    g = lattice(shape)
    a = 3.2 - np.linalg.norm(g - 5.3, axis=-1)
    b = 3.4 - np.linalg.norm(g - np.array([14.1, 13.7, 14.4]), axis=-1)
    return np.maximum(a, b).astype(np.float32)


def torus(shape=(20, 20, 20), centre=(9.4, 9.6, 9.3), R=6.0, r=2.2):
    d = lattice(shape) - np.asarray(centre)
    return (r - np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - R) ** 2 + d[..., 2] ** 2)).astype(np.float32)


def random_field(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def smooth_field(shape):
    """a gyroid: a smooth surface through the whole box"""
    g = lattice(shape) * 0.23
    x, y, z = g[..., 0], g[..., 1], g[..., 2]
    return (np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x)).astype(np.float32)


def corner_configurations(u, threshold):
    """the 8-bit corner configuration of every cell (bit dx | dy << 1 | dz << 2)"""
    inside = u > np.float32(threshold)
    X, Y, Z = u.shape
    return sum(inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << (dx | (dy << 1) | (dz << 2))
               for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))


def edge_use(n_vertices, faces):
    """-> (undirected edges [E,2], times each is used [E], True when no directed edge occurs twice)"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = e[:, 0] * n_vertices + e[:, 1]
    key = np.minimum(e[:, 0], e[:, 1]) * n_vertices + np.maximum(e[:, 0], e[:, 1])
    uniq, count = np.unique(key, return_counts=True)
    return np.stack([uniq // n_vertices, uniq % n_vertices], -1), count, len(np.unique(directed)) == len(directed)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


def assert_closed(vertices, faces, euler):
    """every undirected edge in exactly two faces, once in each direction; V - E + F; outward normals"""
    edges, count, consistent = edge_use(len(vertices), faces)
    assert len(faces) > 0 and (count == 2).all() and consistent
    assert np.array_equal(np.unique(faces), np.arange(len(vertices))), "every vertex is used"
    assert len(vertices) - len(edges) + len(faces) == euler
    assert signed_volume(vertices, faces) > 0


def assert_open_only_at_the_boundary(shape, owners, types, faces, edge_offsets):
    """no edge in more than two faces, none traversed twice in one direction, and every edge in ONE face joins two vertices whose
    lattice edges lie in one common boundary plane of the lattice"""
    edges, count, consistent = edge_use(len(owners), faces)
    assert count.max() <= 2 and consistent
    off = np.asarray(edge_offsets, dtype=np.int64)[types]                 # [V,3]
    n = np.asarray(shape, dtype=np.int64)
    low = (off == 0) & (owners == 0)                                      # [V,3]: the lattice edge lies in the plane index_d = 0
    high = (off == 0) & (owners == n - 1)
    once = edges[count == 1]
    a, b = once[:, 0], once[:, 1]
    common = (low[a] & low[b]) | (high[a] & high[b])
    assert common.any(axis=1).all()
    return int((count == 1).sum())
