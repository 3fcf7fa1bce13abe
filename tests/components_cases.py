"""The shared cases of the connected-component tests (test_components_cpu.py, test_components_gpu.py): shapes, patterns, the scipy
yardstick and the synthetic floater scene.  Patterns are functions of the shape alone (fixed seeds)."""
import functools

import numpy as np

from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd import collision as CO

CONNECTIVITIES = (6, 14, 18, 26)
TILE = _lib.NGP_COMPONENTS_TILE          # the cells per axis of the tile one workgroup of ngp_label_components labels in LDS

BASE_SHAPES = [(1, 1, 1), (1, 1, 130), (130, 1, 1), (1, 130, 1), (3, 5, 7), (17, 9, 65), (33, 34, 66), (96, 92, 24)]


def _seam_shapes():
    """per axis: T - 1, T, T + 1 and 2 T + 1 cells along it (T the tile's), a few cells more than a tile along the other two"""
    rest = (TILE[0] + 1, TILE[1] + 2, TILE[2] + 1)
    out = []
    for axis in range(3):
        for size in (TILE[axis] - 1, TILE[axis], TILE[axis] + 1, 2 * TILE[axis] + 1):
            shape = list(rest)
            shape[axis] = size
            out.append(tuple(shape))
    return out


SHAPES = BASE_SHAPES + [s for s in _seam_shapes() if s not in BASE_SHAPES]
CHAIN_DIRECTIONS = ((1, 1, 0), (1, -1, 0), (1, 1, 1), (1, -1, 1))


def _coords(shape):
    return np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")


def empty(shape):
    return np.zeros(shape, np.uint8)


def full(shape):
    return np.ones(shape, np.uint8)


def corners(shape):
    occ = np.zeros(shape, np.uint8)
    occ[np.ix_(*[[0, n - 1] for n in shape])] = 1
    return occ


def checkerboard(shape):
    x, y, z = _coords(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def chain(shape, direction):
    """cells start + k * direction while inside, from the corner the direction leaves"""
    occ = np.zeros(shape, np.uint8)
    p = [0 if d >= 0 else n - 1 for d, n in zip(direction, shape)]
    while all(0 <= c < n for c, n in zip(p, shape)):
        occ[tuple(p)] = 1
        p = [c + d for c, d in zip(p, direction)]
    return occ


def snake(shape):
    """ONE one-cell-wide path: the rows (along z) y = 0, 2, 4, .. of the planes x = 0, 2, 4, .., joined at alternate ends by one cell
    in the row between, the planes joined by one cell in the plane between, where the path leaves the plane (the last row's far end
    for the planes walked upwards, (0, 0) for the ones walked back).  About N / 4 cells, one component under every connectivity."""
    X, Y, Z = shape
    occ = np.zeros(shape, np.uint8)
    occ[0::2, 0::2, :] = 1
    last = (Y - 1) // 2                                  # index of the last row, y = 2 * last
    for j in range(last):
        occ[0::2, 2 * j + 1, Z - 1 if j % 2 == 0 else 0] = 1
    for i in range((X - 1) // 2):
        if i % 2 == 0:
            occ[2 * i + 1, 2 * last, Z - 1 if last % 2 == 0 else 0] = 1
        else:
            occ[2 * i + 1, 0, 0] = 1
    return occ


def u_shape(shape):
    """two arms along x, at (y, z) = (0, 0) and (Y - 1, Z - 1), that meet only in the last layer x = X - 1"""
    X, Y, Z = shape
    occ = np.zeros(shape, np.uint8)
    occ[:, 0, 0] = 1
    occ[:, Y - 1, Z - 1] = 1
    occ[X - 1, :, 0] = 1
    occ[X - 1, Y - 1, :] = 1
    return occ


def combs(shape):
    """two interleaved combs, the same in every layer x, never within one cell of each other (for Y >= 5): spines y = 0 and Y - 1,
    teeth at z = 0 mod 4 (y <= Y - 3) and z = 2 mod 4 (y >= 2)"""
    X, Y, Z = shape
    occ = np.zeros(shape, np.uint8)
    occ[:, 0, :] = 1
    occ[:, Y - 1, :] = 1
    occ[:, :max(Y - 2, 0), 0::4] = 1
    occ[:, 2:, 2::4] = 1
    return occ


def bernoulli(shape, fill, seed):
    return (np.random.default_rng(seed).random(shape) < fill).astype(np.uint8)


def as_255(shape):
    return bernoulli(shape, 0.3, 7) * np.uint8(255)


def as_bool(shape):
    return bernoulli(shape, 0.3, 8).astype(bool)


def strided(shape):
    """a non-contiguous view: every second cell along z of a wider map, with x and y swapped in memory"""
    wide = bernoulli((shape[1], shape[0], 2 * shape[2]), 0.3, 9)
    view = wide.transpose(1, 0, 2)[:, :, ::2]
    assert view.shape == tuple(shape) and (view.size < 4 or not view.flags["C_CONTIGUOUS"])
    return view


PATTERNS = {"empty": empty, "full": full, "corners": corners, "checkerboard": checkerboard, "snake": snake, "u": u_shape, "combs": combs,
            "fill10": functools.partial(bernoulli, fill=0.1, seed=1), "fill30": functools.partial(bernoulli, fill=0.3, seed=2),
            "fill60": functools.partial(bernoulli, fill=0.6, seed=3), "v255": as_255, "bool": as_bool, "strided": strided}
for _d in CHAIN_DIRECTIONS:
    PATTERNS["chain" + "".join("m" if c < 0 else str(c) for c in _d)] = functools.partial(chain, direction=_d)

# the components of a chain of L cells along a direction, per connectivity: 1 when the direction is one of its offsets, else L
CHAIN_IS_ONE = {(1, 1, 0): {6: False, 14: True, 18: True, 26: True}, (1, -1, 0): {6: False, 14: False, 18: True, 26: True},
                (1, 1, 1): {6: False, 14: True, 18: False, 26: True}, (1, -1, 1): {6: False, 14: False, 18: False, 26: True}}

CASES = [(shape, name) for shape in SHAPES for name in PATTERNS]


def case_id(case):
    return "x".join(str(n) for n in case[0]) + "-" + case[1]


@functools.lru_cache(maxsize=None)
def pattern(shape, name):
    occ = PATTERNS[name](shape)
    occ.setflags(write=False)
    return occ


def structure(connectivity):
    """scipy.ndimage.label's structuring element of a connectivity"""
    from scipy import ndimage
    if connectivity == 14:
        s = np.zeros((3, 3, 3), bool)
        s[1, 1, 1] = True
        for dx, dy, dz in CO.KUHN_OFFSETS:
            s[1 + dx, 1 + dy, 1 + dz] = s[1 - dx, 1 - dy, 1 - dz] = True
        return s
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


@functools.lru_cache(maxsize=None)
def scipy_labels(shape, name, connectivity):
    """the yardstick: (labels, n) of scipy.ndimage.label, computed once per case"""
    from scipy import ndimage
    labels, n = ndimage.label(np.ascontiguousarray(pattern(shape, name)), structure(connectivity))
    labels.setflags(write=False)
    return labels, int(n)


@functools.lru_cache(maxsize=None)
def numpy_labels(shape, name, connectivity):
    """the package's numpy path, computed once per case (what the HIP path is held against)"""
    labels, n = CO.label_components_numpy(pattern(shape, name), connectivity)
    labels.setflags(write=False)
    return labels, n


# ------------------------------------------------------------------ the synthetic floater scene
@functools.lru_cache(maxsize=None)
def floater_scene():
    """truth: the henge's map over reference_box() (6 components under every connectivity, all on z-layer 0, layers 12..23 empty).
    pred: truth minus one whole component, plus blobs in the empty layers, more than one cell apart from each other and the map:
    a single cell, a 2 x 2 x 2 block, two cells that touch by a corner only (one component under 14 and 26, two under 6 and 18;
    the corner offset is (1, 1, 1), a Kuhn edge) and a 10 x 10 x 3 block of 300 cells.
    -> dict(truth, pred, removed (bool map of the component taken out), blobs (bool map), blob_cells {connectivity: sorted sizes})"""
    truth = CO.occupancy_from_fn(CO.henge_fn, CO.reference_box()).numpy()
    assert truth.shape == (96, 92, 24) and not truth[:, :, 12:].any()
    labels, n = scipy_labels_of(truth, 26)
    removed = labels == 3
    blobs = np.zeros_like(truth)
    blobs[10, 10, 15] = True
    blobs[20:22, 10:12, 15:17] = True
    blobs[30, 10, 15] = blobs[31, 11, 16] = True
    blobs[40:50, 20:30, 14:17] = True
    pred = (truth & ~removed) | blobs
    sizes = {c: sorted([1, 8, 300] + ([2] if c in (14, 26) else [1, 1])) for c in CONNECTIVITIES}
    for a in (truth, pred, removed, blobs):
        a.setflags(write=False)
    return {"truth": truth, "pred": pred, "removed": removed, "blobs": blobs, "blob_cells": sizes, "truth_components": n}


def scipy_labels_of(occ, connectivity):
    from scipy import ndimage
    labels, n = ndimage.label(occ, structure(connectivity))
    return labels, int(n)


def check_floater_api(put, get):
    """remove_floaters / floater_report on the scene, for maps handed over by put(numpy bool map) and read back by get(result):
    the assertions the CPU and the GPU test files share"""
    sc = floater_scene()
    truth, pred = put(sc["truth"]), put(sc["pred"])
    same_kind = lambda a, b: type(a) is type(b) and getattr(a, "device", None) == getattr(b, "device", None)      # noqa: E731
    for c in CONNECTIVITIES:
        rep = CO.floater_report(pred, truth, c)
        assert rep["truth_components"] == 6 and rep["pred_components"] == 5 + len(sc["blob_cells"][c])
        assert sorted(rep["phantom"]["cells"]) == sc["blob_cells"][c] and rep["phantom"]["count"] == len(sc["blob_cells"][c])
        boxes = np.zeros_like(sc["blobs"])
        for lo, hi in zip(rep["phantom"]["lo"], rep["phantom"]["hi"]):
            boxes[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
        assert np.array_equal(boxes & sc["pred"], sc["blobs"])                   # the phantoms are exactly the injected cells
        assert rep["missed"]["count"] == 1 and rep["missed"]["cells"] == [int(sc["removed"].sum())]
        lo, hi = rep["missed"]["lo"][0], rep["missed"]["hi"][0]
        where = np.argwhere(sc["removed"])
        assert lo == tuple(where.min(0)) and hi == tuple(where.max(0))
        assert rep["agreement"] == CO.map_agreement(sc["pred"].copy(), sc["truth"].copy())
        assert rep["agreement"]["fp"] == int(sc["blobs"].sum()) and rep["agreement"]["fn"] == int(sc["removed"].sum())

        cleaned, report = CO.remove_floaters(pred, connectivity=c, min_cells=200)
        assert same_kind(cleaned, pred) and cleaned.dtype == pred.dtype
        big = np.zeros_like(sc["blobs"])
        big[40:50, 20:30, 14:17] = True
        assert np.array_equal(get(cleaned), (sc["truth"] & ~sc["removed"]) | big)                 # the 300-cell blob stays
        assert report["dropped"]["count"] == len(sc["blob_cells"][c]) - 1 and report["kept"]["count"] == 6 and report["n"] == rep["pred_components"]
        assert sorted(report["dropped"]["cells"]) == sc["blob_cells"][c][:-1]

        cleaned, report = CO.remove_floaters(pred, connectivity=c, grounded=(2, "lo"))
        assert same_kind(cleaned, pred)
        assert np.array_equal(get(cleaned), sc["truth"] & ~sc["removed"])                          # every blob and nothing else
        assert sorted(report["dropped"]["cells"]) == sc["blob_cells"][c] and report["kept"]["count"] == 5
        assert CO.map_agreement(cleaned, truth)["precision"] == 1.0
        assert CO.remove_floaters(pred, connectivity=c, grounded=(2, "hi"))[1]["kept"]["count"] == 0

        cleaned, report = CO.remove_floaters(pred, connectivity=c, keep_largest=2)
        want = sorted(report["kept"]["cells"] + report["dropped"]["cells"])[-2:]
        assert sorted(report["kept"]["cells"]) == want and int(get(cleaned).sum()) == sum(want)

        cleaned, report = CO.remove_floaters(pred, connectivity=c)
        assert cleaned is pred and report["dropped"]["count"] == 0 and report["kept"]["count"] == rep["pred_components"]
    return sc


def check_floater_errors(put):
    import pytest
    occ = put(floater_scene()["pred"])
    for bad in (dict(connectivity=7), dict(min_cells=-1), dict(keep_largest=0), dict(grounded=(3, "lo")), dict(grounded=(2, "up")),
                dict(grounded="lo")):
        with pytest.raises(ValueError):
            CO.remove_floaters(occ, **bad)
    with pytest.raises(ValueError):
        CO.remove_floaters(occ[0])
    with pytest.raises(ValueError):
        CO.label_components(occ, 7)


def two_blobs(small=True):
    """a 24^3 field with a ball of radius 6 inside (u > 0) and, with small=True, a second one of radius 1.6 far from it"""
    x, y, z = np.meshgrid(*[np.arange(24, dtype=np.float32)] * 3, indexing="ij")
    u = 6.0 - np.sqrt((x - 9.0) ** 2 + (y - 10.0) ** 2 + (z - 11.0) ** 2)
    if small:
        u = np.maximum(u, 1.6 - np.sqrt((x - 19.5) ** 2 + (y - 19.0) ** 2 + (z - 19.0) ** 2))
    return u.astype(np.float32)
