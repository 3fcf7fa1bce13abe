"""The closest-point rule in numpy (world.closest_numpy), MeshWorld.closest on a CPU world, and mesh.surface_error with its
statistics on the CPU: no GPU.  The HIP forms are compared with these bit for bit in test_closest_gpu.py."""
import math

import numpy as np
import pytest
import torch

import closest_cases as CC
from nerfsafetyvalidation_amd import mesh as ME
from nerfsafetyvalidation_amd import world as WO

f32 = np.float32

@pytest.mark.parametrize("name", CC.MESHES)
def test_closest_numpy_against_float64(name):
    """closest_numpy (float32, the rule) against the same formulas in float64 on the same points: distances on all finite points,
    the triangle only on the hand-built points whose triangle is not in doubt.  Measured max |d32 - d64| / S: cube 1.04e-7, henge
    1.59e-6, soup 3.90e-6 (the point 96 S away); relative to max(S, d) 1.06e-7 on all three.  Both are allowed four times that."""
    p, sec = CC.points(name)
    got, want = CC.reference(name), CC.reference64(name)
    S, _ = CC.scale(name)
    finite = np.isfinite(want["distance"])
    assert np.array_equal(finite, np.isfinite(got["distance"])) and finite.sum() == len(p) - (sec["broken"].stop - sec["broken"].start)
    err = np.abs(got["distance"][finite].astype(np.float64) - want["distance"][finite])
    print(name, "max |d32 - d64| / S", err.max() / S, "relative to max(S, d)", (err / np.maximum(S, want["distance"][finite])).max())
    assert err.max() / S <= CC.TOL_OVER_S
    assert (err <= CC.TOL_RELATIVE * np.maximum(S, want["distance"][finite])).all()
    perr = np.abs(got["point"][finite].astype(np.float64) - want["point"][finite]).max(1)
    hand = np.zeros(len(p), bool)
    for tag in CC.HAND:
        if tag in sec:
            hand[sec[tag]] = True
    assert np.array_equal(got["prim"][hand], want["prim"][hand])
    assert (perr[hand[finite]] <= CC.TOL_RELATIVE * 4 * S).all()          # (the same triangle: the same closest point)


@pytest.mark.parametrize("name", CC.MESHES)
def test_vertices_and_misses_are_exact(name):
    p, sec = CC.points(name)
    ref = CC.reference(name)
    vs = sec["vertex"]
    assert (ref["distance"][vs] == 0).all() and np.array_equal(CC.bits(ref["point"][vs]), CC.bits(p[vs])) and (ref["prim"][vs] >= 0).all()
    br = sec["broken"]
    assert np.isposinf(ref["distance"][br]).all() and (ref["prim"][br] == -1).all() and np.isnan(ref["point"][br]).all()
    rest = np.ones(len(p), bool)
    rest[br] = False
    assert np.isfinite(ref["distance"][rest]).all() and (ref["prim"][rest] >= 0).all() and np.isfinite(ref["point"][rest]).all()
    # the lowest index among equal distances
    v, faces, _ = CC.mesh(name)
    if name == "cube":
        c = sec["centre"].start
        assert ref["distance"][c] == f32(0.5) and ref["prim"][c] == 0
    if name == "soup":
        # a point of a repeated face belongs to the earlier copy -- or to a face of a still lower index that is as near
        dup = np.arange(sec["duplicate"].start, sec["duplicate"].stop)
        assert (ref["prim"][dup] <= np.tile(np.asarray(CC.RC.DUPLICATE_OF), 3)).all()
        assert (ref["prim"][dup] == np.tile(np.asarray(CC.RC.DUPLICATE_OF), 3)).sum() >= 25
        assert (ref["distance"][sec["zero_area"]] <= f32(1e-7)).all()


@pytest.mark.parametrize("name", CC.MESHES)
def test_max_distance_is_exact_at_the_boundary(name):
    p, sec = CC.points(name)
    v, faces, _ = CC.mesh(name)
    ref = CC.reference(name)
    _, ext = CC.scale(name)
    pick = np.concatenate([np.arange(sec["near"].start + 100, sec["near"].start + 110), np.arange(sec["outside"].start, sec["outside"].start + 10)])
    for i in pick:
        d = ref["distance"][i]
        assert d > 0
        at = WO.closest_numpy(p[i:i + 1], v, faces, max_distance=d)
        assert CC.bits(at["distance"])[0] == CC.bits(d) and at["prim"][0] == ref["prim"][i]
        below = WO.closest_numpy(p[i:i + 1], v, faces, max_distance=np.nextafter(d, f32(0)))
        assert np.isposinf(below["distance"][0]) and below["prim"][0] == -1 and np.isnan(below["point"][0]).all()
    for md in (0.05 * ext, 0.0):
        CC.same(WO.closest_numpy(p, v, faces, max_distance=md), CC.truncated(ref, md))
    with pytest.raises(ValueError):
        WO.closest_numpy(p[:2], v, faces, max_distance=float("nan"))


def test_cpu_world_closest_interface():
    v, faces, _ = CC.mesh("soup")
    p, _ = CC.points("soup")
    ref = CC.reference("soup")
    world = WO.MeshWorld(v, faces)
    got = world.closest(p)
    assert all(isinstance(a, np.ndarray) for a in got.values()) and set(got) == {"distance", "prim", "point"}
    CC.same(got, ref)
    got = world.closest(torch.from_numpy(p[:60].copy()).reshape(4, 15, 3), coherent=True)
    assert all(isinstance(a, torch.Tensor) for a in got.values())
    assert got["distance"].shape == (4, 15) and got["prim"].shape == (4, 15) and got["point"].shape == (4, 15, 3)
    CC.same(got, {k: a[:60] for k, a in ref.items()})
    empty = world.closest(np.zeros((0, 3), f32))
    assert empty["distance"].shape == (0,) and empty["prim"].shape == (0,) and empty["point"].shape == (0, 3)
    for bad in (np.zeros((4, 2), f32), np.zeros(3, f32)[0]):
        with pytest.raises(ValueError):
            world.closest(bad)
    with pytest.raises(ValueError):
        world.closest(p[:4], max_distance=float("nan"))


# ------------------------------------------------------------------------------------------------------------- surface error
def test_surface_error_two_cubes():
    v1, f1, world = CC.two_cubes()
    CC.check_two_cubes(ME.surface_error(v1, f1, world, thresholds=CC.THRESHOLDS, max_distance=1.0))


def test_surface_error_of_a_mesh_against_itself_and_truncation():
    v, f = CC.lattice_cube(1.0)
    err = ME.surface_error(v, f, WO.MeshWorld(v, f), thresholds=(0.0, 0.1), max_distance=0.5)
    for side in (err.accuracy, err.completeness):
        assert side.misses == 0 and side.mean == 0.0 and side.rms == 0.0 and side.max == 0.0 and side.within[0.0] == side.n
        assert (side.distances == 0).all()
    assert err.f_score == {0.0: 1.0, 0.1: 1.0} and err.hausdorff == 0.0 and err.margin(1.0) == 0.0
    # truncated below delta every point misses: margins are +inf, the Hausdorff distance is max_distance
    v1, f1, world = CC.two_cubes()
    err = ME.surface_error(v1, f1, world, thresholds=(0.01,), max_distance=CC.DELTA / 2)
    assert err.accuracy.misses == err.accuracy.n and err.completeness.misses == err.completeness.n
    assert err.hausdorff == CC.DELTA / 2 and err.margin(0.5) == math.inf and err.f_score[0.01] == 0.0 and math.isnan(err.accuracy.mean)
    # truncated between delta and delta sqrt 3 the corners miss: a quantile among the misses is +inf
    err = ME.surface_error(v1, f1, world, thresholds=(0.01,), max_distance=CC.DELTA * 1.2)
    assert err.accuracy.misses == 0 and 0 < err.completeness.misses < err.completeness.n
    assert err.margin(1.0) == math.inf and err.margin(0.2) < CC.DELTA * 1.2 and err.hausdorff == CC.DELTA * 1.2
    # the world frame: the same numbers
    a = ME.surface_error(v1, f1, world, thresholds=CC.THRESHOLDS, max_distance=1.0)
    b = ME.surface_error(ME.mesh_to_world(v1), f1, world, thresholds=CC.THRESHOLDS, max_distance=1.0, frame="world")
    assert np.array_equal(a.completeness.distances.numpy(), b.completeness.distances.numpy()) and a.hausdorff == b.hausdorff
    with pytest.raises(ValueError):
        ME.surface_error(v1, f1, world, thresholds=(float("nan"),), max_distance=1.0)
    with pytest.raises(ValueError):
        ME.surface_error(v1, f1, world, thresholds=tuple(range(9)), max_distance=1.0)
    with pytest.raises(ValueError):
        ME.surface_error(v1, f1, world, thresholds=(0.1,), max_distance=float("nan"))


@pytest.mark.parametrize("key", (0, 1, 63, 64, 65, 4097, "inf"))
def test_distance_stats_numpy_against_exact_sums(key):
    d = CC.stats_arrays()[key]
    CC.check_stats(ME.distance_stats(d, CC.STATS_THRESHOLDS), CC.exact_stats(d, CC.STATS_THRESHOLDS))
    CC.check_stats(ME.distance_stats(torch.from_numpy(d), ()), CC.exact_stats(d, ()))


def test_sample_surface_and_samples_path():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [3, 0, 2], [0, 2, 2]], f32)         # areas 0.5 and 3
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    a, b = ME.sample_surface(v, f, 4000, seed=3), ME.sample_surface(v, f, 4000, seed=3)
    assert isinstance(a, np.ndarray) and a.dtype == f32 and a.shape == (4000, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, ME.sample_surface(v, f, 4000, seed=4))
    assert torch.equal(ME.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 4000, seed=3), torch.from_numpy(a))
    assert (WO.closest_numpy(a, v, f)["distance"] <= 4e-7 * 3).all()
    share = (a[:, 2] == 2).mean()                                         # 3 / 3.5 of the area; four standard deviations
    assert abs(share - 3 / 3.5) <= 4 * math.sqrt((3 / 3.5) * (0.5 / 3.5) / 4000)
    assert ME.sample_surface(v, f, 0).shape == (0, 3)
    v1, f1, world = CC.two_cubes()
    err = ME.surface_error(v1, f1, world, thresholds=(0.1,), max_distance=1.0, samples=500, seed=1)
    assert err.accuracy.n == err.completeness.n == 500 and err.accuracy.misses == 0
    tol = CC.TOL_RELATIVE * 1.0625
    assert abs(err.accuracy.max - CC.DELTA) <= tol and CC.DELTA - tol <= err.completeness.mean <= err.hausdorff <= CC.DELTA * math.sqrt(3) + tol


def test_error_colors_and_colored_ply(tmp_path):
    d = np.array([0.0, 0.05, 0.1, 0.3, np.inf, np.nan], f32)
    rgb = ME.error_colors(d, 0.1)
    assert rgb.dtype == np.uint8 and rgb.shape == (6, 3)
    assert rgb[:4].tolist() == [list(ME.ERROR_RAMP[0]), list(ME.ERROR_RAMP[1]), list(ME.ERROR_RAMP[2]), list(ME.ERROR_RAMP[2])]
    assert rgb[4:].tolist() == [list(ME.MISS_COLOR)] * 2
    assert np.array_equal(ME.error_colors(torch.from_numpy(d), 0.1), rgb)
    v, f = CC.lattice_cube(1.0)
    world = CC.two_cubes()[2]
    err = ME.surface_error(v, f, world, thresholds=(0.1,), max_distance=1.0)
    colors = ME.error_colors(err.accuracy.distances, 2 * CC.DELTA)
    assert (colors == np.asarray(ME.ERROR_RAMP[1], np.uint8)).all()      # delta everywhere: the middle of the ramp
    path = str(tmp_path / "error.ply")
    ME.write_ply(path, v, f, colors=colors)
    v2, f2, c2 = ME.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(c2, colors)
    with pytest.raises(ValueError):
        ME.error_colors(d, 0.0)
