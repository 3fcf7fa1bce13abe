"""The ray caster's hit rule, binning and host pieces without a GPU: world.py's numpy path (the package's CPU implementation and the
reference of the GPU tests), mesh.read_ply / write_ply, scene.henge_mesh, run_validation's `simulator`, scripts/make_mesh_dataset.py."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raycast_cases as RC
from nerfsafetyvalidation_amd import mesh as ME
from nerfsafetyvalidation_amd import scene as SC
from nerfsafetyvalidation_amd import world as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest relative |t32 - t64| of the numpy path on the cube's rays (all of raycast_cases.rays("cube")) against a float64
# evaluation of the same formulas on the same (ray, triangle): measured 1.64e-7 (test_cube_matches_the_slab_intersection prints it).
# The bound is 4 x that: the factor covers other ray sets of the same geometry.
CUBE_T_REL_MEASURED = 1.64e-7
CUBE_T_REL_BOUND = 4 * CUBE_T_REL_MEASURED


def slab(o, d):
    """the unit cube against rays in float64 -> (t, face, margin): the distance and face (2 * axis + side) of the first boundary
    crossing at t > 0 (entry from outside, exit from inside), NaN / -1 on a miss; margin: how far the case is from any other (from a
    cube edge, from grazing, from t = 0), in units of the cube"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    N = len(o)
    with np.errstate(all="ignore"):
        t0, t1 = (0.0 - o) / d, (1.0 - o) / d
    par = d == 0
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    inside_slab = (o > 0) & (o < 1)
    near, far = np.where(par, np.where(inside_slab, -np.inf, np.inf), near), np.where(par, np.where(inside_slab, np.inf, -np.inf), far)
    t_in, t_out = near.max(1), far.min(1)
    ax_in, ax_out = near.argmax(1), far.argmin(1)
    speed = np.linalg.norm(d, axis=1)
    hit = (t_in <= t_out) & (t_out > 0)
    entering = t_in > 0
    t = np.where(hit, np.where(entering, t_in, t_out), np.nan)
    ax = np.where(entering, ax_in, ax_out)
    side = np.where(entering, d[np.arange(N), ax] < 0, d[np.arange(N), ax] > 0).astype(np.int64)      # entering through x=1 when moving in -x
    face = np.where(hit, 2 * ax + side, -1)
    # margins: the width of the interval and the distance of its end from 0; for a hit also the gap to the second candidate face
    # and the distance of the entry from 0
    s_near, s_far = np.sort(near, 1), np.sort(far, 1)
    with np.errstate(all="ignore"):
        decided = np.minimum(np.abs(t_out - t_in), np.abs(t_out))                         # hit or miss
        gap = np.where(entering, s_near[:, 2] - s_near[:, 1], s_far[:, 1] - s_far[:, 0])  # which face
        margin = np.where(hit, np.minimum(decided, np.minimum(gap, np.abs(t_in))), decided) * speed
    on_plane = (par & ((o == 0) | (o == 1))).any(1)
    margin = np.where(on_plane | ~np.isfinite(margin), 0.0, margin)
    return t, face, margin


def test_cube_matches_the_slab_intersection():
    o, d, sections, _ = RC.rays("cube")
    ref = RC.reference("cube")
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    t, face, margin = slab(o[valid], d[valid])
    prim, t32 = ref["prim"][valid], ref["t"][valid].astype(np.float64)
    clear = margin > 1e-4
    assert clear.sum() > 0.8 * valid.sum()          # (half of the grazing frame starts on a face's plane and leaves: undecided)
    want_hit = face >= 0
    assert np.array_equal(prim[clear] >= 0, want_hit[clear])                              # misses are misses
    sel = clear & want_hit
    assert sel.sum() > 3000 and np.array_equal(prim[sel] // 2, face[sel])                  # the face is correct
    # float32 against float64 of the same formulas, and against the analytic distance
    hit = np.flatnonzero(ref["prim"] >= 0)
    t64 = np.concatenate([np.diagonal(WO.hit_terms(o[hit[i:i + 512]], d[hit[i:i + 512]], RC.tri_data("cube")[ref["prim"][hit[i:i + 512]]],
                                                   np.float64)[3]) for i in range(0, len(hit), 512)])
    measured = float((np.abs(ref["t"][hit] - t64) / np.abs(t64)).max())
    print(f"largest relative |t32 - t64| on the cube: {measured:.3e} (bound {CUBE_T_REL_BOUND:.3e})")
    assert measured <= CUBE_T_REL_BOUND
    assert (np.abs(t32[sel] - t[sel]) <= CUBE_T_REL_BOUND * np.abs(t[sel])).all()
    assert np.isinf(ref["t"][ref["prim"] < 0]).all() and (ref["u"][ref["prim"] < 0] == 0).all()


def accepting(o, d, tri_data):
    """an independent statement of acceptance for a few rays: (ok [R,F], t [R,F])"""
    det, u, v, t = WO.hit_terms(o, d, tri_data)
    with np.errstate(all="ignore"):
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t


def test_ties_go_to_the_lowest_index():
    # duplicates: the copy (at the higher index) is never reported, the original is hit by some ray
    ref = RC.reference("soup")
    assert not np.isin(ref["prim"], list(RC.DUPLICATES)).any()
    assert np.isin(ref["prim"], list(RC.DUPLICATE_OF)).any()
    o, d, sections, tags = RC.rays("soup")
    rows = np.flatnonzero(np.isin(ref["prim"], list(RC.DUPLICATE_OF)))[:64]
    ok, t = accepting(o[rows], d[rows], RC.tri_data("soup"))
    for i, r in enumerate(rows):
        twin = RC.DUPLICATES[RC.DUPLICATE_OF.index(int(ref["prim"][r]))]
        assert ok[i, twin] and t[i, twin] == ref["t"][r]                                  # an exact tie, resolved downwards
    # the cube: axis-parallel rays through the face diagonals (shared edges) and the corners (shared vertices) hit, and every ray
    # reports the lowest index among the closest accepting triangles
    o, d, sections, tags = RC.rays("cube")
    ref = RC.reference("cube")
    hand = sections["hand"]
    axis = hand.start + np.flatnonzero(np.array(tags) == "axis")
    assert (ref["prim"][axis] >= 0).all()
    ok, t = accepting(o[hand], d[hand], RC.tri_data("cube"))
    tm = np.where(ok, t, np.inf)
    closest = ok & (tm == tm.min(1, keepdims=True))
    want = np.where(ok.any(1), closest.argmax(1), -1)
    assert np.array_equal(ref["prim"][hand], want)
    on_edge = closest[np.array(tags) == "axis"].sum(1)
    assert (on_edge >= 2).sum() >= 24                    # the diagonal and corner rays really are accepted by two triangles or more
    shared = hand.start + np.flatnonzero(np.array(tags) == "shared")
    assert (ref["prim"][shared] >= 0).all()


def test_degenerate_triangles_and_rays_miss():
    for name in RC.MESHES:
        o, d, sections, tags = RC.rays(name)
        ref = RC.reference(name)
        hand = sections["hand"]
        bad = hand.start + np.flatnonzero(np.isin(np.array(tags), ["nan", "zero"]))
        assert len(bad) == 10
        assert (ref["prim"][bad] == -1).all() and np.isposinf(ref["t"][bad]).all() and (ref["u"][bad] == 0).all() and (ref["v"][bad] == 0).all()
        away = hand.start + np.flatnonzero(np.array(tags) == "away")
        assert (ref["prim"][away] == -1).all()
    assert not np.isin(RC.reference("soup")["prim"], list(RC.ZERO_AREA)).any()
    # ... not even by rays aimed at them
    v, f, _ = RC.mesh("soup")
    target = v[f[list(RC.ZERO_AREA)]].mean(1)
    org = np.tile(np.array([[0.5, 0.5, -2.0]], np.float32), (len(target), 1))
    out = WO.cast_numpy(org, target - org, RC.tri_data("soup"))
    assert not np.isin(out["prim"], list(RC.ZERO_AREA)).any()
    # a window on t
    o, d, sections, _ = RC.rays("cube")
    win = WO.cast_numpy(o[sections["outside"]], d[sections["outside"]], RC.tri_data("cube"), t_min=0.0, t_max=2.2)
    ref = RC.reference("cube")
    near = ref["t"][sections["outside"]] < np.float32(2.2)
    assert np.array_equal(win["prim"] >= 0, near) and near.any() and not near.all()


@pytest.mark.parametrize("name", RC.MESHES)
@pytest.mark.parametrize("resolution", [None, (16, 7, 3), (1, 1, 1)])
def test_binning_covers_every_overlapped_cell(name, resolution):
    """a restatement in float64: every cell a triangle's exact bounding box touches holds the triangle; every list is ascending"""
    v, f, _ = RC.mesh(name)
    g = WO.grid_params(v.min(0), v.max(0), len(f), resolution)
    cell_start, pair_tri = WO.bin_triangles_numpy(RC.tri_data(name), g)
    n = g["n"]
    assert cell_start.shape == (int(np.prod(n)) + 1,) and cell_start[0] == 0 and cell_start[-1] == len(pair_tri)
    assert (np.diff(cell_start) >= 0).all()
    inner = np.ones(len(pair_tri), bool)
    inner[cell_start[1:-1][cell_start[1:-1] < len(pair_tri)]] = False
    inner[0] = False
    assert (np.diff(pair_tri.astype(np.int64))[inner[1:]] > 0).all()                       # ascending within every cell
    member = set(zip(np.repeat(np.arange(len(cell_start) - 1), np.diff(cell_start)).tolist(), pair_tri.tolist()))
    tri = v[f].astype(np.float64)                                                          # [F, 3, 3]
    lo, hi = tri.min(1), tri.max(1)
    glo, cell = g["lo"].astype(np.float64), g["cell"].astype(np.float64)
    for t in range(len(f)):
        # cells c with [glo + c cell, glo + (c + 1) cell] meeting [lo, hi] (closed intervals)
        ranges = []
        for a in range(3):
            planes = glo[a] + np.arange(n[a] + 1) * cell[a]
            ranges.append(np.flatnonzero((planes[:-1] <= hi[t, a]) & (planes[1:] >= lo[t, a])))
            assert len(ranges[-1]) >= 1
        for x in ranges[0]:
            for y in ranges[1]:
                for z in ranges[2]:
                    assert (int((x * n[1] + y) * n[2] + z), t) in member
    # the automatic grid is a grid: about four cells per triangle at most, never more than 256 per axis
    if resolution is None:
        assert (n >= 1).all() and (n <= 256).all() and np.prod(n) <= 8 * max(len(f), 1) + 8


def test_grid_rule_and_invalid_meshes():
    v, f, c = RC.mesh("cube")
    w = WO.MeshWorld(v, f)
    assert w.dims == tuple(int(x) for x in w.grid["n"]) and w.pairs == len(w.pair_tri) and w.mean_pairs_per_cell == w.pairs / np.prod(w.dims)
    assert (w.grid["grow"] < w.grid["cell"] / 8).all() and (w.grid["lo"] < v.min(0)).all()
    assert WO.MeshWorld(v, f, resolution=5).dims == (5, 5, 5)
    with pytest.raises(ValueError):
        WO.MeshWorld(v, f, resolution=(257, 4, 4))
    with pytest.raises(ValueError):
        WO.MeshWorld(v, f, resolution=(0, 4, 4))
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(ValueError):
        WO.MeshWorld(v, bad)
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        WO.MeshWorld(v, bad)
    with pytest.raises(ValueError):
        WO.MeshWorld(v, f[:0])
    with pytest.raises(ValueError):
        WO.MeshWorld(v[:0], f)
    nan = v.copy()
    nan[2, 0] = np.nan
    with pytest.raises(ValueError):
        WO.MeshWorld(nan, f)
    # the world frame: the same mesh given in the planner's frame
    from nerfsafetyvalidation_amd.mesh import mesh_to_world
    w2 = WO.MeshWorld(mesh_to_world(v).astype(np.float32), f, frame="world")
    assert np.allclose(w2.vertices.numpy(), v, atol=1e-6)
    # an empty batch of rays, and shapes
    out = w.cast(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert out["t"].shape == (0,) and out["prim"].dtype == np.int32
    o, d, sections, _ = RC.rays("cube")
    out = w.cast(torch.from_numpy(o[:6].copy()).reshape(2, 3, 3), torch.from_numpy(d[:6].copy()).reshape(2, 3, 3))
    assert isinstance(out["t"], torch.Tensor) and out["t"].shape == (2, 3)
    assert np.array_equal(out["prim"].numpy().reshape(-1), RC.reference("cube")["prim"][:6])


def test_cpu_render_is_pixel_aligned_and_shaded():
    v, f, c = RC.mesh("soup")
    w = WO.MeshWorld(v, f, c)
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    pose = torch.from_numpy(SC.look_at_poses(np.array([[0.3, 0.2, -1.6]]))[0]).float()
    pose[:3, 3] += torch.tensor([0.5, 0.5, 0.5])
    K = SC.intrinsics(12, 10)
    out = w.render(pose, K, 12, 10, bg_color=[0.25, 0.5, 1.0])
    rays = get_rays(pose[None], K, 12, 10)
    hit = w.cast(rays["rays_o"][0], rays["rays_d"][0])
    assert np.array_equal(out["prim"].numpy().reshape(-1), hit["prim"].numpy())
    miss = out["prim"].numpy() < 0
    assert miss.any() and not miss.all()
    img = out["image"].numpy()
    assert img.dtype == np.float32 and (img[miss] == np.array([0.25, 0.5, 1.0], np.float32)).all()
    assert (img >= 0).all() and (img <= 1).all() and np.array_equal(out["image_u8"].numpy(), (img * np.float32(255)).astype(np.uint8))
    assert np.isposinf(out["depth"].numpy()[miss]).all()
    # the colour is the blend of the corner colours times a factor in [ambient, 1]
    k = np.flatnonzero(~miss.reshape(-1))[0]
    p, u, vv = int(hit["prim"][k]), float(hit["u"][k]), float(hit["v"][k])
    blend = (1 - u - vv) * c[f[p, 0]] + u * c[f[p, 1]] + vv * c[f[p, 2]]
    ratio = img.reshape(-1, 3)[k] / blend
    assert np.allclose(ratio, ratio[0], rtol=1e-4) and 0.3 - 1e-5 <= ratio[0] <= 1 + 1e-5
    grey = WO.MeshWorld(v, f).render(pose, K, 12, 10)["image"].numpy()
    assert (grey[miss] == 1).all() and (grey[~miss] <= 0.5).all() and (grey[~miss] >= 0.15 - 1e-6).all()


def test_ply_round_trip(tmp_path):
    v, f, c = RC.mesh("soup")
    plain, coloured = str(tmp_path / "plain.ply"), str(tmp_path / "coloured.ply")
    ME.write_ply(plain, v, f)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    body = v.astype("<f4").tobytes() + b"".join(b"\x03" + row.astype("<i4").tobytes() for row in f)
    assert open(plain, "rb").read() == header + body
    v2, f2, c2 = ME.read_ply(plain)
    assert c2 is None and v2.dtype == np.float32 and f2.dtype == np.int32 and np.array_equal(v2, v) and np.array_equal(f2, f)
    u8 = np.rint(c * 255).astype(np.uint8)
    ME.write_ply(coloured, v, f, c)
    v3, f3, c3 = ME.read_ply(coloured)
    assert np.array_equal(v3, v) and np.array_equal(f3, f) and c3.dtype == np.uint8 and np.array_equal(c3, u8)
    ME.write_ply(plain, v, f, u8)                         # uint8 colours are stored as they are
    assert open(plain, "rb").read() == open(coloured, "rb").read()
    assert os.path.getsize(coloured) == os.path.getsize(plain)
    w = WO.MeshWorld(v3, f3, c3)                          # uint8 colours are code / 255
    assert np.array_equal(w.colors.numpy(), u8.astype(np.float32) / np.float32(255))
    open(plain, "wb").write(header.replace(b"binary_little_endian", b"ascii") + body)
    with pytest.raises(ValueError):
        ME.read_ply(plain)
    open(plain, "wb").write(header + body[:-1])
    with pytest.raises(ValueError):
        ME.read_ply(plain)


def test_henge_mesh_is_deterministic():
    a, b = SC.henge_mesh(16), SC.henge_mesh(16)
    assert a[0].dtype == np.float32 and a[1].dtype == np.int32 and a[2].dtype == np.float32
    assert len(a[0]) > 500 and len(a[1]) > 1000 and a[2].shape == a[0].shape
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].min() == 0 and a[1].max() == len(a[0]) - 1 and np.abs(a[0]).max() <= 1
    assert (a[2] >= 0).all() and (a[2] <= 1).all() and len(np.unique(np.round(a[2], 1), axis=0)) >= 4      # ground, stones, lintels differ
    # the field is 0 / 1 and the threshold 0.5: every vertex is the midpoint of a lattice edge whose ends differ in occupancy
    idx = (a[0].astype(np.float64) + 1) / 2 * 15
    assert np.abs(2 * idx - np.rint(2 * idx)).max() < 1e-4
    axis = np.linspace(-1.0, 1.0, 16)
    occ = SC.henge_occupancy(axis[:, None, None], axis[None, :, None], axis[None, None, :])
    ends = [occ[tuple(np.floor(idx + 1e-3).astype(int).T)], occ[tuple(np.ceil(idx - 1e-3).astype(int).T)]]
    half = np.abs(idx - np.rint(idx)).max(1) > 0.25
    assert half.all() and (ends[0] != ends[1]).all()
    assert (a[0][:, 1] < -0.29).any() and (a[0][:, 1] > 0.04).any()                       # the ground and the lintels are there


def test_run_validation_checks_the_simulator():
    from nerfsafetyvalidation_amd import rollout as RO
    with pytest.raises(ValueError, match="world"):
        RO.run_validation(RO.STRESS_MONTE_CARLO, None, None, 8, 8, 1, 1, simulator="BlenderSimulator")
    with pytest.raises(ValueError, match="world"):
        RO.run_validation(RO.STRESS_CEM, None, None, 8, 8, 1, simulator="BlenderSimulator", world=None)
    with pytest.raises(ValueError, match="simulator"):
        RO.run_validation(RO.STRESS_MONTE_CARLO, None, None, 8, 8, 1, 1, simulator="GazeboSimulator")
    with pytest.raises(ValueError, match="stress test"):
        RO.run_validation("Grid Search", None, None, 8, 8, 1, 1, simulator="BlenderSimulator", world=object())
    assert RO.RolloutSimulator(None, None, 8, 8, 2).world is None


def test_make_mesh_dataset_loads_through_the_provider(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import make_mesh_dataset as MD
    finally:
        sys.path.pop(0)
    from nerfsafetyvalidation_amd.nerf import provider as P
    v, f, c = RC.mesh("henge")
    ply = str(tmp_path / "henge.ply")
    ME.write_ply(ply, v, f, c)
    out = MD.make(str(tmp_path / "ds"), size=8, n_train=3, n_val=1, n_test=1, ply=ply, device="cpu")
    opt = SimpleNamespace(preload=False, bound=2, fp16=False, num_rays=16, rand_pose=-1, error_map=False, color_space="srgb", path=out, scale=1.0,
                          offset=[0, 0, 0])
    d = P.NeRFDataset(opt, "cpu", type="train")
    assert (d.H, d.W) == (8, 8) and len(d.poses) == 3 and d.images.shape[-1] == 4
    assert np.array_equal(d.poses.numpy(), SC.orbit_poses()[[0, 66, 133]])
    rgba = d.images.data.numpy().reshape(3, 8, 8, 4)
    assert set(np.unique(rgba[..., 3])) == {0, 255}                                       # alpha: 1 on a hit, 0 on a miss
    world = WO.MeshWorld(*ME.read_ply(ply))
    want = world.render(torch.from_numpy(SC.orbit_poses()[66]), SC.intrinsics(8, 8), 8, 8, bg_color=0.0)
    assert np.array_equal(rgba[1, ..., :3], want["image_u8"].numpy()) and np.array_equal(rgba[1, ..., 3] == 255, want["prim"].numpy() >= 0)
    assert len(P.NeRFDataset(opt, "cpu", type="val").poses) == 1
