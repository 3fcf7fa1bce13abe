"""ngp_simplify_* (csrc/simplify.hip) against mesh.py's numpy path, which defines the result: faces, vertex_map and sizes equal,
vertices equal bit for bit; and one pass through save_mesh on a model."""
import os
import time

import numpy as np
import pytest
import torch

import simplify_cases as SC
from nerfsafetyvalidation_amd import mesh as M

pytestmark = pytest.mark.gpu

CASES = SC.all_cases()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _hip(v, f, cell, origin, placement, device):
    out = M.simplify(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), cell, origin=origin, placement=placement)
    assert all(t.is_cuda for t in out) and out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[2].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in out)


def _assert_equal(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[2].shape == want[2].shape, what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    if not _same_bits(got[0], want[0]):
        bad = np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want[0])} vertices differ, first {bad[:5]}: {got[0][bad[:5]]} against {want[0][bad[:5]]}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_path_gives_the_numpy_path_bits(device, name):
    """both placements, on the default stream and on a side stream, and twice: the same bits on every call"""
    v, f, cell, origin = CASES[name]
    side = torch.cuda.Stream(device)
    for placement in ("quadric", "mean"):
        want = M.simplify(v, f, cell, origin=origin, placement=placement)
        _assert_equal(_hip(v, f, cell, origin, placement, device), want, f"{name} {placement}")
        with torch.cuda.stream(side):
            _assert_equal(_hip(v, f, cell, origin, placement, device), want, f"{name} {placement} side stream")
        side.synchronize()
        _assert_equal(_hip(v, f, cell, origin, placement, device), want, f"{name} {placement} again")


def test_twenty_thousand_faces_in_one_cell_finish_quickly(device):
    """a cell that holds the whole mesh is walked by one wave, 64 corners a round: milliseconds, not a lane-serial pass"""
    v, f, cell, origin = CASES["one_cell"]
    tv, tf = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    M.simplify(tv, tf, cell, origin=origin)          # (warm: the library and torch's sort are loaded)
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = M.simplify(tv, tf, cell, origin=origin)
    torch.cuda.synchronize()
    s = time.perf_counter() - t
    print(f"one_cell: {len(f)} faces, {s * 1e3:.2f} ms")
    assert out[0].shape == (3, 3) and out[1].shape == (1, 3) and s < 0.25


def test_a_refused_input_raises_and_leaves_the_library_usable(device):
    v, f, cell, origin = CASES["cube_3"]
    tv, tf = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    with pytest.raises(ValueError, match="below"):
        M.simplify(tv, tf, cell, origin=(0.0, 0.5, 0.0))
    bad = tv.clone()
    bad[5, 2] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        M.simplify(bad, tf, cell, origin=origin)
    with pytest.raises(ValueError, match="2\\^21"):
        M.simplify(tv, tf, 8.0 / 2 ** 21, origin=(0.0, 0.0, 0.0))
    g = tf.clone()
    g[3, 1] = len(v)
    with pytest.raises(ValueError, match="face index"):
        M.simplify(tv, g, cell, origin=origin)
    with pytest.raises(ValueError, match="face index"):
        M.simplify(torch.zeros(0, 3, device=device), torch.zeros(1, 3, dtype=torch.int32, device=device), 1.0)
    for kw in ({"cell": 0.0}, {"cell": float("nan")}, {"cell": 1.0, "placement": "median"}):
        with pytest.raises(ValueError):
            M.simplify(tv, tf, kw.pop("cell"), **kw)
    _assert_equal(tuple(t.cpu().numpy() for t in M.simplify(tv, tf, cell, origin=origin)), M.simplify(v, f, cell, origin=origin), "after the refusals")


def test_save_mesh_with_simplify_cell_on_the_henge_model(device, tmp_path):
    """One pass through the pipeline: save_mesh(simplify_cell=2) at 64^3 on the synthetic scene's model; the file reads back as what
    was returned, and that is simplify() of the isosurface, scaled to the bounds.  Every point of the simplified surface is within
    sqrt(3) cell (world units) of the unsimplified one: an output triangle is an input triangle whose corners moved by at most that
    much, so a point of it is a blend of three points that each have their input corner that near, and the same blend of those corners
    lies on the input triangle.  The opposite direction is NOT asserted: features thinner than a cell may vanish."""
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    from nerfsafetyvalidation_amd.world import MeshWorld
    model = StonehengeScene(H=8, W=8, bound=2).build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    model.eval()
    R, cell = 64, 2
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]

    def query(pts):
        with torch.no_grad():
            return model.density(pts.to(device))["sigma"]

    u = M.extract_fields(lo, hi, R, query)
    thr = float(u.median())
    full_v, full_f = M.save_mesh(model, os.path.join(tmp_path, "full.ply"), resolution=R, threshold=thr)
    path = os.path.join(tmp_path, "simplified.ply")
    verts, tris = M.save_mesh(model, path, resolution=R, threshold=thr, simplify_cell=cell)
    rv, rf, _ = M.read_ply(path)
    assert np.array_equal(rf, tris) and np.array_equal(rv, verts.astype(np.float32))
    assert 0 < len(tris) < len(full_f) and 0 < len(verts) < len(full_v) // 2

    iv, itri = M.isosurface(u, thr)
    sv, sf, _ = M.simplify(iv, itri, cell, origin=(0.0, 0.0, 0.0))
    b_min, b_max = lo.cpu().numpy(), hi.cpu().numpy()
    assert np.array_equal(tris, sf.cpu().numpy())
    assert np.array_equal(verts, sv.cpu().numpy().astype(np.float64) / (R - 1.0) * (b_max - b_min)[None, :] + b_min[None, :])
    _assert_equal(tuple(t.cpu().numpy() for t in (sv, sf)) + (np.zeros(0),),
                  M.simplify(iv.cpu().numpy(), itri.cpu().numpy(), cell, origin=(0.0, 0.0, 0.0))[:2] + (np.zeros(0),), "the henge surface")

    step = float(((b_max - b_min) / (R - 1.0)).max())                  # one lattice step in world units (the bounds are a cube)
    samples = M.sample_surface(torch.from_numpy(verts).to(device, torch.float32), torch.from_numpy(tris).to(device), 20000, seed=3)
    world = MeshWorld(torch.from_numpy(full_v).to(device, torch.float32), torch.from_numpy(full_f).to(device))
    d = world.closest(samples, 4.0 * cell * step)["distance"]
    print(f"henge 64^3: F {len(full_f)} -> {len(tris)}; largest distance to the full surface {float(d.max()) / (cell * step):.3f} cell")
    assert float(d.max()) <= np.sqrt(3.0) * cell * step * (1 + 1e-5)
