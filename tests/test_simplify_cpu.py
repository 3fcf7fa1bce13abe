"""mesh.simplify, the numpy path that defines it: the properties of the rule (DESIGN.md "Mesh simplification") on hand-built meshes.
No GPU."""
import os

import numpy as np
import pytest
import torch

import simplify_cases as SC
from nerfsafetyvalidation_amd import mesh as M

SQRT3 = float(np.sqrt(3.0))


def _cells(vertices, cell, origin):
    o = np.asarray(origin if origin is not None else vertices.min(0), np.float64)
    return np.floor((vertices.astype(np.float64) - o) / cell).astype(np.int64), o


def _checked(v, f, cell, origin=None, placement="quadric"):
    """simplify, with what holds for every input: dtypes and shapes, no face repeats an index, every output vertex is referenced,
    faces are the surviving input faces under vertex_map in input order, every mapped input vertex lies in its output vertex's cell
    (so within sqrt(3) cell of it), every output vertex in its closed cell"""
    ov, of, vmap = M.simplify(v, f, cell, origin=origin, placement=placement)
    assert ov.dtype == np.float32 and of.dtype == np.int32 and vmap.dtype == np.int32
    assert ov.shape == (len(ov), 3) and of.shape == (len(of), 3) and vmap.shape == (len(v),)
    if len(v) == 0 or len(f) == 0:
        assert len(ov) == 0 and len(of) == 0 and (vmap == -1).all()
        return ov, of, vmap
    idx, o = _cells(v, cell, origin)
    fc = idx[f]                                                        # [F,3,3]
    keep = ((fc[:, 0] != fc[:, 1]).any(1) & (fc[:, 1] != fc[:, 2]).any(1) & (fc[:, 0] != fc[:, 2]).any(1))
    assert np.array_equal(of, vmap[f[keep]]) and (of >= 0).all()
    assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
    assert np.array_equal(np.unique(of), np.arange(len(ov)))
    mapped = vmap >= 0
    assert np.array_equal(np.unique(vmap[mapped]), np.arange(len(ov)))
    # vertices of one cell share an output vertex, and the output vertices follow the cells' (ix, iy, iz) order
    out_cell = np.zeros((len(ov), 3), np.int64)
    out_cell[vmap[mapped]] = idx[mapped]
    assert (out_cell[vmap[mapped]] == idx[mapped]).all()
    key = (out_cell[:, 0] << 42) | (out_cell[:, 1] << 21) | out_cell[:, 2]
    assert (np.diff(key) > 0).all()
    # the closed cell, in double; the output is rounded to float32 once more, which moves it by at most half a float32 ulp
    lo, hi = o + out_cell * cell, o + (out_cell + 1) * cell
    slack = 0.5 * np.spacing(np.abs(ov)).astype(np.float64) + 1e-15 * np.abs(lo)
    assert (ov >= lo - slack).all() and (ov <= hi + slack).all()
    dist = np.linalg.norm(v[mapped].astype(np.float64) - ov[vmap[mapped]].astype(np.float64), axis=1)
    assert dist.size == 0 or dist.max() <= SQRT3 * cell * (1 + 1e-6)
    return ov, of, vmap


def _directed_edges_balance(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    n = int(e.max()) + 1 if e.size else 1
    fwd = np.bincount(e[:, 0] * n + e[:, 1], minlength=n * n)
    return np.array_equal(fwd.reshape(n, n), fwd.reshape(n, n).T)


@pytest.fixture(scope="module")
def sphere48():
    v, f = SC.sphere_mesh(48, 18.0)
    assert _directed_edges_balance(f)
    return v, f


@pytest.fixture(scope="module")
def cube():
    v, f = SC.cube_surface()
    assert len(v) == 6 * 64 + 2 and len(f) == 6 * 128 and _directed_edges_balance(f)
    return v, f


def test_identity_below_the_smallest_gap(cube):
    """every referenced vertex comes back with its bits, in key order; faces are the input's under vertex_map; unreferenced: -1"""
    v, f = cube
    v = np.concatenate([v, np.array([[4.2, 4.2, 4.2], [1.1, 7.7, 3.3]], np.float32)])      # two vertices no face uses
    for placement in ("quadric", "mean"):
        ov, of, vmap = _checked(v, f, 0.4, origin=(-0.1, -0.1, -0.1), placement=placement)
        assert len(ov) == len(v) - 2 and (vmap[-2:] == -1).all() and (vmap[:-2] >= 0).all()
        assert np.array_equal(ov[vmap[:-2]].view(np.uint32), v[:-2].view(np.uint32))
        assert np.array_equal(of, vmap[f]) and len(of) == len(f)
        order = np.lexsort((v[:-2, 2], v[:-2, 1], v[:-2, 0]))
        assert np.array_equal(ov, v[:-2][order])


@pytest.mark.parametrize("cell", [2.0, 3.7])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_cell_bound_on_a_sphere(sphere48, cell, placement):
    v, f = sphere48
    ov, of, vmap = _checked(v, f, cell, origin=(0.0, 0.0, 0.0) if cell == 2.0 else None, placement=placement)
    d = np.linalg.norm(v[vmap >= 0].astype(np.float64) - ov[vmap[vmap >= 0]], axis=1).max() / cell
    print(f"cell {cell} {placement}: V {len(v)} -> {len(ov)}, F {len(f)} -> {len(of)}, max move {d:.3f} cell")
    if cell == 2.0:
        assert 4 * len(of) <= len(f)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_a_closed_surface_stays_closed(sphere48, cube, placement):
    """every directed edge (u, v) of the output occurs as often as (v, u): the boundary of a collapsed face cancels, which is why
    duplicate faces stay"""
    for (v, f), cells in ((sphere48, (1.5, 2.0, 3.7, 6.0, 11.0, 40.0)), (cube, (0.9, 2.0, 2.5, 3.0, 4.1, 9.5))):
        for cell in cells:
            ov, of, _ = _checked(v, f, cell, origin=(-0.5, -0.5, -0.5), placement=placement)
            assert _directed_edges_balance(of), (cell, placement)
    assert len(_checked(*cube, 9.5, origin=(-0.5, -0.5, -0.5), placement=placement)[1]) == 0


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_planes_stay_planes(placement):
    v, f = SC.plane_patch()
    assert np.abs(v).max() <= 32
    ov, of, _ = _checked(v, f, 3.3, placement=placement)
    assert 20 < len(ov) < len(v) // 4
    off = np.abs((ov.astype(np.float64) - SC.PLANE_BASE) @ SC.PLANE_NORMAL)
    print(f"{placement}: largest distance from the plane {off.max():.3g}")
    assert off.max() <= 4 * float(np.spacing(np.float32(np.abs(v).max())))


@pytest.mark.parametrize("origin,cell", [((-0.5, -0.5, -0.5), 3.0), ((-0.75, -0.75, -0.75), 2.5)])
def test_corners_stay_corners(cube, origin, cell):
    """what tells the quadric placement from the mean: the cube's corners survive the first and are rounded off by the second"""
    corners = np.array([[x, y, z] for x in (0, 8) for y in (0, 8) for z in (0, 8)], np.float64)
    nearest = {}
    for placement in ("quadric", "mean"):
        ov, _, _ = _checked(*cube, cell, origin=origin, placement=placement)
        nearest[placement] = np.linalg.norm(ov[None].astype(np.float64) - corners[:, None], axis=-1).min(1)
        print(f"cell {cell} {placement}: nearest output vertex to a corner {nearest[placement].min() / cell:.4f} .. {nearest[placement].max() / cell:.4f} cell")
    assert nearest["quadric"].max() <= 0.01 * cell
    assert nearest["mean"].min() > 0.25 * cell


def test_on_a_cell_face_is_the_upper_cell():
    v, f = SC.on_face()
    ov, of, vmap = _checked(v, f, 2.0, origin=(0.0, 0.0, 0.0))
    assert np.array_equal(vmap, [1, 0, 2]) and np.array_equal(of, [[1, 0, 2]]) and np.array_equal(ov, v[[1, 0, 2]])


def test_zero_area_faces_give_the_mean():
    v, f = SC.collinear()
    ov, of, vmap = _checked(v, f, 1.0, origin=(0.0, 0.0, 0.0))
    assert np.array_equal(vmap, [0, 0, 1, 2]) and np.array_equal(of, [[0, 1, 2], [0, 2, 1]])
    assert np.array_equal(ov, np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], np.float32))
    # a zero-area face next to real ones contributes nothing: the result with and without it differs only by that face
    cv, cf = SC.cube_surface()
    extra = np.concatenate([cf, np.array([[0, 0, 300], [5, 200, 5]], np.int32)])
    a, b = M.simplify(cv, cf, 3.0, origin=(-0.5,) * 3), M.simplify(cv, extra, 3.0, origin=(-0.5,) * 3)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2], b[2])


def test_a_minimiser_outside_the_cell_falls_back_to_the_mean():
    v, f = SC.far_minimiser()
    q = _checked(v, f, 1.0, origin=(0.0, 0.0, 0.0))
    m = _checked(v, f, 1.0, origin=(0.0, 0.0, 0.0), placement="mean")
    assert np.array_equal(q[2], [0, 0, 1, 2, 1, 2]) and np.array_equal(q[1], m[1])
    assert np.array_equal(q[0].view(np.uint32), m[0].view(np.uint32))
    assert np.allclose(q[0][0], [0.55, 0.5, 0.49], atol=1e-6)
    # the regularised minimiser itself, by a library solve: beyond the cell [0,1)^3 along x
    V = v.astype(np.float64)
    Q, qb, pc = np.zeros((3, 3)), np.zeros(3), np.array([0.5, 0.5, 0.5])
    for face in f:
        A, B, C = V[face]
        n = np.cross(B - A, C - A)
        Q += np.outer(n, n)
        qb += -n.dot(A - pc) * n
    mu = M.SIMPLIFY_LAMBDA * np.trace(Q)
    x = np.linalg.solve(Q + mu * np.eye(3), mu * (V[:2].mean(0) - pc) - qb)
    assert x[0] > 1.5 and abs(x[2]) < 0.1


def test_everything_in_one_cell_and_empty_inputs():
    v, f = SC.random_mesh(300, 500, 3, extent=1.0)
    ov, of, vmap = _checked(v, f, 2.0, origin=(0.0, 0.0, 0.0))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and (vmap == -1).all() and len(vmap) == 300
    for V, F in ((0, 0), (1, 0), (300, 0)):
        _checked(*SC.random_mesh(V, F, 1), 1.0)
    # tensors in, tensors out
    tv, tf, tm = M.simplify(torch.from_numpy(v), torch.from_numpy(f), 0.25)
    nv, nf, nm = M.simplify(v, f, 0.25)
    assert tv.dtype == torch.float32 and tf.dtype == torch.int32 and tm.dtype == torch.int32
    assert np.array_equal(tv.numpy().view(np.uint32), nv.view(np.uint32)) and np.array_equal(tf.numpy(), nf) and np.array_equal(tm.numpy(), nm)


def test_refusals():
    v, f = SC.cube_surface()
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            M.simplify(v, f, cell)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[7, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            M.simplify(w, f, 1.0, origin=(0.0, 0.0, 0.0))
        with pytest.raises(ValueError):
            M.simplify(w, f, 1.0)
    with pytest.raises(ValueError, match="below"):
        M.simplify(v, f, 1.0, origin=(0.0, 0.5, 0.0))
    M.simplify(v, f, 8.0 / (2 ** 21 - 1))                       # the largest index there is, 2^21 - 1
    with pytest.raises(ValueError, match="2\\^21"):
        M.simplify(v, f, 8.0 / 2 ** 21)
    for bad in (-1, len(v)):
        g = f.copy()
        g[11, 2] = bad
        with pytest.raises(ValueError, match="face index"):
            M.simplify(v, g, 1.0)
    with pytest.raises(ValueError, match="face index"):
        M.simplify(np.zeros((0, 3), np.float32), np.zeros((1, 3), np.int32), 1.0)
    with pytest.raises(ValueError, match="placement"):
        M.simplify(v, f, 1.0, placement="median")


def test_every_case_holds_the_general_properties():
    for name, (v, f, cell, origin) in SC.all_cases().items():
        for placement in ("quadric", "mean"):
            _checked(v, f, cell, origin=origin, placement=placement)


class _Blob(torch.nn.Module):
    """a density with a blob in the middle of [-1, 1]^3 (CPU)"""

    def __init__(self):
        super().__init__()
        self.register_buffer("aabb_infer", torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]))

    def density(self, x):
        return {"sigma": 40.0 * torch.exp(-4.0 * (x * torch.tensor([1.0, 1.5, 2.0])).pow(2).sum(-1))}


def test_save_mesh_and_extract_geometry_with_simplify_cell(tmp_path):
    model, R = _Blob(), 32
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
    query = lambda p: model.density(p)["sigma"]
    plain = M.extract_geometry(lo, hi, R, 10, query)
    zero = M.extract_geometry(lo, hi, R, 10, query, simplify_cell=0)
    assert np.array_equal(plain[0], zero[0]) and np.array_equal(plain[1], zero[1])
    a, b, c = (os.path.join(tmp_path, n) for n in ("a.ply", "b.ply", "c.ply"))
    M.save_mesh(model, a, resolution=R, threshold=10)
    M.save_mesh(model, b, resolution=R, threshold=10, simplify_cell=0)
    assert open(a, "rb").read() == open(b, "rb").read()

    verts, tris = M.save_mesh(model, c, resolution=R, threshold=10, simplify_cell=2)
    iv, itri = M.isosurface(M.extract_fields(lo, hi, R, query).numpy(), 10)
    sv, sf, _ = M.simplify(iv, itri, 2, origin=(0.0, 0.0, 0.0))
    assert 0 < 4 * len(sf) <= len(itri) and np.array_equal(tris, sf)
    b_min, b_max = lo.numpy(), hi.numpy()
    assert np.array_equal(verts, sv.astype(np.float64) / (R - 1.0) * (b_max - b_min)[None, :] + b_min[None, :])
    rv, rf, colors = M.read_ply(c)
    assert colors is None and np.array_equal(rf, sf) and np.array_equal(rv, verts.astype(np.float32))
    with pytest.raises(ValueError, match="simplify_cell"):
        M.extract_geometry(lo, hi, R, 10, query, simplify_cell=-1)

    # Trainer.save_mesh hands the keyword on (its default writes the plain file)
    import types
    from nerfsafetyvalidation_amd.nerf.trainer import Trainer
    stub = types.SimpleNamespace(model=model, fp16=False, log=lambda *a, **k: None, workspace=str(tmp_path), name="blob", epoch=3)
    d, e = os.path.join(tmp_path, "d.ply"), os.path.join(tmp_path, "e.ply")
    Trainer.save_mesh(stub, d, resolution=R, threshold=10)
    Trainer.save_mesh(stub, e, resolution=R, threshold=10, simplify_cell=2)
    assert open(d, "rb").read() == open(a, "rb").read() and open(e, "rb").read() == open(c, "rb").read()
