"""Connected components on the CPU: collision.label_components_numpy against scipy.ndimage.label (the independent yardstick; the
package itself never imports scipy), component_table against bincount / find_objects, remove_floaters and floater_report on the
synthetic scene, and mesh.drop_small_components.  No GPU."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import components_cases as CC
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import mesh as M


def test_offsets_are_the_mesh_edges_and_scipy_structures():
    assert CO.KUHN_OFFSETS == M.EDGE_OFFSETS
    for c in CC.CONNECTIVITIES:
        offsets = CO.connectivity_offsets(c)
        assert len(offsets) == len(set(offsets)) == c and all(tuple(-v for v in o) in offsets for o in offsets)
        s = np.zeros((3, 3, 3), bool)
        s[1, 1, 1] = True
        for dx, dy, dz in offsets:
            s[1 + dx, 1 + dy, 1 + dz] = True
        assert np.array_equal(s, CC.structure(c))


def test_the_numpy_path_does_not_import_scipy():
    text = open(CO.__file__).read() + open(M.__file__).read()
    assert "import scipy" not in text and "from scipy" not in text and "ndimage." not in text.replace("scipy.ndimage.", "")


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_numpy_labels_equal_scipy(case):
    shape, name = case
    occ = CC.pattern(shape, name)
    assert occ.shape == tuple(shape)
    for c in CC.CONNECTIVITIES:
        want, n_want = CC.scipy_labels(shape, name, c)
        got, n = CC.numpy_labels(shape, name, c)
        assert got.dtype == np.int32 and want.dtype == np.int32 and got.shape == tuple(shape)
        assert n == n_want and np.array_equal(got, want), (case, c)
        # ranked by the first cell in C order
        first = np.unique(got.reshape(-1), return_index=True)[1][1 if (got == 0).any() else 0:]
        assert np.all(np.diff(first) > 0)


@pytest.mark.parametrize("shape", [(3, 5, 7), (17, 9, 65), (33, 34, 66)], ids=str)
def test_exact_counts(shape):
    """the counts that tell the four connectivities apart, worked out by hand"""
    N = int(np.prod(shape))
    for c in CC.CONNECTIVITIES:
        n = lambda name: CC.numpy_labels(shape, name, c)[1]          # noqa: E731
        assert n("empty") == 0 and n("full") == 1 and n("snake") == 1 and n("u") == 1
        # a checkerboard's cells differ from their neighbours in parity under 6; an offset with two non-zero entries keeps the parity,
        # and (1,1,0), (1,0,1), (0,1,1) (in 14, 18 and 26) join every even cell to every other within a few steps
        assert n("checkerboard") == ((N + 1) // 2 if c == 6 else 1)
        assert n("corners") == 8                                     # every dimension here is >= 3: no two corners are neighbours
        for d in CC.CHAIN_DIRECTIONS:
            name = "chain" + "".join("m" if v < 0 else str(v) for v in d)
            length = int(CC.pattern(shape, name).sum())
            assert length == min(n_ for n_, v in zip(shape, d) if v != 0)
            assert n(name) == (1 if CC.CHAIN_IS_ONE[d][c] else length), (d, c)
    if shape[1] >= 5:
        assert all(CC.numpy_labels(shape, "combs", c)[1] == 2 for c in CC.CONNECTIVITIES)
    assert int(CC.pattern(shape, "snake").sum()) >= N // 5


def test_label_components_kinds_and_errors():
    occ = CC.pattern((17, 9, 65), "fill30")
    want, n_want = CC.scipy_labels((17, 9, 65), "fill30", 26)
    got, n = CO.label_components(occ)                                           # numpy in, numpy out; 26 is the default
    assert isinstance(got, np.ndarray) and n == n_want and np.array_equal(got, want)
    got, n = CO.label_components(torch.from_numpy(occ.copy()).bool(), 26)     # CPU tensor in, CPU tensor out
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and not got.is_cuda and n == n_want and np.array_equal(got.numpy(), want)
    for bad in (7, 0, "26", None):
        with pytest.raises(ValueError):
            CO.label_components(occ, bad)
    with pytest.raises(ValueError):
        CO.label_components(occ[0])
    with pytest.raises(ValueError):
        CO.label_components(np.zeros((0, 3, 3), np.uint8))


@pytest.mark.parametrize("case", [(s, p) for s in [(1, 1, 130), (3, 5, 7), (17, 9, 65), (33, 34, 66)] for p in ("empty", "full", "fill10", "fill60", "snake")],
                         ids=CC.case_id)
def test_component_table_equals_bincount_and_find_objects(case):
    shape, name = case
    truth = CC.pattern(shape, "fill30")
    for c in (6, 26):
        labels, n = CC.numpy_labels(shape, name, c)
        t = CO.component_table(labels, n, truth)
        assert t.cells.dtype == np.int64 and t.lo.dtype == np.int32 and t.hi.dtype == np.int32 and t.overlap.dtype == np.int64
        assert t.cells.shape == (n,) and t.lo.shape == (n, 3) and t.hi.shape == (n, 3) and t.overlap.shape == (n,)
        assert np.array_equal(t.cells, np.bincount(labels.reshape(-1), minlength=n + 1)[1:])
        boxes = ndimage.find_objects(labels, max_label=n)
        assert np.array_equal(t.lo, np.array([[s.start for s in b] for b in boxes], np.int32).reshape(n, 3))
        assert np.array_equal(t.hi, np.array([[s.stop - 1 for s in b] for b in boxes], np.int32).reshape(n, 3))
        assert np.array_equal(t.overlap, np.bincount(labels[truth != 0], minlength=n + 1)[1:])
        for k in list(range(min(n, 5))) + ([n - 1] if n else []):           # and by mask
            assert t.overlap[k] == int(((labels == k + 1) & (truth != 0)).sum())
        assert CO.component_table(labels, n).overlap is None
        tt = CO.component_table(torch.from_numpy(labels.copy()), n, torch.from_numpy(truth.copy()))
        assert all(isinstance(a, torch.Tensor) for a in (tt.cells, tt.lo, tt.hi, tt.overlap))
        assert np.array_equal(tt.cells.numpy(), t.cells) and np.array_equal(tt.lo.numpy(), t.lo) and np.array_equal(tt.overlap.numpy(), t.overlap)


def test_the_scene_is_what_the_cases_say():
    sc = CC.floater_scene()
    for c in CC.CONNECTIVITIES:
        labels, n = CC.scipy_labels_of(sc["truth"], c)
        assert n == 6
        cells = np.bincount(labels.reshape(-1))[1:]
        assert cells.min() == 244 and all((labels[:, :, 0] == k + 1).any() for k in range(6))
        assert np.array_equal(labels == 3, sc["removed"])
        # the blobs are more than one cell away from the rest of the map and from each other: growing them by one cell meets nothing
        grown = ndimage.binary_dilation(sc["blobs"], np.ones((3, 3, 3), bool))
        assert not (grown & sc["truth"]).any()
        assert ndimage.label(grown, np.ones((3, 3, 3)))[1] == 4


@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_remove_floaters_and_floater_report(kind):
    if kind == "numpy":
        CC.check_floater_api(lambda a: a.copy(), lambda a: np.asarray(a))
    else:
        CC.check_floater_api(lambda a: torch.from_numpy(a.copy()), lambda a: a.numpy())


def test_remove_floaters_errors():
    CC.check_floater_errors(lambda a: a.copy())
    CC.check_floater_errors(lambda a: torch.from_numpy(a.copy()))


def test_occupancy_from_density_passes_the_keywords_on(monkeypatch):
    sc = CC.floater_scene()
    sigma = torch.from_numpy(sc["pred"].astype(np.float32))
    monkeypatch.setattr(CO, "cell_max_density", lambda *a, **k: sigma)
    box = CO.reference_box()
    assert np.array_equal(CO.occupancy_from_density(None, box, 0.5).numpy(), sc["pred"])
    assert np.array_equal(CO.occupancy_from_density(None, box, 0.5, min_cells=200, connectivity=6).numpy(),
                          CO.remove_floaters(sc["pred"], connectivity=6, min_cells=200)[0])
    assert np.array_equal(CO.occupancy_from_density(None, box, 0.5, grounded=(2, "lo")).numpy(), sc["truth"] & ~sc["removed"])


# ------------------------------------------------------------------ mesh.drop_small_components
def test_drop_small_components_gives_the_mesh_without_the_small_blob():
    u, alone = CC.two_blobs(), CC.two_blobs(small=False)
    n_small = int(((u > 0) & ~(alone > 0)).sum())
    assert 0 < n_small < 40 < int((alone > 0).sum())
    v_all, f_all = M.isosurface(u, 0.0)
    v_want, f_want = M.isosurface(alone, 0.0)
    assert len(f_want) < len(f_all)
    cleaned = M.drop_small_components(u, 0.0, 40)
    assert cleaned.dtype == u.dtype and np.array_equal(cleaned != u, (u > 0) & ~(alone > 0)) and np.all(cleaned[cleaned != u] == 0.0)
    v, f = M.isosurface(cleaned, 0.0)
    assert v.tobytes() == v_want.tobytes() and np.array_equal(f, f_want)
    # both blobs have at least n_small points: nothing goes at that bound, everything above the large one's size
    assert M.drop_small_components(u, 0.0, n_small).tobytes() == u.tobytes()
    assert not (M.drop_small_components(u, 0.0, 10 ** 6) > 0).any()
    # a tensor comes back as a tensor, with the same values; NaN is outside and stays
    t = torch.from_numpy(u.copy())
    t[0, 0, 0] = float("nan")
    got = M.drop_small_components(t, 0.0, 40)
    assert isinstance(got, torch.Tensor) and torch.isnan(got[0, 0, 0]) and np.array_equal(got.numpy()[1:], cleaned[1:])


class _Blob(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("aabb_infer", torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.5, 2.0]))

    def density(self, x):
        return {"sigma": 20.0 * torch.exp(-((x - torch.tensor([0.1, 0.2, 0.4])) ** 2).sum(-1) * 3.0)}


def test_min_points_zero_is_the_identity(tmp_path):
    u = CC.two_blobs()
    assert M.drop_small_components(u, 0.0, 0) is u and M.drop_small_components(u, 0.0, 1) is u
    with pytest.raises(ValueError):
        M.drop_small_components(u, 0.0, -1)
    a, b, c = [os.path.join(tmp_path, n) for n in ("a.ply", "b.ply", "c.ply")]
    M.save_mesh(_Blob(), a, resolution=24, threshold=10)
    M.save_mesh(_Blob(), b, resolution=24, threshold=10, min_points=0)
    assert open(a, "rb").read() == open(b, "rb").read()
    verts, tris = M.save_mesh(_Blob(), c, resolution=24, threshold=10, min_points=10 ** 6)
    assert len(verts) == 0 and len(tris) == 0
