"""ngp_label_components / ngp_component_stats (csrc/components.hip) against the package's numpy path (itself held against scipy in
test_components_cpu.py), and the floater API and mesh.drop_small_components on device tensors."""
import numpy as np
import pytest
import torch

import components_cases as CC
from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import mesh as M

pytestmark = pytest.mark.gpu


def _put(occ, device):
    """a pattern as the device tensor of its kind: a bool map as bool, a strided view as a strided tensor"""
    t = torch.from_numpy(np.ascontiguousarray(occ)).to(device)
    if not occ.flags["C_CONTIGUOUS"]:
        wide = torch.zeros(occ.shape[0], occ.shape[1], 2 * occ.shape[2], dtype=t.dtype, device=device)
        wide[:, :, ::2] = t
        t = wide[:, :, ::2]
        assert not t.is_contiguous() or t.numel() < 4
    return t


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_labels_equal_the_numpy_path(device, case):
    shape, name = case
    occ = _put(CC.pattern(shape, name), device)
    for c in CC.CONNECTIVITIES:
        want, n_want = CC.numpy_labels(shape, name, c)
        got, n = CO.label_components(occ, c)
        assert got.dtype == torch.int32 and got.device == occ.device and got.shape == occ.shape and got.is_contiguous()
        assert n == n_want, (case, c)
        assert np.array_equal(got.cpu().numpy(), want), (case, c)
        again, n2 = CO.label_components(occ, c)
        assert n2 == n and torch.equal(again, got)


@pytest.mark.parametrize("name", ["snake", "u"])
@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_the_longest_paths_stay_within_the_loop_bounds(device, shape, name):
    """the legitimate worst case: one component about N / 4 cells long (the snake), or one whose two halves meet only in the last
    layer (the U).  A loop that reached its bound would raise here (n_components < 0)."""
    occ = _put(CC.pattern(shape, name), device)
    for c in CC.CONNECTIVITIES:
        labels, n = CO.label_components(occ, c)
        assert n == 1 and torch.equal(labels != 0, occ != 0) and int(labels.max()) == 1


def test_on_a_non_default_stream(device):
    shape = (33, 34, 66)
    occ = _put(CC.pattern(shape, "fill30"), device)
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        for c in CC.CONNECTIVITIES:
            got, n = CO.label_components(occ, c)
            table = CO.component_table(got, n, occ)
            want, n_want = CC.numpy_labels(shape, "fill30", c)
            assert n == n_want and np.array_equal(got.cpu().numpy(), want)
            assert torch.equal(table.cells, table.overlap) and int(table.cells.sum()) == int(CC.pattern(shape, "fill30").sum())
    torch.cuda.current_stream(device).wait_stream(stream)


TABLE_CASES = [(s, p) for s in [(1, 1, 130), (3, 5, 7), (17, 9, 65), (33, 34, 66), (96, 92, 24)]
               for p in ("empty", "full", "checkerboard", "fill10", "fill60", "snake", "combs")]


@pytest.mark.parametrize("case", TABLE_CASES, ids=CC.case_id)
def test_component_table_equals_the_numpy_path(device, case):
    """`full` is one component: every lane of every wave adds to one row"""
    shape, name = case
    truth = CC.pattern(shape, "fill30")
    truth_dev = torch.from_numpy(truth.copy()).to(device)
    for c in (6, 26):
        labels, n = CC.numpy_labels(shape, name, c)
        want = CO.component_table_numpy(labels, n, truth)
        lab_dev = torch.from_numpy(labels.copy()).to(device)
        got = CO.component_table(lab_dev, n, truth_dev)
        assert got.cells.dtype == torch.int64 and got.lo.dtype == torch.int32 and got.hi.dtype == torch.int32 and got.overlap.dtype == torch.int64
        assert all(a.device == lab_dev.device for a in (got.cells, got.lo, got.hi, got.overlap))
        assert got.cells.shape == (n,) and got.lo.shape == (n, 3) and got.hi.shape == (n, 3) and got.overlap.shape == (n,)
        for a, b in ((got.cells, want.cells), (got.lo, want.lo), (got.hi, want.hi), (got.overlap, want.overlap)):
            assert np.array_equal(a.cpu().numpy(), b), (case, c)
        bare = CO.component_table(lab_dev, n)
        assert bare.overlap is None and torch.equal(bare.cells, got.cells) and torch.equal(bare.lo, got.lo) and torch.equal(bare.hi, got.hi)


def test_remove_floaters_and_floater_report_on_the_device(device):
    sc = CC.check_floater_api(lambda a: torch.from_numpy(a.copy()).to(device), lambda a: a.cpu().numpy())
    CC.check_floater_errors(lambda a: torch.from_numpy(a.copy()).to(device))
    # the cleaned map's distance field is the field of the truth without the component that was taken out
    box = CO.reference_box()
    cleaned, _ = CO.remove_floaters(torch.from_numpy(sc["pred"].copy()).to(device), grounded=(2, "lo"))
    want = CO.SignedDistanceField.from_occupancy(torch.from_numpy(sc["truth"] & ~sc["removed"]).to(device), box)
    assert np.array_equal(CO.SignedDistanceField.from_occupancy(cleaned, box).values, want.values)


def test_drop_small_components_then_the_hip_isosurface(device):
    u = CC.two_blobs()
    cleaned_cpu = M.drop_small_components(u, 0.0, 40)
    v_want, f_want = M.isosurface(cleaned_cpu, 0.0)
    u_dev = torch.from_numpy(u.copy()).to(device)
    cleaned = M.drop_small_components(u_dev, 0.0, 40)
    assert cleaned.device == u_dev.device and cleaned.dtype == torch.float32 and np.array_equal(cleaned.cpu().numpy(), cleaned_cpu)
    v, f = M.isosurface(cleaned, 0.0)
    assert v.cpu().numpy().tobytes() == v_want.tobytes() and np.array_equal(f.cpu().numpy(), f_want)
    assert M.drop_small_components(u_dev, 0.0, 0) is u_dev


def test_argument_checks_launch_nothing(device):
    """a short workspace and a bad connectivity are refused on the host: the outputs keep their bits"""
    lib = _lib.lib()
    X, Y, Z = 9, 10, 33
    occ = torch.ones(X, Y, Z, dtype=torch.uint8, device=device)
    labels = torch.full((X, Y, Z), -7, dtype=torch.int32, device=device)
    n_dev = torch.full((1,), -7, dtype=torch.int32, device=device)
    need = lib.ngp_label_components_workspace(X, Y, Z)
    assert need >= 4 * X * Y * Z and lib.ngp_label_components_workspace(0, Y, Z) == 0 and lib.ngp_label_components_workspace(1 << 16, 1 << 16, 1) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    call = lambda conn, nbytes, x=X: lib.ngp_label_components(_lib.ptr(occ), x, Y, Z, conn, _lib.ptr(labels), _lib.ptr(n_dev), _lib.ptr(ws),   # noqa: E731
                                                              nbytes, _lib.stream())
    assert call(26, need - 1) == -3 and b"workspace too small" in lib.ngp_last_error()          # NGP_EWORKSPACE
    assert call(7, need) == -1 and b"connectivity" in lib.ngp_last_error()                       # NGP_EINVAL
    assert call(26, need, 0) == -1
    torch.cuda.synchronize(device)
    assert int((labels != -7).sum()) == 0 and int(n_dev) == -7 and int(ws.sum()) == 0
    assert call(26, need) == 0
    torch.cuda.synchronize(device)
    assert int(n_dev) == 1 and int((labels != 1).sum()) == 0
    # an n that is label_components' report of a loop bound is refused by name, on the host
    cells = torch.zeros(1, dtype=torch.int64, device=device)
    box = torch.zeros(2, 3, dtype=torch.int32, device=device)
    rc = lib.ngp_component_stats(_lib.ptr(labels), X, Y, Z, -2, None, _lib.ptr(cells), _lib.ptr(box[0]), _lib.ptr(box[1]), None, _lib.stream())
    assert rc == -2 and b"seams" in lib.ngp_last_error()
    with pytest.raises(ValueError):
        CO.label_components(occ, 7)
