"""The voxelisation rule (world.py's docstring) on its numpy path: hand-built triangles in a dyadic box, where the float64 cell
geometry is exact and every answer is known; the candidate ranges against the brute force over all cells; the properties the rule
promises (a superset of the vertex-only map, independent of the order of the faces and of each face's vertices); the Python interface
around it.  No GPU."""
import numpy as np
import pytest
import torch

import raycast_cases as RC
import voxelize_cases as VC
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import world as WO
from nerfsafetyvalidation_amd.mesh import mesh_to_world

f32 = np.float32
HAND = VC.BOXES["hand"]                      # start (-0.5, -0.25, 0), 0.25 m cells, shape (5, 4, 3)
ONE = np.array([[0, 1, 2]], np.int32)


def cells(occ):
    return sorted(tuple(int(i) for i in c) for c in np.argwhere(occ))


def vox(vertices, faces=ONE, box=HAND, **kw):
    return WO.voxelize_numpy(np.asarray(vertices, f32), faces, box, **kw)


def test_a_triangle_inside_one_cell_marks_that_cell():
    # cell (1, 2, 1) is [-0.25, 0] x [0.25, 0.5] x [0.25, 0.5]
    occ = vox([[-0.2, 0.3, 0.3], [-0.1, 0.3, 0.4], [-0.15, 0.45, 0.35]])
    assert occ.shape == HAND.shape and occ.dtype == bool and cells(occ) == [(1, 2, 1)]


def test_a_triangle_in_a_boundary_plane_marks_both_sides():
    """in the plane x = 0 between cells 1 and 2, strictly inside (j, k) = (2, 1): the test is closed, so both cells touch it"""
    occ = vox([[0.0, 0.3, 0.3], [0.0, 0.45, 0.3], [0.0, 0.3, 0.45]])
    assert cells(occ) == [(1, 2, 1), (2, 2, 1)]
    for axis, (lo, hi) in enumerate([((1, 2, 1), (2, 2, 1)), ((2, 1, 1), (2, 2, 1)), ((2, 2, 0), (2, 2, 1))]):
        tri = np.array([[0.05, 0.3, 0.3], [0.2, 0.3, 0.3], [0.05, 0.45, 0.45]])       # inside cell (2, 2, 1) ...
        tri[:, axis] = [0.0, 0.25, 0.25][axis]                                        # ... flattened onto its lower face
        tri[:, (axis + 1) % 3] += [0.0, 0.04, 0.0]                                   # (keeps it a triangle)
        assert cells(vox(tri)) == [lo, hi], axis


def test_a_triangle_touching_a_cell_at_a_corner_marks_it():
    """one vertex on the corner (0, 0.25, 0.25) shared by eight cells, the rest of the triangle inside cell (2, 2, 1)"""
    occ = vox([[0.0, 0.25, 0.25], [0.2, 0.3, 0.4], [0.1, 0.45, 0.3]])
    assert cells(occ) == sorted((i, j, k) for i in (1, 2) for j in (1, 2) for k in (0, 1))
    # pulled off the corner by one float32 step along every axis, only its own cell is left
    eps = np.float32(2.0 ** -20)
    assert cells(vox([[eps, 0.25 + eps, 0.25 + eps], [0.2, 0.3, 0.4], [0.1, 0.45, 0.3]])) == [(2, 2, 1)]


@pytest.mark.parametrize("s", [0.625, 0.5, 1.0, -0.75, 2.25, 2.375])
def test_a_large_triangle_in_a_diagonal_plane(s):
    """the part x, y, z >= -5 of the plane x + y + z = s covers the box: exactly the cells whose corner sums straddle s are marked --
    closed, so for s on the lattice of corner sums (0.5, 1.0; -0.75 and 2.25 are the box's two extreme corners) a cell that meets the
    plane in one corner counts; all of it exact in float64"""
    big = 15.0 + s
    occ = vox([[big - 5.0, -5.0, -5.0], [-5.0, big - 5.0, -5.0], [-5.0, -5.0, big - 5.0]])
    i, j, k = np.meshgrid(*[np.arange(n) for n in HAND.shape], indexing="ij")
    low = sum(HAND.start) + (i + j + k) * 0.25
    want = (low <= s) & (s <= low + 0.75)
    assert np.array_equal(occ, want)
    assert want.sum() == {0.625: 31, 0.5: 37, 1.0: 37, -0.75: 1, 2.25: 1, 2.375: 0}[s]


def test_zero_area_faces_mark_their_vertices_and_stay_in_their_bounding_box():
    a, b = np.array([-0.45, -0.2, 0.05]), np.array([0.7, 0.7, 0.7])
    for tri in ([a, a, b], [a, b, a], [b, a, a], [a, (a + b) / 2, b]):
        occ = vox(tri)
        assert occ[0, 0, 0] and occ[4, 3, 2]                                          # the cells of a and b
        assert 5 <= occ.sum() < occ.size // 2                                         # a chain of cells from one to the other, not a slab
        assert np.array_equal(occ, vox(tri, all_cells=True))
    seg = vox([[-0.2, 0.3, 0.3], [-0.2, 0.3, 0.3], [0.45, 0.3, 0.3]])                 # along x inside the row (j, k) = (2, 1)
    assert cells(seg) == [(1, 2, 1), (2, 2, 1), (3, 2, 1)]
    point = vox([[0.3, 0.1, 0.6]] * 3)
    assert cells(point) == [(3, 1, 2)]
    assert cells(vox([[0.25, 0.25, 0.25]] * 3)) == sorted((i, j, k) for i in (2, 3) for j in (1, 2) for k in (0, 1))   # a point on a corner


def test_a_mesh_outside_the_box_marks_nothing():
    assert not vox([[2.0, 0.1, 0.1], [3.0, 0.2, 0.1], [2.0, 0.3, 0.6]]).any()
    assert not vox([[0.1, 0.1, -0.3], [0.6, 0.2, -0.3], [0.2, 0.6, -0.3]]).any()       # more than a cell below the floor
    assert not vox([[0.1, 0.1, 1e30], [0.6, 0.2, 2e30], [0.2, 0.6, 3e30]]).any()
    for name in RC.MESHES:
        assert not VC.reference(name, "miss").any()
    # a triangle whose bounding box holds the box while its plane passes it by
    assert not vox([[30.0, -10.0, -10.0], [-10.0, 30.0, -10.0], [-10.0, -10.0, 30.0]]).any()


def test_a_mesh_cut_by_the_box_is_clipped():
    """the hand box is the block [2:7, 3:7, 4:7] of a larger box on the same (dyadic) lattice: its map is that block of the larger map"""
    large = CO.GridBox((-1.0, -1.0, -1.0), 4, (12, 12, 12))
    for name in RC.MESHES:
        v, f, _ = RC.mesh(name)
        vw = VC.world_vertices(name, "planner")
        whole = WO.voxelize_numpy(vw, f, large)
        assert np.array_equal(VC.reference(name, "hand"), whole[2:7, 3:7, 4:7]), name
        assert whole.sum() > VC.reference(name, "hand").sum() > 0, name
    tri = [[-2.0, 0.1, 0.1], [3.0, 0.3, 0.1], [0.3, 4.0, 0.3]]
    assert np.array_equal(vox(tri), vox(tri, box=large)[2:7, 3:7, 4:7]) and vox(tri).any()


@pytest.mark.parametrize("box", VC.SMALL)
@pytest.mark.parametrize("name", RC.MESHES)
def test_candidate_ranges_equal_the_brute_force(name, box):
    _, f, _ = RC.mesh(name)
    brute = WO.voxelize_numpy(VC.world_vertices(name, "planner"), f, VC.BOXES[box], all_cells=True)
    assert np.array_equal(VC.reference(name, box), brute)
    assert brute.any()


def test_candidate_ranges_hold_every_overlapping_cell():
    """the ranges themselves on the non-dyadic box: every (face, cell) pair the test accepts lies inside the face's range"""
    box = VC.BOXES["odd"]
    _, f, _ = RC.mesh("soup")
    vw = VC.world_vertices("soup", "planner")
    lo, n = WO.face_candidates(vw, f, box)
    assert np.array_equal(VC.reference("soup", "odd"), WO.voxelize_numpy(vw, f, box, all_cells=True))
    h = 0.5 / box.granularity
    ijk = np.stack(np.meshgrid(*[np.arange(s) for s in box.shape], indexing="ij"), -1).reshape(-1, 3)
    centre = np.asarray(box.start) + (ijk + 0.5) / box.granularity
    for face in list(range(0, 478, 37)) + list(RC.ZERO_AREA) + list(RC.LARGE):
        tri = np.broadcast_to(vw[f[face]].astype(np.float64), (len(ijk), 3, 3))
        hit = ijk[WO.tri_box_overlap(tri, centre, h)]
        assert ((hit >= lo[face]) & (hit < lo[face] + n[face])).all(), face


@pytest.mark.parametrize("name", RC.MESHES)
def test_the_map_holds_the_vertex_only_map(name):
    v, f, _ = RC.mesh(name)
    used = np.unique(f)
    for key in ("hand", "around", "cut", "odd"):
        points = CO.occupancy_from_points(mesh_to_world(v[used]), VC.BOXES[key]).numpy()
        occ = VC.reference(name, key)
        assert not (points & ~occ).any(), (name, key)
        assert occ.any() and (points.any() or name == "cube"), (name, key)      # (the cut box holds faces of the cube, no corner)
        if name == "soup" or key == "odd":
            assert occ.sum() > points.sum(), (name, key)           # triangles larger than a cell add the cells between their vertices
    # the henge's triangles are larger than a 1/40 m cell: the vertex-only map has the holes this map is there to close
    if name == "henge":
        box = CO.GridBox((-1.0, -1.0, -0.25), 40, (32, 32, 24))
        occ = WO.voxelize_numpy(VC.world_vertices(name, "planner"), f, box)
        points = CO.occupancy_from_points(mesh_to_world(v[used]), box).numpy()
        assert not (points & ~occ).any() and points.sum() < 0.5 * occ.sum()


@pytest.mark.parametrize("name", RC.MESHES)
def test_the_map_ignores_the_order_of_faces_and_of_their_vertices(name):
    _, f, _ = RC.mesh(name)
    vw = VC.world_vertices(name, "planner")
    rng = np.random.default_rng(7)
    for key in ("around", "odd"):
        want = VC.reference(name, key)
        assert np.array_equal(WO.voxelize_numpy(vw, f[rng.permutation(len(f))], VC.BOXES[key]), want)
        for shift in (1, 2):
            assert np.array_equal(WO.voxelize_numpy(vw, np.roll(f, shift, axis=1), VC.BOXES[key]), want), (key, shift)
        assert np.array_equal(WO.voxelize_numpy(vw, f[:, ::-1], VC.BOXES[key]), want)         # and the winding


def test_rot_identity_and_planner_and_what_is_refused():
    v, f, _ = RC.mesh("soup")
    world = WO.MeshWorld(v, f)
    box = VC.BOXES["around"]
    same = world.occupancy(box, VC.IDENTITY)
    assert isinstance(same, torch.Tensor) and same.dtype == torch.bool and tuple(same.shape) == box.shape and same.device.type == "cpu"
    assert np.array_equal(same.numpy(), WO.voxelize_numpy(v, f, box))                 # identity: the vertices as they are
    turned = world.occupancy(box)                                                     # PLANNER_ROT: world = NeRF (z, x, y)
    assert np.array_equal(turned.numpy(), VC.reference("soup", "around"))
    assert np.array_equal(VC.world_vertices("soup", "planner"), mesh_to_world(v).astype(f32))
    assert np.array_equal(turned.numpy(), same.numpy().transpose(2, 0, 1)) and not np.array_equal(turned.numpy(), same.numpy())
    flip = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]
    assert np.array_equal(world.occupancy(box, flip).numpy(), WO.voxelize_numpy(np.stack([-v[:, 1], v[:, 0], -v[:, 2]], 1), f, box))
    assert np.array_equal(CO.occupancy_from_mesh(world, box).numpy(), turned.numpy())
    c, s = np.cos(0.7), np.sin(0.7)
    for bad in ([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], [[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
                [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]],
                [[0.5, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0]], np.eye(2), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            world.occupancy(box, bad)
    for bad_box in (CO.GridBox((0.0, 0.0, 0.0), 4, (0, 3, 3)), CO.GridBox((0.0, 0.0, 0.0), 0.0, (3, 3, 3)),
                    CO.GridBox((0.0, np.inf, 0.0), 4, (3, 3, 3)), CO.GridBox((0.0, 0.0, 0.0), 4, (2048, 2048, 512)),
                    CO.GridBox((1e13, 0.0, 0.0), 4, (3, 3, 3))):
        with pytest.raises(ValueError):
            world.occupancy(bad_box)


def test_map_agreement_on_hand_maps():
    truth = np.zeros((2, 3, 2), bool)
    pred = np.zeros((2, 3, 2), bool)
    truth[0, 0, 0] = truth[0, 1, 0] = truth[1, 2, 1] = truth[1, 0, 0] = True
    pred[0, 0, 0] = pred[0, 1, 0] = pred[0, 2, 0] = True
    got = CO.map_agreement(pred, truth)
    assert got == {"tp": 2, "fp": 1, "fn": 2, "tn": 7, "iou": 2 / 5, "precision": 2 / 3, "recall": 2 / 4}
    assert all(type(got[k]) is int for k in ("tp", "fp", "fn", "tn")) and all(type(got[k]) is float for k in ("iou", "precision", "recall"))
    assert CO.map_agreement(torch.from_numpy(pred), torch.from_numpy(truth)) == got
    assert CO.map_agreement(truth, truth) == {"tp": 4, "fp": 0, "fn": 0, "tn": 8, "iou": 1.0, "precision": 1.0, "recall": 1.0}
    none = np.zeros_like(truth)
    assert CO.map_agreement(none, truth) == {"tp": 0, "fp": 0, "fn": 4, "tn": 8, "iou": 0.0, "precision": 1.0, "recall": 0.0}
    assert CO.map_agreement(none, none) == {"tp": 0, "fp": 0, "fn": 0, "tn": 12, "iou": 1.0, "precision": 1.0, "recall": 1.0}
    with pytest.raises(ValueError):
        CO.map_agreement(pred, truth[:1])


def test_sdf_world_needs_a_world():
    from nerfsafetyvalidation_amd import cem as CE
    from nerfsafetyvalidation_amd import rollout as RO
    with pytest.raises(ValueError, match="needs world="):
        RO.RolloutSimulator(None, None, 8, 8, 4, sdf="world")
    with pytest.raises(ValueError, match="needs world="):
        RO.run_rollout(None, None, 8, 8, 2, 4, sdf="world")
    with pytest.raises(ValueError, match="needs world="):
        CE.run_cem(None, None, 8, 8, 4, sdf="world")
    for stress in (RO.STRESS_MONTE_CARLO, RO.STRESS_CEM):
        with pytest.raises(ValueError, match="needs world="):
            RO.run_validation(stress, None, None, 8, 8, 2, 4, sdf="world")
    with pytest.raises(ValueError, match="'world'"):
        RO.RolloutSimulator(None, None, 8, 8, 4, sdf="mesh")
    # None and a field pass through untouched
    field = CO.SignedDistanceField(np.ones((2, 2, 2)), HAND)
    assert RO.RolloutSimulator(None, None, 8, 8, 4, sdf=field).sdf is field and RO.RolloutSimulator(None, None, 8, 8, 4).sdf is None


def test_from_mesh_of_a_cpu_world():
    """ngp_edt_sq is a HIP kernel: a CPU world's (numpy) map is moved to the HIP device when there is one, as from_occupancy does with
    any host map; without one from_mesh says so"""
    v, f, _ = RC.mesh("cube")
    world = WO.MeshWorld(v, f)
    box = VC.BOXES["around"]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            CO.SignedDistanceField.from_mesh(world, box)
        return
    field = CO.SignedDistanceField.from_mesh(world, box)
    want = CO.SignedDistanceField.from_occupancy(torch.from_numpy(VC.reference("cube", "around").copy()), box)
    assert field.box == box and np.array_equal(field.values, want.values)
    # the cube's faces lie in cell-boundary planes and mark the cells on both sides: 0, 1, 8 and 9 of every axis
    assert field.values[5, 5, 5] == 3 / 8 and field.values[4, 4, 4] == 3 / 8 and field.values[0, 0, 0] == 0.0
