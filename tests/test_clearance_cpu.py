"""The clearance rule on the CPU (world.py's docstring): the numpy paths that define it -- world.box_tri_distance2 / box_clearance_numpy,
collision.box_cell_distance2 / box_cells_clearance_numpy -- on hand cases with exact answers, against dense sampling, against each
other and against the body rule's verdict; and the simulators' `clearance` keyword."""
import numpy as np
import pytest
import torch

import body_cases as BC
import clearance_cases as CC
import raycast_cases as RC
import voxelize_cases as VC
from nerfsafetyvalidation_amd import cem as CE
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import rollout as RO
from nerfsafetyvalidation_amd import world as WO
from test_body_cpu import COLUMN, _column_field, _stub_sim

FACE0 = np.array([[0, 1, 2]], np.int32)
HAND = BC.HAND_BOX[None]


def _one(tri, max_distance=CC.INF):
    out = WO.box_clearance_numpy(HAND, CC.triangle(tri)[0].astype(np.float32), FACE0, max_distance)
    assert out["distance"].dtype == np.float64 and out["prim"].dtype == np.int32 and out["hit"].dtype == np.int32
    return float(out["distance"][0]), int(out["prim"][0]), int(out["hit"][0])


# ------------------------------------------------------------------------------------------------------------- hand cases
@pytest.mark.parametrize("name", list(CC.HAND))
def test_hand_triangle_has_its_exact_distance(name):
    tri, d2 = CC.HAND[name]
    assert float(WO.box_tri_distance2(HAND, CC.triangle(tri))[0]) == d2
    assert _one(tri) == (float(np.sqrt(d2)), 0, -1)


def _vertex_rules_only(tri):
    """the smallest of the rule's first 11 candidates (3 vertices against the box, 8 corners against the triangle): the rule without
    its 36 edge pairs"""
    c, R, h, _ = WO.box_parts(HAND)
    p = [WO.box_frame(c, R, CC.triangle(tri)[:, k]) for k in range(3)]
    hh = [h[:, a] for a in range(3)]
    cands = [WO.clamp_gap2(p[k], hh) for k in range(3)]
    for m in range(8):
        cands.append(WO.point_tri_d2([hh[a] if (m >> a) & 1 else -hh[a] for a in range(3)], p[0], p[1], p[2]))
    return float(np.min(cands))


def test_edge_pairs_are_needed():
    """in the edge-to-edge case both vertex rules give a strictly larger value: dropping the 36 edge pairs would report it"""
    tri = CC.HAND["edge to edge"][0]
    assert _vertex_rules_only(tri) > 2.0 + 0.1
    for name in ("a parallel face at gap 3", "a vertex over a face", "a corner over the interior"):
        assert _vertex_rules_only(CC.HAND[name][0]) == CC.HAND[name][1]


@pytest.mark.parametrize("name", list(BC.HAND))
def test_touching_is_zero_and_a_dyadic_step_away_is_not(name):
    """body_cases' triangles: where the verdict is overlap the distance is 0.0 and hit names the face; the touching ones moved by OFF
    (2^-10 for the large one) are a positive distance of at most that away, and hit is -1"""
    tri, overlaps = BC.HAND[name]
    d, prim, hit = _one(tri)
    if overlaps:
        assert (d, prim, hit) == (0.0, 0, 0)
    else:
        assert d > 0.0 and prim == 0 and hit == -1
        if name.startswith("off "):
            assert d <= BC.OFF
        if name == "large, off the corner":
            assert d <= 2.0 ** -10
        if name in ("zero area: a segment beside the box", "zero area: a point off the face"):
            assert d == BC.OFF                                       # a zero-area face is a segment or a point: the rule is defined there


def test_lowest_index_wins_and_bad_rows_are_infinitely_far():
    v, f = BC.hand_mesh()
    boxes, want, _ = BC.hand_boxes()
    out = WO.box_clearance_numpy(boxes, v, f)
    assert out["hit"].tolist() == want.tolist()
    assert out["prim"][0] == 0 and out["distance"][0] == 0.0                        # the duplicate of face 0 is the last face
    assert out["prim"][1:4].tolist() == [-1] * 3 and np.isinf(out["distance"][1:4]).all()      # NaN, an infinite centre, a negative extent
    # 8 along -x: x in [-7.25, -6.75]; the segment through y = 2, z = 0.5 ends at x = 0, 6.75 away, and a large triangle passes nearer
    assert out["prim"][4] >= 0 and 0.0 < out["distance"][4] <= 6.75
    # a duplicated face that does not touch: the lower index
    far = CC.triangle(CC.HAND["a vertex over a face"][0])[0].astype(np.float32)
    out = WO.box_clearance_numpy(HAND, np.concatenate([far, far]), np.arange(6).reshape(2, 3))
    assert (float(out["distance"][0]), int(out["prim"][0]), int(out["hit"][0])) == (0.5, 0, -1)


def test_beyond_max_distance_is_infinitely_far():
    assert _one(CC.HAND["a parallel face at gap 3"][0], CC.MAX_DISTANCE_FAR) == (CC.INF, -1, -1)
    assert _one(CC.HAND["a parallel face at gap 3"][0], 3.0) == (3.0, 0, -1)        # accepted iff distance <= max_distance
    d, prim, hit = _one(CC.LARGE_AROUND)                                            # the triangle's bounds hold the box, its plane is far
    assert abs(d - 8.0 / 3.0 ** 0.5) < 1e-4 and (prim, hit) == (0, -1)              # (float32 vertices at 64: 2^-17)
    assert _one(CC.LARGE_AROUND, CC.MAX_DISTANCE_FAR) == (CC.INF, -1, -1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            _one(CC.LARGE_AROUND, bad)
        with pytest.raises(ValueError, match="max_distance"):
            CO.box_cells_clearance_numpy(HAND, np.ones((1, 1, 1), bool), CO.GridBox((0.0, 0.0, 0.0), 32, (1, 1, 1)), bad)


# ------------------------------------------------------------------------------------------------------------- sampling
def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    boxes = BC.random_boxes([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n, seed, half=(0.2, 0.1, 0.05))
    boxes[:, 12:15] = rng.uniform(0.01, 0.25, (n, 3))
    tri = rng.uniform(-0.5, 1.5, (n, 3, 3)).astype(np.float32).astype(np.float64)
    return boxes, tri


def test_rule_against_dense_sampling():
    """600 seeded pairs, the disjoint ones: the triangle sampled on a barycentric lattice of n = 100 points per edge, every sample's
    distance to the box by the exact clamp.  Every point of a triangle with the longest edge L lies within L / n of a lattice point and
    the point-box distance is 1-Lipschitz, so 0 <= sampled - rule <= L / n (1e-12 of float slack on either side)."""
    n = 100
    boxes, tri = _random_pairs(600, 5)
    d2, over = WO._box_tri_terms(boxes, tri)
    assert np.array_equal(d2, WO.box_tri_distance2(boxes, tri)) and np.array_equal(over, WO.box_tri_overlap(boxes, tri))
    assert np.array_equal(d2 == 0.0, over)
    u, v = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    keep = u + v <= n
    u, v = u[keep] / n, v[keep] / n
    pts = tri[:, 0, None, :] * (1 - u - v)[None, :, None] + tri[:, 1, None, :] * u[None, :, None] + tri[:, 2, None, :] * v[None, :, None]
    c, R, h, _ = WO.box_parts(boxes)
    local = np.einsum("mia,mni->mna", R, pts - c[:, None, :])
    g = np.maximum(np.abs(local) - h[:, None, :], 0.0)
    sampled = np.sqrt((g * g).sum(-1)).min(1)
    L = np.max([np.linalg.norm(tri[:, i] - tri[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))], 0)
    free = ~over
    diff = sampled[free] - np.sqrt(d2[free])
    print(f"{free.sum()} disjoint pairs: sampled - rule in [{diff.min():.3e}, {diff.max():.3e}], at most {(diff / (L[free] / n)).max():.3f} L / n")
    assert free.sum() >= 300 and over.sum() >= 20
    assert (diff >= -1e-12).all() and (diff <= L[free] / n + 1e-12).all()
    assert (sampled[over] <= L[over] / n + 1e-12).all()                             # an overlapping triangle has a sample that near


def test_cell_rule_agrees_with_the_triangle_rule_on_the_cells_surface():
    """400 seeded (box, cell) pairs: where they are disjoint the cell rule's distance equals the smallest of the triangle rule's over
    the cell's 12 surface triangles, to 1e-12"""
    boxes, _ = _random_pairs(400, 6)
    centre = np.random.default_rng(60).uniform(0.2, 0.8, (400, 3))
    s = np.float64(0.5 / 8)
    d2, over = CO._box_cell_terms(boxes, centre, s)
    assert np.array_equal(d2, CO.box_cell_distance2(boxes, centre, s)) and np.array_equal(over, CO.box_cell_overlap(boxes, centre, s))
    v, f, _ = RC.cube()
    best = np.full(400, np.inf)
    for face in f:
        t = centre[:, None, :] + (v.astype(np.float64)[face] * 2 - 1)[None] * s
        best = np.minimum(best, WO.box_tri_distance2(boxes, t))
    free = ~over
    print(f"{free.sum()} disjoint pairs: max |cell rule - triangle rule| = {np.abs(np.sqrt(d2) - np.sqrt(best))[free].max():.3e}")
    assert free.sum() >= 200 and over.sum() >= 20
    assert np.abs(np.sqrt(d2) - np.sqrt(best))[free].max() <= 1e-12
    assert (d2[over] == 0.0).all() and (d2[free] > 0.0).all()


# ------------------------------------------------------------------------------------------------------------- the verdict
@pytest.mark.parametrize("rot", list(VC.ROTS))
@pytest.mark.parametrize("name", RC.MESHES)
def test_mesh_clearance_is_consistent_with_the_verdict(name, rot):
    D, smaller, third = CC.MESH_MAX_DISTANCE[name]
    out = CC.mesh_clearance(name, rot, D)
    assert np.array_equal(out["hit"], BC.mesh_reference(name, rot)[:CC.N])
    assert np.array_equal(out["distance"] == 0.0, out["hit"] >= 0) and np.array_equal(out["prim"][out["hit"] >= 0], out["hit"][out["hit"] >= 0])
    share = CC.shares(out, "prim")
    print(f"{name} / {rot}: hit, gap, beyond = {share}")
    assert min(share) >= CC.MIN_SHARE
    assert np.isinf(out["distance"][17]) and out["prim"][17] == -1                  # body_cases' NaN row
    for other in (smaller, third):
        if rot != "planner" and other == CC.INF:
            continue
        a, b = (out, CC.mesh_clearance(name, rot, other)) if other < D else (CC.mesh_clearance(name, rot, other), out)
        gone = np.isinf(b["distance"])                                               # the smaller max_distance only takes results away
        assert np.array_equal(b["hit"], a["hit"]) and (a["distance"][gone] > min(D, other)).all()
        assert np.array_equal(CC.bits(a["distance"][~gone]), CC.bits(b["distance"][~gone])) and np.array_equal(a["prim"][~gone], b["prim"][~gone])
        assert (b["prim"][gone] == -1).all()


@pytest.mark.parametrize("box", list(VC.BOXES))
def test_map_clearance_is_consistent_with_the_verdict(box):
    share_mesh, D, smaller, larger = CC.MAP_MAX_DISTANCE[box]
    grid = VC.BOXES[box]
    for mesh in RC.MESHES:
        out = CC.map_clearance(mesh, box, D)
        want = np.concatenate([BC.map_reference(mesh, box)[:CC.N], BC.map_reference(mesh, box)[-4:]])
        assert np.array_equal(out["hit"], want)
        assert np.array_equal(out["distance"] == 0.0, out["hit"] >= 0) and np.array_equal(out["cell"][out["hit"] >= 0], want[want >= 0])
        assert np.isinf(out["distance"][-3:]).all() and (out["cell"][-3:] == -1).all()     # far outside, a NaN row, a negative extent
        share = CC.shares(out, "cell")
        print(f"{mesh} in {box}: hit, gap, beyond = {share}")
        if mesh == share_mesh:
            assert min(share) >= CC.MIN_SHARE
        if box == "hand":                                                            # nearly every box hits this small map
            assert share[0] >= CC.HAND_HIT_SHARE
        if box == "miss":                                                            # an empty map: everything is beyond max_distance
            assert share == (0.0, 0.0, 1.0) and not VC.reference(mesh, box).any()
        for a, b, limit in ((out, CC.map_clearance(mesh, box, smaller), smaller), (CC.map_clearance(mesh, box, larger), out, D)):
            gone = np.isinf(b["distance"])                                           # the smaller max_distance only takes results away
            assert np.array_equal(b["hit"], a["hit"]) and (a["distance"][gone] > limit).all() and (b["cell"][gone] == -1).all()
            assert np.array_equal(CC.bits(a["distance"][~gone]), CC.bits(b["distance"][~gone])) and np.array_equal(a["cell"][~gone], b["cell"][~gone])
        for max_distance in (D, smaller, larger):                                    # every cell a candidate: bit for bit the same
            pruned = CC.map_clearance(mesh, box, max_distance)
            brute = CO.box_cells_clearance_numpy(CC.map_boxes(box), VC.reference(mesh, box), grid, max_distance, all_cells=True)
            assert np.array_equal(CC.bits(brute["distance"]), CC.bits(pruned["distance"])), max_distance
            assert np.array_equal(brute["cell"], pruned["cell"]) and np.array_equal(brute["hit"], pruned["hit"]), max_distance


# ------------------------------------------------------------------------------------------------------------- the interface
def test_dispatch_on_the_host():
    v, f, _ = RC.mesh("soup")
    D = CC.MESH_MAX_DISTANCE["soup"][0]
    want = CC.mesh_clearance("soup", "planner", D)
    boxes = BC.mesh_boxes("soup", "planner")[:CC.N]
    world = WO.MeshWorld(np.array(v), np.array(f))
    out = world.box_clearance(np.array(boxes), D)
    assert all(isinstance(out[k], np.ndarray) and np.array_equal(out[k], want[k]) for k in ("distance", "prim", "hit"))
    out = world.box_clearance(torch.from_numpy(np.array(boxes)), D)
    assert all(isinstance(out[k], torch.Tensor) and np.array_equal(out[k].numpy(), want[k]) for k in ("distance", "prim", "hit"))
    assert world.box_clearance(boxes[:0])["distance"].shape == (0,)
    with pytest.raises(ValueError, match="max_distance"):
        world.box_clearance(boxes, -1.0)
    grid, occ = VC.BOXES["cut"], VC.reference("henge", "cut")
    D = CC.MAP_MAX_DISTANCE["cut"][1]
    want = CC.map_clearance("henge", "cut", D)
    out = CO.box_cells_clearance(CC.map_boxes("cut"), occ, grid, D)
    assert all(isinstance(out[k], np.ndarray) and np.array_equal(out[k], want[k]) for k in ("distance", "cell", "hit"))
    out = CO.box_cells_clearance(CC.map_boxes("cut"), torch.from_numpy(np.array(occ)), grid, D)
    assert all(isinstance(out[k], torch.Tensor) and np.array_equal(out[k].numpy(), want[k]) for k in ("distance", "cell", "hit"))
    field = CO.SignedDistanceField(np.where(occ, 0.0, 1.0), grid)
    out = field.box_clearance(CC.map_boxes("cut"), D)
    assert all(np.array_equal(out[k], want[k]) for k in ("distance", "cell", "hit"))
    with pytest.raises(ValueError, match="max_distance"):
        field.box_clearance(CC.map_boxes("cut"), float("nan"))


def test_trajectory_clearance_rescoring():
    """states [n, 6] -> the boxes' clearance in one call, against the field's cells or the world's triangles"""
    field = _column_field()
    body = CO.BodyBox.planner()
    states = np.array([[-0.275, -0.4875, 0.275, 0.0, 0.0, 0.0], [-0.18, -0.538, 0.28, 0.0, 0.0, 0.0], [0.5, 0.5, 0.3, 0.0, 0.0, 0.3]])
    out = CO.trajectory_clearance(states, body, sdf=field, max_distance=0.25)
    want = CO.box_cells_clearance_numpy(CO.body_boxes(states, body), field.occupied, field.box, 0.25)
    assert all(np.array_equal(out[k], want[k]) for k in ("distance", "cell", "hit"))
    # the last pose of the body test's step 1 ends 2.5 cm short of the column in x; the next pose hits it; the third is far
    assert abs(out["distance"][0] - 0.025) < 1e-12 and out["distance"][1] == 0.0 and out["hit"][1] >= 0 and np.isinf(out["distance"][2])
    with pytest.raises(ValueError, match="world="):
        CO.trajectory_clearance(states, body, sdf=field, exact=True, max_distance=0.25)
    with pytest.raises(ValueError, match="BodyBox"):
        CO.trajectory_clearance(states, None, sdf=field, max_distance=0.25)


# ------------------------------------------------------------------------------------------------------------- the simulator
def _walk_minimum(distances, hits, D):
    gap = D
    for d, h in zip(distances, hits):
        gap = min(gap, min(float(d), D))
        if h >= 0:
            break
    return gap


def test_simulator_scores_the_body_s_gap():
    """test_body_cpu's column beside the path.  clearance=None is the body= run byte for byte; with clearance=D the collided column
    is unchanged and column 14 is the smallest min(distance, D) over the poses the walk visits, the distances those of the numpy path
    on the recorded poses: D in open space (step 0), 2.5 cm at the last pose of step 1, 0.0 at the hit"""
    field, body, D = _column_field(), CO.BodyBox.planner(), 0.25
    plain = _stub_sim(sdf=field, body=body)
    rows = plain.run(0)
    none = _stub_sim(sdf=field, body=body, clearance=None)
    assert none.run(0).tobytes() == rows.tobytes() and none.body_clearance == [] and plain.body_clearance == []
    states = []

    class Spy(type(_stub_sim(sdf=field))):
        def measure_body(self, st):
            states.append(np.array(st))
            return super().measure_body(st)

    sim = Spy(None, None, 8, 8, 4, sdf=field, body=body, clearance=D)
    got = sim.run(0)
    assert got.shape == rows.shape and got[:, 22:].tobytes() == rows[:, 22:].tobytes()
    assert got[:, :14].tobytes() == rows[:, :14].tobytes() and got[:, 15:].tobytes() == rows[:, 15:].tobytes()      # only column 14 differs
    assert len(states) == 3 and all(s.shape == (4, 6) for s in states)
    assert [h.tolist() for h in sim.body_hits] == [h.tolist() for h in plain.body_hits]
    for k, st in enumerate(states):
        want = CO.box_cells_clearance_numpy(CO.body_boxes(st, body), field.occupied, field.box, D)
        assert np.array_equal(sim.body_clearance[k], want["distance"]) and np.array_equal(sim.body_hits[k], want["hit"])
        assert got[k, 14] == _walk_minimum(want["distance"], want["hit"], D)
    assert got[0, 14] == D and abs(got[1, 14] - 0.025) < 1e-6 and got[2, 14] == 0.0


def test_exact_clearance_against_a_cpu_world():
    grid = CO.reference_box()
    lo = np.asarray(grid.start) + np.array([COLUMN[0], COLUMN[1], 0]) / grid.granularity
    hi = np.asarray(grid.start) + np.array([COLUMN[0] + 1, COLUMN[1] + 1, grid.shape[2]]) / grid.granularity
    v, f, _ = RC.cube()
    world = WO.MeshWorld((lo + v.astype(np.float64) * (hi - lo)).astype(np.float32), f, frame="world")
    sim = _stub_sim(sdf=_column_field(), world=world, body=CO.BodyBox.planner(), exact=True, clearance=0.25)
    got = sim.run(0)
    assert got[:, 22].tolist() == [0.0, 0.0, 1.0] and got[0, 14] == 0.25 and abs(got[1, 14] - 0.025) < 1e-6 and got[2, 14] == 0.0


def test_clearance_keyword_refusals():
    field, body = _column_field(), CO.BodyBox.planner()
    with pytest.raises(ValueError, match="body="):
        _stub_sim(sdf=field, clearance=0.25)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="clearance"):
            _stub_sim(sdf=field, body=body, clearance=bad)
    for fn, args in ((RO.run_rollout, (None, None, 8, 8, 1, 1)), (RO.run_validation, (RO.STRESS_MONTE_CARLO, None, None, 8, 8, 1, 1)),
                     (CE.run_cem, (None, None, 8, 8, 1))):
        with pytest.raises(ValueError, match="body="):
            fn(*args, sdf=field, clearance=0.25)


# ------------------------------------------------------------------------------------------------------------- the Cross Entropy Method
class _Flat:
    """a proposal whose every step has the log-probability 0: both trajectories get the same reward"""

    def log_prob(self, k, noise):
        return torch.zeros((), dtype=torch.float32)


def _cem_rows(clearance):
    """two constructed trajectories as CEM rows: the straight flight past test_body_cpu's column, pushed away from it along -y at step
    0 -- simulation 0 by 4 cm with the body square to the axes, simulation 1 by 4.5 cm with the body turned by 45 degrees about z, so
    that its corner reaches 7.07 cm where the square body reaches 5"""
    field = _column_field()

    class Sim(CE.CEMSimulator):
        def observe(self, pose):
            return 0.25

        def begin(self, sim):
            noises = torch.zeros(4, 12)
            noises[0, 1] = -0.04 if sim == 0 else -0.045
            noises[0, 8] = 0.0 if sim == 0 else float(np.pi / 4)
            self.q = type("Q", (_Flat,), {"sample": lambda self_, s: noises})()
            super().begin(sim)

    rows = []
    for s in range(2):
        sim = Sim(None, None, 8, 8, 4, sdf=field, body=CO.BodyBox.planner(), clearance=clearance, p=_Flat(), q=None, population=0)
        rows.append(sim.run(s))
    return np.concatenate(rows)


def test_cem_ranks_by_the_body_s_gap():
    """the tilted body passes nearer (its corner) while its centre passes further: under clearance= it is the riskier simulation and
    the first elite, under the centre's value it ranks second or ties"""
    centre, gap = _cem_rows(None), _cem_rows(0.25)
    assert centre.shape == (8, CE.CEM_ROW_WIDTH) and not centre[:, -2].any() and gap[:, -2:].tobytes() == centre[:, -2:].tobytes()
    r_centre, r_gap = CE.simulation_risks(centre, 0, 2), CE.simulation_risks(gap, 0, 2)
    print(f"risks by the centre's value {r_centre.tolist()}, by the body's gap {r_gap.tolist()}")
    assert 0.0 < r_gap[1] < r_gap[0] < 0.25 and CE.select_elite(r_gap, 1).tolist() == [1]
    assert r_centre[1] >= r_centre[0] and CE.select_elite(r_centre, 1).tolist() == [0]
