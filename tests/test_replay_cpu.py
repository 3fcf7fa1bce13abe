"""The failure replay's loop and counts (nerfsafetyvalidation_amd/replay.py) on the CPU: against the rows, counts and view calls the
reference's own replay_MC() / replay_CEM() produced (tests/golden/replay.npz, made by make_golden_replay.py), against the simulator
that wrote the rows, and on hand-built cases for every counting branch.  No GPU: the world is a CPU MeshWorld (numpy ray caster) and
`collision` is overridden, as tests/test_rollout.py does it."""
import os

import numpy as np
import pytest
import torch

import raycast_cases as RC
from nerfsafetyvalidation_amd import cem as CE
from nerfsafetyvalidation_amd import replay as RP
from nerfsafetyvalidation_amd import rollout as RO
from nerfsafetyvalidation_amd import world as WO
from nerfsafetyvalidation_amd.uncertainty.evaluation import metrics as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = np.array([8.0, 8.0, 4.0, 4.0])


@pytest.fixture(scope="module")
def world():
    v, f, _ = RC.mesh("cube")
    return WO.MeshWorld(v, f)


def sphere_sim(centre, radius, base=RP.ReplaySimulator):
    centre = np.asarray(centre, np.float64)

    class Sim(base):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.n_interp = 1                                  # the fixture's stub looks at the new state only

        def collision(self, xyz):
            v = float(np.linalg.norm(np.asarray(xyz, np.float64) - centre) - radius)
            return v < 0, v

    return Sim


def replay(monkeypatch, sim_cls, rows, world, **kw):
    monkeypatch.setattr(RP, "ReplaySimulator", sim_cls)
    kw.setdefault("steps", 4)
    return RP.run_replay(rows, None, K, 8, 8, world=world, sdf=None, in_flight=1, autocast=False, **kw)


@pytest.mark.parametrize("kind", ["mc", "cem"])
def test_replay_reproduces_the_reference(kind, monkeypatch, world):
    z = np.load(os.path.join(G, "replay.npz"))
    want, counts, calls = z[kind + "_replay"], z[kind + "_counts"], z[kind + "_calls"]
    res = replay(monkeypatch, sphere_sim(z["centre_b"], float(z["radius_b"])), z[kind + "_input"], world, steps=int(z["steps"]))
    off = 1 if kind == "cem" else 0
    assert res.rows.shape == want.shape == (want.shape[0], RP.REPLAY_CEM_ROW_WIDTH if off else RP.REPLAY_ROW_WIDTH)
    np.testing.assert_array_equal(res.rows[:, :2 + off], want[:, :2 + off])                      # (population,) simulation, step
    np.testing.assert_allclose(res.rows[:, 2 + off:14 + off], want[:, 2 + off:14 + off], rtol=0, atol=2e-7)    # the noise (the CSV holds float32's digits)
    np.testing.assert_allclose(res.rows[:, 14 + off], want[:, 14 + off], rtol=0, atol=1e-6)      # the collision value: a distance of the position
    np.testing.assert_allclose(res.rows[:, 15 + off:18 + off], want[:, 15 + off:18 + off], rtol=0, atol=1e-6)  # position (test_rollout.py's tolerance)
    np.testing.assert_allclose(res.rows[:, 18 + off:20 + off], want[:, 18 + off:20 + off], rtol=1e-6, atol=1e-4)   # step / cumulative log-likelihood
    np.testing.assert_array_equal(res.rows[:, 20 + off:], want[:, 20 + off:])                    # collided, ever collided
    got = res.counts
    assert [got.step.tp, got.step.tn, got.step.fp, got.step.fn, got.traj.tp, got.traj.tn, got.traj.fp, got.traj.fn] == counts.tolist()
    assert all(c > 0 for c in counts[:4]) and got.step.total == z[kind + "_input"].shape[0] > res.rows.shape[0]
    assert [(s, k, -1 if p is None else p) for s, k, p in res.view_calls] == [tuple(c) for c in calls.tolist()]
    assert res.views == [] and np.array_equal(res.confusion_matrix("step"), [[counts[1], counts[3]], [counts[2], counts[0]]])


def test_replaying_in_the_world_that_wrote_the_rows_agrees_with_itself(monkeypatch, world):
    centre, radius, steps = [-0.0375, -0.614, 0.5875], 0.33, 4
    Stress = sphere_sim(centre, radius, RO.RolloutSimulator)

    class StressSim(Stress):
        def observe(self, pose):
            return 0.05

    rows = np.concatenate([StressSim(None, None, 8, 8, steps, seed=3).run(s) for s in range(6)])
    assert rows.shape[1] == RO.ROW_WIDTH and rows[:, -1].any() and not rows[:, -1].all()
    res = replay(monkeypatch, sphere_sim(centre, radius), rows, world, steps=steps, seed=3)
    assert res.rows.shape == (rows.shape[0], RP.REPLAY_ROW_WIDTH)
    assert res.rows[:, 14:18].tobytes() == rows[:, 14:18].tobytes()                              # value and position, bit for bit
    assert np.array_equal(res.rows[:, :14], rows[:, :14]) and np.array_equal(res.rows[:, -2:], rows[:, -2:])
    for kind, n in (("step", rows.shape[0]), ("traj", 6)):
        c = getattr(res.counts, kind)
        assert c.fp == 0 and c.fn == 0 and c.tp + c.tn == n and c.tp > 0 and c.tn > 0
    assert res.scores("step") == {"accuracy": 1.0, "precision": 1.0, "recall": 1.0, "f1": 1.0}


def stress_rows(flags, cem_population=None):
    """hand-built stress rows: flags[sim] = the NeRF's step verdicts of that simulation; zero noise"""
    out = []
    for s, fl in enumerate(flags):
        for k, f in enumerate(fl):
            row = np.zeros(RO.ROW_WIDTH if cem_population is None else CE.CEM_ROW_WIDTH)
            row[:2] = (s, k) if cem_population is None else (cem_population, s)
            if cem_population is not None:
                row[2] = k
            row[-2], row[-1] = f, any(fl)
            out.append(row)
    return np.asarray(out)


def table_sim(world_flags):
    """a ReplaySimulator whose world collides where world_flags[(population, sim)][step] says so"""
    class Sim(RP.ReplaySimulator):
        def run(self, sim):
            self._sim = sim
            return super().run(sim)

        def action(self, k, state):
            self._k = k
            return super().action(k, state)

        def collision(self, xyz):
            hit = bool(world_flags[(self.population, self._sim)][self._k])
            return hit, (0.0 if hit else 9999.0)

    return Sim


def cells(c):
    return (c.tp, c.tn, c.fp, c.fn)


def test_every_counting_branch_by_hand(monkeypatch, world):
    # sim 0: agree free, agree free, both collide on the LAST recorded step (0 remaining)          -> tp 1, tn 2;          traj tp
    # sim 1: the world collides at step 1 where the NeRF is free; two recorded steps remain, one flagged -> tn 1, fn 1 + 2;  traj fn... the NeRF's last column is True: tp
    # sim 2: the NeRF flags step 2 (its last), the world never collides                           -> tn 2, fp 1;          traj fp
    # sim 3: nobody collides                                                                      -> tn 3;                traj tn
    nerf = [[0, 0, 1], [0, 0, 0, 1], [0, 0, 1], [0, 0, 0]]
    truth = {(None, 0): [0, 0, 1], (None, 1): [0, 1, 0, 0], (None, 2): [0, 0, 0], (None, 3): [0, 0, 0]}
    rows = stress_rows(nerf)
    res = replay(monkeypatch, table_sim(truth), rows, world)
    assert cells(res.counts.step) == (1, 2 + 1 + 2 + 3, 1, 1 + 2) and res.counts.step.total == rows.shape[0] == 13
    assert cells(res.counts.traj) == (2, 1, 1, 0)
    assert [r.shape for r in np.split(res.rows, np.nonzero(np.diff(res.rows[:, 0]))[0] + 1)] == [(3, 22), (2, 22), (3, 22), (3, 22)]
    assert res.view_calls == [(0, 2, None), (1, 1, None), (2, 2, None), (3, 2, None)]
    assert res.rows[:, -1].tolist() == [1] * 3 + [1] * 2 + [0] * 6 and res.rows[:, -2].tolist() == [0, 0, 1, 0, 1] + [0] * 6
    # a world collision where the NeRF is free and recorded a trajectory without any collision: traj fn
    res = replay(monkeypatch, table_sim({(None, 0): [1, 0]}), stress_rows([[0, 0]]), world)
    assert cells(res.counts.step) == (0, 0, 0, 2) and cells(res.counts.traj) == (0, 0, 0, 1)
    # start skips the first simulations; counts= continues (and is not modified)
    before = RP.ReplayCounts(RP.ConfusionCounts(1, 2, 3, 4), RP.ConfusionCounts(5, 6, 7, 8))
    res = replay(monkeypatch, table_sim(truth), rows, world, start=2, counts=before)
    assert cells(res.counts.step) == (1, 2 + 2 + 3, 3 + 1, 4) and cells(res.counts.traj) == (5, 6 + 1, 7 + 1, 8)
    assert cells(before.step) == (1, 2, 3, 4) and cells(before.traj) == (5, 6, 7, 8) and res.view_calls == [(2, 2, None), (3, 2, None)]
    first = replay(monkeypatch, table_sim(truth), rows[rows[:, 0] < 2], world)
    rest = replay(monkeypatch, table_sim(truth), rows, world, start=2, counts=first.counts)
    whole = replay(monkeypatch, table_sim(truth), rows, world)
    assert cells(rest.counts.step) == cells(whole.counts.step) and cells(rest.counts.traj) == cells(whole.counts.traj)
    # CEM rows: the population in front; start_k skips populations, start skips the first simulations of EVERY population
    cem_rows = np.concatenate([stress_rows([[0, 1], [0, 0]], 0), stress_rows([[0, 0], [1]], 1)])
    truth = {(0, 0): [0, 0], (0, 1): [0, 1], (1, 0): [1, 0], (1, 1): [1]}
    res = replay(monkeypatch, table_sim(truth), cem_rows, world)
    assert res.rows.shape[1] == RP.REPLAY_CEM_ROW_WIDTH and res.rows[:, 0].tolist() == [0, 0, 0, 0, 1, 1]
    assert cells(res.counts.step) == (1, 2, 1, 1 + 1 + 1) and cells(res.counts.traj) == (1, 0, 1, 2)
    assert res.view_calls == [(0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)]
    assert replay(monkeypatch, table_sim(truth), cem_rows, world, start_k=1).view_calls == [(0, 0, 1), (1, 0, 1)]
    assert replay(monkeypatch, table_sim(truth), cem_rows, world, start=1).view_calls == [(1, 1, 0), (1, 0, 1)]
    direct = RP.ReplayCounts()
    assert RP.count_simulation(direct, [False, True], [True, False, True, True], True) and cells(direct.step) == (0, 0, 1, 3)


def test_matrix_labels_and_scores():
    c = RP.ReplayCounts(RP.ConfusionCounts(tp=3, tn=5, fp=2, fn=1), RP.ConfusionCounts(tp=1, tn=0, fp=0, fn=2))
    res = RP.ReplayResult(rows=np.zeros((0, 22)), counts=c)
    assert res.confusion_matrix("step").tolist() == [[5, 1], [2, 3]] and res.confusion_matrix("traj").tolist() == [[0, 2], [0, 1]]
    y_true, y_pred = res.labels("step")
    assert y_true.sum() == 4 and y_pred.sum() == 5 and len(y_true) == 11 and ((y_true == 1) & (y_pred == 1)).sum() == 3
    assert ((y_true == 0) & (y_pred == 1)).sum() == 2 and ((y_true == 1) & (y_pred == 0)).sum() == 1
    s = res.scores("step")
    assert s["accuracy"] == M.calculate_accuracy(y_true, y_pred) == 8 / 11 and s["precision"] == M.calculate_precision(y_true, y_pred) == 3 / 5
    assert s["recall"] == M.calculate_recall(y_true, y_pred) == 3 / 4 and s["f1"] == M.calculate_f1_score(y_true, y_pred)
    t = res.scores("traj")
    assert t["recall"] == 1 / 3 and t["precision"] == 1.0
    with pytest.raises(ValueError):
        res.confusion_matrix("frame")


def test_csv_in_and_out(tmp_path):
    path = tmp_path / "results.csv"
    path.write_text("0,0,0.5,True,False\n0,1,-2e-3,true,FALSE\n1,0,7,1,0\n1,1,0.25,0.0,1.0\n")
    got = RP.read_results_csv(path)
    assert got.tolist() == [[0, 0, 0.5, 1, 0], [0, 1, -2e-3, 1, 0], [1, 0, 7, 1, 0], [1, 1, 0.25, 0, 1]]
    rng = np.random.default_rng(0)
    for width, ints in ((RP.REPLAY_ROW_WIDTH, 2), (RP.REPLAY_CEM_ROW_WIDTH, 3)):
        rows = rng.normal(size=(5, width))
        rows[:, :ints] = rng.integers(0, 9, (5, ints))
        rows[:, -2:] = rng.integers(0, 2, (5, 2))
        out = tmp_path / f"replays{width}" / "collisionValuesReplay.csv"
        RP.write_replay_csv(RP.ReplayResult(rows=rows, counts=RP.ReplayCounts()), out)
        text = out.read_text().splitlines()
        assert text[0].split(",")[-1] in ("True", "False") and text[0].split(",")[0].isdigit()
        assert RP.read_results_csv(out).tobytes() == rows.tobytes()
    ragged = tmp_path / "ragged.csv"
    ragged.write_text("0,1,2\n0,1\n")
    with pytest.raises(ValueError):
        RP.read_results_csv(ragged)


def test_refused_inputs(world):
    rows = stress_rows([[0, 0]])
    for width in (RP.REPLAY_ROW_WIDTH, RO.ROW_WIDTH + 1, CE.CEM_ROW_WIDTH - 1):
        with pytest.raises(ValueError, match="width"):
            RP.run_replay(np.zeros((2, width)), None, K, 8, 8, world=world, sdf=None)
    with pytest.raises(ValueError, match="world"):
        RP.run_replay(rows, None, K, 8, 8, world=None)
    with pytest.raises(ValueError, match="MeshWorld"):
        RP.run_replay(rows, None, K, 8, 8, world=object(), sdf="world")           # sdf="world" without a mesh
    with pytest.raises(TypeError):
        RP.run_replay(rows, None, K, 8, 8)                                        # world is required
    with pytest.raises(ValueError, match="model"):
        RP.run_replay(rows, None, K, 8, 8, world=world, sdf=None, planner_cfg={"steps": 2})
    with pytest.raises(ValueError, match="position"):
        RP.run_replay(rows[:, :].copy() + np.eye(1, RO.ROW_WIDTH)[0] * 3, None, K, 8, 8, world=world, sdf=None)     # simulation 3 alone


def test_the_view_of_a_replayed_simulation_on_the_cpu(monkeypatch, world, tmp_path):
    """run_replay(views=): one PNG per simulation, named after the simulation and its last step, of the frame size; the picture
    differs from the world's plain render by the drawn trajectory"""
    from PIL import Image
    rows = stress_rows([[0, 0, 1], [0, 0]])
    res = replay(monkeypatch, table_sim({(None, 0): [0, 1, 0], (None, 1): [0, 0]}), rows, world, views=tmp_path / "views")
    assert [os.path.basename(p) for p in res.views] == ["failure_0_1.png", "failure_1_1.png"]
    pose, intr = RP.overview_camera(8, 8)
    plain = world.render(pose, intr, 8, 8)["image_u8"].numpy()
    for p in res.views:
        img = np.asarray(Image.open(p))
        assert img.shape == (8, 8, 3) and img.dtype == np.uint8
    v, f, _ = RC.mesh("cube")
    floor = WO.MeshWorld((v * np.float32([2.4, 0.1, 2.4]) - np.float32([1.2, 0.5, 1.2])).astype(np.float32), f)      # a slab under the flight
    view = RP.failure_view(floor, res.rows[res.rows[:, 0] == 0], H=160, W=160)         # (a 2 cm tube is two pixels wide at this size)
    over = view["overlay_prim"].numpy()
    assert (over >= 0).sum() >= 15 and set(np.unique(over).tolist()) >= {-1, 0, 1, 2, 3}              # the path's two capsules, both kinds of cube
    plain160 = floor.render(*RP.overview_camera(160, 160), 160, 160)
    assert (plain160["prim"].numpy() >= 0).mean() > 0.2 and np.array_equal(view["prim"].numpy(), plain160["prim"].numpy())
    assert np.array_equal(view["image_u8"].numpy()[over < 0], plain160["image_u8"].numpy()[over < 0])
    assert not np.array_equal(view["image_u8"].numpy(), plain160["image_u8"].numpy())
    assert plain.shape == (8, 8, 3)
