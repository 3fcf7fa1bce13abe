"""The failure replay on the GPU (nerfsafetyvalidation_amd/replay.py) at the shapes of tests/test_world_gpu.py: a Monte-Carlo and a CEM
stress run replayed in the mesh's world with its own collision field and one failure view per simulation; and a replay with the
planner and the estimator, whose only sensor is the world."""
import os

import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import cem as CE
from nerfsafetyvalidation_amd import collision as CO
from nerfsafetyvalidation_amd import replay as RP
from nerfsafetyvalidation_amd import rollout as RO
from nerfsafetyvalidation_amd import scene as SC
from nerfsafetyvalidation_amd import world as WO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def henge(device):
    v, f, c = SC.henge_mesh(24)
    return WO.MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device))


def recount(stress, replayed, cem):
    """the eight counts from the two row arrays alone: per simulation, step by step"""
    off = 1 if cem else 0
    key = lambda rows: [tuple(r) for r in rows[:, :1 + off].astype(int)]
    step, traj = dict(tp=0, tn=0, fp=0, fn=0), dict(tp=0, tn=0, fp=0, fn=0)
    for sim in dict.fromkeys(key(stress)):
        nerf = stress[[k == sim for k in key(stress)]]
        true = replayed[[k == sim for k in key(replayed)]]
        assert 1 <= len(true) <= len(nerf)
        for k in range(len(true)):
            w, n = bool(true[k, -2]), bool(nerf[k, -2])
            step["tp" if w and n else "fn" if w else "fp" if n else "tn"] += 1
        if true[-1, -2]:
            step["fn"] += len(nerf) - len(true)
        else:
            assert len(true) == len(nerf)
        w, n = bool(true[:, -2].any()), bool(nerf[-1, -1])
        assert true[-1, -1] == w
        traj["tp" if w and n else "fn" if w else "fp" if n else "tn"] += 1
    return step, traj


def check_counts(res, stress, cem, n_sims):
    step, traj = recount(stress, res.rows, cem)
    assert vars(res.counts.step) == step and vars(res.counts.traj) == traj
    assert res.counts.step.total == stress.shape[0] and res.counts.traj.total == n_sims


def test_monte_carlo_and_cem_rows_replayed_in_the_world(device, henge, tmp_path):
    from PIL import Image
    H = W = 32
    sc = SC.StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    kw = dict(num_steps=32, upsample_steps=0, max_ray_batch=1024)
    sdf = CO.SignedDistanceField.from_occupancy(CO.occupancy_from_fn(CO.henge_fn, CO.reference_box()), CO.reference_box())
    stress, _ = RO.run_rollout(model, sc.intrinsics, H, W, 2, 2, seed=3, in_flight=2, render_kwargs=kw, sdf=sdf)
    assert stress.shape[1] == RO.ROW_WIDTH
    res = RP.run_replay(stress, model, sc.intrinsics, H, W, world=henge, sdf="world", seed=3, in_flight=2, render_kwargs=kw, views=tmp_path / "mc",
                        steps=2)
    assert res.rows.ndim == 2 and res.rows.shape[1] == RP.REPLAY_ROW_WIDTH and 2 <= res.rows.shape[0] <= stress.shape[0]
    assert np.isfinite(res.rows).all()                                   # the replay row has no sigma column: nothing is NaN
    assert res.rows[:, 0].tolist() == sorted(res.rows[:, 0].tolist()) and set(res.rows[:, 0]) == {0.0, 1.0}
    for r in res.rows:                                                   # every replayed step carries its recorded noise
        assert np.array_equal(r[2:14], stress[(stress[:, 0] == r[0]) & (stress[:, 1] == r[1])][0, 2:14])
    check_counts(res, stress, False, 2)
    # the same collision check as the stress run's, with the same noise: only the field differs (no planner, no estimator)
    same_world = RP.run_replay(stress, None, sc.intrinsics, H, W, world=henge, sdf=sdf, seed=3, in_flight=1, steps=2)
    assert same_world.rows[:, 14:18].tobytes() == stress[:, 14:18].tobytes() and same_world.counts.step.fp == same_world.counts.step.fn == 0
    # one view per simulation, of the frame's size, and not the world's plain frame
    pose, K = RP.overview_camera(H, W)
    plain = henge.render(pose, K, H, W)["image_u8"].cpu().numpy()
    assert len(res.views) == 2 and res.plans == [[], []]
    for path, (s, k, pop) in zip(res.views, res.view_calls):
        assert os.path.basename(path) == f"failure_{s}_{k}.png" and pop is None
        img = np.asarray(Image.open(path))
        assert img.shape == (H, W, 3) and img.dtype == np.uint8 and not np.array_equal(img, plain)
    # CEM rows go through the same call: width 23, the population first
    cem_rows, _, _ = CE.run_cem(model, sc.intrinsics, H, W, 2, m=2, m_elite=1, kmax=1, seed=11, sdf=sdf, in_flight=2, render_kwargs=kw)
    cres = RP.run_replay(cem_rows, model, sc.intrinsics, H, W, world=henge, sdf="world", seed=11, in_flight=2, render_kwargs=kw,
                         views=tmp_path / "cem", steps=2)
    assert cres.rows.shape[1] == RP.REPLAY_CEM_ROW_WIDTH and (cres.rows[:, 0] == 0).all() and set(cres.rows[:, 1]) == {0.0, 1.0}
    assert np.isfinite(cres.rows).all()
    check_counts(cres, cem_rows, True, 2)
    assert [os.path.basename(p) for p in cres.views] == [f"failure_0_{s}_{k}.png" for s, k, _ in cres.view_calls]
    assert all(os.path.exists(p) for p in cres.views)


def test_planner_and_estimator_sense_only_the_world(device, henge, monkeypatch):
    from nerfsafetyvalidation_amd.nav.estimator import estimator_config
    from test_planner_gpu import _net
    H = W = 64
    model = _net(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner.npz")), device)
    K = SC.intrinsics(H, W)
    kw = dict(num_steps=64, upsample_steps=0, max_ray_batch=4096)
    pcfg = RO.planner_config(device, epochs_init=30, epochs_update=10)
    ecfg = estimator_config(device, N_iter=10, batch_size=256)
    gen = torch.Generator().manual_seed(5)
    stress = np.zeros((2, RO.ROW_WIDTH))                                 # one recorded simulation of two steps, nothing flagged
    stress[:, 1] = (0, 1)
    stress[:, 2:14] = torch.normal(torch.zeros(2, 12), torch.tensor(RO.ENV["mpc_noise_std"]).expand(2, 12), generator=gen).numpy()
    sims = []

    class Spy(RP.ReplaySimulator):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.seen = []
            sims.append(self)

        def estimate(self, k, state):
            self.seen.append((self.sensor_image.copy(), self.poses[-1].clone(), self.world_image.copy()))
            return super().estimate(k, state)

    monkeypatch.setattr(RP, "ReplaySimulator", Spy)
    res = RP.run_replay(stress, model, K, H, W, world=henge, sdf="world", seed=5, planner_cfg=pcfg, estimator_cfg=ecfg, render_kwargs=kw,
                        in_flight=1, autocast=False)
    assert len(sims) == 1 and res.rows.shape[1] == RP.REPLAY_ROW_WIDTH and 1 <= res.rows.shape[0] <= 2 and np.isfinite(res.rows).all()
    sim, steps = sims[0], res.rows.shape[0]
    assert len(sim.seen) == steps and sim.frames == 0                    # observe issued no NeRF render of its own
    for sensor, pose, kept in sim.seen:
        want = henge.render(pose, K, H, W)["image_u8"].cpu().numpy()
        assert sensor.dtype == np.uint8 and sensor.shape == (H, W, 3) and np.array_equal(sensor, want) and np.array_equal(kept, want)
    assert len(sim.plans) == 1 + steps and len(res.plans) == 1 and res.plans[0] is sim.plans
    assert all(p.ndim == 2 and p.shape[1] == 3 and p.shape[0] >= 2 and np.isfinite(p).all() for p in sim.plans)
    assert not np.array_equal(sim.plans[0], sim.plans[1])
    assert np.array_equal(res.rows[:, 2:14], stress[:steps, 2:14].astype(np.float32).astype(np.float64))
    check_counts(res, stress, False, 1)
    view = RP.failure_view(henge, res.rows, sim.plans, H=96, W=96)        # the plans as tubes: 1 + steps polylines, then the cubes
    over = view["overlay_prim"].cpu().numpy()
    assert (over >= 0).sum() > 20 and view["image_u8"].shape == (96, 96, 3)
