"""The state estimator on the MI355X: the HIP keypoint detector (csrc/features.hip) against its float32 numpy restatement
(nav/sift_numpy.py) bit for bit -- every Gaussian and DoG layer, the point and interest masks, the keypoint count -- on rendered,
blob and noise frames, square and not; and the rollout whose planner replans from the estimate."""
import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd.nav import features as FE
from nerfsafetyvalidation_amd.nav import sift_numpy as S

pytestmark = pytest.mark.gpu


def _blobs(H, W, seed):
    return S.blob_frame(H, W, seed)


def _rendered(H, W, pose_index, device):
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    rays = get_rays(torch.from_numpy(sc.poses[pose_index:pose_index + 1]).float().to(device), sc.intrinsics, H, W)
    with torch.no_grad():
        out = model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1, perturb=False, num_steps=64, upsample_steps=0)
    img = torch.squeeze(out["image"]).float().cpu().numpy().reshape(H, W, 3)
    img *= 255
    return img.astype(np.uint8)


def _check(img):
    got = FE.sift_interest_mask(img, 5, 3, return_pyramid=True)
    torch.cuda.synchronize()
    want = S.pyramid(img)
    assert len(got["pyramid"]) == len(want)
    for o, ((g, d), (wg, wd)) in enumerate(zip(got["pyramid"], want)):
        assert np.array_equal(g.cpu().numpy(), wg), f"octave {o}: Gaussian layers differ"
        assert np.array_equal(d.cpu().numpy(), wd), f"octave {o}: DoG layers differ"
    pts, mask, n = S.interest_mask(img, 5, 3)
    assert np.array_equal(got["points"].cpu().numpy(), pts)
    assert np.array_equal(got["mask"].cpu().numpy(), mask)
    assert int(got["count"].item()) == n
    return n


@pytest.mark.parametrize("H,W,seed", [(48, 64, 0), (96, 80, 1), (64, 64, 2)])
def test_detector_matches_the_restatement_on_blobs(device, H, W, seed):
    assert _check(_blobs(H, W, seed)) > 0


@pytest.mark.parametrize("H,W", [(40, 56), (128, 128)])
def test_detector_matches_the_restatement_on_noise(device, H, W):
    rng = np.random.default_rng(H + W)
    assert _check(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) > 0


@pytest.mark.parametrize("H,W", [(64, 64), (96, 128), (800, 800)])
def test_detector_matches_the_restatement_on_rendered_frames(device, H, W):
    _check(_rendered(H, W, 7, device))


def test_detector_edge_cases(device):
    flat = np.full((32, 48, 3), 200, np.uint8)
    assert _check(flat) == 0
    xy, extras = FE.find_POI(flat)
    assert xy.shape == (0,) and extras["features"] is None
    img = _blobs(48, 64, 0)
    xy, _ = FE.find_POI(img)
    pts, _, _ = S.interest_mask(img, 5, 0)
    assert np.array_equal(xy, np.argwhere(pts))
    with pytest.raises(ValueError):
        FE.sift_interest_mask(np.zeros((4, 40, 3), np.uint8))


def test_rollout_replans_from_the_estimate(device):
    """2 simulations x 3 steps of 64^2 frames with planner and estimator: the planner's update_state gets the estimate (not the true
    state), the rows keep ROW_WIDTH, one or two simulations in flight give the same rows and estimates."""
    import os
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd import scene as SC
    from nerfsafetyvalidation_amd.nav.estimator import estimator_config
    from test_planner_gpu import _net          # the planner fixture's network: a map A* can plan through
    H = W = 64
    model = _net(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner.npz")), device)

    class sc:
        intrinsics = SC.intrinsics(H, W)
    kw = dict(num_steps=64, upsample_steps=0, max_ray_batch=4096)
    pcfg = RO.planner_config(device, epochs_init=30, epochs_update=10)
    ecfg = estimator_config(device, N_iter=10, batch_size=256)
    seen = {}
    blob_sensor = False

    class Sim(RO.RolloutSimulator):
        def run(self, sim):
            self._sim = sim
            seen[sim] = []
            rows = super().run(sim)
            seen[sim] = (seen[sim], np.stack(self.estimates), list(self.estimate_success), np.stack(self.covariances))
            return rows

        def observe(self, pose):
            sigma = super().observe(pose)
            if self.estimator is not None and blob_sensor:     # the fixture map renders no keypoint: feed frames that have some
                self.sensor_image = S.blob_frame(H, W, 10 * self._sim + len(self.poses))
            return sigma

        def replan(self, k, state):
            real = self.planner.update_state

            def spy(state_est):
                seen[self._sim].append((state.numpy().copy(), state_est.detach().cpu().numpy().copy()))
                return real(state_est)
            self.planner.update_state = spy
            try:
                return super().replan(k, state)
            finally:
                self.planner.update_state = real

    def two_runs():
        rows1, _ = RO.run_rollout(model, sc.intrinsics, H, W, 2, 3, seed=5, in_flight=1, render_kwargs=kw, autocast=False,
                                  planner_cfg=pcfg, estimator_cfg=ecfg)
        seen1 = dict(seen)
        rows2, _ = RO.run_rollout(model, sc.intrinsics, H, W, 2, 3, seed=5, in_flight=2, render_kwargs=kw, autocast=False,
                                  planner_cfg=pcfg, estimator_cfg=ecfg)
        return rows1, seen1, rows2, dict(seen)

    RO.RolloutSimulator, keep = Sim, RO.RolloutSimulator
    try:
        blob_sensor = False
        rendered = two_runs()
        blob_sensor = True
        fitted = two_runs()
    finally:
        RO.RolloutSimulator = keep
    for (rows1, seen1, rows2, seen2), flag in ((rendered, False), (fitted, True)):
        assert rows1.shape == (6, RO.ROW_WIDTH) and np.isfinite(rows1).all()
        assert np.array_equal(rows1, rows2)
        for sim in (0, 1):
            calls, est, ok, cov = seen1[sim]
            assert ok == [flag] * 3                    # the fixture map's frames: failure branch; blob frames: the fit runs
            assert len(calls) == 3 and est.shape == (3, 12) and cov.shape == (3, 12, 12) and np.isfinite(est).all()
            for (true, fed), e in zip(calls, est):
                want = torch.cat([torch.from_numpy(e)[:6], RO.vec_to_rot_matrix(torch.from_numpy(e)[6:9]).reshape(-1), torch.from_numpy(e)[9:]])
                assert np.allclose(fed, want.numpy(), atol=1e-6)          # the planner gets the estimate ...
                assert not np.allclose(fed[:3], true[:3], atol=1e-7)      # ... not the true state
            assert np.array_equal(est, seen2[sim][1]) and ok == seen2[sim][2] and np.array_equal(cov, seen2[sim][3])


def test_estimate_state_on_a_blob_frame(device):
    """the success path on the GPU: a synthetic 64^2 blob frame (not a render) is the sensor image of the synthetic scene's model; the fit runs,
    the Hessian's render term sits in the rotation block only, sig = its inverse, and a second estimator gives the same numbers"""
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.nav.estimator import Estimator, estimator_config
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    H = W = 64
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    model.requires_grad_(False)
    kw = dict(staged=True, bg_color=1.0, perturb=False, num_steps=64, upsample_steps=0)
    img = _blobs(H, W, 2)          # (the synthetic scene's smooth 64^2 renders can hold no keypoint at all: the failure branch)
    pose = torch.from_numpy(sc.poses[7]).float()
    state = torch.zeros(12)
    state[:3] = torch.linalg.solve(torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), pose[:3, 3])

    class Agent:
        @staticmethod
        def drone_dynamics(x, action):
            return RO.drone_dynamics(x, action, 0.1)

    def make():
        return Estimator(estimator_config(device, N_iter=8, batch_size=128), Agent(), state.clone(), seed=2,
                         get_rays_fn=lambda p, inds: get_rays(p.to(device), sc.intrinsics, H, W, inds=inds),
                         render_fn=lambda o, d: model.render(o, d, **kw))
    action = torch.tensor([10.0, 0.0, 0.0, 0.0])
    runs = []
    for _ in range(2):
        e = make()
        est = e.estimate_state(img, None, action)
        assert e.success and e.keypoints > 0 and len(e.losses) == 8 and np.isfinite(e.losses).all()
        runs.append((est.numpy(), np.asarray(e.covariance), e.hessian.cpu().numpy(), list(e.losses)))
    est, cov, hess, losses = runs[0]
    assert np.isfinite(est).all() and np.isfinite(cov).all()
    x1 = Agent.drone_dynamics(state, action)
    A = torch.autograd.functional.jacobian(lambda x: Agent.drone_dynamics(x, action), x1)
    inv = torch.inverse(A @ A.T + torch.eye(12)).to(device)
    quad = (inv + inv.T).cpu().numpy()
    off = hess - quad
    assert np.abs(off[6:9, 6:9]).max() > 0
    off[6:9, 6:9] = 0
    assert np.abs(off).max() <= 1e-6 * np.abs(quad).max()         # the render term lives in the rotation block only
    assert np.allclose(np.linalg.inv(hess.astype(np.float64)), cov, rtol=1e-3, atol=1e-5)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    print("estimate", est, "losses", losses[0], losses[-1], "keypoints", e.keypoints)


def test_estimate_state_against_the_reference_fixture(device):
    """tests/golden/estimator.npz (make_golden_estimator.py: the reference's Estimator on CPU, keypoints given): three
    estimate_state steps on one estimator -- the pixel batches exactly; the pose gradient and the Hessian at the reference's estimate;
    per-iteration losses and states, final states and sig within the drift of a GPU render (tolerances about twice the observed)"""
    import os
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd import scene as SC
    from nerfsafetyvalidation_amd.nav.estimator import Estimator, estimator_config, state_to_pose
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator.npz"), allow_pickle=False)
    net = NeRFNetwork(encoding="hashgrid", bound=int(f["bound"]), cuda_ray=False, density_scale=float(f["density_scale"]), min_near=0.2,
                      density_thresh=0.01, bg_radius=-1)
    g = torch.Generator().manual_seed(int(f["table_seed"]))
    net.encoder.embeddings.data.copy_((torch.rand(net.encoder.embeddings.shape, generator=g) - 0.5).half().float())
    for i, l in enumerate(net.sigma_net):
        l.weight.data.copy_(torch.from_numpy(f[f"sigma{i}"]))
    for i, l in enumerate(net.color_net):
        l.weight.data.copy_(torch.from_numpy(f[f"color{i}"]))
    net = net.to(device).eval()
    net.requires_grad_(False)
    H, W, dt = int(f["H"]), int(f["W"]), float(f["dt"])
    kw = dict(staged=True, bg_color=1.0, perturb=False, num_steps=int(f["num_steps"]), upsample_steps=0)
    step = {"i": 0}

    class Agent:
        @staticmethod
        def drone_dynamics(x, action):
            return RO.drone_dynamics(x, action, dt)

    class Given(Estimator):
        def interest_regions(self, img):          # the fixture's keypoints (no OpenCV anywhere), truncated and dilated as :101-106
            kp = f[f"keypoints{step['i']}"].astype(np.int64)
            pts = np.zeros((img.shape[1], img.shape[0]), np.uint8)
            pts[kp[:, 0], kp[:, 1]] = 1
            return S.dilate(pts, self.kernel_size, self.dil_iter).astype(bool), len(kp)

    cfg = estimator_config(device, N_iter=int(f["n_iter"]), batch_size=int(f["batch_size"]))
    e = Given(cfg, Agent(), torch.from_numpy(f["start_state"]).clone(), seed=int(f["seed"]),
              get_rays_fn=lambda p, inds: get_rays(p.to(device), SC.intrinsics(H, W), H, W, inds=inds),
              render_fn=lambda o, d: net.render(o, d, **kw))
    err = {}
    for i in range(3):
        step["i"] = i
        est = e.estimate_state(f[f"image{i}"], None, torch.from_numpy(f[f"action{i}"])).numpy()
        sig = np.asarray(e.covariance, np.float32)
        err[f"state{i}"] = np.abs(est - f[f"state{i}"]).max()
        err[f"sig{i}"] = np.abs(sig - f[f"sig{i}"]).max() / np.abs(f[f"sig{i}"]).max()
        if i < 2:
            assert e.success
            assert np.array_equal(e.batch, f[f"batch{i}"])
            err[f"losses{i}"] = (np.abs(np.asarray(e.losses) - f[f"losses{i}"]) / np.abs(f[f"losses{i}"])).max()
            err[f"states{i}"] = np.abs(np.asarray(e.states, np.float32) - f[f"states{i}"]).max()
            pose = state_to_pose(torch.from_numpy(f[f"state{i}"]).to(device)).detach().requires_grad_(True)
            Gp, = torch.autograd.grad(e._render_loss(pose, e.target, f[f"batch{i}"]), pose)
            err[f"grad_pose{i}"] = np.abs(Gp.cpu().numpy() - f[f"grad_pose{i}"]).max() / np.abs(f[f"grad_pose{i}"]).max()
            # the Hessian at the reference's own estimate: the arithmetic of measurement_hessian against hessian(measurement_fn)
            h_ref_state = e.measurement_hessian(torch.from_numpy(f[f"state{i}"]).to(device), torch.from_numpy(f[f"sig_prop{i}"]).to(device))
            err[f"hessian_at_ref{i}"] = np.abs(h_ref_state.cpu().numpy() - f[f"hessian{i}"]).max() / np.abs(f[f"hessian{i}"]).max()
        else:
            assert not e.success and e.losses == []
    print({k: float(v) for k, v in err.items()})
    # step 0 starts from the reference's own inputs: last-bit drift only.  From step 1 on the start state and sig come from step 0's
    # estimate, and the render term of the Hessian changes fast with the state (1.6e-5 in the state moves it by ~30 % here; at the
    # reference's state it agrees to 1e-7), so steps 1-2 carry that difference through the Mahalanobis term
    tols = {"state0": 4e-5, "states0": 2e-6, "losses0": 2e-4, "grad_pose0": 4e-5, "hessian_at_ref0": 1e-6, "sig0": 2e-4,
            "state1": 2e-3, "states1": 2.5e-3, "losses1": 0.1, "grad_pose1": 1e-4, "hessian_at_ref1": 1e-6, "sig1": 1e-3,
            "state2": 2e-3, "sig2": 1e-3}
    for k, v in err.items():
        tol = tols[k]
        assert v <= tol, (k, v)
