"""The state estimator's host pieces: the float32 numpy restatement of the keypoint detector (nav/sift_numpy.py, the specification
csrc/features.hip is held to), the cv2.dilate semantics of the interest mask, the reference's pixel enumeration, the failure branch,
and the Hessian argument of nav/estimator.py on a CPU stand-in whose render backward is opaque to autograd like the reference's
encoders."""
import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd.nav import sift_numpy as S
from nerfsafetyvalidation_amd.nav.estimator import Estimator, estimator_config, interest_pixels, state_to_pose


def _blob(H, W, cy, cx, s=3.0):
    y, x = np.mgrid[0:H, 0:W]
    v = 40 + 180 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return np.repeat(v.astype(np.uint8)[..., None], 3, 2)


def test_constant_image_has_no_keypoints():
    pts, mask, n = S.interest_mask(np.full((40, 56, 3), 120, np.uint8))
    assert n == 0 and pts.sum() == 0 and mask.sum() == 0 and pts.shape == (56, 40)


def test_blob_gives_a_keypoint_at_its_centre():
    kp = S.keypoints(_blob(48, 64, 20.0, 30.0))
    assert len(kp) >= 1
    d = np.hypot(kp[:, 0] - 30.0, kp[:, 1] - 20.0)
    assert d.min() < 1.0


def test_transposed_image_gives_the_transposed_set():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 72, 3), dtype=np.uint8)
    img[:, :, 1] = img[:, :, 0]
    img[:, :, 2] = img[:, :, 0]                       # grey: the transpose does not move the channel weights
    pts, _, n = S.interest_mask(img)
    ptsT, _, nT = S.interest_mask(np.ascontiguousarray(img.transpose(1, 0, 2)))
    assert n > 0 and n == nT
    assert np.array_equal(pts, ptsT.T)


def test_grey_weights_land_swapped():
    img = np.zeros((1, 3, 3), np.uint8)
    img[0, 0, 0] = img[0, 1, 1] = img[0, 2, 2] = 255
    assert S.gray(img).tolist() == [[29, 150, 76]]        # BGR2GRAY on an RGB array: R takes the blue weight


@pytest.mark.parametrize("k,it", [(5, 3), (5, 1), (3, 2), (4, 2), (5, 0)])
def test_dilation_against_brute_force(k, it):
    rng = np.random.default_rng(k * 10 + it)
    m = (rng.random((23, 31)) < 0.02).astype(np.uint8)
    m[0, 0] = m[22, 30] = m[0, 17] = 1                # borders
    want = m.copy()
    a = k // 2
    for _ in range(it):                               # cv2.dilate, one iteration at a time, outside pixels ignored
        nxt = np.zeros_like(want)
        for x in range(want.shape[0]):
            for y in range(want.shape[1]):
                win = want[max(x - a, 0):min(x - a + k, want.shape[0]), max(y - a, 0):min(y - a + k, want.shape[1])]
                nxt[x, y] = win.max()
        want = nxt
    assert np.array_equal(S.dilate(m, k, it), want)


def test_interest_pixels_follow_the_reference_enumeration():
    rng = np.random.default_rng(0)
    n = 24
    mask = rng.random((n, n)) < 0.2
    coords = np.asarray(np.stack(np.meshgrid(np.linspace(0, n - 1, n), np.linspace(0, n - 1, n)), -1), dtype=int)   # :100
    assert np.array_equal(interest_pixels(mask), coords[mask])


# ---------------------------------------------------------------- the filter on a CPU stand-in
class _Opaque(torch.autograd.Function):
    """rgb = sigmoid(o . a + d . b) per ray, with a backward that carries no graph (as the reference's extension calls)"""

    @staticmethod
    def forward(ctx, o, d, a, b):
        ctx.save_for_backward(o, d, a, b)
        return torch.sigmoid(o @ a + d @ b)

    @staticmethod
    def backward(ctx, g):
        o, d, a, b = ctx.saved_tensors
        with torch.no_grad():
            y = torch.sigmoid(o @ a + d @ b)
            gz = (g * y * (1 - y)).detach()
            return gz @ a.T.detach(), gz @ b.T.detach(), None, None


def _stub(H, W):
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(3, 3, generator=g), torch.randn(3, 3, generator=g)
    j, i = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="xy")
    dirs = torch.stack([(j - W / 2) / W, -(i - H / 2) / H, -torch.ones_like(i)], -1).reshape(-1, 3)

    def get_rays(pose, inds):
        d = dirs if inds is None else dirs[inds.long()]
        rd = d @ pose[0, :3, :3].T
        return {"rays_o": pose[0, :3, 3].expand(rd.shape)[None], "rays_d": rd[None]}

    def render(o, d):
        return {"image": _Opaque.apply(o.reshape(-1, 3), d.reshape(-1, 3), a, b)[None]}
    return get_rays, render


class _Agent:
    @staticmethod
    def drone_dynamics(x, action):
        from nerfsafetyvalidation_amd.rollout import drone_dynamics
        return drone_dynamics(x, action, 0.1)


class _StubEstimator(Estimator):
    keypoint_count = 5

    def interest_regions(self, img):
        m = np.zeros((img.shape[1], img.shape[0]), bool)
        m[3:9, 2:7] = True
        return m, self.keypoint_count


def _estimator(n_iter=6, count=5):
    get_rays, render = _stub(12, 12)
    start = torch.tensor([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.05, -0.1, 0.2, 0.0, 0.0, 0.0])
    cfg = estimator_config("cpu", N_iter=n_iter, batch_size=16)
    e = _StubEstimator(cfg, _Agent(), start, get_rays_fn=get_rays, render_fn=render, seed=4)
    e.keypoint_count = count
    return e


def test_failure_branch_keeps_the_previous_covariance():
    e = _estimator()
    e.sig = 2.0 * torch.eye(12)
    img = np.zeros((12, 12, 3), np.uint8)
    action = torch.tensor([10.0, 0.0, 0.01, 0.0])
    e.keypoint_count = 0
    want = _Agent.drone_dynamics(e.xt, action)
    est = e.estimate_state(img, None, action)
    assert not e.success and e.losses == [] and e.states == []
    assert torch.equal(est, want)
    assert torch.equal(torch.tensor(e.covariance), 2.0 * torch.eye(12))      # not sig_prop


def test_hessian_matches_double_differentiation_of_the_opaque_render():
    e = _estimator()
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)
    action = torch.tensor([10.0, 0.0, 0.01, 0.0])
    est = e.estimate_state(img, None, action)
    assert e.success and len(e.losses) == 6 and len(e.states) == 6
    assert torch.isfinite(est).all()
    # the reference's recipe: hessian of measurement_fn itself, through the opaque backward
    xt_prev = torch.tensor(e.states[0]) - 1e-6
    A = torch.autograd.functional.jacobian(lambda x: _Agent.drone_dynamics(x, action), _Agent.drone_dynamics(
        torch.tensor([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.05, -0.1, 0.2, 0.0, 0.0, 0.0]), action))
    sig_prop = A @ torch.eye(12) @ A.T + torch.eye(12)
    want = torch.autograd.functional.hessian(lambda x: e.measurement_fn(x, xt_prev, sig_prop, e.target, e.batch), est)
    got = e.measurement_hessian(est, sig_prop)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), (got - want).abs().max()
    inv = torch.inverse(sig_prop)
    off = (got - (inv + inv.T)).clone()
    off[6:9, 6:9] = 0
    assert off.abs().max() == 0                        # the render term lives in the rotation block only
    assert (got - (inv + inv.T))[6:9, 6:9].abs().max() > 0
    assert torch.allclose(torch.tensor(e.covariance), torch.inverse(got), rtol=1e-5, atol=1e-6)


def test_pixel_draws_follow_the_seeded_legacy_stream():
    e = _estimator(n_iter=3)
    img = np.full((12, 12, 3), 90, np.uint8)
    e.estimate_state(img, None, torch.tensor([10.0, 0.0, 0.0, 0.0]))
    region = interest_pixels(e.interest_regions(img)[0])
    np.random.seed(4)                                  # seed_everything(seed) in NerfSimulator.reset
    for _ in range(3):
        last = region[np.random.choice(region.shape[0], size=min(16, region.shape[0]), replace=False)]
    assert np.array_equal(e.batch, last)


def test_state_to_pose_is_the_rollout_camera():
    from nerfsafetyvalidation_amd.rollout import camera_pose
    s = torch.tensor([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.05, -0.1, 0.2, 0.0, 0.0, 0.0])
    assert torch.allclose(state_to_pose(s), camera_pose(s), atol=1e-6)


# ---------------------------------------------------------------- the reference's own run (tests/golden/estimator.npz)
@pytest.fixture(scope="module")
def efx():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator.npz"), allow_pickle=False)


def test_reference_hessian_has_a_render_term_only_in_the_rotation_block(efx):
    """the claim behind Estimator.measurement_hessian, on the reference's own numbers: H - (inv(sig) + inv(sig)^T) vanishes outside
    [6:9, 6:9] and not inside"""
    for i in range(2):
        inv = torch.inverse(torch.from_numpy(efx[f"sig_prop{i}"])).numpy()
        d = efx[f"hessian{i}"] - (inv + inv.T)
        assert np.abs(d[6:9, 6:9]).max() > 1e-4
        d[6:9, 6:9] = 0
        assert np.abs(d).max() == 0
        assert np.allclose(np.linalg.inv(efx[f"hessian{i}"].astype(np.float64)), efx[f"sig{i}"], rtol=1e-4, atol=1e-6)


def test_reference_failure_step_keeps_sig_and_propagates(efx):
    from nerfsafetyvalidation_amd.rollout import drone_dynamics
    assert np.array_equal(efx["sig2"], efx["sig1"])
    assert efx["losses2"].size == 0 and efx["states2"].size == 0
    want = drone_dynamics(torch.from_numpy(efx["state1"]), torch.from_numpy(efx["action2"]), float(efx["dt"])).numpy()
    assert np.allclose(efx["state2"], want, atol=1e-6)


def test_hessian_formula_reproduces_the_reference_hessian(efx):
    """inverse(sig) + inverse(sig)^T + d^2/ds^2 <G, state_to_pose(s)>, with G the reference's own first-order pose gradient, gives the
    Hessian the reference's torch.autograd.functional.hessian returned (to float32 rounding)"""
    for i in range(2):
        G = torch.from_numpy(efx[f"grad_pose{i}"])
        xt = torch.from_numpy(efx[f"state{i}"])
        inv = torch.inverse(torch.from_numpy(efx[f"sig_prop{i}"]))
        got = (inv + inv.T) + torch.autograd.functional.hessian(lambda s: (G * state_to_pose(s)).sum(), xt)
        want = efx[f"hessian{i}"]
        assert np.abs(got.numpy() - want).max() <= 1e-6 * np.abs(want).max()
