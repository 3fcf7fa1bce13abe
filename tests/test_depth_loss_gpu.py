"""Depth supervision's HIP kernels (csrc/depth_loss.hip, ngp_train_depth_targets) against the float64 helper of depth_cases.py, their
determinism, and the term's way through the renderer and the Trainer.

Tolerance of the packed operator, as in test_distortion_gpu.py: the yardstick is the float32 torch chain on the CPU (sigma -> alpha ->
cumprod -> w, cumsum -> t, the loss, autograd) against float64 on the same rays, computed here (depth_cases.torch_chain), never taken
from the kernel: the worst error over the rays, the loss and the parts relative to the ray's float64 value, gradients relative to the
ray's max |gradient|.  A wave scan adds in another order than cumsum: an error of the same size, not the same number, so the kernels
get 8 x that worst value.  Each test prints what it observed."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_cases as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 8.0
A, B = 0.7, 0.3


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.fixture(scope="module")
def fx():
    return DC.load()


@pytest.fixture(scope="module")
def cases(fx):
    return DC.make_targets(fx)


@pytest.fixture(scope="module")
def yardstick(fx, cases):
    """per (scale given?, a, b): (float64 result, worst float32-chain errors), computed once and shared"""
    cache = {}

    def get(with_scale, a, b):
        key = (with_scale, a, b)
        if key not in cache:
            scale = fx["scale"] if with_scale else None
            want = DC.packed64(fx, cases[0], scale, a=a, b=b)
            cache[key] = (want, DC.errors(fx, DC.torch_chain(fx, cases[0], scale, torch.float32, a=a, b=b), want))
        return cache[key]
    return get


def _run_packed(fx, target, device, with_scale, a, b, rays=None, margin=DC.MARGIN):
    from nerfsafetyvalidation_amd import raymarching
    sigmas = _t(fx["sigmas"], device).requires_grad_(True)
    table = _t(fx["rays"], device) if rays is None else rays
    loss, loss_rays, parts = raymarching.depth_rays_train(sigmas, _t(fx["deltas"], device), table, _t(target, device), margin,
                                                          _t(fx["scale"], device) if with_scale else None, a, b, return_rays=True)
    loss.backward()
    return loss.detach(), loss_rays, parts, sigmas.grad


def _as_result(fx, out):
    N = fx["rays"].shape[0]
    return dict(loss_rays=out[1].cpu().numpy().astype(np.float64), parts=out[2].cpu().numpy().astype(np.float64),
                grad_sigma=out[3].cpu().numpy().astype(np.float64) * N)


def _check_packed(fx, cases, yardstick, device, with_scale, a, b, tag):
    target, names = cases
    want, ref_err = yardstick(with_scale, a, b)
    out = _run_packed(fx, target, device, with_scale, a, b)
    got = _as_result(fx, out)
    err = DC.errors(fx, got, want)
    err_mean = abs(float(out[0]) - want["mean"]) / want["mean"]
    print(f"depth_rays_train [{tag}]: " + ", ".join(f"{k} {err[k]:.2e} (bound {SLACK * ref_err[k]:.2e})" for k in err) + f", mean {err_mean:.2e}")
    for k in err:
        assert err[k] <= SLACK * ref_err[k], k
    # the mean: non-negative terms each within the bound, added in double; then the 64-slot float butterflies and one rounding to float
    assert err_mean <= SLACK * ref_err["loss"] + 8 * 2.0 ** -24
    # exactly 0: rays without a measurement, the empty ray, the dropped ray; rows behind the stop, of those rays and of no ray
    slots = fx["rays"][:, 0]
    nothing = np.array([names[n] in DC.NO_MEASUREMENT or not DC.ray_rows(fx, n)[3] for n in range(len(names))])
    assert nothing.sum() >= 10 and (got["loss_rays"][slots[nothing]] == 0).all() and (got["parts"][slots[nothing]] == 0).all()
    written = want["live"].copy()
    for n in np.nonzero(nothing)[0]:
        written[DC.ray_rows(fx, n)[1]] = False
    assert (~fx["owned"]).sum() == 7 and (~written).sum() > 500 and (got["grad_sigma"][~written] == 0).all()
    assert (want["grad_sigma"][~written] == 0).all()
    return got, want


@pytest.mark.parametrize("tag", ["s", "1"])
def test_packed_operator_matches_float64(device, fx, cases, yardstick, tag):
    _check_packed(fx, cases, yardstick, device, tag == "s", A, B, tag)


@pytest.mark.parametrize("a,b", [(A, 0.0), (0.0, B)])
def test_each_term_alone(device, fx, cases, yardstick, a, b):
    """weight_free = 0: the squared miss alone; weight_depth = 0: the front opacity alone.  A +inf ray contributes no depth term."""
    target, names = cases
    got, want = _check_packed(fx, cases, yardstick, device, True, a, b, f"a={a} b={b}")
    slots = fx["rays"][:, 0]
    empty = np.array([name == "inf" for name in names])
    if b == 0:
        assert (got["loss_rays"][slots[empty]] == 0).all()
        for n in np.nonzero(empty)[0]:
            assert (got["grad_sigma"][DC.ray_rows(fx, n)[1]] == 0).all()
    else:
        assert (got["loss_rays"][slots[empty]] > 0).all()
        surface = np.array([name not in DC.NO_MEASUREMENT and name != "inf" and DC.ray_rows(fx, n)[3] for n, name in enumerate(names)])
        # b A with A the stored part: one product
        assert np.abs(got["loss_rays"][slots[surface]] - b * got["parts"][slots[surface], 1]).max() <= 2.0 ** -23


def test_same_bits_again_and_for_every_row_order(device, fx, cases):
    target = cases[0]
    a = _run_packed(fx, target, device, True, A, B)
    b = _run_packed(fx, target, device, True, A, B)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(fx["rays"].shape[0])).to(device)
    c = _run_packed(fx, target, device, True, A, B, rays=_t(fx["rays"], device)[perm].contiguous())
    assert all(torch.equal(x, y) for x, y in zip(a, c))          # the mean over the slots, every slot, every row of grad_sigmas


def _dense_bound(T, d64, z):
    """d and A are sums of T non-negative products: each product rounded once, 6 additions deep inside a 64-sample chunk, one more per
    chunk carried, (8 + T / 64) * 2^-24 of their value.  (d - z)^2 and 2 (d - z) t magnify d's error by 2 d / |d - z|, at most `amp`."""
    surface = np.isfinite(z) & (z > 0)
    amp = max(2.0, float(np.max(2 * d64[surface] / np.abs(d64 - z)[surface])))
    assert amp <= 30
    return amp * (8 + T / 64) * 2.0 ** -24


def _check_dense(device, w, t, z, scale, tag):
    from nerfsafetyvalidation_amd import loss as LS
    n = len(z)
    wt = _t(w, device).requires_grad_(True)
    loss = LS.depth_loss(wt, _t(t, device), _t(z, device), DC.MARGIN, None if scale is None else _t(scale, device), A, B)
    loss.backward()
    want_loss, want_g = DC.dense64(w, t, z, scale, a=A, b=B)
    bound = _dense_bound(w.shape[1], (w.astype(np.float64) * t).sum(axis=1), z.astype(np.float64))
    err = abs(float(loss.detach()) - want_loss.sum() / n) / (want_loss.sum() / n)
    got = wt.grad.cpu().numpy().astype(np.float64) * n
    gmax = np.abs(want_g).max(axis=1, keepdims=True)
    err_g = np.max(np.abs(got - want_g) / np.where(gmax > 0, gmax, 1))
    print(f"depth_loss {list(w.shape)} [{tag}]: loss {err:.2e}, grad_w {err_g:.2e} (bound {bound:.2e})")
    assert loss.shape == () and wt.grad.shape == wt.shape
    assert err <= bound + 8 * 2.0 ** -24 and err_g <= bound
    assert (got[~(z > 0)] == 0).all()                            # no measurement: every gradient row exactly 0
    return float(loss.detach())


def test_dense_operator_matches_float64(device, fx, cases, yardstick):
    target, names = cases
    # [6, 65]: one sample more than a chunk
    rng = np.random.default_rng(9)
    w = (rng.uniform(0, 1, (6, 65)) ** 3 * 0.05).astype(np.float32)
    t = np.sort(rng.uniform(0.5, 3.0, (6, 65)), axis=1).astype(np.float32)
    z = np.array([0.5 * (t[0, 30] + t[0, 31]) + DC.MARGIN, np.inf, 0.0, np.nan, 0.5 * (t[4, 63] + t[4, 64]) + DC.MARGIN, 4.0], dtype=np.float32)
    for r in (0, 4, 5):
        assert np.min(np.abs(t[r].astype(np.float64) - (float(z[r]) - DC.MARGIN))) > 1e-4
    _check_dense(device, w, t, z, rng.uniform(0.3, 0.8, 6).astype(np.float32), "T = 65")
    _check_dense(device, w, t, z, None, "T = 65, no scale")

    # the fixture's rays padded to [37, 1024]: w, t as the float32 CPU chain forms them (zero weights behind the stop and in the padding)
    slots = fx["rays"][:, 0]
    N = len(slots)
    w, t = np.zeros((N, 1024), dtype=np.float32), np.zeros((N, 1024), dtype=np.float32)
    for n in range(N):
        rows = DC.ray_rows(fx, n)[1]
        w[n, :rows.stop - rows.start], t[n, :rows.stop - rows.start] = fx["dense_w_1"][rows], fx["dense_m_1"][rows]
    z = target[slots].copy()
    z[-1] = 0.0                                                  # the ray the packed operator drops
    dense = _check_dense(device, w, t, z, fx["scale"][slots], "fixture, padded")
    # the dense and the packed operator on the same samples: w differs by float32 rounding of the chain, inside the packed bound
    want, ref_err = yardstick(True, A, B)
    packed = float(_run_packed(fx, target, device, True, A, B)[0])
    print(f"dense {dense:.8f} packed {packed:.8f} float64 {want['mean']:.8f}")
    assert abs(dense - packed) <= (SLACK * ref_err["loss"] + 8 * 2.0 ** -24) * want["mean"]


def test_twenty_thousand_short_rays(device):
    """20 000 rays of 3 samples: above the 16 384 rays where the fixed-order mean takes its workspace.  sigma dt in [0.2, 2], so
    alpha >= 0.18 and 1 - exp loses at most a factor 6; targets behind the ray by 0.1 .. 0.5 with d <= 0.1, so the squared miss magnifies
    by at most 2: a dozen operations of an ulp or two each, magnified by 6 -- 256 * 2^-24 on a gradient relative to the ray's largest,
    40 * 2^-24 on the mean (non-negative terms, added in double, then the butterflies)."""
    from nerfsafetyvalidation_amd import raymarching
    rng = np.random.default_rng(11)
    N, M = 20000, 60001
    dt = rng.uniform(0.005, 0.01, (N, 3)).astype(np.float32)
    sigma = (rng.uniform(0.2, 2.0, (N, 3)) / dt).astype(np.float32)
    deltas = np.zeros((M, 2), dtype=np.float32)
    sigmas = np.zeros(M, dtype=np.float32)
    sigmas[:3 * N], deltas[:3 * N, 0], deltas[:3 * N, 1] = sigma.reshape(-1), dt.reshape(-1), dt.reshape(-1)
    index = rng.permutation(N).astype(np.int32)
    table = np.stack([index, 3 * np.arange(N, dtype=np.int32), np.full(N, 3, dtype=np.int32)], axis=1)
    t64 = np.cumsum(dt.astype(np.float64), axis=1)
    z = (t64[:, 2] + rng.uniform(0.1, 0.5, N)).astype(np.float32)
    kind = rng.integers(0, 4, N)
    z[kind == 1], z[kind == 2] = np.inf, 0.0
    z[0], z[-1] = z[0] if np.isfinite(z[0]) and z[0] > 0 else 0.3, np.inf          # the first ray a surface, the last known empty
    target = np.zeros(N, dtype=np.float32)
    target[index] = z
    scale = rng.uniform(0.5, 2.0, N).astype(np.float32)
    s_ray = scale[index].astype(np.float64)

    x = sigma.astype(np.float64) * dt.astype(np.float64)
    alpha = 1 - np.exp(-x)
    T_next = np.cumprod(1 - alpha, axis=1)
    assert T_next.min() > 1e-3                                                      # nothing stops
    w = alpha * np.concatenate([np.ones((N, 1)), T_next[:, :-1]], axis=1)
    z64 = z.astype(np.float64)
    valid, empty = z64 > 0, np.isposinf(z64)
    front = (t64 < (z64 - DC.MARGIN)[:, None]).astype(np.float64)
    d, Af = (w * t64).sum(axis=1), (w * front).sum(axis=1)
    miss = np.where(valid & ~empty, s_ray * (d - np.where(empty | ~valid, 0, z64)), 0.0)
    L = np.where(valid, A * miss ** 2 + B * Af, 0.0)
    pull = np.where(valid & ~empty, 2 * A * s_ray ** 2 * (d - np.where(empty | ~valid, 0, z64)), 0.0)
    g = np.where(valid[:, None], pull[:, None] * t64 + B * front, 0.0)
    gw = g * w
    after = np.concatenate([np.cumsum(gw[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((N, 1))], axis=1)
    grad = dt.astype(np.float64) * (T_next * g - after)

    sig = _t(sigmas, device).requires_grad_(True)
    loss, loss_rays, parts = raymarching.depth_rays_train(sig, _t(deltas, device), _t(table, device), _t(target, device), DC.MARGIN,
                                                          _t(scale, device), A, B, return_rays=True)
    loss.backward()
    err_mean = abs(float(loss.detach()) - L.sum() / N) / (L.sum() / N)
    got = sig.grad.cpu().numpy().astype(np.float64)[:3 * N].reshape(N, 3) * N
    err_first = np.abs(got[0] - grad[0]).max() / np.abs(grad[0]).max()
    err_last = np.abs(got[-1] - grad[-1]).max() / np.abs(grad[-1]).max()
    print(f"20000 x 3: mean {err_mean:.2e} (bound {40 * 2.0 ** -24:.2e}), grad first ray {err_first:.2e}, last ray {err_last:.2e} (bound {256 * 2.0 ** -24:.2e})")
    assert err_mean <= 40 * 2.0 ** -24
    assert err_first <= 256 * 2.0 ** -24 and err_last <= 256 * 2.0 ** -24
    assert (got[~valid] == 0).all() and float(sig.grad[3 * N:].abs().max()) == 0
    lr = loss_rays.cpu().numpy().astype(np.float64)[index]
    assert np.abs(lr - L).max() <= 64 * 2.0 ** -24 * L.max()


def test_depth_targets_kernel(device):
    """ngp_train_depth_targets on a 5 x 7 frame (the second of two in the store) with duplicate pixel ids: 0 and +inf exact, finite
    values within 2 ulp of the float32 numpy expression (contraction of the radicand, one rounding each for the root and the product)."""
    from nerfsafetyvalidation_amd.nerf import targets as TG
    H, W = 5, 7
    rng = np.random.default_rng(2)
    codes = rng.integers(1, 65535, (2, H, W)).astype(np.uint16)
    codes[1, 0, :4] = [0, 1, 65534, 65535]
    intr = (6.5, 5.25, 3.1, 2.8)
    unit = float(np.float32(3.0 / 65534 * 0.8))
    store = TG.DepthStore.from_codes(codes, H, W, unit, intr).to(device)
    pix = np.array([0, 1, 2, 3, 3, 0, 34, 17, 17, 8, 20, 1], dtype=np.int64)
    batch = TG.DepthBatch(store, 1, _t(pix, device)[None], device)
    got = TG.training_depth_targets(batch)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, len(pix))
    got = got[0].cpu().numpy()
    f = np.float32
    x = ((pix % W).astype(f) + f(0.5) - f(intr[2])) / f(intr[0])
    y = ((pix // W).astype(f) + f(0.5) - f(intr[3])) / f(intr[1])
    c = codes[1].reshape(-1)[pix]
    want = (c.astype(f) * f(unit)) * np.sqrt((x * x + y * y) + f(1.0))
    assert want.dtype == np.float32
    assert (got[c == 0] == 0).all() and np.isposinf(got[c == 65535]).all() and (c == 0).sum() == 2 and (c == 65535).sum() == 2
    fin = (c != 0) & (c != 65535)
    ulps = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / np.spacing(want[fin]).astype(np.float64)
    print(f"train_depth_targets: worst {ulps.max():.2f} ulp")
    assert ulps.max() <= 2
    err = np.abs(batch.materialize()[0].cpu().numpy()[fin].astype(np.float64) - want[fin]) / np.spacing(want[fin])
    assert err.max() <= 2                                                      # the torch form on the device: the same expression
    whole = TG.training_depth_targets(TG.DepthBatch(store, 1, None, device))   # evaluation: every pixel in order
    assert tuple(whole.shape) == (1, H * W) and np.array_equal(whole[0].cpu().numpy()[pix], got)


# ------------------------------------------------------------------------------------------------ renderer and Trainer
def _patch_rays(sc, device):
    """64 rays: an 8 x 8 patch at the centre of a 48 x 48 Stonehenge frame"""
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    rays = get_rays(torch.from_numpy(sc.poses).to(device)[7:8], sc.intrinsics, sc.H, sc.W)
    pick = (torch.arange(20, 28, device=device)[:, None] * sc.W + torch.arange(20, 28, device=device)[None, :]).reshape(-1)
    return rays["rays_o"][:, pick].contiguous(), rays["rays_d"][:, pick].contiguous()


@pytest.mark.parametrize("cuda_ray", [True, False])
def test_renderer_term_is_opt_in(device, cuda_ray):
    from nerfsafetyvalidation_amd import raymarching
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=48, W=48, bound=2)
    model = sc.build_model(device, cuda_ray=cuda_ray).train()
    ro, rd = _patch_rays(sc, device)
    kw = dict(staged=False, bg_color=1, perturb=False) if cuda_ray else dict(staged=False, bg_color=1, perturb=False, num_steps=48, upsample_steps=16)
    with torch.no_grad():
        nears, fars = raymarching.near_far_from_aabb(ro.view(-1, 3), rd.view(-1, 3), model.aabb_train, model.min_near)
    target = (nears + 0.4 * (fars - nears)).clone()
    target[:8], target[8:16], target[16] = 0.0, float("inf"), float("nan")
    target = target.view(1, -1)

    def render(**extra):
        torch.manual_seed(11)                  # (training-mode `run` draws the resampling positions)
        model.local_step = 0
        with torch.autocast("cuda", dtype=torch.float16):
            return model.render(ro, rd, **kw, **extra)

    def image_backward(**extra):
        """-> (outputs, the gradients that arrive at the call's sigmas / rgbs, the parameter gradients) of sum(image) * 64"""
        model.zero_grad(set_to_none=True)
        out, seen = render(**extra), {}
        for k in ("sigmas", "rgbs"):
            if out[k].requires_grad:
                out[k].register_hook(lambda g, k=k: seen.__setitem__(k, g.clone()))
        (out["image"].float().sum() * 64.0).backward()
        return out, seen, [None if p.grad is None else p.grad.clone() for p in model.parameters()]

    # Both weights 0: the image and the gradients are those of a call without the depth arguments, bit for bit.  The hash table's
    # gradient is summed by float atomics in arrival order (csrc/gridencoder.hip) and differs between two IDENTICAL calls, so "the same
    # bits" is asked of everything that has them: the gradients arriving at the call's samples, and every parameter whose gradient two
    # plain calls agree on (the two MLPs among them); a parameter that two plain calls disagree on must agree as well as they do.
    plain, plain_seen, plain_grads = image_backward()
    _, again_seen, again_grads = image_backward()
    off, off_seen, off_grads = image_backward(lambda_depth=0, lambda_free=0, depth_margin=0.02, depth_target=target)
    assert list(plain) == list(off) and "loss_depth" not in off and "loss_depth_parts" not in off
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(plain[k], off[k]), k
    assert set(plain_seen) == set(off_seen) and (not cuda_ray or set(plain_seen) == {"sigmas", "rgbs"})
    for k in plain_seen:
        assert torch.equal(plain_seen[k], off_seen[k]) and torch.equal(plain_seen[k], again_seen[k]), k
    exact = 0
    for (name, _), p, q, r in zip(model.named_parameters(), plain_grads, again_grads, off_grads):
        if p is None:
            assert q is None and r is None, name
        elif torch.equal(p, q):
            assert torch.equal(p, r), name
            exact += 1
        else:
            spread = float((p.float() - q.float()).abs().max())
            print(f"{name}: two plain calls differ by {spread:.3e} (max |grad| {float(p.float().abs().max()):.3e})")
            assert "embeddings" in name and float((p.float() - r.float()).abs().max()) <= SLACK * spread, name
    assert exact >= 2
    assert "loss_depth" not in render(lambda_depth=1.0, lambda_free=1.0)        # the weights without a target

    model.zero_grad(set_to_none=True)
    on = render(lambda_depth=0.5, lambda_free=0.1, depth_margin=0.02, depth_target=target)
    assert set(on) == set(plain) | {"loss_depth", "loss_depth_parts"}
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(plain[k], on[k]), k
    term, parts = on["loss_depth"], on["loss_depth_parts"]
    assert term.shape == () and torch.isfinite(term) and float(term.detach()) > 0
    assert tuple(parts.shape) == (2,) and not parts.requires_grad and torch.isfinite(parts).all()
    assert abs(float(term.detach()) - (0.5 * float(parts[0]) + 0.1 * float(parts[1]))) <= 1e-5 * float(term.detach()) + 1e-7
    if cuda_ray:
        # by hand: the same march (no jitter), depth_rays_train on that call's sigmas, the target counted from the ray's near
        counter = torch.zeros(2, dtype=torch.int32, device=device)
        _, _, deltas, rays = raymarching.march_rays_train(ro.view(-1, 3), rd.view(-1, 3), model.bound, model.density_bitfield, model.cascade,
                                                          model.grid_size, nears, fars, counter, model.mean_count, False, 128, False, 0, 1024)
        rel = model.march_depth_target(target.view(-1), nears)
        assert float(rel[0]) == 0 and float(rel[8]) == float("inf") and float(rel[16]) == 0 and torch.equal(rel[17:], (target.view(-1) - nears)[17:])
        by_hand = raymarching.depth_rays_train(on["sigmas"].detach(), deltas, rays, rel, 0.02, 1 / (fars - nears), 0.5, 0.1)
        assert torch.equal(by_hand, term.detach())
    (term * 1024.0).backward()            # (scaled as a GradScaler would: the sigma net runs its backward in half)
    table, sigma_w, color_w = model.encoder.embeddings.grad, model.sigma_net.weights.grad, model.color_net.weights.grad
    assert table is not None and torch.isfinite(table).all() and float(table.float().abs().max()) > 0
    assert sigma_w is not None and torch.isfinite(sigma_w).all() and float(sigma_w.float().abs().max()) > 0
    assert color_w is None or float(color_w.float().abs().max()) == 0

    with torch.no_grad():
        assert "loss_depth" not in render(lambda_depth=0.5, depth_target=target)
    model.eval()
    with torch.no_grad():
        assert "loss_depth" not in render(lambda_depth=0.5, depth_target=target)


def test_trainer_takes_three_depth_supervised_steps(device, tmp_path):
    """a 32 x 32, 4-view dataset written with --depth from henge_mesh, cuda_ray, both weights positive"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import make_mesh_dataset as MD
    finally:
        sys.path.pop(0)
    from nerfsafetyvalidation_amd.nerf.provider import NeRFDataset
    from nerfsafetyvalidation_amd.nerf.targets import DepthBatch
    from nerfsafetyvalidation_amd.nerf.trainer import Trainer
    from nerfsafetyvalidation_amd.optim import Adam
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    root = MD.make(str(tmp_path / "ds"), size=32, n_train=4, n_val=1, n_test=1, device=str(device), resolution=32, depth=True)
    assert "integer_depth_scale" in json.load(open(os.path.join(root, "transforms_train.json")))
    opt = SimpleNamespace(path=root, preload=True, scale=1.0, offset=[0, 0, 0], bound=2, fp16=True, num_rays=512, rand_pose=-1, error_map=False,
                          color_space="srgb", update_extra_interval=16, iters=30000, cuda_ray=True, dt_gamma=0, max_steps=1024,
                          lambda_depth=0.1, lambda_free=0.01, depth_margin=0.02)
    sc = StonehengeScene(H=32, W=32, bound=2)
    model = sc.build_model(device, table_seed=1)
    model.encoder.reset_parameters()
    model.reset_extra_state()
    torch.manual_seed(0)
    trainer = Trainer("ngp", opt, model, device=device, workspace=str(tmp_path / "ws"), optimizer=lambda m: Adam(m.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-15),
                      criterion=torch.nn.MSELoss(reduction="none"), fp16=True, use_checkpoint="scratch", mute=True, use_tensorboardX=False)
    data = NeRFDataset(opt, device, type="train")
    assert data.depths is not None and data.depths.data.is_cuda and tuple(data.depths.data.shape) == (4, 32 * 32)
    loader = data.dataloader()
    trainer.model.train()
    losses = []
    for step, batch in enumerate(loader):
        if step == 3:
            break
        assert isinstance(batch["depth"], DepthBatch)
        if step % 16 == 0:
            with trainer._autocast():
                trainer.model.update_extra_state()
        trainer.optimizer.zero_grad()
        with trainer._autocast():
            _, _, loss = trainer.train_step(batch)
        assert trainer.last_loss_depth is not None and torch.isfinite(trainer.last_loss_depth) and torch.isfinite(trainer.last_loss_depth_parts).all()
        if step == 2:       # the depth terms alone reach the density network, and nothing else
            (trainer.last_loss_depth * 1024.0).backward()
            sigma_w, color_w = model.sigma_net.weights.grad, model.color_net.weights.grad
            assert sigma_w is not None and torch.isfinite(sigma_w).all() and float(sigma_w.float().abs().max()) > 0
            assert color_w is None or float(color_w.float().abs().max()) == 0
        else:
            trainer.scaler.scale(loss).backward()
            trainer.scaler.step(trainer.optimizer)
            trainer.scaler.update()
        losses.append((float(loss.detach()), float(trainer.last_loss_depth.detach())))
    print("loss, loss_depth per step:", losses)
    assert len(losses) == 3 and all(np.isfinite(v).all() for v in losses)
    assert all(depth > 0 for _, depth in losses)
