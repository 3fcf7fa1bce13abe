"""Caller-owned workspaces on the device: every entry point that carves its scratch through csrc/workspace.hpp runs in a workspace of
EXACTLY the bytes its ngp_*_workspace function answers, between two guard regions that must come back untouched; computes the same
bits in a workspace four times as large with other contents; and, one byte short, returns NGP_EWORKSPACE naming both sizes and
launches nothing.  Shapes: the smallest that put something into every region of a layout."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL, OTHER, GUARD = 0xA5, 0x3C, 256
NGP_EWORKSPACE = -3


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


class Case:
    """call(workspace pointer, bytes) -> status; outputs: tensors the call only writes; inouts: (tensor, its value before the call)"""

    def __init__(self, need, call, outputs, inouts=()):
        self.need, self.call, self.outputs, self.inouts = need, call, list(outputs), list(inouts)

    def run(self, pointer, nbytes):
        for o in self.outputs:
            _bytes(o).fill_(FILL)
        for t, before in self.inouts:
            t.copy_(before)
        rc = self.call(pointer, nbytes)
        torch.cuda.synchronize()
        return rc

    def results(self):
        return [_bytes(t).clone() for t in self.outputs + [t for t, _ in self.inouts]]


def exercise(case, device):
    from nerfsafetyvalidation_amd import _lib
    L, need = _lib.lib(), case.need
    assert need > 0
    buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0
    middle = buf.data_ptr() + GUARD
    assert case.run(middle, need) == 0, L.ngp_last_error()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + need:] == FILL).all()), "wrote outside the workspace"
    exact = case.results()
    assert any(bool((r != FILL).any()) for r in exact), "the call wrote nothing"
    big = torch.full((4 * need,), OTHER, dtype=torch.uint8, device=device)
    assert case.run(big.data_ptr(), 4 * need) == 0, L.ngp_last_error()
    for i, (a, b) in enumerate(zip(exact, case.results())):
        assert torch.equal(a, b), f"result {i} depends on the workspace's size or contents"
    buf.fill_(FILL)
    assert case.run(middle, need - 1) == NGP_EWORKSPACE
    msg = L.ngp_last_error().decode()
    assert "workspace too small" in msg and f"({need - 1} < {need} bytes)" in msg, msg
    assert all(bool((_bytes(o) == FILL).all()) for o in case.outputs), "launched before it refused"
    assert all(torch.equal(_bytes(t), _bytes(before)) for t, before in case.inouts), "launched before it refused"
    assert bool((buf == FILL).all())
    assert case.run(middle, need) == 0      # (and the refusal broke nothing: the callers below look at these results)
    for a, b in zip(exact, case.results()):
        assert torch.equal(a, b)
    case.buffer = buf                        # `middle` stays valid for the caller
    return L, middle


def _rand(device, *shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(device)


# ---------------------------------------------------------------------------------------------------------------- train march
@pytest.mark.parametrize("N", [5, 1024], ids=["plain", "occupancy_copies_and_trace"])
def test_march_rays_train(device, N):
    from nerfsafetyvalidation_amd import _lib, raymarching
    L, s = _lib.lib(), _lib.stream()
    C_, H, bound, max_steps = 2, 16, 2.0, 64
    g = torch.Generator().manual_seed(N)
    bits = (torch.randint(0, 256, (C_ * H ** 3 // 8,), generator=g, dtype=torch.uint8) & torch.randint(0, 256, (C_ * H ** 3 // 8,), generator=g, dtype=torch.uint8)).to(device)
    yz = torch.rand(N, 2, generator=g) * 2 - 1
    o = torch.cat([torch.full((N, 1), -3.0), yz], 1).to(device).contiguous()
    d = torch.nn.functional.normalize(torch.cat([torch.ones(N, 1), (torch.rand(N, 2, generator=g) - 0.5) * 0.4], 1), dim=1).to(device).contiguous()
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32, device=device)
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, 0.2)
    M = N * max_steps
    xyzs, dirs, deltas = torch.empty(M, 3, device=device), torch.empty(M, 3, device=device), torch.empty(M, 2, device=device)
    rays = torch.empty(N, 3, dtype=torch.int32, device=device)
    counter = torch.zeros(2, dtype=torch.int32, device=device)
    call = lambda ws, n: L.ngp_march_rays_train(_lib.ptr(o), _lib.ptr(d), _lib.ptr(bits), bound, 0.0, max_steps, N, C_, H, M, _lib.ptr(nears),   # noqa: E731
                                                 _lib.ptr(fars), _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(deltas), _lib.ptr(rays), _lib.ptr(counter), 0,
                                                 ws, n, s)
    exercise(Case(L.ngp_march_rays_train_workspace(N), call, [xyzs, dirs, deltas, rays], [(counter, torch.zeros_like(counter))]), device)
    assert int(counter[1]) == N and 0 < int(counter[0]) <= M


# ---------------------------------------------------------------------------------------------------------------- volumes
def test_edt_sq(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    X, Y, Z = 4, 5, 6
    occ = (_rand(device, X, Y, Z, seed=1) < 0.2).to(torch.uint8).contiguous()
    d2 = torch.empty(X, Y, Z, dtype=torch.int32, device=device)
    call = lambda ws, n: L.ngp_edt_sq(_lib.ptr(occ), X, Y, Z, _lib.ptr(d2), ws, n, s)      # noqa: E731
    exercise(Case(L.ngp_edt_sq_workspace(X, Y, Z), call, [d2]), device)


def test_label_components(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    X, Y, Z = 5, 6, 7
    occ = (_rand(device, X, Y, Z, seed=2) < 0.4).to(torch.uint8).contiguous()
    labels = torch.empty(X, Y, Z, dtype=torch.int32, device=device)
    n_comp = torch.empty(1, dtype=torch.int32, device=device)
    call = lambda ws, n: L.ngp_label_components(_lib.ptr(occ), X, Y, Z, 26, _lib.ptr(labels), _lib.ptr(n_comp), ws, n, s)      # noqa: E731
    exercise(Case(L.ngp_label_components_workspace(X, Y, Z), call, [labels, n_comp]), device)
    assert int(n_comp) >= 1


def test_isosurface_count_and_emit(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    X, Y, Z = 5, 6, 7
    u = (_rand(device, X, Y, Z, seed=3) - 0.5).contiguous()
    need = L.ngp_isosurface_workspace(X, Y, Z)
    totals = torch.zeros(2, dtype=torch.int64, device=device)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    assert L.ngp_isosurface_count(_lib.ptr(u), X, Y, Z, 0.0, _lib.ptr(scratch), need, _lib.ptr(totals), s) == 0
    V, F = totals.tolist()
    assert V > 0 and F > 0
    verts, faces = torch.empty(V, 3, device=device), torch.empty(F, 3, dtype=torch.int32, device=device)
    emit = lambda ws, n: L.ngp_isosurface_emit(_lib.ptr(u), X, Y, Z, 0.0, ws, n, V, F, _lib.ptr(verts), _lib.ptr(faces), s)      # noqa: E731

    def call(ws, n):      # the emit reads what the count left in the same workspace
        return L.ngp_isosurface_count(_lib.ptr(u), X, Y, Z, 0.0, ws, n, _lib.ptr(totals), s) or emit(ws, n)
    case = Case(need, call, [totals, verts, faces])
    L, middle = exercise(case, device)
    assert emit(middle, need - 1) == NGP_EWORKSPACE and f"isosurface_emit: workspace too small ({need - 1} < {need} bytes)".encode() in L.ngp_last_error()


# ---------------------------------------------------------------------------------------------------------------- sums
def test_distance_stats_with_an_open_group_at_each_end(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    seen, n = 70, 130
    d = _rand(device, seen + n, seed=4)
    d[::17] = float("inf")
    th = (C.c_float * 2)(0.3, 0.6)
    state = torch.zeros(L.ngp_distance_stats_state_bytes(), dtype=torch.uint8, device=device)
    stats = torch.empty(16, dtype=torch.float64, device=device)
    first = torch.empty(L.ngp_distance_stats_workspace(seen), dtype=torch.uint8, device=device)
    assert L.ngp_distance_stats(_lib.ptr(d), seen, 0, th, 2, _lib.ptr(state), _lib.ptr(stats), _lib.ptr(first), first.numel(), s) == 0
    torch.cuda.synchronize()
    before = state.clone()
    tail = d[seen:]
    call = lambda ws, nb: L.ngp_distance_stats(_lib.ptr(tail), n, seen, th, 2, _lib.ptr(state), _lib.ptr(stats), ws, nb, s)      # noqa: E731
    exercise(Case(L.ngp_distance_stats_workspace(n), call, [stats], [(state, before)]), device)
    finite = d[torch.isfinite(d)].double()
    assert stats[0].item() == finite.numel() and stats[12].item() == seen + n and abs(stats[1].item() - finite.sum().item()) < 1e-9


def test_uq_stats(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    c, d, r = _rand(device, 500, 3, seed=5), _rand(device, 500, seed=6), _rand(device, 300, seed=7)
    stats = torch.empty(8, dtype=torch.float64, device=device)
    call = lambda ws, n: L.ngp_uq_stats(_lib.ptr(c), 0, _lib.ptr(d), 500, _lib.ptr(r), 300, _lib.ptr(stats), ws, n, s)      # noqa: E731
    exercise(Case(L.ngp_uq_stats_workspace(), call, [stats]), device)
    assert stats[3].item() == 300 and stats[6].item() == 500


def test_sigma_fit(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    n, max_wg = 300, 3
    feat, y, theta = _rand(device, n, 32, seed=8), _rand(device, n, seed=9), (_rand(device, 3072, seed=10) - 0.5) * 0.2
    loss, grad = torch.empty(1, dtype=torch.float64, device=device), torch.empty(3072, device=device)
    call = lambda ws, nb: L.ngp_sigma_fit_eval(_lib.ptr(feat), _lib.ptr(y), n, _lib.ptr(theta), 0.0, 1.0, 2, max_wg, ws, nb, _lib.ptr(loss),   # noqa: E731
                                                _lib.ptr(grad), s)
    exercise(Case(L.ngp_sigma_fit_workspace(n, max_wg), call, [loss, grad]), device)
    assert L.ngp_sigma_fit_workspace(n, max_wg) == 3 * (8 + (2048 + 64) * 4)


def test_image_quality(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    B, H, W = 2, 71, 133
    pred, target = _rand(device, B, 3, H, W, seed=11), _rand(device, B, 3, H, W, seed=12)
    ssim, stats = torch.empty(B, H, W, device=device), torch.empty(B * 8, dtype=torch.float64, device=device)
    call = lambda ws, n: L.ngp_image_quality(_lib.ptr(pred), _lib.ptr(target), None, B, H, W, 3 * H * W, H * W, W, 1, 1.0, _lib.ptr(ssim),   # noqa: E731
                                              _lib.ptr(stats), ws, n, s)
    exercise(Case(L.ngp_image_quality_workspace(B, H, W), call, [ssim, stats]), device)


def test_sift_interest_mask(device):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    H = W = 8
    rgb = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(13), dtype=torch.uint8).to(device)
    points, mask = torch.empty(H * W, dtype=torch.uint8, device=device), torch.empty(H * W, dtype=torch.uint8, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    call = lambda ws, n: L.ngp_sift_interest_mask(_lib.ptr(rgb), H, W, 3, 1, _lib.ptr(points), _lib.ptr(mask), _lib.ptr(count), ws, n, s)      # noqa: E731
    exercise(Case(L.ngp_sift_workspace(H, W), call, [points, mask, count]), device)


# ---------------------------------------------------------------------------------------------------------------- density grid
@pytest.mark.parametrize("cascade,H", [(8, 4), (2, 32)], ids=["a_level_smaller_than_a_workgroup", "32x32x32x2"])
def test_density_grid_update_and_finish(device, cascade, H):
    """(8, 4): eight levels of 64 cells -- eight partial sums, where the size function once counted two"""
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    H3, n = H ** 3, 50 if H == 4 else 1000
    g = torch.Generator().manual_seed(H)
    grid0 = torch.where(torch.rand(cascade, H3, generator=g) < 0.2, torch.tensor(-1.0), torch.rand(cascade, H3, generator=g)).to(device).contiguous()
    grid = grid0.clone()
    idx = torch.randint(0, H3, (n,), generator=g, dtype=torch.int32).to(device)
    sig = torch.rand(n, generator=g).to(device)
    mean_thresh = torch.empty(2, device=device)
    bitfield = torch.empty(cascade * H3 // 8, dtype=torch.uint8, device=device)
    need = L.ngp_density_grid_workspace(cascade, H)
    assert need >= H3 * 8 + cascade * -(-H3 // 256) * 8
    finish = lambda ws, nb: L.ngp_density_grid_finish(_lib.ptr(grid), cascade, H, 0.01, _lib.ptr(mean_thresh), _lib.ptr(bitfield), ws, nb, s)      # noqa: E731

    def call(ws, nb):
        return L.ngp_density_grid_update(_lib.ptr(grid), cascade, H, cascade - 1, _lib.ptr(idx), _lib.ptr(sig), n, 1.0, 0.95, ws, nb, s) or finish(ws, nb)
    case = Case(need, call, [mean_thresh, bitfield], [(grid, grid0)])
    L, middle = exercise(case, device)
    assert finish(middle, need - 1) == NGP_EWORKSPACE and f"density_grid_finish: workspace too small ({need - 1} < {need} bytes)".encode() in L.ngp_last_error()
    want = grid.clamp(min=0).double().mean().item()
    assert abs(mean_thresh[0].item() - want) <= 1e-6 * want and bool(bitfield.any())


def test_mark_untrained_grid_in_camera_batches(device):
    """2049 poses, the seven cameras of density_grid.npz over and over: two launches, the second reading the first's flags from the
    workspace ngp_mark_untrained_grid_workspace sizes -- and, repeats adding nothing to a union, the seven cameras' own marking.
    Three cascades: the density grid's workspace, which the renderer used to hand over, is too small for the flags."""
    from nerfsafetyvalidation_amd import _lib
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    f = np.load(os.path.join(G, "density_grid.npz"))
    H = 32
    net = NeRFNetwork(encoding="hashgrid", bound=4, cuda_ray=True, min_near=0.2, density_thresh=0.01, bg_radius=-1)
    assert net.cascade == 3
    net.grid_size = H
    net.density_grid = torch.zeros(net.cascade, H ** 3)
    net.density_bitfield = torch.zeros(net.cascade * H ** 3 // 8, dtype=torch.uint8)
    net = net.to(device).eval()
    L = _lib.lib()
    assert L.ngp_mark_untrained_grid_workspace(2049, 3, H) == 3 * H ** 3 * 4 > L.ngp_density_grid_workspace(3, H)
    assert L.ngp_mark_untrained_grid_workspace(7, 3, H) == 0
    net.mark_untrained_grid(f["poses"], f["intrinsics"])
    seven = net.density_grid.clone()
    assert 0 < int((seven == -1).sum()) < seven.numel()
    many = np.tile(f["poses"], (293, 1, 1))[:2049]
    assert many.shape == (2049, 4, 4)
    net.density_grid.zero_()
    net.mark_untrained_grid(many, f["intrinsics"])
    torch.cuda.synchronize()
    assert torch.equal(_bytes(net.density_grid), _bytes(seven))
    # one byte short of the flags: refused by name, the grid untouched
    net.density_grid.zero_()
    cams = torch.from_numpy(many).to(device).contiguous()
    fx, fy, cx, cy = [float(v) for v in f["intrinsics"]]
    need = 3 * H ** 3 * 4
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    rc = L.ngp_mark_untrained_grid(_lib.ptr(cams), 2049, fx, fy, cx, cy, 4.0, 3, H, _lib.ptr(net.density_grid), _lib.ptr(ws), need - 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc == NGP_EWORKSPACE and f"mark_untrained_grid: workspace too small ({need - 1} < {need} bytes)".encode() in L.ngp_last_error()
    assert bool((net.density_grid == 0).all())


# ---------------------------------------------------------------------------------------------------------------- the mean of the losses
N_MEAN, T_MEAN = 16385, 2      # the first ray count whose mean goes through group sums in the workspace


@pytest.mark.parametrize("entry", ["photo_loss_forward", "distortion_forward", "distortion_train_forward", "depth_loss_forward", "depth_loss_train_forward"])
def test_mean_based_losses(device, entry):
    from nerfsafetyvalidation_amd import _lib
    L, s = _lib.lib(), _lib.stream()
    N, T = N_MEAN, T_MEAN
    M = N * T
    row = torch.arange(N, dtype=torch.int32, device=device)
    rays = torch.stack([row, row * T, torch.full_like(row, T)], dim=1).contiguous()
    a, b2 = _rand(device, M, seed=14) * 0.5, _rand(device, M, 2, seed=15) * 0.1
    pos = _rand(device, M, seed=16)
    target = _rand(device, N, seed=17) + 0.5
    loss_rays, pair, loss = torch.empty(N, device=device), torch.empty(N, 2, device=device), torch.empty(1, device=device)
    p = _lib.ptr
    if entry == "photo_loss_forward":
        pred, gt = _rand(device, N, 3, seed=18), _rand(device, N, 3, seed=19)
        need, outputs = L.ngp_photo_loss_workspace(N), [loss_rays, loss]
        call = lambda ws, n: L.ngp_photo_loss_forward(p(pred), 0, p(gt), N, p(loss_rays), p(loss), None, 0, None, ws, n, s)      # noqa: E731
    elif entry == "distortion_forward":
        need, outputs = L.ngp_distortion_workspace(N), [loss_rays, pair, loss]
        call = lambda ws, n: L.ngp_distortion_forward(p(a), p(pos), None, 0.01, p(rays), M, N, p(loss_rays), p(pair), p(loss), ws, n, s)      # noqa: E731
    elif entry == "distortion_train_forward":
        need, outputs = L.ngp_distortion_workspace(N), [loss_rays, pair, loss]
        call = lambda ws, n: L.ngp_distortion_train_forward(p(a), p(b2), p(rays), None, M, N, p(loss_rays), p(pair), p(loss), ws, n, s)      # noqa: E731
    elif entry == "depth_loss_forward":
        need, outputs = L.ngp_depth_loss_workspace(N), [loss_rays, pair, loss]
        call = lambda ws, n: L.ngp_depth_loss_forward(p(a), p(pos), p(rays), p(target), None, 0.05, 1.0, 1.0, M, N, p(loss_rays), p(pair), p(loss),   # noqa: E731
                                                       ws, n, s)
    else:
        need, outputs = L.ngp_depth_loss_workspace(N), [loss_rays, pair, loss]
        call = lambda ws, n: L.ngp_depth_loss_train_forward(p(a), p(b2), p(rays), p(target), None, 0.05, 1.0, 1.0, M, N, p(loss_rays), p(pair),   # noqa: E731
                                                             p(loss), ws, n, s)
    assert need == 257 * 4
    exercise(Case(need, call, outputs), device)
    assert abs(loss.item() - loss_rays.double().mean().item()) <= 1e-5 * abs(loss.item()) and loss.item() != 0


# ---------------------------------------------------------------------------------------------------------------- upsample
def test_render_upsample_takes_its_workspace_or_the_per_ray_route(device, monkeypatch):
    """65 536 rays, the smallest batch that goes through the workspace: exact bytes between guards, the same bits with four times as
    many; one byte short is NOT an error here -- the call takes the one-launch route and leaves the workspace alone."""
    from nerfsafetyvalidation_amd import _lib, raymarching
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=256, W=256, bound=2, radius=1.5)
    model = sc.build_model(device, cuda_ray=False)
    ro, rd = Hh.pinhole_rays(sc.poses[47], sc.intrinsics, sc.H, sc.W)
    o, d = torch.from_numpy(np.ascontiguousarray(ro)).to(device), torch.from_numpy(np.ascontiguousarray(rd)).to(device)
    N, T, U = o.shape[0], 4, 2
    assert N == 65536
    need = _lib.lib().ngp_render_upsample_workspace(N, T, U)
    assert need == N * ((T + 2 * U) * 4 + (T + U) * 32) and _lib.lib().ngp_render_upsample_workspace(N - 1, T, U) == 0
    buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=device)
    big = torch.full((4 * need,), OTHER, dtype=torch.uint8, device=device)
    given = {}

    def workspace(name, *dims, device):
        assert name == "render_upsample" and dims == (N, T, U)
        return given["buffer"], given["bytes"]
    monkeypatch.setattr(_lib, "workspace", workspace)
    res = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fm = model.fused_model()
        assert fm.upsample_fits(T, U)
        nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_infer, model.min_near)
        for form, buffer, nbytes in (("exact", buf[GUARD:GUARD + need], need), ("big", big, 4 * need), ("short", buf[GUARD:GUARD + need], need - 1)):
            if form == "short":
                buf.fill_(FILL)
            given.update(buffer=buffer, bytes=nbytes)
            res[form] = [_bytes(t).clone() for t in fm.render_upsample(o, d, nears, fars, T, U, N - 2500, 0)]
            torch.cuda.synchronize()
            if form == "exact":
                assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + need:] == FILL).all()), "wrote outside the workspace"
                assert bool((buf[GUARD:GUARD + need] != FILL).any())
    for i, (a, b) in enumerate(zip(res["exact"], res["big"])):
        assert torch.equal(a, b), i
    assert bool((buf == FILL).all()), "the per-ray route touched the workspace"
    for i in (4, 5):      # the samples' sigmas and colours are the same bits on either route (the per-ray sums run in another order)
        a, b = res["exact"][i].view(torch.float32), res["short"][i].view(torch.float32)
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), i
