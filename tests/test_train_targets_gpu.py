"""csrc/train_data.hip (ngp_train_targets, ngp_photo_loss_forward / _backward) against the torch chain of nerf/targets.py on the same
device and against float64.  Shapes: the sizes around a wave (63 / 64 / 65), one more than the workgroups of the three kernels (257,
1025), 4097, and 16385 where the loss takes its two-launch form; frames of 35 and of 1023 pixels."""
import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd.nerf import targets as TG

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1025, 4097, 16385)
FRAMES = ((5, 7), (33, 31))


def ulps(got, want64, dtype=np.float32):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    unit = np.spacing(np.maximum(np.abs(want64), np.finfo(dtype).tiny).astype(dtype)).astype(np.float64)
    return np.abs(got - want64) / unit


def make_store(H, W, C, dtype, device, seed=0):
    """3 frames; uint8 codes and the tensor the reference would hold for them (float32 code / 255, or its half)"""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (3, H * W, C), dtype=torch.uint8, generator=g)
    if C == 4:
        codes[:, 0, 3], codes[:, 1, 3] = 0, 255
    codes = codes.to(device)
    values = TG.code_table().to(device)[codes.long()]
    store = codes if dtype == torch.uint8 else values.to(dtype)
    return store.contiguous(), codes, values


def pixel_ids(N, n_pix, device, seed):
    """random ids with 0, n_pix - 1 and a duplicate among them (N > n_pix repeats anyway)"""
    g = torch.Generator().manual_seed(seed)
    inds = torch.randint(0, n_pix, (N,), generator=g)
    fixed = [0, n_pix - 1, n_pix - 1]
    inds[:min(N, 3)] = torch.tensor(fixed[:min(N, 3)])
    return inds.to(device)


# (the round-to-half flag belongs to the uint8 store: an f16 store is half already, an f32 store never is)
@pytest.mark.parametrize("dtype,half", [(torch.uint8, False), (torch.uint8, True), (torch.float16, False), (torch.float32, False)])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("HW", FRAMES)
def test_targets_equal_the_torch_chain_in_srgb(device, HW, C, dtype, half):
    H, W = HW
    n_pix = H * W
    store, codes, values = make_store(H, W, C, dtype, device)
    in_half = half or dtype == torch.float16
    held = values.half() if in_half else values                      # the tensor the reference holds (provider.py:250-254)
    for frame, N in [(2, n) for n in SIZES] + [(0, 65), (1, 64)]:
        inds = pixel_ids(N, n_pix, device, N)
        images = torch.gather(held[frame:frame + 1], 1, torch.stack(C * [inds[None]], -1))
        for backdrop in ("white", "random"):
            bg = 1 if backdrop == "white" else torch.rand_like(images[..., :3])
            want = TG.reference_targets(images.clone(), bg, "srgb")
            got = TG.gather_targets(store, frame * n_pix, n_pix, inds, None if backdrop == "white" else bg.float().reshape(-1, 3).contiguous(),
                                    None, half)
            assert got.dtype == torch.float32 and torch.equal(got, want.float().view(-1, 3)), (frame, N, backdrop)
    # every pixel in order (evaluation), the last frame
    want = TG.reference_targets(held[2:3].clone(), 1, "srgb").float().view(-1, 3)
    assert torch.equal(TG.gather_targets(store, 2 * n_pix, n_pix, None, None, None, half), want)


@pytest.mark.parametrize("C", [3, 4])
def test_targets_in_linear_space_look_the_table_up(device, C):
    H, W = 33, 31
    n_pix = H * W
    store, codes, values = make_store(H, W, C, torch.uint8, device, seed=1)
    table = TG.code_table(linear=True).to(device)
    assert float(table[0]) == 0.0 and float(table[255]) == 1.0 and float(table[10]) == float(np.float32(10 / 255) / np.float32(12.92))
    for N in SIZES:
        inds = pixel_ids(N, n_pix, device, N)
        picked = codes[2][inds].long()
        images = torch.cat([table[picked[:, :3]], values[2][inds][:, 3:]], -1)[None]        # alpha is never converted
        bg = torch.rand(1, N, 3, device=device)
        want = TG.reference_targets(images, bg, "srgb")                                      # (the colours are linear already)
        got = TG.gather_targets(store, 2 * n_pix, n_pix, inds, bg.reshape(-1, 3).contiguous(), table, False)
        assert torch.equal(got, want.view(-1, 3)), N
    with pytest.raises(RuntimeError, match="uint8 store"):
        TG.gather_targets(values.contiguous(), 0, n_pix, None, None, table, False)


def test_image_store_and_pixel_batch_serve_both_forms(device):
    H, W, C = 5, 7, 4
    _, codes, values = make_store(H, W, C, torch.uint8, device, seed=2)
    for half in (False, True):
        store = TG.ImageStore(codes, H, W, half=half)
        assert tuple(store.shape) == (3, H, W, C) and store.nbytes() == 3 * H * W * C
        held = values.half() if half else values
        assert torch.equal(store[[1]], held[1:2].view(1, H, W, C)) and store[[1]].dtype == store.dtype
        inds = pixel_ids(65, H * W, device, 3)[None]
        batch = TG.PixelBatch(store, 1, inds, device)
        assert tuple(batch.shape) == (1, 65, C)
        bg = torch.rand(1, 65, 3, device=device, dtype=store.dtype)
        want = TG.reference_targets(batch.materialize(), bg, "srgb").float()
        assert torch.equal(TG.training_targets(batch, bg, "srgb"), want)
        frame = TG.PixelBatch(store, 2, None, device)
        assert tuple(frame.shape) == (1, H, W, C)
        assert torch.equal(TG.training_targets(frame, None, "srgb"), TG.reference_targets(frame.materialize(), 1, "srgb").float())
        host = TG.PixelBatch(TG.ImageStore(codes.cpu(), H, W, half=half), 1, inds, device)                 # not preloaded: one frame moves
        assert torch.equal(TG.training_targets(host, bg, "srgb"), want)


def test_pixel_ids_outside_the_frame_read_nothing(device):
    store, _, _ = make_store(5, 7, 4, torch.uint8, device)
    inds = torch.tensor([0, -1, 35, 34, 1 << 40], device=device)
    got = TG.gather_targets(store, 2 * 35, 35, inds, None, None, False)
    assert torch.isnan(got[[1, 2, 4]]).all() and not torch.isnan(got[[0, 3]]).any()
    with pytest.raises(RuntimeError, match="outside the image store"):
        TG.gather_targets(store, 3 * 35, 35, None, None, None, False)


def _loss_inputs(N, dtype, device):
    g = torch.Generator().manual_seed(N)
    pred = torch.rand(N, 3, generator=g).to(dtype).to(device)
    gt = torch.rand(N, 3, generator=g).to(device)
    return pred, gt


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_photo_loss_against_float64(device, dtype):
    lib = _lib.lib()
    assert lib.ngp_photo_loss_workspace(16384) == 0 and lib.ngp_photo_loss_workspace(16385) == 257 * 4
    for N in SIZES:
        pred, gt = _loss_inputs(N, dtype, device)
        d = pred.double() - gt.double()
        want_ray = (d * d).sum(-1) / 3
        map_len = max(128 * 128, N + 5)
        row = torch.rand(map_len, device=device)
        before = row.clone()
        inds_coarse = torch.randperm(map_len, device=device)[:N]          # distinct, as multinomial(replacement=False) draws them
        per_ray, mean = TG.photo_loss_forward(pred, gt, row, inds_coarse)
        assert ulps(per_ray.cpu().numpy(), want_ray.cpu().numpy()).max() <= 4, N          # three adds and a divide
        # the sum: N * 2^-24 relative is the worst case of any fp32 order over non-negative terms (here: of the per-ray values it adds)
        terms = per_ray.double().mean().item()
        assert abs(mean.item() - terms) <= N * 2.0 ** -24 * terms, N
        assert abs(mean.item() - want_ray.mean().item()) <= (N * 2.0 ** -24 + 4 * 2.0 ** -23) * want_ray.mean().item(), N     # + the terms' own 4 ulp
        # the chain on the same device agrees within the same bound
        chain = TG.reference_loss(torch.nn.MSELoss(reduction="none"), pred.float()[None], gt[None])
        assert abs(mean.item() - chain.item()) <= 2 * N * 2.0 ** -24 * terms + 4 * 2.0 ** -23 * terms, N
        per_ray2, mean2 = TG.photo_loss_forward(pred, gt)
        assert torch.equal(mean, mean2) and torch.equal(per_ray, per_ray2), N              # the same bits run to run
        # error map: row[i] = 0.1 * row[i] + 0.9 * loss on the touched entries, all others untouched
        touched = torch.zeros(map_len, dtype=torch.bool, device=device)
        touched[inds_coarse] = True
        assert torch.equal(row[~touched], before[~touched]), N
        want_row = 0.1 * before.double()[inds_coarse] + 0.9 * want_ray
        assert ulps(row[inds_coarse].cpu().numpy(), want_row.cpu().numpy()).max() <= 4, N
        assert row._version > before._version


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_photo_loss_gradient_with_the_scale_on_the_device(device, dtype):
    for N in SIZES:
        pred, gt = _loss_inputs(N, dtype, device)
        g = torch.tensor(65536.0, device=device)
        grad = TG.photo_loss_backward(pred, gt, g)
        assert grad.dtype == dtype and grad.shape == pred.shape
        want = 65536.0 * 2 * (pred.double() - gt.double()) / (3 * N)
        if dtype == torch.float16:       # (|pred - gt| < 1: 65536 * 2 / 3 still fits a half)
            assert torch.isfinite(grad).all()
            assert ulps(grad.float().cpu().numpy(), want.cpu().numpy(), np.float16).max() <= 4, N
        else:
            assert ulps(grad.cpu().numpy(), want.cpu().numpy()).max() <= 4, N
    # through autograd, as the Trainer uses it: GradScaler's scaled loss seeds the node with a device scalar
    pred, gt = _loss_inputs(4097, torch.float32, device)
    pred.requires_grad_(True)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    loss = TG.photometric_loss(pred[None], gt[None])
    assert loss.shape == () and loss.dtype == torch.float32
    scaler.scale(loss).backward()
    assert torch.equal(pred.grad, TG.photo_loss_backward(pred.detach(), gt, torch.tensor(65536.0, device=device)))
    chain_pred = pred.detach().clone().requires_grad_(True)
    scaler.scale(TG.reference_loss(torch.nn.MSELoss(reduction="none"), chain_pred[None], gt[None])).backward()
    assert ulps(pred.grad.cpu().numpy(), chain_pred.grad.double().cpu().numpy()).max() <= 8      # each within 4 ulp of float64


def test_bad_arguments_are_refused(device):
    pred, gt = _loss_inputs(8, torch.float32, device)
    with pytest.raises(RuntimeError, match="inds_coarse"):
        TG.photo_loss_forward(pred, gt, torch.zeros(16, device=device), None)
    with pytest.raises(RuntimeError):
        TG.photometric_loss(pred, gt.half())
    lib = _lib.lib()
    assert lib.ngp_photo_loss_forward(_lib.ptr(pred), 0, _lib.ptr(gt), 20000, _lib.ptr(pred), _lib.ptr(pred), None, 0, None, None, 0, None) == -3
    assert b"workspace too small" in lib.ngp_last_error()
    assert lib.ngp_train_targets(_lib.ptr(pred), 0, 5, 0, 8, None, 8, None, None, 0, _lib.ptr(gt), None) == -1
