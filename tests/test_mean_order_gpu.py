"""The fixed-order mean (DESIGN.md "Cross-lane arithmetic"; csrc/wave_ops.hpp final_mean, csrc/train_data.hip mean_of_rays) against a
numpy function that performs the documented additions in the documented order.  Both users -- ngp_photo_loss_forward's mean and
ngp_distortion_forward's loss -- must equal it BIT FOR BIT when it is given their own per-ray output.  Sizes: around a wave (63 / 64 /
65), one more than the workgroups of the kernels (257, 1025), 4097, and both sides of the 16384-ray threshold between the
one-workgroup and the two-launch form."""
import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import _lib

SIZES = (1, 63, 64, 65, 257, 1025, 4097, 16385) + (16384,)


def butterfly(v):
    """xor butterfly over the last axis (64 lanes), offsets 32 .. 1, in v's dtype: every lane ends with the total"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v


def documented_mean(values):
    """float32 [N] -> float32 scalar, the order of DESIGN.md "Cross-lane arithmetic" """
    values = np.asarray(values, dtype=np.float32)
    N = values.size
    n_groups = (N + 63) // 64
    padded = np.zeros(n_groups * 64, dtype=np.float32)
    padded[:N] = values
    groups = butterfly(padded.reshape(n_groups, 64))[:, 0]                  # (1) float32 butterfly over each group of 64
    assert groups.dtype == np.float32
    acc = np.zeros(64, dtype=np.float64)
    for start in range(0, n_groups, 64):                                    # (2) lane l adds groups l, l + 64, ... in float64, in that order
        part = groups[start:start + 64].astype(np.float64)
        acc[:part.size] = acc[:part.size] + part
    total = butterfly(acc)[0]                                               # (3) the same butterfly in float64
    return np.float32(total / np.float64(N))                                # (4) / N, rounded to float32


def test_documented_mean_is_a_mean():
    """the emulation itself, on the CPU: a plain float64 mean to within float32 rounding.  Non-negative terms: the float32 butterfly
    of a group is off by at most 6 roundings (6 * 2^-24 relative), the float64 steps by far less, the final rounding by 2^-24."""
    rng = np.random.default_rng(0)
    for N in SIZES:
        values = rng.random(N, dtype=np.float32) ** 2
        want = values.astype(np.float64).mean()
        got = documented_mean(values)
        assert got.dtype == np.float32
        assert abs(float(got) - want) <= 8 * 2.0 ** -24 * want, N
    assert documented_mean(np.full(64, 3.0, dtype=np.float32)) == np.float32(3.0)
    # the order is the one written down: a float32 butterfly of 2^24, 1, 1, 0, ... loses what a float64 sum keeps
    v = np.zeros(64, dtype=np.float32)
    v[0], v[32], v[16] = 2.0 ** 24, 1.0, 1.0                                # step 32: lane 0 = 2^24 + 1 -> 2^24 (ties to even); step 16: + 1 again
    assert documented_mean(v) == np.float32(2.0 ** 24 / 64) != np.float32((2.0 ** 24 + 2) / 64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_photo_loss_mean_has_the_documented_order(device, dtype):
    from nerfsafetyvalidation_amd.nerf import targets as TG
    for N in SIZES:
        g = torch.Generator().manual_seed(N)
        pred = torch.rand(N, 3, generator=g).to(dtype).to(device)
        gt = torch.rand(N, 3, generator=g).to(device)
        per_ray, mean = TG.photo_loss_forward(pred, gt)
        want = documented_mean(per_ray.cpu().numpy())
        assert mean.cpu().numpy().reshape(()).view(np.uint32) == want.view(np.uint32), (N, mean.item(), float(want))


@pytest.mark.gpu
def test_distortion_mean_has_the_documented_order(device):
    lib = _lib.lib()
    T = 5
    for N in SIZES:
        g = torch.Generator().manual_seed(N)
        w = (torch.rand(N, T, generator=g) / T).to(device).contiguous()
        m = torch.rand(N, T, generator=g).sort(dim=1).values.to(device).contiguous()
        row = torch.arange(N, dtype=torch.int32, device=device)
        rays = torch.stack([row, row * T, torch.full_like(row, T)], dim=1).contiguous()
        loss_rays = torch.zeros(N, dtype=torch.float32, device=device)
        totals = torch.zeros(N, 2, dtype=torch.float32, device=device)
        loss = torch.zeros((), dtype=torch.float32, device=device)
        nbytes = lib.ngp_distortion_workspace(N)
        assert nbytes == lib.ngp_photo_loss_workspace(N) == (0 if N <= 16384 else (N + 63) // 64 * 4), N
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
        _lib.check(lib.ngp_distortion_forward(_lib.ptr(w), _lib.ptr(m), None, 1.0 / T, _lib.ptr(rays), N * T, N, _lib.ptr(loss_rays),
                                              _lib.ptr(totals), _lib.ptr(loss), _lib.ptr(ws), nbytes, _lib.stream()), "distortion_forward")
        per_ray = loss_rays.cpu().numpy()
        assert per_ray.max() > 0.0, N
        want = documented_mean(per_ray)
        assert loss.cpu().numpy().reshape(()).view(np.uint32) == want.view(np.uint32), (N, loss.item(), float(want))
