"""ngp_image_quality (csrc/image_metrics.hip) and what is built on it, on the MI355X, against this directory's own float64 restatement
of the recipe (image_metrics_cases.py: reflect pad + one 121-tap grouped conv2d on the CPU).

The accuracy gate: the float32 form of the same restatement is the yardstick -- it is the arithmetic the reference runs -- and the
kernel may be off from float64 by at most twice what the yardstick is off by ON THE SAME INPUT (the factor allows for another
summation order).  PSNR: within 1e-5 dB of float64 (a float32 difference carries <= 1.8e-7 relative error per term after squaring, the
sums are double: 10 / ln 10 x 1.8e-7 = 8e-7 dB, and a factor of about ten over that).

Shapes (tile = 16 x 32): 6 x 6 both halos reflect inside one tile; 17 x 70 shorter than a tile and wider than one with a remainder;
45 x 33 mixed; 71 x 133 several tiles and a remainder both ways.

Observed on an MI355X, max |map - float64| kernel / float32 yardstick: 6x6 2.86e-8 / 1.17e-4, 17x70 2.98e-8 / 1.39e-4, 45x33 2.98e-8 /
1.43e-4, 71x133 2.98e-8 / 1.78e-4, constant images 1.50e-8 / 2.39e-4; per-image SSIM 4.9e-13 / 2.1e-5 .. 2.7e-5; PSNR at most 1.4e-9 dB
from float64 on the raw sums, 8.0e-7 dB through the float32 modules; measure_psnr() - PSNRMeter 1.9e-6 dB (DESIGN.md "Image-quality
metrics")."""
import functools
import os

import numpy as np
import pytest
import torch

import image_metrics_cases as IC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(6, 6), (17, 70), (45, 33), (71, 133)]
PSNR_TOL_DB = 1e-5


@functools.lru_cache(maxsize=None)
def case(H, W):
    """images, masks, and the float64 / float32 restatements (computed once per shape on the CPU and shared, never modified)"""
    pred, target = IC.make_images(H, W)
    gen = torch.Generator().manual_seed(100 + H)
    binary = (torch.rand(2, H, W, generator=gen) < 0.5).float()
    weights = torch.rand(2, H, W, generator=gen)
    assert binary.sum((1, 2)).min() > 0
    masks = {"none": None, "binary": binary, "weights": weights}
    ref = {k: IC.restated(pred, target, m, torch.float64) for k, m in masks.items()}
    yard = {k: IC.restated(pred, target, m, torch.float32) for k, m in masks.items()}
    return pred, target, masks, ref, yard


def run(E, device, pred, target, mask=None, **kw):
    out = E.image_quality(pred.to(device), target.to(device), None if mask is None else mask.to(device), return_map=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def psnr_close(got, want):
    """inf where the reference is inf (an identical channel), within PSNR_TOL_DB elsewhere"""
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    return bool(torch.equal(torch.isposinf(got), torch.isposinf(want)) and ((got[fin] - want[fin]).abs() <= PSNR_TOL_DB).all())


@pytest.fixture(scope="module")
def E(device):
    from nerfsafetyvalidation_amd.uncertainty import evaluation
    return evaluation


@pytest.mark.parametrize("H,W", SHAPES)
def test_map_and_sums_against_float64(E, device, H, W):
    pred, target, masks, ref, yard = case(H, W)
    for tag, mask in masks.items():
        got = run(E, device, pred, target, mask)
        assert got["ssim_map"].dtype == torch.float32 and got["ssim_map"].shape == (2, H, W) and got["ssim"].dtype == torch.float64
        err_k = (got["ssim_map"].double() - ref[tag]["ssim_map"]).abs().max().item()
        err_y = (yard[tag]["ssim_map"].double() - ref[tag]["ssim_map"]).abs().max().item()
        s_k = (got["ssim"] - ref[tag]["ssim"]).abs().max().item()
        s_y = (yard[tag]["ssim"].double() - ref[tag]["ssim"]).abs().max().item()
        p_k = (got["psnr"] - ref[tag]["psnr"])[torch.isfinite(ref[tag]["psnr"])].abs().max().item()
        print(f"image_quality {H}x{W} mask={tag}: map range [{ref[tag]['ssim_map'].min():.3f}, {ref[tag]['ssim_map'].max():.3f}]  "
              f"max|map - f64| kernel {err_k:.3e} / float32 restatement {err_y:.3e};  per-image ssim kernel {s_k:.3e} / float32 {s_y:.3e};  "
              f"psnr {p_k:.3e} dB")
        assert err_k <= 2 * err_y
        assert s_k <= 2 * s_y
        assert psnr_close(got["psnr"], ref[tag]["psnr"])
        # per channel too (the image with the identical channel has an infinite mean): the channels that differ
        want_mse = (((pred.double() - target.double()) ** 2) * (1.0 if mask is None else mask.double()[:, None])).sum((2, 3)) / (
            H * W if mask is None else mask.double().sum((1, 2))[:, None])
        nz = want_mse > 0
        assert torch.equal(got["mse"] == 0, ~nz)
        assert ((10 * torch.log10(got["mse"][nz] / want_mse[nz])).abs() <= PSNR_TOL_DB).all()


@pytest.mark.parametrize("H,W", [(6, 6), (45, 33)])
def test_constant_images_closed_form(E, device, H, W):
    a, b = 0.3, 0.8
    pred, target = torch.full((2, 3, H, W), a), torch.full((2, 3, H, W), b)
    got = run(E, device, pred, target)
    ref, yard = IC.restated(pred, target), IC.restated(pred, target, dtype=torch.float32)
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    closed = (2 * a32 * b32 + 1e-4) / (a32 * a32 + b32 * b32 + 1e-4)
    assert (ref["ssim_map"] - closed).abs().max() <= IC.F64_CANCELLATION         # the restatement has the closed form, borders included
    err_k = (got["ssim_map"].double() - ref["ssim_map"]).abs().max().item()
    err_y = (yard["ssim_map"].double() - ref["ssim_map"]).abs().max().item()
    print(f"image_quality constant {H}x{W}: max|map - f64| kernel {err_k:.3e} / float32 restatement {err_y:.3e}")
    assert err_k <= 2 * err_y
    assert (got["ssim"] - closed).abs().max() <= 2 * (yard["ssim"].double() - ref["ssim"]).abs().max()
    assert psnr_close(got["psnr"], ref["psnr"])


def test_layouts_give_identical_bits(E, device):
    pred, target, masks, _, _ = case(71, 133)
    p, t = pred.to(device), target.to(device)
    a_stats, a_map = E.image_quality_stats(p, t, masks["weights"].to(device), return_map=True)
    pl, tl = p.permute(0, 2, 3, 1).contiguous(), t.permute(0, 2, 3, 1).contiguous()          # [B,H,W,3]
    b_stats, b_map = E.image_quality_stats(pl, tl, masks["weights"].to(device)[..., None], channels_last=True, return_map=True)
    assert torch.equal(a_stats, b_stats) and torch.equal(a_map, b_map)
    assert a_stats[:, 5].tolist() == [71 * 133] * 2 and a_stats[:, 6:].abs().max() == 0
    # a channels-last MEMORY layout behind a [B,3,H,W] view is read in place as well, and float64 inputs are cast
    c_stats, _ = E.image_quality_stats(pl.permute(0, 3, 1, 2), tl.permute(0, 3, 1, 2), masks["weights"].to(device))
    assert torch.equal(a_stats, c_stats)
    d_stats, _ = E.image_quality_stats(p.double(), t.double(), masks["weights"].to(device).double()[:, None])
    assert torch.equal(a_stats, d_stats)


def test_repeatable_and_independent_of_the_batch(E, device):
    pred, target, masks, _, _ = case(45, 33)
    p, t, m = pred.to(device), target.to(device), masks["binary"].to(device)
    s1, m1 = E.image_quality_stats(p, t, m, return_map=True)
    s2, m2 = E.image_quality_stats(p, t, m, return_map=True)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    s3, m3 = E.image_quality_stats(p[1:2], t[1:2], m[1:2], return_map=True)
    assert torch.equal(s1[1:2], s3) and torch.equal(m1[1:2], m3)
    # two streams, each call with its own workspace: same bits as the default stream
    streams, outs = [torch.cuda.Stream(device), torch.cuda.Stream(device)], []
    torch.cuda.synchronize()
    for st in streams:
        with torch.cuda.stream(st):
            outs.append(E.image_quality_stats(p, t, m, return_map=True))
    torch.cuda.synchronize()
    for s, mp in outs:
        assert torch.equal(s, s1) and torch.equal(mp, m1)


def test_masks_and_optional_arguments(E, device):
    pred, target, _, _, _ = case(17, 70)
    p, t = pred.to(device), target.to(device)
    zero = E.image_quality(p, t, torch.zeros(2, 17, 70, device=device))
    assert torch.isnan(zero["ssim"]).all() and not torch.isfinite(zero["psnr"]).any()        # 0 / 0, as torch's division gives
    plain = E.image_quality(p, t)                                                            # no mask, no map
    assert "ssim_map" not in plain and torch.equal(plain["ssim"], E.image_quality(p, t, return_map=True)["ssim"])
    ones = E.image_quality(p, t, torch.ones(2, 1, 17, 70, device=device))
    assert torch.equal(ones["ssim"], plain["ssim"]) and torch.equal(ones["mse"], plain["mse"])


def test_refusals_launch_nothing(E, device):
    from nerfsafetyvalidation_amd import _lib
    lib = _lib.lib()
    p, t = torch.rand(1, 3, 8, 8, device=device), torch.rand(1, 3, 8, 8, device=device)
    stats = torch.full((1, 8), -7.0, dtype=torch.float64, device=device)
    work = torch.zeros(1024, dtype=torch.float64, device=device)
    args = lambda H, W, rng: (p.data_ptr(), t.data_ptr(), None, 1, H, W, 192, 64, 8, 1, rng, None, stats.data_ptr(), work.data_ptr(), 8192, _lib.stream())
    assert lib.ngp_image_quality(*args(5, 8, 1.0)) == -1 and b"reflect" in lib.ngp_last_error()
    assert lib.ngp_image_quality(*args(8, 5, 1.0)) == -1
    assert lib.ngp_image_quality(*args(8, 8, 0.0)) == -1 and b"data_range" in lib.ngp_last_error()
    assert lib.ngp_image_quality(p.data_ptr(), t.data_ptr(), None, 1, 8, 8, 192, 64, 8, 1, 1.0, None, None, work.data_ptr(), 8192, _lib.stream()) == -1
    assert lib.ngp_image_quality(p.data_ptr(), t.data_ptr(), None, 1, 8, 8, 192, 64, 8, 1, 1.0, None, stats.data_ptr(), work.data_ptr(), 8, _lib.stream()) == -3
    assert lib.ngp_image_quality_workspace(1, 5, 8) == 0 and lib.ngp_image_quality_workspace(2, 71, 133) == 2 * 5 * 5 * 5 * 8
    torch.cuda.synchronize()
    assert torch.equal(stats.cpu(), torch.full((1, 8), -7.0, dtype=torch.float64)) and work.abs().max() == 0      # nothing ran
    assert lib.ngp_image_quality(*args(8, 8, 1.0)) == 0
    torch.cuda.synchronize()
    assert stats[0, 5].item() == 64 and stats[0, 1].item() == 64
    with pytest.raises(ValueError, match="reflect"):
        E.image_quality(torch.rand(1, 3, 5, 8, device=device), torch.rand(1, 3, 5, 8, device=device))
    with pytest.raises(ValueError, match="data_range"):
        E.image_quality(p, t, data_range=0.0)


def test_element_offsets_are_64_bit(E, device):
    """a channel stride of 2^30 elements: channel 2 starts 2^31 elements into the buffer, past what a 32-bit offset holds"""
    H, W = 16, 40
    pred, target = IC.make_images(H, W, B=1)
    base = torch.empty(2 * 2 ** 30 + 2 * H * W, dtype=torch.float32, device=device)
    views = [torch.as_strided(base, (1, 3, H, W), (0, 2 ** 30, W, 1), storage_offset=k * H * W) for k in range(2)]
    views[0].copy_(pred.to(device))
    views[1].copy_(target.to(device))
    got = E.image_quality_stats(views[0], views[1], return_map=True)
    want = E.image_quality_stats(pred.to(device), target.to(device), return_map=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("tag", ["none", "binary", "weights"])
def test_modules_reproduce_the_reference_fixture(E, device, tag):
    f = np.load(os.path.join(GOLDEN, "image_metrics.npz"))
    preds, target = torch.from_numpy(f["preds"]), torch.from_numpy(f["target"])
    mask = None if tag == "none" else torch.from_numpy(f[f"mask_{tag}"])
    ssim = E.SSIMModule()(preds.to(device), target.to(device), None if mask is None else mask.to(device)).cpu()
    psnr = E.calculate_psnr(preds.to(device), target.to(device), None if mask is None else mask.to(device)).cpu()
    assert ssim.dtype == psnr.dtype == torch.float32 and ssim.shape == psnr.shape == (2,)
    yard = IC.restated(preds, target, None if mask is None else mask[:, 0], torch.float32)
    err_k = np.abs(ssim.double().numpy() - f[f"ssim_{tag}"]).max()
    err_y = np.abs(yard["ssim"].double().numpy() - f[f"ssim_{tag}"]).max()
    p_k = np.abs(psnr.double().numpy() - f[f"psnr_{tag}"]).max()
    print(f"modules on the fixture, mask={tag}: ssim kernel {err_k:.3e} / float32 restatement {err_y:.3e}; psnr {p_k:.3e} dB")
    assert err_k <= 2 * err_y
    assert p_k <= PSNR_TOL_DB


def test_meter_over_three_frames(device):
    from nerfsafetyvalidation_amd.nerf.utils import PSNRMeter, SSIMMeter
    meter, psnr_meter = SSIMMeter(), PSNRMeter()
    ssim64, ssim32, psnr64 = [], [], []
    for k in range(3):
        pred, target = IC.make_images(45, 33, B=1, seed=20 + k)
        ssim64.append(IC.restated(pred, target)["ssim"].item())
        ssim32.append(IC.restated(pred, target, dtype=torch.float32)["ssim"].item())
        psnr64.append(-10 * np.log10(((pred.double() - target.double()) ** 2).mean().item()))
        pl, tl = pred.permute(0, 2, 3, 1).contiguous().to(device), target.permute(0, 2, 3, 1).contiguous().to(device)
        meter.update(pl, tl)
        psnr_meter.update(pl, tl)
    assert torch.is_tensor(meter.V) and meter.V.is_cuda and meter.N == 3                   # the sums stay on the device until measure()
    err_k, err_y = abs(meter.measure() - np.mean(ssim64)), abs(np.mean(ssim32) - np.mean(ssim64))
    d_f64, d_meter = abs(meter.measure_psnr() - np.mean(psnr64)), abs(meter.measure_psnr() - psnr_meter.measure())
    print(f"SSIMMeter, 3 frames of 45x33: ssim kernel {err_k:.3e} / float32 restatement {err_y:.3e}; measure_psnr - float64 {d_f64:.3e} dB, "
          f"measure_psnr - PSNRMeter {d_meter:.3e} dB")
    assert err_k <= 2 * err_y
    assert d_f64 <= PSNR_TOL_DB
    assert d_meter <= 1e-4
    assert meter.report().startswith("SSIM = ")
    meter.clear()
    assert meter.N == 0
