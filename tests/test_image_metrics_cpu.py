"""uncertainty/evaluation on the CPU: the host path of image_quality against the reference's modules (tests/golden/image_metrics.npz,
which pins their masking and averaging), closed forms for the SSIM core, the confusion-matrix scores, the --ssim flag and SSIMMeter in a
Trainer evaluation.  No GPU.  The oracle is this directory's own float64 restatement (image_metrics_cases.py), never the package."""
import os
import warnings

import numpy as np
import pytest
import torch

import image_metrics_cases as IC
from nerfsafetyvalidation_amd.uncertainty import evaluation as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag", ["none", "binary", "weights"])
def test_host_path_reproduces_the_reference_modules(tag):
    f = np.load(os.path.join(GOLDEN, "image_metrics.npz"))
    preds, target = torch.from_numpy(f["preds"]), torch.from_numpy(f["target"])
    assert preds.dtype == torch.float32 and preds.shape == (2, 3, 17, 23)
    mask = None if tag == "none" else torch.from_numpy(f[f"mask_{tag}"]).double()
    psnr = E.PSNRModule()(preds.double(), target.double(), mask)
    ssim = E.calculate_ssim(preds.double(), target.double(), mask)
    assert psnr.shape == ssim.shape == (2,) and psnr.dtype == torch.float64
    assert np.abs(psnr.numpy() - f[f"psnr_{tag}"]).max() <= 1e-6
    assert np.abs(ssim.numpy() - f[f"ssim_{tag}"]).max() <= 1e-6
    # and the fixture's SSIM core is the one this directory restates
    want = IC.restated(preds, target, None if mask is None else mask[:, 0])
    assert np.abs(want["ssim"].numpy() - f[f"ssim_{tag}"]).max() <= IC.F64_CANCELLATION and np.abs(want["psnr"].numpy() - f[f"psnr_{tag}"]).max() <= 1e-9


@pytest.mark.parametrize("shape", [(6, 6), (17, 23)])
def test_constant_images_have_the_closed_form_everywhere(shape):
    """p = a, t = b: both variances and the covariance vanish, so every pixel -- borders included -- is (2ab + c1) / (a^2 + b^2 + c1):
    the reflect padding supplies every tap and the window sums to one."""
    a, b = 0.3, 0.8
    p, t = torch.full((1, 3) + shape, a, dtype=torch.float64), torch.full((1, 3) + shape, b, dtype=torch.float64)
    out = E.image_quality(p, t, return_map=True)
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    assert out["ssim_map"].shape == (1,) + shape
    assert (out["ssim_map"] - want).abs().max() <= IC.F64_CANCELLATION and abs(out["ssim"].item() - want) <= IC.F64_CANCELLATION
    assert abs(out["psnr"].item() - 10 * np.log10(1 / (a - b) ** 2)) <= 1e-9


def test_identical_images_give_one_and_infinite_psnr():
    p, _ = IC.make_images(9, 14)
    out = E.image_quality(p.double(), p.double().clone(), return_map=True)
    # var_p, var_t and cov are one and the same number, up to the clamp: where rounding leaves it at -1e-17, the variances are 0 and the
    # covariance is not, against c2 = 9e-4 -- a map within IC.F64_CANCELLATION of one, not bit-equal to it
    assert (out["ssim_map"] - 1).abs().max() <= IC.F64_CANCELLATION and out["ssim_map"].shape == (2, 9, 14)
    assert (out["ssim"] - 1).abs().max() <= IC.F64_CANCELLATION
    assert torch.isposinf(out["psnr"]).all() and torch.equal(out["mse"], torch.zeros(2, 3, dtype=torch.float64))


def test_layouts_and_map_agree_with_the_restatement():
    p, t = IC.make_images(13, 11)
    want = IC.restated(p, t)
    a = E.image_quality(p.double(), t.double(), return_map=True)
    b = E.image_quality(p.double().permute(0, 2, 3, 1).contiguous(), t.double().permute(0, 2, 3, 1).contiguous(), channels_last=True, return_map=True)
    assert (a["ssim_map"] - want["ssim_map"]).abs().max() <= IC.F64_CANCELLATION       # two float64 evaluations of one recipe
    for k in ("ssim", "psnr", "mse", "ssim_map"):
        assert torch.equal(a[k], b[k]) or (torch.isinf(a[k]) == torch.isinf(b[k])).all()


def test_too_small_frames_and_bad_shapes_raise():
    with pytest.raises(ValueError, match="reflect"):
        E.image_quality(torch.rand(1, 3, 5, 9), torch.rand(1, 3, 5, 9))
    with pytest.raises(ValueError, match="reflect"):
        E.SSIMModule()(torch.rand(1, 3, 9, 5), torch.rand(1, 3, 9, 5))
    with pytest.raises(ValueError):
        E.image_quality(torch.rand(1, 4, 8, 8), torch.rand(1, 4, 8, 8))
    with pytest.raises(ValueError, match="data_range"):
        E.image_quality(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8), data_range=0.0)


def test_all_zero_mask_gives_nan():
    p, t = IC.make_images(8, 8)
    mask = torch.zeros(2, 1, 8, 8)
    assert torch.isnan(E.SSIMModule()(p, t, mask)).all()
    assert torch.isnan(E.PSNRModule()(p, t, mask)).all()


def test_confusion_matrix_scores():
    y_true = np.array([1, 1, 1, 0, 0, 0, 0, 1])
    y_pred = np.array([1, 0, 1, 1, 0, 0, 0, 1])          # tp 3, fn 1, fp 1, tn 3
    assert E.calculate_accuracy(y_true, y_pred) == 6 / 8
    assert E.calculate_precision(y_true, y_pred) == 3 / 4
    assert E.calculate_recall(y_true, y_pred) == 3 / 4
    assert E.calculate_f1_score(y_true, y_pred) == pytest.approx(2 * (0.75 * 0.75) / 1.5, abs=1e-15)
    y_pred2 = np.array([1, 1, 1, 1, 0, 0, 1, 0])          # tp 3, fn 1, fp 2
    assert E.calculate_precision(y_true, y_pred2) == 3 / 5 and E.calculate_recall(y_true, y_pred2) == 3 / 4
    assert E.calculate_f1_score(y_true, y_pred2) == pytest.approx(2 * 0.6 * 0.75 / 1.35, abs=1e-15)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(E.calculate_precision(y_true, np.zeros(8, dtype=int)))   # nothing predicted positive: 0 / 0, not guarded


def test_lpips_says_what_is_missing():
    with pytest.raises(NotImplementedError, match="weights"):
        E.LPIPSModule()(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="weights"):
        E.calculate_lpips(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))


def test_ssim_flag():
    from nerfsafetyvalidation_amd.main_nerf import parse_args
    assert parse_args(["data", "--ssim"]).ssim is True
    assert parse_args(["data"]).ssim is False and parse_args(["data", "-O"]).ssim is False


def test_trainer_evaluation_reports_ssim_after_psnr(tmp_path):
    """A Trainer with [PSNRMeter(), SSIMMeter()] on tests/golden/blender_tiny (set up as test_trainer_cpu.py's): an `SSIM =` line in the
    log, stats["results"] still the PSNR, and the SSIM equal to the float64 restatement on the same predictions."""
    from test_trainer_cpu import StubModel, make_trainer
    from nerfsafetyvalidation_amd.nerf import provider as P
    from nerfsafetyvalidation_amd.nerf.utils import PSNRMeter, SSIMMeter

    seen = []

    class Recorder(SSIMMeter):
        def update(self, preds, truths):
            seen.append((preds.detach().clone(), truths.detach().clone()))
            super().update(preds, truths)

    model = StubModel()
    trainer, opt = make_trainer(tmp_path, model, metrics=[PSNRMeter(), Recorder()], use_checkpoint="scratch", use_loss_as_metric=False)
    loader = P.NeRFDataset(opt, "cpu", type="val").dataloader()
    trainer.evaluate(loader)

    assert len(seen) >= 1 and all(p.shape == t.shape and p.shape[-1] == 3 and p.dim() == 4 for p, t in seen)
    ssims, ssims32, psnrs = [], [], []
    for p, t in seen:
        want = IC.restated(p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2))
        ssims += want["ssim"].tolist()
        ssims32 += IC.restated(p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), dtype=torch.float32)["ssim"].tolist()
        psnrs.append(-10 * np.log10(np.mean((p.numpy() - t.numpy()) ** 2)))          # PSNRMeter's formula
    log = open(trainer.log_path).read()
    lines = [ln for ln in log.splitlines() if ln.startswith(("PSNR = ", "SSIM = "))]
    assert [ln[:4] for ln in lines] == ["PSNR", "SSIM"]                               # PSNR first, then SSIM
    got_ssim = float(lines[1].split("=")[1])
    # float32 frames go through the host path at float32: twice what the float32 restatement is off by, one float32 ulp of 1 for the
    # order of the sums, and half a unit of the sixth printed digit
    bound = 2 * abs(np.mean(ssims32) - np.mean(ssims)) + 2.0 ** -23
    print(f"trainer SSIM {got_ssim}, float64 restatement {np.mean(ssims)!r}, float32 restatement off by {abs(np.mean(ssims32) - np.mean(ssims)):.3e}")
    assert abs(got_ssim - np.mean(ssims)) <= bound + 5e-7
    assert len(trainer.stats["results"]) == 1 and trainer.stats["results"][0] == pytest.approx(np.mean(psnrs), abs=1e-9)
    assert float(lines[0].split("=")[1]) == pytest.approx(np.mean(psnrs), abs=1e-6)

    # the meter on its own: same frames, both numbers, and clear() starts over
    meter = SSIMMeter()
    for p, t in seen:
        meter.update(p, t)
    assert abs(meter.measure() - np.mean(ssims)) <= bound and abs(meter.measure_psnr() - np.mean(psnrs)) <= 1e-4
    assert meter.report() == f"SSIM = {meter.measure():.6f}"

    class Writer:
        def add_scalar(self, *a):
            self.got = a

    w = Writer()
    meter.write(w, 7, prefix="evaluate")
    assert w.got == (os.path.join("evaluate", "SSIM"), meter.measure(), 7)
    meter.clear()
    assert meter.N == 0 and meter.U == 0
