"""Trainer + NeRFDataset end to end on the GPU: the workload of test_training_gpu.py::test_student_fits_the_scene (a student network
fitted to 8 teacher views of the synthetic scene at 64x64), served from a blender-format folder written by write_blender_dataset."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
TRAIN_VIEWS = list(range(0, 200, 25))          # train_demo.run's eight views
HELD_OUT = [12, 112]


def _options(path):
    # (the render options train_demo.run renders with: dt_gamma 0, max_steps 1024; opt.iters at main_nerf's default, so the scheduler barely moves)
    return SimpleNamespace(path=path, preload=True, scale=1.0, offset=[0, 0, 0], bound=2, fp16=True, num_rays=1024, rand_pose=-1, error_map=False,
                           color_space="srgb", update_extra_interval=16, iters=30000, cuda_ray=True, dt_gamma=0, max_steps=1024)


@pytest.fixture(scope="module")
def dataset(device, tmp_path_factory):
    from nerfsafetyvalidation_amd.nerf.provider import write_blender_dataset
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    from nerfsafetyvalidation_amd.scene import CAMERA_ANGLE_X, StonehengeScene
    sc = StonehengeScene(H=H, W=H, bound=2)
    teacher = sc.build_model(device)
    root = str(tmp_path_factory.mktemp("henge"))
    poses = torch.from_numpy(sc.poses).to(device)
    for split, views in (("train", TRAIN_VIEWS), ("val", HELD_OUT)):
        frames = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for v in views:
                r = get_rays(poses[v:v + 1], sc.intrinsics, H, H)
                image = teacher.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False)["image"].float()[0]
                frames.append((image.clamp(0, 1) * 255).round().to(torch.uint8).view(H, H, 3).cpu().numpy())
        write_blender_dataset(root, sc.poses[views], np.stack(frames), CAMERA_ANGLE_X, split)
    return sc, root


def _student(sc, device):
    student = sc.build_model(device, table_seed=1)
    student.encoder.reset_parameters()
    student.reset_extra_state()
    return student


def _trainer(sc, root, device, workspace, **kw):
    from nerfsafetyvalidation_amd.nerf.provider import NeRFDataset
    from nerfsafetyvalidation_amd.nerf.trainer import Trainer
    from nerfsafetyvalidation_amd.nerf.utils import PSNRMeter
    from nerfsafetyvalidation_amd.optim import Adam
    opt = _options(root)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    args = dict(device=device, workspace=workspace, optimizer=lambda m: Adam(m.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-15),
                criterion=torch.nn.MSELoss(reduction="none"), ema_decay=0.95, fp16=True, metrics=[PSNRMeter()], use_loss_as_metric=False,
                best_mode="max", lr_scheduler=lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda it: 0.1 ** min(it / opt.iters, 1)),
                scheduler_update_every_step=True, use_checkpoint="scratch", eval_interval=1000, mute=True, use_tensorboardX=False)
    args.update(kw)
    trainer = Trainer("ngp", opt, _student(sc, device), **args)
    train_loader = NeRFDataset(opt, device, type="train").dataloader()
    valid_loader = NeRFDataset(opt, device, type="val").dataloader()
    return trainer, train_loader, valid_loader


@pytest.fixture(scope="module")
def trained(device, dataset, tmp_path_factory):
    sc, root = dataset
    trainer, train_loader, valid_loader = _trainer(sc, root, device, str(tmp_path_factory.mktemp("workspace")))
    store = train_loader._data.images
    assert store.data.dtype == torch.uint8 and store.data.is_cuda and tuple(store.data.shape) == (8, H * H, 3) and store.half
    trainer.train(train_loader, valid_loader, 15)                  # 15 epochs x 8 frames = 120 steps
    return trainer, train_loader, valid_loader


def test_trainer_fits_the_scene(trained):
    trainer, _, _ = trained
    losses = trainer.stats["loss"]
    print("epoch losses", losses)
    assert trainer.epoch == 15 and trainer.global_step == 120 and len(losses) == 15
    assert all(l == l for l in losses)                             # no NaN
    assert losses[-1] < 0.1 * losses[0], (losses[0], losses[-1])  # the bar test_student_fits_the_scene holds this workload to
    assert trainer.model.iter_density == 8                         # steps 0, 16, ..., 112
    assert trainer.model.mean_count > 0 and trainer.ema.num_updates == 15
    assert abs(trainer.optimizer.param_groups[0]["lr"] - 1e-2 * 0.1 ** (120 / 30000)) < 1e-12


def test_evaluate_reports_the_psnr_and_writes_the_frames(device, trained):
    from PIL import Image
    from nerfsafetyvalidation_amd.nerf.targets import code_table
    trainer, _, valid_loader = trained
    n_before = len(trainer.stats["results"])
    trainer.evaluate(valid_loader, name="held_out")
    assert len(trainer.stats["results"]) == n_before + 1
    psnrs = []
    trainer.model.eval()
    trainer.ema.store()
    trainer.ema.copy_to()
    with torch.no_grad():
        for i, data in enumerate(valid_loader, 1):
            with torch.autocast("cuda", dtype=torch.float16):
                pred, depth, gt, loss = trainer.eval_step(data)
            assert pred.shape == (1, H, H, 3) and gt.shape == (1, H, H, 3) and depth.shape == (1, H, H)
            p64, g64 = pred.double().cpu().numpy(), gt.double().cpu().numpy()
            psnrs.append(-10 * np.log10(np.mean((p64 - g64) ** 2)))
            assert abs(loss.item() - np.mean((p64 - g64) ** 2)) <= (H * H * 2.0 ** -24 + 2.0 ** -21) * np.mean((p64 - g64) ** 2)
            png = np.array(Image.open(os.path.join(trainer.workspace, "validation", f"held_out_{i:04d}_rgb.png")))
            assert np.array_equal(png, (pred[0].float().cpu().numpy() * 255).astype(np.uint8))
            # the evaluation's targets: the stored frame on white, code / 255 (held in half where the reference holds half)
            codes = valid_loader._data.images.data[i - 1].view(H, H, 3)
            assert torch.equal(gt[0], code_table().to(device)[codes.long()].half().float())
    trainer.ema.restore()
    print("held-out PSNR", psnrs)
    assert abs(-trainer.stats["results"][-1] - np.mean(psnrs)) < 1e-4          # best_mode 'max' stores -PSNR
    assert all(np.isfinite(psnrs))


def test_fused_and_torch_targets_agree_on_the_first_steps(device, dataset, tmp_path):
    from nerfsafetyvalidation_amd.nerf import targets
    sc, root = dataset
    runs = {}
    assert targets.fused_targets is True
    for fused in (True, False):
        targets.fused_targets = fused
        try:
            trainer, train_loader, _ = _trainer(sc, root, device, str(tmp_path / f"fused_{fused}"))
            from nerfsafetyvalidation_amd.nerf.targets import PixelBatch
            torch.manual_seed(1)
            assert isinstance(next(iter(train_loader))["images"], PixelBatch) == fused
            torch.manual_seed(1)
            torch.cuda.manual_seed(1)
            trainer.epoch = 1
            trainer.train_one_epoch(train_loader)
            runs[fused] = trainer.last_epoch_losses
        finally:
            targets.fused_targets = True
    print("fused", runs[True][:3], "torch chain", runs[False][:3])
    for a, b in zip(runs[True][:3], runs[False][:3]):
        assert abs(a - b) <= 1024 * 2.0 ** -24 * b, (runs[True][:3], runs[False][:3])


def test_checkpoint_loads_into_a_fresh_model_and_renders_the_same_frame(device, dataset, trained):
    from nerfsafetyvalidation_amd import checkpoint as CK
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    sc, _ = dataset
    trainer, _, _ = trained
    files = sorted(glob.glob(os.path.join(trainer.ckpt_path, "ngp_ep*.pth")))
    assert [os.path.basename(f) for f in files] == ["ngp_ep0014.pth", "ngp_ep0015.pth"]      # max_keep_ckpt = 2
    fresh = sc.build_model(device, table_seed=2)
    missing, unexpected, meta = CK.load_checkpoint(fresh, files[-1])
    assert not missing and not unexpected and meta["epoch"] == 15 and meta["global_step"] == 120
    full = CK._read(files[-1])
    assert {"optimizer", "lr_scheduler", "scaler", "ema", "mean_count", "mean_density"} <= set(full)
    rays = get_rays(torch.from_numpy(sc.poses[40:41]).to(device), sc.intrinsics, H, H)
    images = []
    for model in (trainer.model, fresh):
        model.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            images.append(model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1, perturb=False)["image"])
    assert torch.equal(images[0], images[1]) and float(images[0].float().std()) > 0
