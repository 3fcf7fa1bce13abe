"""Train, evaluate and test a NeRF on a posed-image dataset (reference: main_nerf.py):

    python -m nerfsafetyvalidation_amd.main_nerf PATH --workspace W -O --iters 30000

The reference's flags and their meaning (`-O` = --fp16 --cuda_ray --preload, `--ff` = the fully fused MLP).  Without the GUI
(`--gui`, `--W/--H/--radius/--fovy/--max_spp`), the TCNN backend (`--tcnn`) and CLIP guidance (`--clip_text`, `--rand_pose`)."""
import argparse

import numpy as np
import torch

from .nerf.provider import NeRFDataset
from .nerf.trainer import Trainer
from .nerf.utils import PSNRMeter, SSIMMeter, seed_everything
from .optim import Adam


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m nerfsafetyvalidation_amd.main_nerf")
    parser.add_argument('path', type=str)
    parser.add_argument('-O', action='store_true', help="equals --fp16 --cuda_ray --preload")
    parser.add_argument('--test', action='store_true', help="test mode")
    parser.add_argument('--workspace', type=str, default='workspace')
    parser.add_argument('--seed', type=int, default=0)

    ### training options
    parser.add_argument('--iters', type=int, default=30000, help="training iters")
    parser.add_argument('--lr', type=float, default=1e-2, help="initial learning rate")
    parser.add_argument('--ckpt', type=str, default='latest')
    parser.add_argument('--num_rays', type=int, default=4096, help="num rays sampled per image for each training step")
    parser.add_argument('--cuda_ray', action='store_true', help="use the occupancy-grid ray marcher instead of uniform sampling")
    parser.add_argument('--max_steps', type=int, default=1024, help="max num steps sampled per ray (only valid when using --cuda_ray)")
    parser.add_argument('--num_steps', type=int, default=512, help="num steps sampled per ray (only valid when NOT using --cuda_ray)")
    parser.add_argument('--upsample_steps', type=int, default=0, help="num steps up-sampled per ray (only valid when NOT using --cuda_ray)")
    parser.add_argument('--update_extra_interval', type=int, default=16, help="iter interval to update extra status (only valid when using --cuda_ray)")
    parser.add_argument('--max_ray_batch', type=int, default=4096, help="batch size of rays at inference (only valid when NOT using --cuda_ray)")

    ### network backbone options
    parser.add_argument('--fp16', action='store_true', help="use amp mixed precision training")
    parser.add_argument('--ff', action='store_true', help="use fully-fused MLP")
    parser.add_argument('--encoding_dir', type=str, default='sphere_harmonics', choices=['sphere_harmonics', 'frequency'],
                        help="view-direction encoding (frequency = positional encoding, degree 6; not with --ff)")

    ### dataset options
    parser.add_argument('--color_space', type=str, default='srgb', help="Color space, supports (linear, srgb)")
    parser.add_argument('--preload', action='store_true', help="keep the image store on the GPU")
    # (the default values are for the fox dataset)
    parser.add_argument('--bound', type=float, default=2, help="assume the scene is bounded in box[-bound, bound]^3, if > 1, will invoke adaptive ray marching.")
    parser.add_argument('--scale', type=float, default=0.33, help="scale camera location into box[-bound, bound]^3")
    parser.add_argument('--offset', type=float, nargs='*', default=[0, 0, 0], help="offset of camera location")
    parser.add_argument('--dt_gamma', type=float, default=1 / 128, help="dt_gamma (>=0) for adaptive ray marching. set to 0 to disable")
    parser.add_argument('--min_near', type=float, default=0.2, help="minimum near distance for camera")
    parser.add_argument('--density_thresh', type=float, default=10, help="threshold for density grid to be occupied")
    parser.add_argument('--bg_radius', type=float, default=-1, help="if positive, use a background model at sphere(bg_radius)")

    ### experimental
    parser.add_argument('--error_map', action='store_true', help="use error map to sample rays")

    ### regularisation (not in the reference's entry point; its loss.py has the term)
    parser.add_argument('--lambda_distort', type=float, default=0, help="weight of the distortion loss on the ray weights (0 = off)")

    ### depth supervision (not in the reference; DESIGN.md "Depth supervision").  The dataset names its maps with Instant-NGP's keys.
    parser.add_argument('--lambda_depth', type=float, default=0, help="weight of the depth term: the squared miss of the expected ray distance (0 = off)")
    parser.add_argument('--lambda_free', type=float, default=0, help="weight of the free-space term: the opacity in front of the measured surface (0 = off)")
    parser.add_argument('--depth_margin', type=float, default=0.02,
                        help="the free-space term ends this far in front of the surface, in scene units (0.02: about one cell of the 128^3 grid at bound 1)")

    ### evaluation (not in the reference)
    parser.add_argument('--ssim', action='store_true', help="also report SSIM at evaluation (after PSNR, which still picks the best checkpoint)")

    opt = parser.parse_args(argv)
    opt.rand_pose = -1      # (CLIP-guided training on random poses is not ported; the dataset and the Trainer read the field)

    if opt.O:
        opt.fp16 = True
        opt.cuda_ray = True
        opt.preload = True
    if opt.ff:
        opt.fp16 = True
        assert opt.bg_radius <= 0, "background model is not implemented for --ff"
        assert opt.encoding_dir == 'sphere_harmonics', "--encoding_dir frequency is not implemented for --ff (its colour input is SH-only)"
    return opt


def main(argv=None):
    opt = parse_args(argv)
    if opt.ff:
        from .nerf.network_ff import NeRFNetwork
    else:
        from .nerf.network import NeRFNetwork

    print(opt)
    seed_everything(opt.seed)

    model = NeRFNetwork(
        encoding="hashgrid",
        encoding_dir=opt.encoding_dir,
        bound=opt.bound,
        cuda_ray=opt.cuda_ray,
        density_scale=1,
        min_near=opt.min_near,
        density_thresh=opt.density_thresh,
        bg_radius=opt.bg_radius,
    )
    print(model)

    criterion = torch.nn.MSELoss(reduction='none')
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

    if opt.test:
        metrics = [PSNRMeter(), ] + ([SSIMMeter()] if opt.ssim else [])
        trainer = Trainer('ngp', opt, model, device=device, workspace=opt.workspace, criterion=criterion, fp16=opt.fp16, metrics=metrics,
                          use_checkpoint=opt.ckpt)
        test_loader = NeRFDataset(opt, device=device, type='test').dataloader()
        if test_loader.has_gt:
            trainer.evaluate(test_loader)  # blender has gt, so evaluate it.
        trainer.test(test_loader, write_video=True)
        return trainer

    optimizer = lambda model: Adam(model.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)

    train_loader = NeRFDataset(opt, device=device, type='train').dataloader()

    # decay to 0.1 * init_lr at last iter step
    scheduler = lambda optimizer: torch.optim.lr_scheduler.LambdaLR(optimizer, lambda iter: 0.1 ** min(iter / opt.iters, 1))

    metrics = [PSNRMeter(), ] + ([SSIMMeter()] if opt.ssim else [])
    trainer = Trainer('ngp', opt, model, device=device, workspace=opt.workspace, optimizer=optimizer, criterion=criterion, ema_decay=0.95,
                      fp16=opt.fp16, lr_scheduler=scheduler, scheduler_update_every_step=True, metrics=metrics, use_checkpoint=opt.ckpt,
                      eval_interval=50)

    valid_loader = NeRFDataset(opt, device=device, type='val', downscale=1).dataloader()

    max_epoch = np.ceil(opt.iters / len(train_loader)).astype(np.int32)
    trainer.train(train_loader, valid_loader, max_epoch)

    # also test
    test_loader = NeRFDataset(opt, device=device, type='test').dataloader()
    if test_loader.has_gt:
        trainer.evaluate(test_loader)  # blender has gt, so evaluate it.
    trainer.test(test_loader, write_video=True)
    return trainer


if __name__ == '__main__':
    main()
