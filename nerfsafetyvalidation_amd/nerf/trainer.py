"""Trainer (reference: nerf/utils.py:257-1059) and the EMA of the weights it evaluates with (torch_ema's published rule).

The host logic is the reference's, quirks included:
  * update_extra_state every `opt.update_extra_interval` steps under autocast, mark_untrained_grid at the start of train (cuda_ray);
  * the EMA is updated ONCE PER EPOCH, after the loop (utils.py:814-815), not per step;
  * eval_step renders staged, on white, without perturbation; `best` checkpoints hold the EMA weights and drop density_grid;
  * the error map weights the OLD value by 0.1 (utils.py:474); `render(..., **vars(opt))` splats the options.
The data side of a step (targets, loss, error map) is `targets.py`: HIP kernels on a HIP device, the reference's torch chain otherwise.

Not ported: the CLIP branch (`rand_pose >= 0`), DDP (`world_size > 1`), the GUI methods, `rich` (plain print), mp4 output
(`test(write_video=True)` writes PNG frames).  tensorboardX is used only when it can be imported.

One difference in bookkeeping: the per-step losses of an epoch are read back together at its end (`last_epoch_losses`), not one
`.item()` per step, unless a tensorboard writer or `report_metric_at_train` needs them as they come; `stats["loss"]` is the same mean."""
import os
import time

import numpy as np
import torch
import torch.nn as nn

from .. import checkpoint as _checkpoint
from . import targets
from .targets import DepthBatch, PixelBatch
from .utils import linear_to_srgb


class ExponentialMovingAverage:
    """torch_ema.ExponentialMovingAverage's rule and state keys: num_updates += 1; d = min(decay, (1 + n) / (10 + n));
    shadow -= (1 - d) * (shadow - param).  copy_to / restore write through `.data`, which no version counter sees: `invalidate`
    (the model's invalidate_fused) is called after them."""

    def __init__(self, parameters, decay, use_num_updates=True, invalidate=None):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        parameters = list(parameters)
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow_params = [p.clone().detach() for p in parameters]
        self.collected_params = None
        self._params = parameters
        self._invalidate = invalidate

    def update(self):
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        one_minus_decay = 1.0 - decay
        with torch.no_grad():
            for s_param, param in zip(self.shadow_params, self._params):
                if param.requires_grad:
                    tmp = s_param - param
                    tmp.mul_(one_minus_decay)
                    s_param.sub_(tmp)

    def _written(self):
        if self._invalidate is not None:
            self._invalidate()

    def copy_to(self):
        for s_param, param in zip(self.shadow_params, self._params):
            if param.requires_grad:
                param.data.copy_(s_param.data)
        self._written()

    def store(self):
        self.collected_params = [param.clone() for param in self._params]

    def restore(self):
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        for c_param, param in zip(self.collected_params, self._params):
            param.data.copy_(c_param.data)
        self._written()

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params,
                "collected_params": self.collected_params}

    def load_state_dict(self, state_dict):
        self.decay = state_dict["decay"]
        self.num_updates = state_dict["num_updates"]
        shadow = state_dict["shadow_params"]
        if len(shadow) != len(self._params):
            raise ValueError("shadow_params and the model's parameters differ in number")
        self.shadow_params = [s.to(device=p.device, dtype=p.dtype).clone() for s, p in zip(shadow, self._params)]
        collected = state_dict["collected_params"]
        self.collected_params = None if collected is None else [c.to(device=p.device, dtype=p.dtype).clone() for c, p in zip(collected, self._params)]


def _write_png(path, array):
    from PIL import Image
    Image.fromarray(array).save(path)


class Trainer(object):
    def __init__(self,
                 name,  # name of this experiment
                 opt,  # extra conf
                 model,  # network
                 criterion=None,  # loss function
                 optimizer=None,  # optimizer (a function of the model)
                 ema_decay=None,  # if use EMA, set the decay
                 lr_scheduler=None,  # scheduler (a function of the optimizer)
                 metrics=[],  # metrics for evaluation, if None, use val_loss to measure performance, else use the first metric.
                 local_rank=0,
                 world_size=1,
                 device=None,
                 mute=False,
                 fp16=False,  # amp optimize level
                 eval_interval=1,  # eval once every $ epoch
                 max_keep_ckpt=2,  # max num of saved ckpts in disk
                 workspace='workspace',  # workspace to save logs & ckpts
                 best_mode='min',  # the smaller/larger result, the better
                 use_loss_as_metric=True,  # use loss as the first metric
                 report_metric_at_train=False,  # also report metrics at training
                 use_checkpoint="latest",  # which ckpt to use at init time
                 use_tensorboardX=True,  # whether to use tensorboard for logging
                 scheduler_update_every_step=False,  # whether to call scheduler.step() after every train step
                 ):
        if world_size > 1:
            raise NotImplementedError("Trainer: distributed training (world_size > 1) is not ported")
        if getattr(opt, "rand_pose", -1) >= 0:
            raise NotImplementedError("Trainer: rand_pose >= 0 (the CLIP branch) is not ported")

        self.name = name
        self.opt = opt
        self.mute = mute
        self.metrics = metrics
        self.local_rank = local_rank
        self.world_size = world_size
        self.workspace = workspace
        self.ema_decay = ema_decay
        self.fp16 = fp16
        self.best_mode = best_mode
        self.use_loss_as_metric = use_loss_as_metric
        self.report_metric_at_train = report_metric_at_train
        self.max_keep_ckpt = max_keep_ckpt
        self.eval_interval = eval_interval
        self.use_checkpoint = use_checkpoint
        self.use_tensorboardX = use_tensorboardX
        self.time_stamp = time.strftime("%Y-%m-%d_%H-%M-%S")
        self.scheduler_update_every_step = scheduler_update_every_step
        self.device = device if device is not None else torch.device(f'cuda:{local_rank}' if torch.cuda.is_available() else 'cpu')
        self.device = torch.device(self.device)
        self.log_ptr = None

        model.to(self.device)
        self.model = model

        if isinstance(criterion, nn.Module):
            criterion.to(self.device)
        self.criterion = criterion

        if optimizer is None:
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=0.001, weight_decay=5e-4)  # naive adam
        else:
            self.optimizer = optimizer(self.model)

        if lr_scheduler is None:
            self.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lr_lambda=lambda epoch: 1)  # fake scheduler
        else:
            self.lr_scheduler = lr_scheduler(self.optimizer)

        if ema_decay is not None:
            self.ema = ExponentialMovingAverage(self.model.parameters(), decay=ema_decay, invalidate=getattr(self.model, "invalidate_fused", None))
        else:
            self.ema = None

        self.scaler = torch.amp.GradScaler("cuda", enabled=self.fp16)

        # variable init
        self.epoch = 0
        self.global_step = 0
        self.local_step = 0
        self.error_map = None
        self.last_epoch_losses = []
        self.stats = {
            "loss": [],
            "valid_loss": [],
            "results": [],  # metrics[0], or valid_loss
            "checkpoints": [],  # record path of saved ckpt, to automatically remove old ckpt
            "best_result": None,
        }

        # auto fix
        if len(metrics) == 0 or self.use_loss_as_metric:
            self.best_mode = 'min'

        # workspace prepare
        if self.workspace is not None:
            os.makedirs(self.workspace, exist_ok=True)
            self.log_path = os.path.join(workspace, f"log_{self.name}.txt")
            self.log_ptr = open(self.log_path, "a+")

            self.ckpt_path = os.path.join(self.workspace, 'checkpoints')
            self.best_path = f"{self.ckpt_path}/{self.name}.pth"
            os.makedirs(self.ckpt_path, exist_ok=True)

        self.log(f'[INFO] Trainer: {self.name} | {self.time_stamp} | {self.device} | {"fp16" if self.fp16 else "fp32"} | {self.workspace}')
        self.log(f'[INFO] #parameters: {sum([p.numel() for p in model.parameters() if p.requires_grad])}')

        if self.workspace is not None:
            if self.use_checkpoint == "scratch":
                self.log("[INFO] Training from scratch ...")
            elif self.use_checkpoint == "latest":
                self.log("[INFO] Loading latest checkpoint ...")
                self.load_checkpoint()
            elif self.use_checkpoint == "latest_model":
                self.log("[INFO] Loading latest checkpoint (model only)...")
                self.load_checkpoint(model_only=True)
            elif self.use_checkpoint == "best":
                if os.path.exists(self.best_path):
                    self.log("[INFO] Loading best checkpoint ...")
                    self.load_checkpoint(self.best_path)
                else:
                    self.log(f"[INFO] {self.best_path} not found, loading latest ...")
                    self.load_checkpoint()
            else:  # path to ckpt
                self.log(f"[INFO] Loading {self.use_checkpoint} ...")
                self.load_checkpoint(self.use_checkpoint)

    def __del__(self):
        if getattr(self, "log_ptr", None):
            self.log_ptr.close()

    def log(self, *args, **kwargs):
        """(`style=...` of the reference's rich console is accepted and ignored)"""
        if self.local_rank == 0:
            if not self.mute:
                print(*args)
            if self.log_ptr:
                print(*args, file=self.log_ptr)
                self.log_ptr.flush()  # write immediately to file

    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16)

    def _cuda_ray(self):
        return getattr(self.model, "cuda_ray", False)

    ### ------------------------------

    def train_step(self, data):
        rays_o = data['rays_o']  # [B, N, 3]
        rays_d = data['rays_d']  # [B, N, 3]

        if 'images' not in data:
            raise NotImplementedError("Trainer.train_step: a batch without ground-truth images is the CLIP branch, which is not ported")

        images = data['images']  # [B, N, 3/4], or the pixel ids that stand for it (PixelBatch)
        B, N, C = images.shape

        fused = isinstance(images, PixelBatch)
        if fused and not targets.is_plain_mse(self.criterion):
            images, fused = images.materialize(), False

        if C == 3 or self.model.bg_radius > 0:
            bg_color = 1
        else:  # train with a random background colour per pixel if there is no background model and an alpha channel
            bg_color = torch.rand(B, N, 3, dtype=images.store.dtype if fused else images.dtype, device=self.device)

        if fused:
            gt_rgb = targets.training_targets(images, None if C == 3 or not torch.is_tensor(bg_color) else bg_color, self.opt.color_space)
        else:
            gt_rgb = targets.reference_targets(images, bg_color, self.opt.color_space)

        # depth supervision (opt-in): the targets of the same pixels as ray distances, by the fused launch or the torch form; the
        # weights and the margin reach the renderer through vars(opt)
        lam_depth, lam_free = getattr(self.opt, "lambda_depth", 0), getattr(self.opt, "lambda_free", 0)
        extra = {}
        if (lam_depth > 0 or lam_free > 0) and 'depth' in data:
            depth = data['depth']
            if isinstance(depth, DepthBatch):
                depth = targets.training_depth_targets(depth) if targets.fused_targets else depth.materialize()
            extra['depth_target'] = depth

        outputs = self.model.render(rays_o, rays_d, staged=False, bg_color=bg_color, perturb=True, force_all_rays=False, **extra, **vars(self.opt))

        pred_rgb = outputs['image']

        if fused and (self.error_map is None or self.error_map.is_cuda):
            row = None if self.error_map is None else self.error_map[data['index'][0]]
            loss = targets.photometric_loss(pred_rgb, gt_rgb, row, data['inds_coarse'] if row is not None else None)
        else:
            loss = targets.reference_loss(self.criterion, pred_rgb, gt_rgb, self.error_map, data.get('index'), data.get('inds_coarse'))

        # the distortion regulariser (opt-in): the renderer computed it because `lambda_distort` reached it through vars(opt)
        self.last_loss_distort = None
        lam = getattr(self.opt, "lambda_distort", 0)
        if lam > 0:
            self.last_loss_distort = outputs["loss_distort"]
            loss = loss + lam * self.last_loss_distort

        # the depth terms, already weighted by lambda_depth and lambda_free (loss.depth_loss)
        self.last_loss_depth = self.last_loss_depth_parts = None
        if 'depth_target' in extra:
            self.last_loss_depth, self.last_loss_depth_parts = outputs["loss_depth"], outputs["loss_depth_parts"]
            loss = loss + self.last_loss_depth

        return pred_rgb, gt_rgb, loss

    def eval_step(self, data):
        rays_o = data['rays_o']  # [B, N, 3]
        rays_d = data['rays_d']  # [B, N, 3]
        images = data['images']  # [B, H, W, 3/4]
        B, H, W, C = images.shape

        fused = isinstance(images, PixelBatch)
        if fused and not targets.is_plain_mse(self.criterion):
            images, fused = images.materialize(), False

        bg_color = 1  # eval with fixed background color
        if fused:
            gt_rgb = targets.training_targets(images, None, self.opt.color_space)
        else:
            gt_rgb = targets.reference_targets(images, bg_color, self.opt.color_space)

        outputs = self.model.render(rays_o, rays_d, staged=True, bg_color=bg_color, perturb=False, **vars(self.opt))

        pred_rgb = outputs['image'].reshape(B, H, W, 3)
        pred_depth = outputs['depth'].reshape(B, H, W)

        if fused:
            loss = targets.photometric_loss(pred_rgb, gt_rgb)
        else:
            loss = self.criterion(pred_rgb, gt_rgb).mean()

        return pred_rgb, pred_depth, gt_rgb, loss

    # moved out bg_color and perturb for more flexible control...
    def test_step(self, data, bg_color=None, perturb=False):
        rays_o = data['rays_o']  # [B, N, 3]
        rays_d = data['rays_d']  # [B, N, 3]
        H, W = data['H'], data['W']

        if bg_color is not None:
            bg_color = bg_color.to(self.device)

        outputs = self.model.render(rays_o, rays_d, staged=True, bg_color=bg_color, perturb=perturb, **vars(self.opt))

        pred_rgb = outputs['image'].reshape(-1, H, W, 3)
        pred_depth = outputs['depth'].reshape(-1, H, W)

        return pred_rgb, pred_depth

    def save_mesh(self, save_path=None, resolution=256, threshold=10, simplify_cell=0):
        from .. import mesh
        if save_path is None:
            save_path = os.path.join(self.workspace, 'meshes', f'{self.name}_{self.epoch}.ply')
        self.log(f"==> Saving mesh to {save_path}")
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        mesh.save_mesh(self.model, save_path, resolution=resolution, threshold=threshold, fp16=self.fp16, simplify_cell=simplify_cell)
        self.log("==> Finished saving mesh.")

    ### ------------------------------

    def _open_writer(self):
        self.writer = None
        if self.use_tensorboardX and self.local_rank == 0:
            try:
                import tensorboardX
            except ImportError:
                self.log("[INFO] tensorboardX is not installed: no tensorboard log")
                self.use_tensorboardX = False
                return
            self.writer = tensorboardX.SummaryWriter(os.path.join(self.workspace, "run", self.name))

    def train(self, train_loader, valid_loader, max_epochs):
        self._open_writer()

        # mark untrained region (i.e., not covered by any camera from the training dataset)
        if self._cuda_ray():
            self.model.mark_untrained_grid(train_loader._data.poses, train_loader._data.intrinsics)

        # get a ref to error_map
        self.error_map = train_loader._data.error_map

        for epoch in range(self.epoch + 1, max_epochs + 1):
            self.epoch = epoch

            self.train_one_epoch(train_loader)

            if self.workspace is not None and self.local_rank == 0:
                self.save_checkpoint(full=True, best=False)

            if self.epoch % self.eval_interval == 0:
                self.evaluate_one_epoch(valid_loader)
                self.save_checkpoint(full=False, best=True)

        if self.use_tensorboardX and self.local_rank == 0 and self.writer is not None:
            self.writer.close()

    def evaluate(self, loader, name=None):
        self.use_tensorboardX, use_tensorboardX = False, self.use_tensorboardX
        self.evaluate_one_epoch(loader, name)
        self.use_tensorboardX = use_tensorboardX

    def test(self, loader, save_path=None, name=None, write_video=True):
        if save_path is None:
            save_path = os.path.join(self.workspace, 'results')
        if name is None:
            name = f'{self.name}_ep{self.epoch:04d}'
        os.makedirs(save_path, exist_ok=True)

        self.log(f"==> Start Test, save results to {save_path}")
        if write_video:
            self.log("[INFO] mp4 output is not ported: the frames are written as PNG files")

        self.model.eval()
        with torch.no_grad():
            for i, data in enumerate(loader):
                with self._autocast():
                    preds, preds_depth = self.test_step(data)

                if self.opt.color_space == 'linear':
                    preds = linear_to_srgb(preds)

                pred = preds[0].detach().float().cpu().numpy()
                pred = (pred * 255).astype(np.uint8)

                pred_depth = preds_depth[0].detach().float().cpu().numpy()
                pred_depth = (pred_depth * 255).astype(np.uint8)

                _write_png(os.path.join(save_path, f'{name}_{i:04d}_rgb.png'), pred)
                _write_png(os.path.join(save_path, f'{name}_{i:04d}_depth.png'), pred_depth)

        self.log("==> Finished Test.")

    def train_gui(self, *args, **kwargs):
        raise NotImplementedError("Trainer.train_gui: the GUI is not ported")

    def test_gui(self, *args, **kwargs):
        raise NotImplementedError("Trainer.test_gui: the GUI is not ported")

    def train_one_epoch(self, loader):
        self.log(f"==> Start Training Epoch {self.epoch}, lr={self.optimizer.param_groups[0]['lr']:.6f} ...")

        if self.local_rank == 0 and self.report_metric_at_train:
            for metric in self.metrics:
                metric.clear()

        self.model.train()

        writer = getattr(self, "writer", None) if self.use_tensorboardX else None
        every_step = writer is not None or self.report_metric_at_train      # someone wants each loss as it comes
        step_losses = []

        self.local_step = 0

        for data in loader:

            # update grid every 16 steps
            if self._cuda_ray() and self.global_step % self.opt.update_extra_interval == 0:
                with self._autocast():
                    self.model.update_extra_state()

            self.local_step += 1
            self.global_step += 1

            self.optimizer.zero_grad()

            with self._autocast():
                preds, truths, loss = self.train_step(data)

            self.scaler.scale(loss).backward()
            self.scaler.step(self.optimizer)
            self.scaler.update()

            if self.scheduler_update_every_step:
                self.lr_scheduler.step()

            if not every_step:
                step_losses.append(loss.detach())
                continue

            loss_val = loss.item()
            step_losses.append(loss_val)
            if self.report_metric_at_train:
                for metric in self.metrics:
                    metric.update(preds, truths)
            if writer is not None:
                writer.add_scalar("train/loss", loss_val, self.global_step)
                if getattr(self, "last_loss_distort", None) is not None:
                    writer.add_scalar("train/loss_distort", self.last_loss_distort.item(), self.global_step)
                if getattr(self, "last_loss_depth", None) is not None:
                    writer.add_scalar("train/loss_depth", self.last_loss_depth.item(), self.global_step)
                writer.add_scalar("train/lr", self.optimizer.param_groups[0]['lr'], self.global_step)

        if self.ema is not None:
            self.ema.update()

        if step_losses and torch.is_tensor(step_losses[0]):
            step_losses = torch.stack(step_losses).float().cpu().tolist()       # the epoch's one read-back
        self.last_epoch_losses = step_losses
        total_loss = 0
        for loss_val in step_losses:
            total_loss += loss_val
        average_loss = total_loss / self.local_step
        self.stats["loss"].append(average_loss)

        if self.local_rank == 0 and self.report_metric_at_train:
            for metric in self.metrics:
                self.log(metric.report(), style="red")
                if writer is not None:
                    metric.write(writer, self.epoch, prefix="train")
                metric.clear()

        if not self.scheduler_update_every_step:
            if isinstance(self.lr_scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                self.lr_scheduler.step(average_loss)
            else:
                self.lr_scheduler.step()

        self.log(f"==> Finished Epoch {self.epoch}, loss={average_loss:.6f}.")

    def evaluate_one_epoch(self, loader, name=None):
        self.log(f"++> Evaluate at epoch {self.epoch} ...")

        if name is None:
            name = f'{self.name}_ep{self.epoch:04d}'

        total_loss = 0
        if self.local_rank == 0:
            for metric in self.metrics:
                metric.clear()

        self.model.eval()

        if self.ema is not None:
            self.ema.store()
            self.ema.copy_to()

        writer = getattr(self, "writer", None) if self.use_tensorboardX else None

        with torch.no_grad():
            self.local_step = 0

            for data in loader:
                self.local_step += 1

                with self._autocast():
                    preds, preds_depth, truths, loss = self.eval_step(data)

                loss_val = loss.item()
                total_loss += loss_val

                if self.local_rank == 0:
                    for metric in self.metrics:
                        metric.update(preds, truths)

                    # save image
                    save_path = os.path.join(self.workspace, 'validation', f'{name}_{self.local_step:04d}_rgb.png')
                    save_path_depth = os.path.join(self.workspace, 'validation', f'{name}_{self.local_step:04d}_depth.png')
                    os.makedirs(os.path.dirname(save_path), exist_ok=True)

                    if self.opt.color_space == 'linear':
                        preds = linear_to_srgb(preds)

                    pred = preds[0].detach().float().cpu().numpy()
                    pred = (pred * 255).astype(np.uint8)

                    pred_depth = preds_depth[0].detach().float().cpu().numpy()
                    pred_depth = (pred_depth * 255).astype(np.uint8)

                    _write_png(save_path, pred)
                    _write_png(save_path_depth, pred_depth)

        average_loss = total_loss / self.local_step
        self.stats["valid_loss"].append(average_loss)

        if self.local_rank == 0:
            if not self.use_loss_as_metric and len(self.metrics) > 0:
                result = self.metrics[0].measure()
                self.stats["results"].append(result if self.best_mode == 'min' else - result)  # if max mode, use -result
            else:
                self.stats["results"].append(average_loss)  # if no metric, choose best by min loss

            for metric in self.metrics:
                self.log(metric.report(), style="blue")
                if writer is not None:
                    metric.write(writer, self.epoch, prefix="evaluate")
                metric.clear()

        if self.ema is not None:
            self.ema.restore()

        self.log(f"++> Evaluate epoch {self.epoch} Finished, loss={average_loss:.6f}.")

    def save_checkpoint(self, name=None, full=False, best=False, remove_old=True):
        if name is None:
            name = f'{self.name}_ep{self.epoch:04d}'

        extra = {}
        if full:
            extra['optimizer'] = self.optimizer.state_dict()
            extra['lr_scheduler'] = self.lr_scheduler.state_dict()
            extra['scaler'] = self.scaler.state_dict()
            if self.ema is not None:
                extra['ema'] = self.ema.state_dict()

        if not best:
            file_path = f"{self.ckpt_path}/{name}.pth"

            if remove_old:
                self.stats["checkpoints"].append(file_path)

                if len(self.stats["checkpoints"]) > self.max_keep_ckpt:
                    old_ckpt = self.stats["checkpoints"].pop(0)
                    if os.path.exists(old_ckpt):
                        os.remove(old_ckpt)

            _checkpoint.save_checkpoint(self.model, file_path, self.epoch, self.global_step, self.stats, best=False, extra=extra)

        else:
            if len(self.stats["results"]) > 0:
                if self.stats["best_result"] is None or self.stats["results"][-1] < self.stats["best_result"]:
                    self.log(f"[INFO] New best result: {self.stats['best_result']} --> {self.stats['results'][-1]}")
                    self.stats["best_result"] = self.stats["results"][-1]

                    # save ema results (and drop density_grid: nobody continues training from the best checkpoint)
                    if self.ema is not None:
                        self.ema.store()
                        self.ema.copy_to()

                    _checkpoint.save_checkpoint(self.model, self.best_path, self.epoch, self.global_step, self.stats, best=True, extra=extra)

                    if self.ema is not None:
                        self.ema.restore()
            else:
                self.log("[WARN] no evaluated results found, skip saving best checkpoint.")

    def load_checkpoint(self, checkpoint=None, model_only=False):
        if checkpoint is None:
            checkpoint = _checkpoint.latest_checkpoint(self.ckpt_path, self.name)
            if checkpoint:
                self.log(f"[INFO] Latest checkpoint is {checkpoint}")
            else:
                self.log("[WARN] No checkpoint found, model randomly initialized.")
                return

        checkpoint_dict = _checkpoint._read(checkpoint, self.device)       # (weights only: nothing in the file is executed)

        if 'model' not in checkpoint_dict:
            self.model.load_state_dict(checkpoint_dict)
            self.log("[INFO] loaded model.")
            return

        missing_keys, unexpected_keys = self.model.load_state_dict(checkpoint_dict['model'], strict=False)
        self.log("[INFO] loaded model.")
        if len(missing_keys) > 0:
            self.log(f"[WARN] missing keys: {missing_keys}")
        if len(unexpected_keys) > 0:
            self.log(f"[WARN] unexpected keys: {unexpected_keys}")

        if self.ema is not None and 'ema' in checkpoint_dict:
            self.ema.load_state_dict(checkpoint_dict['ema'])

        if self._cuda_ray():
            if 'mean_count' in checkpoint_dict:
                self.model.mean_count = checkpoint_dict['mean_count']
            if 'mean_density' in checkpoint_dict:
                self.model.mean_density = checkpoint_dict['mean_density']

        if model_only:
            return

        self.stats = checkpoint_dict['stats']
        self.epoch = checkpoint_dict['epoch']
        self.global_step = checkpoint_dict['global_step']
        self.log(f"[INFO] load at epoch {self.epoch}, global step {self.global_step}")

        if self.optimizer and 'optimizer' in checkpoint_dict:
            try:
                self.optimizer.load_state_dict(checkpoint_dict['optimizer'])
                self.log("[INFO] loaded optimizer.")
            except Exception:
                self.log("[WARN] Failed to load optimizer.")

        if self.lr_scheduler and 'lr_scheduler' in checkpoint_dict:
            try:
                self.lr_scheduler.load_state_dict(checkpoint_dict['lr_scheduler'])
                self.log("[INFO] loaded scheduler.")
            except Exception:
                self.log("[WARN] Failed to load scheduler.")

        if self.scaler and 'scaler' in checkpoint_dict:
            try:
                self.scaler.load_state_dict(checkpoint_dict['scaler'])
                self.log("[INFO] loaded scaler.")
            except Exception:
                self.log("[WARN] Failed to load scaler.")
