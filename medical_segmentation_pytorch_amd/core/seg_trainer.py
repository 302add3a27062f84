"""Segmentation trainer -- reference ``core/seg_trainer.py:15-181``.

Hot loop (``train_one_epoch``) keeps the reference's step semantics: zero_grad -> forward (autocast
for the eager engine; the fused engine is bf16 by construction) -> loss (+ KD term) -> backward ->
scaler.step(optimizer) -> scaler.update -> scheduler.step (per iteration) -> EMA update.

MI355X changes:
  * no per-iteration host sync: losses stay on the device and are flushed to TensorBoard / the
    progress bar every ``config.log_interval`` iterations (the reference syncs twice per step);
  * fused engine + static shapes: after ``graph_warmup`` eager iterations the whole step
    (weight repack, forward, loss, backward, all-reduce, optimizer) is captured into ONE hipGraph
    and replayed; the scheduler writes lr/momentum through the optimizer's device hyper tensor;
  * validation metrics accumulate a device confusion matrix (HIP kernel) and all-reduce it once.
"""
from __future__ import annotations

import contextlib
import os
import time

import numpy as np
import torch
from PIL import Image

from ..models import get_teacher_model
from ..ops.bn import flush_pending
from ..ops.calibration import uncertainty_map
from ..ops.components import postprocess
from ..runtime.trainer_engine import StepEngine, iteration
from ..utils import FusedModel, de_parallel, get_colormap, get_seg_metrics, sampler_set_epoch
from ..utils.metrics import _CalibrationMetric
from .base_trainer import BaseTrainer
from ..ops.resample import colorize, resize_bilinear
from ..ops.tiled import sliding_window_inference
from ..utils.tracing import trace_range
from ..utils.watchdog import check_finite
from .loss import kd_loss_fn


def _tqdm(it, enable):
    if not enable:
        return it
    try:
        from tqdm import tqdm
        return tqdm(it)
    except Exception:   # pragma: no cover
        return it


def _finite_or_none(v):
    """nan / inf -> None, so val_history.json stays strict JSON (a boundary metric with nothing scored is nan)."""
    if isinstance(v, list):
        return [_finite_or_none(x) for x in v]
    return v if v == v and abs(v) != float('inf') else None


def add_checkpoint_temperature(path, T):
    """Add (or replace) the float ``temperature`` key of the checkpoint at ``path`` in place; every other key is
    written back as it was read."""
    T = float(T)
    if not 0 < T < float('inf'):
        raise ValueError(f'temperature must be a finite number > 0, got {T!r}')
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    ckpt['temperature'] = T
    tmp = f'{path}.tmp'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


class SegTrainer(BaseTrainer):
    def __init__(self, config):
        super().__init__(config)
        if config.is_testing:
            self.colormap = torch.tensor(get_colormap(config)).to(self.device)
        else:
            self.teacher_model = get_teacher_model(config, self.device)
            if self.teacher_model is not None and self.fused:
                from ..runtime.fused_model import supports
                if supports(self.teacher_model):   # KD teacher fwd on the HIP kernels (eval-mode BN)
                    for p in self.teacher_model.parameters():
                        p.requires_grad_(False)
                    self.teacher_model = FusedModel(self.teacher_model).eval()
            self.metrics = [get_seg_metrics(config, m).to(self.device) for m in config.metrics]
        self.engine = None
        self._ema_exec = (None, None)
        self._loss_hist = []
        self.val_history = []

    # ------------------------------------------------------------------------------------------------
    def _accum(self):
        return max(1, int(getattr(self.config_ref, 'accum_steps', 1) or 1))

    def eager_step(self, images, masks):
        """One eager micro-step.  Gradient accumulation (``config.accum_steps`` K): zero_grad on a group's
        first micro-batch, ``loss / K`` back-propagated on each (torch DDP: ``no_sync`` on all but the last),
        ``scaler.step`` / ``update`` on its last; ``self._stepped`` tells the caller."""
        config = self.config_ref
        accum = self._accum()
        micro = getattr(self, '_micro', 0)
        first, last = micro == 0, micro == accum - 1
        self._micro = 0 if last else micro + 1
        self._stepped = last
        if getattr(self, 'channels_last', False) and images.dim() == 4:
            images = images.contiguous(memory_format=torch.channels_last)
        if first:
            self.optimizer.zero_grad()
            ex = getattr(self.model, 'executor', None)
            if ex is not None:   # prepacked conv weights must follow the last optimizer step
                ex.repack()
        amp = config.amp_training and not self.fused and self.device.type == 'cuda'
        dtype = torch.float16 if config.amp_dtype == 'fp16' else torch.bfloat16
        with torch.autocast('cuda', dtype=dtype, enabled=amp):
            preds = self.model(images)
            loss = self.loss_fn(preds, masks)
        if config.kd_training:
            with torch.autocast('cuda', dtype=dtype, enabled=self.device.type == 'cuda'):
                with torch.no_grad():
                    teacher_preds = self.teacher_model(images)
            loss_kd = kd_loss_fn(config, preds.float(), teacher_preds.detach().float())
            loss = loss + config.kd_loss_coefficient * loss_kd
            self._last_kd = loss_kd.detach()
        obj = loss if accum == 1 else loss * (1.0 / accum)
        no_sync = self.model.no_sync() if (not last and hasattr(self.model, 'no_sync')) else contextlib.nullcontext()
        with no_sync:   # torch DDP: the gradient all-reduce only on the group's last micro-batch
            self.scaler.scale(obj).backward()
        flush_pending()
        if last:
            self.scaler.step(self.optimizer)
            self.scaler.update()
        return loss.detach()

    def _use_graph(self, config):
        # every loss (CE, device-side OHEM, BCE+Dice), the KD term and the fused fp16 GradScaler are
        # capture-safe; the eager teacher fallback is not.  A step that issues torch.distributed
        # collectives (gradient buckets, SyncBN over RCCL) is captured too when config.graph_collectives:
        # torch 2.10's process group records captured RCCL calls as graph nodes and keeps their works off
        # its watchdog (round 6: tools/dev/graph_rccl_probe.py, tests/test_gpu_distributed.py).  The
        # bucket rebuild (first step) and every communicator init happen in the eager warm-up steps.
        kd_ok = not config.kd_training or isinstance(self.teacher_model, FusedModel)
        collectives = getattr(self.optimizer, 'bucketer', None) is not None or \
            (config.DDP and config.gpu_num > 1)
        # (RCCL only: gloo collectives run on the host and cannot be captured -- the same-GPU gloo rehearsal)
        nccl = torch.distributed.is_available() and torch.distributed.is_initialized() and \
            torch.distributed.get_backend() == 'nccl'
        coll_ok = not collectives or (getattr(config, 'graph_collectives', True) and nccl)
        return self.fused and config.use_graph and kd_ok and not config.use_aux and coll_ok

    def step_engine(self, config):
        """The fused engine's device step (:class:`runtime.trainer_engine.StepEngine`) -- the same object
        ``bench.py`` times; built on first use, after ``parallel_model`` wrapped the model."""
        if self.engine is None and self.fused and isinstance(self.model, FusedModel):
            kd_fn = (lambda s, t: kd_loss_fn(config, s, t)) if config.kd_training else None
            self.engine = StepEngine(self.model, self.optimizer, self.loss_fn, self.scaler,
                                     teacher=self.teacher_model if config.kd_training else None, kd_fn=kd_fn,
                                     kd_coef=config.kd_loss_coefficient, use_graph=self._use_graph(config),
                                     warmup=config.graph_warmup, accum_steps=getattr(config, 'accum_steps', 1))
            if self.main_rank and self.logger:
                self.logger.info(f'step engine: hipGraph capture {"on" if self.engine.use_graph else "off"} '
                                 f'(world {config.gpu_num if config.DDP else 1}, gradient bucketer '
                                 f'{"on" if getattr(self.optimizer, "bucketer", None) is not None else "off"})')
        return self.engine

    def train_step(self, images, masks):
        """One training iteration (reference core/seg_trainer.py:24-95 body): the device step (fused
        engine: :class:`StepEngine`, hipGraph-replayed; eager engine: autocast + GradScaler), then the
        per-iteration scheduler step and EMA update.  ``train_one_epoch`` and ``bench.py`` call this."""
        config = self.config_ref
        self.train_itrs += 1
        self._last_kd = None
        engine = self.step_engine(config)
        if engine is not None:
            loss = iteration(engine, self.scheduler, self.ema_model, self.train_itrs, images, masks)
            self._last_kd = engine.last_kd.clone() if engine.last_kd is not None else None
            return loss
        loss = self.eager_step(images, masks)
        if self._stepped:   # (gradient accumulation: only after an optimizer step)
            self.scheduler.step()
            self.ema_model.update(self.model, self.train_itrs // self._accum())
        return loss

    def _flush_logs(self, config, pbar=None):
        if not self._loss_hist:
            return
        vals = torch.stack([v for _, v, _ in self._loss_hist]).float().cpu().tolist()
        if config.DDP:
            from ..runtime import comm as ipc_comm
            ipc_comm.check()   # a timed-out peer-memory exchange poisons the step with NaN: name the cause
        check_finite(vals, self._loss_hist[-1][0])
        kds = [k for _, _, k in self._loss_hist]
        kdv = torch.stack(kds).float().cpu().tolist() if all(k is not None for k in kds) else None
        if config.use_tb and self.main_rank and self.writer is not None:
            for (itr, _, _), v in zip(self._loss_hist, vals):
                self.writer.add_scalar('train/loss', v, itr)
            if kdv is not None:
                for (itr, _, _), v, tot in zip(self._loss_hist, kdv, vals):
                    self.writer.add_scalar('train/loss_kd', v, itr)
                    self.writer.add_scalar('train/loss_total', tot, itr)
        if pbar is not None and hasattr(pbar, 'set_description'):
            pbar.set_description(f'Epoch:{self.cur_epoch}/{config.total_epoch}    |Loss:{vals[-1]:4.4g}    |')
        self.last_loss = vals[-1]
        self._loss_hist = []

    def train_one_epoch(self, config):
        self.config_ref = config
        self.model.train()
        sampler_set_epoch(config, self.train_loader, self.cur_epoch)
        if hasattr(self.loss_fn, 'set_epoch'):
            self.loss_fn.set_epoch(self.cur_epoch)     # epoch-scheduled loss weights (BoundaryLoss)
        pbar = _tqdm(self.train_loader, self.main_rank and config.progress_bar)
        wd = getattr(self, 'watchdog', None)
        for cur_itrs, (images, masks) in enumerate(pbar):
            self.cur_itrs = cur_itrs
            with trace_range('train/h2d'):
                images = images.to(self.device, dtype=torch.float32, non_blocking=True)
                masks = masks.to(self.device, dtype=torch.float32 if config.num_class == 1 else torch.long,
                                 non_blocking=True)
            with trace_range('train/step'):
                loss = self.train_step(images, masks)
            if wd is not None:
                wd.beat()
            self._loss_hist.append((self.train_itrs, loss.clone(), self._last_kd))
            if len(self._loss_hist) >= config.log_interval:
                self._flush_logs(config, pbar)
        self._flush_logs(config, pbar)

    # ------------------------------------------------------------------------------------------------
    def _ema_forward(self, images):
        ema = self.ema_model.ema
        if not self.fused or getattr(self.config_ref, 'val_fp32', False):
            # reference protocol: the EMA model in fp32 without autocast (core/seg_trainer.py:114)
            return ema(images).float()
        owner, ex = self._ema_exec
        if owner is not ema:
            ex = FusedModel(ema).eval()
            self._ema_exec = (ema, ex)
        return ex(images)

    def _log_inference(self, tiled):
        if tiled is not None and self.logger and self.main_rank and not getattr(self, '_inference_logged', False):
            self._inference_logged = True
            self.logger.info(f'Sliding-window inference / flip TTA: {tiled} (window None: the whole image)\n')

    def _eval_batches(self, config, loader, tiled):
        """The evaluation forward of ``validate`` and ``calibrate`` over ``loader``: yields (logits at the masks'
        resolution -- two-class for a sigmoid head --, masks)."""
        pbar = _tqdm(loader, self.main_rank and config.progress_bar)
        for images, masks in pbar:
            images = images.to(self.device, dtype=torch.float32)
            _, _, H, W = images.shape
            stride = config.val_img_stride
            # windows run at native resolution; flip TTA alone keeps the stride-aligned whole image as its one window
            resized = (H % stride != 0 or W % stride != 0) and (tiled is None or tiled['window'] is None)
            if resized:
                images = resize_bilinear(images, (H // stride * stride, W // stride * stride))
            masks = masks.to(self.device, dtype=torch.long)
            with trace_range('val/forward'):
                if tiled is None:
                    preds = self._ema_forward(images)
                else:
                    preds = sliding_window_inference(images, self._ema_forward,
                                                     **{**tiled, 'window': tiled['window'] or images.shape[2:]})
            if resized:
                preds = resize_bilinear(preds, masks.size()[1:], align_corners=True)
            if preds.shape[1] == 1:   # binary (sigmoid) path -> two-class logits for the confmat
                preds = torch.cat([torch.zeros_like(preds), preds], 1)
            yield preds, masks

    @torch.no_grad()
    def validate(self, config, loader, val_best=False):
        self.config_ref = config
        t_val = time.perf_counter()
        tiled = config.inference_settings()
        self._log_inference(tiled)
        calib = [m for m in self.metrics if isinstance(m, _CalibrationMetric)]
        if calib:
            calib[0].acc.set_temperature(self.temperature)
        for preds, masks in self._eval_batches(config, loader, tiled):
            for metric in self.metrics:
                metric.update(preds.detach().float(), masks)
        scores = [metric.compute() for metric in self.metrics]
        score = scores[0].mean()
        if self.main_rank and self.logger:
            for i in range(len(config.metrics)):
                if val_best:
                    self.logger.info(f'\n\nTrain {config.total_epoch} epochs finished.' +
                                     f'\n\nBest m{config.metrics[i]} is: {scores[i].mean():.4f}\n')
                else:
                    infos = f' Epoch{self.cur_epoch} m{config.metrics[i]}: {scores[i].mean():.4f} \t| ' + \
                            f'best m{config.metrics[0]} so far: {self.best_score:.4f}\n'
                    if len(config.metrics) > 1 and i != len(config.metrics) - 1:
                        infos = infos[:-1]
                    self.logger.info(infos)
                one_sided = getattr(self.metrics[i], 'last_one_sided', None)
                if one_sided is not None and int(one_sided.sum()) > 0:
                    self.logger.info(f' m{config.metrics[i]}: {int(one_sided.sum())} (image, class) pairs with exactly '
                                     f'one empty mask scored at the image diagonal (per class {one_sided.tolist()})')
                if config.use_tb and self.writer is not None and self.cur_epoch < config.total_epoch:
                    self.writer.add_scalar(f'val/m{config.metrics[i]}', scores[i].mean().item(), self.cur_epoch + 1)
                    if config.metrics[i] == 'iou':
                        for j in range(scores[i].numel()):
                            self.writer.add_scalar(f'val/IoU_cls{j:02d}', scores[i][j].item(), self.cur_epoch + 1)
        self.last_scores = {m: s.detach().cpu() for m, s in zip(config.metrics, scores)}
        # per-validation record (save_dir/val_history.json, written by BaseTrainer.run): accuracy vs time
        rec = {'epoch': int(self.cur_epoch), 'train_itrs': int(getattr(self, 'train_itrs', 0)),
               'elapsed_s': round(time.perf_counter() - getattr(self, '_t_run', time.perf_counter()), 2),
               'val_s': round(time.perf_counter() - t_val, 3),   # this validation: loader, forward, metrics
               'score': _finite_or_none(float(score)), 'val_best': bool(val_best),
               'fp32': bool(getattr(config, 'val_fp32', False))}
        if tiled is not None:
            rec['inference'] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in tiled.items()}
        for m, v in self.last_scores.items():
            rec[m] = _finite_or_none(v.tolist())
        if calib:     # the reliability diagram behind the calibration metrics (all ranks)
            rel = calib[0].reliability()
            rec['calibration'] = {'temperature': float(self.temperature), 'bins': int(calib[0].acc.bins),
                                  'count': rel['count'].tolist(),
                                  'accuracy': _finite_or_none(rel['accuracy'].tolist()),
                                  'confidence': _finite_or_none(rel['confidence'].tolist())}
        self.val_history.append(rec)
        for metric in self.metrics:
            metric.reset()
        return score

    @torch.no_grad()
    def calibrate(self, config, loader, ckpt_path=None):
        """Post-hoc temperature scaling of the model ``validate`` evaluates (after ``val_best``: the best checkpoint):
        fit T on ``loader`` through the evaluation forward (resize, sliding windows, TTA), keep it in
        ``self.temperature``, add it to ``best.pth`` (or ``ckpt_path``) and validate once more at the new temperature.
        The argmax does not depend on T, so the label-map metrics are those of the validation before."""
        from ..ops.calibration import fit_temperature
        self.config_ref = config
        tiled = config.inference_settings()
        T, info = fit_temperature(
            lambda: ((p.detach().float(), m) for p, m in self._eval_batches(config, loader, tiled)),
            config.ignore_index, config.calibration_rounds, group=getattr(config, 'dist_group', None),
            device=self.device, return_info=True)
        self.temperature = T
        if self.main_rank:
            if self.logger:
                self.logger.info(f'\nTemperature scaling: T = {T:.5f} after {info["rounds"]} rounds\n')
            add_checkpoint_temperature(f'{config.save_dir}/best.pth' if ckpt_path is None else ckpt_path, T)
        if config.DDP:      # rank 0 alone rewrote the checkpoint that the next val_best reads
            from ..utils.parallel import get_group
            torch.distributed.barrier(group=get_group(config))
        self.validate(config, loader, val_best=True)
        self.val_history[-1]['calibrated'] = True
        return T

    @torch.no_grad()
    def predict(self, config):
        if config.DDP:
            raise ValueError('Predict mode currently does not support DDP.')
        if self.logger:
            self.logger.info('\nStart predicting...\n')
        model = de_parallel(self.model).eval()
        fwd = FusedModel(model).eval() if self.fused else model
        post = dict(fill_holes=bool(getattr(config, 'post_fill_holes', False)),
                    min_area=int(getattr(config, 'post_min_area', 0)),
                    keep_largest=bool(getattr(config, 'post_keep_largest', False)))
        clean = post['fill_holes'] or post['min_area'] > 0 or post['keep_largest']
        if clean and self.logger:
            self.logger.info(f'Post-processing the predicted masks: {post}, '
                             f'connectivity {getattr(config, "cc_connectivity", 8)}\n')
        tiled = config.inference_settings()
        self._log_inference(tiled)
        unc_mode = getattr(config, 'save_uncertainty', None)
        if unc_mode and self.logger:
            self.logger.info(f'Saving {unc_mode} uncertainty maps at temperature {self.temperature:.5f}\n')
        for images, images_aug, img_names in _tqdm(self.test_loader, config.progress_bar):
            images_aug = images_aug.to(self.device, dtype=torch.float32)
            if tiled is None:
                preds = fwd(images_aug)
            else:
                preds = sliding_window_inference(images_aug, lambda x: fwd(x).float(),
                                                 **{**tiled, 'window': tiled['window'] or images_aug.shape[2:]})
            # (from the final logits, blended or not, before any clean-up of the label map)
            unc = uncertainty_map(preds.float(), self.temperature, unc_mode).cpu().numpy() if unc_mode else None
            if clean:
                # the label map stays on the device: argmax (logit > 0 for a sigmoid head), clean-up, colours
                labels = (preds[:, 0] > 0) if preds.shape[1] == 1 else preds.argmax(1)
                labels, errors = postprocess(labels.to(torch.uint8), max(config.num_class, 2), debug=True,
                                             connectivity=getattr(config, 'cc_connectivity', 8), **post)
                preds = self.colormap[labels.long()].cpu().numpy()
                if int(errors) != 0:      # read after the copy above has synchronised anyway
                    raise RuntimeError(f'post-processing: the labelling kernels reported {int(errors)} loops that '
                                       f'hit their iteration cap; the masks of {list(img_names)} were not saved')
            else:
                preds = colorize(preds, self.colormap).cpu().numpy()
            images = images.cpu().numpy()
            for i in range(preds.shape[0]):
                save_path = os.path.join(config.save_dir, img_names[i])
                suffix = img_names[i].split('.')[-1]
                pred = Image.fromarray(preds[i].astype(np.uint8))
                if config.save_mask:
                    pred.save(save_path)
                if unc is not None:
                    Image.fromarray(unc[i]).save(os.path.splitext(save_path)[0] + '_unc.png')
                if config.blend_prediction:
                    blend_path = save_path.replace(f'.{suffix}', f'_blend.{suffix}')
                    image = Image.fromarray(images[i].astype(np.uint8))
                    if image.size != pred.size:
                        image = image.resize(pred.size, Image.BILINEAR)
                    Image.blend(image, pred, config.blend_alpha).save(blend_path)
