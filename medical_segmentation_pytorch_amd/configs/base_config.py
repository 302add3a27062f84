"""Configuration object with the reference's field names -- ``configs/base_config.py:5-123``.

Every default of the reference ``BaseConfig`` is kept (Appendix A of SURVEY.md).  Additions are the
MI355X engine knobs at the bottom (``engine``, ``use_graph``, ``bucket_cap_mb`` ...) which old
configs simply do not set.  ``init_dependent_config`` derives the same fields as the reference
(``base_config.py:106-123``) and, unlike it, may be re-run after CLI overrides
(SURVEY Appendix E.4): derived fields are only filled when still unset.
"""
from __future__ import annotations

import os


class BaseConfig:
    def __init__(self):
        # Dataset
        self.dataset = None
        self.subset = None
        self.dataroot = None
        self.data_root = None          # field read by the polyp dataset (reference polyp.py:14)
        self.num_class = -1
        self.ignore_index = 255
        self.num_channel = None
        self.use_test_set = False

        # Model
        self.model = None
        self.encoder = None
        self.decoder = None
        self.encoder_weights = 'imagenet'
        self.base_channel = None

        # Training
        self.total_epoch = 200
        self.base_lr = 0.01
        self.train_bs = 16             # per GPU
        self.use_aux = False
        self.aux_coef = None

        # Validating
        self.metrics = ['dice']        # the first one drives best-checkpoint selection
        self.nsd_tolerance = 2.0       # pixels: the 'nsd' (surface Dice) metric counts boundary pixels this close
        self.lesion_min_overlap = 0.0  # 'lesion_*' metrics: a component is a hit when at least this fraction of its
                                       # area (and at least one pixel) lies in the other mask
        self.cc_connectivity = 8       # 4 | 8: pixel connectivity of the lesion metrics and the post-processing
        # calibration (ops/calibration.py; absent from the reference): the 'ece' | 'mce' | 'nll' | 'brier' metrics,
        # post-hoc temperature scaling and the uncertainty maps of predict mode
        self.calibration_bins = 15     # 1..64 equal-width confidence bins of the reliability statistics
        self.calibrate_temperature = False   # fit T on the validation split after training, store it in best.pth
        self.calibration_rounds = 2    # 1..4 passes over the split, each refining the grid of the one before
        self.temperature = None        # None: the checkpoint's (1.0 when it has none) | an override > 0
        self.save_uncertainty = None   # None | 'entropy' | 'confidence': predict mode writes <stem>_unc.png
        self.val_bs = 16
        self.begin_val_epoch = 0
        self.val_interval = 1
        self.val_img_stride = 1

        # Inference (validate, predict, app): sliding windows and flip test-time augmentation (ops/tiled.py; absent
        # from the reference).  Both unset: one whole-image forward, exactly as before.
        self.infer_window = None       # None | w | (h, w): run the network on windows of this size at native
                                       # resolution (a positive multiple of val_img_stride)
        self.infer_overlap = 0.5       # fraction of a window shared with its neighbour, in [0, 0.75]
        self.infer_blend = 'gaussian'  # 'gaussian' | 'constant' importance map of the overlap blend
        self.infer_sigma_scale = 0.125   # gaussian sigma as a fraction of the window extent
        self.infer_batch = 16          # windows (views included) per forward
        self.tta_flips = ''            # '' | 'h' | 'v' | 'hv': mirrored views averaged with the identity
        self.tta_average = 'logits'    # 'logits' | 'probs': what the windows and views average

        # Testing
        self.is_testing = False
        self.test_bs = 16
        self.test_data_folder = None
        self.colormap = 'random'
        self.colormap_path = None
        self.save_mask = True
        self.blend_prediction = True
        self.blend_alpha = 0.3
        # mask clean-up of the predicted label map, applied in this order (ops/components.postprocess)
        self.post_fill_holes = False   # fill background holes enclosed by foreground
        self.post_min_area = 0         # remove foreground components smaller than this many pixels
        self.post_keep_largest = False   # keep only the largest component per class

        # Loss
        self.loss_type = 'ce'
        self.class_weights = None
        self.ohem_thrs = 0.7
        self.reduction = 'mean'
        # softmax-head overlap / focal losses (core.loss.RegionLoss; absent from the reference)
        self.loss_pixel_weight = 1.0   # weight of the ce / focal term
        self.loss_region_weight = 1.0  # weight of the dice / tversky term
        self.dice_smooth = 1.0
        self.dice_ignore_background = False   # leave class 0 out of the region mean
        self.tversky_alpha = 0.3       # false-positive weight
        self.tversky_beta = 0.7        # false-negative weight
        self.focal_gamma = 2.0         # 0 (plain ce) or >= 1
        # boundary (signed-distance) term of the '*boundary' loss types (core.loss.BoundaryLoss)
        self.loss_boundary_weight = 0.01      # >= 0
        self.boundary_ramp_epochs = 0         # weight * min(1, (epoch + 1) / R) for R > 0
        self.boundary_include_background = False   # True: class 0 gets a distance map as well
        # Lovasz-softmax term of the '*lovasz_softmax' loss types (core.loss.LovaszSoftmaxLoss): weighted by
        # loss_region_weight, class 0 left out with dice_ignore_background
        self.lovasz_per_image = False  # True: sort and average per image; False: over the whole batch

        # Scheduler
        self.lr_policy = 'cos_warmup'
        self.warmup_epochs = 3
        self.step_size = None          # reference StepLR needs it but never defines it (Appendix E.3)

        # Optimizer
        self.optimizer_type = 'sgd'
        self.momentum = 0.9
        self.weight_decay = 1e-4

        # Monitoring
        self.save_ckpt = True
        self.save_dir = 'save'
        self.use_tb = True
        self.tb_log_dir = None
        self.ckpt_name = None
        self.logger_name = None

        # Training setting
        self.amp_training = False
        self.resume_training = True
        self.load_ckpt = True
        self.load_ckpt_path = None
        self.base_workers = 8
        self.random_seed = 1
        self.use_ema = False

        # Augmentation
        self.crop_size = 512
        self.crop_h = None
        self.crop_w = None
        self.scale = 1.0
        self.randscale = 0.0
        self.brightness = 0.0
        self.contrast = 0.0
        self.saturation = 0.0
        self.h_flip = 0.0
        self.v_flip = 0.0
        # rotation / shift / elastic warp and gamma / blur / noise (utils/transforms.SegAugment, csrc/augment.hip;
        # absent from the reference).  Every group is off at its default and then draws no random number.
        self.aug_rotate = 0.0          # rotation limit in degrees: theta ~ U[-r, r]
        self.aug_shift = 0.0           # translation limit as a fraction of the crop
        self.aug_affine_p = 0.5        # probability of the rotate / shift group
        self.aug_elastic_sigma = 0.0   # std (pixels) of the B-spline control-point displacements; 0 = off
        self.aug_elastic_cells = 4     # B-spline cells per axis over the crop, 1..8
        self.aug_elastic_p = 0.5
        self.aug_border = 'reflect'    # 'reflect' (reflect-101) | 'constant' (zeros) outside the scaled image,
                                       # for warped samples
        self.aug_gamma = None          # None | [lo, hi]: gamma ~ U[lo, hi], v <- 255 (v / 255)^gamma
        self.aug_gamma_p = 0.5
        self.aug_blur_sigma = None     # None | [lo, hi] pixels, hi <= 2.5: Gaussian blur
        self.aug_blur_p = 0.5
        self.aug_noise_std = None      # None | [lo, hi] in 0..255 levels: additive Gaussian noise
        self.aug_noise_p = 0.5

        # DDP
        self.synBN = True
        self.destroy_ddp_process = True
        self.local_rank = int(os.getenv('LOCAL_RANK', -1))
        self.main_rank = self.local_rank in [-1, 0]

        # Knowledge distillation
        self.kd_training = False
        self.teacher_ckpt = ''
        self.teacher_model = 'smp'
        self.teacher_encoder = None
        self.teacher_decoder = None
        self.kd_loss_type = 'kl_div'
        self.kd_loss_coefficient = 1.0
        self.kd_temperature = 4.0

        # ---- MI355X engine knobs (new; absent from the reference) ----
        self.engine = 'auto'           # 'auto' | 'fused' (HIP kernels) | 'eager' (stock torch ops)
        self.amp_dtype = 'bf16'        # CDNA4 autocast dtype when amp_training: 'bf16' | 'fp16'
        self.use_graph = True          # capture the static-shape train step in a hipGraph
        self.eager_channels_last = True   # eager engine on a GPU: channels-last activations (MIOpen NHWC
                                          # kernels; 1.8x the NCHW step on MI355X, profiles/r02/eager_sweep)
        self.bucket_cap_mb = 64        # gradient bucket size for the RCCL all-reduce
        self.grad_compress = None      # None | 'bf16' all-reduce compression
        self.lr_scale = 'reference'    # lr vs batch: 'reference' (x gpu_num) | 'sqrt' | 'linear' in
                                       # global_batch / lr_ref_batch (utils/optimizer.lr_batch_factor)
        self.lr_ref_batch = 16         # the batch base_lr is tuned for (MyConfig train_bs)
        self.accum_steps = 1           # gradient accumulation: micro-batches per optimizer step (DDP averaging
                                       # semantics: global batch = train_bs x gpu_num x accum_steps; BN
                                       # statistics per micro-batch, as torch DDP + no_sync)
        self.syncbn_comm = 'rccl'      # SyncBN statistic exchange: 'rccl' | 'auto' (IPC peer-memory kernel on one
                                       # node after a self-test, RCCL otherwise) | 'ipc'  (env MSP_SYNCBN_COMM
                                       # overrides; IPC is opt-in until a cross-GPU run of it is recorded)
        self.gpu_augment = True        # run augmentation on the GPU over an HBM-resident dataset
        self.dist_backend = None       # None -> 'nccl' (RCCL) on GPU, 'gloo' on CPU
        self.log_interval = 50         # device-side loss accumulation, host sync every N iters
        self.ckpt_extra_state = True   # also save scaler/EMA/RNG (extra keys; old readers ignore)
        self.synthetic_data = False    # generate a synthetic polyp set when data_root is missing
        self.synthetic_num = (64, 16, 16)
        self.synthetic_size = 352
        self.cap_workers = True        # cap DataLoader workers at the host CPU count (ref: gpu_num*base_workers)
        self.teacher_base_channel = None
        self.graph_warmup = 3          # eager iterations before the hipGraph capture
        self.bucketer_world1 = False   # attach the RCCL gradient bucketer at world size 1 too (bench --ddp)
        self.graph_collectives = True  # capture a step that issues torch.distributed collectives (gradient
                                       # buckets, SyncBN over RCCL) in the hipGraph too (RCCL calls are graph
                                       # nodes; tools/dev/graph_rccl_probe.py); False: such steps run eagerly
        self.val_fp32 = False          # validate the EMA model in fp32 eager PyTorch exactly as the reference
                                       # (core/seg_trainer.py:114); False: the bf16 fused executor (fast)
        self.progress_bar = True
        self.trace = False             # roctx ranges around step phases + per-phase HIP-event timing
        self.watchdog_timeout_s = 0    # >0: dump stacks + exit(75) after this long without a step
        self.dist_timeout_min = 30     # process-group timeout (a dead peer errors instead of hanging)
        self.dist_group = None         # process sub-group (concurrent HPO trials); None = WORLD
        self.device_index = None       # explicit GPU index: single-device run without DataParallel scaling
                                       # (bench.py), or every DDP rank on that one device (gloo rehearsal)

    # ------------------------------------------------------------------
    def init_dependent_config(self):
        """Derive dependent fields (reference base_config.py:106-123).  Fields this pass derived
        itself are re-derived on a later call (after CLI overrides); user-set values are kept."""
        assert len(self.metrics) > 0
        if self.metrics[0] in ('hd95', 'assd'):
            raise ValueError(f"metrics[0] drives best-checkpoint selection as higher-is-better; '{self.metrics[0]}' is "
                             f"a distance (lower is better) -- put 'dice', 'iou' or 'nsd' first")
        if self.metrics[0] in ('ece', 'mce', 'nll', 'brier'):
            raise ValueError(f"metrics[0] drives best-checkpoint selection as higher-is-better; '{self.metrics[0]}' is "
                             f"a calibration error (lower is better) -- put 'dice', 'iou' or 'nsd' first")
        self.check_calibration()
        if not 0.0 <= float(self.lesion_min_overlap) <= 1.0:
            raise ValueError(f'lesion_min_overlap must be in [0, 1], got {self.lesion_min_overlap}')
        if self.cc_connectivity not in (4, 8):
            raise ValueError(f'cc_connectivity must be 4 or 8, got {self.cc_connectivity!r}')
        if int(self.post_min_area) != self.post_min_area or self.post_min_area < 0:
            raise ValueError(f'post_min_area must be an integer >= 0, got {self.post_min_area!r}')
        if isinstance(self.loss_boundary_weight, bool) or not isinstance(self.loss_boundary_weight, (int, float)) \
                or not self.loss_boundary_weight >= 0:
            raise ValueError(f'loss_boundary_weight must be a number >= 0, got {self.loss_boundary_weight!r}')
        if isinstance(self.boundary_ramp_epochs, bool) or not isinstance(self.boundary_ramp_epochs, (int, float)) \
                or int(self.boundary_ramp_epochs) != self.boundary_ramp_epochs or self.boundary_ramp_epochs < 0:
            raise ValueError(f'boundary_ramp_epochs must be an integer >= 0, got {self.boundary_ramp_epochs!r}')
        self.check_inference()
        auto = getattr(self, '_auto_derived', set())

        def derive(name, value, cond):
            if getattr(self, name) is None or name in auto:
                if cond:
                    setattr(self, name, value)
                    auto.add(name)

        derive('load_ckpt_path', f'{self.save_dir}/last.pth', not self.is_testing)
        derive('tb_log_dir', f'{self.save_dir}/tb_logs/', True)
        derive('crop_h', self.crop_size, True)
        derive('crop_w', self.crop_size, True)
        if self.data_root is None and self.dataroot is not None:
            self.data_root = self.dataroot
        if self.dataroot is None and self.data_root is not None:
            self.dataroot = self.data_root
        if self.logger_name is None:
            self.logger_name = 'seg_trainer'
        if self.dataset in ('polyp', 'synthetic'):
            self.num_class = 2 if self.num_class == -1 else self.num_class
            self.num_channel = 3 if self.num_channel is None else self.num_channel
        self._auto_derived = auto
        self.check_augment()           # after crop_h / crop_w are derived: the blur radius is checked against them
        return self

    def check_augment(self):
        """Validate the rotation / shift / elastic / gamma / blur / noise fields; ranges become ``(lo, hi)``."""
        for name in ('aug_affine_p', 'aug_elastic_p', 'aug_gamma_p', 'aug_blur_p', 'aug_noise_p'):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:
                raise ValueError(f'{name} must be in [0, 1], got {getattr(self, name)!r}')
        if not 0.0 <= float(self.aug_rotate) <= 180.0:
            raise ValueError(f'aug_rotate must be in [0, 180] degrees, got {self.aug_rotate!r}')
        if not 0.0 <= float(self.aug_shift) <= 1.0:
            raise ValueError(f'aug_shift must be in [0, 1] (a fraction of the crop), got {self.aug_shift!r}')
        if not 0.0 <= float(self.aug_elastic_sigma) <= 64.0:
            raise ValueError(f'aug_elastic_sigma must be in [0, 64] pixels, got {self.aug_elastic_sigma!r}')
        if int(self.aug_elastic_cells) != self.aug_elastic_cells or not 1 <= self.aug_elastic_cells <= 8:
            raise ValueError(f'aug_elastic_cells must be an integer in 1..8, got {self.aug_elastic_cells!r}')
        if self.aug_border not in ('reflect', 'constant'):
            raise ValueError(f"aug_border must be 'reflect' or 'constant', got {self.aug_border!r}")

        def pair(name, lo_min, hi_max, lo_open=False):
            v = getattr(self, name)
            if v is None:
                return None
            v = list(v) if isinstance(v, (tuple, list)) else [v, v]
            if (len(v) != 2 or not all(isinstance(x, (int, float)) for x in v) or v[0] > v[1] or v[0] < lo_min
                    or (lo_open and v[0] <= lo_min) or v[1] > hi_max):
                raise ValueError(f"{name} must be [lo, hi] with {lo_min} {'<' if lo_open else '<='} lo <= hi <= "
                                 f'{hi_max}, got {getattr(self, name)!r}')
            setattr(self, name, (float(v[0]), float(v[1])))
            return getattr(self, name)

        pair('aug_gamma', 0.0, 10.0, lo_open=True)
        pair('aug_noise_std', 0.0, 255.0)
        blur = pair('aug_blur_sigma', 0.0, 2.5, lo_open=True)
        if blur is not None and self.crop_h is not None and self.crop_w is not None:
            import math
            radius = min(int(math.ceil(3.0 * blur[1])), 8)
            if 2 * radius >= min(self.crop_h, self.crop_w):
                raise ValueError(f'aug_blur_sigma {blur!r}: twice the blur radius ({radius}) must be below the crop '
                                 f'({self.crop_h} x {self.crop_w})')

    def check_calibration(self):
        """Validate the calibration / temperature / uncertainty fields."""
        for name, lo, hi in (('calibration_bins', 1, 64), ('calibration_rounds', 1, 4)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or not lo <= v <= hi:
                raise ValueError(f'{name} must be an integer in {lo}..{hi}, got {v!r}')
            setattr(self, name, int(v))
        if not isinstance(self.calibrate_temperature, bool):
            raise ValueError(f'calibrate_temperature must be a bool, got {self.calibrate_temperature!r}')
        t = self.temperature
        if t is not None and (isinstance(t, bool) or not isinstance(t, (int, float)) or not 0 < t < float('inf')):
            raise ValueError(f'temperature must be None or a finite number > 0, got {t!r}')
        if self.save_uncertainty not in (None, 'entropy', 'confidence'):
            raise ValueError(f"save_uncertainty must be None, 'entropy' or 'confidence', got {self.save_uncertainty!r}")

    INFERENCE_FIELDS = ('infer_window', 'infer_overlap', 'infer_blend', 'infer_sigma_scale', 'infer_batch',
                        'tta_flips', 'tta_average')

    def set_inference(self, **fields):
        """Set sliding-window / TTA fields by name (``None`` keeps the current value), validate them and return
        :meth:`inference_settings` -- for callers that do not go through the parser (``app.py``)."""
        for k, v in fields.items():
            if k not in self.INFERENCE_FIELDS:
                raise ValueError(f'unknown inference option {k!r} (one of {self.INFERENCE_FIELDS})')
            if v is not None:
                setattr(self, k, v)
        self.check_inference()
        return self.inference_settings()

    def check_inference(self):
        """Validate the sliding-window / TTA fields; ``infer_window`` is normalised to ``None`` or ``(h, w)``."""
        if not 0.0 <= float(self.infer_overlap) <= 0.75:
            raise ValueError(f'infer_overlap must be in [0, 0.75], got {self.infer_overlap!r}')
        if self.infer_blend not in ('gaussian', 'constant'):
            raise ValueError(f"infer_blend must be 'gaussian' or 'constant', got {self.infer_blend!r}")
        if self.tta_flips not in ('', 'h', 'v', 'hv'):
            raise ValueError(f"tta_flips must be '', 'h', 'v' or 'hv', got {self.tta_flips!r}")
        if self.tta_average not in ('logits', 'probs'):
            raise ValueError(f"tta_average must be 'logits' or 'probs', got {self.tta_average!r}")
        if not float(self.infer_sigma_scale) > 0:
            raise ValueError(f'infer_sigma_scale must be > 0, got {self.infer_sigma_scale!r}')
        if int(self.infer_batch) != self.infer_batch or self.infer_batch < 1:
            raise ValueError(f'infer_batch must be an integer >= 1, got {self.infer_batch!r}')
        win = self.infer_window
        if win is not None:
            win = list(win) if isinstance(win, (tuple, list)) else [win]
            if len(win) == 1:
                win = win * 2
            stride = max(1, int(self.val_img_stride))
            if len(win) != 2 or any(int(v) != v or v < 1 or v % stride for v in win):
                raise ValueError(f'infer_window must be one or two positive multiples of val_img_stride ({stride}), '
                                 f'got {self.infer_window!r}')
            self.infer_window = (int(win[0]), int(win[1]))

    def inference_settings(self):
        """``None`` when neither sliding windows nor flip TTA are asked for, else the keyword arguments of
        ``ops.tiled.sliding_window_inference`` (``window`` None: the caller takes the whole image)."""
        if self.infer_window is None and not self.tta_flips:
            return None
        return {'window': self.infer_window, 'overlap': float(self.infer_overlap), 'blend': self.infer_blend,
                'sigma_scale': float(self.infer_sigma_scale), 'flips': self.tta_flips, 'average': self.tta_average,
                'batch': int(self.infer_batch)}

    def to_dict(self):
        return {k: v for k, v in vars(self).items() if not k.startswith('_')}
