"""Losses -- reference ``core/loss.py:6-49``.

On a ROCm device with the HIP extension the CE / OHEM / KD-KL losses run the fused single-pass
kernels of ``csrc/loss.hip`` (loss + gradient in one pass); elsewhere plain PyTorch with identical
semantics.  Added (north star): ``'bce_dice'`` for ``num_class == 1``, and for
softmax heads (``num_class >= 2``) the overlap / focal family of :class:`RegionLoss`: ``dice``,
``tversky``, ``focal``, ``ce_dice``, ``ce_tversky``, ``focal_dice``, ``focal_tversky``.  Each of those, and the
empty base, can carry the boundary (signed-distance) term of :class:`BoundaryLoss`: ``boundary``,
``ce_boundary``, ``ce_dice_boundary`` and so on.  :class:`LovaszSoftmaxLoss` adds the Lovasz-softmax surrogate of the
Jaccard index: ``lovasz_softmax``, ``ce_lovasz_softmax``, ``focal_lovasz_softmax``.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import _ext


def _fused_ok(t):
    return t.is_cuda and t.dim() == 4 and _ext.available()


class CrossEntropyLoss(nn.Module):
    def __init__(self, ignore_index=255, reduction='mean', weight=None):
        super().__init__()
        self.ignore_index, self.reduction = ignore_index, reduction
        self.register_buffer('weight', weight if weight is None else weight.float())

    def forward(self, logits, labels):
        if self.reduction == 'mean' and _fused_ok(logits):
            from ..ops.losses import cross_entropy
            return cross_entropy(logits.float(), labels, self.weight, self.ignore_index)
        return F.cross_entropy(logits.float(), labels, weight=self.weight, ignore_index=self.ignore_index,
                               reduction=self.reduction)


class OhemCELoss(nn.Module):
    """Online hard example mining CE (reference core/loss.py:6-20), device-agnostic threshold."""

    def __init__(self, thresh, ignore_index=255):
        super().__init__()
        self.thresh = -math.log(thresh)
        self.ignore_index = ignore_index

    def forward(self, logits, labels):
        if _fused_ok(logits):
            from ..ops.losses import ohem_cross_entropy
            return ohem_cross_entropy(logits.float(), labels, math.exp(-self.thresh), self.ignore_index)
        n_min = labels[labels != self.ignore_index].numel() // 16
        loss = F.cross_entropy(logits.float(), labels, ignore_index=self.ignore_index, reduction='none').view(-1)
        loss_hard = loss[loss > self.thresh]
        if loss_hard.numel() < n_min:
            loss_hard, _ = loss.topk(n_min)
        return torch.mean(loss_hard)


class BceDiceLoss(nn.Module):
    """Binary (num_class == 1) loss: BCE-with-logits + soft Dice on the sigmoid."""

    def __init__(self, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
        super().__init__()
        self.bw, self.dw, self.smooth = bce_weight, dice_weight, smooth

    def forward(self, logits, labels):
        logits = logits.float()
        target = labels.float().view_as(logits) if labels.dim() == logits.dim() else labels.float().unsqueeze(1)
        if _fused_ok(logits):
            from ..ops.losses import bce_dice
            return bce_dice(logits, target, self.bw, self.dw, self.smooth)
        bce = F.binary_cross_entropy_with_logits(logits, target)
        p = torch.sigmoid(logits)
        inter = (p * target).flatten(1).sum(1)
        den = p.flatten(1).sum(1) + target.flatten(1).sum(1)
        dice = 1 - ((2 * inter + self.smooth) / (den + self.smooth)).mean()
        return self.bw * bce + self.dw * dice


class RegionLoss(nn.Module):
    """Softmax-head (``num_class >= 2``) loss: ``pixel_weight * L_pix + region_weight * L_reg``.

    A pixel is valid iff ``label != ignore_index and 0 <= label < C``; with ``p = softmax(logits)``,
    ``y_c = [label == c]`` and ``w_c = weight[c]`` (or 1):

    * ``L_pix = sum_valid(w_t l) / sum_valid(w_t)`` over the batch, ``l = -log p_t`` (``pixel='ce'``) or
      ``-(1 - p_t)^gamma log p_t`` (``'focal'``; ``gamma`` is 0 -- exactly CE -- or >= 1, since the gradient
      of a fractional power below 1 is unbounded at ``p_t -> 1``).  With no valid pixel ``L_pix`` is 0
      with zero gradient (``F.cross_entropy`` gives NaN there).
    * ``L_reg = 1 - mean_{n, c} TI_nc`` with, over the valid pixels of sample ``n``, ``I = sum p_c y_c``,
      ``P = sum p_c``, ``T = sum y_c`` and ``TI = (I + s) / (I + a (P - I) + b (T - I) + s)``:
      ``region='tversky'`` uses ``a = alpha``, ``b = beta``, ``s = smooth``; ``'dice'`` is ``a = b = 0.5``,
      ``s = smooth / 2``, i.e. ``(2I + smooth) / (P + T + smooth)`` as in :class:`BceDiceLoss`.
      ``ignore_background`` leaves class 0 out of the mean.

    The region sums are per sample, so nothing is exchanged across DDP ranks: every rank's loss is the mean
    over its own samples, the same semantics as ``ce``.  On a ROCm device with the HIP extension this is
    ``ops.losses.region_loss`` (fused, deterministic, graph-capturable); elsewhere the plain-torch form
    below, in the input's floating dtype."""

    def __init__(self, pixel='ce', region='dice', ignore_index=255, weight=None, pixel_weight=1.0, region_weight=1.0,
                 smooth=1.0, alpha=0.3, beta=0.7, gamma=2.0, ignore_background=False):
        super().__init__()
        if pixel not in (None, 'ce', 'focal') or region not in (None, 'dice', 'tversky') or pixel == region:
            raise ValueError(f'RegionLoss: pixel={pixel!r} region={region!r}')
        if pixel == 'focal' and not (gamma == 0 or gamma >= 1):
            raise ValueError(f'focal_gamma must be 0 or >= 1, got {gamma}')
        self.pixel, self.region, self.ignore_index = pixel, region, ignore_index
        self.pw, self.rw = float(pixel_weight), float(region_weight)
        self.smooth, self.alpha, self.beta, self.gamma = float(smooth), float(alpha), float(beta), float(gamma)
        self.ignore_background = bool(ignore_background)
        self.register_buffer('weight', weight if weight is None else weight.float())

    def forward(self, logits, labels):
        if _fused_ok(logits):
            from ..ops.losses import region_loss
            return region_loss(logits.float(), labels, self.weight, self.ignore_index, self.pixel, self.region,
                               self.pw, self.rw, self.smooth, self.alpha, self.beta, self.gamma,
                               self.ignore_background)
        x = logits if logits.dtype in (torch.float32, torch.float64) else logits.float()
        C = x.shape[1]
        valid = (labels != self.ignore_index) & (labels >= 0) & (labels < C)
        vf = valid.unsqueeze(1).to(x.dtype)
        y = F.one_hot(torch.where(valid, labels, torch.zeros_like(labels)), C).movedim(-1, 1).to(x.dtype) * vf
        p = F.softmax(x, 1)
        loss = x.new_zeros(())
        if self.pixel is not None:
            logpt = (F.log_softmax(x, 1) * y).sum(1)               # x_t - lse; 0 on ignored pixels
            l = -logpt
            if self.pixel == 'focal' and self.gamma != 0:
                l = l * (p * (vf - y)).sum(1) ** self.gamma        # 1 - p_t as the sum over the other classes
            w = vf[:, 0] if self.weight is None else (y * self.weight.to(x.dtype).view(1, C, 1, 1)).sum(1)
            W = w.sum()
            loss = loss + self.pw * torch.where(W > 0, (w * l).sum() / torch.where(W > 0, W, torch.ones_like(W)),
                                                torch.zeros_like(W))
        if self.region is not None:
            a, b, s = (0.5, 0.5, 0.5 * self.smooth) if self.region == 'dice' else (self.alpha, self.beta, self.smooth)
            inter, ps, ts = (p * y).sum((2, 3)), (p * vf).sum((2, 3)), y.sum((2, 3))
            ti = (inter + s) / (inter + a * (ps - inter) + b * (ts - inter) + s)
            loss = loss + self.rw * (1 - ti[:, 1 if self.ignore_background else 0:].mean())
        return loss


def boundary_weight_at(epoch, weight, ramp_epochs):
    """Weight of the boundary term in 0-based ``epoch``: ``weight * min(1, (epoch + 1) / ramp_epochs)`` for
    ``ramp_epochs > 0`` (the "increase" schedule of the paper), ``weight`` for 0.  A function of the epoch alone,
    so a resumed run needs nothing from the checkpoint."""
    if ramp_epochs <= 0:
        return float(weight)
    return float(weight) * min(1.0, (int(epoch) + 1) / float(ramp_epochs))


class BoundaryLoss(nn.Module):
    """``base(logits, labels) + w * L_B`` for softmax heads: ``base`` an optional :class:`RegionLoss`, ``L_B`` the
    boundary loss of Kervadec et al. (MIDL 2019),

        ``L_B = sum_{n, c in S, valid x} p_c(x) * phi_nc(x) / (|S| * max(V, 1))``

    with ``p = softmax(logits)``, ``phi`` the signed distance map of ``ops.surface.signed_distance`` (negative
    inside class ``c``, positive outside, 0 at invalid pixels and for a class absent from or filling the image),
    ``S`` the foreground classes (all classes with ``include_background``) and ``V`` the number of valid pixels of
    the batch (the :class:`RegionLoss` rule).  No valid pixel: ``L_B`` is 0 with zero gradient.  A mean over the
    rank's own pixels: nothing is exchanged under DDP.

    ``w`` lives in the one-element buffer ``bw`` on the device, so a captured graph reads the current value:
    :meth:`set_epoch` fills it with ``weight * min(1, (epoch + 1) / ramp_epochs)`` (``weight`` when
    ``ramp_epochs == 0``) and no re-capture is needed.  On a ROCm device with the HIP extension ``L_B`` is
    ``ops.losses.boundary_loss``; elsewhere the plain-torch form below, in the input's floating dtype."""

    def __init__(self, base=None, weight=0.01, ramp_epochs=0, ignore_index=255, include_background=False,
                 device=None):
        super().__init__()
        if base is not None and not isinstance(base, RegionLoss):
            raise ValueError(f'BoundaryLoss: base must be a RegionLoss or None, got {type(base).__name__}')
        if not float(weight) >= 0:
            raise ValueError(f'loss_boundary_weight must be >= 0, got {weight!r}')
        if int(ramp_epochs) != ramp_epochs or ramp_epochs < 0:
            raise ValueError(f'boundary_ramp_epochs must be an integer >= 0, got {ramp_epochs!r}')
        self.base, self.weight, self.ramp_epochs = base, float(weight), int(ramp_epochs)
        self.ignore_index, self.include_background = ignore_index, bool(include_background)
        self.register_buffer('bw', torch.full((1,), boundary_weight_at(0, weight, ramp_epochs), dtype=torch.float32,
                                              device=device), persistent=False)

    def set_epoch(self, epoch):
        self.bw.fill_(boundary_weight_at(epoch, self.weight, self.ramp_epochs))

    def classes(self, num_class):
        return list(range(0 if self.include_background else 1, num_class))

    def boundary_term(self, logits, labels):
        cls = self.classes(logits.shape[1])
        if _fused_ok(logits):
            from ..ops.losses import boundary_loss
            return boundary_loss(logits.float(), labels, self.ignore_index, cls)
        from ..ops.surface import signed_distance
        x = logits if logits.dtype in (torch.float32, torch.float64) else logits.float()
        C = x.shape[1]
        valid = (labels != self.ignore_index) & (labels >= 0) & (labels < C)
        phi = signed_distance(labels, C, self.ignore_index, cls).to(x.dtype)     # 0 at invalid pixels
        V = valid.sum().clamp_min(1).to(x.dtype)
        return (F.softmax(x, 1)[:, cls] * phi).sum() / (len(cls) * V)

    def forward(self, logits, labels):
        lb = self.boundary_term(logits, labels)
        loss = self.bw.to(lb.dtype).reshape(()) * lb
        return loss if self.base is None else self.base(logits, labels) + loss


class LovaszSoftmaxLoss(nn.Module):
    """``base(logits, labels) + weight * L`` for softmax heads: ``base`` an optional pixel-only :class:`RegionLoss`
    (``region=None``), ``L`` the Lovasz-softmax loss of Berman et al. (CVPR 2018), the convex surrogate of the
    Jaccard index, over the classes present in a segment.

    With ``p = softmax(logits)`` and the :class:`RegionLoss` validity rule, a segment is the whole batch
    (``per_image=False``, as in Berman's code) or one image.  For a segment ``s`` and class ``c``, over the valid
    pixels of ``s``: ``y = [label == c]``, ``e = |y - p_c|``, ``G = sum y``; the class is *present* iff ``G > 0``.
    The pixels are sorted by ``e`` descending, ties in ascending pixel index (raster order, ``n`` major in batch
    mode).  Along that order, with ``F_i`` the number of ``y = 1`` among the first ``i + 1`` pixels and
    ``B_i = i + 1 - F_i``: ``I_i = G - F_i``, ``U_i = G + B_i``, ``J_i = 1 - I_i / U_i`` and
    ``g_i = J_i - J_{i-1}`` (``J_{-1} = 0``), i.e. ``g_i = 1 / U_i`` where ``y_i = 1`` and
    ``I_i / (U_i (U_i - 1))`` where ``y_i = 0``.  ``L_sc = sum_i e_i g_i`` with ``g`` a constant under
    differentiation; ``L_s`` is the mean of ``L_sc`` over the present classes (class 0 left out with
    ``ignore_background``; 0 if none is left) and ``L = mean_s L_s``: an image without a valid pixel adds 0 and
    still counts.  No valid pixel at all: ``L = 0`` with zero gradient.

    Only the 'present' mode, no class weights.  The batch-mode sort is over the rank's own micro-batch: nothing is
    exchanged across DDP ranks or accumulation micro-batches, the same semantics as ``ce``.  On a ROCm device with
    the HIP extension ``L`` is ``ops.losses.lovasz_softmax`` (fused, deterministic, graph-capturable); elsewhere
    the plain-torch form below, in the input's floating dtype: invalid pixels carry the error 0 instead of being
    compacted (everything at ``e = 0`` contributes nothing), so there is no boolean indexing and no host sync."""

    def __init__(self, base=None, weight=1.0, per_image=False, ignore_index=255, ignore_background=False):
        super().__init__()
        if base is not None and not (isinstance(base, RegionLoss) and base.region is None):
            raise ValueError('LovaszSoftmaxLoss: base must be a pixel-only RegionLoss (region=None) or None, got '
                             f'{type(base).__name__}')
        self.base, self.weight, self.per_image = base, float(weight), bool(per_image)
        self.ignore_index, self.ignore_background = ignore_index, bool(ignore_background)

    def lovasz_term(self, logits, labels):
        if logits.dim() == 4 and logits.shape[1] == 1:
            raise ValueError('LovaszSoftmaxLoss needs a softmax head: num_class must be >= 2, got 1')
        if _fused_ok(logits):
            from ..ops.losses import lovasz_softmax
            return lovasz_softmax(logits.float(), labels, self.ignore_index, self.per_image, self.ignore_background)
        return self.plain_term(logits, labels)

    def plain_term(self, logits, labels):
        """The specification in plain torch (``torch.sort``), on any device."""
        x = logits if logits.dtype in (torch.float32, torch.float64) else logits.float()
        N, C = x.shape[:2]
        valid = (labels != self.ignore_index) & (labels >= 0) & (labels < C)
        vf = valid.unsqueeze(1).to(x.dtype)
        y = F.one_hot(torch.where(valid, labels, torch.zeros_like(labels)), C).movedim(-1, 1).to(x.dtype) * vf
        e = (y - F.softmax(x, 1)).abs() * vf                       # 0 at invalid pixels
        if self.per_image:                                         # rows [S, C, P]
            e, y = e.flatten(2), y.flatten(2)
        else:
            e, y = e.movedim(1, 0).reshape(1, C, -1), y.movedim(1, 0).reshape(1, C, -1)
        es, order = torch.sort(e, dim=-1, descending=True, stable=True)
        ys = y.detach().gather(-1, order).long()
        G = ys.sum(-1, keepdim=True)
        Fi = ys.cumsum(-1)
        U = G + torch.arange(1, e.shape[-1] + 1, device=x.device) - Fi           # G + B_i
        g = torch.where(ys > 0, 1 / U.clamp_min(1).to(x.dtype),
                        (G - Fi).to(x.dtype) / (U * (U - 1)).clamp_min(1).to(x.dtype))
        present = (G[..., 0] > 0).to(x.dtype)                      # [S, C]
        if self.ignore_background:
            present = present * (torch.arange(C, device=x.device) > 0).to(x.dtype)
        Lsc = (es * g).sum(-1) * present
        return (Lsc.sum(1) / present.sum(1).clamp_min(1)).mean()

    def forward(self, logits, labels):
        loss = self.weight * self.lovasz_term(logits, labels)
        return loss if self.base is None else self.base(logits, labels) + loss


_PIXEL_TERMS, _REGION_TERMS = ('ce', 'focal'), ('dice', 'tversky')
REGION_LOSS_TYPES = ('dice', 'tversky', 'focal', 'ce_dice', 'ce_tversky', 'focal_dice', 'focal_tversky')
BOUNDARY_LOSS_TYPES = ('boundary', 'ce_boundary', 'focal_boundary', 'dice_boundary', 'tversky_boundary',
                       'ce_dice_boundary', 'ce_tversky_boundary', 'focal_dice_boundary', 'focal_tversky_boundary')
LOVASZ_LOSS_TYPES = ('lovasz_softmax', 'ce_lovasz_softmax', 'focal_lovasz_softmax')


def _region_loss_of(terms, config, weights):
    pixel = next((k for k in terms if k in _PIXEL_TERMS), None)
    region = next((k for k in terms if k in _REGION_TERMS), None)
    return RegionLoss(pixel, region, ignore_index=config.ignore_index, weight=weights,
                      pixel_weight=config.loss_pixel_weight, region_weight=config.loss_region_weight,
                      smooth=config.dice_smooth, alpha=config.tversky_alpha, beta=config.tversky_beta,
                      gamma=config.focal_gamma, ignore_background=config.dice_ignore_background)


def get_loss_fn(config, device):
    weights = None if config.class_weights is None else torch.tensor(config.class_weights, dtype=torch.float32,
                                                                      device=device)
    lt = config.loss_type
    if lt == 'ce':
        return CrossEntropyLoss(ignore_index=config.ignore_index, reduction=config.reduction, weight=weights)
    if lt == 'ohem':
        return OhemCELoss(thresh=config.ohem_thrs, ignore_index=config.ignore_index)
    multi = config.num_class >= 2
    if lt in ('bce_dice', 'bce', 'dice') and not multi:
        bw = 0.0 if lt == 'dice' else 1.0
        dw = 0.0 if lt == 'bce' else 1.0
        return BceDiceLoss(bw, dw)
    if lt in ('bce_dice', 'bce'):
        raise ValueError(f"loss_type '{lt}' is for a one-channel sigmoid head, but num_class = {config.num_class}; "
                         f"use one of {REGION_LOSS_TYPES}")
    if lt in REGION_LOSS_TYPES:
        if not multi:
            raise ValueError(f"loss_type '{lt}' needs a softmax head, but num_class = {config.num_class}; "
                             f"use 'bce', 'dice' or 'bce_dice'")
        return _region_loss_of(lt.split('_'), config, weights)
    if lt in BOUNDARY_LOSS_TYPES:
        if not multi:
            raise ValueError(f"loss_type '{lt}' needs a softmax head (the boundary term integrates the softmax "
                             f"against per-class distance maps), but num_class = {config.num_class}")
        terms = lt.split('_')[:-1]
        base = _region_loss_of(terms, config, weights) if terms else None
        return BoundaryLoss(base, weight=config.loss_boundary_weight, ramp_epochs=config.boundary_ramp_epochs,
                            ignore_index=config.ignore_index, include_background=config.boundary_include_background,
                            device=device)
    if lt in LOVASZ_LOSS_TYPES:
        if not multi:
            raise ValueError(f"loss_type '{lt}' needs a softmax head (the Lovasz-softmax errors are taken on the "
                             f"softmax), but num_class = {config.num_class}")
        pixel = lt[:-len('_lovasz_softmax')] if lt != 'lovasz_softmax' else None
        base = _region_loss_of([pixel], config, weights) if pixel else None
        return LovaszSoftmaxLoss(base, weight=config.loss_region_weight, per_image=config.lovasz_per_image,
                                 ignore_index=config.ignore_index, ignore_background=config.dice_ignore_background)
    raise NotImplementedError(f'Unsupport loss type: {lt}')


def kd_loss_fn(config, outputs, outputsT):
    if config.kd_loss_type == 'kl_div':
        if _fused_ok(outputs):
            from ..ops.losses import kd_kl_div
            return kd_kl_div(outputs.float(), outputsT.detach().float(), config.kd_temperature)
        T = config.kd_temperature
        return F.kl_div(F.log_softmax(outputs / T, dim=1), F.softmax(outputsT.detach() / T, dim=1),
                        reduction='mean') * T ** 2
    if config.kd_loss_type == 'mse':
        if _fused_ok(outputs):
            from ..ops.losses import kd_mse
            return kd_mse(outputs.float(), outputsT.detach().float())
        return F.mse_loss(outputs, outputsT.detach())
    raise NotImplementedError(f'Unsupport kd loss type: {config.kd_loss_type}')
