"""Segmentation metrics -- reference ``utils/metrics.py:4-13`` (torchmetrics 1.2.0 ``JaccardIndex``
(task='multiclass', ignore_index, average='none') and ``Dice`` (average='macro')), SURVEY App. C.

Both accumulate ONE ``[C, C]`` int64 confusion matrix (``confmat[target][pred]`` with the per-pixel
argmax prediction): on MI355X it is filled by the ``confmat_update`` HIP kernel (LDS histogram),
on CPU by ``torch.bincount``.  ``compute()`` all-reduces the matrix across ranks (one RCCL
all-reduce of C*C int64, instead of torchmetrics' per-state all_gathers) and derives:
  * IoU per class  = TP / (TP + FP + FN)
  * Dice (macro)   = mean over classes present of 2TP / (2TP + FP + FN)   (includes background)
Dice here ignores no index (the reference constructs ``Dice`` without ``ignore_index``), IoU drops
``ignore_index`` pixels; for {0,1} polyp masks both see the same pixels.

Boundary metrics (an addition over the reference): ``HausdorffDistance95``, ``AverageSurfaceDistance`` and
``SurfaceDice`` score the foreground classes' contours per image (``ops/surface.py`` has the semantics; on
MI355X the ``surface.hip`` distance-transform kernels).  The three share one :class:`SurfaceAccumulator`, so a
batch's statistics are computed once however many of them are requested.

Lesion-wise metrics (an addition too): ``LesionRecall``, ``LesionPrecision`` and ``LesionF1`` count connected
components instead of pixels -- how many ground-truth lesions were found and how many predicted blobs were false
alarms (``ops/components.py`` has the semantics; on MI355X the ``components.hip`` labelling kernels).  They share
one :class:`LesionAccumulator` in the same way.

Calibration metrics (an addition as well): ``ExpectedCalibrationError``, ``MaximumCalibrationError``,
``NegativeLogLikelihood`` and ``BrierScore`` score the probabilities instead of the label map, at the temperature of
their shared :class:`CalibrationAccumulator` (``ops/calibration.py`` has the semantics; on MI355X the
``calibration.hip`` kernels).
"""
from __future__ import annotations

import weakref

import torch
import torch.distributed as dist
import torch.nn as nn


def confmat_torch(preds, target, num_classes, ignore_index=None):
    if preds.dim() == target.dim() + 1:
        pred = preds.argmax(1)
    else:
        pred = preds
    t = target.reshape(-1).long()
    p = pred.reshape(-1).long()
    valid = (t >= 0) & (t < num_classes)
    if ignore_index is not None:
        valid &= t != ignore_index
    idx = t[valid] * num_classes + p[valid]
    return torch.bincount(idx, minlength=num_classes * num_classes).view(num_classes, num_classes)


class _ConfmatMetric(nn.Module):
    def __init__(self, num_classes, ignore_index=None, sync=True, group=None):
        super().__init__()
        self.group = group
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.sync = sync
        self.register_buffer('confmat', torch.zeros(num_classes, num_classes, dtype=torch.long))

    @torch.no_grad()
    def update(self, preds, target):
        target = target.to(self.confmat.device)
        preds = preds.to(self.confmat.device)
        if preds.is_cuda and preds.dim() == 4 and preds.dtype == torch.float32 and self.num_classes ** 2 <= 1024:
            from ..ops import _ext
            if _ext.available():
                ig = self.ignore_index if self.ignore_index is not None else -1
                _ext.require().confmat_update(preds.contiguous(), target.contiguous().long(), self.confmat, ig)
                return
        self.confmat += confmat_torch(preds, target, self.num_classes, self.ignore_index)

    def _synced(self):
        cm = self.confmat.clone()
        if self.sync and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(cm, group=self.group)
        return cm

    def reset(self):
        self.confmat.zero_()


class JaccardIndex(_ConfmatMetric):
    def __init__(self, task='multiclass', num_classes=2, ignore_index=None, average='none', sync=True):
        assert task == 'multiclass'
        super().__init__(num_classes, ignore_index, sync)
        self.average = average

    def compute(self):
        cm = self._synced().double()
        tp = cm.diag()
        fp = cm.sum(0) - tp
        fn = cm.sum(1) - tp
        iou = tp / (tp + fp + fn).clamp_min(1e-12)
        iou = torch.where(tp + fp + fn > 0, iou, torch.zeros_like(iou))
        if self.average == 'macro':
            return iou.mean().float()
        return iou.float()


class Dice(_ConfmatMetric):
    def __init__(self, num_classes=2, average='macro', ignore_index=None, sync=True):
        super().__init__(num_classes, ignore_index, sync)
        self.average = average

    def compute(self):
        cm = self._synced().double()
        tp = cm.diag()
        fp = cm.sum(0) - tp
        fn = cm.sum(1) - tp
        den = 2 * tp + fp + fn
        present = den > 0
        dice = torch.where(present, 2 * tp / den.clamp_min(1e-12), torch.zeros_like(tp))
        if self.average == 'macro':
            return (dice[present].mean() if present.any() else dice.sum() * 0).float()
        return dice.float()


def foreground_dice(preds, target, fg=1):
    """Per-image foreground Dice averaged over images (the DUCK-Net paper's convention)."""
    pred = preds.argmax(1) if preds.dim() == target.dim() + 1 else preds
    p = (pred == fg).flatten(1).float()
    t = (target == fg).flatten(1).float()
    inter = (p * t).sum(1)
    den = p.sum(1) + t.sum(1)
    return torch.where(den > 0, 2 * inter / den.clamp_min(1e-12), torch.ones_like(den)).mean()


class SurfaceAccumulator(nn.Module):
    """Per-class state of the boundary metrics: fp64 sums of the per-image hd95 / assd / nsd, the number of
    scored (image, class) pairs and the number of those with exactly one empty mask.  Shared by the metric
    objects built from one config: ``update`` by a metric that has not yet seen the batch the accumulator scored
    last is a no-op (the tensors are held until the next batch), ``reset`` by any of them zeroes it once."""

    def __init__(self, num_classes, ignore_index=None, nsd_tolerance=2.0):
        super().__init__()
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.nsd_tolerance = float(nsd_tolerance)
        k = num_classes - 1
        self.register_buffer('sum', torch.zeros(3, k, dtype=torch.float64))
        self.register_buffer('count', torch.zeros(k, dtype=torch.long))
        self.register_buffer('onesided', torch.zeros(k, dtype=torch.long))
        self._last, self._seen = None, set()

    @torch.no_grad()
    def update(self, preds, target, owner=None):
        # the same batch again from another metric of the group (``owner``): same memory, same shape, not written
        # since.  The tensors are held, so their storage cannot be handed to another batch in between.
        key = tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t._version) for t in (preds, target))
        if self._last is not None and self._last[0] == key and owner is not None and owner not in self._seen:
            self._seen.add(owner)
            return
        from ..ops.surface import surface_stats
        dev = self.sum.device
        surface_stats(preds.to(dev), target.to(dev), self.num_classes, self.ignore_index, self.nsd_tolerance,
                      {'sum': self.sum, 'count': self.count, 'onesided': self.onesided})
        self._last, self._seen = (key, preds, target), {owner}

    def reset(self):
        self.sum.zero_()
        self.count.zero_()
        self.onesided.zero_()
        self._last, self._seen = None, set()


class _SurfaceMetric(nn.Module):
    """Mean over the foreground classes with a scored pair of (sum of per-image values / scored pairs); nan when
    nothing was scored.  ``compute`` all-reduces the packed state once (SUM over ``group``)."""
    row = 0

    def __init__(self, num_classes=2, ignore_index=None, nsd_tolerance=2.0, sync=True, group=None, accumulator=None):
        super().__init__()
        if num_classes < 2:
            raise ValueError('surface metrics need num_classes >= 2')
        self.group = group
        self.num_classes = num_classes
        self.sync = sync
        self.last_one_sided = None     # set by compute(): [C-1] one-sided-empty pairs over all ranks
        self.acc = accumulator if accumulator is not None else SurfaceAccumulator(num_classes, ignore_index,
                                                                                  nsd_tolerance)
        if self.acc.num_classes != num_classes:
            raise ValueError('shared accumulator was built for another number of classes')

    def update(self, preds, target):
        self.acc.update(preds, target, owner=id(self))

    def reset(self):
        self.acc.reset()

    def _synced(self):
        a = self.acc
        st = torch.cat([a.sum[self.row:self.row + 1], a.count[None].double(), a.onesided[None].double()])
        if self.sync and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(st, group=self.group)
        return st

    def _per_class(self, st):
        return torch.where(st[1] > 0, st[0] / st[1].clamp_min(1.0), torch.full_like(st[0], float('nan')))

    def per_class(self):
        """``[C-1]`` fp32 per foreground class, nan where no pair was scored."""
        return self._per_class(self._synced()).float()

    def one_sided(self):
        """``[C-1]`` int64: scored pairs in which exactly one of the two masks was empty (all ranks; a
        collective like ``compute``, which leaves the same vector in ``last_one_sided``)."""
        return self._synced()[2].round().long()

    def compute(self):
        st = self._synced()
        self.last_one_sided = st[2].round().long()
        pc = self._per_class(st)
        scored = st[1] > 0
        # nanmean without a host sync: nan (0 / 0) when no class was scored
        return (torch.where(scored, pc, torch.zeros_like(pc)).sum() / scored.sum()).float()


class HausdorffDistance95(_SurfaceMetric):
    """Per-image max of the two directional 95th-percentile boundary distances (MONAI's convention, not
    medpy's pooled percentile), in pixels; lower is better."""
    row = 0


class AverageSurfaceDistance(_SurfaceMetric):
    """Average symmetric surface distance in pixels; lower is better."""
    row = 1


class SurfaceDice(_SurfaceMetric):
    """Normalised surface Dice: the fraction of both boundaries within ``nsd_tolerance`` pixels of the other."""
    row = 2


class LesionAccumulator(nn.Module):
    """Per-class state of the lesion-wise metrics: int64 ``counts [4, C-1]`` (GT components, GT hits, predicted
    components, predicted hits) and the labelling kernels' error counter.  Shared by the metric objects built
    from one config exactly as :class:`SurfaceAccumulator` is: a batch is scored once however many of them see
    it, and ``reset`` by any of them zeroes it once."""

    def __init__(self, num_classes, ignore_index=None, min_overlap=0.0, connectivity=8):
        super().__init__()
        if not 0.0 <= float(min_overlap) <= 1.0:
            raise ValueError(f'min_overlap must be in [0, 1], got {min_overlap}')
        if connectivity not in (4, 8):
            raise ValueError(f'connectivity must be 4 or 8, got {connectivity!r}')
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.min_overlap = float(min_overlap)
        self.connectivity = int(connectivity)
        self.register_buffer('counts', torch.zeros(4, num_classes - 1, dtype=torch.long))
        self.register_buffer('err', torch.zeros(1, dtype=torch.long))
        self._last, self._seen = None, set()

    @torch.no_grad()
    def update(self, preds, target, owner=None):
        key = tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t._version) for t in (preds, target))
        if self._last is not None and self._last[0] == key and owner is not None and owner not in self._seen:
            self._seen.add(owner)
            return
        from ..ops.components import lesion_stats
        dev = self.counts.device
        lesion_stats(preds.to(dev), target.to(dev), self.num_classes, self.ignore_index, self.min_overlap,
                     self.connectivity, {'counts': self.counts, 'err': self.err})
        self._last, self._seen = (key, preds, target), {owner}

    def reset(self):
        self.counts.zero_()
        self.err.zero_()
        self._last, self._seen = None, set()


class _LesionMetric(nn.Module):
    """Mean over the scored foreground classes of a ratio of component counts (``ops/components.py`` has the
    semantics); nan when no class is scored or the kernels reported an error.  ``compute`` all-reduces the packed
    int64 state once (SUM over ``group``)."""

    def __init__(self, num_classes=2, ignore_index=None, min_overlap=0.0, connectivity=8, sync=True, group=None,
                 accumulator=None):
        super().__init__()
        if num_classes < 2:
            raise ValueError('lesion metrics need num_classes >= 2')
        self.group = group
        self.num_classes = num_classes
        self.sync = sync
        self.acc = accumulator if accumulator is not None else LesionAccumulator(num_classes, ignore_index,
                                                                                 min_overlap, connectivity)
        if self.acc.num_classes != num_classes:
            raise ValueError('shared accumulator was built for another number of classes')

    def update(self, preds, target):
        self.acc.update(preds, target, owner=id(self))

    def reset(self):
        self.acc.reset()

    def _synced(self):
        st = torch.cat([self.acc.counts.reshape(-1), self.acc.err])
        if self.sync and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(st, group=self.group)
        return st[:-1].view(4, -1).double(), st[-1]

    @staticmethod
    def _ratio(hits, comps):
        return torch.where(comps > 0, hits / comps.clamp_min(1.0), torch.zeros_like(hits))

    def _values(self, c):
        """``c [4, C-1]`` fp64 -> (per-class value, per-class scored flag)"""
        raise NotImplementedError

    def counts(self):
        """``[4, C-1]`` int64 over all ranks (a collective like ``compute``): GT components, GT hits, predicted
        components, predicted hits."""
        return self._synced()[0].round().long()

    def per_class(self):
        """``[C-1]`` fp32 per foreground class, nan where the class is not scored."""
        c, err = self._synced()
        v, scored = self._values(c)
        return torch.where(scored & (err == 0), v, torch.full_like(v, float('nan'))).float()

    def compute(self):
        c, err = self._synced()
        v, scored = self._values(c)
        # nanmean without a host sync: nan (0 / 0) when no class was scored
        mean = torch.where(scored, v, torch.zeros_like(v)).sum() / scored.sum()
        return torch.where(err == 0, mean, torch.full_like(mean, float('nan'))).float()


class LesionRecall(_LesionMetric):
    """Found ground-truth components / ground-truth components; a class is scored iff it has ground-truth ones."""

    def _values(self, c):
        return self._ratio(c[1], c[0]), c[0] > 0


class LesionPrecision(_LesionMetric):
    """Predicted components that hit the ground truth / predicted components; scored iff the class has predicted
    ones."""

    def _values(self, c):
        return self._ratio(c[3], c[2]), c[2] > 0


class LesionF1(_LesionMetric):
    """2PR / (P + R) per class, a side without components counting 0; scored iff the class has components on either
    side."""

    def _values(self, c):
        r, p = self._ratio(c[1], c[0]), self._ratio(c[3], c[2])
        f1 = torch.where(p + r > 0, 2 * p * r / (p + r).clamp_min(1e-300), torch.zeros_like(p))
        return f1, (c[0] > 0) | (c[2] > 0)


class CalibrationAccumulator(nn.Module):
    """State of the calibration metrics: int64 ``ints [2, M]`` (per-bin pixel count and hits) and fp64
    ``sums [M + 2]`` (per-bin confidence sum, NLL sum, Brier sum), plus the one-element ``temperature`` the
    probabilities are taken at.  Shared by the metric objects built from one config exactly as
    :class:`SurfaceAccumulator` is: a batch is scored once however many of the four see it, and ``reset`` by any
    of them zeroes it once (the temperature stays)."""

    def __init__(self, num_classes, ignore_index=None, bins=15):
        super().__init__()
        from ..ops.calibration import new_state
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        st = new_state(bins)
        self.bins = st['ints'].shape[1]
        self.register_buffer('ints', st['ints'])
        self.register_buffer('sums', st['sums'])
        self.register_buffer('temperature', torch.ones(1, dtype=torch.float64))
        self._t = 1.0      # host copy of ``temperature``: the kernels take it by value, without a device read
        self._last, self._seen = None, set()

    def set_temperature(self, T):
        from ..ops.calibration import _check_temperature
        self._t = _check_temperature(T)
        self.temperature.fill_(self._t)

    @torch.no_grad()
    def update(self, preds, target, owner=None):
        key = tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t._version) for t in (preds, target))
        if self._last is not None and self._last[0] == key and owner is not None and owner not in self._seen:
            self._seen.add(owner)
            return
        from ..ops.calibration import calibration_stats, state_views
        dev = self.sums.device
        calibration_stats(preds.to(dev), target.to(dev), state_views(self.ints, self.sums), self._t,
                          self.ignore_index, self.bins)
        self._last, self._seen = (key, preds, target), {owner}

    def reset(self):
        self.ints.zero_()
        self.sums.zero_()
        self._last, self._seen = None, set()


class _CalibrationMetric(nn.Module):
    """One of (ece, mce, nll, brier) of the shared state (``ops/calibration.py`` has the semantics); nan when no
    pixel was scored; lower is better.  ``compute`` all-reduces the packed state once (SUM over ``group``)."""
    index = 0

    def __init__(self, num_classes=2, ignore_index=None, bins=15, sync=True, group=None, accumulator=None):
        super().__init__()
        if num_classes < 2:
            raise ValueError('calibration metrics need num_classes >= 2')
        self.group = group
        self.num_classes = num_classes
        self.sync = sync
        self.acc = accumulator if accumulator is not None else CalibrationAccumulator(num_classes, ignore_index, bins)
        if self.acc.num_classes != num_classes:
            raise ValueError('shared accumulator was built for another number of classes')

    def update(self, preds, target):
        self.acc.update(preds, target, owner=id(self))

    def reset(self):
        self.acc.reset()

    def _synced(self):
        """(counts ``[2, M]`` fp64, sums ``[M + 2]``) over all ranks; the counts are exact below 2^53"""
        a = self.acc
        st = torch.cat([a.ints.reshape(-1).double(), a.sums])
        if self.sync and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(st, group=self.group)
        return st[:2 * a.bins].view(2, a.bins), st[2 * a.bins:]

    def reliability(self):
        """Per bin over all ranks (a collective like ``compute``): int64 ``count``, and fp64 ``accuracy`` and mean
        ``confidence`` (nan in an empty bin)."""
        ints, sums = self._synced()
        den = ints[0].clamp_min(1.0)
        nan = torch.full_like(den, float('nan'))
        return {'count': ints[0].round().long(), 'accuracy': torch.where(ints[0] > 0, ints[1] / den, nan),
                'confidence': torch.where(ints[0] > 0, sums[:self.acc.bins] / den, nan)}

    def compute(self):
        from ..ops.calibration import metrics_from_state
        return metrics_from_state(*self._synced())[self.index].float()


class ExpectedCalibrationError(_CalibrationMetric):
    """``sum_b |correct_b - conf_sum_b| / V``: the mean gap between confidence and accuracy."""
    index = 0


class MaximumCalibrationError(_CalibrationMetric):
    """The largest per-bin gap between accuracy and mean confidence over the non-empty bins."""
    index = 1


class NegativeLogLikelihood(_CalibrationMetric):
    """Mean of ``logsumexp(z / T) - z_label / T`` over the valid pixels."""
    index = 2


class BrierScore(_CalibrationMetric):
    """Mean of ``sum_c (p_c - y_c)^2`` over the valid pixels."""
    index = 3


SURFACE_METRICS = {'hd95': HausdorffDistance95, 'assd': AverageSurfaceDistance, 'nsd': SurfaceDice}
LESION_METRICS = {'lesion_recall': LesionRecall, 'lesion_precision': LesionPrecision, 'lesion_f1': LesionF1}
CALIBRATION_METRICS = {'ece': ExpectedCalibrationError, 'mce': MaximumCalibrationError,
                       'nll': NegativeLogLikelihood, 'brier': BrierScore}
LOWER_IS_BETTER = ('hd95', 'assd', 'ece', 'mce', 'nll', 'brier')
_SURFACE_ACC = weakref.WeakKeyDictionary()     # config object -> the accumulator its surface metrics share
_LESION_ACC = weakref.WeakKeyDictionary()      # config object -> the accumulator its lesion metrics share
_CALIBRATION_ACC = weakref.WeakKeyDictionary()     # config object -> the accumulator its calibration metrics share


def _lesion_metric(config, metric_name, nc, group):
    try:
        acc, store = _LESION_ACC.get(config), _LESION_ACC.__setitem__
    except TypeError:      # a config object that cannot be weakly referenced keeps it itself
        acc, store = getattr(config, '_lesion_accumulator', None), \
            lambda c, a: setattr(c, '_lesion_accumulator', a)
    ov = float(getattr(config, 'lesion_min_overlap', 0.0))
    conn = int(getattr(config, 'cc_connectivity', 8))
    if acc is None or acc.num_classes != nc or acc.ignore_index != config.ignore_index \
            or acc.min_overlap != ov or acc.connectivity != conn:
        acc = LesionAccumulator(nc, config.ignore_index, ov, conn)
        store(config, acc)
    return LESION_METRICS[metric_name](num_classes=nc, group=group, accumulator=acc)


def _calibration_metric(config, metric_name, nc, group):
    try:
        acc, store = _CALIBRATION_ACC.get(config), _CALIBRATION_ACC.__setitem__
    except TypeError:      # a config object that cannot be weakly referenced keeps it itself
        acc, store = getattr(config, '_calibration_accumulator', None), \
            lambda c, a: setattr(c, '_calibration_accumulator', a)
    bins = int(getattr(config, 'calibration_bins', 15))
    if acc is None or acc.num_classes != nc or acc.ignore_index != config.ignore_index or acc.bins != bins:
        acc = CalibrationAccumulator(nc, config.ignore_index, bins)
        store(config, acc)
    return CALIBRATION_METRICS[metric_name](num_classes=nc, group=group, accumulator=acc)


def get_seg_metrics(config, metric_name):
    nc = max(config.num_class, 2)          # num_class == 1 (sigmoid) is scored as background/foreground
    group = getattr(config, 'dist_group', None)
    if metric_name in CALIBRATION_METRICS:
        return _calibration_metric(config, metric_name, nc, group)
    if metric_name in LESION_METRICS:
        return _lesion_metric(config, metric_name, nc, group)
    if metric_name in SURFACE_METRICS:
        # one accumulator per config: the metrics requested together share a batch's statistics
        try:
            acc, store = _SURFACE_ACC.get(config), _SURFACE_ACC.__setitem__
        except TypeError:      # a config object that cannot be weakly referenced keeps it itself
            acc, store = getattr(config, '_surface_accumulator', None), \
                lambda c, a: setattr(c, '_surface_accumulator', a)
        tol = float(getattr(config, 'nsd_tolerance', 2.0))
        if acc is None or acc.num_classes != nc or acc.ignore_index != config.ignore_index \
                or acc.nsd_tolerance != tol:
            acc = SurfaceAccumulator(nc, config.ignore_index, tol)
            store(config, acc)
        return SURFACE_METRICS[metric_name](num_classes=nc, group=group, accumulator=acc)
    if metric_name == 'iou':
        m = JaccardIndex(task='multiclass', num_classes=nc, ignore_index=config.ignore_index, average='none')
    elif metric_name == 'dice':
        m = Dice(num_classes=nc, average='macro')
    else:
        raise ValueError(f'Unsupported metric: {metric_name}.\n')
    m.group = group
    return m

