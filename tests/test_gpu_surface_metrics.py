"""Boundary metrics on the MI355X kernels (``csrc/surface.hip``) against the plain-torch specification on the CPU:
the distance transform and the boundary bitwise, every count and order statistic exactly, the fp values within
the rounding of one square root per distance and the final fp32 cast."""
import functools
import math
import os

import pytest
import torch

from medical_segmentation_pytorch_amd.ops import surface as S
from medical_segmentation_pytorch_amd.utils import metrics as M

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 7, 9), (2, 2, 33, 70), (2, 3, 64, 64), (1, 5, 20, 24), (1, 2, 5, 1100), (1, 2, 300, 3),
          (2, 2, 1, 40)]
IGNORE = 255
TOL = 2.0


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(logits [N, C, H, W], target [N, H, W]) on the CPU.  Label maps first -- two offset ellipses per class plus
    2 % salt noise, a column of frame pixels, an empty prediction (image 1), both empty (image 2), two ignored
    rows (columns when H < 5), one label == C and one == -1 -- then logits with an unambiguous argmax."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    pred = torch.zeros(n, h, w, dtype=torch.long)
    tgt = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        for k in range(1, c):
            cy, cx = (h - 1) * (0.25 + 0.5 * ((k + i) % 2)), w * k / c
            ry, rx = max(h * 0.22, 0.6), max(w * 0.5 / c, 0.6)
            dy, dx = min(2.0, h * 0.1), min(3.0, w * 0.1)
            tgt[i][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1] = k
            pred[i][((ys - cy - dy) / ry) ** 2 + ((xs - cx - dx) / (rx * 1.1)) ** 2 <= 1] = k
        for lab in (pred, tgt):
            salt = torch.rand(h, w, generator=g) < 0.02
            lab[i][salt] = torch.randint(0, c, (int(salt.sum()),), generator=g)
    tgt[0, :, 0] = 1                                   # a column of frame pixels
    if n > 1:
        pred[1] = 0                                    # empty prediction
    if n > 2:
        pred[2], tgt[2] = 0, 0                         # both empty
    if h >= 5:
        tgt[0, h // 2:h // 2 + 2, :] = IGNORE
    else:
        tgt[0, :, w // 2:w // 2 + 2] = IGNORE
    tgt[0, h - 1, w - 1] = c
    tgt[0, 0, max(w - 2, 0)] = -1
    noise = (torch.rand(n, c, h, w, generator=g) - 0.5)
    logits = 4.0 * torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).float() + noise
    top = logits.topk(2, dim=1).values
    assert (top[:, 0] - top[:, 1]).min() > 1e-3        # no ties
    return logits.contiguous(), tgt


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    logits, tgt = _case(shape)
    st = S.new_state(shape[1])
    dbg = S.surface_stats(logits, tgt, shape[1], IGNORE, TOL, st, debug=True, native=False)
    return st, dbg


def _device_run(shape, gpu):
    logits, tgt = _case(shape)
    st = S.new_state(shape[1], gpu)
    dbg = S.surface_stats(logits.to(gpu), tgt.to(gpu), shape[1], IGNORE, TOL, st, debug=True)
    return st, dbg


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_edt_and_boundary_bitwise(gpu, shape):
    logits, tgt = _case(shape)
    n, c, h, w = shape
    corners = torch.zeros(4, h, w, dtype=torch.bool)
    corners[0, 0, 0] = corners[1, 0, -1] = corners[2, -1, 0] = corners[3, -1, -1] = True
    masks = torch.cat([tgt == 1, logits.argmax(1) == 1, torch.zeros(1, h, w, dtype=torch.bool), corners,
                       torch.ones(1, h, w, dtype=torch.bool)])
    b_ref, e_ref = S.mask_boundary(masks), S.edt_sq(masks)
    b, e = S.mask_boundary(masks.to(gpu)), S.edt_sq(masks.to(gpu))
    assert b.is_cuda and b.dtype == torch.bool and e.dtype == torch.int32
    assert torch.equal(b.cpu(), b_ref)
    assert torch.equal(e.cpu(), e_ref)
    assert (e.cpu()[2 * n] == S.EDT_NONE).all()                        # the all-zero mask
    assert int(e.cpu()[2 * n + 1].max()) == (h - 1) ** 2 + (w - 1) ** 2    # one pixel in a corner
    # non-bool input and leading dimensions
    e5 = S.edt_sq(masks.to(gpu).float().view(1, -1, 1, h, w))
    assert e5.shape == (1, masks.shape[0], 1, h, w) and torch.equal(e5.flatten(0, 2), e)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_counts_and_order_statistics_exact(gpu, shape):
    _, ref = _oracle(shape)
    _, got = _device_run(shape, gpu)
    for key in ('counts', 'within', 'order'):
        assert torch.equal(got[key].cpu(), ref[key]), key
    assert int(ref['counts'].sum()) > 0


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_values_against_fp64_oracle(gpu, shape):
    n, c, h, w = shape
    ref_state, ref = _oracle(shape)
    logits, tgt = _case(shape)
    acc = M.SurfaceAccumulator(c, IGNORE, TOL).to(gpu)
    ms = [cls(num_classes=c, accumulator=acc) for cls in M.SURFACE_METRICS.values()]
    lg, tg = logits.to(gpu), tgt.to(gpu)
    for m in ms:
        m.update(lg, tg)
    assert torch.equal(acc.count.cpu(), ref_state['count']) and torch.equal(acc.onesided.cpu(), ref_state['onesided'])
    per = ref['per_image']                               # [N, K, 3] fp64, nan = not scored
    scored = ~per[..., 0].isnan()
    for j, (name, m) in enumerate(zip(M.SURFACE_METRICS, ms)):
        want_pc = torch.where(scored, per[..., j], torch.zeros_like(per[..., j])).sum(0) / scored.sum(0)
        got_pc, got = m.per_class().cpu().double(), float(m.compute())
        assert got_pc.dtype == torch.float64 and m.compute().dtype == torch.float32 and m.compute().dim() == 0
        have = scored.any(0)
        assert torch.equal(got_pc.isnan(), ~have)
        want = float(want_pc[have].mean()) if have.any() else float('nan')
        err_pc = (got_pc[have] - want_pc[have]).abs()
        print(f'{shape} {name}: compute {got!r} oracle {want!r}; per-class max abs err '
              f'{float(err_pc.max()) if have.any() else 0.0:.3e}')
        if name == 'nsd':
            assert (err_pc <= 1e-6).all() and abs(got - want) <= 1e-6
        else:
            assert (err_pc <= 1e-5 * want_pc[have].abs()).all() and abs(got - want) <= 1e-5 * abs(want)
    if n > 1:
        assert int(ref_state['onesided'].sum()) > 0
    if n > 2:
        assert int(ref_state['count'].max()) < n          # the pair with both masks empty is not scored


def test_repeatable_rescratch_and_confmat_untouched(gpu):
    a, b = SHAPES[2], SHAPES[1]
    runs = [_device_run(a, gpu) for _ in range(2)]
    other = _device_run(b, gpu)                           # another shape: the scratch is re-sized
    again = _device_run(a, gpu)
    for st, dbg in (runs[1], again):
        for k in ('sum', 'count', 'onesided'):
            assert torch.equal(st[k], runs[0][0][k]), k   # bitwise, fp64 sums included
        assert torch.equal(dbg['per_image'].nan_to_num(-1.0), runs[0][1]['per_image'].nan_to_num(-1.0))
    assert torch.equal(other[1]['counts'].cpu(), _oracle(b)[1]['counts'])
    # Dice on the same tensors, with and without the surface metrics in between
    logits, tgt = (t.to(gpu) for t in _case(a))
    plain = M.Dice(num_classes=a[1]).to(gpu)
    plain.update(logits, tgt)
    plain.update(logits, tgt)
    mixed = M.Dice(num_classes=a[1]).to(gpu)
    surf = M.SurfaceDice(num_classes=a[1], ignore_index=IGNORE).to(gpu)
    keep = (logits.clone(), tgt.clone())
    mixed.update(logits, tgt)
    surf.update(logits, tgt)
    mixed.update(logits, tgt)
    assert torch.equal(mixed.confmat, plain.confmat)
    assert torch.equal(logits, keep[0]) and torch.equal(tgt, keep[1])


def test_trainer_validate_with_surface_metrics(gpu, tmp_path):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.utils import get_seg_metrics
    names = ['dice', 'iou', 'hd95', 'assd', 'nsd']
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 6, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 4, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 1, 0, False, False
    c.engine, c.metrics = 'fused', list(names)
    c.init_dependent_config()
    t = SegTrainer(c)
    assert t.fused and t.metrics[2].acc is t.metrics[3].acc is t.metrics[4].acc
    seen, calls = [], []
    acc = t.metrics[2].acc
    upd = acc.update
    acc.update = lambda p, m, **k: (seen.append((p.detach().cpu().clone(), m.cpu().clone())), upd(p, m, **k))[1]
    real = S.surface_stats
    S.surface_stats = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        t.validate(c, t.val_loader)
    finally:
        S.surface_stats = real
    full = {k: v.clone() for k, v in t.last_scores.items()}
    assert len(calls) == 2 and len(seen) == 6             # 2 batches (4 + 2 images) x 3 metrics: the kernels ran once per batch
    assert set(names) <= set(t.val_history[-1])
    t.metrics = [get_seg_metrics(c, m).to(t.device) for m in names[:2]]
    c.metrics = names[:2]
    t.validate(c, t.val_loader)
    assert torch.equal(t.last_scores['dice'], full['dice']) and torch.equal(t.last_scores['iou'], full['iou'])
    # the oracle on the concatenated predictions
    logits = torch.cat([p for p, _ in seen[::3]])
    masks = torch.cat([m for _, m in seen[::3]])
    assert logits.shape == (6, 2, 64, 64)
    st = S.new_state(2)
    S.surface_stats(logits, masks, 2, c.ignore_index, c.nsd_tolerance, st, native=False)
    assert int(st['count'][0]) > 0
    want = (st['sum'][:, 0] / st['count'][0]).tolist()
    for name, w in zip(names[2:], want):
        got = float(full[name])
        print(f'trainer {name}: {got!r} oracle {w!r}')
        assert abs(got - w) <= (1e-6 if name == 'nsd' else 1e-5 * abs(w))
    assert os.path.isdir(c.save_dir) and not math.isnan(float(full['dice']))
