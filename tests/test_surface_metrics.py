"""Boundary metrics (HD95 / ASSD / NSD), CPU tier: the plain-torch specification in ``ops/surface.py`` against
scipy and hand-computed values, the metric objects' state handling, config / trainer wiring and the gloo sync."""
import json
import math
import os
import sys

import pytest
import torch

from medical_segmentation_pytorch_amd.ops import surface as S
from medical_segmentation_pytorch_amd.utils import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logits(pred_labels, num_classes):
    """[N, H, W] labels -> [N, C, H, W] logits whose argmax is the label (margin 1)."""
    return torch.nn.functional.one_hot(pred_labels, num_classes).permute(0, 3, 1, 2).float().contiguous()


def _stats(pred, tgt, num_classes=2, ignore_index=None, tol=2.0):
    st = S.new_state(num_classes)
    dbg = S.surface_stats(_logits(pred, num_classes), tgt, num_classes, ignore_index, tol, st, debug=True)
    return st, dbg


def _blobs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    h, w = shape
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    m = ((ys - h * 0.45) / max(h * 0.3, 1)) ** 2 + ((xs - w * 0.55) / max(w * 0.25, 1)) ** 2 <= 1
    return m ^ (torch.rand(h, w, generator=g) < 0.05)


HAND_SHAPES = [(7, 9), (33, 70), (1, 40), (40, 1)]


@pytest.mark.parametrize('shape', HAND_SHAPES)
def test_boundary_and_edt_match_scipy(shape):
    ndi = pytest.importorskip('scipy.ndimage')
    import numpy as np
    h, w = shape
    cases = [_blobs(shape, s) for s in range(3)]
    full = torch.ones(h, w, dtype=torch.bool)
    corner = torch.zeros(h, w, dtype=torch.bool)
    corner[0, 0] = corner[-1, -1] = True
    frame = torch.zeros(h, w, dtype=torch.bool)
    frame[:, 0] = True
    cases += [full, corner, frame]
    m = torch.stack(cases)
    b, e = S.mask_boundary(m), S.edt_sq(m)
    assert b.dtype == torch.bool and e.dtype == torch.int32
    cross = ndi.generate_binary_structure(2, 1)
    for i, c in enumerate(cases):
        a = c.numpy()
        assert np.array_equal(b[i].numpy(), a ^ ndi.binary_erosion(a, cross)), i
        ref = np.rint(ndi.distance_transform_edt(~a) ** 2).astype(np.int64)
        assert np.array_equal(e[i].numpy().astype(np.int64), ref), i


def test_edt_of_empty_map_and_size_limit():
    e = S.edt_sq(torch.zeros(2, 5, 6))
    assert (e == S.EDT_NONE).all() and S.EDT_NONE == 2 ** 31 - 1
    with pytest.raises(ValueError):
        S.edt_sq(torch.zeros(1, 16385, dtype=torch.bool))


def test_full_image_and_frame_touching_boundary():
    b = S.mask_boundary(torch.ones(6, 8))
    ref = torch.zeros(6, 8, dtype=torch.bool)
    ref[0], ref[-1], ref[:, 0], ref[:, -1] = True, True, True, True
    assert torch.equal(b, ref)                      # full image: the frame only
    m = torch.zeros(6, 8)
    m[0:3, 0:4] = 1                                 # touches the top and left frame
    ref = m.bool().clone()
    ref[1, 1:3] = False                             # interior: all four neighbours inside
    assert torch.equal(S.mask_boundary(m), ref)


def test_single_pixels():
    pred = torch.zeros(1, 10, 12, dtype=torch.long)
    tgt = torch.zeros(1, 10, 12, dtype=torch.long)
    pred[0, 2, 3], tgt[0, 5, 7] = 1, 1               # offset (3, 4): distance 5
    for tol, nsd in ((2.0, 0.0), (5.0, 1.0)):
        st, dbg = _stats(pred, tgt, tol=tol)
        assert dbg['per_image'][0, 0].tolist() == [5.0, 5.0, nsd]
        assert dbg['order'].flatten().tolist() == [25] * 4 and dbg['counts'].flatten().tolist() == [1, 1]
        assert st['count'].tolist() == [1] and st['onesided'].tolist() == [0]


def test_offset_rectangles():
    """Two 6 x 8 rectangles offset by (3, 4): each boundary has 24 pixels, values worked out by hand from the
    geometry (pixels inside the overlap reach the other contour at the other rectangle's nearest edge)."""
    pred = torch.zeros(1, 24, 24, dtype=torch.long)
    tgt = torch.zeros(1, 24, 24, dtype=torch.long)
    pred[0, 4:10, 4:12] = 1
    tgt[0, 7:13, 8:16] = 1
    st, dbg = _stats(pred, tgt, tol=2.0)
    bp = S.mask_boundary(pred[0] == 1).nonzero().tolist()
    bg = S.mask_boundary(tgt[0] == 1).nonzero().tolist()
    assert len(bp) == len(bg) == 24

    def direct(a, b):
        return sorted(min((y - v) ** 2 + (x - u) ** 2 for v, u in b) for y, x in a)
    dpg, dgp = direct(bp, bg), direct(bg, bp)
    assert dpg == dgp                               # the configuration is point-symmetric
    assert dpg[-1] == 25 and dpg[0] == 0            # far corner is (3, 4) away; the contours cross
    pos = 0.95 * 23
    lo, hi = math.floor(pos), math.ceil(pos)
    q = math.sqrt(dpg[lo]) + (pos - lo) * (math.sqrt(dpg[hi]) - math.sqrt(dpg[lo]))
    hd, assd, nsd = dbg['per_image'][0, 0].tolist()
    assert abs(hd - q) < 1e-12
    assert abs(assd - sum(math.sqrt(v) for v in dpg) / 24) < 1e-12
    assert abs(nsd - sum(v <= 4 for v in dpg) / 24) < 1e-15
    assert dbg['order'][0, 0, 0].tolist() == [dpg[lo], dpg[hi]]
    assert dbg['within'].flatten().tolist() == [sum(v <= 4 for v in dpg)] * 2


def test_identical_masks():
    lab = _blobs((20, 31), 1).long()[None]
    st, dbg = _stats(lab, lab)
    assert dbg['per_image'][0, 0].tolist() == [0.0, 0.0, 1.0]


def test_empty_rules():
    h, w = 9, 12
    empty = torch.zeros(1, h, w, dtype=torch.long)
    some = empty.clone()
    some[0, 2:5, 3:7] = 1
    for name, cls in M.SURFACE_METRICS.items():
        m = cls(num_classes=2)
        m.update(_logits(empty, 2), empty)
        assert math.isnan(float(m.compute())) and m.compute().dtype == torch.float32 and m.compute().dim() == 0
        assert m.acc.count.tolist() == [0] and torch.isnan(m.per_class()).all()
        m.update(_logits(empty, 2), some)           # empty prediction
        m.update(_logits(some, 2), empty)           # empty ground truth
        want = 0.0 if name == 'nsd' else math.sqrt(h * h + w * w)
        assert abs(float(m.compute()) - want) <= 1e-6 * max(want, 1)
        assert m.acc.count.tolist() == [2] and m.acc.onesided.tolist() == [2]
        assert m.last_one_sided.tolist() == [2] and m.one_sided().tolist() == [2]


def test_ignored_and_out_of_range_labels_leave_both_masks():
    pred = torch.zeros(1, 12, 14, dtype=torch.long)
    tgt = torch.zeros(1, 12, 14, dtype=torch.long)
    pred[0, 2:9, 2:10] = 1
    tgt[0, 3:10, 4:12] = 1
    holes = tgt.clone()
    holes[0, 5] = 255                               # ignored row
    holes[0, 7, 6] = 2                              # == C
    holes[0, 8, 7] = -1
    gone = (holes[0] == 255) | (holes[0] == 2) | (holes[0] == -1)
    st, dbg = _stats(pred, holes, ignore_index=255)
    # the same as scoring masks with those pixels cut out of both (label 0 there is not scored either, but the
    # cut pixels must not count as mask pixels of class 1 on either side)
    p2, t2 = pred.clone(), tgt.clone()
    p2[0][gone], t2[0][gone] = 0, 0
    st2, dbg2 = _stats(p2, t2)
    assert torch.equal(dbg['counts'], dbg2['counts']) and torch.equal(dbg['per_image'], dbg2['per_image'])
    assert int(dbg['counts'][0, 0, 0]) != int(S.mask_boundary(pred[0] == 1).sum())


def _batch(n=4, c=3, h=18, w=22, seed=0):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.zeros(n, h, w, dtype=torch.long)
    pred = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        for k in range(1, c):
            y0, x0 = int(torch.randint(0, h - 6, (1,), generator=g)), int(torch.randint(0, w - 6, (1,), generator=g))
            tgt[i, y0:y0 + 5, x0:x0 + 6] = k
            pred[i, y0 + 1:y0 + 6, x0:x0 + 5] = k
    pred[0] = 0                                     # one empty prediction
    return _logits(pred, c), tgt


def test_additivity_reset_and_shared_accumulation(monkeypatch):
    from types import SimpleNamespace
    logits, tgt = _batch()
    cfg = SimpleNamespace(num_class=3, ignore_index=255, nsd_tolerance=2.0)
    ms = [M.get_seg_metrics(cfg, n) for n in ('hd95', 'assd', 'nsd')]
    assert [type(m) for m in ms] == [M.HausdorffDistance95, M.AverageSurfaceDistance, M.SurfaceDice]
    assert ms[0].acc is ms[1].acc is ms[2].acc
    calls = []
    real = S.surface_stats
    monkeypatch.setattr(S, 'surface_stats', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for m in ms:                                    # the trainer's loop: a fresh detach() view per metric
        m.update(logits.detach().float(), tgt)
    assert len(calls) == 1
    ms[0].update(logits, tgt)                       # the same metric again: a new batch, scored again
    assert len(calls) == 2 and ms[0].acc.count.tolist() == [8, 8]
    ms[2].reset()
    for m in ms:
        m.update(logits, tgt)
    assert len(calls) == 3
    full = [m.compute() for m in ms]
    per = [m.per_class() for m in ms]
    assert all(p.shape == (2,) and p.dtype == torch.float32 for p in per)
    for m, p in zip(ms, per):
        assert abs(float(m.compute()) - float(p.mean())) < 1e-6
    ms[1].reset()                                   # one reset clears the shared state
    assert ms[0].acc.count.sum() == 0 and math.isnan(float(ms[2].compute()))
    for half in (slice(0, 2), slice(2, 4)):
        for m in ms:
            m.update(logits[half].contiguous(), tgt[half].contiguous())
    assert len(calls) == 5
    for a, m in zip(full, ms):
        assert abs(float(a) - float(m.compute())) <= 1e-6 * abs(float(a))
    assert ms[0].acc.onesided.tolist() == [1, 1]
    # num_class == 1 (sigmoid head) is scored as two classes
    one = M.get_seg_metrics(SimpleNamespace(num_class=1, ignore_index=255), 'nsd')
    assert one.num_classes == 2 and one.acc.sum.shape == (3, 1)
    with pytest.raises(ValueError):
        M.get_seg_metrics(cfg, 'hausdorff')


def test_config_and_parser():
    from medical_segmentation_pytorch_amd.configs import MyConfig, load_parser
    c = MyConfig()
    assert c.nsd_tolerance == 2.0
    for first in ('hd95', 'assd'):
        c = MyConfig()
        c.metrics = [first, 'dice']
        with pytest.raises(ValueError):
            c.init_dependent_config()
    c = MyConfig()
    c.metrics = ['nsd', 'hd95', 'assd']
    c.init_dependent_config()
    c = load_parser(MyConfig(), ['--metrics', 'dice', 'iou', 'hd95', 'assd', 'nsd', '--nsd_tolerance', '3.5'])
    assert c.metrics == ['dice', 'iou', 'hd95', 'assd', 'nsd'] and c.nsd_tolerance == 3.5


def _train_cfg(tmp, metrics):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    c = MyConfig()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp / 'data'), str(tmp / ('save_' + '_'.join(metrics)))
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 4, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 2, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 2, 1, False, False
    c.metrics = list(metrics)
    c.random_seed = 1
    c.init_dependent_config()
    c.DDP, c.gpu_num, c.num_workers = False, 1, 0
    return c


def test_trainer_writes_surface_metrics(tmp_path):
    """Two CPU epochs with ['dice', 'hd95', 'nsd']: strict-JSON history with the new keys, and the best
    checkpoint is still chosen by metrics[0] alone -- the validation with the highest Dice -- and scores the
    same Dice under a ['dice'] trainer (two training runs are not comparable bit for bit on the CPU engine, so
    the selection is checked on this run's own records and checkpoint)."""
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = _train_cfg(tmp_path, ['dice', 'hd95', 'nsd'])
    SegTrainer(c).run(c)
    text = open(os.path.join(c.save_dir, 'val_history.json')).read()

    def strict(name):
        raise AssertionError(f'{name} in val_history.json')
    h = json.loads(text, parse_constant=strict)
    rows = [r for r in h['history'] if not r['val_best']]
    final = [r for r in h['history'] if r['val_best']]
    assert len(rows) == 2 and len(final) == 1
    for r in h['history']:
        assert r['score'] == r['dice']
        assert r['hd95'] is None or 0 <= r['hd95'] <= math.sqrt(2) * 64
        assert r['nsd'] is None or 0 <= r['nsd'] <= 1
    best_row = max(rows, key=lambda r: r['dice'])
    best = torch.load(os.path.join(c.save_dir, 'best.pth'), weights_only=True)
    assert best['cur_epoch'] == best_row['epoch']
    assert final[0]['dice'] == best_row['dice'] == h['best_score']
    c2 = _train_cfg(tmp_path, ['dice'])
    t2 = SegTrainer(c2)
    score = t2.val_best(c2, t2.val_loader, ckpt_path=os.path.join(c.save_dir, 'best.pth'))
    assert float(score) == best_row['dice']
    assert 'hd95' not in t2.val_history[-1]


def test_accuracy_summary_carries_surface_keys(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import accuracy_main
    finally:
        sys.path.pop(0)
    row = {'epoch': 0, 'train_itrs': 2, 'elapsed_s': 1.0, 'score': 0.9, 'val_best': False, 'fp32': False,
           'dice': 0.9, 'iou': [0.9, 0.8], 'hd95': 3.25, 'nsd': None}
    h = {'best_score': 0.9, 'wall_s': 2.0, 'iters_per_epoch': 2, 'train_bs': 4,
         'history': [row, dict(row, val_best=True)]}
    p = tmp_path / 'val_history.json'
    p.write_text(json.dumps(h))
    out = accuracy_main.summarise(str(p), 0.98)
    assert out['best']['hd95'] == 3.25 and out['best']['nsd'] is None and 'assd' not in out['best']
    assert out['val_best']['hd95'] == 3.25 and out['history'][0]['hd95'] == 3.25


_WORKER = '''
import json, os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, {root!r})
from medical_segmentation_pytorch_amd.utils import metrics as M
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo', rank=rank, world_size=world)
data = torch.load({data!r})
acc = M.SurfaceAccumulator(3, 255, 2.0)
ms = [cls(num_classes=3, accumulator=acc) for cls in M.SURFACE_METRICS.values()]
logits, target = data['logits'][rank::world].contiguous(), data['target'][rank::world].contiguous()
for m in ms:
    m.update(logits, target)
out = {{'compute': [float(m.compute()) for m in ms], 'per_class': [m.per_class().tolist() for m in ms],
       'one_sided': ms[0].last_one_sided.tolist()}}
json.dump(out, open(os.path.join({out!r}, f'rank{{rank}}.json'), 'w'))
dist.destroy_process_group()
'''


def test_sharded_compute_equals_single_process(tmp_path):
    from medical_segmentation_pytorch_amd.utils.launch import spawn_ranks
    logits, tgt = _batch(n=4, seed=3)
    torch.save({'logits': logits, 'target': tgt}, tmp_path / 'data.pt')
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER.format(root=ROOT, data=str(tmp_path / 'data.pt'), out=str(tmp_path)))
    assert spawn_ranks(2, [str(script)]) == 0
    acc = M.SurfaceAccumulator(3, 255, 2.0)
    ms = [cls(num_classes=3, accumulator=acc) for cls in M.SURFACE_METRICS.values()]
    for m in ms:
        m.update(logits, tgt)
    for r in range(2):
        got = json.load(open(tmp_path / f'rank{r}.json'))
        for i, m in enumerate(ms):
            assert abs(got['compute'][i] - float(m.compute())) <= 1e-6 * max(1.0, abs(float(m.compute())))
            assert torch.allclose(torch.tensor(got['per_class'][i]), m.per_class(), rtol=1e-6, atol=1e-7)
        assert got['one_sided'] == acc.onesided.tolist() == [1, 1]
