"""Connected components on the CPU: the plain-torch specification of ``ops/components.py`` against scipy, hand
cases for every clean-up rule and for the lesion-wise counts, the metric objects, and the configuration /
``predict`` wiring."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from medical_segmentation_pytorch_amd.ops import components as CC
from medical_segmentation_pytorch_amd.utils import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITIES = (0.3, 0.5, 0.62, 0.8)       # either side of the site-percolation thresholds (0.593 at 4, 0.407 at 8)
SHAPES = [(1, 1), (1, 7), (6, 1), (2, 2), (5, 9), (13, 8), (24, 24)]


def _random_masks(shape, seed=0, per_density=3):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(per_density, *shape, generator=g) < d for d in DENSITIES])


def _structure(connectivity):
    ndimage = pytest.importorskip('scipy.ndimage')
    return ndimage, (ndimage.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), bool))


# ---- specification against scipy ------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_label_and_areas_equal_scipy(shape, connectivity):
    ndimage, st = _structure(connectivity)
    masks = _random_masks(shape, seed=31 * shape[0] + shape[1])
    labels, num = CC.label(masks, connectivity)
    areas = CC.component_areas(masks, connectivity)
    assert labels.dtype == torch.int32 and num.dtype == torch.long and areas.dtype == torch.int32
    assert labels.shape == masks.shape and num.shape == masks.shape[:1]
    for i in range(masks.shape[0]):
        ref, k = ndimage.label(masks[i].numpy(), st)
        assert int(num[i]) == k
        assert np.array_equal(labels[i].numpy(), ref)
        count = np.bincount(ref.ravel(), minlength=k + 1)
        count[0] = 0
        assert np.array_equal(areas[i].numpy(), count[ref])


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_binary_fill_holes_equals_scipy(shape):
    ndimage, _ = _structure(4)
    masks = _random_masks(shape, seed=7 + shape[0] * shape[1])
    out = CC.postprocess(masks.long(), 2, fill_holes=True)
    assert out.dtype == torch.uint8 and out.shape == masks.shape
    for i in range(masks.shape[0]):
        assert np.array_equal(out[i].numpy().astype(bool), ndimage.binary_fill_holes(masks[i].numpy()))


def test_serpentine_converges_in_few_rounds():
    h = w = 33
    lab = torch.full((1, h, w), CC.SKIP, dtype=torch.uint8)
    lab[0, ::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        lab[0, y, w - 1 if k % 2 == 0 else 0] = 1
    root, rounds = CC._roots_torch(lab, 4)
    assert rounds <= 64 and set(root.unique().tolist()) == {-1, 0}
    assert CC.label(lab == 1, 4)[1].tolist() == [1]


# ---- hand cases ---------------------------------------------------------------------------------------------------
def test_diagonal_pair_and_leading_dimensions():
    m = torch.zeros(4, 5)
    m[1, 1] = m[2, 2] = 3.5                          # non-bool input: nonzero means set
    l8, n8 = CC.label(m, 8)
    l4, n4 = CC.label(m, 4)
    assert n8.shape == () and int(n8) == 1 and int(n4) == 2
    assert l8[1, 1] == l8[2, 2] == 1 and l4[1, 1] == 1 and l4[2, 2] == 2
    l5, n5 = CC.label(m.view(1, 1, 4, 5).expand(2, 3, 4, 5), 4)
    assert l5.shape == (2, 3, 4, 5) and n5.shape == (2, 3) and torch.equal(l5[1, 2], l4) and (n5 == 2).all()
    assert CC.component_areas(m, 8).tolist()[1][1] == 2 and CC.component_areas(m, 4).max() == 1
    with pytest.raises(ValueError):
        CC.label(m, 6)


def _ring_map():
    lab = torch.zeros(1, 9, 10, dtype=torch.long)
    lab[0, 1:8, 1:8] = 1
    lab[0, 2:7, 2:7] = 0                             # the hole of the ring
    lab[0, 4, 4] = 2                                 # an island of another class inside it
    return lab


def test_ring_with_island_of_another_class():
    out = CC.postprocess(_ring_map(), 3, fill_holes=True)
    want = torch.zeros(1, 9, 10, dtype=torch.uint8)
    want[0, 1:8, 1:8] = 1
    want[0, 4, 4] = 2
    assert torch.equal(out, want)


def test_hole_touching_the_frame_is_not_filled():
    lab = torch.zeros(1, 6, 7, dtype=torch.long)
    lab[0, 0:5, 1:6] = 1
    lab[0, 0:3, 3] = 0                               # a notch open at the top row
    assert torch.equal(CC.postprocess(lab, 2, fill_holes=True), lab.to(torch.uint8))
    lab[0, 0, 3] = 1                                 # closed: now it is a hole
    filled = CC.postprocess(lab, 2, fill_holes=True)
    assert filled[0, 1, 3] == 1 and filled[0, 2, 3] == 1 and int(filled.sum()) == int(lab.sum()) + 2


def test_keep_largest_tie_goes_to_the_raster_first():
    lab = torch.zeros(1, 8, 12, dtype=torch.long)
    lab[0, 5:7, 1:4] = 1                             # area 6, later in raster order
    lab[0, 1:4, 7:9] = 1                             # area 6, first
    lab[0, 6, 9:11] = 2
    lab[0, 1, 1] = 2                                 # class 2: area 1 first, area 2 later -> the larger wins
    out = CC.postprocess(lab, 3, keep_largest=True)
    want = torch.zeros_like(lab)
    want[0, 1:4, 7:9] = 1
    want[0, 6, 9:11] = 2
    assert torch.equal(out, want.to(torch.uint8))


def test_rule_order_speck_inside_a_hole():
    lab = torch.zeros(1, 9, 9, dtype=torch.long)
    lab[0, 1:8, 1:8] = 1
    lab[0, 2:7, 2:7] = 0
    lab[0, 4, 4] = 1                                 # a speck of the SAME class inside the hole
    solid = torch.zeros(1, 9, 9, dtype=torch.uint8)
    solid[0, 1:8, 1:8] = 1
    for min_area in (0, 1, 2, 40):
        assert torch.equal(CC.postprocess(lab, 2, fill_holes=True, min_area=min_area), solid)
    no_fill = CC.postprocess(lab, 2, min_area=2)     # without the fill the speck is a component of area 1
    assert no_fill[0, 4, 4] == 0 and int(no_fill.sum()) == 24


def test_min_area_is_strict_and_per_class():
    lab = torch.zeros(2, 6, 9, dtype=torch.long)
    lab[0, 0, 0:3] = 1                               # area 3
    lab[0, 2, 0:4] = 1                               # area 4
    lab[0, 4, 0:2] = 2
    lab[0, 4, 2:4] = 1                               # touching pixels of two classes do not add up
    lab[1, 1, 1], lab[1, 2, 2] = 1, 1                # diagonal pair: area 2 at connectivity 8, two of area 1 at 4
    out = CC.postprocess(lab, 3, min_area=4)
    assert int(out[0].sum()) == 4 and (out[0, 2, 0:4] == 1).all()
    out3 = CC.postprocess(lab, 3, min_area=3)
    assert (out3[0, 0, 0:3] == 1).all() and int((out3[0] == 2).sum()) == 0
    assert int(CC.postprocess(lab, 3, min_area=2, connectivity=8)[1].sum()) == 2
    assert int(CC.postprocess(lab, 3, min_area=2, connectivity=4)[1].sum()) == 0


def test_all_options_off_returns_the_same_tensor():
    lab = _ring_map()
    assert CC.postprocess(lab, 3) is lab
    with pytest.raises(ValueError):
        CC.postprocess(lab, 3, min_area=-1)
    with pytest.raises(ValueError):
        CC.postprocess(lab.float(), 3, fill_holes=True)
    with pytest.raises(ValueError):
        CC.postprocess(lab, 3, fill_holes=True, connectivity=6)
    # debug: the label range is checked and the (here always zero) error counter comes back
    same, errors = CC.postprocess(lab, 3, debug=True)
    assert same is lab and errors.dtype == torch.int32 and errors.tolist() == [0]
    out, errors = CC.postprocess(lab, 3, fill_holes=True, debug=True)
    assert torch.equal(out, CC.postprocess(lab, 3, fill_holes=True)) and errors.tolist() == [0]
    with pytest.raises(ValueError):
        CC.postprocess(lab, 2, fill_holes=True, debug=True)          # the map holds class 2


# ---- lesion_stats ---------------------------------------------------------------------------------------------------
def _logits(lab, c):
    return 4.0 * torch.nn.functional.one_hot(lab.clamp(0, c - 1), c).permute(0, 3, 1, 2).float()


def _stats(pred, tgt, c=2, **kw):
    st = CC.new_state(c)
    dbg = CC.lesion_stats(_logits(pred, c), tgt, c, state=st, debug=True, **kw)
    assert int(st['err']) == 0 and torch.equal(dbg['per_image'].sum(0).t(), st['counts'])
    return st['counts'], dbg['per_image']


def _found_missed_false_alarm():
    tgt = torch.zeros(1, 12, 16, dtype=torch.long)
    pred = torch.zeros_like(tgt)
    tgt[0, 1:4, 1:4] = 1                             # found
    tgt[0, 8:10, 2:5] = 1                            # missed
    pred[0, 2:5, 2:5] = 1                            # overlaps the first
    pred[0, 6:8, 11:14] = 1                          # false alarm
    return pred, tgt


def test_two_lesions_one_found_one_false_alarm():
    counts, per = _stats(*_found_missed_false_alarm())
    assert counts[:, 0].tolist() == [2, 1, 2, 1] and per[0, 0].tolist() == [2, 1, 2, 1]


def test_bridging_blob():
    tgt = torch.zeros(1, 8, 14, dtype=torch.long)
    pred = torch.zeros_like(tgt)
    tgt[0, 2:5, 1:4] = 1
    tgt[0, 2:5, 8:11] = 1
    pred[0, 3, 2:10] = 1                             # one blob across both
    assert _stats(pred, tgt)[0][:, 0].tolist() == [2, 2, 1, 1]


def test_min_overlap_at_exactly_half():
    tgt = torch.zeros(1, 6, 10, dtype=torch.long)
    pred = torch.zeros_like(tgt)
    tgt[0, 1, 1:5] = 1                               # area 4
    pred[0, 1, 3:9] = 1                              # area 6, 2 shared: half of the target, a third of the blob
    assert _stats(pred, tgt, min_overlap=0.5)[0][:, 0].tolist() == [1, 1, 1, 0]
    assert _stats(pred, tgt, min_overlap=0.51)[0][:, 0].tolist() == [1, 0, 1, 0]
    assert _stats(pred, tgt, min_overlap=1 / 3)[0][:, 0].tolist() == [1, 1, 1, 1]
    assert _stats(pred, tgt)[0][:, 0].tolist() == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        _stats(pred, tgt, min_overlap=1.5)


def test_ignored_pixels_split_a_lesion_and_absent_class():
    tgt = torch.zeros(1, 9, 9, dtype=torch.long)
    tgt[0, 1:8, 3:6] = 1
    pred = tgt.clone()
    tgt[0, 4] = 255                                  # an ignored row cuts it, and the prediction, in two
    counts, _ = _stats(pred, tgt, c=3, ignore_index=255)
    assert counts[:, 0].tolist() == [2, 2, 2, 2]
    assert counts[:, 1].tolist() == [0, 0, 0, 0]     # class 2: absent on both sides
    whole, _ = _stats(pred, tgt.clamp_max(1), c=3)
    assert whole[:, 0].tolist() == [1, 1, 1, 1]
    acc = M.LesionAccumulator(3, 255)
    ms = {n: cls(num_classes=3, accumulator=acc) for n, cls in M.LESION_METRICS.items()}
    ms['lesion_f1'].update(_logits(pred, 3), tgt)
    for m in ms.values():
        assert m.per_class().tolist()[0] == 1.0 and math.isnan(m.per_class().tolist()[1])
        assert float(m.compute()) == 1.0             # the absent class is not scored


def test_metric_values_and_scoring_rules():
    c = 4
    tgt = torch.zeros(1, 12, 16, dtype=torch.long)
    pred = torch.zeros_like(tgt)
    p1, t1 = _found_missed_false_alarm()
    tgt[t1 == 1], pred[p1 == 1] = 1, 1               # class 1: recall 1/2, precision 1/2
    pred[0, 10:12, 8:10] = 2                         # class 2: predicted only -> precision 0, F1 0, no recall
    tgt[0, 0, 10:13] = 3                             # class 3: ground truth only -> recall 0, F1 0, no precision
    acc = M.LesionAccumulator(c, 255)
    rec, prec, f1 = (cls(num_classes=c, accumulator=acc) for cls in M.LESION_METRICS.values())
    logits = _logits(pred, c)
    for m in (rec, prec, f1):
        m.update(logits, tgt)
    assert rec.counts().tolist() == [[2, 0, 1], [1, 0, 0], [2, 1, 0], [1, 0, 0]]
    nan = float('nan')
    for m, want in ((rec, [0.5, nan, 0.0]), (prec, [0.5, 0.0, nan]), (f1, [0.5, 0.0, 0.0])):
        got = m.per_class()
        assert got.dtype == torch.float32 and torch.allclose(got, torch.tensor(want), equal_nan=True)
        have = [w for w in want if w == w]
        assert abs(float(m.compute()) - sum(have) / len(have)) < 1e-7
        assert m.compute().dtype == torch.float32 and m.compute().dim() == 0
    # a nonzero error counter turns every value into nan
    acc.err += 1
    assert all(math.isnan(float(m.compute())) for m in (rec, prec, f1)) and torch.isnan(f1.per_class()).all()


# ---- metric objects -----------------------------------------------------------------------------------------------
def test_shared_accumulator_reset_and_nan(monkeypatch):
    pred, tgt = _found_missed_false_alarm()
    logits = _logits(pred, 2)
    cfg = SimpleNamespace(num_class=2, ignore_index=255, lesion_min_overlap=0.0, cc_connectivity=8)
    names = ('lesion_recall', 'lesion_precision', 'lesion_f1')
    ms = [M.get_seg_metrics(cfg, n) for n in names]
    assert [type(m) for m in ms] == [M.LesionRecall, M.LesionPrecision, M.LesionF1]
    assert ms[0].acc is ms[1].acc is ms[2].acc
    calls = []
    real = CC.lesion_stats
    monkeypatch.setattr(CC, 'lesion_stats', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for m in ms:                                     # the trainer's loop: a fresh detach() view per metric
        m.update(logits.detach().float(), tgt)
    assert len(calls) == 1 and ms[0].acc.counts[:, 0].tolist() == [2, 1, 2, 1]
    ms[0].update(logits, tgt)                        # the same metric again: a new batch
    assert len(calls) == 2 and ms[0].acc.counts[:, 0].tolist() == [4, 2, 4, 2]
    assert [float(m.compute()) for m in ms] == [0.5, 0.5, 0.5]
    ms[2].reset()                                    # one reset clears the shared state
    assert int(ms[0].acc.counts.sum()) == 0
    for m in ms:
        assert math.isnan(float(m.compute())) and m.compute().dtype == torch.float32
    empty = torch.zeros_like(tgt)
    ms[1].update(_logits(empty, 2), empty)           # nothing on either side: still nothing scored
    assert len(calls) == 3 and all(math.isnan(float(m.compute())) for m in ms)
    # other settings of the same config object: a new accumulator
    cfg.cc_connectivity = 4
    assert M.get_seg_metrics(cfg, 'lesion_f1').acc is not ms[0].acc
    one = M.get_seg_metrics(SimpleNamespace(num_class=1, ignore_index=255), 'lesion_f1')
    assert one.num_classes == 2 and one.acc.counts.shape == (4, 1) and one.acc.connectivity == 8
    with pytest.raises(ValueError):
        M.LesionAccumulator(2, 255, min_overlap=1.5)
    with pytest.raises(ValueError):
        M.LesionAccumulator(2, 255, connectivity=6)


_WORKER = '''
import json, os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, {root!r})
from medical_segmentation_pytorch_amd.utils import metrics as M
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo', rank=rank, world_size=world)
data = torch.load({data!r})
acc = M.LesionAccumulator(3, 255)
ms = [cls(num_classes=3, accumulator=acc) for cls in M.LESION_METRICS.values()]
logits, target = data['logits'][rank::world].contiguous(), data['target'][rank::world].contiguous()
for m in ms:
    m.update(logits, target)
out = {{'compute': [float(m.compute()) for m in ms], 'counts': ms[0].counts().tolist()}}
json.dump(out, open(os.path.join({out!r}, f'rank{{rank}}.json'), 'w'))
dist.destroy_process_group()
'''


def test_sharded_compute_equals_single_process(tmp_path):
    from medical_segmentation_pytorch_amd.utils.launch import spawn_ranks
    g = torch.Generator().manual_seed(5)
    tgt = (torch.rand(4, 14, 18, generator=g) < 0.25).long() * torch.randint(1, 3, (4, 14, 18), generator=g)
    pred = torch.where(torch.rand(4, 14, 18, generator=g) < 0.8, tgt, torch.zeros_like(tgt))
    logits = _logits(pred, 3)
    torch.save({'logits': logits, 'target': tgt}, tmp_path / 'data.pt')
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER.format(root=ROOT, data=str(tmp_path / 'data.pt'), out=str(tmp_path)))
    assert spawn_ranks(2, [str(script)]) == 0
    acc = M.LesionAccumulator(3, 255)
    ms = [cls(num_classes=3, accumulator=acc) for cls in M.LESION_METRICS.values()]
    for m in ms:
        m.update(logits, tgt)
    assert int(acc.counts[0].min()) > 1
    for r in range(2):
        got = json.load(open(tmp_path / f'rank{r}.json'))
        assert got['counts'] == acc.counts.tolist()
        for i, m in enumerate(ms):
            assert abs(got['compute'][i] - float(m.compute())) <= 1e-7


# ---- configuration and wiring ---------------------------------------------------------------------------------------
def test_config_and_parser():
    from medical_segmentation_pytorch_amd.configs import MyConfig, load_parser
    c = MyConfig()
    assert (c.lesion_min_overlap, c.cc_connectivity, c.post_fill_holes, c.post_min_area, c.post_keep_largest) == \
        (0.0, 8, False, 0, False)
    for field, bad in (('lesion_min_overlap', -0.1), ('lesion_min_overlap', 1.01), ('cc_connectivity', 6),
                       ('post_min_area', -1)):
        c = MyConfig()
        setattr(c, field, bad)
        with pytest.raises(ValueError):
            c.init_dependent_config()
    for first in ('lesion_recall', 'lesion_precision', 'lesion_f1'):   # higher is better: any may drive selection
        c = MyConfig()
        c.metrics = [first, 'dice']
        c.init_dependent_config()
    c = load_parser(MyConfig(), ['--metrics', 'dice', 'lesion_f1', '--lesion_min_overlap', '0.25',
                                 '--cc_connectivity', '4', '--post_fill_holes', '--post_min_area', '20',
                                 '--post_keep_largest'])
    assert c.metrics == ['dice', 'lesion_f1'] and c.lesion_min_overlap == 0.25 and c.cc_connectivity == 4
    assert c.post_fill_holes is True and c.post_min_area == 20 and c.post_keep_largest is True
    c = load_parser(MyConfig(), [])
    assert c.post_fill_holes is False and c.post_keep_largest is False and c.post_min_area == 0
    with pytest.raises(SystemExit):
        load_parser(MyConfig(), ['--cc_connectivity', '6'])


class _Brightness(torch.nn.Module):
    """two-class logits from the image itself: foreground where the normalised image is bright"""

    def forward(self, x):
        v = x.mean(1, keepdim=True)
        return torch.cat([-v, v], 1)


def _predict_cfg(tmp_path, **kw):
    from PIL import Image
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.models import get_model
    folder = tmp_path / 'images'
    os.makedirs(folder, exist_ok=True)
    img = np.zeros((40, 48, 3), np.uint8)
    img[4:16, 5:20] = 255                            # the larger blob
    img[26:32, 30:40] = 255                          # the smaller one
    Image.fromarray(img).save(folder / 'two_blobs.png')
    c = MyConfig()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'pred')
    c.is_testing, c.test_data_folder, c.test_bs = True, str(folder), 1
    c.progress_bar, c.blend_prediction, c.base_workers = False, False, 0
    c.colormap_path = str(tmp_path / 'colormap.json')
    with open(c.colormap_path, 'w') as f:
        json.dump({'0': [0, 0, 0], '1': [250, 160, 30]}, f)
    for k, v in kw.items():
        setattr(c, k, v)
    c.init_dependent_config()
    c.DDP, c.gpu_num, c.num_workers = False, 1, 0
    os.makedirs(c.save_dir, exist_ok=True)
    c.load_ckpt_path = str(tmp_path / 'init.pth')
    torch.save({'state_dict': get_model(c).state_dict()}, c.load_ckpt_path)
    return c


def _predicted_foreground(tmp_path, monkeypatch, **kw):
    from PIL import Image
    from medical_segmentation_pytorch_amd.core import SegTrainer, seg_trainer
    c = _predict_cfg(tmp_path, **kw)
    t = SegTrainer(c)
    t.model = _Brightness()
    calls = []
    real = seg_trainer.colorize
    monkeypatch.setattr(seg_trainer, 'colorize', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    t.predict(c)
    rgb = torch.from_numpy(np.asarray(Image.open(os.path.join(c.save_dir, 'two_blobs.png')).convert('RGB')).copy())
    colors = t.colormap.cpu().to(torch.uint8)
    assert ((rgb == colors[0]).all(-1) | (rgb == colors[1]).all(-1)).all() and not torch.equal(colors[0], colors[1])
    return (rgb == colors[1]).all(-1), calls


def test_predict_keep_largest_saves_one_blob(tmp_path, monkeypatch):
    raw, calls = _predicted_foreground(tmp_path / 'raw', monkeypatch)
    assert len(calls) == 1 and int(CC.label(raw)[1]) == 2          # options off: the colorize path, two blobs
    assert int(raw.sum()) == 12 * 15 + 6 * 10
    kept, calls = _predicted_foreground(tmp_path / 'kept', monkeypatch, post_keep_largest=True)
    assert len(calls) == 0 and int(CC.label(kept)[1]) == 1
    want = torch.zeros_like(raw)
    want[4:16, 5:20] = True
    assert torch.equal(kept, want)
