"""Calibration metrics, temperature scaling and uncertainty maps, CPU tier: the plain-torch specification in
``ops/calibration.py`` against a pure-Python fp64 loop and hand-computed values, the metric objects' state handling,
the temperature fit against a golden-section search, config / checkpoint / trainer / predict wiring and the gloo
sync."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from medical_segmentation_pytorch_amd.ops import calibration as K
from medical_segmentation_pytorch_amd.utils import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255
NAMES = ('ece', 'mce', 'nll', 'brier')


def _batch(shape, seed, scale=2.0):
    """random logits and labels; a label 255, one == C and one == -1, and the last image fully ignored"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, h, w, generator=g) * scale
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0, 0, 0], t[0, -1, -1], t[0, h // 2, w // 2] = IGNORE, c, -1
    if n > 1:
        t[-1] = IGNORE
    return z, t


def _loop_oracle(z, t, T, bins, ignore_index=IGNORE):
    """the semantics of the issue, pixel by pixel in Python floats (fp64)"""
    n, c, h, w = z.shape
    count, correct, conf_sum, nll, brier = [0] * bins, [0] * bins, [0.0] * bins, 0.0, 0.0
    for i in range(n):
        for y in range(h):
            for x in range(w):
                lab = int(t[i, y, x])
                if lab == ignore_index or not 0 <= lab < c:
                    continue
                zs = [float(z[i, k, y, x]) / T for k in range(c)]
                m = max(zs)
                es = [math.exp(v - m) for v in zs]
                s = sum(es)
                p = [e / s for e in es]
                conf = max(p)
                pred = zs.index(m)                    # the first maximum
                b = min(bins - 1, int(conf * bins))
                count[b] += 1
                correct[b] += int(pred == lab)
                conf_sum[b] += conf
                nll += math.log(s) + m - zs[lab]
                brier += sum((p[k] - (k == lab)) ** 2 for k in range(c))
    return count, correct, conf_sum, nll, brier


def _values(state):
    return [float(v) for v in K.metrics_from_state(state['ints'], state['sums'])]


@pytest.mark.parametrize('shape,bins,T', [((2, 2, 6, 7), 15, 1.0), ((3, 4, 5, 5), 10, 2.5), ((2, 7, 4, 6), 64, 0.5)])
def test_plain_form_matches_python_loop(shape, bins, T):
    z, t = _batch(shape, 7 + bins)
    st = K.calibration_stats(z.double(), t, None, T, IGNORE, bins)
    count, correct, conf_sum, nll, brier = _loop_oracle(z.double(), t, T, bins)
    assert st['count'].tolist() == count and st['correct'].tolist() == correct and sum(count) > 20
    assert torch.allclose(st['conf_sum'], torch.tensor(conf_sum, dtype=torch.float64), rtol=1e-12, atol=1e-12)
    assert abs(float(st['nll_sum']) - nll) <= 1e-11 * nll and abs(float(st['brier_sum']) - brier) <= 1e-11 * brier
    v = sum(count)
    ece = sum(abs(a - b) for a, b in zip(correct, conf_sum)) / v
    mce = max(abs(a - b) / n for a, b, n in zip(correct, conf_sum, count) if n)
    for got, want in zip(_values(st), (ece, mce, nll / v, brier / v)):
        assert abs(got - want) <= 1e-11 * max(1.0, abs(want))
    # the fp32 form agrees to fp32 accuracy (a pixel may change bins at an edge, so the sums only)
    st32 = K.calibration_stats(z, t, None, T, IGNORE, bins)
    assert int(st32['count'].sum()) == v
    assert abs(float(st32['nll_sum']) - nll) <= 1e-5 * nll and abs(float(st32['brier_sum']) - brier) <= 1e-5 * brier


def test_four_pixels_by_hand():
    ln3, ln9 = math.log(3.0), math.log(9.0)
    # p = (.25, .75) hit | (.9, .1) miss | (.5, .5) tie -> class 0, hit | (.75, .25) hit
    z = torch.tensor([[0.0, ln3], [ln9, 0.0], [0.0, 0.0], [ln3, 0.0]], dtype=torch.float64).t().reshape(1, 2, 2, 2)
    t = torch.tensor([1, 1, 0, 0]).reshape(1, 2, 2)
    st = K.calibration_stats(z, t, None, 1.0, IGNORE, 5)
    assert st['count'].tolist() == [0, 0, 1, 2, 1] and st['correct'].tolist() == [0, 0, 1, 2, 0]
    assert torch.allclose(st['conf_sum'], torch.tensor([0, 0, 0.5, 1.5, 0.9], dtype=torch.float64), atol=1e-14)
    ece, mce, nll, brier = _values(st)
    assert abs(ece - 1.9 / 4) < 1e-14 and abs(mce - 0.9) < 1e-14
    assert abs(nll - (2 * -math.log(0.75) + math.log(10.0) + math.log(2.0)) / 4) < 1e-14
    assert abs(brier - (0.125 + 1.62 + 0.5 + 0.125) / 4) < 1e-14
    # T = 2 halves the logits: (0, ln 3) -> p = (1, sqrt 3) / (1 + sqrt 3)
    st2 = K.calibration_stats(z, t, None, 2.0, IGNORE, 5)
    r = math.sqrt(3.0) / (1 + math.sqrt(3.0))
    assert st2['count'].tolist() == [0, 0, 1, 3, 0]
    assert abs(float(st2['conf_sum'][3]) - (2 * r + 0.75)) < 1e-14


def test_validity_rule_and_empty():
    z, t = _batch((2, 3, 4, 5), 3)
    st = K.calibration_stats(z, t, None, 1.0, IGNORE, 15)
    assert int(st['count'].sum()) == 4 * 5 - 3                   # image 1 fully ignored; 255, C and -1 in image 0
    valid = (t != IGNORE) & (t >= 0) & (t < 3)
    assert int(valid.sum()) == 4 * 5 - 3
    only = K.calibration_stats(z, torch.where(valid, t, torch.full_like(t, IGNORE)), None, 1.0, IGNORE, 15)
    assert torch.equal(only['ints'], st['ints']) and torch.equal(only['sums'], st['sums'])
    # ignore_index None: 255 is out of range anyway
    assert torch.equal(K.calibration_stats(z, t, None, 1.0, None, 15)['count'], st['count'])
    # V = 0: nan, not an error; the state stays zero
    empty = K.calibration_stats(z[1:], t[1:], None, 1.0, IGNORE, 15)
    assert int(empty['ints'].sum()) == 0 and float(empty['sums'].abs().sum()) == 0
    assert all(math.isnan(v) for v in _values(empty))
    assert float(K.nll_grid(z[1:], t[1:], [1.0, 2.0], IGNORE).abs().sum()) == 0
    assert K.fit_temperature([(z[1:], t[1:])], IGNORE) == 1.0
    ms = [M.CALIBRATION_METRICS[n](num_classes=3, ignore_index=IGNORE) for n in NAMES]
    for m in ms:
        m.update(z[1:], t[1:])
        assert math.isnan(float(m.compute())) and m.compute().dtype == torch.float32


def test_one_bin():
    z, t = _batch((2, 3, 6, 6), 11)
    st = K.calibration_stats(z.double(), t, None, 1.0, IGNORE, 1)
    many = K.calibration_stats(z.double(), t, None, 1.0, IGNORE, 15)
    assert st['count'].tolist() == [int(many['count'].sum())] and st['correct'].tolist() == [int(many['correct'].sum())]
    ece, mce, nll, brier = _values(st)
    v = float(st['count'][0])
    assert abs(ece - abs(float(st['correct'][0]) - float(st['conf_sum'][0])) / v) < 1e-15 and ece == mce
    assert abs(nll - _values(many)[2]) < 1e-12 and abs(brier - _values(many)[3]) < 1e-12
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            K.calibration_stats(z, t, None, 1.0, IGNORE, bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            K.calibration_stats(z, t, None, bad, IGNORE, 15)


def test_sigmoid_head_is_two_class_softmax():
    g = torch.Generator().manual_seed(2)
    z = torch.randn(2, 1, 6, 5, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, 2, (2, 6, 5), generator=g)
    two = torch.cat([torch.zeros_like(z), z], 1)
    a, b = K.calibration_stats(z, t, None, 1.5, IGNORE, 15), K.calibration_stats(two, t, None, 1.5, IGNORE, 15)
    assert torch.equal(a['ints'], b['ints']) and torch.equal(a['sums'], b['sums'])
    # conf = max(sigmoid, 1 - sigmoid), nll = BCE-with-logits at z / T
    bce = torch.nn.functional.binary_cross_entropy_with_logits(z[:, 0] / 1.5, t.double(), reduction='sum')
    assert abs(float(a['nll_sum']) - float(bce)) < 1e-10
    assert torch.equal(K.nll_grid(z, t, [0.5, 1.0]), K.nll_grid(two, t, [0.5, 1.0]))
    for mode in K.MODES:
        assert torch.equal(K.uncertainty_map(z, 1.5, mode), K.uncertainty_map(two, 1.5, mode))
    p = torch.sigmoid(z[:, 0] / 1.5)
    want = ((1 - torch.maximum(p, 1 - p)) / 0.5 * 255).round().to(torch.uint8)
    assert torch.equal(K.uncertainty_map(z, 1.5, 'confidence'), want)


def test_two_batches_equal_one():
    z, t = _batch((4, 3, 9, 8), 5)
    t[-1] = torch.randint(0, 3, (9, 8), generator=torch.Generator().manual_seed(1))
    one = K.calibration_stats(z, t, None, 1.3, IGNORE, 15)
    two = K.calibration_stats(z[:1], t[:1], None, 1.3, IGNORE, 15)
    K.calibration_stats(z[1:], t[1:], two, 1.3, IGNORE, 15)
    assert torch.equal(one['ints'], two['ints'])
    assert torch.allclose(one['sums'], two['sums'], rtol=1e-12, atol=0)
    betas = [0.5, 1.0, 1.7]
    s1 = K.nll_grid(z, t, betas, IGNORE)
    s2 = K.nll_grid(z[1:], t[1:], betas, IGNORE, K.nll_grid(z[:1], t[:1], betas, IGNORE))
    assert torch.allclose(s1, s2, rtol=1e-12, atol=0)
    assert abs(float(s1[1]) - float(K.calibration_stats(z, t, None, 1.0, IGNORE, 15)['nll_sum'])) < 1e-4
    with pytest.raises(ValueError):
        K.calibration_stats(z, t, one, 1.0, IGNORE, 10)         # a state of another bin count
    with pytest.raises(ValueError):
        K.nll_grid(z, t, [1.0] * 65)


def test_shared_accumulator_scores_a_batch_once(monkeypatch):
    calls = []
    real = K.calibration_stats
    monkeypatch.setattr(K, 'calibration_stats', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cfg = SimpleNamespace(num_class=3, ignore_index=IGNORE, calibration_bins=10)
    ms = [M.get_seg_metrics(cfg, n) for n in NAMES]
    assert all(m.acc is ms[0].acc for m in ms) and ms[0].acc.bins == 10
    assert tuple(ms[0].acc.temperature.shape) == (1,) and float(ms[0].acc.temperature) == 1.0
    z, t = _batch((2, 3, 6, 6), 9)
    for m in ms:
        m.update(z, t)
    assert len(calls) == 1
    want = _values(K.calibration_stats(z, t, None, 1.0, IGNORE, 10))
    for m, w in zip(ms, want):
        assert abs(float(m.compute()) - w) <= 1e-6 * max(1.0, abs(w))
    for m in ms:                                                 # the same tensors again: a new batch, scored once
        m.update(z, t)
    assert len(calls) == 3 and int(ms[0].acc.ints[0].sum()) == 2 * int(real(z, t, None, 1.0, IGNORE, 10)['count'].sum())
    rel = ms[0].reliability()
    assert rel['count'].tolist() == ms[0].acc.ints[0].tolist() and rel['accuracy'].shape == (10,)
    some = rel['count'] > 0
    assert bool(rel['accuracy'][~some].isnan().all()) and bool((rel['confidence'][some] > 1 / 3).all())
    ms[2].reset()
    assert int(ms[0].acc.ints.sum()) == 0 and float(ms[0].acc.sums.abs().sum()) == 0
    # the temperature is the accumulator's: T = 2 gives the T = 2 statistics
    ms[0].acc.set_temperature(2.0)
    assert float(ms[0].acc.temperature) == 2.0
    ms[1].update(z, t)
    want2 = _values(real(z, t, None, 2.0, IGNORE, 10))
    assert abs(float(ms[0].compute()) - want2[0]) < 1e-6 and abs(float(ms[2].compute()) - want2[2]) < 1e-6
    cfg.calibration_bins = 15
    assert M.get_seg_metrics(cfg, 'ece').acc is not ms[0].acc
    one = M.get_seg_metrics(SimpleNamespace(num_class=1, ignore_index=IGNORE), 'brier')
    assert one.num_classes == 2 and one.acc.bins == 15
    assert set(NAMES) <= set(M.LOWER_IS_BETTER) and set(M.CALIBRATION_METRICS) == set(NAMES)


# ---- the temperature fit ---------------------------------------------------------------------------------------------
def _nll_at(z64, t, log2_t):
    return float(K.nll_grid(z64, t, [2.0 ** -log2_t], IGNORE, native=False)[0])


def golden_section_log2_t(z64, t, lo=-3.0, hi=3.0, iters=80):
    """argmin over log2 T of the fp64 NLL (convex in 1 / T)"""
    r = (math.sqrt(5.0) - 1) / 2
    a, b = lo, hi
    c, d = b - r * (b - a), a + r * (b - a)
    fc, fd = _nll_at(z64, t, c), _nll_at(z64, t, d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - r * (b - a)
            fc = _nll_at(z64, t, c)
        else:
            a, c, fc = c, d, fd
            d = a + r * (b - a)
            fd = _nll_at(z64, t, d)
    return (a + b) / 2


def fit_case(t0, seed=0, shape=(2, 3, 24, 24)):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    base = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2
    p = torch.softmax(base, 1).permute(0, 2, 3, 1).reshape(-1, c)
    labels = torch.multinomial(p, 1, generator=g).view(n, h, w)
    labels[0, 0, :5] = IGNORE
    return (t0 * base).float(), labels


@pytest.mark.parametrize('t0', [0.5, 1.0, 2.5])
def test_fit_temperature_against_golden_section(t0):
    z, t = fit_case(t0)
    T, info = K.fit_temperature([(z[:1], t[:1]), (z[1:], t[1:])], IGNORE, 2, return_info=True)
    star = golden_section_log2_t(z.double(), t)
    step = 6 / 32 * 2 / 32
    err = abs(math.log2(T) - star)
    print(f'T0 {t0}: T_fit {T!r} T* {2 ** star!r} |log2| {err:.5f} step {step:.5f}')
    assert err <= step and abs(star - math.log2(t0)) < 0.2
    assert _nll_at(z.double(), t, math.log2(T)) <= _nll_at(z.double(), t, 0.0)
    assert info['rounds'] == 2 and len(info['exponents']) == 33 and T == 1.0 / float(
        torch.tensor(2.0 ** info['exponents'][info['index']], dtype=torch.float64).float())
    # one round: the coarse grid; more rounds never do worse on the grid's own sums
    T1 = K.fit_temperature([(z, t)], IGNORE, 1)
    assert abs(math.log2(T1) - star) <= 6 / 32
    T3 = K.fit_temperature(lambda: iter([(z, t)]), IGNORE, 3)
    assert abs(math.log2(T3) - star) <= 6 / 32 * (2 / 32) ** 2 + 1e-6
    with pytest.raises(ValueError):
        K.fit_temperature([(z, t)], IGNORE, 5)


def test_grid_construction():
    e = K.first_exponents()
    assert len(e) == 33 and e[0] == -3.0 and e[16] == 0.0 and e[32] == 3.0
    r = K.refine_exponents(e, 20)
    assert r[0] == e[19] and r[32] == e[21] and r[16] == e[20]
    assert K.refine_exponents(e, 0)[0] == e[0] and K.refine_exponents(e, 0)[32] == e[1]
    assert K.refine_exponents(e, 32)[0] == e[31] and K.refine_exponents(e, 32)[32] == e[32]


# ---- uncertainty maps ------------------------------------------------------------------------------------------------
def test_uncertainty_map_values():
    z = torch.zeros(1, 4, 2, 3, dtype=torch.float64)
    z[0, 2, 0, 0] = 50.0                                       # certain
    z[0, :2, 1, 1] = 30.0                                      # two classes tie: H = ln 2, conf = 1/2
    ent, conf = K.uncertainty_map(z, 1.0, 'entropy'), K.uncertainty_map(z, 1.0, 'confidence')
    assert ent.dtype == torch.uint8 and ent.shape == (1, 2, 3)
    assert int(ent[0, 0, 0]) == 0 and int(conf[0, 0, 0]) == 0 and int(ent[0, 0, 1]) == 255 and int(conf[0, 0, 1]) == 255
    assert int(ent[0, 1, 1]) == round(255 * math.log(2) / math.log(4)) and int(conf[0, 1, 1]) == round(255 * 0.5 / 0.75)
    hot = K.uncertainty_map(z, 100.0, 'entropy')               # a high temperature whitens
    assert int(hot[0, 0, 0]) > 200
    with pytest.raises(ValueError):
        K.uncertainty_map(z, 1.0, 'variance')
    with pytest.raises(ValueError):
        K.uncertainty_map(z, 0.0, 'entropy')


# ---- configuration and wiring ---------------------------------------------------------------------------------------
def test_config_and_parser():
    from medical_segmentation_pytorch_amd.configs import MyConfig, load_parser
    c = MyConfig()
    assert (c.calibration_bins, c.calibrate_temperature, c.calibration_rounds, c.temperature, c.save_uncertainty) == \
        (15, False, 2, None, None)
    for field, bad in (('calibration_bins', 0), ('calibration_bins', 65), ('calibration_bins', 2.5),
                       ('calibration_rounds', 0), ('calibration_rounds', 5), ('temperature', 0.0),
                       ('temperature', -1.0), ('temperature', float('inf')), ('temperature', 'hot'),
                       ('save_uncertainty', 'variance'), ('calibrate_temperature', 'yes')):
        c = MyConfig()
        setattr(c, field, bad)
        with pytest.raises(ValueError):
            c.init_dependent_config()
    for first in NAMES:                                         # lower is better: none may drive the selection
        c = MyConfig()
        c.metrics = [first, 'dice']
        with pytest.raises(ValueError):
            c.init_dependent_config()
        c.metrics = ['dice', first]
        c.init_dependent_config()
    c = load_parser(MyConfig(), ['--metrics', 'dice', 'ece', 'mce', 'nll', 'brier', '--calibration_bins', '20',
                                 '--calibrate_temperature', '--calibration_rounds', '3', '--temperature', '1.5',
                                 '--save_uncertainty', 'confidence'])
    assert c.metrics == ['dice', 'ece', 'mce', 'nll', 'brier'] and c.calibration_bins == 20
    assert c.calibrate_temperature is True and c.calibration_rounds == 3 and c.temperature == 1.5
    assert c.save_uncertainty == 'confidence'
    c = load_parser(MyConfig(), [])
    assert c.calibrate_temperature is False and c.temperature is None and c.save_uncertainty is None
    with pytest.raises(SystemExit):
        load_parser(MyConfig(), ['--save_uncertainty', 'variance'])


class _Brightness(torch.nn.Module):
    """two-class logits from the image itself: foreground where the normalised image is bright"""

    def forward(self, x):
        v = x.mean(1, keepdim=True)
        return torch.cat([-v, v], 1)


def _predict_cfg(tmp_path, ckpt_extra=None, **kw):
    from PIL import Image
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.models import get_model
    folder = tmp_path / 'images'
    os.makedirs(folder, exist_ok=True)
    g = np.random.default_rng(0)
    img = (g.random((40, 37, 3)) * 255).astype(np.uint8)
    img[4:16, 5:20] = 255
    Image.fromarray(img).save(folder / 'blob.png')
    c = MyConfig()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'pred')
    c.is_testing, c.test_data_folder, c.test_bs = True, str(folder), 1
    c.progress_bar, c.blend_prediction, c.base_workers = False, False, 0
    for k, v in kw.items():
        setattr(c, k, v)
    c.init_dependent_config()
    c.DDP, c.gpu_num, c.num_workers = False, 1, 0
    os.makedirs(c.save_dir, exist_ok=True)
    c.load_ckpt_path = str(tmp_path / 'init.pth')
    torch.save({'state_dict': get_model(c).state_dict(), **(ckpt_extra or {})}, c.load_ckpt_path)
    return c


def test_checkpoint_round_trip(tmp_path):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.core.seg_trainer import add_checkpoint_temperature
    c = _predict_cfg(tmp_path / 'old')
    assert SegTrainer(c).temperature == 1.0                      # a checkpoint without the key
    before = torch.load(c.load_ckpt_path, weights_only=True)
    before.update(cur_epoch=3, best_score=0.5, optimizer=None, scheduler=None)
    torch.save(before, c.load_ckpt_path)
    add_checkpoint_temperature(c.load_ckpt_path, 1.75)
    after = torch.load(c.load_ckpt_path, weights_only=True)
    assert after['temperature'] == 1.75 and isinstance(after['temperature'], float)
    assert set(after) == set(before) | {'temperature'}
    for k, v in before.items():
        if k == 'state_dict':
            assert list(v) == list(after[k]) and all(torch.equal(v[n], after[k][n]) for n in v)
        else:
            assert after[k] == v
    assert SegTrainer(c).temperature == 1.75
    c.temperature = 0.8                                          # the override wins
    assert SegTrainer(c).temperature == 0.8
    with pytest.raises(ValueError):
        add_checkpoint_temperature(c.load_ckpt_path, 0.0)
    assert not os.path.exists(c.load_ckpt_path + '.tmp')


def test_predict_writes_uncertainty_maps(tmp_path):
    from PIL import Image
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = _predict_cfg(tmp_path / 'plain')
    t = SegTrainer(c)
    t.model = _Brightness()
    t.predict(c)
    plain = set(os.listdir(c.save_dir))                          # the flag unset: exactly the files of before
    assert 'blob.png' in plain and not any('unc' in f for f in plain)
    mask = Image.open(os.path.join(c.save_dir, 'blob.png'))
    means = {}
    for mode, T in (('entropy', 1.0), ('confidence', 1.0), ('entropy', 4.0)):
        c = _predict_cfg(tmp_path / f'{mode}{T}', ckpt_extra={'temperature': T}, save_uncertainty=mode)
        t = SegTrainer(c)
        t.model = _Brightness()
        assert t.temperature == T
        t.predict(c)
        assert set(os.listdir(c.save_dir)) == plain | {'blob_unc.png'}
        unc = Image.open(os.path.join(c.save_dir, 'blob_unc.png'))
        assert unc.mode == 'L' and unc.size == mask.size
        assert np.array_equal(np.asarray(Image.open(os.path.join(c.save_dir, 'blob.png'))), np.asarray(mask))
        a = np.asarray(unc)
        means[(mode, T)] = a.mean()
        assert a[6:14, 7:18].mean() < a.mean()                  # the saturated blob is the certain region
    assert means[('entropy', 4.0)] > means[('entropy', 1.0)]


def _train_cfg(tmp, metrics, **kw):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    c = MyConfig()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp / 'data'), str(tmp / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 4, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 2, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 1, 0, False, True
    c.metrics = list(metrics)
    c.random_seed = 1
    for k, v in kw.items():
        setattr(c, k, v)
    c.init_dependent_config()
    c.DDP, c.gpu_num, c.num_workers = False, 1, 0
    return c


def test_trainer_run_with_temperature_calibration(tmp_path):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = _train_cfg(tmp_path, ['dice', 'ece', 'nll'], calibrate_temperature=True, calibration_bins=10)
    t = SegTrainer(c)
    best_score = t.run(c)

    def strict(name):
        raise AssertionError(f'{name} in val_history.json')
    h = json.loads(open(os.path.join(c.save_dir, 'val_history.json')).read(), parse_constant=strict)
    hist = h['history']
    # epoch validation, val_best on val, the calibrated validation, val_best on the test split
    assert [r['val_best'] for r in hist] == [False, True, True, True]
    assert [bool(r.get('calibrated')) for r in hist] == [False, False, True, False]
    for r in hist:
        cal = r['calibration']
        assert cal['bins'] == 10 and len(cal['count']) == len(cal['accuracy']) == len(cal['confidence']) == 10
        assert sum(cal['count']) == 4 * 64 * 64
        assert r['ece'] is not None and r['nll'] > 0
    best = torch.load(os.path.join(c.save_dir, 'best.pth'), weights_only=True)
    T = best['temperature']
    assert isinstance(T, float) and T == t.temperature and 1 / 8 <= T <= 8
    assert set(best) == {'cur_epoch', 'best_score', 'state_dict', 'optimizer', 'scheduler', 'temperature'}
    before, after, test = hist[1], hist[2], hist[3]
    assert before['calibration']['temperature'] == 1.0 and after['calibration']['temperature'] == T
    assert test['calibration']['temperature'] == T              # the held-out split at the stored temperature
    assert before['dice'] == after['dice'] == h['best_score'] == float(best_score)
    assert after['nll'] <= before['nll'] + 1e-7                 # float32 records of NLL(T_fit) <= NLL(1)
    # a run without the flag: no key, no calibrated record
    c2 = _train_cfg(tmp_path / 'plain', ['dice', 'ece'])
    SegTrainer(c2).run(c2)
    h2 = json.load(open(os.path.join(c2.save_dir, 'val_history.json')))['history']
    assert not any('calibrated' in r for r in h2) and all(r['calibration']['temperature'] == 1.0 for r in h2)
    assert 'temperature' not in torch.load(os.path.join(c2.save_dir, 'best.pth'), weights_only=True)
    # tools/calibrate.py on that uncalibrated checkpoint: the key is added in place, one JSON result
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import calibrate
    finally:
        sys.path.pop(0)
    ckpt2 = os.path.join(c2.save_dir, 'best.pth')
    old = torch.load(ckpt2, weights_only=True)
    out = calibrate.main(['--ckpt', ckpt2, '--model', 'unet', '--base_channel', '8', '--data_root', c2.data_root,
                          '--save_dir', str(tmp_path / 'tool'), '--synthetic_data', '--synthetic_num', '8', '4', '4',
                          '--synthetic_size', '64', '--crop_size', '64', '--val_bs', '2', '--base_workers', '0',
                          '--no_progress_bar', '--metrics', 'dice'])
    new = torch.load(ckpt2, weights_only=True)
    assert new['temperature'] == out['T'] and out['T_before'] == 1.0 and out['nll_after'] <= out['nll_before'] + 1e-7
    assert set(new) == set(old) | {'temperature'} and out['pixels'] == 4 * 64 * 64
    assert all(torch.equal(v, new['state_dict'][k]) for k, v in old['state_dict'].items())
    c3 = _train_cfg(tmp_path / 'none', ['dice'])
    t3 = SegTrainer(c3)
    t3.val_best(c3, t3.val_loader, ckpt_path=os.path.join(c.save_dir, 'best.pth'))
    assert t3.temperature == T and 'calibration' not in t3.val_history[-1]


# ---- gloo world 2 --------------------------------------------------------------------------------------------------------
_WORKER = '''
import json, os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, {root!r})
from medical_segmentation_pytorch_amd.ops import calibration as K
from medical_segmentation_pytorch_amd.utils import metrics as M
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo', rank=rank, world_size=world)
data = torch.load({data!r})
acc = M.CalibrationAccumulator(3, 255, 15)
ms = [cls(num_classes=3, accumulator=acc) for cls in M.CALIBRATION_METRICS.values()]
logits, target = data['logits'][rank::world].contiguous(), data['target'][rank::world].contiguous()
for m in ms:
    m.update(logits, target)
out = {{'compute': [float(m.compute()) for m in ms], 'count': ms[0].reliability()['count'].tolist(),
       'T': K.fit_temperature([(logits, target)], 255, 2)}}
json.dump(out, open(os.path.join({out!r}, f'rank{{rank}}.json'), 'w'))
dist.destroy_process_group()
'''


def test_sharded_compute_equals_single_process(tmp_path):
    from medical_segmentation_pytorch_amd.utils.launch import spawn_ranks
    logits, tgt = fit_case(2.5, seed=3, shape=(4, 3, 14, 18))
    torch.save({'logits': logits, 'target': tgt}, tmp_path / 'data.pt')
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER.format(root=ROOT, data=str(tmp_path / 'data.pt'), out=str(tmp_path)))
    assert spawn_ranks(2, [str(script)]) == 0
    acc = M.CalibrationAccumulator(3, 255, 15)
    ms = [cls(num_classes=3, accumulator=acc) for cls in M.CALIBRATION_METRICS.values()]
    for m in ms:
        m.update(logits, tgt)
    T = K.fit_temperature([(logits, tgt)], 255, 2)
    assert 2.0 < T < 3.2
    for r in range(2):
        got = json.load(open(tmp_path / f'rank{r}.json'))
        assert got['count'] == acc.ints[0].tolist() and got['T'] == T
        for i, m in enumerate(ms):
            assert abs(got['compute'][i] - float(m.compute())) <= 1e-6
