"""Sliding-window inference with flip TTA: the plain-torch specification (``ops/tiled.py``) on the CPU -- geometry,
partition of unity, un-mirroring, padding, chunk independence, the 'probs' mode, the config fields and the trainer
entry points.

The bar of the fp32 comparisons is ``(2K + 3) * 2^-24 * max|value|``: the fp32 bound of a K-term weighted sum, a
K-term normaliser and one division, K = the largest number of (window, view) terms on a pixel of the case."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from medical_segmentation_pytorch_amd.ops import tiled as T

EPS = 2.0 ** -24
# (H, W, wh, ww, overlap)
SHAPES = [(70, 93, 32, 32, .5), (33, 70, 32, 64, .25), (40, 40, 32, 32, .75), (20, 50, 32, 32, .5),
          (97, 131, 64, 32, .6), (17, 23, 5, 12, .5), (32, 32, 32, 32, .5), (64, 96, 32, 32, 0)]


def _bar(plan, peak):
    return (2 * plan.max_terms + 3) * EPS * float(peak)


def test_window_starts_examples():
    assert T.window_starts(93, 32, .5) == [0, 16, 32, 48, 61]
    assert T.window_starts(70, 32, .5) == [0, 16, 32, 38]
    assert T.window_starts(33, 32, .25) == [0, 1]
    assert T.window_starts(20, 32, .5) == [0]
    assert T.window_starts(64, 32, 0) == [0, 32]
    with pytest.raises(ValueError):
        T.window_starts(64, 32, 0.8)


def test_window_starts_properties():
    rs = np.random.RandomState(0)
    for _ in range(300):
        w = int(rs.randint(1, 80))
        L = int(rs.randint(w + 1, 400))
        o = float(rs.choice([0, .1, .25, .5, .6, .75, rs.rand() * .75]))
        s = T.window_starts(L, w, o)
        assert s[0] == 0 and s[-1] == L - w
        assert all(b > a for a, b in zip(s, s[1:]))
        covered = np.zeros(L, bool)
        for a in s:
            covered[a:a + w] = True
        assert covered.all()
        assert len(s) == -(-(L - w) // max(1, int(w * (1 - o)))) + 1


def test_importance_vectors():
    wy, wx = T.importance_vectors(32, 64, 'constant')
    assert torch.equal(wy, torch.ones(32)) and torch.equal(wx, torch.ones(64))
    wy, wx = T.importance_vectors(352, 5, 'gaussian', 0.125)
    assert wy.dtype == torch.float32 and wy.shape == (352,) and wx.shape == (5,)
    k = np.arange(352, dtype=np.float64)
    want = np.exp(-(k - 175.5) ** 2 / (2 * (0.125 * 352) ** 2)).astype(np.float32)
    assert np.array_equal(wy.numpy(), want)
    assert torch.equal(wy, wy.flip(0)) and float(wy[0] * wy[0]) > 1e-8      # symmetric, far above underflow
    with pytest.raises(ValueError):
        T.importance_vectors(8, 8, 'hann')
    with pytest.raises(ValueError):
        T.importance_vectors(8, 8, 'gaussian', 0.0)


def test_plan_counts_terms():
    p = T.tile_plan(70, 93, 32, .5, 'gaussian', .125, 'hv')
    assert (p.ny, p.nx, p.V) == (4, 5, 4) and p.max_terms == 36 and p.windows(3) == 240
    assert p.decode(((2 * 4 + 3) * 5 + 1) * 4 + 2) == (2, 3, 1, 2)
    p = T.tile_plan(20, 50, 32, .5)
    assert (p.py, p.px, p.Hp, p.Wp, p.ny) == (6, 0, 32, 50, 1)


@pytest.mark.parametrize('blend', T.BLENDS)
@pytest.mark.parametrize('flips', T.FLIPS)
@pytest.mark.parametrize('average', T.AVERAGES)
def test_partition_of_unity(blend, flips, average):
    for (h, w, wh, ww, o) in [(70, 93, 32, 32, .5), (33, 70, 32, 64, .25), (64, 96, 32, 32, 0)]:
        plan = T.tile_plan(h, w, (wh, ww), o, blend, .125, flips)
        img = torch.full((2, 3, h, w), 1.75)
        img[:, 1] = -0.5
        img[:, 2] = 0.25
        out = T.sliding_window_inference(img, lambda x: x, (wh, ww), o, blend, .125, flips, average, batch=7)
        assert out.shape == img.shape and out.dtype == torch.float32
        if average == 'logits':
            assert float((out - img).abs().max()) <= _bar(plan, 1.75)
        else:                       # the logits of the averaged softmax: the constant's log-softmax
            want = torch.log_softmax(img.double(), 1)
            assert float((out.double() - want).abs().max()) <= 1e-5


@pytest.mark.parametrize('shape', SHAPES)
def test_pointwise_predictor_equals_whole_image(shape):
    h, w, wh, ww, o = shape
    torch.manual_seed(1)
    weight, bias = torch.randn(4, 3, 1, 1), torch.randn(4)
    img = torch.randn(2, 3, h, w)
    whole = F.conv2d(img, weight, bias)
    for flips, blend in (('', 'gaussian'), ('hv', 'gaussian'), ('h', 'constant')):
        plan = T.tile_plan(h, w, (wh, ww), o, blend, .125, flips)
        out = T.sliding_window_inference(img, lambda x: F.conv2d(x, weight, bias), (wh, ww), o, blend, .125, flips,
                                         batch=5)
        assert out.shape == whole.shape and float((out - whole).abs().max()) <= _bar(plan, whole.abs().max())


def _shift_right(x):
    return F.pad(x, (1, 0))[..., :-1]


def _shift_down(x):
    return F.pad(x, (0, 0, 1, 0))[..., :-1, :]


def test_unmirroring_is_done():
    torch.manual_seed(2)
    img = torch.randn(2, 3, 16, 24)
    out = T.sliding_window_inference(img, _shift_right, (16, 24), 0.5, 'constant', flips='h')
    left = F.pad(img, (0, 1))[..., 1:]
    assert torch.allclose(out, (_shift_right(img) + left) / 2, rtol=0, atol=4 * EPS * float(img.abs().max()))
    out = T.sliding_window_inference(img, _shift_down, (16, 24), 0.5, 'gaussian', flips='v')
    up = F.pad(img, (0, 0, 0, 1))[..., 1:, :]
    assert torch.allclose(out, (_shift_down(img) + up) / 2, rtol=0, atol=7 * EPS * float(img.abs().max()))
    # a mirror that was not undone would give the shifted image alone
    assert not torch.allclose(out, _shift_down(img), atol=1e-3)


def test_flip_equivariant_predictor():
    torch.manual_seed(3)
    img = torch.randn(1, 2, 70, 93)
    k = torch.full((2, 1, 3, 3), 1 / 9.)

    def box(x):
        return F.conv2d(x, k, padding=1, groups=2)
    plain = T.sliding_window_inference(img, box, 32, flips='')
    tta = T.sliding_window_inference(img, box, 32, flips='hv')
    plan = T.tile_plan(70, 93, 32, .5, 'gaussian', .125, 'hv')
    assert float((plain - tta).abs().max()) <= _bar(plan, plain.abs().max())


def test_small_image_padding_and_crop():
    torch.manual_seed(4)
    img = torch.randn(2, 3, 20, 50) + 3.0
    seen = []

    def identity(x):
        seen.append(x.clone())
        return x
    out = T.sliding_window_inference(img, identity, 32, 0.5, 'constant', batch=100)
    assert out.shape == (2, 3, 20, 50)
    assert float((out - img).abs().max()) <= 9 * EPS * float(img.abs().max())
    win = seen[0]
    assert win.shape == (2 * 1 * 3, 3, 32, 32)                 # x starts [0, 16, 18]
    assert torch.equal(win[0, :, 6:26, :], img[0, :, :, 0:32]) and torch.equal(win[2, :, 6:26, :], img[0, :, :, 18:50])
    assert float(win[:, :, :6].abs().max()) == 0 and float(win[:, :, 26:].abs().max()) == 0
    assert bool((win[:, :, 6:26] != 0).all())


def test_gather_past_the_end_is_zero():
    img = torch.randn(1, 3, 40, 40) + 5
    plan = T.tile_plan(40, 40, 32, .75, flips='h')
    m = plan.windows(1)
    g = T.gather_windows(img, plan, m - 2, 5)
    assert g.shape == (5, 3, 32, 32) and bool((g[:2] != 0).all()) and float(g[2:].abs().max()) == 0
    assert torch.equal(g[1], img[0, :, 8:40, 8:40].flip(-1))


@pytest.mark.parametrize('average', T.AVERAGES)
def test_chunking_is_bitwise_irrelevant(average):
    torch.manual_seed(5)
    for c in (1, 3):
        plan = T.tile_plan(70, 93, 32, .5, 'gaussian', .125, 'hv')
        logits = 3 * torch.randn(plan.windows(2), c, 32, 32)
        ref = T.blend_windows(logits, plan, 2, average, batch=None)
        for batch in (1, 5):
            assert torch.equal(T.blend_windows(logits, plan, 2, average, batch=batch), ref)
    img = torch.randn(2, 3, 40, 40)
    outs = [T.sliding_window_inference(img, lambda x: x[:, :2] * 2, 32, .75, flips='v', average=average, batch=b)
            for b in (1, 5, 10 ** 6)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def _probs_oracle(logits, plan, n):
    """fp64 average of the per-window softmax / sigmoid, by hand"""
    c = logits.shape[1]
    num = torch.zeros(n, c, plan.Hp, plan.Wp, dtype=torch.float64)
    den = torch.zeros(n, 1, plan.Hp, plan.Wp, dtype=torch.float64)
    wt = plan.wy.double()[:, None] * plan.wx.double()[None, :]
    for m in range(plan.windows(n)):
        i, iy, ix, v = plan.decode(m)
        x = logits[m].double()
        p = torch.sigmoid(x) if c == 1 else torch.softmax(x, 0)
        fx, fy = plan.views[v]
        p = p.flip([d for d, f in ((-1, fx), (-2, fy)) if f]) if fx or fy else p
        y0, x0 = plan.sy[iy], plan.sx[ix]
        num[i, :, y0:y0 + plan.wh, x0:x0 + plan.ww] += wt * p
        den[i, :, y0:y0 + plan.wh, x0:x0 + plan.ww] += wt
    return (num / den)[:, :, plan.py:plan.py + plan.H, plan.px:plan.px + plan.W]


@pytest.mark.parametrize('c', [1, 3])
def test_probs_mode(c):
    torch.manual_seed(6)
    plan = T.tile_plan(20, 70, 32, .5, 'gaussian', .125, 'hv')
    logits = 3 * torch.randn(plan.windows(2), c, 32, 32)
    out = T.blend_windows(logits, plan, 2, 'probs', batch=4)
    got = torch.sigmoid(out.double()) if c == 1 else torch.softmax(out.double(), 1)
    assert float((got - _probs_oracle(logits, plan, 2)).abs().max()) <= 2e-5
    extreme = logits.clone()
    extreme[:, 0] = 200.0
    extreme[::2, 0] = -200.0
    extreme[1, :] = 200.0
    for t in (extreme, torch.full_like(logits, 200.0), torch.full_like(logits, -200.0)):
        assert bool(torch.isfinite(T.blend_windows(t, plan, 2, 'probs')).all())


# ---- configuration ----------------------------------------------------------------------------------------
def _cfg():
    from medical_segmentation_pytorch_amd.configs import MyConfig
    return MyConfig()


@pytest.mark.parametrize('field,value', [('infer_overlap', -0.1), ('infer_overlap', 0.8), ('infer_blend', 'hann'),
                                         ('tta_flips', 'vh'), ('tta_flips', 'x'), ('tta_average', 'mean'),
                                         ('infer_sigma_scale', 0.0), ('infer_sigma_scale', -1.0), ('infer_batch', 0),
                                         ('infer_window', 0), ('infer_window', (64, -32)), ('infer_window', (1, 2, 3))])
def test_config_rejects(field, value):
    c = _cfg()
    setattr(c, field, value)
    with pytest.raises(ValueError):
        c.init_dependent_config()


def test_config_window_must_follow_the_stride():
    c = _cfg()
    c.val_img_stride, c.infer_window = 32, 80
    with pytest.raises(ValueError):
        c.init_dependent_config()
    c.infer_window = [96]
    c.init_dependent_config()
    assert c.infer_window == (96, 96) and c.inference_settings()['window'] == (96, 96)


def test_config_defaults_are_off():
    c = _cfg()
    c.init_dependent_config()
    assert c.infer_window is None and c.tta_flips == '' and c.inference_settings() is None
    assert (c.infer_overlap, c.infer_blend, c.infer_sigma_scale, c.infer_batch, c.tta_average) == \
        (0.5, 'gaussian', 0.125, 16, 'logits')


def test_parser_round_trip():
    from medical_segmentation_pytorch_amd.configs import load_parser
    c = load_parser(_cfg(), ['--infer_window', '64', '96', '--infer_overlap', '0.25', '--infer_blend', 'constant',
                             '--infer_sigma_scale', '0.2', '--infer_batch', '4', '--tta_flips', 'hv', '--tta_average',
                             'probs'])
    assert c.inference_settings() == {'window': (64, 96), 'overlap': 0.25, 'blend': 'constant', 'sigma_scale': 0.2,
                                      'flips': 'hv', 'average': 'probs', 'batch': 4}
    c = load_parser(_cfg(), ['--infer_window', '352'])
    assert c.infer_window == (352, 352) and c.inference_settings()['flips'] == ''
    c = load_parser(_cfg(), ['--tta_flips', 'h'])
    assert c.inference_settings()['window'] is None
    assert load_parser(_cfg(), []).inference_settings() is None
    with pytest.raises(ValueError):
        load_parser(_cfg(), ['--infer_overlap', '0.9'])


# ---- trainer entry points ---------------------------------------------------------------------------------
def _train_cfg(tmp_path, size=64, **kw):
    c = _cfg()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 4, 4), size
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 4, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 1, 0, False, False
    c.use_tb, c.engine = False, 'eager'
    for k, v in kw.items():
        setattr(c, k, v)
    c.init_dependent_config()
    return c


def _predict_cfg(tmp_path, shape=(48, 64), **kw):
    from PIL import Image
    from medical_segmentation_pytorch_amd.models import get_model
    folder = tmp_path / 'images'
    os.makedirs(folder, exist_ok=True)
    rs = np.random.RandomState(7)
    Image.fromarray((rs.rand(*shape, 3) * 255).astype(np.uint8)).save(folder / 'frame.png')
    c = _cfg()
    c.model, c.base_channel = 'unet', 8
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'pred')
    c.is_testing, c.test_data_folder, c.test_bs = True, str(folder), 1
    c.progress_bar, c.blend_prediction, c.base_workers, c.engine = False, False, 0, 'eager'
    c.colormap_path = str(tmp_path / 'colormap.json')
    with open(c.colormap_path, 'w') as f:
        json.dump({'0': [0, 0, 0], '1': [250, 160, 30]}, f)
    for k, v in kw.items():
        setattr(c, k, v)
    c.init_dependent_config()
    c.DDP, c.gpu_num, c.num_workers = False, 1, 0
    os.makedirs(c.save_dir, exist_ok=True)
    c.load_ckpt_path = str(tmp_path / 'init.pth')
    torch.manual_seed(8)
    torch.save({'state_dict': get_model(c).state_dict()}, c.load_ckpt_path)
    return c


def _forbid_tiled(monkeypatch):
    from medical_segmentation_pytorch_amd.core import seg_trainer

    def boom(*a, **k):
        raise AssertionError('ops.tiled was called with the inference options unset')
    for name in ('sliding_window_inference', 'gather_windows', 'blend_windows', 'accumulate_windows',
                 'finalize_windows', 'tile_plan', 'window_starts', 'importance_vectors'):
        monkeypatch.setattr(T, name, boom)
    monkeypatch.setattr(seg_trainer, 'sliding_window_inference', boom)


def test_defaults_never_reach_the_tiled_ops(tmp_path, monkeypatch):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    _forbid_tiled(monkeypatch)
    c = _train_cfg(tmp_path / 'train')
    t = SegTrainer(c)
    score = t.validate(c, t.val_loader)
    assert torch.isfinite(score) and 'inference' not in t.val_history[-1]
    p = _predict_cfg(tmp_path / 'predict')
    SegTrainer(p).predict(p)
    assert os.path.isfile(os.path.join(p.save_dir, 'frame.png'))


def test_validate_with_windows_on_the_cpu(tmp_path):
    from medical_segmentation_pytorch_amd.core import SegTrainer, seg_trainer
    c = _train_cfg(tmp_path, size=80, infer_window=48, tta_flips='h', infer_batch=5, metrics=['dice', 'hd95'])
    t = SegTrainer(c)
    calls = []
    real = seg_trainer.sliding_window_inference

    def spy(images, predictor, **kw):
        calls.append((tuple(images.shape), kw))
        return real(images, predictor, **kw)
    seg_trainer.sliding_window_inference = spy
    try:
        score = t.validate(c, t.val_loader)
        again = t.validate(c, t.val_loader)
    finally:
        seg_trainer.sliding_window_inference = real
    assert calls and calls[0][0][2:] == (80, 80) and calls[0][1]['window'] == (48, 48) and calls[0][1]['flips'] == 'h'
    assert torch.isfinite(score) and torch.equal(score, again)
    rec = t.val_history[-1]
    assert rec['inference'] == {'window': [48, 48], 'overlap': 0.5, 'blend': 'gaussian', 'sigma_scale': 0.125,
                                'flips': 'h', 'average': 'logits', 'batch': 5}
    json.dumps(rec)


def test_tta_alone_uses_the_whole_image_as_window(tmp_path):
    from medical_segmentation_pytorch_amd.core import SegTrainer, seg_trainer
    c = _train_cfg(tmp_path, tta_flips='hv', tta_average='probs')
    t = SegTrainer(c)
    calls = []
    real = seg_trainer.sliding_window_inference

    def spy(images, predictor, **kw):
        calls.append(kw)
        return real(images, predictor, **kw)
    seg_trainer.sliding_window_inference = spy
    try:
        assert torch.isfinite(t.validate(c, t.val_loader))
    finally:
        seg_trainer.sliding_window_inference = real
    assert calls and tuple(calls[0]['window']) == (64, 64) and t.val_history[-1]['inference']['window'] is None


def test_predict_with_windows_writes_native_size_masks(tmp_path):
    from PIL import Image
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = _predict_cfg(tmp_path, shape=(72, 100), infer_window=(48, 64), tta_flips='v', infer_batch=3)
    t = SegTrainer(c)
    t.predict(c)
    saved = Image.open(os.path.join(c.save_dir, 'frame.png'))
    assert saved.size == (100, 72)
    # the saved colours are those of the blended logits
    fwd = t.model.eval()
    with torch.no_grad():
        for _, images_aug, _names in t.test_loader:
            want = T.sliding_window_inference(images_aug.float(), lambda x: fwd(x).float(), (48, 64), flips='v',
                                              batch=7)
    labels = want.argmax(1)[0] if want.shape[1] > 1 else (want[0, 0] > 0).long()
    rgb = torch.from_numpy(np.asarray(saved.convert('RGB')).copy())
    assert torch.equal(rgb.long(), t.colormap.cpu()[labels].long())


def test_app_predictor_takes_the_same_route(tmp_path):
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from app import PolyPredictorApp
    from medical_segmentation_pytorch_amd.models import DuckNet
    torch.manual_seed(9)
    torch.save({'state_dict': DuckNet(2, 3, 4).state_dict()}, tmp_path / 'ck.pth')
    kw = dict(model='ducknet', base_channel=4, size=96, device=torch.device('cpu'))
    plain = PolyPredictorApp(str(tmp_path / 'ck.pth'), **kw)
    tiled = PolyPredictorApp(str(tmp_path / 'ck.pth'), inference={'infer_window': [64], 'tta_flips': 'hv',
                                                                  'infer_batch': 3, 'infer_overlap': None}, **kw)
    assert plain.tiled is None and tiled.tiled['window'] == (64, 64) and tiled.tiled['overlap'] == 0.5
    img = Image.fromarray((np.random.RandomState(1).rand(50, 70, 3) * 255).astype(np.uint8))
    x = tiled.preprocess_image(img)
    mask = tiled.predict(x)
    assert mask.shape == (96, 96) and mask.dtype == np.uint8
    with torch.no_grad():
        want = T.sliding_window_inference(x, lambda t: tiled.model(t).float(), 64, flips='hv', batch=16)
    assert np.array_equal(mask, want.argmax(1)[0].numpy().astype(np.uint8))
    assert plain.predict(x).shape == (96, 96)
    with pytest.raises(ValueError):
        PolyPredictorApp(str(tmp_path / 'ck.pth'), inference={'infer_overlap': 0.9}, **kw)
    with pytest.raises(ValueError):
        PolyPredictorApp(str(tmp_path / 'ck.pth'), inference={'window': 64}, **kw)
