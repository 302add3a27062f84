"""Sliding-window inference on the MI355X kernels (``csrc/tiled.hip``) against the plain-torch specification
(``ops/tiled.py``) run in fp64 on the CPU.

Bounds (derived, not tuned): 'logits' mode ``|out - oracle| <= (2K + 3) * 2^-24 * max|logit|`` -- the fp32 bound of a
K-term weighted sum, a K-term normaliser and one division, K = the largest number of (window, view) terms on a pixel
of the case, from the geometry; 'probs' mode ``|softmax(out) - oracle p| <= 2e-5`` (sigmoid for C = 1), about 4x
``(C + 2K + 10) * 2^-24`` at the largest case (C = 19, K = 36).  The gather is a pure copy: ``torch.equal``."""
import functools
import math

import pytest
import torch

from medical_segmentation_pytorch_amd.ops import tiled as T

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# (H, W, wh, ww, overlap): clipped last window on both axes (36 terms with 'hv') | windows one pixel apart, non-square |
# step 8 | image smaller than the window in y | ten windows along x, the last 3 pixels after the ninth | odd extents,
# ww % 4 != 0, unaligned rows (scalar path) | exactly one window | abutting tiles
SHAPES = [(70, 93, 32, 32, .5), (33, 70, 32, 64, .25), (40, 40, 32, 32, .75), (20, 50, 32, 32, .5),
          (97, 131, 64, 32, .6), (17, 23, 5, 12, .5), (32, 32, 32, 32, .5), (64, 96, 32, 32, 0)]
CLASSES = (1, 2, 3, 4, 19)


def _cases():
    """A thinned cross-product: per shape every class count once, images / flips / blend / average rotating so that
    across the shapes every class count meets every flip setting, both blends and both averaging modes."""
    out = []
    for si, shape in enumerate(SHAPES):
        for j, c in enumerate(CLASSES):
            out.append((shape, (1, 3)[(si + j) % 2], c, T.FLIPS[(si + j) % 4], T.BLENDS[(si + j // 2) % 2],
                        T.AVERAGES[(si // 2 + j) % 2]))
    # the busiest pixels (K = 36) on the generic and on a register path, in both modes; W % 4 == 0 with 'hv'
    out += [(SHAPES[0], 1, 19, 'hv', 'gaussian', 'probs'), (SHAPES[0], 3, 19, 'hv', 'gaussian', 'logits'),
            (SHAPES[0], 3, 4, 'hv', 'gaussian', 'probs'), (SHAPES[0], 1, 3, 'hv', 'constant', 'logits'),
            (SHAPES[2], 3, 3, 'hv', 'gaussian', 'logits'), (SHAPES[4], 1, 4, 'hv', 'gaussian', 'logits'),
            (SHAPES[7], 1, 2, 'hv', 'gaussian', 'probs'), (SHAPES[3], 3, 1, 'hv', 'gaussian', 'probs')]
    return out


CASES = _cases()


def _id(case):
    (h, w, wh, ww, o), n, c, flips, blend, average = case
    return f'{h}x{w}-{wh}x{ww}-o{o}-N{n}-C{c}-{flips or "id"}-{blend}-{average}'


def _plan(case):
    (h, w, wh, ww, o), _, _, flips, blend, _ = case
    return T.tile_plan(h, w, (wh, ww), o, blend, .125, flips)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(fp32 window logits on the CPU, fp64 oracle of the blend): computed once per case and left unchanged"""
    _, n, c, _, _, average = case
    plan = _plan(case)
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    logits = 3 * torch.randn(plan.windows(n), c, plan.wh, plan.ww, generator=g)
    oracle = T.blend_windows(logits.double(), plan, n, average, native=False)
    return logits, oracle


def _max_terms(plan):
    """K from the geometry alone: the largest count of covering windows per axis, times the views"""
    def axis(starts, w, L, pad):
        return max(sum(1 for s in starts if s <= p < s + w) for p in range(pad, pad + L))
    return axis(plan.sy, plan.wh, plan.H, plan.py) * axis(plan.sx, plan.ww, plan.W, plan.px) * plan.V


def test_case_list_covers_the_grid():
    assert {c[2] for c in CASES} == set(CLASSES) and {c[1] for c in CASES} == {1, 3}
    for c in CLASSES:
        mine = [k for k in CASES if k[2] == c]
        assert {k[3] for k in mine} == set(T.FLIPS) and {k[4] for k in mine} == set(T.BLENDS)
        assert {k[5] for k in mine} == set(T.AVERAGES) and {k[0] for k in mine} == set(SHAPES)
    assert _max_terms(T.tile_plan(70, 93, 32, .5, flips='hv')) == 36


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_gather_is_the_specification_bitwise(gpu, shape):
    h, w, wh, ww, o = shape
    torch.manual_seed(3)
    img = torch.randn(3, 3, h, w) + 4.0          # no zeros in the image: a zero in a window is padding
    dev = img.to(gpu)
    for flips in T.FLIPS:
        plan = T.tile_plan(h, w, (wh, ww), o, flips=flips)
        m = plan.windows(3)
        want = T.gather_windows(img, plan, 0, m + 8, native=False)
        assert float(want[m:].abs().max()) == 0
        got = T.gather_windows(dev, plan, 0, m + 8)
        assert got.is_cuda and torch.equal(got.cpu(), want), flips
        for m0, count in ((0, 1), (m - 2, 5), (m // 2, 7), (m + 1, 2)):
            assert torch.equal(T.gather_windows(dev, plan, m0, count).cpu(), want[m0:m0 + count]), (flips, m0)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_blend_against_the_fp64_oracle(gpu, case):
    _, n, c, _, _, average = case
    plan = _plan(case)
    logits, oracle = _inputs(case)
    k = _max_terms(plan)
    assert k == plan.max_terms
    dev = logits.to(gpu)
    out = T.blend_windows(dev, plan, n, average)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == oracle.shape
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    if average == 'logits':
        bar = (2 * k + 3) * EPS * float(logits.abs().max())
        err = float((got - oracle).abs().max())
        print(f'{_id(case)}: K {k} max err {err:.3e} bar {bar:.3e}')
        assert err <= bar
    else:
        prob = (torch.sigmoid, torch.sigmoid) if c == 1 else (lambda t: torch.softmax(t, 1),) * 2
        err = float((prob[0](got) - prob[1](oracle)).abs().max())
        print(f'{_id(case)}: K {k} max prob err {err:.3e} bar 2e-5; (C + 2K + 10) eps = {(c + 2 * k + 10) * EPS:.3e}')
        assert err <= 2e-5
    # bitwise repeatable, and independent of how the windows were chunked
    assert torch.equal(T.blend_windows(dev, plan, n, average), out)
    for batch in (1, 5):
        assert torch.equal(T.blend_windows(dev, plan, n, average, batch=batch), out), batch


@pytest.mark.parametrize('case', [k for k in CASES if k[5] == 'logits'], ids=_id)
def test_labels_match_where_the_oracle_is_decided(gpu, case):
    _, n, c, _, _, average = case
    plan = _plan(case)
    logits, oracle = _inputs(case)
    out = T.blend_windows(logits.to(gpu), plan, n, average).cpu().double()
    bar = (2 * _max_terms(plan) + 3) * EPS * float(logits.abs().max())
    if c == 1:
        decided = oracle[:, 0].abs() > 2 * bar
        same = (out[:, 0] > 0) == (oracle[:, 0] > 0)
    else:
        top = oracle.topk(2, dim=1).values
        decided = (top[:, 0] - top[:, 1]) > 2 * bar
        same = out.argmax(1) == oracle.argmax(1)
    left_out = 1.0 - float(decided.double().mean())
    print(f'{_id(case)}: {left_out:.5%} of the pixels undecided in fp64')
    assert left_out <= 0.005
    assert bool(same[decided].all())


def _ducknet(gpu):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.models import get_model
    from medical_segmentation_pytorch_amd.utils import FusedModel
    c = MyConfig()
    c.model, c.base_channel, c.num_class, c.num_channel = 'ducknet', 17, 2, 3
    torch.manual_seed(21)
    return FusedModel(get_model(c).to(gpu)).eval()


def test_end_to_end_with_the_fused_executor(gpu):
    fwd = _ducknet(gpu)
    torch.manual_seed(22)
    images = torch.randn(2, 3, 96, 160, device=gpu)
    seen = []

    def predictor(x):
        y = fwd(x).float()
        seen.append(y.abs().max())
        return y
    with torch.no_grad():
        got = T.sliding_window_inference(images, predictor, 64, overlap=0.5, flips='hv', batch=16)
        n_dev = len(seen)
        want = T.sliding_window_inference(images, predictor, 64, overlap=0.5, flips='hv', batch=16, native=False)
    plan = T.tile_plan(96, 160, 64, .5, flips='hv')
    assert plan.windows(2) == 2 * 2 * 4 * 4 and n_dev == 4 and len(seen) == 8
    assert got.shape == (2, 2, 96, 160) and got.dtype == torch.float32 and want.is_cuda
    peak = float(torch.stack(seen).max())
    bar = (2 * _max_terms(plan) + 3) * EPS * peak
    err = float((got - want).abs().max())
    print(f'DUCKNet-17 windows: K {_max_terms(plan)} max|logit| {peak:.3f} max err {err:.3e} bar {bar:.3e}')
    assert bool(torch.isfinite(got).all()) and err <= bar
    assert float(got.std()) > 0


def test_trainer_validate_with_windows_and_tta(gpu, tmp_path):
    from medical_segmentation_pytorch_amd.configs import MyConfig, load_parser
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 6, 4), 96
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 4, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 1, 0, False, False
    c.engine, c.metrics = 'fused', ['dice', 'hd95']
    c = load_parser(c, ['--infer_window', '64', '--tta_flips', 'hv'])
    t = SegTrainer(c)
    assert t.fused
    t.validate(c, t.val_loader)
    first = {k: v.clone() for k, v in t.last_scores.items()}
    assert t.val_history[-1]['inference']['window'] == [64, 64] and t.val_history[-1]['inference']['flips'] == 'hv'
    for name in ('dice', 'hd95'):
        assert bool(torch.isfinite(first[name]).all()), (name, first[name])
    assert math.isfinite(t.val_history[-1]['score'])
    t.validate(c, t.val_loader)
    for name in ('dice', 'hd95'):
        assert torch.equal(t.last_scores[name], first[name]), name


def test_resume_on_the_device_restores_the_host_rng(gpu, tmp_path):
    """``accuracy_main.py --eval-only`` resumes from ``last.pth``; the checkpoint is mapped to the device, the numpy
    RNG keys in it included."""
    import numpy as np
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core import SegTrainer

    def cfg():
        c = MyConfig()
        c.model, c.base_channel, c.engine = 'unet', 8, 'eager'
        c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
        c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 4, 4), 64
        c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 4, 0
        c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set, c.use_tb = 1, 0, False, False, False
        c.init_dependent_config()
        return c
    c = cfg()
    SegTrainer(c).run(c)
    saved = torch.load(c.load_ckpt_path, map_location='cpu', weights_only=True)['rng']['numpy']
    np.random.seed(12345)
    t = SegTrainer(cfg())
    assert t.device.type == 'cuda' and t.cur_epoch == 1
    state = np.random.get_state()
    assert np.array_equal(state[1], saved[0].numpy().astype(np.uint32)) and state[2] == saved[1]
