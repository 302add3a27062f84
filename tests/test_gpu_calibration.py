"""Calibration statistics, the temperature grid and uncertainty maps on the MI355X kernels (``csrc/calibration.hip``)
against the plain-torch specification evaluated in fp64 on the CPU.

The inputs are edge-separated: every pixel's distribution is built directly, with its top probability ``(b + u) / M``,
``u`` in [0.1, 0.9], inside ``[1 / C + 0.05, 0.999]`` and the remainder split within 2 % of evenly, and the logits are
``T log p``.  Every test asserts on the fp64 oracle that ``conf * M`` stays 0.05 away from an integer, that the top two
probabilities are 1e-3 apart and that ``|z| <= 32``, so an fp32 evaluation lands in the same bin with the same argmax
and the integer tables must agree bit for bit.  The floating sums and the four metrics have the 1e-4 relative bar of
the region and Lovasz loss tests; labels hit the top class with probability 0.3 and are uniform otherwise, which keeps
the oracle ECE far above the asserted 0.02."""
import functools
import math
import os

import pytest
import torch

from medical_segmentation_pytorch_amd.ops import calibration as K
from medical_segmentation_pytorch_amd.utils import metrics as M

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 20, 24), (3, 3, 7, 9), (2, 2, 72, 72), (2, 5, 40, 40), (1, 64, 8, 8)]
BINS = [1, 15, 64]
TEMPS = [0.5, 1.0, 2.5]
IGNORE = 255
RTOL = 1e-4
NAMES = ('ece', 'mce', 'nll', 'brier')


@functools.lru_cache(maxsize=None)
def _case(shape, bins, T):
    """(fp32 logits, labels, fp64 CPU oracle state) for edge-separated distributions; no pixel is left out"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * bins + int(10 * T) + c)
    P = n * h * w
    lo, hi = 1.0 / c + 0.05, 0.999
    top = torch.empty(P, dtype=torch.float64)
    todo = torch.ones(P, dtype=torch.bool)
    for _ in range(200):          # (b + u) / M with u in [0.1, 0.9], redrawn until it lies in [lo, hi]
        k = int(todo.sum())
        if k == 0:
            break
        b = torch.randint(0, bins, (k,), generator=g).double()
        u = 0.1 + 0.8 * torch.rand(k, generator=g, dtype=torch.float64)
        cand = (b + u) / bins
        ok = (cand >= lo) & (cand <= hi)
        idx = todo.nonzero()[:, 0]
        top[idx[ok]] = cand[ok]
        todo[idx[ok]] = False
    assert not bool(todo.any())
    rest = 1.0 + 0.02 * (2 * torch.rand(P, c - 1, generator=g, dtype=torch.float64) - 1)
    rest = rest / rest.sum(1, keepdim=True) * (1.0 - top)[:, None]
    assert bool(((rest * (c - 1) / (1.0 - top)[:, None] - 1).abs() <= 0.0405).all())
    cls = torch.randint(0, c, (P,), generator=g)                 # the top class
    p = torch.empty(P, c, dtype=torch.float64)
    others = torch.arange(c)[None, :].expand(P, c)
    others = others[others != cls[:, None]].view(P, c - 1)
    p.scatter_(1, others, rest)
    p.scatter_(1, cls[:, None], top[:, None])
    z = (T * p.log()).view(n, h, w, c).permute(0, 3, 1, 2).contiguous().float()
    hit = torch.rand(P, generator=g) < 0.3
    t = torch.where(hit, cls, torch.randint(0, c, (P,), generator=g)).view(n, h, w)
    t[0, 0, 0], t[0, -1, -1], t[0, h // 2, w // 2] = IGNORE, c, -1
    if shape == (3, 3, 7, 9):
        t[1] = IGNORE                                            # a fully ignored image
    # the separation, on the fp64 oracle's own view of the fp32 logits
    z64 = z.double()
    pr = torch.softmax(z64 / T, 1)
    two = pr.topk(2, 1).values
    conf = two[:, 0]
    frac = conf * bins - (conf * bins).floor()
    assert float(torch.minimum(frac, 1 - frac).min()) >= 0.05
    assert float((two[:, 0] - two[:, 1]).min()) >= 1e-3 and float(z.abs().max()) <= 32
    st = K.calibration_stats(z64, t, None, T, IGNORE, bins, native=False)
    return z, t, st


def _close(got, want, what):
    got, want = float(got), float(want)
    print(f'{what}: {got!r} oracle {want!r} rel {abs(got - want) / max(abs(want), 1e-300):.2e}')
    assert abs(got - want) <= RTOL * abs(want)


@pytest.mark.parametrize('T', TEMPS)
@pytest.mark.parametrize('bins', BINS)
@pytest.mark.parametrize('shape', SHAPES)
def test_stats_match_oracle(gpu, shape, bins, T):
    z, t, want = _case(shape, bins, T)
    got = K.calibration_stats(z.to(gpu), t.to(gpu), None, T, IGNORE, bins)
    assert got['ints'].is_cuda and got['ints'].dtype == torch.long and got['sums'].dtype == torch.float64
    assert torch.equal(got['count'].cpu(), want['count']) and torch.equal(got['correct'].cpu(), want['correct'])
    assert int(want['count'].sum()) == int((t != IGNORE).sum()) - 2
    for b in range(bins):
        if int(want['count'][b]):
            _close(got['conf_sum'][b], want['conf_sum'][b], f'conf_sum[{b}]')
        else:
            assert float(got['conf_sum'][b]) == 0.0
    _close(got['nll_sum'], want['nll_sum'], 'nll_sum')
    _close(got['brier_sum'], want['brier_sum'], 'brier_sum')
    wv = K.metrics_from_state(want['ints'], want['sums'])
    assert float(wv[0]) >= 0.02
    gv = K.metrics_from_state(got['ints'], got['sums'])
    for name, a, b in zip(NAMES, gv, wv):
        _close(a, b, name)


@pytest.mark.parametrize('k', [1, 33, 64])
@pytest.mark.parametrize('shape', SHAPES)
def test_nll_grid_matches_oracle(gpu, shape, k):
    z, t, _ = _case(shape, 15, 1.0)
    betas = torch.tensor([1.0]) if k == 1 else torch.tensor(
        [2.0 ** (-3 + 6 * i / (k - 1)) for i in range(k)], dtype=torch.float64).float()
    want = K.nll_grid(z.double(), t, betas, IGNORE, native=False)
    got = K.nll_grid(z.to(gpu), t.to(gpu), betas, IGNORE)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (k,)
    for i in range(k):
        _close(got[i], want[i], f'S[{i}] beta {float(betas[i]):.4g}')
    if k == 33:      # beta = 1 is the NLL sum of the statistics kernel's oracle
        _close(got[16], _case(shape, 15, 1.0)[2]['nll_sum'], 'S[16] against nll_sum')


def _nll_at(z64, t, log2_t):
    return float(K.nll_grid(z64, t, [2.0 ** -log2_t], IGNORE, native=False)[0])


def _golden_section_log2_t(z64, t, lo=-3.0, hi=3.0, iters=80):
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


@pytest.mark.parametrize('t0', TEMPS)
def test_device_fit_against_golden_section(gpu, t0):
    g = torch.Generator().manual_seed(int(10 * t0))
    n, c, h, w = 2, 3, 40, 40
    base = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2
    labels = torch.multinomial(torch.softmax(base, 1).permute(0, 2, 3, 1).reshape(-1, c), 1, generator=g).view(n, h, w)
    labels[0, 0, :5] = IGNORE
    z = (t0 * base).float()
    batches = [(z[:1].to(gpu), labels[:1].to(gpu)), (z[1:].to(gpu), labels[1:].to(gpu))]
    T = K.fit_temperature(batches, IGNORE, 2)
    star = _golden_section_log2_t(z.double(), labels)
    step = 6 / 32 * 2 / 32
    print(f'T0 {t0}: T_fit {T!r} T* {2 ** star!r} |log2| {abs(math.log2(T) - star):.5f} step {step:.5f}')
    assert abs(math.log2(T) - star) <= step
    assert _nll_at(z.double(), labels, math.log2(T)) <= _nll_at(z.double(), labels, 0.0)


def test_repeated_calls_give_the_same_bits(gpu):
    z, t, _ = _case((2, 2, 72, 72), 15, 1.0)
    zg, tg = z.to(gpu), t.to(gpu)
    a, b = K.calibration_stats(zg, tg, None, 1.0, IGNORE, 15), K.calibration_stats(zg, tg, None, 1.0, IGNORE, 15)
    assert torch.equal(a['ints'], b['ints']) and torch.equal(a['sums'], b['sums'])
    betas = K._betas(K.first_exponents())
    assert torch.equal(K.nll_grid(zg, tg, betas, IGNORE), K.nll_grid(zg, tg, betas, IGNORE))
    for mode in K.MODES:
        assert torch.equal(K.uncertainty_map(zg, 1.0, mode), K.uncertainty_map(zg, 1.0, mode))


def test_two_batches_equal_one(gpu):
    z, t, want = _case((2, 2, 72, 72), 15, 2.5)
    zg, tg = z.to(gpu), t.to(gpu)
    one = K.calibration_stats(zg, tg, None, 2.5, IGNORE, 15)
    two = K.calibration_stats(zg[:1], tg[:1], None, 2.5, IGNORE, 15)
    K.calibration_stats(zg[1:], tg[1:], two, 2.5, IGNORE, 15)
    assert torch.equal(one['ints'], two['ints']) and torch.equal(one['ints'].cpu(), want['ints'])
    # fp64 sums of fp32 terms in another order: far inside the fp32 rounding of the terms
    assert torch.allclose(one['sums'], two['sums'], rtol=1e-10, atol=0)
    betas = [0.5, 1.0, 2.0]
    s1 = K.nll_grid(zg, tg, betas, IGNORE)
    s2 = K.nll_grid(zg[1:], tg[1:], betas, IGNORE, K.nll_grid(zg[:1], tg[:1], betas, IGNORE))
    assert torch.allclose(s1, s2, rtol=1e-10, atol=0)


def test_no_valid_pixel_leaves_the_state_zero(gpu):
    z, _, _ = _case((3, 3, 7, 9), 15, 1.0)
    t = torch.full((3, 7, 9), IGNORE)
    t[0, 0, 0], t[1, 1, 1] = 3, -1
    st = K.calibration_stats(z.to(gpu), t.to(gpu), None, 1.0, IGNORE, 15)
    assert int(st['ints'].abs().sum()) == 0 and float(st['sums'].abs().sum()) == 0
    assert all(math.isnan(float(v)) for v in K.metrics_from_state(st['ints'], st['sums']))
    assert float(K.nll_grid(z.to(gpu), t.to(gpu), [0.5, 1.0], IGNORE).abs().sum()) == 0
    assert K.fit_temperature([(z.to(gpu), t.to(gpu))], IGNORE) == 1.0


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('shape', [(2, 1, 9, 37), (2, 2, 5, 37), (1, 5, 6, 37), (2, 5, 8, 12), (1, 1, 4, 8)])
def test_uncertainty_map_within_one_level(gpu, shape, mode):
    """W = 37: image rows and planes that are no multiple of four pixels, and a store tail; (2, 5, 8, 12) and
    (1, 1, 4, 8) take the float4 loads."""
    g = torch.Generator().manual_seed(shape[1] + shape[3])
    z = torch.randn(*shape, generator=g) * 3
    for T in (0.5, 1.0, 2.5):
        want = K.uncertainty_map(z.double(), T, mode, native=False)
        got = K.uncertainty_map(z.to(gpu), T, mode)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == want.shape
        diff = (got.cpu().int() - want.int()).abs()
        print(f'{shape} {mode} T {T}: max level difference {int(diff.max())}, differing {int((diff > 0).sum())}')
        assert int(diff.max()) <= 1 and int(want.max()) - int(want.min()) > 32


def test_metrics_through_get_seg_metrics(gpu):
    from types import SimpleNamespace
    z, t, want = _case((2, 5, 40, 40), 15, 2.5)
    cfg = SimpleNamespace(num_class=5, ignore_index=IGNORE, calibration_bins=15)
    ms = [M.get_seg_metrics(cfg, n).to(gpu) for n in NAMES]
    acc = ms[0].acc
    assert all(m.acc is acc for m in ms) and acc.ints.is_cuda and acc.temperature.is_cuda
    acc.set_temperature(2.5)
    calls = []
    real = K.calibration_stats
    K.calibration_stats = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        zg, tg = z.to(gpu), t.to(gpu)
        for m in ms:
            m.update(zg, tg)
    finally:
        K.calibration_stats = real
    assert len(calls) == 1 and torch.equal(acc.ints.cpu(), want['ints'])
    for name, m, w in zip(NAMES, ms, K.metrics_from_state(want['ints'], want['sums'])):
        v = m.compute()
        assert v.is_cuda and v.dtype == torch.float32
        print(f'{name}: {float(v)!r} oracle {float(w)!r}')
        assert abs(float(v) - float(w)) <= RTOL * abs(float(w))
    rel = ms[0].reliability()
    assert torch.equal(rel['count'].cpu(), want['count'])
    ms[3].reset()
    assert int(acc.ints.sum()) == 0 and float(acc.temperature) == 2.5


def test_trainer_validate_and_calibrate_fused(gpu, tmp_path):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (8, 6, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 4, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.use_test_set = 1, 0, False, False
    c.engine, c.metrics, c.calibrate_temperature = 'fused', ['dice', 'ece', 'nll'], True
    c.init_dependent_config()
    t = SegTrainer(c)
    assert t.fused and t.metrics[1].acc is t.metrics[2].acc and t.temperature == 1.0
    seen = []
    acc = t.metrics[1].acc
    upd = acc.update
    acc.update = lambda p, m, **k: (seen.append((p.detach().cpu().clone(), m.cpu().clone())), upd(p, m, **k))[1]
    t.validate(c, t.val_loader)
    first = dict(t.val_history[-1])
    assert len(seen) == 4 and first['calibration']['temperature'] == 1.0          # 2 batches x 2 metrics
    logits, masks = torch.cat([p for p, _ in seen[::2]]), torch.cat([m for _, m in seen[::2]])
    assert logits.shape == (6, 2, 64, 64)
    want = K.calibration_stats(logits.double(), masks, None, 1.0, c.ignore_index, 15, native=False)
    v = int(want['count'].sum())
    assert sum(first['calibration']['count']) == v == 6 * 64 * 64
    ece, _, nll, _ = (float(x) for x in K.metrics_from_state(want['ints'], want['sums']))
    print(f'trainer nll {first["nll"]!r} oracle {nll!r}; ece {first["ece"]!r} oracle {ece!r}')
    assert abs(first['nll'] - nll) <= RTOL * nll
    # the network's confidences are not edge-separated: a pixel within fp32 rounding of a bin edge may change bins,
    # which moves the ECE by at most 1 / V; four such pixels are allowed
    assert abs(first['ece'] - ece) <= RTOL * ece + 4.0 / v
    t.save_ckpt(c, save_best=True)
    t.val_best(c, t.val_loader)
    before = dict(t.val_history[-1])
    T = t.calibrate(c, t.val_loader)
    after = t.val_history[-1]
    assert after['calibrated'] is True and after['calibration']['temperature'] == T == t.temperature
    assert 1 / 8 <= T <= 8 and before['dice'] == after['dice']
    assert after['nll'] <= before['nll'] * (1 + 1e-6)
    best = torch.load(os.path.join(c.save_dir, 'best.pth'), weights_only=True)
    assert best['temperature'] == T
    # the fit against the oracle's golden section on the logits the metrics saw
    last = seen[-4::2]                                           # the calibrated validation's two batches
    star = _golden_section_log2_t(torch.cat([p for p, _ in last]).double(), torch.cat([m for _, m in last]))
    print(f'T_fit {T!r} T* {2 ** star!r}')
    assert abs(math.log2(T) - star) <= 6 / 32 * 2 / 32
