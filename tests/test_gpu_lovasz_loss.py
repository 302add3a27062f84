"""Fused Lovasz-softmax loss (``csrc/lovasz.hip`` on the sort of ``csrc/sort.hip``) on the MI355X against the
plain-torch ``LovaszSoftmaxLoss`` in fp64 on the CPU: loss and gradient on inputs with separated errors, loss on
random and saturated logits, determinism, hipGraph replay, the module and the trainer.

Gradients are compared on *separated* inputs only: the sorted order decides which coefficient a pixel gets, and two
errors closer than fp32 rounding may legitimately swap between the device and the fp64 oracle.  The inputs put the
softmax on a lattice (:func:`_separated`), and every test asserts a minimum gap of 1e-5 between the fp64 errors of
the logits it passes.  For ``C >= 3`` the lattice is ``p_j = (k + 0.25 + 0.1 j) / D`` with ``D = C P`` wherever the
first ``C - 1`` classes then leave a positive remainder for the last one; at ``(1, 64, 8, 8)`` they do not
(``sum_j 0.1 j`` alone is 195 of 4096), so ``D`` grows by ``ceil(0.05 (C - 1) (C - 2))`` there.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_BAR = GRAD_BAR = 1e-4
MIN_GAP = 1e-5
SHAPES = [(3, 2, 20, 24), (2, 3, 7, 9), (2, 2, 72, 72), (2, 3, 72, 72), (2, 5, 40, 40), (1, 64, 8, 8)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _labels(shape, g):
    """Two ignored rows, a fully ignored image (N >= 3), one class absent from image 0, one label == C, one == -1."""
    n, c, h, w = shape
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0][t[0] == c - 1] = 0
    t[0, 1], t[n - 1, h - 1] = 255, 255
    if n >= 3:
        t[1] = 255
    t[0, 0, 0], t[0, 0, 1] = c, -1
    return t


def _separated(shape, seed=0):
    n, c, h, w = shape
    P = n * h * w
    g = torch.Generator().manual_seed(seed + sum(shape))
    k = torch.randperm(P, generator=g).double()
    if c == 2:
        p1 = (k + 0.25) / P
        p = torch.stack([1 - p1, p1], 1)
    else:
        D = c * P
        if (c - 1) * (P - 0.75) + 0.05 * (c - 1) * (c - 2) >= D:     # the last class would get p <= 0
            D += math.ceil(0.05 * (c - 1) * (c - 2))
        cols = [(k + 0.25 + 0.1 * j) / D for j in range(c - 1)]
        p = torch.stack(cols + [1 - sum(cols)], 1)
    assert p.min() > 0
    x = p.log().float().reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    return x, _labels(shape, g)


def _random(shape, scale=1.0):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g) * scale
    t = _labels(shape, g)
    if scale != 1.0:
        x[0, :, 2, 2] = -80.0
        x[0, 0, 2, 2] = 80.0
        t[0, 2, 2] = 1               # saturated and wrong: e = 1
        x[0, :, 2, 3] = -80.0
        x[0, 0, 2, 3] = 80.0
        t[0, 2, 3] = 0               # saturated and right: e = 0
    return x, t


def _min_gap(x, t):
    """Smallest distance between two fp64 errors of one class over the valid pixels of the batch (every image's
    errors are a subset, so the bound holds per image as well)."""
    c = x.shape[1]
    valid = (t != 255) & (t >= 0) & (t < c)
    p = torch.softmax(x.double(), 1)
    gap = float('inf')
    for k in range(c):
        e = ((t == k).double() - p[:, k]).abs()[valid]
        gap = min(gap, e.sort()[0].diff().min().item())
    return gap


_ORACLE = {}


def _oracle(key, x, t, per_image, ignore_bg):
    """The plain-torch module in fp64 on the CPU, upstream gradient 0.5; computed once per case."""
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    key = key + (per_image, ignore_bg)
    if key not in _ORACLE:
        xr = x.double().requires_grad_(True)
        loss = LovaszSoftmaxLoss(per_image=per_image, ignore_background=ignore_bg)(xr, t)
        (loss * 0.5).backward()
        _ORACLE[key] = (loss.item(), xr.grad)
    return _ORACLE[key]


def _fused(x, t, per_image, ignore_bg, gpu):
    from medical_segmentation_pytorch_amd.ops.losses import lovasz_softmax
    xg = x.to(gpu).requires_grad_(True)
    loss = lovasz_softmax(xg, t.to(gpu), 255, per_image, ignore_bg)
    (loss * 0.5).backward()
    return loss, xg.grad


def _check(key, x, t, per_image, ignore_bg, gpu, grad_bar=True):
    ref, gref = _oracle(key, x, t, per_image, ignore_bg)
    loss, grad = _fused(x, t, per_image, ignore_bg, gpu)
    err_l, err_g = abs(loss.item() - ref), _rel(grad.cpu(), gref)
    print(f'lovasz {key} per_image={per_image} ignore_bg={ignore_bg}: loss {loss.item():.7f} ref {ref:.7f} '
          f'|d| {err_l:.2e}; grad rel L2 {err_g:.2e}')
    assert loss.dtype == torch.float32 and torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    assert err_l <= LOSS_BAR, (err_l, loss.item(), ref)
    if grad_bar:
        assert err_g <= GRAD_BAR, err_g
    invalid = ((t == 255) | (t < 0) | (t >= x.shape[1])).unsqueeze(1).expand_as(x)
    assert torch.count_nonzero(grad.cpu()[invalid]) == 0   # ignored pixels: exact zeros
    return loss, grad


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_fused_matches_fp64_oracle(gpu, shape, per_image):
    x, t = _separated(shape)
    gap = _min_gap(x, t)
    print(f'{shape}: minimum gap {gap:.2e}')
    assert gap >= MIN_GAP, gap
    _check(('sep', shape), x, t, per_image, False, gpu)


@pytest.mark.parametrize('per_image', [False, True])
def test_ignore_background(gpu, per_image):
    x, t = _separated((2, 3, 72, 72))
    assert _min_gap(x, t) >= MIN_GAP
    _check(('sep', (2, 3, 72, 72)), x, t, per_image, True, gpu)


@pytest.mark.parametrize('scale', [1.0, 30.0])
@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_loss_on_random_and_saturated_logits(gpu, shape, per_image, scale):
    """The loss is continuous in the errors, so a swap of two near-equal ones does not move it."""
    x, t = _random(shape, scale)
    _check(('rnd', shape, scale), x, t, per_image, False, gpu, grad_bar=False)


def test_empty_cases(gpu):
    from medical_segmentation_pytorch_amd.ops.losses import lovasz_softmax
    for per_image in (False, True):
        x = torch.randn(2, 3, 9, 9, device=gpu, requires_grad=True)
        t = torch.full((2, 9, 9), 255, device=gpu)
        t[0, 0, 0], t[1, 1, 1] = 3, -1
        loss = lovasz_softmax(x, t, 255, per_image)
        loss.backward()
        assert loss.item() == 0.0 and torch.count_nonzero(x.grad) == 0
        x.grad = None
        loss = lovasz_softmax(x, torch.zeros_like(t), 255, per_image, True)   # only class 0, ignored as background
        loss.backward()
        assert loss.item() == 0.0 and torch.count_nonzero(x.grad) == 0


def test_class_chunks(gpu, monkeypatch):
    """Classes sorted one or two at a time give the bits of the single-chunk run."""
    from medical_segmentation_pytorch_amd.ops import losses
    x, t = _random((2, 5, 40, 40))
    for per_image in (False, True):
        l0, g0 = _fused(x, t, per_image, False, gpu)
        for ck in (1, 2):
            monkeypatch.setattr(losses, 'lovasz_chunk_classes', lambda n, c, hw, pi, ck=ck: ck)
            l1, g1 = _fused(x, t, per_image, False, gpu)
            monkeypatch.undo()
            assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert losses.lovasz_chunk_classes(2, 5, 1600, False) == 5
    assert losses.lovasz_chunk_classes(320, 4, 352 * 352, False) == 3
    assert losses.lovasz_chunk_classes(60000, 64, 4, True) == 1


@pytest.mark.parametrize('shape', [(3, 2, 20, 24), (2, 3, 72, 72)], ids=lambda s: 'x'.join(map(str, s)))
def test_bitwise_repeatable(gpu, shape):
    x, t = _random(shape)
    for per_image in (False, True):
        l1, g1 = _fused(x, t, per_image, False, gpu)
        l2, g2 = _fused(x, t, per_image, False, gpu)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_loss_in_captured_graph(gpu, per_image):
    """Forward + backward inside a hipGraph: a replay on refreshed inputs is bitwise the eager result."""
    from medical_segmentation_pytorch_amd.ops.losses import lovasz_softmax

    def run(x, tgt):
        return lovasz_softmax(x, tgt, 255, per_image)

    torch.manual_seed(3)
    x = torch.randn(2, 2, 72, 72, device=gpu, requires_grad=True)
    tgt = torch.randint(0, 2, (2, 72, 72), device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm-up outside the capture
        run(x, tgt).backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(g):
        out = run(x, tgt)
        out.backward()
    for scale in (1.0, 0.05, 4.0):
        with torch.no_grad():
            x.copy_(torch.randn_like(x) * scale)
            tgt.copy_(torch.randint(0, 2, tgt.shape, device=gpu))
            tgt[0, 3] = 255
            x.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        xe = x.detach().clone().requires_grad_(True)
        eager = run(xe, tgt)
        eager.backward()
        assert torch.equal(out.detach(), eager.detach()), (scale, out.item(), eager.item())
        assert torch.equal(x.grad, xe.grad)


def test_module_takes_fused_path(gpu):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss, get_loss_fn
    c = MyConfig().init_dependent_config()
    c.loss_type, c.class_weights, c.loss_region_weight = 'ce_lovasz_softmax', [1.0, 3.0], 0.8
    fn = get_loss_fn(c, gpu).to(gpu)
    assert isinstance(fn, LovaszSoftmaxLoss)
    x, t = _separated((3, 2, 20, 24))
    xg = x.to(gpu).requires_grad_(True)
    term = fn.lovasz_term(xg, t.to(gpu))
    assert '_Lovasz' in type(term.grad_fn).__name__
    loss = fn(xg, t.to(gpu))
    loss.backward()
    xr = x.double().requires_grad_(True)
    ref = fn.cpu()(xr, t)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_BAR and _rel(xg.grad.cpu(), xr.grad) <= GRAD_BAR


def test_class_cap_and_shapes(gpu):
    from medical_segmentation_pytorch_amd.ops._ext import require
    from medical_segmentation_pytorch_amd.ops.losses import lovasz_softmax
    assert require().lovasz_max_classes() == 64
    x = torch.randn(1, 65, 4, 4, device=gpu)
    t = torch.randint(0, 65, (1, 4, 4), device=gpu)
    with pytest.raises(RuntimeError, match='64'):
        lovasz_softmax(x, t)
    with pytest.raises(ValueError, match='num_class'):
        lovasz_softmax(x[:, :1], t)
    with pytest.raises(ValueError, match='target'):
        lovasz_softmax(x[:, :3], t[:, :2])


def _cfg(tmp, **kw):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp / 'data'), str(tmp / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (16, 4, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 2, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.log_interval = 3, 1, False, 3
    c.graph_warmup = 2
    for k, v in kw.items():
        setattr(c, k, v)
    return c.init_dependent_config()


@pytest.mark.parametrize('lt', ['lovasz_softmax', 'ce_lovasz_softmax'])
def test_trainer_graph_with_lovasz_loss(gpu, tmp_path, lt):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    c = _cfg(tmp_path, engine='fused', loss_type=lt)
    t = SegTrainer(c)
    assert isinstance(t.loss_fn, LovaszSoftmaxLoss)
    t.run(c)
    assert t.engine is not None and t.engine.graph is not None
    assert torch.isfinite(torch.tensor(t.last_loss))
    assert os.path.isfile(os.path.join(c.save_dir, 'last.pth'))
