"""Fused softmax-head Dice / Tversky / focal losses (``csrc/loss.hip`` region_*) on the MI355X: against the
plain-torch ``RegionLoss`` in fp64, at every kernel path (C = 2, 3, 4 registers / generic, 4-pixel vector /
scalar), with ignored and out-of-range labels; determinism, hipGraph replay and the trainer."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

TYPES = {'dice': (None, 'dice'), 'tversky': (None, 'tversky'), 'focal': ('focal', None), 'ce_dice': ('ce', 'dice'),
         'ce_tversky': ('ce', 'tversky'), 'focal_dice': ('focal', 'dice'), 'focal_tversky': ('focal', 'tversky')}
SHAPES = [(3, 2, 20, 24), (3, 3, 20, 24), (2, 4, 7, 9), (2, 5, 72, 72), (1, 64, 8, 8)]
KW = dict(pixel_weight=0.7, region_weight=1.3, smooth=0.5, alpha=0.4, beta=0.6)
LOSS_BAR = GRAD_BAR = 1e-4


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _weights(c):
    return 0.5 + torch.arange(c, dtype=torch.float32) % 3 * 0.75   # 0.5, 1.25, 2.0, 0.5, ...


def _case(shape, scale=1.0):
    """Logits, labels with two ignored rows, a fully ignored sample (N >= 3), one class absent from sample 0,
    one label == C and one == -1."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g) * scale
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0][t[0] == c - 1] = 0          # class C-1 absent from sample 0
    t[0, 1], t[n - 1, h - 1] = 255, 255
    if n >= 3:
        t[1] = 255
    t[0, 0, 0], t[0, 0, 1] = c, -1
    if scale != 1.0:
        x[0, :, 2, 2] = -80.0
        x[0, 0, 2, 2] = 80.0
        t[0, 2, 2] = 1               # the saturated pixel is wrong: p_t underflows
        x[0, :, 2, 3] = -80.0
        x[0, 0, 2, 3] = 80.0
        t[0, 2, 3] = 0               # and one saturated pixel that is right: 1 - p_t = 0
    return x, t


def _oracle(x, t, lt, gamma, ignore_bg, weight=True):
    """The plain-torch module in fp64 on the CPU, upstream gradient 0.5."""
    from medical_segmentation_pytorch_amd.core.loss import RegionLoss
    pixel, region = TYPES[lt]
    xr = x.double().requires_grad_(True)
    fn = RegionLoss(pixel, region, 255, _weights(x.shape[1]) if weight else None, gamma=gamma,
                    ignore_background=ignore_bg, **KW)
    loss = fn(xr, t)
    (loss * 0.5).backward()
    return loss.item(), xr.grad


def _fused(x, t, lt, gamma, ignore_bg, gpu, weight=True):
    from medical_segmentation_pytorch_amd.ops.losses import region_loss
    pixel, region = TYPES[lt]
    xg = x.to(gpu).requires_grad_(True)
    loss = region_loss(xg, t.to(gpu), _weights(x.shape[1]).to(gpu) if weight else None, 255, pixel, region,
                       gamma=gamma, ignore_background=ignore_bg, **KW)
    (loss * 0.5).backward()
    return loss, xg.grad


def _check(x, t, lt, gamma, ignore_bg, gpu, weight=True):
    ref, gref = _oracle(x, t, lt, gamma, ignore_bg, weight)
    loss, grad = _fused(x, t, lt, gamma, ignore_bg, gpu, weight)
    err_l, err_g = abs(loss.item() - ref), _rel(grad.cpu(), gref)
    print(f'{lt} {tuple(x.shape)} gamma={gamma}: loss {loss.item():.7f} ref {ref:.7f} |d| {err_l:.2e}; '
          f'grad rel L2 {err_g:.2e}')
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    assert err_l <= LOSS_BAR, (err_l, loss.item(), ref)
    assert err_g <= GRAD_BAR, err_g
    invalid = ((t == 255) | (t < 0) | (t >= x.shape[1])).unsqueeze(1).expand_as(x)
    assert torch.count_nonzero(grad.cpu()[invalid]) == 0   # ignored pixels: exact zeros
    return loss, grad


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('lt', sorted(TYPES))
def test_fused_matches_fp64_oracle(gpu, lt, shape):
    x, t = _case(shape)
    _check(x, t, lt, 2.0, False, gpu)


# the paths the table above leaves out: C = 4 vector, C = 2 / 3 scalar, and several blocks and loop
# iterations per sample on the vector (72 x 72) and the scalar (71 x 71) register paths
EXTRA = [(2, 4, 8, 12), (2, 2, 7, 9), (2, 3, 5, 7), (2, 3, 72, 72), (2, 4, 72, 72), (2, 2, 71, 71)]


@pytest.mark.parametrize('shape', EXTRA, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('lt', ['ce_dice', 'focal_tversky'])
def test_remaining_kernel_paths(gpu, lt, shape):
    x, t = _case(shape)
    _check(x, t, lt, 2.0, False, gpu)


@pytest.mark.parametrize('shape', [(3, 2, 20, 24), (2, 5, 72, 72)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('gamma', [1.0, 1.5, 0.0])
def test_gamma_paths_background_and_no_weights(gpu, gamma, shape):
    """The general-gamma branch, gamma == 1, gamma == 0 (CE), dice_ignore_background and weight=None."""
    x, t = _case(shape)
    _check(x, t, 'focal_tversky', gamma, True, gpu, weight=False)


def test_generic_path_uses_several_splits(gpu):
    from medical_segmentation_pytorch_amd.ops._ext import require
    assert require().region_splits(72 * 72) >= 2
    assert require().region_splits(7 * 9) == 1


@pytest.mark.parametrize('shape', SHAPES[:4], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('lt', ['ce_dice', 'focal_tversky', 'focal'])
def test_large_logits(gpu, lt, shape):
    x, t = _case(shape, scale=30.0)
    _check(x, t, lt, 2.0, False, gpu)


def test_class_cap(gpu):
    from medical_segmentation_pytorch_amd.ops._ext import require
    from medical_segmentation_pytorch_amd.ops.losses import region_loss
    assert require().region_max_classes() == 64
    x = torch.randn(1, 65, 4, 4, device=gpu)
    t = torch.randint(0, 65, (1, 4, 4), device=gpu)
    with pytest.raises(RuntimeError, match='64'):
        region_loss(x, t)


def test_module_takes_fused_path(gpu):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core.loss import RegionLoss, get_loss_fn
    c = MyConfig().init_dependent_config()
    c.loss_type, c.class_weights = 'focal_tversky', [1.0, 3.0]
    fn = get_loss_fn(c, gpu).to(gpu)
    assert isinstance(fn, RegionLoss)
    x, t = _case((3, 2, 20, 24))
    xg = x.to(gpu).requires_grad_(True)
    loss = fn(xg, t.to(gpu))
    assert '_Region' in type(loss.grad_fn).__name__
    loss.backward()
    xr = x.double().requires_grad_(True)
    ref = fn.cpu()(xr, t)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_BAR and _rel(xg.grad.cpu(), xr.grad) <= GRAD_BAR


@pytest.mark.parametrize('shape', [(3, 2, 20, 24), (2, 4, 7, 9), (2, 5, 72, 72)], ids=lambda s: 'x'.join(map(str, s)))
def test_bitwise_repeatable(gpu, shape):
    x, t = _case(shape)
    l1, g1 = _fused(x, t, 'focal_tversky', 2.0, False, gpu)
    l2, g2 = _fused(x, t, 'focal_tversky', 2.0, False, gpu)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


@pytest.mark.parametrize('lt', ['ce_dice', 'focal_tversky'])
def test_region_loss_in_captured_graph(gpu, lt):
    """Forward + backward inside a hipGraph: a replay on refreshed inputs is bitwise the eager result."""
    from medical_segmentation_pytorch_amd.ops.losses import region_loss
    pixel, region = TYPES[lt]
    wt = _weights(2).to(gpu)

    def run(x, tgt):
        return region_loss(x, tgt, wt, 255, pixel, region, **KW)

    torch.manual_seed(3)
    x = torch.randn(2, 2, 32, 32, device=gpu, requires_grad=True)
    tgt = torch.randint(0, 2, (2, 32, 32), device=gpu)
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


@pytest.mark.parametrize('lt,accum', [('ce_dice', 1), ('focal_tversky', 1), ('ce_dice', 2)])
def test_trainer_graph_with_region_loss(gpu, tmp_path, lt, accum):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.core.loss import RegionLoss
    c = _cfg(tmp_path, engine='fused', loss_type=lt, accum_steps=accum)
    t = SegTrainer(c)
    assert isinstance(t.loss_fn, RegionLoss)
    t.run(c)
    assert t.engine is not None and t.engine.graph is not None
    assert torch.isfinite(torch.tensor(t.last_loss))
    assert os.path.isfile(os.path.join(c.save_dir, 'last.pth'))
