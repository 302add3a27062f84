"""Boundary (signed-distance) loss on the MI355X: the fused signed distance map (``csrc/surface.hip`` sdf_*)
bitwise against the plain-torch specification, the fused loss (``csrc/loss.hip`` boundary_*) against the
plain-torch ``BoundaryLoss`` in fp64, determinism, hipGraph replay with an in-place weight change, the trainer."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_BAR = GRAD_BAR = 1e-4      # the bars of test_gpu_region_loss.py


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------ signed distance
def _sdf_labels(n, h, w, c):
    """Discs of the classes 1 .. c-2 on background (class c-1 is absent: a degenerate plane); image 0 carries an
    ignored stripe and the labels ``c`` and ``-1``; image 1 is one class wherever it is valid (a plane whose
    ``neg`` set is empty) with an ignored row; image 3 is ignored altogether."""
    g = torch.Generator().manual_seed(n * 7919 + h * 31 + w + c)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    t = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        for k in range(1, max(2, c - 1)):
            for _ in range(3):
                cy, cx = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
                r = int(torch.randint(0, max(1, min(max(h, w) // 6, 40)) + 1, (1,), generator=g))
                t[i][(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = k
    if w > 2:
        t[0, :, w // 2] = 255
    if h > 2:
        t[0, h // 2, :] = 255
    if h * w > 1:
        t[0, 0, 0], t[0, h - 1, w - 1] = c, -1
    if n > 1:
        t[1] = 1
        t[1, h - 1] = 255
    if n > 3:
        t[3] = 255
    return t


SDF_CASES = [(3, 1, 1, 3, None), (2, 1, 40, 3, None), (2, 40, 1, 3, None), (4, 37, 53, 3, None),
             (2, 19, 300, 3, None), (2, 300, 19, 3, None), (1, 2, 2048, 3, None), (1, 64, 64, 4, [0, 1, 2, 3])]


@pytest.mark.parametrize('case', SDF_CASES, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_signed_distance_bitwise(gpu, case):
    from medical_segmentation_pytorch_amd.ops.surface import signed_distance
    n, h, w, c, classes = case
    t = _sdf_labels(n, h, w, c)
    ref = signed_distance(t, c, 255, classes, squared=True)
    got = signed_distance(t.to(gpu), c, 255, classes, squared=True)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == ref.shape
    assert torch.equal(got.cpu(), ref)
    if h * w > 1:
        assert torch.count_nonzero(ref[0, 0]) > 0                      # a live plane ...
    assert torch.count_nonzero(ref[0, (c - 2) if classes is None else (c - 1)]) == 0   # ... and the absent class
    phi_ref = signed_distance(t, c, 255, classes)
    phi = signed_distance(t.to(gpu), c, 255, classes)
    assert phi.dtype == torch.float32 and torch.equal(phi.cpu(), phi_ref)   # the device root is correctly rounded
    again = signed_distance(t.to(gpu), c, 255, classes, squared=True)
    assert torch.equal(again, got)
    # int32 labels and no ignore_index (255 >= c is out of range anyway)
    assert torch.equal(signed_distance(t.to(gpu).int(), c, None, classes, squared=True), got)


def test_phi_root_is_correctly_rounded_for_every_distance(gpu):
    """phi of every s in [-2^23, 2^23] (the range the size cap allows) against the IEEE fp32 root of the CPU."""
    from medical_segmentation_pytorch_amd.ops._ext import require
    from medical_segmentation_pytorch_amd.ops.surface import _phi_torch
    s = torch.arange(-2 ** 23, 2 ** 23 + 1, dtype=torch.int32)
    phi = torch.empty(s.shape, dtype=torch.float32, device=gpu)
    require().sdf_phi(s.to(gpu), phi)
    assert torch.equal(phi.cpu(), _phi_torch(s))


@pytest.mark.parametrize('hw', [(1, 2049), (2049, 1)])
def test_size_cap_on_both_paths(gpu, hw):
    from medical_segmentation_pytorch_amd.ops.losses import boundary_loss
    from medical_segmentation_pytorch_amd.ops.surface import signed_distance
    t = torch.zeros(1, *hw, dtype=torch.long)
    for dev in ('cpu', gpu):
        with pytest.raises(ValueError, match='2048'):
            signed_distance(t.to(dev), 2)
    with pytest.raises(ValueError, match='2048'):
        boundary_loss(torch.zeros(1, 2, *hw, device=gpu), t.to(gpu))


# -------------------------------------------------------------------------------- loss against the oracle
SHAPES = [(3, 2, 20, 24), (3, 3, 20, 24), (2, 4, 7, 9), (2, 5, 72, 72), (2, 2, 71, 71), (1, 64, 8, 8)]


def _case(shape, scale=1.0):
    """Logits, labels with two ignored rows, a fully ignored sample (N >= 3), one class absent from sample 0,
    one label == C and one == -1 (the construction of test_gpu_region_loss.py)."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g) * scale
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0][t[0] == c - 1] = 0
    t[0, 1], t[n - 1, h - 1] = 255, 255
    if n >= 3:
        t[1] = 255
    t[0, 0, 0], t[0, 0, 1] = c, -1
    if scale != 1.0:
        x[0, :, 2, 2] = -80.0
        x[0, 0, 2, 2] = 80.0
        t[0, 2, 2] = 1
        x[0, :, 2, 3] = -80.0
        x[0, 0, 2, 3] = 80.0
        t[0, 2, 3] = 0
    return x, t


def _oracle(x, t, include_bg):
    """The plain-torch module in fp64 on the CPU, upstream gradient 0.5; also mean |p * phi|."""
    from medical_segmentation_pytorch_amd.core.loss import BoundaryLoss
    from medical_segmentation_pytorch_amd.ops.surface import signed_distance
    fn = BoundaryLoss(None, weight=1.0, ignore_index=255, include_background=include_bg)
    xr = x.double().requires_grad_(True)
    loss = fn(xr, t)
    (loss * 0.5).backward()
    c = x.shape[1]
    cls = fn.classes(c)
    valid = (t != 255) & (t >= 0) & (t < c)
    phi = signed_distance(t, c, 255, cls).double()
    mag = (torch.softmax(x.double(), 1)[:, cls] * phi).abs().sum().item() / (len(cls) * max(int(valid.sum()), 1))
    return loss.item(), xr.grad, mag


def _fused(x, t, include_bg, gpu):
    from medical_segmentation_pytorch_amd.ops.losses import boundary_loss
    xg = x.to(gpu).requires_grad_(True)
    loss = boundary_loss(xg, t.to(gpu), 255, list(range(0 if include_bg else 1, x.shape[1])))
    (loss * 0.5).backward()
    return loss, xg.grad


def _check(x, t, include_bg, gpu):
    ref, gref, mag = _oracle(x, t, include_bg)
    loss, grad = _fused(x, t, include_bg, gpu)
    err_l, err_g = abs(loss.item() - ref) / max(1.0, mag), _rel(grad.cpu(), gref)
    print(f'boundary {tuple(x.shape)} bg={include_bg}: loss {loss.item():.7f} ref {ref:.7f} mean|p phi| {mag:.4f} '
          f'rel |d| {err_l:.2e}; grad rel L2 {err_g:.2e}')
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    assert err_l <= LOSS_BAR, (err_l, loss.item(), ref)
    assert err_g <= GRAD_BAR, err_g
    invalid = ((t == 255) | (t < 0) | (t >= x.shape[1])).unsqueeze(1).expand_as(x)
    assert torch.count_nonzero(grad.cpu()[invalid]) == 0   # ignored pixels: exact zeros
    assert gref.abs().max() > 0


@pytest.mark.parametrize('include_bg', [False, True], ids=['fg', 'bg'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_matches_fp64_oracle(gpu, shape, include_bg):
    _check(*_case(shape), include_bg, gpu)


@pytest.mark.parametrize('include_bg', [False, True], ids=['fg', 'bg'])
@pytest.mark.parametrize('shape', SHAPES[:4], ids=lambda s: 'x'.join(map(str, s)))
def test_large_logits(gpu, shape, include_bg):
    _check(*_case(shape, scale=30.0), include_bg, gpu)


def test_no_valid_pixel(gpu):
    x, t = _case((2, 3, 6, 7))
    t[:] = 255
    loss, grad = _fused(x, t, False, gpu)
    assert loss.item() == 0.0 and torch.count_nonzero(grad) == 0


def test_class_cap(gpu):
    from medical_segmentation_pytorch_amd.ops.losses import boundary_loss
    x = torch.randn(1, 65, 4, 4, device=gpu)
    t = torch.randint(0, 65, (1, 4, 4), device=gpu)
    with pytest.raises(RuntimeError, match='64'):
        boundary_loss(x, t)


@pytest.mark.parametrize('shape', [(3, 2, 20, 24), (2, 4, 7, 9), (2, 5, 72, 72)], ids=lambda s: 'x'.join(map(str, s)))
def test_bitwise_repeatable(gpu, shape):
    x, t = _case(shape)
    l1, g1 = _fused(x, t, False, gpu)
    l2, g2 = _fused(x, t, False, gpu)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_module_takes_fused_path(gpu):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core.loss import BoundaryLoss, get_loss_fn
    c = MyConfig().init_dependent_config()
    c.loss_type, c.class_weights, c.loss_boundary_weight = 'focal_tversky_boundary', [1.0, 3.0], 0.05
    fn = get_loss_fn(c, gpu)
    assert isinstance(fn, BoundaryLoss) and fn.bw.is_cuda
    x, t = _case((3, 2, 20, 24))
    xg = x.to(gpu).requires_grad_(True)
    assert '_Boundary' in type(fn.boundary_term(xg, t.to(gpu)).grad_fn).__name__
    loss = fn(xg, t.to(gpu))
    loss.backward()
    xr = x.double().requires_grad_(True)
    ref = fn.cpu()(xr, t)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_BAR and _rel(xg.grad.cpu(), xr.grad) <= GRAD_BAR


def test_boundary_loss_in_captured_graph(gpu):
    """Forward + backward inside a hipGraph: a replay on refreshed inputs is bitwise the eager result, also after
    the weight buffer was refilled in place (no re-capture)."""
    from medical_segmentation_pytorch_amd.core.loss import BoundaryLoss, RegionLoss
    fn = BoundaryLoss(RegionLoss('ce', 'dice', 255), weight=0.04, ramp_epochs=4, device=gpu)
    torch.manual_seed(3)
    x = torch.randn(2, 2, 32, 32, device=gpu, requires_grad=True)
    tgt = torch.randint(0, 2, (2, 32, 32), device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm-up outside the capture
        fn(x, tgt).backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(g):
        out = fn(x, tgt)
        out.backward()
    for epoch, scale in ((0, 1.0), (0, 0.05), (2, 4.0), (5, 1.0)):
        fn.set_epoch(epoch)
        with torch.no_grad():
            x.copy_(torch.randn_like(x) * scale)
            tgt.copy_(torch.randint(0, 2, tgt.shape, device=gpu))
            tgt[0, 3] = 255
            x.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        xe = x.detach().clone().requires_grad_(True)
        eager = fn(xe, tgt)
        eager.backward()
        assert torch.equal(out.detach(), eager.detach()), (epoch, scale, out.item(), eager.item())
        assert torch.equal(x.grad, xe.grad)
        base = fn.base(xe.detach(), tgt)
        assert (out.detach() != base).item()                 # the boundary term is in the replayed value
    assert fn.bw.item() == torch.tensor(0.04).item()


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


@pytest.mark.parametrize('accum', [1, 2])
def test_trainer_graph_with_boundary_loss(gpu, tmp_path, accum):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.core.loss import BoundaryLoss, boundary_weight_at
    c = _cfg(tmp_path, engine='fused', loss_type='ce_dice_boundary', boundary_ramp_epochs=2,
             loss_boundary_weight=0.02, accum_steps=accum)
    t = SegTrainer(c)
    assert isinstance(t.loss_fn, BoundaryLoss)
    t.run(c)
    assert t.engine is not None and t.engine.graph is not None
    assert torch.isfinite(torch.tensor(t.last_loss))
    assert os.path.isfile(os.path.join(c.save_dir, 'last.pth'))
    assert t.loss_fn.bw.item() == torch.tensor(boundary_weight_at(2, 0.02, 2)).item()
