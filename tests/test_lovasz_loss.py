"""Lovasz-softmax loss, CPU tier: routing, the plain-torch form of ``LovaszSoftmaxLoss`` against an independent
pure-Python fp64 loop (Berman's cumulative formula on a compacted, stably sorted list), the vertex identity
``L_sc = 1 - IoU_c``, the gradient against central differences, ties, empty cases and dtypes."""
import math

import pytest
import torch

CPU = torch.device('cpu')


def _cfg(**kw):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    c = MyConfig()
    for k, v in kw.items():
        setattr(c, k, v)
    return c.init_dependent_config()


def _case(shape, seed=0):
    """Logits and labels with two ignored rows, a fully ignored image (the last), a class absent from image 0,
    one label == C and one == -1."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0][t[0] == c - 1] = 0
    t[0, 1], t[0, h - 1] = 255, 255
    t[n - 1] = 255
    t[0, 0, 0], t[0, 0, 1] = c, -1
    return x, t


def _loop_reference(x, t, per_image, ignore_background, ignore_index=255):
    """fp64, pure Python: compact the valid pixels of a segment, sort them stably by error (descending), walk
    the order with Berman's Jaccard differences J_i - J_{i-1}."""
    n, c, h, w = x.shape
    p = torch.softmax(x.double(), 1).tolist()
    lab = t.tolist()
    segments = [[i] for i in range(n)] if per_image else [list(range(n))]
    total = 0.0
    for seg in segments:
        per_class = []
        for k in range(1 if ignore_background else 0, c):
            items = []
            for i in seg:
                for a in range(h):
                    for b in range(w):
                        v = lab[i][a][b]
                        if v == ignore_index or v < 0 or v >= c:
                            continue
                        y = 1 if v == k else 0
                        items.append((abs(y - p[i][k][a][b]), y))
            G = sum(y for _, y in items)
            if G == 0:
                continue
            items.sort(key=lambda it: -it[0])       # list.sort is stable: ties keep ascending pixel index
            cum_y = cum_n = 0
            prev = loss = 0.0
            for e, y in items:
                cum_y += y
                cum_n += 1 - y
                jac = 1.0 - (G - cum_y) / (G + cum_n)
                loss += e * (jac - prev)
                prev = jac
            per_class.append(loss)
        total += sum(per_class) / len(per_class) if per_class else 0.0
    return total / len(segments)


def _separated(shape, seed=0):
    """Softmax outputs on a lattice, so that no two errors of a class are closer than ~0.1 / (C P)."""
    n, c, h, w = shape
    P = n * h * w
    g = torch.Generator().manual_seed(seed)
    k = torch.randperm(P, generator=g).double()
    if c == 2:
        p1 = (k + 0.25) / P
        p = torch.stack([1 - p1, p1], 1)
    else:
        cols = [(k + 0.25 + 0.1 * j) / (c * P) for j in range(c - 1)]
        p = torch.stack(cols + [1 - sum(cols)], 1)
    x = p.log().reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    t = torch.randint(0, c, (n, h, w), generator=g)
    return x, t


def test_routing():
    from medical_segmentation_pytorch_amd.core.loss import (LOVASZ_LOSS_TYPES, LovaszSoftmaxLoss, RegionLoss,
                                                            get_loss_fn)
    assert LOVASZ_LOSS_TYPES == ('lovasz_softmax', 'ce_lovasz_softmax', 'focal_lovasz_softmax')
    kw = dict(num_class=3, class_weights=[1.0, 2.0, 3.0], loss_pixel_weight=0.7, loss_region_weight=1.3,
              focal_gamma=1.5, dice_ignore_background=True, lovasz_per_image=True)
    for lt, pixel in zip(LOVASZ_LOSS_TYPES, (None, 'ce', 'focal')):
        fn = get_loss_fn(_cfg(loss_type=lt, **kw), CPU)
        assert type(fn) is LovaszSoftmaxLoss
        assert (fn.weight, fn.per_image, fn.ignore_background, fn.ignore_index) == (1.3, True, True, 255)
        if pixel is None:
            assert fn.base is None
        else:
            assert type(fn.base) is RegionLoss and (fn.base.pixel, fn.base.region) == (pixel, None)
            assert (fn.base.pw, fn.base.gamma) == (0.7, 1.5)
            assert torch.equal(fn.base.weight, torch.tensor([1.0, 2.0, 3.0]))
    fn = get_loss_fn(_cfg(loss_type='lovasz_softmax'), CPU)
    assert (fn.weight, fn.per_image, fn.ignore_background) == (1.0, False, False)
    for lt in LOVASZ_LOSS_TYPES:
        with pytest.raises(ValueError, match='num_class'):
            get_loss_fn(_cfg(loss_type=lt, num_class=1), CPU)
    with pytest.raises(ValueError, match='RegionLoss'):
        LovaszSoftmaxLoss(RegionLoss('ce', 'dice'))
    with pytest.raises(ValueError, match='num_class'):
        LovaszSoftmaxLoss()(torch.zeros(1, 1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))


def test_parser_and_config():
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.configs.parser import load_parser
    assert MyConfig().lovasz_per_image is False
    c = load_parser(MyConfig(), ['--loss_type', 'ce_lovasz_softmax', '--lovasz_per_image'])
    assert (c.loss_type, c.lovasz_per_image) == ('ce_lovasz_softmax', True)
    assert load_parser(MyConfig(), ['--loss_type', 'focal_lovasz_softmax']).lovasz_per_image is False


@pytest.mark.parametrize('ignore_background', [False, True])
@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', [(2, 3, 4, 5), (3, 2, 6, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_plain_form_matches_loop_reference(shape, per_image, ignore_background):
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    x, t = _case(shape)
    got = LovaszSoftmaxLoss(per_image=per_image, ignore_background=ignore_background)(x, t).item()
    ref = _loop_reference(x, t, per_image, ignore_background)
    assert ref > 0 and abs(got - ref) <= 1e-12, (got, ref)


def test_base_and_weight():
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss, RegionLoss
    x, t = _case((2, 3, 4, 5))
    base = RegionLoss('ce', None, pixel_weight=0.7)
    got = LovaszSoftmaxLoss(base, weight=1.3)(x, t).item()
    assert abs(got - (base(x, t).item() + 1.3 * _loop_reference(x, t, False, False))) <= 1e-12


def _hard_logits(pred, c):
    return (torch.nn.functional.one_hot(pred, c).movedim(-1, 1).double() * 2 - 1) * 40


def test_vertex_identity():
    """With p in {0, 1} (up to exp(-80)) the loss of a class is 1 - IoU_c: the Lovasz extension interpolates the
    Jaccard loss."""
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 2, 4, 6, 7
    t = torch.randint(0, c - 1, (n, h, w), generator=g)        # class 3 absent from the labels
    pred = torch.randint(0, c, (n, h, w), generator=g)
    t[0, 0] = 255
    valid = t != 255
    for per_image in (False, True):
        segs = [slice(i, i + 1) for i in range(n)] if per_image else [slice(0, n)]
        ref = 0.0
        for s in segs:
            ious = []
            for k in range(c):
                a, b = (pred[s] == k) & valid[s], (t[s] == k) & valid[s]
                if b.any():
                    ious.append(1.0 - (a & b).sum().item() / (a | b).sum().item())
            ref += sum(ious) / len(ious)
        got = LovaszSoftmaxLoss(per_image=per_image)(_hard_logits(pred, c), t).item()
        assert abs(got - ref / len(segs)) <= 1e-12, (per_image, got, ref)
    fn = LovaszSoftmaxLoss()
    assert abs(fn(_hard_logits(t.clamp(max=c - 1), c), t).item()) <= 1e-12              # perfect prediction
    assert abs(fn(_hard_logits((t.clamp(max=c - 1) + 1) % (c - 1), c), t).item() - 1.0) <= 1e-12   # all wrong
    for seed in range(3):
        x, tt = _case((2, 3, 4, 5), seed)
        assert 0.0 <= fn(x * 3, tt).item() <= 1.0


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', [(2, 2, 3, 4), (2, 3, 3, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_gradient_matches_central_differences(shape, per_image):
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    x, t = _separated(shape)
    t[0, 0, 0] = 255
    fn = LovaszSoftmaxLoss(per_image=per_image)
    xr = x.clone().requires_grad_(True)
    fn(xr, t).backward()
    eps = 1e-6
    num = torch.zeros_like(x)
    flat, nflat = x.view(-1), num.view(-1)
    for i in range(flat.numel()):
        old = flat[i].item()
        flat[i] = old + eps
        up = fn(x, t).item()
        flat[i] = old - eps
        dn = fn(x, t).item()
        flat[i] = old
        nflat[i] = (up - dn) / (2 * eps)
    assert (xr.grad - num).abs().max().item() <= 1e-8
    assert torch.count_nonzero(xr.grad[0, :, 0, 0]) == 0 and xr.grad.abs().max() > 1e-3


def test_ties_follow_ascending_index():
    """Two pixels with identical logits and different labels: every error is 0.5, so only the tie rule decides
    which pixel gets which coefficient.  C = 2, G = 1 per class: the first pixel in raster order gets rank 0."""
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    x = torch.zeros(1, 2, 1, 2, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[[1, 0]]])
    loss = LovaszSoftmaxLoss()(x, t)
    loss.backward()
    # class 1: y = (1, 0) in sorted order: g = (1 / 1, 0 / (2 * 1)) = (1, 0); class 0: y = (0, 1): U = (2, 2),
    # g = (1 / (2 * 1), 1 / 2) = (0.5, 0.5).  dL/dp_c = sign(p_c - y) g / 2 classes
    dp = torch.tensor([[[[0.25, -0.25]], [[-0.5, 0.0]]]], dtype=torch.float64)
    p = torch.full_like(dp, 0.5)
    expect = p * (dp - (dp * p).sum(1, keepdim=True))
    assert abs(loss.item() - 0.5 * (0.5 * 1.0 + 0.5 * 0.5 + 0.5 * 0.5)) <= 1e-15
    assert torch.allclose(x.grad, expect, rtol=0, atol=1e-15), (x.grad, expect)
    # the labels swapped: now the first pixel is the y = 0 one
    x2 = torch.zeros(1, 2, 1, 2, dtype=torch.float64, requires_grad=True)
    LovaszSoftmaxLoss()(x2, torch.tensor([[[0, 1]]])).backward()
    dp2 = torch.tensor([[[[-0.5, 0.0]], [[0.25, -0.25]]]], dtype=torch.float64)
    assert torch.allclose(x2.grad, p * (dp2 - (dp2 * p).sum(1, keepdim=True)), rtol=0, atol=1e-15)


@pytest.mark.parametrize('per_image', [False, True])
def test_empty_cases(per_image):
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    x = torch.randn(2, 3, 4, 4, dtype=torch.float64, requires_grad=True)
    t = torch.full((2, 4, 4), 255)
    t[0, 0, 0], t[1, 1, 1] = 3, -1
    loss = LovaszSoftmaxLoss(per_image=per_image)(x, t)
    loss.backward()
    assert loss.item() == 0.0 and torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad) == 0
    x.grad = None
    loss = LovaszSoftmaxLoss(per_image=per_image, ignore_background=True)(x, torch.zeros(2, 4, 4, dtype=torch.long))
    loss.backward()
    assert loss.item() == 0.0 and torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad) == 0


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_output_dtype(dtype):
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss, RegionLoss
    x, t = _case((2, 3, 4, 5))
    for fn in (LovaszSoftmaxLoss(), LovaszSoftmaxLoss(RegionLoss('ce', None))):
        out = fn(x.to(dtype), t)
        assert out.dtype == torch.float32 and math.isfinite(out.item())
