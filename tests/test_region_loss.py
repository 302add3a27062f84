"""Softmax-head Dice / Tversky / focal losses (``core.loss.RegionLoss``): routing, the plain-torch form
against an independent per-class / per-sample loop, identities, gradients and edge cases (CPU tier)."""
import math

import pytest
import torch
import torch.nn.functional as F

from medical_segmentation_pytorch_amd.configs import MyConfig
from medical_segmentation_pytorch_amd.configs.parser import load_parser
from medical_segmentation_pytorch_amd.core.loss import (BceDiceLoss, CrossEntropyLoss, OhemCELoss, RegionLoss,
                                                        get_loss_fn)

CPU = torch.device('cpu')
TYPES = {'dice': (None, 'dice'), 'tversky': (None, 'tversky'), 'focal': ('focal', None), 'ce_dice': ('ce', 'dice'),
         'ce_tversky': ('ce', 'tversky'), 'focal_dice': ('focal', 'dice'), 'focal_tversky': ('focal', 'tversky')}


def _cfg(**kw):
    c = MyConfig().init_dependent_config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize('lt', sorted(TYPES))
def test_routing_new_types(lt):
    c = _cfg(loss_type=lt, num_class=2, class_weights=[1.0, 3.0], dice_smooth=0.5, tversky_alpha=0.4,
             tversky_beta=0.6, focal_gamma=1.5, loss_pixel_weight=0.7, loss_region_weight=1.3,
             dice_ignore_background=True)
    fn = get_loss_fn(c, CPU)
    assert type(fn) is RegionLoss
    assert (fn.pixel, fn.region) == TYPES[lt]
    assert (fn.smooth, fn.alpha, fn.beta, fn.gamma, fn.pw, fn.rw) == (0.5, 0.4, 0.6, 1.5, 0.7, 1.3)
    assert fn.ignore_background is True and fn.ignore_index == c.ignore_index
    assert torch.equal(fn.weight, torch.tensor([1.0, 3.0]))


def test_routing_defaults_and_existing_types():
    c = _cfg(loss_type='ce_dice')
    assert c.num_class == 2   # MyConfig's default head
    fn = get_loss_fn(c, CPU)
    assert (fn.pw, fn.rw, fn.smooth, fn.alpha, fn.beta, fn.gamma) == (1.0, 1.0, 1.0, 0.3, 0.7, 2.0)
    assert fn.ignore_background is False and fn.weight is None
    assert type(get_loss_fn(_cfg(loss_type='ce'), CPU)) is CrossEntropyLoss
    assert type(get_loss_fn(_cfg(loss_type='ohem'), CPU)) is OhemCELoss
    for lt, (bw, dw) in {'dice': (0.0, 1.0), 'bce': (1.0, 0.0), 'bce_dice': (1.0, 1.0)}.items():
        fn = get_loss_fn(_cfg(loss_type=lt, num_class=1), CPU)
        assert type(fn) is BceDiceLoss and (fn.bw, fn.dw) == (bw, dw)


@pytest.mark.parametrize('lt,nc', [('bce', 2), ('bce_dice', 2), ('bce_dice', 3), ('ce_dice', 1)])
def test_routing_value_errors(lt, nc):
    with pytest.raises(ValueError, match='num_class'):
        get_loss_fn(_cfg(loss_type=lt, num_class=nc), CPU)


def test_routing_unknown_type():
    with pytest.raises(NotImplementedError):
        get_loss_fn(_cfg(loss_type='lovasz'), CPU)


# ------------------------------------------------------------------- an independent loop reference (fp64)
def _loop_reference(x, t, weight, ignore_index, pixel, region, pw, rw, smooth, alpha, beta, gamma, ignore_bg):
    n_, c_, h_, w_ = x.shape
    xs, ts = x.tolist(), t.tolist()
    num_pix = den_pix = 0.0
    ti_sum, ti_cnt = 0.0, 0
    for n in range(n_):
        inter, ps, tsum = [0.0] * c_, [0.0] * c_, [0.0] * c_
        for i in range(h_):
            for j in range(w_):
                lab = ts[n][i][j]
                if lab == ignore_index or lab < 0 or lab >= c_:
                    continue
                v = [xs[n][c][i][j] for c in range(c_)]
                m = max(v)
                e = [math.exp(a - m) for a in v]
                se = sum(e)
                p = [a / se for a in e]
                logpt = v[lab] - (m + math.log(se))
                wt = 1.0 if weight is None else weight[lab]
                if pixel == 'ce':
                    num_pix += wt * -logpt
                elif pixel == 'focal':
                    q = sum(p[c] for c in range(c_) if c != lab)
                    num_pix += wt * -(q ** gamma) * logpt
                den_pix += wt
                for c in range(c_):
                    ps[c] += p[c]
                inter[lab] += p[lab]
                tsum[lab] += 1.0
        for c in range(1 if ignore_bg else 0, c_):
            if region == 'dice':
                ti = (2 * inter[c] + smooth) / (ps[c] + tsum[c] + smooth)
            else:
                fp, fn = ps[c] - inter[c], tsum[c] - inter[c]
                ti = (inter[c] + smooth) / (inter[c] + alpha * fp + beta * fn + smooth)
            ti_sum += ti
            ti_cnt += 1
    total = 0.0
    if pixel is not None:
        total += pw * (num_pix / den_pix if den_pix > 0 else 0.0)
    if region is not None:
        total += rw * (1.0 - ti_sum / ti_cnt)
    return total


def _inputs(n=2, c=3, h=4, w=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2
    t = torch.randint(0, c, (n, h, w), generator=g)
    t[0, 1] = 255   # one ignored row
    return x, t


@pytest.mark.parametrize('ignore_bg', [False, True])
@pytest.mark.parametrize('lt', sorted(TYPES))
def test_fallback_matches_loop_reference(lt, ignore_bg):
    x, t = _inputs()
    pixel, region = TYPES[lt]
    weight = [0.5, 2.0, 1.25]
    kw = dict(pixel_weight=0.7, region_weight=1.3, smooth=0.5, alpha=0.4, beta=0.6, gamma=1.5)
    fn = RegionLoss(pixel, region, 255, torch.tensor(weight), ignore_background=ignore_bg, **kw)
    got = fn(x, t)
    assert got.dtype == torch.float64
    ref = _loop_reference(x, t, weight, 255, pixel, region, 0.7, 1.3, 0.5, 0.4, 0.6, 1.5, ignore_bg)
    assert abs(got.item() - ref) <= 1e-12, (got.item(), ref)


def test_fallback_masks_out_of_range_labels():
    x, t = _inputs()
    t2 = t.clone()
    t2[1, 0, 0], t2[1, 0, 1] = 3, -1      # label == C and a negative label: ignored like 255
    t3 = t.clone()
    t3[1, 0, 0], t3[1, 0, 1] = 255, 255
    fn = RegionLoss('focal', 'tversky', 255)
    assert fn(x, t2).item() == fn(x, t3).item()


# ---------------------------------------------------------------------------------------------- identities
def test_identity_region_weight_zero_is_cross_entropy():
    x, t = _inputs()
    w = torch.tensor([0.5, 2.0, 1.25], dtype=torch.float64)
    got = RegionLoss('ce', 'dice', 255, w, region_weight=0.0)(x, t)
    ref = F.cross_entropy(x, t, weight=w, ignore_index=255)
    assert abs(got.item() - ref.item()) <= 1e-12
    assert abs(RegionLoss('ce', None, 255, w)(x, t).item() - ref.item()) <= 1e-12


def test_identity_focal_gamma_zero_is_ce():
    x, t = _inputs()
    a = RegionLoss('focal', 'dice', 255, gamma=0.0)(x, t)
    b = RegionLoss('ce', 'dice', 255)(x, t)
    assert a.item() == b.item()


def test_identity_tversky_half_half_is_dice():
    x, t = _inputs()
    s = 0.8
    a = RegionLoss(None, 'tversky', 255, alpha=0.5, beta=0.5, smooth=s / 2)(x, t)
    b = RegionLoss(None, 'dice', 255, smooth=s)(x, t)
    assert abs(a.item() - b.item()) <= 1e-12


# ------------------------------------------------------------------------------- gradients and edge cases
@pytest.mark.parametrize('lt', ['ce_dice', 'focal_tversky'])
def test_gradcheck(lt):
    x, t = _inputs(2, 3, 4, 4, seed=1)
    x.requires_grad_(True)
    pixel, region = TYPES[lt]
    fn = RegionLoss(pixel, region, 255, torch.tensor([0.5, 2.0, 1.25]), gamma=1.5, ignore_background=True)
    assert torch.autograd.gradcheck(lambda v: fn(v, t), (x,), eps=1e-6, atol=1e-6)


def test_fully_ignored_sample_has_zero_gradient():
    x, t = _inputs()
    t[1] = 255
    x.requires_grad_(True)
    loss = RegionLoss('focal', 'tversky', 255)(x, t)
    loss.backward()
    assert torch.isfinite(loss)
    assert torch.count_nonzero(x.grad[1]) == 0 and torch.count_nonzero(x.grad[0]) > 0
    assert torch.count_nonzero(x.grad[0, :, 1]) == 0   # the ignored row of the other sample


@pytest.mark.parametrize('lt', ['ce_dice', 'focal', 'tversky'])
def test_all_ignored_batch(lt):
    x, t = _inputs()
    t[:] = 255
    x.requires_grad_(True)
    pixel, region = TYPES[lt]
    loss = RegionLoss(pixel, region, 255, region_weight=1.3, smooth=0.5)(x, t)
    loss.backward()
    # every TI is s / s = 1, so the region term is rw * (1 - 1); the pixel term is defined as 0
    assert loss.item() == 0.0
    assert torch.count_nonzero(x.grad) == 0


def test_dtype_follows_input():
    x, t = _inputs()
    assert RegionLoss('ce', 'dice')(x.float(), t).dtype == torch.float32
    assert RegionLoss('ce', 'dice')(x.half(), t).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ parser
def test_parser_flags_land_in_config():
    c = load_parser(MyConfig(), ['--loss_type', 'focal_tversky', '--focal_gamma', '1.5', '--tversky_alpha', '0.4',
                                 '--tversky_beta', '0.6', '--dice_smooth', '0.5', '--dice_ignore_background',
                                 '--loss_pixel_weight', '0.25', '--loss_region_weight', '2'])
    assert (c.loss_type, c.focal_gamma, c.tversky_alpha, c.tversky_beta, c.dice_smooth) == \
        ('focal_tversky', 1.5, 0.4, 0.6, 0.5)
    assert c.dice_ignore_background is True and (c.loss_pixel_weight, c.loss_region_weight) == (0.25, 2.0)
    fn = get_loss_fn(c, CPU)
    assert (fn.pixel, fn.region, fn.gamma, fn.ignore_background) == ('focal', 'tversky', 1.5, True)
    d = MyConfig()
    assert (d.loss_pixel_weight, d.loss_region_weight, d.dice_smooth, d.dice_ignore_background, d.tversky_alpha,
            d.tversky_beta, d.focal_gamma) == (1.0, 1.0, 1.0, False, 0.3, 0.7, 2.0)


def test_fractional_gamma_rejected_when_built():
    c = load_parser(MyConfig(), ['--loss_type', 'focal', '--focal_gamma', '0.5'])
    assert c.focal_gamma == 0.5
    with pytest.raises(ValueError, match='focal_gamma'):
        get_loss_fn(c, CPU)
