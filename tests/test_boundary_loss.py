"""Boundary (signed-distance) loss, CPU tier: ``ops.surface.signed_distance`` against scipy's Euclidean distance
transform and the ``_edt_sq_torch`` composition, the hand cases of its definition, ``core.loss.BoundaryLoss``
against the analytic gradient, routing / config / parser / schedule, and a short eager trainer run."""
import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

from medical_segmentation_pytorch_amd.configs import MyConfig
from medical_segmentation_pytorch_amd.configs.parser import load_parser
from medical_segmentation_pytorch_amd.core.loss import (BOUNDARY_LOSS_TYPES, BceDiceLoss, BoundaryLoss,
                                                        CrossEntropyLoss, OhemCELoss, RegionLoss,
                                                        boundary_weight_at, get_loss_fn)
from medical_segmentation_pytorch_amd.ops.surface import SDF_MAX_DIM, _edt_sq_torch, signed_distance

CPU = torch.device('cpu')
NINE = ('boundary', 'ce_boundary', 'focal_boundary', 'dice_boundary', 'tversky_boundary', 'ce_dice_boundary',
        'ce_tversky_boundary', 'focal_dice_boundary', 'focal_tversky_boundary')


def _blobs(n, c, h, w, seed):
    """Labels made of a few discs per class on background 0 (the last image keeps every class)."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    t = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        for k in range(1, c):
            for _ in range(2):
                cy, cx = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
                r = 1 + int(torch.randint(0, max(2, min(h, w) // 3 + 1), (1,), generator=g))
                t[i][(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = k
    return t


def _valid(t, c, ignore_index):
    v = (t >= 0) & (t < c)
    return v if ignore_index is None else v & (t != ignore_index)


def _scipy_planes(t, c, ignore_index, classes):
    """(s, phi) in fp64 from scipy: edt(~pos) at neg pixels, -(edt(~neg)) at pos pixels, as the definition says."""
    valid = _valid(t, c, ignore_index).numpy()
    tn = t.numpy()
    s = np.zeros((t.shape[0], len(classes)) + tuple(t.shape[1:]), dtype=np.float64)
    phi = np.zeros_like(s)
    for n in range(t.shape[0]):
        for k, cl in enumerate(classes):
            pos, neg = valid[n] & (tn[n] == cl), valid[n] & (tn[n] != cl)
            if not pos.any() or not neg.any():
                continue
            to_pos, to_neg = distance_transform_edt(~pos), distance_transform_edt(~neg)
            s[n, k] = np.rint(to_pos ** 2) * neg - np.rint(to_neg ** 2) * pos
            phi[n, k] = to_pos * neg - (to_neg - 1.0) * pos
    return s, phi


def _edt_composition(t, c, ignore_index, classes):
    valid = _valid(t, c, ignore_index)
    out = []
    for cl in classes:
        pos, neg = valid & (t == cl), valid & (t != cl)
        live = (pos.flatten(1).any(1) & neg.flatten(1).any(1)).view(-1, 1, 1)
        a, b = _edt_sq_torch(pos), _edt_sq_torch(neg)
        zero = torch.zeros_like(a)
        out.append(torch.where(live, torch.where(neg, a, zero) - torch.where(pos, b, zero), zero))
    return torch.stack(out, 1)


# ------------------------------------------------------------------------------------------ signed distance
@pytest.mark.parametrize('c', [2, 3])
@pytest.mark.parametrize('hw', [(1, 1), (1, 7), (7, 1), (37, 53), (19, 300)], ids=lambda s: 'x'.join(map(str, s)))
def test_signed_distance_matches_scipy_and_edt(hw, c):
    t = _blobs(2, c, *hw, seed=hw[0] * 1000 + hw[1] + c)
    if hw[0] * hw[1] > 1:
        t[0, 0, 0] = 255
    classes = list(range(1, c))
    s = signed_distance(t, c, 255, squared=True)
    assert s.dtype == torch.int32 and s.shape == (2, c - 1) + hw
    ref_s, ref_phi = _scipy_planes(t, c, 255, classes)
    assert np.array_equal(s.numpy().astype(np.int64), ref_s.astype(np.int64))
    assert torch.equal(s, _edt_composition(t, c, 255, classes))
    phi = signed_distance(t, c, 255)
    assert phi.dtype == torch.float32
    ulp = np.spacing(np.abs(ref_phi).astype(np.float32)).astype(np.float64)
    assert (np.abs(phi.numpy().astype(np.float64) - ref_phi) <= ulp).all()
    # the stated values: >= 1 outside, <= -1 inside (phi <= 0 there), 0 at invalid pixels
    valid = _valid(t, c, 255)
    for k, cl in enumerate(classes):
        live = s[:, k].flatten(1).ne(0).any(1).view(-1, 1, 1)
        assert (s[:, k][live & valid & (t != cl)] >= 1).all() and (s[:, k][live & valid & (t == cl)] <= -1).all()
        assert (s[:, k][~valid] == 0).all()


def test_classes_argument_and_background_plane():
    t = _blobs(2, 3, 9, 11, seed=5)
    every = signed_distance(t, 3, None, classes=[0, 1, 2], squared=True)
    assert torch.equal(every[:, 1:], signed_distance(t, 3, squared=True))
    assert torch.equal(signed_distance(t, 3, classes=[2, 0], squared=True), every[:, [2, 0]])
    # two classes: the background plane is the negated foreground plane moved by the inside convention
    b = (t > 0).long()
    s = signed_distance(b, 2, classes=[0, 1], squared=True)
    assert torch.equal(s[:, 0], -s[:, 1])
    for bad in ([], [1, 1], [3], [-1]):
        with pytest.raises(ValueError, match='classes'):
            signed_distance(t, 3, classes=bad)


def test_hand_single_pixel_in_a_corner():
    t = torch.zeros(1, 4, 5, dtype=torch.long)
    t[0, 0, 0] = 1
    s = signed_distance(t, 2, squared=True)[0, 0]
    ys, xs = torch.meshgrid(torch.arange(4), torch.arange(5), indexing='ij')
    ref = (ys * ys + xs * xs).int()
    ref[0, 0] = -1
    assert torch.equal(s, ref)
    phi = signed_distance(t, 2)[0, 0]
    assert phi[0, 0] == 0.0 and phi[3, 4] == 5.0 and phi[0, 1] == 1.0


def test_hand_degenerate_planes_are_zero():
    t = torch.zeros(2, 5, 6, dtype=torch.long)
    t[0, 1:3, 1:4] = 1                       # class 2 absent from image 0
    t[1] = 2                                 # class 2 covers every valid pixel of image 1 ...
    t[1, 0] = 255                            # ... the rest being ignored; class 1 is absent there
    s = signed_distance(t, 3, 255, squared=True)
    assert s[0, 0].ne(0).all() and torch.count_nonzero(s[0, 1]) == 0
    assert torch.count_nonzero(s[1]) == 0
    assert torch.count_nonzero(signed_distance(t, 3, 255)[1]) == 0


def test_hand_distances_cross_an_ignored_stripe():
    t = torch.zeros(1, 3, 7, dtype=torch.long)
    t[0, :, :2] = 1
    t[0, :, 2:4] = 255                       # two ignored columns between the lesion and the background
    s = signed_distance(t, 2, 255, squared=True)[0, 0]
    assert torch.equal(s[1], torch.tensor([-16, -9, 0, 0, 9, 16, 25], dtype=torch.int32))
    assert torch.equal(s[0], s[1]) and torch.equal(s[2], s[1])
    phi = signed_distance(t, 2, 255)[0, 0]
    assert torch.equal(phi[1], torch.tensor([-3.0, -2.0, 0.0, 0.0, 3.0, 4.0, 5.0]))


def test_hand_out_of_range_labels_are_ignored():
    t = _blobs(1, 2, 8, 9, seed=2)
    a, b = t.clone(), t.clone()
    a[0, 3, 3], a[0, 4, 4], a[0, 0] = 2, -1, 255
    b[0, 3, 3], b[0, 4, 4], b[0, 0] = 255, 255, 255
    assert torch.equal(signed_distance(a, 2, 255, squared=True), signed_distance(b, 2, 255, squared=True))
    # without an ignore_index only the range rule applies
    assert torch.equal(signed_distance(a, 2, None, squared=True), signed_distance(b, 2, 255, squared=True))


def test_hand_all_ignored_image_and_empty_batch():
    t = _blobs(2, 2, 6, 6, seed=3)
    t[1] = 255
    s = signed_distance(t, 2, 255, squared=True)
    assert torch.count_nonzero(s[1]) == 0 and torch.count_nonzero(s[0]) > 0
    assert signed_distance(t[:0], 2, 255).shape == (0, 1, 6, 6)


def test_phi_root_is_correctly_rounded_for_every_distance():
    """Every s the size cap allows: phi uses the IEEE fp32 root (numpy's), whatever torch.sqrt does on this CPU."""
    from medical_segmentation_pytorch_amd.ops.surface import _phi_torch
    v = np.arange(0, 2 ** 23 + 1, dtype=np.int32)
    root = np.sqrt(v.astype(np.float32))
    s = torch.from_numpy(v)
    assert np.array_equal(_phi_torch(s).numpy(), root)
    inside = _phi_torch(-s).numpy()
    assert np.array_equal(inside[1:], np.float32(1.0) - root[1:]) and inside[0] == 0.0


@pytest.mark.parametrize('hw', [(1, SDF_MAX_DIM + 1), (SDF_MAX_DIM + 1, 1)])
def test_size_cap(hw):
    assert SDF_MAX_DIM == 2048
    with pytest.raises(ValueError, match='2048'):
        signed_distance(torch.zeros(1, *hw, dtype=torch.long), 2)
    with pytest.raises(ValueError, match='integer'):
        signed_distance(torch.zeros(1, 2, 2), 2)


# --------------------------------------------------------------------------------------------------- loss
def _loss_case(n=3, c=3, h=9, w=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2
    t = _blobs(n, c, h, w, seed)
    t[0, 1] = 255
    t[0, 0, 0], t[0, 0, 1] = c, -1
    t[1][t[1] == c - 1] = 0                  # one class absent from image 1
    return x, t


def _analytic(x, t, classes, ignore_index=255, g=1.0):
    """The loss and gradient formulas of the definition, written out."""
    c = x.shape[1]
    valid = _valid(t, c, ignore_index)
    phi = torch.zeros_like(x)
    phi[:, classes] = signed_distance(t, c, ignore_index, classes).to(x.dtype)
    p = torch.softmax(x, 1)
    norm = len(classes) * max(int(valid.sum()), 1)
    vf = valid.unsqueeze(1).to(x.dtype)
    loss = (p * phi * vf).sum() / norm
    grad = g / norm * p * (phi - (p * phi).sum(1, keepdim=True)) * vf
    return loss, grad


@pytest.mark.parametrize('include_bg', [False, True])
@pytest.mark.parametrize('c', [2, 3, 5])
def test_gradient_formula_matches_autograd(c, include_bg):
    x, t = _loss_case(c=c, seed=c)
    fn = BoundaryLoss(None, weight=1.0, include_background=include_bg)
    xr = x.clone().requires_grad_(True)
    loss = fn(xr, t)
    assert loss.dtype == torch.float64
    (loss * 0.5).backward()
    ref, gref = _analytic(x, t, fn.classes(c), g=0.5)
    assert abs(loss.item() - ref.item()) <= 1e-12
    assert (xr.grad - gref).abs().max().item() <= 1e-14
    invalid = ~_valid(t, c, 255)
    assert torch.count_nonzero(xr.grad.movedim(1, -1)[invalid]) == 0


def test_gradcheck_with_base():
    x, t = _loss_case(2, 3, 5, 6, seed=4)
    x.requires_grad_(True)
    fn = BoundaryLoss(RegionLoss('ce', 'dice', 255), weight=0.3)
    assert torch.autograd.gradcheck(lambda v: fn(v, t), (x,), eps=1e-6, atol=1e-6)
    base = RegionLoss('ce', 'dice', 255)(x, t)
    lb = BoundaryLoss(None, weight=1.0)(x, t)
    w = float(np.float32(0.3))                                               # the weight buffer is fp32
    assert abs(fn(x, t).item() - (base.item() + w * lb.item())) <= 1e-12


def test_no_valid_pixel_gives_zero_loss_and_gradient():
    x, t = _loss_case()
    t[:] = 255
    x.requires_grad_(True)
    loss = BoundaryLoss(None, weight=1.0)(x, t)
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(x.grad) == 0


def test_dtype_follows_input():
    x, t = _loss_case()
    assert BoundaryLoss(None)(x.float(), t).dtype == torch.float32
    assert BoundaryLoss(RegionLoss('ce', 'dice'))(x.half(), t).dtype == torch.float32


# ------------------------------------------------------------------------------- routing, config and parser
def _cfg(**kw):
    c = MyConfig()
    for k, v in kw.items():
        setattr(c, k, v)
    return c.init_dependent_config()


@pytest.mark.parametrize('lt', NINE)
def test_routing_boundary_types(lt):
    assert set(NINE) == set(BOUNDARY_LOSS_TYPES)
    c = _cfg(loss_type=lt, class_weights=[1.0, 3.0], loss_boundary_weight=0.05, boundary_ramp_epochs=4,
             boundary_include_background=True, dice_smooth=0.5, focal_gamma=1.5)
    fn = get_loss_fn(c, CPU)
    assert type(fn) is BoundaryLoss
    assert (fn.weight, fn.ramp_epochs, fn.include_background, fn.ignore_index) == (0.05, 4, True, c.ignore_index)
    terms = lt.split('_')[:-1]
    if not terms:
        assert fn.base is None
    else:
        assert type(fn.base) is RegionLoss
        assert fn.base.pixel == next((k for k in terms if k in ('ce', 'focal')), None)
        assert fn.base.region == next((k for k in terms if k in ('dice', 'tversky')), None)
        assert (fn.base.smooth, fn.base.gamma) == (0.5, 1.5) and torch.equal(fn.base.weight, torch.tensor([1.0, 3.0]))
    assert fn.bw.shape == (1,) and fn.bw.dtype == torch.float32 and 'bw' in dict(fn.named_buffers())
    assert fn.classes(3) == [0, 1, 2] and BoundaryLoss(None).classes(3) == [1, 2]
    x, t = _loss_case(2, 2, 6, 7)
    assert torch.isfinite(fn(x, t))


def test_defaults_and_existing_types_unchanged():
    d = MyConfig()
    assert (d.loss_boundary_weight, d.boundary_ramp_epochs, d.boundary_include_background) == (0.01, 0, False)
    assert type(get_loss_fn(_cfg(loss_type='ce'), CPU)) is CrossEntropyLoss
    assert type(get_loss_fn(_cfg(loss_type='ohem'), CPU)) is OhemCELoss
    assert type(get_loss_fn(_cfg(loss_type='bce_dice', num_class=1), CPU)) is BceDiceLoss
    for lt in ('dice', 'tversky', 'focal', 'ce_dice', 'ce_tversky', 'focal_dice', 'focal_tversky'):
        fn = get_loss_fn(_cfg(loss_type=lt), CPU)
        assert type(fn) is RegionLoss and not hasattr(fn, 'set_epoch')


@pytest.mark.parametrize('lt', ['boundary', 'dice_boundary', 'ce_dice_boundary'])
def test_sigmoid_head_is_rejected(lt):
    with pytest.raises(ValueError, match='softmax head'):
        get_loss_fn(_cfg(loss_type=lt, num_class=1), CPU)


@pytest.mark.parametrize('field,value', [('loss_boundary_weight', -0.1), ('loss_boundary_weight', float('nan')),
                                         ('loss_boundary_weight', 'x'), ('boundary_ramp_epochs', -1),
                                         ('boundary_ramp_epochs', 1.5), ('boundary_ramp_epochs', None)])
def test_invalid_config_values(field, value):
    with pytest.raises(ValueError, match=field):
        _cfg(**{field: value})


def test_parser_flags_land_in_config():
    c = load_parser(MyConfig(), ['--loss_type', 'ce_dice_boundary', '--loss_boundary_weight', '0.02',
                                 '--boundary_ramp_epochs', '10', '--boundary_include_background'])
    assert (c.loss_type, c.loss_boundary_weight, c.boundary_ramp_epochs, c.boundary_include_background) == \
        ('ce_dice_boundary', 0.02, 10, True)
    for lt in NINE:
        assert load_parser(MyConfig(), ['--loss_type', lt]).loss_type == lt
    with pytest.raises(SystemExit):
        load_parser(MyConfig(), ['--loss_type', 'boundary_ce'])
    with pytest.raises(ValueError, match='loss_boundary_weight'):
        load_parser(MyConfig(), ['--loss_boundary_weight', '-1'])


def test_schedule():
    assert [boundary_weight_at(e, 0.02, 0) for e in range(6)] == [0.02] * 6
    assert [boundary_weight_at(e, 0.02, 4) for e in range(6)] == [0.005, 0.01, 0.015, 0.02, 0.02, 0.02]
    fn = BoundaryLoss(None, weight=0.02, ramp_epochs=4)
    assert fn.bw.item() == np.float32(0.005)          # epoch 0 until the trainer says otherwise
    buf = fn.bw
    for e, want in enumerate([0.005, 0.01, 0.015, 0.02, 0.02, 0.02]):
        fn.set_epoch(e)
        assert fn.bw is buf and fn.bw.item() == np.float32(want)   # filled in place: a captured graph sees it
    x, t = _loss_case()
    fn.set_epoch(1)
    assert abs(fn(x, t).item() - float(np.float32(0.01)) * BoundaryLoss(None, weight=1.0)(x, t).item()) <= 1e-15
    for bad in (dict(weight=-1.0), dict(ramp_epochs=-2), dict(ramp_epochs=0.5), dict(base=CrossEntropyLoss())):
        with pytest.raises(ValueError):
            BoundaryLoss(**bad)


# ------------------------------------------------------------------------------------------------ trainer
def test_eager_cpu_trainer_run(tmp_path):
    from medical_segmentation_pytorch_amd.core import SegTrainer
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (16, 4, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 2, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.log_interval = 3, 1, False, 3
    c.loss_type, c.boundary_ramp_epochs, c.loss_boundary_weight = 'ce_dice_boundary', 2, 0.02
    c = c.init_dependent_config()
    t = SegTrainer(c)
    assert isinstance(t.loss_fn, BoundaryLoss) and isinstance(t.loss_fn.base, RegionLoss)
    t.run(c)
    assert torch.isfinite(torch.tensor(t.last_loss))
    assert t.loss_fn.bw.item() == np.float32(boundary_weight_at(2, 0.02, 2)) == np.float32(0.02)
