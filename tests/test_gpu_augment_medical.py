"""Rotation / shift / elastic warp and gamma / blur / noise on the GPU (csrc/augment.hip: aug_warp, aug_pointwise,
aug_blur) against the host specification evaluated on the SAME parameter records (MI355X only)."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from test_augment_medical_cpu import ALL_ON, _base_record, _lattice, _with_records, intensity_cases

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (64, 64), (150, 90), (48, 70), (120, 120), (33, 200)]
CROP = (64, 80)
LEVEL = 1.0 / (0.225 * 255)       # one uint8 level after Normalize (the channel with the smallest std)
NEW_KEYS = ('affine', 'elastic', 'gamma', 'blur', 'noise')


def _make_split(root, sizes, seed=0):
    rng = np.random.default_rng(seed)
    for split in ('train', 'validation', 'test'):
        for sub in ('images', 'masks'):
            (root / split / sub).mkdir(parents=True, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)),
                        rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
        msk = ((((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2) < 1).astype(np.uint8) * 255
        Image.fromarray(img).save(root / 'train' / 'images' / f'{i:03d}.jpg', quality=95)
        Image.fromarray(msk).save(root / 'train' / 'masks' / f'{i:03d}.jpg', quality=95)


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp('medical_aug_split')
    _make_split(root, SIZES)
    return root


def _dataset(root, crop=CROP, randscale=0.0, jitter=0.0, **medical):
    from medical_segmentation_pytorch_amd.datasets.polyp import PolypDataset
    cfg = SimpleNamespace(data_root=str(root), crop_h=crop[0], crop_w=crop[1], randscale=randscale, brightness=jitter,
                          contrast=jitter, saturation=jitter, h_flip=0.5, v_flip=0.5, num_class=2, **medical)
    ds = PolypDataset(cfg, 'train')
    if not jitter:
        ds.transform.jitter = (0.0, 0.0, 0.0, 0.0)      # no hue either
    return ds


def _levels(x, aug):
    """Normalized [B, 3, H, W] batch -> integer uint8 levels."""
    std = torch.tensor(aug.std).view(1, 3, 1, 1)
    mean = torch.tensor(aug.mean).view(1, 3, 1, 1)
    return torch.round(x.cpu() * std + mean)


WARPS = {
    'affine': dict(aug_rotate=30.0, aug_shift=0.1, aug_affine_p=1.0),
    'elastic1': dict(aug_elastic_sigma=3.0, aug_elastic_cells=1, aug_elastic_p=1.0),
    'elastic4': dict(aug_elastic_sigma=3.0, aug_elastic_cells=4, aug_elastic_p=1.0),
    'elastic8': dict(aug_elastic_sigma=3.0, aug_elastic_cells=8, aug_elastic_p=1.0),
    'both': dict(aug_rotate=180.0, aug_shift=0.25, aug_affine_p=1.0, aug_elastic_sigma=4.0, aug_elastic_cells=4,
                 aug_elastic_p=1.0),
}


@pytest.mark.parametrize('border', ['reflect', 'constant'])
@pytest.mark.parametrize('warp', list(WARPS))
def test_warp_alone_is_exact(gpu, split, warp, border):
    """Unscaled warp, no jitter: the device repeats the specification's fp32 operations one by one (contraction
    off), so image and mask agree at every pixel."""
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader, reference_batch
    ds = _dataset(split, aug_border=border, **WARPS[warp])
    aug = ds.transform
    loader = DeviceAugLoader(ds, 6, gpu, seed=3)
    idx = list(range(len(ds)))
    prms = [aug.sample_params(*loader.data.shapes[i]) for i in idx]
    assert all(not p['scaled'] and not p['jittered'] for p in prms)
    assert all((p.get('affine') is not None) or (p.get('elastic') is not None) for p in prms)
    x, m = loader.batch(idx, prms)
    xr, mr = reference_batch(aug, ds, idx, prms)
    torch.cuda.synchronize()
    assert loader.ex_batches == 1
    d = (x.cpu() - xr).abs()
    print(f'{warp}/{border}: max {d.max().item() / LEVEL:.3g} levels, {(d > 0).float().mean().item():.2e} differ, '
          f'mask mismatches {(m.cpu() != mr).sum().item()}')
    assert torch.equal(m.cpu(), mr)
    assert torch.equal(x.cpu(), xr)


@pytest.mark.parametrize('theta,k', [(90.0, 1), (-90.0, 3)])
def test_rotation_by_a_quarter_turn_is_rot90(gpu, theta, k):
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader, DeviceDataset
    from medical_segmentation_pytorch_amd.utils.transforms import SegAugment, normalize_to_tensor
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (48, 48, 3)).astype(np.uint8)
    msk = rng.integers(0, 2, (48, 48)).astype(np.uint8)
    aug = SegAugment(48, 48, aug_rotate=180.0)
    loader = DeviceAugLoader(None, 1, gpu, data=DeviceDataset.from_arrays([img], [msk], gpu), aug=aug)
    x, m = loader.batch([0], [_base_record(48, 48, (48, 48), affine=(theta, 0.0, 0.0))])
    ref = normalize_to_tensor(np.rot90(img, k).astype(np.float32), aug.mean, aug.std)
    assert torch.equal(x[0].cpu(), ref)
    assert np.array_equal(m[0].cpu().numpy(), np.rot90(msk, k))


def _mixed(split):
    kw = {k: v for k, v in ALL_ON.items() if not k.endswith('_p')}      # every group at its default p = 0.5
    ds = _dataset(split, randscale=[-0.5, 1.0], jitter=0.5, **kw)
    ds.transform.seed(12)
    idx = list(range(6)) * 4
    prms = [ds.transform.sample_params(*SIZES[i]) for i in idx]
    return ds, idx, prms


def test_mixed_batch(gpu, split):
    """p = 0.5 for every group: applied and skipped samples share a batch.  A sample that drew no new op comes out
    of the warp kernel's integer path (and past the other kernels) bit for bit as from the plain aug_batch path;
    the whole batch is within the bounds of the existing full-pipeline comparison."""
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader, reference_batch
    ds, idx, prms = _mixed(split)
    aug = ds.transform
    for k in NEW_KEYS:
        applied = sum(p[k] is not None for p in prms)
        assert 0 < applied < len(prms), k
    plain = [i for i, p in enumerate(prms) if all(p[k] is None for k in NEW_KEYS)]
    assert len(plain) >= 2 and any(prms[i]['scaled'] for i in plain) and any(prms[i]['jittered'] for i in plain)
    loader = DeviceAugLoader(ds, len(idx), gpu, seed=0)
    x, m = loader.batch(idx, prms)
    assert loader.ex_batches == 1
    old = _dataset(split, randscale=[-0.5, 1.0], jitter=0.5)
    assert not old.transform.medical
    old_loader = DeviceAugLoader(old, len(idx), gpu, seed=0, data=loader.data)
    x0, m0 = old_loader.batch(idx, [{k: v for k, v in p.items() if k not in NEW_KEYS} for p in prms])
    assert old_loader.ex_batches == 0
    torch.cuda.synchronize()
    assert torch.equal(x[plain], x0[plain]) and torch.equal(m[plain], m0[plain])
    xr, mr = reference_batch(aug, ds, idx, prms)
    d = (x.cpu() - xr).abs()
    print(f'mixed: max {d.max().item() / LEVEL:.2f} levels, mean {d.mean().item() / LEVEL:.4f}, mask '
          f'{(m.cpu() != mr).float().mean().item():.2e}')
    assert d.max().item() < 2.5 * LEVEL
    assert d.mean().item() < 0.02 * LEVEL
    assert (m.cpu() != mr).float().mean().item() < 1e-3


@pytest.mark.parametrize('name,crop,fields', intensity_cases())
def test_intensity_ops(gpu, name, crop, fields):
    """Gamma, blur (a 33x47 crop: tile edges off the 32-pixel tile, radius 8 and 1), noise, alone and together:
    every value within one uint8 level of the specification, and at most 1e-3 of them different at all (only a
    value within the arithmetic's error of a rounding tie can flip; tests/test_augment_medical_cpu.py measures
    that share on these inputs between an fp32 and an fp64 evaluation)."""
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader, DeviceDataset
    from medical_segmentation_pytorch_amd.utils.transforms import SegAugment
    img = np.random.default_rng(8).integers(0, 256, crop + (3,)).astype(np.uint8)
    msk = np.zeros(crop, np.uint8)
    aug = SegAugment(*crop, aug_gamma=[0.5, 2.0], aug_blur_sigma=[0.3, 2.5], aug_noise_std=[1.0, 20.0])
    loader = DeviceAugLoader(None, 2, gpu, data=DeviceDataset.from_arrays([img], [msk], gpu), aug=aug)
    prms = [_base_record(*crop, crop, vflip=True, **fields), _base_record(*crop, crop, hflip=True)]
    x, m = loader.batch([0, 0], prms)
    ref = [_with_records(aug, [p])(img, msk.astype(np.int64))[0] for p in prms]
    torch.cuda.synchronize()
    assert torch.equal(x[1].cpu(), ref[1])                      # the sample without an op is copied through
    a, b = _levels(x[:1], aug), _levels(ref[0][None], aug)
    diff = (a - b).abs()
    print(f'{name}: max {diff.max().item():.0f} level, {(diff > 0).float().mean().item():.2e} of the values differ')
    assert diff.max().item() <= 1
    assert (diff > 0).float().mean().item() <= 1e-3


def _full(split):
    ds = _dataset(split, randscale=[-0.5, 1.0], jitter=0.5, **ALL_ON)
    ds.transform.jitter_p = 1.0
    return ds


def test_full_pipeline_matches_host(gpu, split):
    """Scale, jitter and every new op on every sample, within the bounds of the existing comparison (which cover
    the contracted resize arithmetic)."""
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader, reference_batch
    ds = _full(split)
    aug = ds.transform
    loader = DeviceAugLoader(ds, 6, gpu, seed=3)
    scaled = 0
    for rep in range(3):
        idx = list(range(len(ds)))
        random.Random(rep).shuffle(idx)
        prms = [aug.sample_params(*loader.data.shapes[i]) for i in idx]
        assert all(p[k] is not None for p in prms for k in NEW_KEYS) and all(p['jittered'] for p in prms)
        scaled += sum(p['scaled'] for p in prms)
        x, m = loader.batch(idx, prms)
        xr, mr = reference_batch(aug, ds, idx, prms)
        torch.cuda.synchronize()
        d = (x.cpu() - xr).abs()
        print(f'rep {rep}: max {d.max().item() / LEVEL:.2f} levels, mean {d.mean().item() / LEVEL:.4f}, mask '
              f'{(m.cpu() != mr).float().mean().item():.2e}')
        assert d.max().item() < 2.5 * LEVEL
        assert d.mean().item() < 0.02 * LEVEL
        assert (m.cpu() != mr).float().mean().item() < 1e-3
    assert scaled >= 4          # both scale directions took part


def test_same_records_give_the_same_bits(gpu, split):
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader
    ds = _full(split)
    loader = DeviceAugLoader(ds, 6, gpu, seed=3)
    idx = list(range(len(ds)))
    prms = [ds.transform.sample_params(*loader.data.shapes[i]) for i in idx]
    x1, m1 = loader.batch(idx, prms)
    x2, m2 = loader.batch(idx, prms)
    assert torch.equal(x1, x2) and torch.equal(m1, m2)


def test_device_loader_epoch_with_all_options(gpu, tmp_path):
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader
    _make_split(tmp_path, [(80, 80)] * 10)
    ds = _dataset(tmp_path, crop=(64, 64), randscale=[-0.5, 1.0], jitter=0.3, **ALL_ON)
    loader = DeviceAugLoader(ds, 4, gpu, seed=1)
    batches = list(loader)
    assert len(batches) == 2 and loader.ex_batches == 2
    for x, m in batches:
        assert x.shape == (4, 3, 64, 64) and m.shape == (4, 64, 64) and x.is_cuda
        assert torch.isfinite(x).all() and set(m.unique().tolist()) <= {0, 1}


def test_trainer_steps_with_the_options_on(gpu, tmp_path):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    from medical_segmentation_pytorch_amd.core import SegTrainer
    from medical_segmentation_pytorch_amd.datasets.device_loader import DeviceAugLoader
    c = MyConfig()
    c.model, c.base_channel = 'ducknet', 17
    c.data_root, c.save_dir = str(tmp_path / 'data'), str(tmp_path / 'save')
    c.synthetic_data, c.synthetic_num, c.synthetic_size = True, (16, 4, 4), 64
    c.crop_size, c.train_bs, c.val_bs, c.base_workers = 64, 4, 2, 0
    c.total_epoch, c.warmup_epochs, c.progress_bar, c.log_interval = 1, 0, False, 3
    c.graph_warmup = 2
    for k, v in ALL_ON.items():
        setattr(c, k, v)
    c.init_dependent_config()
    t = SegTrainer(c)
    t.run(c)
    assert isinstance(t.train_loader, DeviceAugLoader) and t.train_loader.aug.medical
    assert t.train_itrs >= 3 and t.train_loader.ex_batches >= 3
    assert torch.isfinite(torch.tensor(t.last_loss))
