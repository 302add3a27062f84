"""Rotation / shift / elastic warp and gamma / blur / noise augmentation: the specification in
``utils/transforms.py`` (host path and oracle of the HIP kernels), its random draws, the config fields and the
parser flags.  No GPU."""
import json
import os

import numpy as np
import pytest

from medical_segmentation_pytorch_amd.utils import transforms as T
from medical_segmentation_pytorch_amd.utils.transforms import SegAugment

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_parent_draws.json')
ALL_ON = dict(aug_rotate=30.0, aug_shift=0.1, aug_affine_p=1.0, aug_elastic_sigma=3.0, aug_elastic_cells=4,
              aug_elastic_p=1.0, aug_gamma=[0.7, 1.5], aug_gamma_p=1.0, aug_blur_sigma=[0.5, 2.5], aug_blur_p=1.0,
              aug_noise_std=[2.0, 10.0], aug_noise_p=1.0)


def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    msk = ((((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2) < 1).astype(np.int64)
    return img, msk


def _with_records(aug, prms):
    """``aug`` evaluating the given records instead of drawing (as ``device_loader.reference_batch`` does)."""
    it = iter(prms)
    aug.sample_params = lambda h, w: next(it)
    return aug


def _base_record(h, w, crop, **kw):
    ch, cw = crop
    ph, pw = max(ch - h, 0), max(cw - w, 0)
    prm = {'nh': h, 'nw': w, 'scaled': False, 'pad': (ph // 2, ph - ph // 2, pw // 2, pw - pw // 2), 'y0': 0, 'x0': 0,
           'jittered': False, 'ops': [], 'hflip': False, 'vflip': False}
    prm.update(kw)
    return prm


def _lattice(n, seed, sigma=3.0):
    rng = np.random.default_rng(seed)
    return {'n': n, 'dy': (rng.standard_normal((n + 3, n + 3)) * sigma).astype(np.float32),
            'dx': (rng.standard_normal((n + 3, n + 3)) * sigma).astype(np.float32)}


# ---- random draws -------------------------------------------------------------------------------------------
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _plain(rec):
    """A record as JSON stores it (tuples as lists)."""
    return json.loads(json.dumps(rec))


@pytest.mark.parametrize('case', ['full', 'plain'])
def test_options_off_draws_are_the_recorded_ones(case):
    """Records and RNG state of the pipeline with every new option at its default, against draws recorded from the
    code before the options existed (tests/golden/augment_parent_draws.json)."""
    g = _golden()
    aug = SegAugment(*g['crop'], **g['cases'][case]['kwargs'])
    assert not aug.medical
    aug.seed(g['seed'])
    recs = [aug.sample_params(h, w) for h, w in g['shapes']]
    assert _plain(recs) == g['cases'][case]['records']
    assert aug.rng.random() == g['cases'][case]['next_random']


def test_new_draws_come_after_the_existing_ones():
    g = _golden()
    kw = g['cases']['full']['kwargs']
    aug = SegAugment(*g['crop'], **kw, **{**ALL_ON, 'aug_affine_p': 0.5, 'aug_elastic_p': 0.5, 'aug_gamma_p': 0.5,
                                         'aug_blur_p': 0.5, 'aug_noise_p': 0.5})
    assert aug.medical
    # every sample draws from a fresh, identically seeded generator in both pipelines: the new draws of one sample
    # come after ITS existing ones
    off = SegAugment(*g['crop'], **kw)
    for k, (h, w) in enumerate(g['shapes']):
        aug.seed(100 + k)
        off.seed(100 + k)
        a, b = aug.sample_params(h, w), off.sample_params(h, w)
        assert {key: a[key] for key in b} == b
        assert set(a) - set(b) == {'affine', 'elastic', 'gamma', 'blur', 'noise'}


def test_draw_order_and_ranges():
    """affine (p, theta, ty, tx), elastic (p, dy lattice, dx lattice), gamma, blur, noise (p, std, key), in that
    order, from the generator state that the existing draws leave behind."""
    aug = SegAugment(64, 80, **ALL_ON)
    aug.seed(5)
    p = aug.sample_params(64, 80)
    off = SegAugment(64, 80)
    off.seed(5)
    off.sample_params(64, 80)
    rng = off.rng
    assert rng.random() < 1.0
    th, ty, tx = rng.uniform(-30.0, 30.0), rng.uniform(-0.1, 0.1) * 64, rng.uniform(-0.1, 0.1) * 80
    assert p['affine'] == (th, ty, tx)
    assert rng.random() < 1.0
    dy = [rng.gauss(0.0, 3.0) for _ in range(49)]
    dx = [rng.gauss(0.0, 3.0) for _ in range(49)]
    assert p['elastic']['n'] == 4
    assert np.array_equal(p['elastic']['dy'], np.asarray(dy, np.float32).reshape(7, 7))
    assert np.array_equal(p['elastic']['dx'], np.asarray(dx, np.float32).reshape(7, 7))
    assert rng.random() < 1.0
    assert p['gamma'] == rng.uniform(0.7, 1.5)
    assert rng.random() < 1.0
    assert p['blur'] == rng.uniform(0.5, 2.5)
    assert rng.random() < 1.0
    assert p['noise'] == (rng.uniform(2.0, 10.0), rng.getrandbits(64))
    assert aug.rng.random() == rng.random()


# ---- warp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,scaled', [((96, 128), False), ((48, 70), False), ((150, 90), True)])
def test_identity_warp_is_the_unwarped_pipeline(size, scaled):
    img, msk = _image(*size)
    aug = SegAugment(64, 80, randscale=[-0.5, 1.0], h_flip=1.0, aug_rotate=10.0, aug_elastic_sigma=2.0)
    off = SegAugment(64, 80, randscale=[-0.5, 1.0], h_flip=1.0)
    off.seed(3)
    prm = off.sample_params(*size)
    if scaled:
        prm.update(nh=100, nw=61, scaled=True, pad=(0, 0, 9, 10), y0=17, x0=0)
    x0, m0 = _with_records(off, [prm])(img, msk)
    forced = dict(prm, affine=(0.0, 0.0, 0.0), elastic={'n': 4, 'dy': np.zeros((7, 7), np.float32),
                                                         'dx': np.zeros((7, 7), np.float32)})
    x1, m1 = _with_records(aug, [forced])(img, msk)
    assert np.array_equal(x0.numpy(), x1.numpy()) and np.array_equal(m0.numpy(), m1.numpy())


@pytest.mark.parametrize('theta,k', [(90.0, 1), (-90.0, 3), (180.0, 2)])
def test_rotation_by_quarter_turns_is_rot90(theta, k):
    img, msk = _image(48, 48, seed=1)
    aug = SegAugment(48, 48, aug_rotate=180.0)
    prm = _base_record(48, 48, (48, 48), affine=(theta, 0.0, 0.0))
    x, m = _with_records(aug, [prm])(img, msk)
    ref = T.normalize_to_tensor(np.rot90(img, k).astype(np.float32), aug.mean, aug.std)
    assert np.array_equal(x.numpy(), ref.numpy())
    assert np.array_equal(m.numpy(), np.rot90(msk, k))


def test_warp_matches_map_coordinates():
    from scipy import ndimage
    img, msk = _image(96, 128, seed=2)
    prm = _base_record(96, 128, (64, 80), y0=32, x0=48, affine=(25.0, 5.5, -7.25), elastic=_lattice(4, 7))
    fy, fx = T.warp_coords(prm, (64, 80))
    assert fy.dtype == np.float32 and fx.dtype == np.float32
    assert fy.min() < 0 or fx.min() < 0 or fy.max() > 95 or fx.max() > 127     # the border rule is exercised
    pre, mk = T.warp_gather(img, msk, fy, fx, 'reflect')
    coords = np.stack([fy.astype(np.float64), fx.astype(np.float64)])
    for c in range(3):
        ref = ndimage.map_coordinates(img[..., c].astype(np.float64), coords, order=1, mode='mirror')
        assert np.abs(pre[..., c] - ref).max() < 1e-3
    near = ndimage.map_coordinates(msk.astype(np.float64), coords, order=0, mode='mirror')
    clear = (np.abs(fy - np.floor(fy) - 0.5) > 1e-3) & (np.abs(fx - np.floor(fx) - 0.5) > 1e-3)
    assert clear.mean() > 0.99
    assert np.array_equal(mk[clear], near[clear].astype(mk.dtype))


@pytest.mark.parametrize('n', [1, 4, 8])
def test_bspline_partition_of_unity(n):
    """A constant control lattice displaces every pixel by that constant: a pure translation."""
    lat = np.full((n + 3, n + 3), 3.0, np.float32)
    d = T.bspline_displacement(lat, n, 64, 80)
    assert d.shape == (64, 80) and np.abs(d - 3.0).max() < 1e-5
    img, msk = _image(96, 128, seed=3)
    aug = SegAugment(64, 80, aug_elastic_sigma=1.0, aug_elastic_cells=n)
    moved = _base_record(96, 128, (64, 80), y0=10, x0=20, elastic={'n': n, 'dy': lat, 'dx': -lat})
    x, m = _with_records(aug, [moved])(img, msk)
    x0, m0 = _with_records(SegAugment(64, 80), [_base_record(96, 128, (64, 80), y0=13, x0=17)])(img, msk)
    assert np.array_equal(x.numpy(), x0.numpy()) and np.array_equal(m.numpy(), m0.numpy())


def test_constant_border_is_zero_outside_the_image():
    img = np.random.default_rng(4).integers(100, 256, (40, 40, 3)).astype(np.uint8)
    msk = np.ones((40, 40), np.int64)
    aug = SegAugment(64, 64, aug_rotate=45.0, aug_border='constant')
    prm = _base_record(40, 40, (64, 64), affine=(45.0, 0.0, 0.0))
    assert prm['pad'] == (12, 12, 12, 12)
    fy, fx = T.warp_coords(prm, (64, 64))
    pre, mk = T.warp_gather(img, msk, fy, fx, 'constant')
    outside = (fy <= -1) | (fy >= 40) | (fx <= -1) | (fx >= 40)          # all four neighbours outside
    inside = (fy >= 0) & (fy <= 39) & (fx >= 0) & (fx <= 39)             # all four inside
    assert outside.mean() > 0.2 and inside.mean() > 0.2
    x, m = _with_records(aug, [prm])(img, msk)
    raw = x.numpy().transpose(1, 2, 0) * aug.std + aug.mean
    assert np.abs(raw[outside]).max() < 1e-3 and raw[inside].min() > 99.0
    ry, rx = np.rint(fy), np.rint(fx)
    m_out = (ry < 0) | (ry > 39) | (rx < 0) | (rx > 39)
    assert np.array_equal(m.numpy() == 0, m_out)
    # reflect mode never produces the fill value from this image
    xr, mr = _with_records(SegAugment(64, 64, aug_rotate=45.0), [prm])(img, msk)
    assert (xr.numpy().transpose(1, 2, 0) * aug.std + aug.mean).min() > 99.0 and mr.min() == 1


# ---- intensity ----------------------------------------------------------------------------------------------
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,out', PHILOX_KAT)
def test_philox_known_answers(ctr, key, out):
    got = T.philox4x32(np.array([ctr], np.uint32), key)
    assert tuple(int(v) for v in got[0]) == out


def test_noise_normals_statistics():
    std = 7.5
    z = T.noise_normals(0x0123456789abcdef, 64, 64).astype(np.float64) * std
    n = z.size
    assert n == 64 * 64 * 3
    assert abs(z.mean()) < 5 * std / np.sqrt(n)
    assert abs(z.std() - std) < 5 * std / np.sqrt(2 * n)
    # the three channels of a pixel and neighbouring pixels are distinct draws
    assert len(np.unique(z)) > 0.99 * n


def test_noise_counter_is_the_output_pixel():
    """The noise field belongs to the output frame: flipping the sample does not flip the noise."""
    img, msk = _image(64, 80, seed=5)
    img[:] = 128
    aug = SegAugment(64, 80, aug_noise_std=[5.0, 5.0])
    base = _base_record(64, 80, (64, 80), noise=(5.0, 99))
    a, _ = _with_records(aug, [base])(img, msk)
    b, _ = _with_records(aug, [dict(base, hflip=True, vflip=True)])(img, msk)
    assert np.array_equal(a.numpy(), b.numpy())


def test_gamma_one_is_identity():
    img, msk = _image(64, 80, seed=6)
    aug = SegAugment(64, 80, aug_gamma=[1.0, 1.0])
    base = _base_record(64, 80, (64, 80))
    a, _ = _with_records(aug, [base])(img, msk)
    b, _ = _with_records(aug, [dict(base, gamma=1.0)])(img, msk)
    assert np.array_equal(a.numpy(), b.numpy())
    dark = T.gamma_op(np.full((2, 2, 3), 64.0, np.float32), 2.0)
    assert np.allclose(dark, 255.0 * (64.0 / 255.0) ** 2, atol=1e-3)


@pytest.mark.parametrize('sigma,radius', [(0.3, 1), (1.0, 3), (2.5, 8)])
def test_blur_matches_correlate1d(sigma, radius):
    from scipy import ndimage
    assert T.blur_radius(sigma) == radius
    taps = T.blur_taps(sigma)
    assert taps.dtype == np.float32 and len(taps) == radius + 1
    full = np.concatenate([taps[:0:-1], taps]).astype(np.float64)
    assert abs(full.sum() - 1.0) < 1e-6
    img = np.random.default_rng(7).integers(0, 256, (33, 47, 3)).astype(np.float32)
    got = T.gaussian_blur(img, taps)
    ref = ndimage.correlate1d(img.astype(np.float64), full, axis=1, mode='mirror')
    ref = ndimage.correlate1d(ref, full, axis=0, mode='mirror')
    assert np.abs(got - ref).max() < 1e-3
    # symmetric taps: the blur commutes with the flips exactly
    assert np.array_equal(T.gaussian_blur(img[::-1, ::-1], taps), got[::-1, ::-1])


def intensity_cases():
    """(name, crop, record fields) of the gamma / blur / noise comparisons; the GPU tests use the same list."""
    return [('gamma', (64, 80), {'gamma': 0.6}), ('gamma_hi', (64, 80), {'gamma': 1.7}),
            ('blur_r8', (33, 47), {'blur': 2.5}), ('blur_r1', (33, 47), {'blur': 0.3}),
            ('noise', (64, 80), {'noise': (12.0, 0x9e3779b97f4a7c15)}),
            ('all', (64, 80), {'gamma': 1.3, 'blur': 1.2, 'noise': (6.0, 0x0123456789abcdef)}),
            ('all_small', (33, 47), {'gamma': 0.8, 'blur': 2.5, 'noise': (20.0, 7)})]


@pytest.mark.parametrize('name,crop,fields', intensity_cases())
def test_fp32_and_fp64_specification_agree(name, crop, fields):
    """Only values within the arithmetic's error of a rounding tie can differ between an fp32 and an fp64
    evaluation of the specification: fewer than 1e-3 of them, on the inputs of the GPU comparison."""
    img = np.random.default_rng(8).integers(0, 256, crop + (3,)).astype(np.float32)
    prm = dict(fields, hflip=False, vflip=True)
    a = np.round(T.medical_intensity(img, prm, np.float32))
    b = np.round(T.medical_intensity(img, prm, np.float64))
    diff = a != b
    print(f'{name}: {diff.mean():.2e} of the values differ, max {np.abs(a - b).max():.0f} level')
    assert np.abs(a - b).max() <= 1 and diff.mean() < 1e-3


def test_intensity_order_and_single_rounding():
    img, msk = _image(64, 80, seed=9)
    aug = SegAugment(64, 80, **ALL_ON)
    prm = _base_record(64, 80, (64, 80), gamma=1.4, blur=1.0, noise=(4.0, 11), hflip=True)
    x, _ = _with_records(aug, [prm])(img, msk)
    v = T.gamma_op(img.astype(np.float32), 1.4)
    v = T.gaussian_blur(v, T.blur_taps(1.0))
    v = np.clip(v + T.noise_normals(11, 64, 80)[:, ::-1] * np.float32(4.0), 0, 255)
    ref = T.normalize_to_tensor(np.round(v)[:, ::-1], aug.mean, aug.std)
    assert np.array_equal(x.numpy(), ref.numpy())


def test_host_pipeline_runs_with_everything_on():
    img, msk = _image(150, 90, seed=10)
    aug = SegAugment(64, 80, randscale=[-0.5, 1.0], brightness=0.5, contrast=0.5, saturation=0.5, h_flip=0.5,
                     v_flip=0.5, **ALL_ON)
    aug.seed(0)
    for _ in range(4):
        x, m = aug(img, msk)
        assert x.shape == (3, 64, 80) and m.shape == (64, 80)
        assert np.isfinite(x.numpy()).all() and set(np.unique(m.numpy())) <= {0, 1}


# ---- config and parser --------------------------------------------------------------------------------------
def _config(**kw):
    from medical_segmentation_pytorch_amd.configs import MyConfig
    c = MyConfig()
    c.crop_size = 64
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_config_defaults_are_off():
    c = _config().init_dependent_config()
    assert (c.aug_rotate, c.aug_shift, c.aug_elastic_sigma, c.aug_gamma, c.aug_blur_sigma, c.aug_noise_std) == \
        (0.0, 0.0, 0.0, None, None, None)
    assert (c.aug_affine_p, c.aug_elastic_p, c.aug_gamma_p, c.aug_blur_p, c.aug_noise_p) == (0.5,) * 5
    assert c.aug_elastic_cells == 4 and c.aug_border == 'reflect'


@pytest.mark.parametrize('field,value', [
    ('aug_rotate', -1.0), ('aug_rotate', 200.0), ('aug_shift', -0.1), ('aug_shift', 1.5), ('aug_affine_p', 1.2),
    ('aug_elastic_sigma', -1.0), ('aug_elastic_cells', 0), ('aug_elastic_cells', 9), ('aug_elastic_cells', 2.5),
    ('aug_elastic_p', -0.1), ('aug_border', 'wrap'), ('aug_gamma', [0.0, 1.0]), ('aug_gamma', [1.5, 0.5]),
    ('aug_gamma', [1.0]), ('aug_gamma_p', 2.0), ('aug_blur_sigma', [0.5, 2.6]), ('aug_blur_sigma', [0.0, 1.0]),
    ('aug_blur_p', -1.0), ('aug_noise_std', [-1.0, 5.0]), ('aug_noise_std', [0.0, 300.0]), ('aug_noise_p', 1.5)])
def test_config_rejects_out_of_range(field, value):
    with pytest.raises(ValueError, match=field):
        _config(**{field: value}).init_dependent_config()


def test_config_checks_blur_radius_against_crop():
    _config(aug_blur_sigma=[0.5, 2.5]).init_dependent_config()                # radius 8 in a 64 crop
    with pytest.raises(ValueError, match='aug_blur_sigma'):
        _config(crop_size=16, aug_blur_sigma=[0.5, 2.5]).init_dependent_config()
    with pytest.raises(ValueError):
        SegAugment(16, 64, aug_blur_sigma=[0.5, 2.5])


def test_parser_flags_reach_the_config():
    from medical_segmentation_pytorch_amd.configs.parser import load_parser
    c = load_parser(_config(), ['--aug_rotate', '20', '--aug_shift', '0.1', '--aug_affine_p', '0.7',
                                '--aug_elastic_sigma', '4', '--aug_elastic_cells', '6', '--aug_elastic_p', '0.3',
                                '--aug_border', 'constant', '--aug_gamma', '0.7', '1.5', '--aug_gamma_p', '0.2',
                                '--aug_blur_sigma', '0.5', '1.5', '--aug_blur_p', '0.1', '--aug_noise_std', '0', '8',
                                '--aug_noise_p', '0.9'])
    assert (c.aug_rotate, c.aug_shift, c.aug_affine_p) == (20.0, 0.1, 0.7)
    assert (c.aug_elastic_sigma, c.aug_elastic_cells, c.aug_elastic_p, c.aug_border) == (4.0, 6, 0.3, 'constant')
    assert (c.aug_gamma, c.aug_gamma_p) == ((0.7, 1.5), 0.2)
    assert (c.aug_blur_sigma, c.aug_blur_p) == ((0.5, 1.5), 0.1)
    assert (c.aug_noise_std, c.aug_noise_p) == ((0.0, 8.0), 0.9)


def test_dataset_passes_the_fields_and_tolerates_their_absence(tmp_path):
    from types import SimpleNamespace
    from medical_segmentation_pytorch_amd.datasets.polyp import PolypDataset
    for sub in ('images', 'masks'):
        (tmp_path / 'train' / sub).mkdir(parents=True)
    old = SimpleNamespace(data_root=str(tmp_path), crop_h=64, crop_w=80, randscale=[-0.5, 1.0], brightness=0.5,
                          contrast=0.5, saturation=0.5, h_flip=0.5, v_flip=0.5, num_class=2)
    assert not PolypDataset(old, 'train').transform.medical
    new = SimpleNamespace(**vars(old), aug_rotate=15.0, aug_blur_sigma=(0.5, 1.0), aug_border='constant')
    t = PolypDataset(new, 'train').transform
    assert t.medical and t.rotate == 15.0 and t.blur_sigma == (0.5, 1.0) and t.border == 'constant'
