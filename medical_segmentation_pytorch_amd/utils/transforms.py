"""Data augmentation with the reference's albumentations 1.3.0 semantics (SURVEY Appendix D;
reference ``datasets/polyp.py:37-53``, ``utils/transforms.py:11-32``), implemented natively
(albumentations / OpenCV are not available):

  RandomScale(scale_limit, p=0.5)   factor ~ U[1+lo, 1+hi]; image bilinear, mask nearest
  PadIfNeeded(h, w)                 centred BORDER_REFLECT_101 padding
  RandomCrop(h, w)
  ColorJitter(b, c, s, hue=0.2, p=0.5)  factors ~ U[max(0,1-x), 1+x], random order
  HorizontalFlip(p), VerticalFlip(p)
  Normalize(ImageNet mean/std, max_pixel 255) + ToTensor (HWC -> CHW; mask stays HW)

Additions of this project, each off at its default (the medical-imaging staples of nnU-Net / MONAI
``Rand2DElastic`` / albumentations ``ShiftScaleRotate``): rotation + shift and a cubic B-spline free-form
deformation, composed with the crop and the flips into ONE inverse-map gather, then gamma, Gaussian blur and
Gaussian noise after ColorJitter.  The functions below are the specification: the host path, and the oracle
``csrc/augment.hip`` is checked against on the same parameter records.
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def to_numpy(array):
    if not isinstance(array, np.ndarray):
        array = np.asarray(array)
    return array


def resize(img, h, w, mode='bilinear'):
    """HWC uint8/float or HW array -> resized (cv2.INTER_LINEAR / INTER_NEAREST equivalents)."""
    t = torch.from_numpy(np.ascontiguousarray(img))
    squeeze = t.dim() == 2
    if squeeze:
        t = t[..., None]
    x = t.permute(2, 0, 1)[None].float()
    if mode == 'nearest':
        y = F.interpolate(x, size=(h, w), mode='nearest')
    else:
        y = F.interpolate(x, size=(h, w), mode='bilinear', align_corners=False)
    y = y[0].permute(1, 2, 0)
    if img.dtype == np.uint8:
        y = y.round().clamp(0, 255).to(torch.uint8)
    else:
        y = y.to(torch.from_numpy(np.zeros(0, dtype=img.dtype)).dtype)
    y = y.numpy()
    return y[..., 0] if squeeze else y


class Scale:
    """Deterministic resize by ``scale`` (reference utils/transforms.py:11-32)."""

    def __init__(self, scale, interpolation=1, p=1, is_testing=False):
        self.scale, self.interpolation, self.p, self.is_testing = scale, interpolation, p, is_testing

    def __call__(self, image, mask=None):
        img = to_numpy(image)
        h, w = img.shape[:2]
        nh, nw = int(h * self.scale), int(w * self.scale)
        out = {'image': resize(img, nh, nw, 'nearest' if self.interpolation == 0 else 'bilinear')}
        if not self.is_testing and mask is not None:
            out['mask'] = resize(to_numpy(mask), nh, nw, 'nearest')
        return out


def _reflect101_pad(a, top, bottom, left, right):
    pad = [(top, bottom), (left, right)] + [(0, 0)] * (a.ndim - 2)
    return np.pad(a, pad, mode='reflect')   # numpy 'reflect' == OpenCV BORDER_REFLECT_101


def _gray(img):
    return img[..., 0] * 0.299 + img[..., 1] * 0.587 + img[..., 2] * 0.114


def _adjust_hue(img, shift):
    """Hue rotation in HSV space (shift in [-0.5, 0.5] of a full turn); img float RGB 0..255."""
    x = img / 255.0
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mx, mn = x.max(-1), x.min(-1)
    d = mx - mn
    h = np.zeros_like(mx)
    m = d > 1e-12
    rc = np.where(m, (mx - r) / np.where(m, d, 1), 0)
    gc = np.where(m, (mx - g) / np.where(m, d, 1), 0)
    bc = np.where(m, (mx - b) / np.where(m, d, 1), 0)
    h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc))
    h = (h / 6.0) % 1.0
    h = np.where(m, h, 0)
    s = np.where(mx > 1e-12, d / np.where(mx > 1e-12, mx, 1), 0)
    v = mx
    h = (h + shift) % 1.0
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    i = i.astype(np.int32) % 6
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]),
                    np.choose(i, [p, p, t, v, v, q])], -1)
    return out * 255.0


# ---------------------------------------------------------------------------------------------------
# Warp (rotation / shift / B-spline deformation) -- fp32 arithmetic in ONE written-down order, which
# ``aug_warp_kernel`` repeats with contraction off, so an unscaled warp is reproduced bit for bit.
AUG_MAX_CELLS = 8          # B-spline cells per axis; the control lattice is (n + 3) x (n + 3)
BLUR_MAX_RADIUS = 8
BLUR_MAX_SIGMA = 2.5
_F = np.float32
_COORD_LIMIT = _F(32768.0)   # coordinates are clamped here before the float -> int conversion


def affine_matrix(theta_deg, ty, tx, crop_h, crop_w):
    """fp32 [2, 3] matrix M of the inverse map q = c + R(theta)^T (p - c - t) written as q = A p + b with
    A = R^T, b = c - A (c + t); p = (cy, cx) crop pixel, rows (y, x).  Positive theta turns the picture
    counter-clockwise on the screen (``np.rot90`` direction).  cos / sin are taken in fp64 and rounded once;
    values below 1e-12 snap to 0 so that multiples of 90 degrees are exact."""
    th = math.radians(float(theta_deg))
    c, s = math.cos(th), math.sin(th)
    c, s = (0.0 if abs(c) < 1e-12 else c), (0.0 if abs(s) < 1e-12 else s)
    a = np.array([[c, s], [-s, c]], np.float64)      # rows (y, x), y pointing down
    ctr = np.array([(crop_h - 1) / 2.0, (crop_w - 1) / 2.0], np.float64)
    b = ctr - a @ (ctr + np.array([float(ty), float(tx)]))
    return np.concatenate([a, b[:, None]], 1).astype(np.float32)


def _bspline_basis(u):
    """Uniform cubic B-spline basis B0..B3 at fp32 ``u`` in [0, 1) (fixed fp32 operation order)."""
    sixth = _F(1.0 / 6.0)
    t = _F(1) - u
    u2 = u * u
    u3 = u2 * u
    b0 = ((t * t) * t) * sixth
    b1 = ((_F(3) * u3 - _F(6) * u2) + _F(4)) * sixth
    b2 = ((((_F(-3) * u3) + _F(3) * u2) + _F(3) * u) + _F(1)) * sixth
    b3 = u3 * sixth
    return b0, b1, b2, b3


def bspline_displacement(lattice, n, crop_h, crop_w):
    """d(p) = sum_ab B_a(u_y) B_b(u_x) P[i+a][j+b] for every crop pixel; ``lattice`` fp32 [(n+3), (n+3)]."""
    lattice = np.asarray(lattice, np.float32).reshape(n + 3, n + 3)
    sy = np.arange(crop_h, dtype=np.float32) * _F(n / crop_h)
    sx = np.arange(crop_w, dtype=np.float32) * _F(n / crop_w)
    iy = np.minimum(np.floor(sy), n - 1).astype(np.int64)
    ix = np.minimum(np.floor(sx), n - 1).astype(np.int64)
    by = _bspline_basis(sy - iy.astype(np.float32))
    bx = _bspline_basis(sx - ix.astype(np.float32))
    rows = []
    for a in range(4):
        p = [lattice[(iy + a)[:, None], (ix + b)[None, :]] for b in range(4)]
        rows.append(((bx[0][None] * p[0] + bx[1][None] * p[1]) + bx[2][None] * p[2]) + bx[3][None] * p[3])
    return ((by[0][:, None] * rows[0] + by[1][:, None] * rows[1]) + by[2][:, None] * rows[2]) + by[3][:, None] * rows[3]


def warp_coords(prm, crop):
    """fp32 coordinate maps (fy, fx), in the SCALED image, of every crop pixel of a warping sample:
    q = (m0 cy + m1 cx) + m2, + d(p) when elastic, + (crop origin - pad) ; clamped to +-32768."""
    ch, cw = crop
    cy = np.arange(ch, dtype=np.float32)[:, None]
    cx = np.arange(cw, dtype=np.float32)[None, :]
    aff = prm.get('affine')
    m = affine_matrix(*aff, ch, cw) if aff is not None else affine_matrix(0.0, 0.0, 0.0, ch, cw)
    qy = (m[0, 0] * cy + m[0, 1] * cx) + m[0, 2]
    qx = (m[1, 0] * cy + m[1, 1] * cx) + m[1, 2]
    el = prm.get('elastic')
    if el is not None:
        qy = qy + bspline_displacement(el['dy'], el['n'], ch, cw)
        qx = qx + bspline_displacement(el['dx'], el['n'], ch, cw)
    t, _, l, _ = prm['pad']
    fy = qy + _F(prm['y0'] - t)
    fx = qx + _F(prm['x0'] - l)
    return np.clip(fy, -_COORD_LIMIT, _COORD_LIMIT), np.clip(fx, -_COORD_LIMIT, _COORD_LIMIT)


def _reflect101_index(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def warp_gather(img, msk, fy, fx, border='reflect'):
    """Sample the (scaled) uint8 image bilinearly and the mask at the nearest integer coordinate; neighbours
    outside the image come through the border rule.  Returns (fp32 image BEFORE the uint8 rounding, mask)."""
    h, w = msk.shape
    y0f, x0f = np.floor(fy), np.floor(fx)
    ly, lx = fy - y0f, fx - x0f
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    my, mx = np.rint(fy).astype(np.int64), np.rint(fx).astype(np.int64)

    def fetch(a, yy, xx):
        if border == 'reflect':
            return a[_reflect101_index(yy, h), _reflect101_index(xx, w)]
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None] if v.ndim == 3 else inside, v, 0)

    v00, v01 = fetch(img, y0, x0).astype(np.float32), fetch(img, y0, x0 + 1).astype(np.float32)
    v10, v11 = fetch(img, y0 + 1, x0).astype(np.float32), fetch(img, y0 + 1, x0 + 1).astype(np.float32)
    ly, lx = ly[..., None], lx[..., None]
    one = _F(1)
    out = (one - ly) * ((one - lx) * v00 + lx * v01) + ly * ((one - lx) * v10 + lx * v11)
    return out, fetch(msk, my, mx)


# ---------------------------------------------------------------------------------------------------
# Intensity: gamma, Gaussian blur, Gaussian noise (``dtype``: fp32 is the specification; fp64 measures how
# many values sit close enough to a rounding tie for the arithmetic's last bits to decide them)
def gamma_op(img, g, dtype=np.float32):
    x = np.asarray(img, dtype)
    return np.clip(dtype(255) * np.power(x / dtype(255), dtype(g)), 0, 255)


def blur_radius(sigma):
    return min(int(math.ceil(3.0 * float(sigma))), BLUR_MAX_RADIUS)


def blur_taps(sigma):
    """fp32 taps w[0..r] of the symmetric kernel: exp(-k^2 / 2 sigma^2), normalised by the sum over
    k = -r..r accumulated in fp32 in index order."""
    r = blur_radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float32)
    e = np.exp(-(k * k) / _F(2.0 * float(sigma) * float(sigma))).astype(np.float32)
    tot = _F(0)
    for v in e:
        tot = _F(tot + v)
    return (e[r:] / tot).astype(np.float32)


def gaussian_blur(img, taps, dtype=np.float32):
    """Separable blur, rows then columns, reflect-101 inside the crop.  Each output is
    w0 x[i] + sum_k w_k (x[i-k] + x[i+k]), k ascending: symmetric, so it commutes with the flips exactly."""
    x = np.asarray(img, dtype)
    taps = np.asarray(taps, dtype)
    r = len(taps) - 1
    for axis in (1, 0):
        n = x.shape[axis]
        idx = np.arange(n)
        acc = taps[0] * x
        for k in range(1, r + 1):
            lo = np.take(x, _reflect101_index(idx - k, n), axis)
            hi = np.take(x, _reflect101_index(idx + k, n), axis)
            acc = acc + taps[k] * (lo + hi)
        x = acc
    return np.clip(x, 0, 255)


_PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 (Salmon et al., SC'11): ``counter`` [..., 4], ``key`` [..., 2] uint32 -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & _MASK32 for i in range(4)]
    k = [int(v) & 0xFFFFFFFF for v in np.asarray(key).reshape(-1)[:2]]
    sh = np.uint64(32)
    for r in range(rounds):
        k0 = np.uint64((k[0] + r * _PHILOX_W[0]) & 0xFFFFFFFF)
        k1 = np.uint64((k[1] + r * _PHILOX_W[1]) & 0xFFFFFFFF)
        p0, p1 = _PHILOX_M[0] * c[0], _PHILOX_M[1] * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> sh) ^ c[3] ^ k1, p0 & _MASK32]
    return np.stack(c, -1).astype(np.uint32)


def noise_normals(key64, crop_h, crop_w, dtype=np.float32):
    """[crop_h, crop_w, 3] standard normals of the OUTPUT frame: counter (y * crop_w + x, 0, 0, 0), key (low
    word, high word) of ``key64``; the four outputs become uniforms (k + 0.5) 2^-32 and two Box-Muller pairs,
    whose first three normals go to R, G, B."""
    ctr = np.zeros((crop_h * crop_w, 4), np.uint32)
    ctr[:, 0] = np.arange(crop_h * crop_w, dtype=np.uint32)
    x = philox4x32(ctr, (key64 & 0xFFFFFFFF, (key64 >> 32) & 0xFFFFFFFF))
    u = (x.astype(dtype) + dtype(0.5)) * dtype(2.0 ** -32)
    two_pi = dtype(np.float32(2.0 * math.pi))
    r0 = np.sqrt(dtype(-2) * np.log(u[:, 0]))
    r1 = np.sqrt(dtype(-2) * np.log(u[:, 2]))
    z = np.stack([r0 * np.cos(two_pi * u[:, 1]), r0 * np.sin(two_pi * u[:, 1]), r1 * np.cos(two_pi * u[:, 3])], -1)
    return z.astype(dtype).reshape(crop_h, crop_w, 3)


def medical_intensity(img, prm, dtype=np.float32):
    """Gamma -> blur -> noise on a crop-frame RGB image (each clips to [0, 255], none rounds).  The noise
    field is defined on the output frame, so it is flipped back into the crop frame here; gamma is per
    pixel and the blur is symmetric, so evaluating them before the flips changes nothing."""
    img = np.asarray(img, dtype)
    if prm.get('gamma') is not None:
        img = gamma_op(img, prm['gamma'], dtype)
    if prm.get('blur') is not None:
        img = gaussian_blur(img, blur_taps(prm['blur']), dtype)
    if prm.get('noise') is not None:
        std, key = prm['noise']
        z = noise_normals(key, img.shape[0], img.shape[1], dtype)
        if prm['hflip']:
            z = z[:, ::-1]
        if prm['vflip']:
            z = z[::-1]
        img = np.clip(img + z * dtype(std), 0, 255)
    return img


def _pair(v, name):
    if v is None:
        return None
    v = [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v), float(v)]
    if len(v) != 2 or v[0] > v[1]:
        raise ValueError(f'{name} must be [lo, hi] with lo <= hi, got {v!r}')
    return (v[0], v[1])


class SegAugment:
    """Train-time pipeline of the reference (polyp.py:38-47); ``rng`` is a ``random.Random``."""

    def __init__(self, crop_h, crop_w, randscale=0.0, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.2,
                 h_flip=0.0, v_flip=0.0, scale_p=0.5, jitter_p=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 aug_rotate=0.0, aug_shift=0.0, aug_affine_p=0.5, aug_elastic_sigma=0.0, aug_elastic_cells=4,
                 aug_elastic_p=0.5, aug_border='reflect', aug_gamma=None, aug_gamma_p=0.5, aug_blur_sigma=None,
                 aug_blur_p=0.5, aug_noise_std=None, aug_noise_p=0.5):
        if isinstance(randscale, (list, tuple)):
            lo, hi = randscale
        else:
            lo, hi = -float(randscale), float(randscale)
        self.scale_range = (1 + lo, 1 + hi)
        self.crop = (crop_h, crop_w)
        self.jitter = (brightness, contrast, saturation, hue)
        self.h_flip, self.v_flip = h_flip, v_flip
        self.scale_p, self.jitter_p = scale_p, jitter_p
        self.mean = np.asarray(mean, np.float32) * 255.0
        self.std = np.asarray(std, np.float32) * 255.0
        # rotation / shift / elastic warp and gamma / blur / noise: every group is off at its default
        if aug_border not in ('reflect', 'constant'):
            raise ValueError(f"aug_border must be 'reflect' or 'constant', got {aug_border!r}")
        if not 1 <= int(aug_elastic_cells) <= AUG_MAX_CELLS:
            raise ValueError(f'aug_elastic_cells must be in 1..{AUG_MAX_CELLS}, got {aug_elastic_cells!r}')
        self.rotate, self.shift, self.affine_p = float(aug_rotate), float(aug_shift), aug_affine_p
        self.elastic_sigma, self.elastic_cells, self.elastic_p = float(aug_elastic_sigma), int(aug_elastic_cells), \
            aug_elastic_p
        self.border = aug_border
        self.gamma, self.gamma_p = _pair(aug_gamma, 'aug_gamma'), aug_gamma_p
        self.blur_sigma, self.blur_p = _pair(aug_blur_sigma, 'aug_blur_sigma'), aug_blur_p
        self.noise_std, self.noise_p = _pair(aug_noise_std, 'aug_noise_std'), aug_noise_p
        if self.blur_sigma is not None and (self.blur_sigma[0] <= 0 or self.blur_sigma[1] > BLUR_MAX_SIGMA or
                                            2 * blur_radius(self.blur_sigma[1]) >= min(crop_h, crop_w)):
            raise ValueError(f'aug_blur_sigma must lie in (0, {BLUR_MAX_SIGMA}] with twice the radius below the crop, '
                             f'got {aug_blur_sigma!r}')
        self.rng = random.Random()

    @property
    def medical(self):
        """True when any rotation / shift / elastic / gamma / blur / noise option is on."""
        return bool(self.rotate or self.shift or self.elastic_sigma or self.gamma or self.blur_sigma
                    or self.noise_std)

    def seed(self, s):
        self.rng.seed(s)

    def sample_params(self, h, w):
        """Draw every random number of one sample (same calls, same order as the pixel pipeline), for
        an ``h x w`` source.  The CPU pipeline (:meth:`__call__`) and the GPU one
        (``datasets.device_loader``) both evaluate these records, so a seed gives the same batch."""
        rng = self.rng
        prm = {'nh': h, 'nw': w, 'scaled': False}
        if self.scale_range != (1.0, 1.0) and rng.random() < self.scale_p:
            f = rng.uniform(*self.scale_range)
            prm.update(nh=max(int(round(h * f)), 1), nw=max(int(round(w * f)), 1), scaled=True)
        ch, cw = self.crop
        h2, w2 = prm['nh'], prm['nw']
        ph, pw = max(ch - h2, 0), max(cw - w2, 0)
        prm['pad'] = (ph // 2, ph - ph // 2, pw // 2, pw - pw // 2)
        h2, w2 = h2 + ph, w2 + pw
        prm['y0'] = rng.randint(0, h2 - ch)
        prm['x0'] = rng.randint(0, w2 - cw)
        ops = []
        b, c, s, hue = self.jitter
        jittered = bool(b or c or s or hue) and rng.random() < self.jitter_p
        if jittered:
            if b:
                ops.append(('b', rng.uniform(max(0.0, 1 - b), 1 + b)))
            if c:
                ops.append(('c', rng.uniform(max(0.0, 1 - c), 1 + c)))
            if s:
                ops.append(('s', rng.uniform(max(0.0, 1 - s), 1 + s)))
            if hue:
                ops.append(('h', rng.uniform(-hue, hue)))
            rng.shuffle(ops)
        prm['jittered'], prm['ops'] = jittered, ops
        prm['hflip'] = rng.random() < self.h_flip
        prm['vflip'] = rng.random() < self.v_flip
        # the groups below draw after everything above (a seed gives the same scale, crop, jitter and flips
        # whether or not they are on); a group that is off draws nothing and adds no field
        if self.rotate or self.shift:
            prm['affine'] = None
            if rng.random() < self.affine_p:
                prm['affine'] = (rng.uniform(-self.rotate, self.rotate), rng.uniform(-self.shift, self.shift) * ch,
                                 rng.uniform(-self.shift, self.shift) * cw)
        if self.elastic_sigma:
            prm['elastic'] = None
            if rng.random() < self.elastic_p:
                n = self.elastic_cells
                dy = [rng.gauss(0.0, self.elastic_sigma) for _ in range((n + 3) ** 2)]
                dx = [rng.gauss(0.0, self.elastic_sigma) for _ in range((n + 3) ** 2)]
                prm['elastic'] = {'n': n, 'dy': np.asarray(dy, np.float32).reshape(n + 3, n + 3),
                                  'dx': np.asarray(dx, np.float32).reshape(n + 3, n + 3)}
        if self.gamma is not None:
            prm['gamma'] = rng.uniform(*self.gamma) if rng.random() < self.gamma_p else None
        if self.blur_sigma is not None:
            prm['blur'] = rng.uniform(*self.blur_sigma) if rng.random() < self.blur_p else None
        if self.noise_std is not None:
            prm['noise'] = None
            if rng.random() < self.noise_p:
                prm['noise'] = (rng.uniform(*self.noise_std), rng.getrandbits(64))
        return prm

    def __call__(self, image, mask):
        img, msk = to_numpy(image), to_numpy(mask)
        prm = self.sample_params(*img.shape[:2])
        if prm['scaled']:
            img = resize(img, prm['nh'], prm['nw'], 'bilinear')
            msk = resize(msk, prm['nh'], prm['nw'], 'nearest')
        ch, cw = self.crop
        if prm.get('affine') is not None or prm.get('elastic') is not None:
            # pad, crop and warp are one gather from the scaled image; the result rounds as a warp of a
            # uint8 image would
            fy, fx = warp_coords(prm, self.crop)
            img, msk = warp_gather(img, msk, fy, fx, self.border)
            img = np.clip(np.rint(img), 0, 255)
        else:
            if any(prm['pad']):
                t, bt, l, r = prm['pad']
                img = _reflect101_pad(img, t, bt, l, r)
                msk = _reflect101_pad(msk, t, bt, l, r)
            y0, x0 = prm['y0'], prm['x0']
            img = img[y0:y0 + ch, x0:x0 + cw]
            msk = msk[y0:y0 + ch, x0:x0 + cw]
        img = img.astype(np.float32)
        if prm['jittered']:
            for op, v in prm['ops']:
                if op == 'b':
                    img = np.clip(img * v, 0, 255)
                elif op == 'c':
                    m = _gray(img).mean()
                    img = np.clip((img - m) * v + m, 0, 255)
                elif op == 's':
                    g = _gray(img)[..., None]
                    img = np.clip((img - g) * v + g, 0, 255)
                else:
                    img = np.clip(_adjust_hue(img, v), 0, 255)
        intensity = any(prm.get(k) is not None for k in ('gamma', 'blur', 'noise'))
        if intensity:
            img = medical_intensity(img, prm)
        if prm['jittered'] or intensity:
            img = np.clip(np.round(img), 0, 255)     # one rounding for the whole intensity chain
        if prm['hflip']:
            img, msk = img[:, ::-1], msk[:, ::-1]
        if prm['vflip']:
            img, msk = img[::-1], msk[::-1]
        return normalize_to_tensor(img, self.mean, self.std), torch.from_numpy(np.ascontiguousarray(msk)).long()


def normalize_to_tensor(img, mean=None, std=None):
    mean = np.asarray(IMAGENET_MEAN, np.float32) * 255.0 if mean is None else mean
    std = np.asarray(IMAGENET_STD, np.float32) * 255.0 if std is None else std
    x = (np.asarray(img, np.float32) - mean) / std
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))
