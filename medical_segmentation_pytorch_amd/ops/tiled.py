"""Sliding-window inference with flip test-time augmentation (``csrc/tiled.hip``).  An addition over the
reference, which pushes the whole (resized) image through the network in one call.

Semantics (both paths implement exactly this):
  * geometry, per axis (``L`` image extent, ``w`` window extent, ``o`` overlap in [0, 0.75]): step
    ``s = max(1, int(w * (1 - o)))``; ``L <= w``: one window at start 0 over the image zero-padded to ``w`` with
    ``(w - L) // 2`` pixels before and the rest after (zeros in normalised space = the dataset mean colour), the
    result cropped back to ``L``; otherwise ``n = ceil((L - w) / s) + 1`` windows at ``min(i * s, L - w)`` -- the last
    one clipped to the frame, so the starts are strictly increasing but no uniform grid;
  * views: ``flips`` '' (identity), 'h' (identity, horizontal mirror), 'v' (identity, vertical mirror), 'hv'
    (identity, h, v, h∘v).  A view mirrors the WINDOW before the forward and its logits back before blending;
  * window index ``m = ((n_img * ny + iy) * nx + ix) * V + v``: the order in which windows reach the predictor and
    the order of every sum;
  * importance map ``weight(y, x) = wy[y] * wx[x]`` (fp32 vectors): all ones ('constant') or
    ``exp(-(k - c)^2 / (2 sigma^2))``, ``c = (w - 1) / 2``, ``sigma = sigma_scale * w`` ('gaussian'), computed in
    fp64 and rounded once, no clamping;
  * ``out = sum_m weight * f(x_m) / sum_m weight`` over the windows and views covering the pixel, fp32 sums in
    ascending ``m`` -- independent of how the windows were chunked.  ``average='logits'``: ``f`` = identity.
    ``average='probs'``: ``f`` = softmax over the classes (sigmoid for a one-channel head) and the result is the
    logits of the averaged distribution, ``log(max(p, FLT_MIN))`` for ``C >= 2`` and ``log(p / (1 - p))`` with
    ``p`` clamped to ``[FLT_MIN, 1 - 2^-24]`` for ``C == 1``, so every consumer of logits keeps working;
  * the normaliser ``sum_m weight`` is separable, ``V * ysum[y] * xsum[x]``; the two vectors are summed in fp64
    from the fp32 weights and rounded once.

On the GPU with the extension the HIP kernels run (one gather, one blend per chunk, one finalise; no host read, no
synchronisation; the first use of a geometry on a device copies its small tables there, so warm a geometry up once
before capturing it in a graph); otherwise the plain-torch form below, which is the specification in code and the
oracle of the GPU tests (it runs in the dtype of its input, so an fp64 input gives the fp64 oracle).
"""
from __future__ import annotations

import functools
import math

import torch

from . import _ext

FLIPS = ('', 'h', 'v', 'hv')
BLENDS = ('gaussian', 'constant')
AVERAGES = ('logits', 'probs')
MAX_OVERLAP = 0.75
MAX_CLASSES = 64               # the blend kernels' generic class loop
FLT_MIN = 1.1754943508222875e-38
P_MAX = 1.0 - 2.0 ** -24


def _native(t):
    return t.is_cuda and _ext.available()


# ---- geometry ---------------------------------------------------------------------------------------------
def window_starts(L, w, overlap):
    """Starts of the windows of extent ``w`` along an axis of extent ``L`` (in the padded frame when ``L < w``)."""
    L, w = int(L), int(w)
    if L < 1 or w < 1:
        raise ValueError(f'window_starts: extents must be >= 1, got L={L}, w={w}')
    if not 0.0 <= float(overlap) <= MAX_OVERLAP:
        raise ValueError(f'overlap must be in [0, {MAX_OVERLAP}], got {overlap}')
    if L <= w:
        return [0]
    s = max(1, int(w * (1.0 - float(overlap))))
    n = -(-(L - w) // s) + 1
    return [min(i * s, L - w) for i in range(n)]


def _importance64(w, blend, sigma_scale):
    if blend == 'constant':
        return torch.ones(w, dtype=torch.float64)
    if blend != 'gaussian':
        raise ValueError(f"blend must be one of {BLENDS}, got {blend!r}")
    if not float(sigma_scale) > 0:
        raise ValueError(f'sigma_scale must be > 0, got {sigma_scale}')
    k = torch.arange(w, dtype=torch.float64)
    sigma = float(sigma_scale) * w
    return torch.exp(-(k - (w - 1) / 2.0) ** 2 / (2.0 * sigma * sigma))


def importance_vectors(wh, ww, blend='gaussian', sigma_scale=0.125):
    """The two fp32 factors ``(wy [wh], wx [ww])`` of the separable importance map."""
    return (_importance64(int(wh), blend, sigma_scale).float(), _importance64(int(ww), blend, sigma_scale).float())


def _pair(window):
    if isinstance(window, (tuple, list)):
        if len(window) == 1:
            return int(window[0]), int(window[0])
        if len(window) != 2:
            raise ValueError(f'window must be one integer or two (h, w), got {window!r}')
        return int(window[0]), int(window[1])
    return int(window), int(window)


class TilePlan:
    """Everything that depends only on the geometry ``(H, W, window, overlap, blend, sigma_scale, flips)``: the window
    starts, the padding, the importance vectors, the separable normaliser and, per image row / column, the range of
    windows covering it.  Device copies are made once per device and kept."""

    def __init__(self, H, W, window, overlap, blend, sigma_scale, flips):
        if flips not in FLIPS:
            raise ValueError(f'flips must be one of {FLIPS}, got {flips!r}')
        self.H, self.W = int(H), int(W)
        self.wh, self.ww = _pair(window)
        self.overlap, self.blend, self.sigma_scale, self.flips = float(overlap), blend, float(sigma_scale), flips
        self.sy, self.sx = window_starts(self.H, self.wh, overlap), window_starts(self.W, self.ww, overlap)
        self.ny, self.nx = len(self.sy), len(self.sx)
        self.py, self.px = max(0, self.wh - self.H) // 2, max(0, self.ww - self.W) // 2
        self.Hp, self.Wp = max(self.H, self.wh), max(self.W, self.ww)
        self.views = {'': [(0, 0)], 'h': [(0, 0), (1, 0)], 'v': [(0, 0), (0, 1)],
                      'hv': [(0, 0), (1, 0), (0, 1), (1, 1)]}[flips]       # (mirror x, mirror y) per view
        self.V = len(self.views)
        self.flip_code = FLIPS.index(flips)
        self.wy, self.wx = importance_vectors(self.wh, self.ww, blend, sigma_scale)
        ylo, yhi, self.ysum = self._axis(self.sy, self.wh, self.H, self.py, self.wy)
        xlo, xhi, self.xsum = self._axis(self.sx, self.ww, self.W, self.px, self.wx)
        self.cover = torch.tensor(ylo + yhi + xlo + xhi, dtype=torch.int32)     # [2 H + 2 W]
        self.starts = torch.tensor(self.sy + self.sx, dtype=torch.int32)        # [ny + nx]
        self.max_terms = max(h - l + 1 for l, h in zip(ylo, yhi)) * max(h - l + 1 for l, h in zip(xlo, xhi)) * self.V
        self._dev = {}

    @staticmethod
    def _axis(starts, w, L, pad, weight):
        """per image coordinate: first / last covering window and the fp64 sum of their fp32 weights, rounded once"""
        lo, hi, tot = [], [], []
        w64 = weight.double()
        for p in range(pad, pad + L):
            cov = [i for i, s in enumerate(starts) if s <= p < s + w]
            lo.append(cov[0])
            hi.append(cov[-1])
            tot.append(sum(float(w64[p - starts[i]]) for i in cov))
        return lo, hi, torch.tensor(tot, dtype=torch.float64)

    def windows(self, n_images):
        return int(n_images) * self.ny * self.nx * self.V

    def decode(self, m):
        v = m % self.V
        ix = (m // self.V) % self.nx
        iy = (m // (self.V * self.nx)) % self.ny
        return m // (self.V * self.nx * self.ny), iy, ix, v

    def rows_of(self, m0, m1, n_images):
        """``(n0, n1, y0, y1)``: images [n0, n1) and image rows [y0, y1) touched by the real windows in [m0, m1)"""
        m1 = min(m1, self.windows(n_images))
        if m1 <= m0:
            return 0, 0, 0, 0
        na, iya, _, _ = self.decode(m0)
        nb, iyb, _, _ = self.decode(m1 - 1)
        if na != nb:
            return na, nb + 1, 0, self.H
        y0 = max(0, self.sy[iya] - self.py)
        y1 = min(self.H, self.sy[iyb] + self.wh - self.py)
        return na, nb + 1, y0, y1

    def on(self, device):
        """fp32 / int32 device copies: ``wy, wx, ysum, xsum, starts, cover``.  The first call per plan and device
        copies them from the host, so a plan must be used once outside a graph capture before it is used inside one;
        later calls launch kernels only."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:      # 'cuda' and 'cuda:<current>' are one device
            device = torch.device('cuda', torch.cuda.current_device())
        key = (device.type, device.index)
        if key not in self._dev:
            self._dev[key] = {'wy': self.wy.to(device), 'wx': self.wx.to(device),
                              'ysum': self.ysum.float().to(device), 'xsum': self.xsum.float().to(device),
                              'starts': self.starts.to(device), 'cover': self.cover.to(device)}
        return self._dev[key]


@functools.lru_cache(maxsize=32)
def _plan(H, W, window, overlap, blend, sigma_scale, flips):
    return TilePlan(H, W, window, overlap, blend, sigma_scale, flips)


def tile_plan(H, W, window, overlap=0.5, blend='gaussian', sigma_scale=0.125, flips=''):
    """The cached :class:`TilePlan` of one geometry."""
    return _plan(int(H), int(W), _pair(window), float(overlap), blend, float(sigma_scale), flips)


def _check_average(average):
    if average not in AVERAGES:
        raise ValueError(f'average must be one of {AVERAGES}, got {average!r}')


# ---- plain-torch specification ----------------------------------------------------------------------------
def _flip(t, view):
    dims = [d for d, f in ((-1, view[0]), (-2, view[1])) if f]
    return t.flip(dims) if dims else t


def _gather_torch(images, plan, m0, count):
    n, cin = images.shape[:2]
    padded = images.new_zeros(n, cin, plan.Hp, plan.Wp)
    padded[:, :, plan.py:plan.py + plan.H, plan.px:plan.px + plan.W] = images
    out = images.new_zeros(count, cin, plan.wh, plan.ww)
    for b in range(min(count, plan.windows(n) - m0)):
        i, iy, ix, v = plan.decode(m0 + b)
        y, x = plan.sy[iy], plan.sx[ix]
        out[b] = _flip(padded[i, :, y:y + plan.wh, x:x + plan.ww], plan.views[v])
    return out


def _accumulate_torch(acc, logits, plan, m0, average):
    """acc: the padded-frame accumulator [N, C, Hp, Wp]; adds the windows [m0, m0 + B) that exist, in ascending m"""
    n = acc.shape[0]
    weight = plan.wy.to(acc)[:, None] * plan.wx.to(acc)[None, :]
    for b in range(min(logits.shape[0], plan.windows(n) - m0)):
        i, iy, ix, v = plan.decode(m0 + b)
        x = logits[b].to(acc.dtype)
        if average == 'probs':
            x = torch.sigmoid(x) if x.shape[0] == 1 else torch.softmax(x, 0)
        y0, x0 = plan.sy[iy], plan.sx[ix]
        acc[i, :, y0:y0 + plan.wh, x0:x0 + plan.ww] += weight * _flip(x, plan.views[v])
    return acc


def _finalize_torch(acc, plan, average):
    """crop the padded accumulator to the image, divide by the normaliser, back to logits in 'probs' mode"""
    out = acc[:, :, plan.py:plan.py + plan.H, plan.px:plan.px + plan.W]
    ysum, xsum = plan.ysum.to(acc), plan.xsum.to(acc)       # fp64 sums, rounded once for an fp32 accumulator
    out = out / ((ysum[:, None] * xsum[None, :]) * float(plan.V))
    if average == 'probs':
        if out.shape[1] == 1:
            p = out.clamp(FLT_MIN, P_MAX)
            out = torch.log(p / (1.0 - p))
        else:
            out = torch.log(out.clamp_min(FLT_MIN))
    return out.contiguous()


# ---- public pieces ----------------------------------------------------------------------------------------
def gather_windows(images, plan, m0=0, count=None, native=None):
    """Windows ``[m0, m0 + count)`` of ``images`` [N, Cin, H, W] as ``[count, Cin, wh, ww]``: crop, zero padding and
    the view's mirror in one pass (a pure copy).  Indices past the last window give zero windows."""
    if images.dim() != 4 or tuple(images.shape[2:]) != (plan.H, plan.W):
        raise ValueError(f'images must be [N, Cin, {plan.H}, {plan.W}], got {tuple(images.shape)}')
    total = plan.windows(images.shape[0])
    count = total - m0 if count is None else int(count)
    if m0 < 0 or count < 1:
        raise ValueError(f'gather_windows: need m0 >= 0 and count >= 1, got m0={m0}, count={count}')
    if native is None:
        native = _native(images) and images.dtype == torch.float32
    if not native:
        return _gather_torch(images, plan, m0, count)
    images = images.contiguous()
    dev = plan.on(images.device)
    out = torch.empty(count, images.shape[1], plan.wh, plan.ww, dtype=torch.float32, device=images.device)
    _ext.require().window_gather(images, out, dev['starts'], plan.ny, plan.nx, plan.py, plan.px, plan.flip_code, m0)
    return out


def new_accumulator(plan, n_images, channels, like, native):
    """zeros: ``[N, C, H, W]`` for the kernels, the padded frame ``[N, C, Hp, Wp]`` for the specification"""
    if native:
        return torch.zeros(n_images, channels, plan.H, plan.W, dtype=torch.float32, device=like.device)
    return torch.zeros(n_images, channels, plan.Hp, plan.Wp, dtype=like.dtype, device=like.device)


def accumulate_windows(acc, logits, plan, m0, average='logits', native=None):
    """Add the logits ``[B, C, wh, ww]`` of windows ``[m0, m0 + B)`` (those that exist) into ``acc``."""
    _check_average(average)
    if logits.dim() != 4 or tuple(logits.shape[1:]) != (acc.shape[1], plan.wh, plan.ww):
        raise ValueError(f'logits must be [B, {acc.shape[1]}, {plan.wh}, {plan.ww}], got {tuple(logits.shape)}')
    if native is None:
        native = _native(acc) and acc.dtype == torch.float32 and tuple(acc.shape[2:]) == (plan.H, plan.W)
    if not native:
        return _accumulate_torch(acc, logits, plan, m0, average)
    if not 1 <= acc.shape[1] <= MAX_CLASSES:
        raise ValueError(f'the blend kernels take 1 .. {MAX_CLASSES} classes, got {acc.shape[1]}')
    dev = plan.on(acc.device)
    n0, n1, y0, y1 = plan.rows_of(m0, m0 + logits.shape[0], acc.shape[0])
    if n1 > n0:
        _ext.require().window_blend_accumulate(logits.contiguous().float(), acc, dev['starts'], dev['cover'], dev['wy'],
                                               dev['wx'], plan.ny, plan.nx, plan.py, plan.px, plan.flip_code, m0,
                                               average == 'probs', n0, n1, y0, y1)
    return acc


def finalize_windows(acc, plan, average='logits', native=None):
    """The blended logits ``[N, C, H, W]`` of a fully accumulated ``acc`` (in place on the device path)."""
    _check_average(average)
    if native is None:
        native = _native(acc) and acc.dtype == torch.float32 and tuple(acc.shape[2:]) == (plan.H, plan.W)
    if not native:
        return _finalize_torch(acc, plan, average)
    dev = plan.on(acc.device)
    _ext.require().window_blend_finalize(acc, dev['ysum'], dev['xsum'], plan.V, average == 'probs')
    return acc


def blend_windows(logits, plan, n_images, average='logits', batch=None, native=None):
    """Blend the logits ``[M, C, wh, ww]`` of ALL windows of ``n_images`` images (``M = plan.windows(n_images)``) into
    ``[N, C, H, W]``, feeding them to the accumulator ``batch`` at a time (the result does not depend on it)."""
    m = plan.windows(n_images)
    if logits.dim() != 4 or logits.shape[0] != m:
        raise ValueError(f'logits must be [{m}, C, {plan.wh}, {plan.ww}], got {tuple(logits.shape)}')
    _check_average(average)
    if native is None:
        native = _native(logits) and logits.dtype == torch.float32
    acc = new_accumulator(plan, n_images, logits.shape[1], logits, native)
    batch = m if batch is None else max(1, int(batch))
    for m0 in range(0, m, batch):
        accumulate_windows(acc, logits[m0:m0 + batch], plan, m0, average, native)
    return finalize_windows(acc, plan, average, native)


def sliding_window_inference(images, predictor, window, overlap=0.5, blend='gaussian', sigma_scale=0.125, flips='',
                             average='logits', batch=16, native=None):
    """fp32 ``[N, C, H, W]`` logits of ``images`` [N, Cin, H, W]: ``predictor`` (``[B, Cin, wh, ww]`` ->
    ``[B, C, wh, ww]``) runs on fixed-size windows, ``batch`` at a time in window-index order; a short last chunk is
    filled up with zero windows, so the predictor only ever sees one shape.  ``native=False`` runs the plain-torch
    specification on the tensors' device (benchmarks, oracles)."""
    if images.dim() != 4:
        raise ValueError(f'images must be [N, Cin, H, W], got {tuple(images.shape)}')
    _check_average(average)
    if int(batch) < 1:
        raise ValueError(f'batch must be >= 1, got {batch}')
    n, _, h, w = images.shape
    plan = tile_plan(h, w, window, overlap, blend, sigma_scale, flips)
    images = images.float()
    if native is None:
        native = _native(images)
    total = plan.windows(n)
    step = min(int(batch), total)
    acc = None
    for m0 in range(0, total, step):
        logits = predictor(gather_windows(images, plan, m0, step, native))
        if logits.dim() != 4 or logits.shape[0] != step or tuple(logits.shape[2:]) != (plan.wh, plan.ww):
            raise ValueError(f'predictor must map [B, Cin, {plan.wh}, {plan.ww}] to [B, C, {plan.wh}, {plan.ww}], '
                             f'got {tuple(logits.shape)} for B = {step}')
        logits = logits.float()
        if acc is None:
            acc = new_accumulator(plan, n, logits.shape[1], logits, native)
        accumulate_windows(acc, logits, plan, m0, average, native)
    return finalize_windows(acc, plan, average, native)
