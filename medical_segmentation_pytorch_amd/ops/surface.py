"""Boundary (surface-distance) metrics of a segmentation batch: HD95, ASSD and NSD, on an exact integer
squared Euclidean distance transform (``csrc/surface.hip``).  An addition over the reference, which only
scores overlap (Dice / IoU).

Semantics (both paths implement exactly this):
  * prediction = per-pixel argmax (first maximum wins); a pixel whose target is ``ignore_index`` or outside
    ``[0, C)`` is in no class, in either mask; foreground classes ``1 .. C-1`` are scored;
  * boundary of a mask = its pixels with a 4-neighbour outside the mask, pixels outside the image counting as
    outside (``mask ^ binary_erosion(mask, cross)``), so mask pixels on the image frame are boundary pixels;
  * distances are Euclidean in pixels (spacing 1) from every boundary pixel of one mask to the nearest boundary
    pixel of the other; the squared distance is an exact integer;
  * per image and class: ``hd95 = max(q95(D_pg), q95(D_gp))`` -- the maximum of the two directional 95th
    percentiles (linear interpolation, numpy's default), which is MONAI's convention and NOT the pooled
    percentile medpy takes; ``assd = (sum D_pg + sum D_gp) / (|D_pg| + |D_gp|)``; ``nsd`` = the fraction of
    both multisets with ``d2 <= floor(tolerance^2)`` (integer comparison);
  * both masks empty: the pair is not scored; exactly one empty: ``hd95 = assd = sqrt(H^2 + W^2)``, ``nsd = 0``
    and the pair is counted as one-sided.

On the GPU with the extension the HIP kernels run (no host synchronisation, scratch cached by shape); otherwise
the plain-torch form below, which is the specification in code and the oracle of the GPU tests.
"""
from __future__ import annotations

import math

import torch

from . import _ext

EDT_MAX_DIM = 16384
EDT_NONE = 2 ** 31 - 1     # edt_sq of a map without any set pixel


def _native(t):
    return t.is_cuda and _ext.available()


def new_state(num_classes, device=None):
    """Per-class accumulator of :func:`surface_stats`: fp64 sums of the per-image (hd95, assd, nsd), the number
    of scored (image, class) pairs and the number of those with exactly one empty mask."""
    k = num_classes - 1
    return {'sum': torch.zeros(3, k, dtype=torch.float64, device=device),
            'count': torch.zeros(k, dtype=torch.long, device=device),
            'onesided': torch.zeros(k, dtype=torch.long, device=device)}


MAX_ROWS = 2 ** 24 - 1      # image rows per device call: the row pass launches one 256-thread block per row


def _check_hw(h, w, images=1):
    if h < 1 or w < 1 or h > EDT_MAX_DIM or w > EDT_MAX_DIM:
        raise ValueError(f'distance transform: H and W must be in [1, {EDT_MAX_DIM}], got {h} x {w}')
    if images * h > MAX_ROWS:
        raise ValueError(f'distance transform: {images} images of {h} rows exceed {MAX_ROWS} rows per call')


# ---- plain-torch specification ----------------------------------------------------------------------------
def _boundary_torch(mask):
    m = mask != 0
    p = torch.zeros(*m.shape[:-2], m.shape[-2] + 2, m.shape[-1] + 2, dtype=torch.bool, device=m.device)
    p[..., 1:-1, 1:-1] = m
    eroded = m & p[..., :-2, 1:-1] & p[..., 2:, 1:-1] & p[..., 1:-1, :-2] & p[..., 1:-1, 2:]
    return m & ~eroded


def _nearest_sq(a, b, chunk=1 << 22):
    """a [Na, 2], b [Nb, 2] int64 coordinates, Nb > 0 -> [Na] exact squared distance to the nearest row of b."""
    out = torch.empty(a.shape[0], dtype=torch.long, device=a.device)
    step = max(1, chunk // max(1, b.shape[0]))
    for i in range(0, a.shape[0], step):
        d = a[i:i + step, None, :] - b[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(1).values
    return out


def _edt_sq_torch(mask):
    m = mask != 0
    h, w = m.shape[-2:]
    flat = m.reshape(-1, h, w)
    out = torch.full(flat.shape, EDT_NONE, dtype=torch.int32, device=m.device)
    ys, xs = torch.meshgrid(torch.arange(h, device=m.device), torch.arange(w, device=m.device), indexing='ij')
    grid = torch.stack([ys.reshape(-1), xs.reshape(-1)], 1)
    for i in range(flat.shape[0]):
        pts = flat[i].nonzero()
        if pts.shape[0]:
            out[i] = _nearest_sq(grid, pts).view(h, w).to(torch.int32)
    return out.view(m.shape)


def _labels_torch(preds, target, num_classes, ignore_index):
    t = target.long()
    valid = (t >= 0) & (t < num_classes)
    if ignore_index is not None:
        valid &= t != ignore_index
    none = torch.full_like(t, -1)
    return torch.where(valid, preds.argmax(1), none), torch.where(valid, t, none)


def _rank_values(d2):
    """sorted d2 at floor / ceil of the q95 rank 0.95 (n - 1)"""
    s = d2.sort().values
    pos = 0.95 * (s.numel() - 1)
    return int(s[math.floor(pos)]), int(s[math.ceil(pos)])


def _surface_stats_torch(preds, target, num_classes, ignore_index, tol2, state, debug):
    n, _, h, w = preds.shape
    k = num_classes - 1
    pl, tl = _labels_torch(preds, target, num_classes, ignore_index)
    diag = math.sqrt(h * h + w * w)
    src = preds.device
    per = torch.full((n, k, 3), float('nan'), dtype=torch.float64, device=src)
    counts = torch.zeros(2, n, k, dtype=torch.long, device=src)
    within = torch.zeros(2, n, k, dtype=torch.long, device=src)
    order = torch.zeros(2, n, k, 2, dtype=torch.long, device=src)
    for i in range(n):
        for c in range(1, num_classes):
            bp = _boundary_torch(pl[i] == c).nonzero()
            bg = _boundary_torch(tl[i] == c).nonzero()
            counts[0, i, c - 1], counts[1, i, c - 1] = bp.shape[0], bg.shape[0]
            if bp.shape[0] == 0 and bg.shape[0] == 0:
                continue
            if bp.shape[0] == 0 or bg.shape[0] == 0:
                per[i, c - 1] = torch.tensor([diag, diag, 0.0], dtype=torch.float64, device=src)
                continue
            dirs = (_nearest_sq(bp, bg), _nearest_sq(bg, bp))
            q, total, close = [], 0.0, 0
            for j, d2 in enumerate(dirs):
                d = d2.double().sqrt()
                q.append(float(torch.quantile(d, 0.95)))
                total += float(d.sum())
                close += int((d2 <= tol2).sum())
                within[j, i, c - 1] = int((d2 <= tol2).sum())
                order[j, i, c - 1, 0], order[j, i, c - 1, 1] = _rank_values(d2)
            npts = bp.shape[0] + bg.shape[0]
            per[i, c - 1] = torch.tensor([max(q), total / npts, close / npts], dtype=torch.float64,
                                         device=src)
    scored = ~per[..., 0].isnan()
    dev = state['sum'].device
    state['sum'] += torch.where(scored[..., None], per, torch.zeros_like(per)).sum(0).t().to(dev)
    state['count'] += scored.sum(0).to(dev)
    state['onesided'] += ((counts[0] == 0) != (counts[1] == 0)).sum(0).to(dev)
    if debug:
        return {'counts': counts, 'within': within, 'order': order, 'per_image': per}
    return None


# ---- device path ------------------------------------------------------------------------------------------
_SCRATCH = {}


def _scratch(device, n, k, h, w):
    """Work buffers of one update, cached for the last shape seen per device (re-sized when it changes)."""
    key = (n, k, h, w)
    hit = _SCRATCH.get(device)
    if hit is None or hit[0] != key:
        b = 2 * n * k
        hit = (key, {'lab': torch.empty(2 * n, h, w, dtype=torch.uint8, device=device),
                     'bnd': torch.empty(b, h, w, dtype=torch.uint8, device=device),
                     'd2': torch.empty(b, h, w, dtype=torch.int32, device=device),
                     'stats': torch.empty(b, 4, dtype=torch.long, device=device),
                     'sums': torch.empty(b, dtype=torch.float64, device=device)})
        _SCRATCH[device] = hit
    return hit[1]


def _surface_stats_device(preds, target, num_classes, ignore_index, tol2, state, debug):
    C = _ext.require()
    n, _, h, w = preds.shape
    k = num_classes - 1
    _check_hw(h, w, 2 * n * k)
    s = _scratch(preds.device, n, k, h, w)
    ig = ignore_index if ignore_index is not None else -1
    C.surface_labels(preds, target, s['lab'], ig)
    C.surface_boundary(s['lab'], s['bnd'], k)       # [2 (prediction, target), n, k] planes
    # image (src, n, k) of d2: distance to the boundary of src, evaluated at the boundary pixels of the other
    # source -- so planes [0, nk) hold D_gp and planes [nk, 2nk) hold D_pg
    C.edt_sq(s['bnd'], s['d2'], s['bnd'], n * k)
    C.surface_reduce(s['d2'], s['stats'], s['sums'], h * h + w * w, min(tol2, EDT_NONE - 1))
    per = torch.empty(n, k, 3, dtype=torch.float64, device=preds.device) if debug else None
    C.surface_finalize(s['stats'], s['sums'], state['sum'], state['count'], state['onesided'], per, n, k, h, w)
    if not debug:
        return None
    st = s['stats'].view(2, n, k, 4).flip(0)       # direction 0 = prediction -> ground truth
    both = ((st[0, ..., 0] > 0) & (st[1, ..., 0] > 0))[None, ..., None]
    zero = torch.zeros_like(st[..., 1:])
    rest = torch.where(both, st[..., 1:], zero)
    return {'counts': st[..., 0].clone(), 'within': rest[..., 0], 'order': rest[..., 1:], 'per_image': per}


# ---- public ops -------------------------------------------------------------------------------------------
def mask_boundary(mask):
    """bool ``[..., H, W]``: the pixels of ``mask != 0`` with a 4-neighbour outside it (outside the image counts)."""
    h, w = mask.shape[-2:]
    if not _native(mask) or mask.numel() == 0:
        return _boundary_torch(mask)
    _check_hw(h, w)
    lab = (mask != 0).to(torch.uint8).reshape(-1, h, w).contiguous()
    _check_hw(h, w, lab.shape[0])
    out = torch.empty_like(lab)
    _ext.require().surface_boundary(lab, out, 1)
    return out.view(mask.shape).bool()


def edt_sq(mask):
    """int32 ``[..., H, W]``: exact squared Euclidean distance (pixels) to the nearest nonzero pixel of the same
    image; ``EDT_NONE`` (INT32_MAX) everywhere in an image without one.  H, W <= 16384."""
    h, w = mask.shape[-2:]
    _check_hw(h, w)
    if not _native(mask) or mask.numel() == 0:
        return _edt_sq_torch(mask)
    m = (mask != 0).to(torch.uint8).reshape(-1, h, w).contiguous()
    _check_hw(h, w, m.shape[0])
    out = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    _ext.require().edt_sq(m, out)
    return out.view(mask.shape)


SDF_MAX_DIM = 2048          # signed_distance: d^2 <= 2 * 2048^2 = 2^23, exact in fp32
SDF_MAX_CLASSES = 64


def _sdf_classes(num_classes, classes):
    if not 2 <= num_classes <= SDF_MAX_CLASSES:
        raise ValueError(f'signed distance: num_classes must be in [2, {SDF_MAX_CLASSES}], got {num_classes}')
    cls = list(range(1, num_classes)) if classes is None else [int(c) for c in classes]
    if not cls or len(set(cls)) != len(cls) or min(cls) < 0 or max(cls) >= num_classes:
        raise ValueError(f'signed distance: classes must be distinct values in [0, {num_classes}), got {classes!r}')
    return cls


def _check_sdf_hw(h, w):
    if h < 1 or w < 1 or h > SDF_MAX_DIM or w > SDF_MAX_DIM:
        raise ValueError(f'signed distance: H and W must be in [1, {SDF_MAX_DIM}], got {h} x {w}')


_SDF_COL_NONE = 1 << 15     # vertical "no such pixel in this column"; its square 2^30 exceeds every real d^2


def _col_dist(m):
    """bool [B, H, W] -> int32 vertical distance to the nearest set pixel of the column (_SDF_COL_NONE: none)."""
    h = m.shape[1]
    y = torch.arange(h, device=m.device, dtype=torch.int32).view(1, h, 1)
    far = torch.full_like(y, -2 * _SDF_COL_NONE).expand_as(m)     # |y -+ far| > _SDF_COL_NONE for every row
    above = torch.where(m, y.expand_as(m), far).cummax(1).values                      # last set row <= y
    below = -torch.where(m, -y.expand_as(m), far).flip(1).cummax(1).values.flip(1)    # first set row >= y
    return torch.minimum(y - above, below - y).clamp_max(_SDF_COL_NONE)


def _row_min(g2, chunk=1 << 24):
    """int32 [B, H, W] squared vertical field -> min over x' of (x - x')^2 + g2[.., x'] (broadcast, rows in chunks)."""
    b, h, w = g2.shape
    x = torch.arange(w, device=g2.device, dtype=torch.int32)
    dx2 = (x.view(w, 1) - x.view(1, w)) ** 2
    flat = g2.reshape(b * h, w)
    out = torch.empty_like(flat)
    step = max(1, chunk // (w * w))
    for i in range(0, flat.shape[0], step):
        out[i:i + step] = (flat[i:i + step, None, :] + dx2).min(-1).values
    return out.view(b, h, w)


def _signed_distance_sq_torch(labels, num_classes, ignore_index, cls):
    t = labels.long()
    n, h, w = t.shape
    valid = (t >= 0) & (t < num_classes)
    if ignore_index is not None:
        valid &= t != ignore_index
    sel = torch.tensor(cls, device=t.device).view(1, -1, 1, 1)
    pos = (valid.unsqueeze(1) & (t.unsqueeze(1) == sel)).reshape(-1, h, w)
    neg = (valid.unsqueeze(1) & (t.unsqueeze(1) != sel)).reshape(-1, h, w)
    live = (pos.flatten(1).any(1) & neg.flatten(1).any(1)).view(-1, 1, 1)
    to_pos = _row_min(_col_dist(pos) ** 2)
    to_neg = _row_min(_col_dist(neg) ** 2)
    zero = torch.zeros_like(to_pos)
    s = torch.where(neg, to_pos, zero) - torch.where(pos, to_neg, zero)
    return torch.where(live, s, zero).view(n, len(cls), h, w)


def _sqrt_rn_f32(v):
    """Correctly rounded fp32 square root of integers ``0 <= v < 2^24``.  ``torch.sqrt`` on fp32 is not correctly
    rounded on every CPU (its vector kernels allow slightly more than half an ulp), so the candidate from the fp64
    root is checked against its two rounding boundaries: those are 25-bit numbers, so their squares are exact in
    fp64, and one step to the neighbour settles a candidate that lies on the wrong side."""
    v64 = v.double()
    r = v64.sqrt().float()
    up = torch.nextafter(r, torch.full_like(r, float('inf')))
    dn = torch.nextafter(r, torch.full_like(r, float('-inf')))
    hi, lo = (r.double() + up.double()) * 0.5, (r.double() + dn.double()) * 0.5
    return torch.where(v64 > hi * hi, up, torch.where((v64 < lo * lo) & (r > 0), dn, r))


def _phi_torch(s):
    f = _sqrt_rn_f32(s.abs())
    return torch.where(s > 0, f, torch.where(s < 0, 1.0 - f, torch.zeros_like(f)))


def signed_distance(labels, num_classes, ignore_index=None, classes=None, squared=False):
    """Signed distance map of integer labels ``[N, H, W]`` per class of ``classes`` (default ``1 .. C-1``):
    ``[N, len(classes), H, W]``.

    A pixel is valid iff ``label != ignore_index and 0 <= label < num_classes``.  Per image and class ``c``,
    ``pos`` = valid pixels labelled ``c`` and ``neg`` = the other valid pixels.  ``squared=True`` gives the exact
    int32 ``s``: ``+d^2`` to the nearest ``pos`` pixel at a ``neg`` pixel (>= 1), ``-d^2`` to the nearest ``neg``
    pixel at a ``pos`` pixel (<= -1), 0 at an invalid pixel (distances are measured across those), and 0
    everywhere in a plane whose ``pos`` or ``neg`` set is empty.  Otherwise the fp32 signed distance
    ``phi = sqrt(s)`` (s > 0), ``1 - sqrt(-s)`` (s < 0), ``0``, i.e. ``edt(neg) * neg - (edt(pos) - 1) * pos`` with
    scipy's ``distance_transform_edt`` (the root is the correctly rounded fp32 one; ``|s| <= 2^23`` is exact).
    H, W <= ``SDF_MAX_DIM``.  On the GPU with the extension one column pass and one row pass of ``csrc/surface.hip``
    (no host synchronisation); otherwise the separable plain-torch form above, the specification in code."""
    if labels.dim() != 3 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f'labels must be integer [N, H, W], got {labels.dtype} {tuple(labels.shape)}')
    cls = _sdf_classes(int(num_classes), classes)
    n, h, w = labels.shape
    _check_sdf_hw(h, w)
    if n == 0:
        return torch.zeros(0, len(cls), h, w, dtype=torch.int32 if squared else torch.float32, device=labels.device)
    if not _native(labels):
        s = _signed_distance_sq_torch(labels, int(num_classes), ignore_index, cls)
        return s if squared else _phi_torch(s)
    C = _ext.require()
    s = torch.empty(n, len(cls), h, w, dtype=torch.int32, device=labels.device)
    C.sdf_sq(labels.contiguous().long(), s, cls, int(num_classes), -1 if ignore_index is None else int(ignore_index))
    if squared:
        return s
    phi = torch.empty(s.shape, dtype=torch.float32, device=s.device)
    C.sdf_phi(s, phi)
    return phi


def surface_stats(preds, target, num_classes, ignore_index=None, nsd_tolerance=2.0, state=None, debug=False,
                  native=None):
    """Add the boundary statistics of one batch into ``state`` (see :func:`new_state`).

    preds ``[N, C, H, W]`` fp32 logits (C == num_classes >= 2), target ``[N, H, W]`` integer labels.  With
    ``debug`` returns, per direction (0: prediction -> ground truth, 1: the reverse), image and foreground class:
    ``counts`` ``[2, N, C-1]`` boundary sizes, ``within`` the numbers with ``d2 <= T``, ``order`` ``[2, N, C-1, 2]``
    the squared distances at floor / ceil of the q95 rank (the last two are zero unless both masks are non-empty)
    and ``per_image`` ``[N, C-1, 3]`` fp64 (hd95, assd, nsd; nan where not scored).  ``native=False`` runs the
    plain-torch form on the tensors' device (benchmarks, oracles)."""
    if preds.dim() != 4 or preds.shape[1] != num_classes or num_classes < 2:
        raise ValueError(f'preds must be [N, {num_classes}, H, W] with num_classes >= 2, got {tuple(preds.shape)}')
    if target.shape != preds.shape[:1] + preds.shape[2:]:
        raise ValueError(f'target must be [N, H, W] = {tuple(preds.shape[:1] + preds.shape[2:])}, '
                         f'got {tuple(target.shape)}')
    _check_hw(preds.shape[2], preds.shape[3])
    if state is None:
        state = new_state(num_classes, preds.device)
    tol2 = int(math.floor(float(nsd_tolerance) ** 2))
    if preds.shape[0] == 0:
        return None
    if native is None:
        native = _native(preds) and state['sum'].is_cuda
    if native:
        return _surface_stats_device(preds.contiguous().float(), target.contiguous().long(), num_classes,
                                     ignore_index, tol2, state, debug)
    return _surface_stats_torch(preds.float(), target.to(preds.device), num_classes, ignore_index, tol2, state, debug)
