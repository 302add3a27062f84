"""Connected components of label maps: labelling, mask clean-up at prediction time and lesion-wise detection
counts (``csrc/components.hip``).  An addition over the reference, which saves the raw argmax and only scores
overlap (Dice / IoU).

Semantics (both paths implement exactly this):
  * a label plane is uint8 ``[H, W]``; a pixel equal to ``SKIP`` (255) belongs to nothing, any other pixel is
    connected to a neighbour holding the SAME value -- ``connectivity`` 4: the edge neighbours, 8: the diagonal ones
    too.  Every pixel gets the plane-local linear index ``y * W + x`` of the raster-first pixel of its component
    (its *root*), a skipped pixel ``-1``; so all classes of a map, background included, are labelled at once;
  * ``label``: the roots of the set pixels numbered ``1 .. K`` in raster order of the first pixel -- exactly
    ``scipy.ndimage.label`` with the cross (4) or the full 3 x 3 (8) structure;
  * ``postprocess`` applies, in this order: **fill_holes** -- a hole is a 4-connected component of label-0 pixels
    without a pixel on the image frame (always connectivity 4, as ``scipy.ndimage.binary_fill_holes``); all its
    pixels take the label of the pixel immediately left of its raster-first pixel (which exists and is foreground:
    the first pixel is not on the frame and a label-0 left neighbour would belong to the hole), an island of
    another class inside a hole keeps its class; **min_area** -- foreground components (given connectivity, pixels
    connect only within a class) of the map after filling with fewer than ``min_area`` pixels become 0;
    **keep_largest** -- per image and foreground class only the component of largest area survives, a tie goes to
    the raster-first one;
  * ``lesion_stats``: prediction = per-pixel argmax, a pixel whose target is ``ignore_index`` or outside ``[0, C)``
    is in neither mask (the label planes of ``ops/surface.py``).  Per image and foreground class ``c``, ``G`` are the
    components of ``target == c`` and ``P`` those of ``argmax == c``; a component of area ``a`` with ``i`` pixels in
    the other source's class-``c`` mask is a *hit* iff ``i >= 1 and i >= min_overlap * a`` (the product in fp64).
    The state counts, per class: GT components, GT hits, predicted components, predicted hits.

On the GPU with the extension the HIP kernels run (no host synchronisation, scratch cached by shape); otherwise
the plain-torch form below, which is the specification in code and the oracle of the GPU tests.
"""
from __future__ import annotations

import torch

from . import _ext
from .surface import _check_hw, _labels_torch

SKIP = 255
KEY_COLS = 256
MAX_PLANES = 65534          # the lesion counters carry the plane in grid.y


def _native(t):
    return t.is_cuda and _ext.available()


def _check_connectivity(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f'connectivity must be 4 or 8, got {connectivity!r}')


def new_state(num_classes, device=None):
    """Accumulator of :func:`lesion_stats`: ``counts`` int64 ``[4, C-1]`` (GT components, GT hits, predicted
    components, predicted hits) and the kernels' error counter ``err`` int64 ``[1]`` (0 on every correct run)."""
    return {'counts': torch.zeros(4, num_classes - 1, dtype=torch.long, device=device),
            'err': torch.zeros(1, dtype=torch.long, device=device)}


# ---- plain-torch specification ----------------------------------------------------------------------------
def _shift(t, dy, dx, fill):
    """t[..., y + dy, x + dx] with ``fill`` outside the plane"""
    h, w = t.shape[-2:]
    out = torch.full_like(t, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[..., yd, xd] = t[..., ys, xs]
    return out


def _roots_torch(lab, connectivity):
    """lab integer ``[B, H, W]`` -> int64 ``[B, H, W]`` root index (-1 at SKIP pixels) and the number of rounds.
    Min-index propagation over the neighbour shifts with hooking and pointer jumping in between (a serpentine
    of length ~ H*W/2 converges in a dozen rounds, plain propagation needs thousands)."""
    b, h, w = lab.shape
    lab = lab.long()
    valid = lab != SKIP
    big = h * w
    idx = torch.arange(h * w, device=lab.device).view(1, h, w).expand(b, h, w)
    cur = torch.where(valid, idx, torch.full_like(idx, big))
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)]
    if connectivity == 8:
        steps += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    same = [valid & (_shift(lab, dy, dx, -1) == lab) for dy, dx in steps]
    rounds = 0
    while True:
        rounds += 1
        new = cur
        for (dy, dx), s in zip(steps, same):
            new = torch.where(s, torch.minimum(new, _shift(cur, dy, dx, big)), new)
        # hooking: the pixel my label names takes the smallest label seen here, so a low label that enters a long
        # run at its far end reaches the whole run through the run's own first pixel
        flat = new.reshape(b, -1)
        at = cur.reshape(b, -1).clamp_max(big - 1)
        flat = torch.minimum(flat, flat.scatter_reduce(1, at, flat, 'amin', include_self=True))
        for _ in range(3):      # pointer jumping: the label of my label's pixel
            flat = torch.where(flat < big, flat.gather(1, flat.clamp_max(big - 1)), flat)
        new = flat.view(b, h, w)
        if torch.equal(new, cur):
            break
        cur = new
    return torch.where(valid, cur, torch.full_like(cur, -1)), rounds


def _root_sums(root, weight):
    """int64 ``[B, H*W]``: at every root position the sum of ``weight`` over its component (0 elsewhere)"""
    b = root.shape[0]
    flat = root.reshape(b, -1)
    out = torch.zeros_like(flat)
    return out.scatter_add_(1, flat.clamp_min(0), (weight.reshape(b, -1) & (flat >= 0)).long())


def _at_root(sums, root):
    """gather ``sums [B, H*W]`` at every pixel's root (0 at skipped pixels) -> ``[B, H, W]``"""
    flat = root.reshape(root.shape[0], -1)
    return torch.where(flat >= 0, sums.gather(1, flat.clamp_min(0)), torch.zeros_like(flat)).view(root.shape)


def _planes_of_mask(mask):
    h, w = mask.shape[-2:]
    m = (mask != 0).reshape(-1, h, w)
    return torch.where(m, 1, SKIP).to(torch.uint8).contiguous()


def _label_torch(lab, connectivity):
    root, _ = _roots_torch(lab, connectivity)
    b, h, w = root.shape
    idx = torch.arange(h * w, device=root.device).view(1, -1)
    flat = root.reshape(b, -1)
    rank = (flat == idx).long().cumsum(1)
    labels = torch.where(flat >= 0, rank.gather(1, flat.clamp_min(0)), torch.zeros_like(flat))
    return labels.view(b, h, w).to(torch.int32), rank[:, -1].clone()


def _areas_torch(lab, connectivity):
    root, _ = _roots_torch(lab, connectivity)
    return _at_root(_root_sums(root, root >= 0), root).to(torch.int32)


def _postprocess_torch(lab, fill_holes, min_area, keep_largest, connectivity):
    b, h, w = lab.shape
    lab = lab.long()
    if fill_holes:
        root, _ = _roots_torch(lab, 4)
        frame = torch.zeros(b, h, w, dtype=torch.bool, device=lab.device)
        frame[:, 0], frame[:, -1], frame[:, :, 0], frame[:, :, -1] = True, True, True, True
        touches = _at_root(_root_sums(root, frame), root)
        hole = (lab == 0) & (touches == 0)
        left = lab.reshape(b, -1).gather(1, (root.reshape(b, -1) - 1).clamp_min(0)).view(b, h, w)
        lab = torch.where(hole, left, lab)
    if min_area > 0 or keep_largest:
        root, _ = _roots_torch(lab, connectivity)
        sums = _root_sums(root, root >= 0)
        area = _at_root(sums, root)
        fg = lab != 0
        keep = fg & (area >= min_area)
        if keep_largest:
            flat, lf = root.reshape(b, -1), lab.reshape(b, -1)
            idx = torch.arange(h * w, device=lab.device).view(1, -1)
            is_root = (flat == idx) & (lf != 0)
            key = torch.where(is_root, (sums << 32) | (0xffffffff - idx), torch.zeros_like(sums))
            best = torch.zeros(b, KEY_COLS, dtype=torch.long, device=lab.device)
            best.scatter_reduce_(1, lf, key, 'amax', include_self=True)
            winner = 0xffffffff - (best & 0xffffffff)
            keep &= (winner.gather(1, lf) == flat).view(b, h, w)
        lab = torch.where(keep, lab, torch.zeros_like(lab))
    return lab.to(torch.uint8)


def _lesion_planes_torch(preds, target, num_classes, ignore_index):
    pl, tl = _labels_torch(preds, target, num_classes, ignore_index)
    lab = torch.cat([pl, tl])
    return torch.where(lab < 0, torch.full_like(lab, SKIP), lab)


def _lesion_stats_torch(preds, target, num_classes, ignore_index, min_overlap, connectivity, state, debug):
    n, _, h, w = preds.shape
    k = num_classes - 1
    lab = _lesion_planes_torch(preds, target, num_classes, ignore_index)          # [2n, H, W]
    root, _ = _roots_torch(lab, connectivity)
    area = _root_sums(root, root >= 0)
    inter = _root_sums(root, lab == lab.roll(n, 0))
    lf = lab.reshape(2 * n, -1)
    idx = torch.arange(h * w, device=lab.device).view(1, -1)
    comp = (root.reshape(2 * n, -1) == idx) & (lf >= 1) & (lf <= k)
    hit = comp & (inter >= 1) & (inter.double() >= float(min_overlap) * area.double())
    cls = (lf - 1).clamp(0, k - 1)
    per = torch.zeros(n, k, 4, dtype=torch.long, device=lab.device)
    for src, col in ((1, 0), (0, 2)):           # target planes -> columns 0, 1; prediction planes -> 2, 3
        sl = slice(src * n, (src + 1) * n)
        for j, flag in enumerate((comp, hit)):
            per[:, :, col + j] = torch.zeros(n, k, dtype=torch.long, device=lab.device).scatter_add_(
                1, cls[sl], flag[sl].long())
    state['counts'] += per.sum(0).t().to(state['counts'].device)
    return {'per_image': per, 'err': state['err'].clone()} if debug else None


# ---- device path ------------------------------------------------------------------------------------------
_SCRATCH = {}


def _scratch(device, b, h, w):
    """Work buffers of one labelling, cached for the last shape seen per device (re-sized when it changes)."""
    key = (b, h, w)
    hit = _SCRATCH.get(device)
    if hit is None or hit[0] != key:
        i32 = dict(dtype=torch.int32, device=device)
        hit = (key, {'lab': torch.empty(b, h, w, dtype=torch.uint8, device=device),
                     'tmp': torch.empty(b, h, w, dtype=torch.uint8, device=device),
                     'root': torch.empty(b, h, w, **i32), 'area': torch.empty(b, h, w, **i32),
                     'aux': torch.empty(b, h, w, **i32), 'err': torch.zeros(1, **i32),
                     'key': torch.empty(b, KEY_COLS, dtype=torch.long, device=device)})
        _SCRATCH[device] = hit
    return hit[1]


def _check_planes(b, h, w):
    _check_hw(h, w, b)
    if b * ((h + 31) // 32) * ((w + 31) // 32) > 2 ** 31 - 1:
        raise ValueError(f'connected components: {b} images of {h} x {w} are too many tiles for one call')


def _label_device(lab, connectivity, want_areas):
    C = _ext.require()
    b, h, w = lab.shape
    _check_planes(b, h, w)
    i32 = dict(dtype=torch.int32, device=lab.device)
    root, area, aux = (torch.empty(b, h, w, **i32) for _ in range(3))
    err = torch.zeros(1, **i32)
    C.cc_label(lab, root, area, aux, err, 0, connectivity, 0)
    if want_areas:
        C.cc_gather(root, area, aux)
        return aux, None, err
    num = torch.empty(b, dtype=torch.long, device=lab.device)
    C.cc_rank(root, aux, num)
    C.cc_gather(root, aux, area)
    return area, num, err


def _postprocess_device(lab, fill_holes, min_area, keep_largest, connectivity):
    C = _ext.require()
    b, h, w = lab.shape
    _check_planes(b, h, w)
    s = _scratch(lab.device, b, h, w)
    cur = lab
    errors = torch.zeros(1, dtype=torch.int32, device=lab.device)     # every labelling zeroes its own counter
    if fill_holes:
        C.cc_label(cur, s['root'], s['area'], s['aux'], s['err'], 0, 4, 0)
        errors += s['err']
        C.cc_apply(cur, s['root'], s['area'], s['aux'], None, s['tmp'], 0, 0)
        cur = s['tmp']
    if min_area > 0 or keep_largest:
        C.cc_label(cur, s['root'], s['area'], s['aux'], s['err'], 0, connectivity, 0)
        errors += s['err']
        if keep_largest:
            C.cc_largest(cur, s['root'], s['area'], s['key'])
        out = torch.empty_like(lab)
        C.cc_apply(cur, s['root'], s['area'], s['aux'], s['key'] if keep_largest else None, out, 1, min_area)
        return out, errors
    return cur.clone(), errors


def _lesion_stats_device(preds, target, num_classes, ignore_index, min_overlap, connectivity, state, debug):
    C = _ext.require()
    n, _, h, w = preds.shape
    k = num_classes - 1
    if 2 * n > MAX_PLANES:
        raise ValueError(f'lesion_stats: at most {MAX_PLANES // 2} images per call, got {n}')
    _check_planes(2 * n, h, w)
    s = _scratch(preds.device, 2 * n, h, w)
    ig = ignore_index if ignore_index is not None else -1
    C.surface_labels(preds, target, s['lab'], ig)          # [2 (prediction, target), n] planes, 255 = no class
    C.cc_label(s['lab'], s['root'], s['area'], s['aux'], s['err'], n, connectivity, 1)
    per = torch.zeros(n, k, 4, dtype=torch.long, device=preds.device) if debug else None
    C.cc_lesion(s['lab'], s['root'], s['area'], s['aux'], s['err'], state['counts'], state['err'], per, k,
                float(min_overlap))
    return {'per_image': per, 'err': state['err'].clone()} if debug else None


# ---- public ops -------------------------------------------------------------------------------------------
def label(mask, connectivity=8):
    """``(labels, num)``: ``labels`` int32 ``[..., H, W]`` numbers the components of ``mask != 0`` from 1 in raster
    order of their first pixel (0 = unset) and ``num`` int64 ``[...]`` counts them, per image -- elementwise
    ``scipy.ndimage.label`` with the cross (``connectivity`` 4) or the full 3 x 3 structure (8)."""
    _check_connectivity(connectivity)
    h, w = mask.shape[-2:]
    lead = mask.shape[:-2]
    if mask.numel() == 0:
        return (torch.zeros(mask.shape, dtype=torch.int32, device=mask.device),
                torch.zeros(lead, dtype=torch.long, device=mask.device))
    _check_hw(h, w)
    lab = _planes_of_mask(mask)
    if _native(mask):
        labels, num, _ = _label_device(lab, connectivity, False)
    else:
        labels, num = _label_torch(lab, connectivity)
    return labels.view(mask.shape), num.view(lead)


def component_areas(mask, connectivity=8):
    """int32 ``[..., H, W]``: at every pixel of ``mask != 0`` the area of its component, 0 elsewhere."""
    _check_connectivity(connectivity)
    if mask.numel() == 0:
        return torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
    _check_hw(*mask.shape[-2:])
    lab = _planes_of_mask(mask)
    if _native(mask):
        return _label_device(lab, connectivity, True)[0].view(mask.shape)
    return _areas_torch(lab, connectivity).view(mask.shape)


def label_errors(mask, connectivity=8):
    """The labelling kernels' error counter for ``mask`` (int32 ``[1]``; loops that hit their iteration cap): 0 on
    every correct run, and always 0 on the plain-torch path."""
    _check_connectivity(connectivity)
    if not _native(mask) or mask.numel() == 0:
        return torch.zeros(1, dtype=torch.int32, device=mask.device)
    return _label_device(_planes_of_mask(mask), connectivity, True)[2]


def postprocess(labels, num_classes, fill_holes=False, min_area=0, keep_largest=False, connectivity=8, native=None,
                debug=False):
    """Cleaned uint8 label map of the shape of ``labels`` (integer ``[N, H, W]``, values in ``[0, num_classes)``):
    fill_holes, then min_area, then keep_largest (module docstring).  With all three off ``labels`` itself is
    returned.  ``native=False`` runs the plain-torch form on the tensor's device.

    The label values are not checked by default (the check reads the tensor back).  ``debug`` checks them and
    returns ``(cleaned, errors)``: ``errors`` int32 ``[1]`` sums the labelling kernels' error counter over the
    labellings of this call (0 on every correct run and on the plain-torch path; a nonzero value means the map
    is not to be trusted)."""
    _check_connectivity(connectivity)
    min_area = int(min_area)
    if min_area < 0:
        raise ValueError(f'min_area must be >= 0, got {min_area}')
    if not 1 <= num_classes <= SKIP:
        raise ValueError(f'num_classes must be in [1, {SKIP}], got {num_classes}')
    if labels.dim() != 3 or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f'labels must be an integer [N, H, W] map, got {labels.dtype} {tuple(labels.shape)}')
    errors = torch.zeros(1, dtype=torch.int32, device=labels.device)
    if debug and labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= num_classes):
        raise ValueError(f'labels must lie in [0, {num_classes}), got [{int(labels.min())}, {int(labels.max())}]')
    if not (fill_holes or min_area > 0 or keep_largest):
        return (labels, errors) if debug else labels
    if labels.numel() == 0:
        return (labels.to(torch.uint8), errors) if debug else labels.to(torch.uint8)
    _check_hw(*labels.shape[-2:])
    if native is None:
        native = _native(labels)
    lab = labels.to(torch.uint8).contiguous()
    if native:
        out, errors = _postprocess_device(lab, bool(fill_holes), min_area, bool(keep_largest), connectivity)
    else:
        out = _postprocess_torch(lab, bool(fill_holes), min_area, bool(keep_largest), connectivity)
    return (out, errors) if debug else out


def lesion_stats(preds, target, num_classes, ignore_index=None, min_overlap=0.0, connectivity=8, state=None,
                 debug=False, native=None):
    """Add the lesion-wise counts of one batch into ``state`` (see :func:`new_state`).

    preds ``[N, C, H, W]`` fp32 logits (C == num_classes >= 2), target ``[N, H, W]`` integer labels.  With ``debug``
    returns ``per_image`` int64 ``[N, C-1, 4]`` (GT components, GT hits, predicted components, predicted hits per
    image and foreground class) and ``err``, the state's error counter after this batch.  ``native=False`` runs
    the plain-torch form on the tensors' device (benchmarks, oracles)."""
    if preds.dim() != 4 or preds.shape[1] != num_classes or num_classes < 2:
        raise ValueError(f'preds must be [N, {num_classes}, H, W] with num_classes >= 2, got {tuple(preds.shape)}')
    if target.shape != preds.shape[:1] + preds.shape[2:]:
        raise ValueError(f'target must be [N, H, W] = {tuple(preds.shape[:1] + preds.shape[2:])}, '
                         f'got {tuple(target.shape)}')
    if num_classes > SKIP:
        raise ValueError(f'num_classes must be <= {SKIP}')
    if not 0.0 <= float(min_overlap) <= 1.0:
        raise ValueError(f'min_overlap must be in [0, 1], got {min_overlap}')
    _check_connectivity(connectivity)
    _check_hw(preds.shape[2], preds.shape[3])
    if state is None:
        state = new_state(num_classes, preds.device)
    if preds.shape[0] == 0:
        return None
    if native is None:
        native = _native(preds) and state['counts'].is_cuda
    if native:
        return _lesion_stats_device(preds.contiguous().float(), target.contiguous().long(), num_classes,
                                    ignore_index, min_overlap, connectivity, state, debug)
    return _lesion_stats_torch(preds.float(), target.to(preds.device), num_classes, ignore_index, min_overlap,
                               connectivity, state, debug)
