"""Fused loss kernels (``csrc/loss.hip``) as autograd Functions over NCHW fp32 logits.

* :func:`cross_entropy` == ``nn.CrossEntropyLoss(weight, ignore_index, reduction='mean')``
  (reference ``core/loss.py:30-31``): one kernel computes the loss partials and d(loss)/d(logits);
  backward is a scalar rescale, no second pass over the logits.
* :func:`ohem_cross_entropy` == reference ``OhemCELoss`` (``core/loss.py:6-20``): the per-pixel
  losses come from the same fused kernel; the selection (threshold, exact top-k fallback by radix
  select) runs in device kernels with no host sync, so OHEM steps are graph-captured too.
* :func:`kd_kl_div` == ``F.kl_div(log_softmax(s/T), softmax(t/T)) * T**2`` with the default
  elementwise-mean reduction (reference ``core/loss.py:42-46``).
* :func:`kd_mse` == ``F.mse_loss(s, t)`` (reference ``core/loss.py:47-48``), one fused pass.
* :func:`bce_dice` == ``bw * BCEWithLogits + dw * (1 - mean_n soft-Dice_n)`` for binary heads
  (``num_class == 1``): a per-sample reduction kernel in forward, the gradient
  kernel in backward (it needs the sample's Dice sums), upstream gradient read on the device.
* :func:`region_loss` == ``pw * pixel + rw * region`` for softmax heads (``num_class >= 2``; the
  plain-torch form is ``core.loss.RegionLoss``): pixel term CE or focal (weighted mean over the valid
  pixels), region term per-sample soft Dice / Tversky on the softmax.  Forward is the per-sample
  statistics pass plus a one-block finalize (coefficient table and loss scalar stay on the device);
  backward is one gradient pass that recomputes the softmax.  No atomics, no host read: bitwise
  repeatable and graph-capturable like the others.
* :func:`boundary_loss`: the softmax integrated against the signed distance map of the labels (the
  plain-torch form is ``core.loss.BoundaryLoss``); the map comes from ``csrc/surface.hip`` inside the
  same call and is kept as int32 squared distances for the gradient pass.
* :func:`lovasz_softmax`: the Lovasz-softmax loss (the plain-torch form is ``core.loss.LovaszSoftmaxLoss``) on
  the segmented radix sort of ``csrc/sort.hip``; the kernels are ``csrc/lovasz.hip``.
"""
from __future__ import annotations

import math

import torch

from ._ext import require


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index):
        C = require()
        logits = logits.contiguous().float()
        target = target.contiguous().long()
        n, c, h, w = logits.shape
        grad = torch.empty_like(logits)
        part = torch.empty(C.ce_blocks(n * h * w), 2, dtype=torch.float32, device=logits.device)
        C.ce_fwd_bwd(logits, target, weight, grad, None, part, ignore_index)
        tot = part.sum(0)
        ctx.save_for_backward(grad, tot)
        return tot[0] / tot[1]

    @staticmethod
    def backward(ctx, g):
        grad, tot = ctx.saved_tensors
        return grad * (g / tot[1]), None, None, None


def cross_entropy(logits, target, weight=None, ignore_index=255):
    if weight is not None:
        weight = weight.to(device=logits.device, dtype=torch.float32).contiguous()
    return _CE.apply(logits, target, weight, ignore_index)


class _OHEM(torch.autograd.Function):
    """Per-pixel CE from the fused kernel; hard-pixel selection (threshold, else exact top-k) entirely on
    the device (``loss.hip`` ohem_*): no host synchronisation, so the step stays graph-capturable.

    Two documented differences from the reference ``OhemCELoss`` (``core/loss.py:6-20``):
      * no valid pixel at all (n_min = 0) and none above the threshold: the loss is 0 here, the
        reference's ``torch.mean`` of an empty tensor is NaN;
      * pixels tied at the k-th largest loss in the top-k fallback each get the fractional weight
        (n_min - #greater) / #tied, where ``torch.topk`` gives the full 1/n_min to an arbitrary subset of
        them: the loss VALUE is identical, the per-pixel gradients differ on the tied pixels only.
        Tests that compare gradients bit-for-bit use tie-free inputs."""

    @staticmethod
    def forward(ctx, logits, target, thresh, ignore_index):
        C = require()
        logits = logits.contiguous().float()
        target = target.contiguous().long()
        n, c, h, w = logits.shape
        dev = logits.device
        grad = torch.empty_like(logits)
        P = n * h * w
        pix = torch.empty(P, dtype=torch.float32, device=dev)
        nb = C.ce_blocks(P)
        part = torch.empty(nb, 2, dtype=torch.float32, device=dev)
        C.ce_fwd_bwd(logits, target, None, grad, pix, part, ignore_index)
        bpart = torch.empty(nb, 3, dtype=torch.float32, device=dev)
        state = torch.empty(C.ohem_state_words(), dtype=torch.int32, device=dev)
        hist = torch.empty(256, dtype=torch.int32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        C.ohem_select(pix, target, thresh, ignore_index, bpart, state, hist, loss)
        ctx.save_for_backward(grad, pix, state)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        grad, pix, state = ctx.saved_tensors
        out = grad.clone()
        require().ohem_backward(out, pix, state, g.reshape(1).float().contiguous())
        return out, None, None, None


def ohem_cross_entropy(logits, target, thresh=0.7, ignore_index=255):
    return _OHEM.apply(logits, target, -math.log(thresh), ignore_index)


class _KDKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, T):
        C = require()
        s = s.contiguous().float()
        t = t.detach().contiguous().float()
        grad = torch.empty_like(s)
        n, c, h, w = s.shape
        part = torch.empty(C.ce_blocks(n * h * w), dtype=torch.float32, device=s.device)
        C.kd_kl_fwd_bwd(s, t, grad, part, T)
        ctx.save_for_backward(grad)
        return part.sum() * (T * T) / s.numel()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def kd_kl_div(student, teacher, T=4.0):
    return _KDKL.apply(student, teacher, float(T))


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t):
        C = require()
        s = s.contiguous().float()
        t = t.detach().contiguous().float()
        grad = torch.empty_like(s)
        part = torch.empty(C.ce_blocks(s.numel()), dtype=torch.float32, device=s.device)
        C.mse_fwd_bwd(s, t, grad, part)
        ctx.save_for_backward(grad)
        return part.sum() / s.numel()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def kd_mse(student, teacher):
    return _MSE.apply(student, teacher)


class _BCEDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, bw, dw, smooth):
        C = require()
        x = logits.contiguous().float()
        t = target.contiguous().float().view_as(x)
        n = x.shape[0]
        hw = x.numel() // n
        part = torch.empty(n, C.bce_dice_splits(hw), 4, dtype=torch.float32, device=x.device)
        C.bce_dice_stats(x, t, part)
        sums = part.sum(1)                                    # [N, 4]: BCE, p*t, p, t
        den = sums[:, 2] + sums[:, 3] + smooth
        num = 2 * sums[:, 1] + smooth
        loss = bw * sums[:, 0].sum() / x.numel() + dw * (1 - (num / den).mean())
        ctx.save_for_backward(x, t, torch.stack([den, num], 1).contiguous())
        ctx.bw, ctx.dw = bw, dw
        return loss

    @staticmethod
    def backward(ctx, g):
        C = require()
        x, t, coef = ctx.saved_tensors
        grad = torch.empty_like(x)
        C.bce_dice_grad(x, t, coef, g.detach().float().reshape(1).contiguous(), grad, ctx.bw, ctx.dw)
        return grad, None, None, None, None


def bce_dice(logits, target, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
    return _BCEDice.apply(logits, target, float(bce_weight), float(dice_weight), float(smooth))


_PIX = {None: 0, 'ce': 1, 'focal': 2}


class _Region(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, pix, gamma, pw, rw, a, b, smooth, c0):
        C = require()
        x = logits.contiguous().float()
        t = target.contiguous().long()
        n, c, h, w = x.shape
        dev = x.device
        part = torch.empty(n, C.region_splits(h * w), 2 + 3 * c, dtype=torch.float32, device=dev)
        coef = torch.empty(2 * n * c + 1, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        C.region_fwd(x, t, weight, part, coef, loss, ignore_index, pix, gamma, pw, rw, a, b, smooth, c0)
        ctx.save_for_backward(x, t, coef, weight)
        ctx.args = (ignore_index, pix, gamma, pw, rw, a, b, c0)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, t, coef, weight = ctx.saved_tensors
        grad = torch.empty_like(x)
        require().region_grad(x, t, weight, coef, g.detach().float().reshape(1).contiguous(), grad, *ctx.args)
        return (grad,) + (None,) * 11


class _Boundary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, classes):
        C = require()
        x = logits.contiguous().float()
        t = target.contiguous().long()
        n, c, h, w = x.shape
        dev = x.device
        s = torch.empty(n, len(classes), h, w, dtype=torch.int32, device=dev)
        C.sdf_sq(t, s, classes, c, ignore_index)
        part = torch.empty(C.boundary_blocks(n * h * w), 2, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)        # loss, 1 / (K max(V, 1))
        C.boundary_fwd(x, t, s, classes, part, out[:1], out[1:], ignore_index)
        ctx.save_for_backward(x, t, s, out)
        ctx.args = (ignore_index, classes)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x, t, s, out = ctx.saved_tensors
        ignore_index, classes = ctx.args
        grad = torch.empty_like(x)
        require().boundary_grad(x, t, s, classes, out[1:], g.detach().float().reshape(1).contiguous(), grad,
                                ignore_index)
        return grad, None, None, None


LOVASZ_WS_BYTES = 2 << 30     # bound of the sort workspace of one class chunk


def lovasz_chunk_classes(n, c, hw, per_image):
    """Classes sorted per chunk: as many as keep ``16 * CK * N * H * W`` bytes under ``LOVASZ_WS_BYTES`` (at least
    one), and the chunk's rows ``S * CK`` within the launch grid."""
    ck = max(1, min(c, LOVASZ_WS_BYTES // (16 * n * hw)))
    return max(1, min(ck, 65535 // n)) if per_image else ck


class _Lovasz(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, per_image, c0):
        C = require()
        x = logits.contiguous().float()
        t = target.contiguous().long()
        n, c, h, w = x.shape
        dev = x.device
        S, P = (n, h * w) if per_image else (1, n * h * w)
        nblk = -(-P // C.lovasz_tile())
        ck = lovasz_chunk_classes(n, c, h * w, per_image)
        i32 = dict(dtype=torch.int32, device=dev)
        ws = torch.empty(4 * S * ck * P, **i32)                     # keys and payload, in and out of a pass
        table = torch.empty(S * ck, C.sort_bins(), -(-P // C.sort_tile()), **i32)
        dtot = torch.empty(S * ck, C.sort_bins(), **i32)
        cnt, gtot = torch.empty(S * c, nblk, **i32), torch.empty(S * c, **i32)
        part = torch.empty(S * c, nblk, dtype=torch.float32, device=dev)
        coef = torch.empty_like(x)
        out = torch.empty(2 * S * c + 1, dtype=torch.float32, device=dev)   # row loss, scale, loss
        for lo in range(0, c, ck):
            k = min(ck, c - lo)
            C.lovasz_chunk(x, t, ws[:4 * S * k * P], table, dtot, cnt, gtot, part, coef, ignore_index, per_image,
                           lo, k)
        scale, loss = out[S * c:2 * S * c], out[2 * S * c:]
        C.lovasz_finalize(x, t, part, gtot, out[:S * c], scale, loss, per_image, c0)
        ctx.save_for_backward(x, t, coef, scale)
        ctx.args = (ignore_index, per_image)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, t, coef, scale = ctx.saved_tensors
        grad = torch.empty_like(x)
        require().lovasz_grad(x, t, coef, scale, g.detach().float().reshape(1).contiguous(), grad, *ctx.args)
        return grad, None, None, None, None


def lovasz_softmax(logits, target, ignore_index=255, per_image=False, ignore_background=False):
    """Lovasz-softmax loss (Berman et al., CVPR 2018), 'present' classes, on fp32 NCHW logits and int64
    ``[N, H, W]`` labels; the plain-torch form and the definition are ``core.loss.LovaszSoftmaxLoss``.

    Per segment (the batch, or each image with ``per_image``) and class the errors ``|y - p_c|`` of all pixels
    (0 at invalid ones) are sorted descending, ties in ascending pixel index, by ``csrc/sort.hip``; one pass along
    the sorted order turns the running integer counts into the Lovasz gradient ``g``, sums ``e g`` and scatters
    ``sign(p - y) g`` back to pixel order; a one-block finalize takes the mean over the present classes and the
    segments.  Backward is one pass that recomputes the softmax.  No float atomics, no host read: bitwise
    repeatable and graph-capturable.  The batch-mode sort is over the rank's own micro-batch: nothing is exchanged
    across DDP ranks or accumulation micro-batches, the same semantics as ``cross_entropy``.

    ``C <= 64``, segment length ``< 2^31``.  Classes are sorted in chunks of ``CK = lovasz_chunk_classes(...)``;
    peak workspace in bytes, with ``V = N * H * W``, ``T = sort_tile()``, rows ``R = S * C`` and ``Rk = S * CK``:
    ``16 * CK * V`` (keys and payload, in and out of a pass) ``+ 4 * 256 * Rk * (ceil(P / T) + 1)`` (digit table)
    ``+ 8 * R * ceil(P / T) + 12 * R`` (counts, partials, per-row results) ``+ 4 * C * V`` (the coefficient tensor
    kept for backward)."""
    if logits.dim() != 4 or target.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f'lovasz_softmax: logits [N, C, H, W] and target [N, H, W], got {tuple(logits.shape)} and '
                         f'{tuple(target.shape)}')
    n, c, h, w = logits.shape
    if c == 1:
        raise ValueError('lovasz_softmax needs a softmax head: num_class must be >= 2, got 1')
    if c > 64:
        raise RuntimeError(f'lovasz loss: num_class must be in [2, 64], got {c}')
    if (h * w if per_image else n * h * w) >= 1 << 31:
        raise RuntimeError(f'lovasz loss: segment length must be < 2^31, got {h * w if per_image else n * h * w}')
    return _Lovasz.apply(logits, target, int(ignore_index), bool(per_image), 1 if ignore_background else 0)


def boundary_loss(logits, target, ignore_index=255, classes=None):
    """Boundary loss (Kervadec et al., MIDL 2019) on fp32 NCHW logits and int64 ``[N, H, W]`` labels:
    ``sum_{n, c in classes, valid x} softmax(logits)_c(x) * phi_nc(x) / (len(classes) * max(V, 1))`` with ``phi``
    the signed distance map of ``ops.surface.signed_distance`` (negative inside class ``c``; 0 for a class that is
    absent from or fills the image) and ``V`` the valid pixels of the batch.  ``classes`` defaults to
    ``1 .. C-1``.  The distance map is computed on the device from the labels of this call (column + row pass),
    then one pass for the loss and one for the gradient; no atomics, no host read: bitwise repeatable and
    graph-capturable.  A mean over the rank's own valid pixels, like ``cross_entropy``: nothing is exchanged
    under DDP.  H, W <= 2048, C <= 64."""
    from .surface import _check_sdf_hw, _sdf_classes
    if logits.dim() != 4 or target.shape != logits.shape[:1] + logits.shape[2:]:
        raise ValueError(f'boundary_loss: logits [N, C, H, W] and target [N, H, W], got {tuple(logits.shape)} and '
                         f'{tuple(target.shape)}')
    if logits.shape[1] > 64:
        raise RuntimeError(f'boundary loss: num_class must be in [2, 64], got {logits.shape[1]}')
    cls = _sdf_classes(logits.shape[1], classes)
    _check_sdf_hw(logits.shape[2], logits.shape[3])
    return _Boundary.apply(logits, target, int(ignore_index), cls)


def region_loss(logits, target, weight=None, ignore_index=255, pixel='ce', region='dice', pixel_weight=1.0,
                region_weight=1.0, smooth=1.0, alpha=0.3, beta=0.7, gamma=2.0, ignore_background=False):
    """``pixel_weight * L_pix + region_weight * L_reg`` on fp32 NCHW logits and int64 ``[N, H, W]`` labels.

    ``pixel``: None | 'ce' | 'focal' (``gamma`` 0 or >= 1; 0 is CE); ``region``: None | 'dice' | 'tversky'
    (``alpha`` / ``beta`` weigh false positives / negatives; Dice is Tversky(0.5, 0.5) with ``smooth / 2``,
    i.e. ``(2I + smooth) / (P + T + smooth)``).  A pixel counts iff ``target != ignore_index`` and
    ``0 <= target < C``.  The region sums are per sample, so nothing is exchanged across DDP ranks: each
    rank's loss is the mean over its own samples, the same semantics as ``cross_entropy``."""
    if pixel not in _PIX or region not in (None, 'dice', 'tversky') or (pixel is None and region is None):
        raise ValueError(f'region_loss: pixel={pixel!r} region={region!r}')
    gamma = float(gamma)
    if pixel == 'focal' and not (gamma == 0.0 or gamma >= 1.0):
        raise ValueError(f'focal_gamma must be 0 or >= 1, got {gamma}')
    pix = 1 if pixel == 'focal' and gamma == 0.0 else _PIX[pixel]
    a, b, s = (0.5, 0.5, 0.5 * smooth) if region == 'dice' else (alpha, beta, smooth)
    if weight is not None:
        weight = weight.to(device=logits.device, dtype=torch.float32).contiguous()
    return _Region.apply(logits, target, weight, int(ignore_index), pix, gamma if pix == 2 else 0.0,
                         float(pixel_weight) if pixel is not None else 0.0,
                         float(region_weight) if region is not None else 0.0, float(a), float(b), float(s),
                         1 if ignore_background else 0)
