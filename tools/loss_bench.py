#!/usr/bin/env python3
"""Forward + backward time of the fused losses at the bench shapes: ``cross_entropy`` (one pass) against
every softmax-head region loss type (two passes), with HIP events.  Bytes moved are the compulsory
traffic of the loss kernels: CE reads logits + int64 labels and writes the gradient (its backward then
rescales that gradient with a torch op, one more read + write, listed apart); a region loss reads logits +
labels in each of its two passes and writes the gradient once.  From bytes alone a region loss should take
(2 (L + T) + L) / (2 L + T) of the CE kernel's time: 1.67x at C = 2.

    python tools/loss_bench.py [--iters 20] [--out profiles/region_loss/loss_bench.json]

``--mode boundary`` times the boundary (signed-distance) term instead, see :func:`boundary_mode`:

    python tools/loss_bench.py --mode boundary [--iters 10] [--trials 5] [--out profiles/boundary_loss/boundary_bench.json]

``--mode lovasz`` times the Lovasz-softmax loss against its plain-torch form and CE, see :func:`lovasz_mode`:

    python tools/loss_bench.py --mode lovasz [--iters 5] [--trials 3] [--out profiles/lovasz_loss/lovasz_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from medical_segmentation_pytorch_amd.ops.losses import cross_entropy, region_loss  # noqa: E402

TYPES = {'dice': (None, 'dice'), 'tversky': (None, 'tversky'), 'focal': ('focal', None), 'ce_dice': ('ce', 'dice'),
         'ce_tversky': ('ce', 'tversky'), 'focal_dice': ('focal', 'dice'), 'focal_tversky': ('focal', 'tversky')}


def timeit(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _blob_labels(n, c, h, w, dev):
    """A few discs per foreground class and image on background 0, two ignored rows: lesion-like targets."""
    g = torch.Generator(device='cpu').manual_seed(0)
    ys = torch.arange(h, device=dev).view(1, h, 1)
    xs = torch.arange(w, device=dev).view(1, 1, w)
    t = torch.zeros(n, h, w, dtype=torch.long, device=dev)
    for k in range(1, c):
        for _ in range(3):
            cy = torch.randint(0, h, (n, 1, 1), generator=g).to(dev)
            cx = torch.randint(0, w, (n, 1, 1), generator=g).to(dev)
            r = torch.randint(4, max(5, min(h, w) // 5), (n, 1, 1), generator=g).to(dev)
            t[(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = k
    t[:, :2] = 255
    return t


def _baseline_phi(t, c, classes):
    """The signed distance map with the ops that predate ``signed_distance``: two ``edt_sq`` per class plus torch
    select / sign / sqrt."""
    from medical_segmentation_pytorch_amd.ops.surface import edt_sq
    valid = (t != 255) & (t >= 0) & (t < c)
    planes = []
    for k in classes:
        pos, neg = valid & (t == k), valid & (t != k)
        live = (pos.flatten(1).any(1) & neg.flatten(1).any(1)).view(-1, 1, 1)
        to_pos, to_neg = edt_sq(pos).float().sqrt(), edt_sq(neg).float().sqrt()
        phi = torch.where(neg, to_pos, torch.zeros_like(to_pos)) - torch.where(pos, to_neg - 1.0,
                                                                               torch.zeros_like(to_neg))
        planes.append(torch.where(live, phi, torch.zeros_like(phi)))
    return torch.stack(planes, 1), valid


def boundary_mode(a):
    """The boundary term at the bench shapes: signed-distance pass, loss forward and loss backward of the fused
    path, each timed alone, against the same tensors from two ``edt_sq`` calls per class plus torch glue and an
    autograd softmax * phi mean.  Every figure is the median of ``--trials`` windows of ``--iters`` calls; the
    baseline's run-to-run spread (max - min over the trials) is reported with the ratio."""
    from medical_segmentation_pytorch_amd.ops._ext import require
    from medical_segmentation_pytorch_amd.ops.losses import boundary_loss
    from medical_segmentation_pytorch_amd.ops.surface import signed_distance
    C = require()
    dev = torch.device('cuda', 0)
    rows = []
    for n, c, h, w in a.shapes or [(320, 2, 352, 352), (64, 4, 352, 352)]:
        torch.manual_seed(0)
        x = torch.randn(n, c, h, w, device=dev, requires_grad=True)
        t = _blob_labels(n, c, h, w, dev)
        classes = list(range(1, c))
        s = signed_distance(t, c, 255, classes, squared=True)
        part = torch.empty(C.boundary_blocks(n * h * w), 2, device=dev)
        out = torch.empty(2, device=dev)
        gup = torch.ones(1, device=dev)
        grad = torch.empty_like(x)
        xd = x.detach()

        def base_loss(phi, valid):
            p = torch.softmax(x, 1)[:, classes]
            return (p * phi).sum() / (len(classes) * valid.sum().clamp_min(1))

        phi_b, valid_b = _baseline_phi(t, c, classes)
        same = bool(torch.equal(phi_b, signed_distance(t, c, 255, classes)))
        x.grad = None
        lb = base_loss(phi_b, valid_b)
        lb.backward()
        gb = x.grad.clone()
        x.grad = None
        lf = boundary_loss(x, t, 255, classes)
        lf.backward()
        agree = {'phi_bitwise_equal': same, 'loss_fused': lf.item(), 'loss_baseline': lb.item(),
                 'grad_rel_l2': ((x.grad - gb).norm() / gb.norm()).item()}

        def base_step():
            x.grad = None
            base_loss(phi_b, valid_b).backward()

        def fused_step():
            x.grad = None
            boundary_loss(x, t, 255, classes).backward()

        cases = {
            'fused_sdf': lambda: C.sdf_sq(t, s, classes, c, 255),
            'fused_fwd': lambda: C.boundary_fwd(xd, t, s, classes, part, out[:1], out[1:], 255),
            'fused_bwd': lambda: C.boundary_grad(xd, t, s, classes, out[1:], gup, grad, 255),
            'fused_all': fused_step,
            'baseline_sdf': lambda: _baseline_phi(t, c, classes),
            'baseline_loss_fwd_bwd': base_step,
        }
        ms = {k: [] for k in cases}
        for _ in range(a.trials):                      # the variants alternate inside every trial
            for k, fn in cases.items():
                ms[k].append(timeit(fn, a.iters, warmup=2))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        base = [ms['baseline_sdf'][i] + ms['baseline_loss_fwd_bwd'][i] for i in range(a.trials)]
        base_med = sorted(base)[len(base) // 2]
        row = {'shape': [n, c, h, w], 'classes': classes, 'ms_median': {k: round(v, 4) for k, v in med.items()},
               'ms_trials': {k: [round(u, 4) for u in v] for k, v in ms.items()},
               'baseline_total_ms': round(base_med, 4), 'baseline_spread_ms': round(max(base) - min(base), 4),
               'fused_total_ms': round(med['fused_all'], 4),
               'baseline_over_fused': round(base_med / med['fused_all'], 2),
               'sdf_baseline_over_fused': round(med['baseline_sdf'] / med['fused_sdf'], 2), 'agreement': agree}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, t, s, grad, phi_b, valid_b, gb
        torch.cuda.empty_cache()
    out_path = a.out or os.path.join('profiles', 'boundary_loss', 'boundary_bench.json')
    os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'trials': a.trials,
                   'note': 'ms per call (HIP events); fused_all = signed distance + forward + backward through '
                           'autograd; baseline = 2 edt_sq per class + torch glue, then autograd softmax * phi',
                   'rows': rows}, f, indent=1)


def lovasz_mode(a):
    """The Lovasz-softmax loss at the bench shapes, both ``per_image`` settings: forward + backward of the fused
    path (keys, 4-pass radix sort, coefficients, finalize, gradient) against the plain-torch form of
    ``LovaszSoftmaxLoss`` on the same device (``torch.sort``) and against ``cross_entropy``; the sort alone
    (``sort_segments`` on the same number of keys) is timed apart.  Every figure is the median of ``--trials``
    windows of ``--iters`` calls.  Bytes are the compulsory traffic of the fused path: per class and pixel
    ``passes * 20`` (key read by the histogram, key + payload read and written by the scatter) + 8 written by the key
    pass + 4 (payload) read by the count pass + 8 read by the coefficient pass + 4 coefficient written and 4 read
    again, plus logits and labels read by the key and gradient passes and the gradient written."""
    from medical_segmentation_pytorch_amd.core.loss import LovaszSoftmaxLoss
    from medical_segmentation_pytorch_amd.ops._ext import require
    from medical_segmentation_pytorch_amd.ops.losses import lovasz_softmax
    from medical_segmentation_pytorch_amd.ops.sort import sort_segments
    passes = require().sort_passes()
    dev = torch.device('cuda', 0)
    rows = []
    for n, c, h, w in a.shapes or [(320, 2, 352, 352), (32, 4, 352, 352)]:
        torch.manual_seed(0)
        x = torch.randn(n, c, h, w, device=dev, requires_grad=True)
        t = _blob_labels(n, c, h, w, dev)
        V = n * h * w
        nbytes = c * V * (passes * 20 + 28) + 2 * (c * V * 4 + V * 8) + c * V * 4

        def step(fn):
            x.grad = None
            fn().backward()

        for per_image in (False, True):
            plain = LovaszSoftmaxLoss(per_image=per_image)
            keys = torch.rand((n * c, h * w) if per_image else (c, V), device=dev)
            x.grad = None
            lf = lovasz_softmax(x, t, 255, per_image)
            lf.backward()
            gf = x.grad.clone()
            x.grad = None
            lp = plain.plain_term(x, t)
            lp.backward()
            agree = {'loss_fused': lf.item(), 'loss_plain': lp.item(),
                     'grad_rel_l2': ((gf - x.grad).norm() / x.grad.norm()).item()}
            del gf
            cases = {
                'fused': lambda: step(lambda: lovasz_softmax(x, t, 255, per_image)),
                'fused_fwd': lambda: lovasz_softmax(x.detach(), t, 255, per_image),
                'sort_only': lambda: sort_segments(keys),
                'torch_sort_only': lambda: torch.sort(keys, dim=1, descending=True, stable=True),
                'plain_torch': lambda: step(lambda: plain.plain_term(x, t)),
                'ce': lambda: step(lambda: cross_entropy(x, t)),
            }
            ms = {k: [] for k in cases}
            for _ in range(a.trials):                  # the variants alternate inside every trial
                for k, fn in cases.items():
                    ms[k].append(timeit(fn, a.iters, warmup=1))
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            row = {'shape': [n, c, h, w], 'per_image': per_image, 'ms_median': {k: round(v, 4) for k, v in med.items()},
                   'ms_trials': {k: [round(u, 4) for u in v] for k, v in ms.items()},
                   'plain_over_fused': round(med['plain_torch'] / med['fused'], 2),
                   'fused_over_ce': round(med['fused'] / med['ce'], 2),
                   'torch_sort_over_sort': round(med['torch_sort_only'] / med['sort_only'], 2),
                   'bytes': nbytes, 'tb_per_s': round(nbytes / med['fused'] / 1e9, 3), 'agreement': agree}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del keys
            torch.cuda.empty_cache()
        del x, t
        torch.cuda.empty_cache()
    out_path = a.out or os.path.join('profiles', 'lovasz_loss', 'lovasz_bench.json')
    os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'trials': a.trials,
                   'note': 'ms per call (HIP events); fused / plain_torch / ce = forward + backward through autograd',
                   'rows': rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['region', 'boundary', 'lovasz'], default='region')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--trials', type=int, default=5, help='boundary mode: timed windows per variant')
    ap.add_argument('--shapes', type=int, nargs=4, action='append', metavar=('N', 'C', 'H', 'W'))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode == 'boundary':
        return boundary_mode(a)
    if a.mode == 'lovasz':
        return lovasz_mode(a)
    a.out = a.out or os.path.join('profiles', 'region_loss', 'loss_bench.json')
    dev = torch.device('cuda', 0)
    rows = []
    for n, c, h, w in a.shapes or [(320, 2, 352, 352), (32, 4, 352, 352)]:
        torch.manual_seed(0)
        x = torch.randn(n, c, h, w, device=dev, requires_grad=True)
        t = torch.randint(0, c, (n, h, w), device=dev)
        t[:, :2] = 255
        logits, labels = x.numel() * 4, t.numel() * 8

        def step(fn):
            x.grad = None
            fn().backward()

        ce_ms = timeit(lambda: step(lambda: cross_entropy(x, t)), a.iters)
        ce_bytes = logits + labels + logits
        rows.append({'shape': [n, c, h, w], 'loss': 'ce', 'ms': round(ce_ms, 4), 'bytes': ce_bytes,
                     'bytes_with_backward_rescale': ce_bytes + 2 * logits,
                     'tb_per_s': round(ce_bytes / ce_ms / 1e9, 3), 'ratio_to_ce': 1.0})
        for lt, (pixel, region) in TYPES.items():
            ms = timeit(lambda: step(lambda: region_loss(x, t, None, 255, pixel, region)), a.iters)
            nbytes = 2 * (logits + labels) + logits
            rows.append({'shape': [n, c, h, w], 'loss': lt, 'ms': round(ms, 4), 'bytes': nbytes,
                         'tb_per_s': round(nbytes / ms / 1e9, 3), 'ratio_to_ce': round(ms / ce_ms, 3)})
        for r in rows[-8:]:
            print(json.dumps(r), flush=True)
        del x, t
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'iters': a.iters,
           'note': 'ms = forward + backward per call; ce includes its torch rescale of the gradient in backward',
           'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
