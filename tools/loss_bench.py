#!/usr/bin/env python3
"""Forward + backward time of the fused losses at the bench shapes: ``cross_entropy`` (one pass) against
every softmax-head region loss type (two passes), with HIP events.  Bytes moved are the compulsory
traffic of the loss kernels: CE reads logits + int64 labels and writes the gradient (its backward then
rescales that gradient with a torch op, one more read + write, listed apart); a region loss reads logits +
labels in each of its two passes and writes the gradient once.  From bytes alone a region loss should take
(2 (L + T) + L) / (2 L + T) of the CE kernel's time: 1.67x at C = 2.

    python tools/loss_bench.py [--iters 20] [--out profiles/region_loss/loss_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shapes', type=int, nargs=4, action='append', metavar=('N', 'C', 'H', 'W'))
    ap.add_argument('--out', default=os.path.join('profiles', 'region_loss', 'loss_bench.json'))
    a = ap.parse_args()
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
