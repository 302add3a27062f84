#!/usr/bin/env python3
"""Cost of the sliding-window glue (gather, blend, finalise) on one large image, against the network's forward on
the same windows.

For an image ``[N, Cin, H, W]`` (default ``1 3 2048 2048``), window 352, overlap 0.5, flips 'hv', C = 2, chunks of
``--batch`` windows:
  * ``window_gather`` of every chunk, ``window_blend_accumulate`` of every chunk and ``window_blend_finalize``
    (``csrc/tiled.hip``) on synthetic window logits, with the achieved bytes per second against the floor of each:
    gather -- windows written once and read once; blend -- window logits read once, the output rows a chunk touches
    read and written once per chunk; finalise -- the output read and written once,
  * the plain-torch specification of ``ops/tiled.py`` (a loop of slice-adds per window and view) on the same GPU,
  * the ``FusedModel`` eval forward of DUCKNet-17 on the same chunks of windows, timed in the same run.
Times are HIP events around ``--iters`` back-to-back passes after ``--warmup`` passes.  Prints one JSON line; ``--out``
also writes it.  A run without a GPU fails.

    python tools/tiled_bench.py --out profiles/tiled_inference/tiled_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def time_gpu(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--image', type=int, nargs=4, default=[1, 3, 2048, 2048], metavar=('N', 'CIN', 'H', 'W'))
    ap.add_argument('--window', type=int, default=352)
    ap.add_argument('--overlap', type=float, default=0.5)
    ap.add_argument('--flips', default='hv', choices=['', 'h', 'v', 'hv'])
    ap.add_argument('--blend', default='gaussian', choices=['gaussian', 'constant'])
    ap.add_argument('--average', default='logits', choices=['logits', 'probs'])
    ap.add_argument('--classes', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--torch-iters', type=int, default=2, help='timed passes of the plain-torch specification')
    ap.add_argument('--no-forward', action='store_true', help='skip the DUCKNet-17 forward')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tiled_bench: no GPU')
    from medical_segmentation_pytorch_amd.ops import _ext
    from medical_segmentation_pytorch_amd.ops import tiled as T
    _ext.require()
    dev = torch.device('cuda', 0)
    n, cin, h, w = a.image
    c, b = a.classes, a.batch
    plan = T.tile_plan(h, w, a.window, a.overlap, a.blend, 0.125, a.flips)
    total = plan.windows(n)
    chunks = list(range(0, total, b))
    torch.manual_seed(0)
    images = torch.randn(n, cin, h, w, device=dev)
    logits = 3 * torch.randn(len(chunks) * b, c, plan.wh, plan.ww, device=dev)   # a short last chunk is padded

    def gather():
        for m0 in chunks:
            T.gather_windows(images, plan, m0, b)
    acc = T.new_accumulator(plan, n, c, logits, True)

    def accumulate():
        for m0 in chunks:
            T.accumulate_windows(acc, logits[m0:m0 + b], plan, m0, a.average, True)

    def finalize():
        T.finalize_windows(acc, plan, a.average, True)

    def spec():
        s = T.new_accumulator(plan, n, c, logits, False)
        for m0 in chunks:
            T.accumulate_windows(s, logits[m0:m0 + b], plan, m0, a.average, False)
        return T.finalize_windows(s, plan, a.average, False)

    def spec_gather():
        for m0 in chunks:
            T.gather_windows(images, plan, m0, b, native=False)

    px = plan.wh * plan.ww
    touched = sum((lambda r: (r[1] - r[0]) * (r[3] - r[2]))(plan.rows_of(m0, m0 + b, n)) for m0 in chunks) * w * c
    floor = {'gather': 2 * total * cin * px * 4, 'accumulate': (total * c * px + 2 * touched) * 4,
             'finalize': 2 * n * c * h * w * 4}
    row = {'image': [n, cin, h, w], 'window': [plan.wh, plan.ww], 'overlap': a.overlap, 'flips': a.flips,
           'blend': a.blend, 'average': a.average, 'classes': c, 'batch': b, 'windows': total, 'chunks': len(chunks),
           'max_terms_per_pixel': plan.max_terms}
    for name, fn in (('gather', gather), ('accumulate', accumulate), ('finalize', finalize)):
        ms = time_gpu(fn, a.warmup, a.iters)
        row[f'{name}_ms'] = round(ms, 4)
        row[f'{name}_floor_bytes'] = floor[name]
        row[f'{name}_gbps'] = round(floor[name] / ms / 1e6, 1)
    row['blend_ms'] = round(row['accumulate_ms'] + row['finalize_ms'], 4)
    row['torch_blend_same_gpu_ms'] = round(time_gpu(spec, 1, a.torch_iters), 3)
    row['torch_gather_same_gpu_ms'] = round(time_gpu(spec_gather, 1, a.torch_iters), 3)
    row['torch_over_hip_blend'] = round(row['torch_blend_same_gpu_ms'] / row['blend_ms'], 2)
    # both paths on the same logits: the difference is rounding only
    acc.zero_()
    accumulate()
    finalize()
    row['max_abs_diff_vs_torch'] = float((acc - spec()).abs().max())
    if not a.no_forward:
        from medical_segmentation_pytorch_amd.models.ducknet import DuckNet
        from medical_segmentation_pytorch_amd.utils import FusedModel
        model = FusedModel(DuckNet(num_class=c, n_channel=cin, base_channel=17).to(dev)).eval()
        x = torch.randn(b, cin, plan.wh, plan.ww, device=dev)
        with torch.no_grad():
            per_chunk = time_gpu(lambda: model(x), a.warmup, a.iters)
        row['forward_chunk_ms'] = round(per_chunk, 4)
        row['forward_ms'] = round(per_chunk * len(chunks), 3)
        glue = row['gather_ms'] + row['blend_ms']
        row['glue_ms'] = round(glue, 4)
        row['glue_share_of_total'] = round(glue / (glue + row['forward_ms']), 5)
    out = {'tool': 'tiled_bench', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rows': [row]}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
