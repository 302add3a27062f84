#!/usr/bin/env python3
"""Cost of the lesion-wise metrics (recall + precision + F1) and of the mask clean-up per batch on one GPU, against
forwarding the batch.

For each shape ``[N, C, H, W]`` (default: the validation batch ``16 2 352 352`` and ``16 4 352 352``), on the masks of
``tools/surface_bench.py`` (two offset ellipses per class with 1 % salt noise):
  * one ``update`` of all three lesion metrics on the HIP kernels (``csrc/components.hip``; the three share one pass),
  * the plain-torch path of ``ops/components.py`` on the same GPU,
  * ``postprocess`` of the argmax with fill_holes + min_area + keep_largest on the kernels,
  * the ``FusedModel`` eval forward of DUCKNet-17 on a batch of the same N, H, W, timed in the same run.
Times are HIP events around ``--iters`` back-to-back calls after ``--warmup`` calls.  Prints one JSON line; ``--out``
also writes it.  A run without a GPU fails.

    python tools/components_bench.py --out profiles/components/components_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/components_bench.py --device-only
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from surface_bench import make_batch, time_gpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, nargs='+', default=[16, 2, 352, 352, 16, 4, 352, 352])
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--torch-iters', type=int, default=2, help='timed calls of the plain-torch path (slow)')
    ap.add_argument('--min-area', type=int, default=20)
    ap.add_argument('--device-only', action='store_true', help='only the HIP paths (profiling runs)')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('components_bench: no GPU')
    from medical_segmentation_pytorch_amd.models.ducknet import DuckNet
    from medical_segmentation_pytorch_amd.ops import _ext
    from medical_segmentation_pytorch_amd.ops import components as CC
    from medical_segmentation_pytorch_amd.utils import FusedModel
    from medical_segmentation_pytorch_amd.utils import metrics as M
    _ext.require()
    dev = torch.device('cuda', 0)
    rows = []
    for j in range(0, len(a.shapes), 4):
        n, c, h, w = a.shapes[j:j + 4]
        logits, tgt = make_batch(n, c, h, w)
        lg, tg = logits.to(dev), tgt.to(dev)
        acc = M.LesionAccumulator(c, 255).to(dev)
        ms = [cls(num_classes=c, accumulator=acc) for cls in M.LESION_METRICS.values()]

        def update():
            for m in ms:                 # the first metric's second sight of the tensors starts a new batch
                m.update(lg, tg)
        row = {'shape': [n, c, h, w], 'update_ms': round(time_gpu(update, a.warmup, a.iters), 4)}
        acc.reset()
        update()
        row['values'] = {k: float(m.compute()) for k, m in zip(M.LESION_METRICS, ms)}
        row['counts'] = acc.counts.tolist()
        row['errors'] = int(acc.err)
        labels = lg.argmax(1).to(torch.uint8)
        rules = dict(fill_holes=True, min_area=a.min_area, keep_largest=True)
        row['postprocess_ms'] = round(time_gpu(lambda: CC.postprocess(labels, c, **rules), a.warmup, a.iters), 4)
        row['postprocess_changed_pixels_per_image'] = round(
            float((CC.postprocess(labels, c, **rules) != labels).sum()) / n, 1)
        if not a.device_only:
            st = CC.new_state(c, dev)
            row['torch_same_gpu_ms'] = round(time_gpu(
                lambda: CC.lesion_stats(lg, tg, c, 255, state=st, native=False), 1, a.torch_iters), 2)
            row['postprocess_torch_same_gpu_ms'] = round(time_gpu(
                lambda: CC.postprocess(labels, c, native=False, **rules), 1, a.torch_iters), 2)
            torch.manual_seed(0)
            model = FusedModel(DuckNet(num_class=c, n_channel=3, base_channel=17).to(dev)).eval()
            x = torch.randn(n, 3, h, w, device=dev)
            with torch.no_grad():
                row['forward_ms'] = round(time_gpu(lambda: model(x), a.warmup, a.iters), 4)
            row['update_over_forward'] = round(row['update_ms'] / row['forward_ms'], 4)
            del model
        rows.append(row)
    out = {'tool': 'components_bench', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rows': rows}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
