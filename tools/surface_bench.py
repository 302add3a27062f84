#!/usr/bin/env python3
"""Cost of the boundary metrics (hd95 + assd + nsd) per validation batch on one GPU, against forwarding it.

For each shape ``[N, C, H, W]`` (default: the validation batch ``16 2 352 352`` and ``16 4 352 352``), on masks of
two offset ellipses per class with 1 % salt noise:
  * one ``update`` of all three metrics on the HIP kernels (``csrc/surface.hip``; the three share one pass),
  * the plain-torch path of ``ops/surface.py`` on the same GPU,
  * where scipy imports, the scipy formulation (binary_erosion + distance_transform_edt) on the CPU,
  * the ``FusedModel`` eval forward of DUCKNet-17 on a batch of the same N, H, W, timed in the same run.
Times are HIP events around ``--iters`` back-to-back calls after ``--warmup`` calls (host clock for scipy).  Prints
one JSON line; ``--out`` also writes it.  A run without a GPU fails.

    python tools/surface_bench.py --out profiles/surface_metrics/surface_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/surface_bench.py --device-only
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def make_batch(n, c, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    pred = torch.zeros(n, h, w, dtype=torch.long)
    tgt = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        for k in range(1, c):
            cy, cx = h * (0.3 + 0.4 * float(torch.rand((), generator=g))), w * (k - 0.5) / (c - 1)
            ry, rx = h * (0.12 + 0.15 * float(torch.rand((), generator=g))), w * 0.35 / (c - 1)
            dy, dx = (torch.rand(2, generator=g) * 8 - 4).tolist()
            tgt[i][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1] = k
            pred[i][((ys - cy - dy) / (ry * 1.05)) ** 2 + ((xs - cx - dx) / rx) ** 2 <= 1] = k
        salt = torch.rand(h, w, generator=g) < 0.01
        pred[i][salt] = torch.randint(0, c, (int(salt.sum()),), generator=g)
    logits = 4.0 * torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).float() \
        + torch.rand(n, c, h, w, generator=g) - 0.5
    return logits.contiguous(), tgt


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


def scipy_stats(pred, tgt, c, tol):
    """The same per-image values with scipy on the CPU (None without scipy)."""
    try:
        import numpy as np
        from scipy import ndimage as ndi
    except ImportError:
        return None
    cross = ndi.generate_binary_structure(2, 1)
    out = []
    for i in range(pred.shape[0]):
        for k in range(1, c):
            p, t = pred[i] == k, tgt[i] == k
            bp, bt = p ^ ndi.binary_erosion(p, cross), t ^ ndi.binary_erosion(t, cross)
            if not bp.any() or not bt.any():
                continue
            dpg = ndi.distance_transform_edt(~bt)[bp]
            dgp = ndi.distance_transform_edt(~bp)[bt]
            out.append((max(np.percentile(dpg, 95), np.percentile(dgp, 95)),
                        (dpg.sum() + dgp.sum()) / (dpg.size + dgp.size),
                        ((dpg <= tol).sum() + (dgp <= tol).sum()) / (dpg.size + dgp.size)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, nargs='+', default=[16, 2, 352, 352, 16, 4, 352, 352])
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--torch-iters', type=int, default=2, help='timed calls of the plain-torch path (slow)')
    ap.add_argument('--device-only', action='store_true', help='only the HIP path (profiling runs)')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('surface_bench: no GPU')
    from medical_segmentation_pytorch_amd.models.ducknet import DuckNet
    from medical_segmentation_pytorch_amd.ops import _ext
    from medical_segmentation_pytorch_amd.ops import surface as S
    from medical_segmentation_pytorch_amd.utils import FusedModel
    from medical_segmentation_pytorch_amd.utils import metrics as M
    _ext.require()
    dev = torch.device('cuda', 0)
    rows = []
    for j in range(0, len(a.shapes), 4):
        n, c, h, w = a.shapes[j:j + 4]
        logits, tgt = make_batch(n, c, h, w)
        lg, tg = logits.to(dev), tgt.to(dev)
        acc = M.SurfaceAccumulator(c, 255, 2.0).to(dev)
        ms = [cls(num_classes=c, accumulator=acc) for cls in M.SURFACE_METRICS.values()]

        def update():
            for m in ms:                 # the first metric's second sight of the tensors starts a new batch
                m.update(lg, tg)
        row = {'shape': [n, c, h, w], 'update_ms': round(time_gpu(update, a.warmup, a.iters), 4)}
        acc.reset()
        update()
        row['values'] = {k: float(m.compute()) for k, m in zip(M.SURFACE_METRICS, ms)}
        st = S.new_state(c, dev)
        dbg = S.surface_stats(lg, tg, c, 255, 2.0, st, debug=True)
        row['boundary_pixels_per_image'] = round(float(dbg['counts'].sum()) / n, 1)
        if not a.device_only:
            st = S.new_state(c, dev)
            row['torch_same_gpu_ms'] = round(time_gpu(
                lambda: S.surface_stats(lg, tg, c, 255, 2.0, st, native=False), 1, a.torch_iters), 2)
            pred_np, tgt_np = logits.argmax(1).numpy(), tgt.numpy()
            t0 = time.perf_counter()
            ref = scipy_stats(pred_np, tgt_np, c, 2.0)
            row['scipy_cpu_ms'] = None if ref is None else round((time.perf_counter() - t0) * 1e3, 2)
            torch.manual_seed(0)
            model = FusedModel(DuckNet(num_class=c, n_channel=3, base_channel=17).to(dev)).eval()
            x = torch.randn(n, 3, h, w, device=dev)
            with torch.no_grad():
                row['forward_ms'] = round(time_gpu(lambda: model(x), a.warmup, a.iters), 4)
            row['update_over_forward'] = round(row['update_ms'] / row['forward_ms'], 4)
            del model
        rows.append(row)
    out = {'tool': 'surface_bench', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rows': rows}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
