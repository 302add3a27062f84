#!/usr/bin/env python3
"""Cost of the calibration kernels per batch on one GPU, against the plain-torch path on the same device.

For each shape ``[N, C, H, W]`` (default: the validation batch ``16 2 352 352`` and the training batch
``320 2 352 352``), on the masks of ``tools/surface_bench.py`` with logits of margin 4:
  * ``calibration_stats`` at 15 bins (``calib_stats`` + its finalize, ``csrc/calibration.hip``),
  * ``nll_grid`` at the 33 inverse temperatures of a fit round (``calib_nll_grid`` + its finalize),
  * ``uncertainty_map`` in both modes,
  * the plain-torch form of each (``native=False``) on the same GPU, and the relative difference of the results,
  * the bytes each kernel has to read and write, and the rate that time makes of them.
Times are HIP events around ``--iters`` back-to-back calls after ``--warmup`` calls.  Prints one JSON line; ``--out``
also writes it.  A run without a GPU fails.

    python tools/calibration_bench.py --out profiles/calibration/calibration_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/calibration_bench.py --device-only
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
    ap.add_argument('--shapes', type=int, nargs='+', default=[16, 2, 352, 352, 320, 2, 352, 352])
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--torch-iters', type=int, default=3, help='timed calls of the plain-torch path')
    ap.add_argument('--bins', type=int, default=15)
    ap.add_argument('--device-only', action='store_true', help='only the HIP paths (profiling runs)')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('calibration_bench: no GPU')
    from medical_segmentation_pytorch_amd.ops import _ext
    from medical_segmentation_pytorch_amd.ops import calibration as K
    _ext.require()
    dev = torch.device('cuda', 0)
    betas = K._betas(K.first_exponents()).to(dev)
    rows = []
    for j in range(0, len(a.shapes), 4):
        n, c, h, w = a.shapes[j:j + 4]
        small, tgt_small = make_batch(min(n, 16), c, h, w)
        reps = -(-n // small.shape[0])
        lg = small.to(dev).repeat(reps, 1, 1, 1)[:n].contiguous()
        tg = tgt_small.to(dev).repeat(reps, 1, 1)[:n].contiguous()
        px = n * h * w
        row = {'shape': [n, c, h, w]}
        st = K.new_state(a.bins, dev)
        row['stats_ms'] = round(time_gpu(lambda: K.calibration_stats(lg, tg, st, 1.0, 255, a.bins), a.warmup, a.iters), 4)
        row['stats_read_GBps'] = round(px * (4 * c + 8) / row['stats_ms'] / 1e6, 1)
        sums = torch.zeros(betas.numel(), dtype=torch.float64, device=dev)
        row['nll_grid33_ms'] = round(time_gpu(lambda: K.nll_grid(lg, tg, betas, 255, sums), a.warmup, a.iters), 4)
        row['nll_grid33_read_GBps'] = round(px * (4 * c + 8) / row['nll_grid33_ms'] / 1e6, 1)
        for mode in K.MODES:
            row[f'uncertainty_{mode}_ms'] = round(time_gpu(lambda: K.uncertainty_map(lg, 1.0, mode), a.warmup, a.iters), 4)
            row[f'uncertainty_{mode}_GBps'] = round(px * (4 * c + 1) / row[f'uncertainty_{mode}_ms'] / 1e6, 1)
        one = K.calibration_stats(lg, tg, None, 1.0, 255, a.bins)
        row['values'] = dict(zip(('ece', 'mce', 'nll', 'brier'),
                                 (float(v) for v in K.metrics_from_state(one['ints'], one['sums']))))
        if not a.device_only:
            ref = K.new_state(a.bins, dev)
            row['stats_torch_same_gpu_ms'] = round(time_gpu(
                lambda: K.calibration_stats(lg, tg, ref, 1.0, 255, a.bins, native=False), 1, a.torch_iters), 3)
            rs = torch.zeros_like(sums)
            row['nll_grid33_torch_same_gpu_ms'] = round(time_gpu(
                lambda: K.nll_grid(lg, tg, betas, 255, rs, native=False), 1, a.torch_iters), 3)
            row['uncertainty_entropy_torch_same_gpu_ms'] = round(time_gpu(
                lambda: K.uncertainty_map(lg, 1.0, 'entropy', native=False), 1, a.torch_iters), 3)
            want = K.calibration_stats(lg, tg, None, 1.0, 255, a.bins, native=False)
            row['ints_equal_torch'] = bool(torch.equal(one['ints'], want['ints']))
            row['sums_max_rel_diff_torch'] = float(((one['sums'] - want['sums']).abs()
                                                    / want['sums'].abs().clamp_min(1e-300)).max())
            g1, g2 = K.nll_grid(lg, tg, betas, 255), K.nll_grid(lg, tg, betas, 255, native=False)
            row['nll_grid_max_rel_diff_torch'] = float(((g1 - g2).abs() / g2.abs().clamp_min(1e-300)).max())
        rows.append(row)
        del lg, tg
    out = {'tool': 'calibration_bench', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'bins': a.bins,
           'rows': rows}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
