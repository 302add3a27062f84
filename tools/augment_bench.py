#!/usr/bin/env python3
"""Cost of the rotation / shift / elastic warp, gamma / noise and blur kernels (``csrc/augment.hip``) at the bench
batch, against the existing geometry launch measured in the same run.

On the bench's data (``--batch`` 320 crops of ``--size`` 352 from its synthetic split, MyConfig draws of scale, crop,
jitter and flips) it times single launches of
  * ``aug_geometry`` (the existing gather),
  * ``aug_warp`` with every sample rotating and shifting, and with the B-spline deformation on top at 4 and 8 cells,
  * ``aug_pointwise`` with gamma, with noise and with both on every sample,
  * ``aug_blur`` at radius 3 (sigma 1.0) and radius 8 (sigma 2.5) on every sample,
and whole ``DeviceAugLoader.batch()`` calls (host draws and table packing included) with every new option off and
with every one on at p = 1, i.e. the most a batch can cost.  Kernel times are HIP events around ``--iters``
back-to-back launches, repeated ``--reps`` times after ``--warmup`` launches: median, min and max over the repeats.
``batch()`` is a host clock around ``--iters`` calls ending in a device synchronise.  Prints one JSON line; ``--out``
also writes it.  A run without a GPU fails.

    python tools/augment_bench.py --out profiles/augment/augment_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STEP_MS = 479.0   # the bench step at batch 320 (README), the yardstick of the batch() share


def time_gpu(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return {'median_ms': round(statistics.median(out), 4), 'min_ms': round(min(out), 4), 'max_ms': round(max(out), 4)}


def time_host(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return {'median_ms': round(statistics.median(out), 3), 'min_ms': round(min(out), 3), 'max_ms': round(max(out), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=320)
    ap.add_argument('--size', type=int, default=352)
    ap.add_argument('--train-images', type=int, default=128)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('augment_bench: no GPU')
    from bench import synthetic_split
    from medical_segmentation_pytorch_amd.datasets import device_loader as DL
    from medical_segmentation_pytorch_amd.ops import _ext
    from medical_segmentation_pytorch_amd.utils.transforms import SegAugment
    C = _ext.require()
    dev = torch.device('cuda', 0)
    B, S = a.batch, a.size
    imgs, msks = synthetic_split(a.train_images, S, a.seed)
    data = DL.DeviceDataset.from_arrays(imgs, msks, dev)
    base = dict(randscale=[-0.5, 1.0], brightness=0.5, contrast=0.5, saturation=0.5, h_flip=0.5, v_flip=0.5)
    every = dict(aug_rotate=30.0, aug_shift=0.1, aug_affine_p=1.0, aug_elastic_sigma=4.0, aug_elastic_cells=4,
                 aug_elastic_p=1.0, aug_gamma=[0.7, 1.5], aug_gamma_p=1.0, aug_blur_sigma=[0.5, 2.5], aug_blur_p=1.0,
                 aug_noise_std=[2.0, 10.0], aug_noise_p=1.0)
    off = DL.DeviceAugLoader(None, B, dev, seed=a.seed, data=data, aug=SegAugment(S, S, **base))
    on = DL.DeviceAugLoader(None, B, dev, seed=a.seed, data=data, aug=SegAugment(S, S, **base, **every))
    out_x = torch.empty(B, 3, S, S, device=dev)
    out_m = torch.empty(B, S, S, dtype=torch.int64, device=dev)

    # ---- single launches on one drawn batch
    idx = next(off.stream())
    prms = [off.aug.sample_params(*data.shapes[i]) for i in idx]
    ip, _ = DL.pack_params(prms, idx, C.aug_iparams())
    ip_d = torch.from_numpy(ip).to(dev)
    rng = np.random.default_rng(a.seed)

    def tables(**fields):
        recs = [dict(p, **{k: (v(i) if callable(v) else v) for k, v in fields.items()}) for i, p in enumerate(prms)]
        xi, xf, _ = DL.pack_params_ex(recs, (S, S), 'reflect', *C.aug_xparams())
        return torch.from_numpy(xi).to(dev), torch.from_numpy(xf).to(dev)

    def affine(_):
        return (float(rng.uniform(-30, 30)), float(rng.uniform(-0.1, 0.1)) * S, float(rng.uniform(-0.1, 0.1)) * S)

    def lattice(n):
        return lambda _: {'n': n, 'dy': rng.normal(0, 4.0, (n + 3, n + 3)).astype(np.float32),
                          'dx': rng.normal(0, 4.0, (n + 3, n + 3)).astype(np.float32)}

    work, work2 = on.work, on.work2
    rows = {}

    def gather(t=None):
        C.aug_gather(data.images, data.masks, data.meta, ip_d, t[0] if t else None, t[1] if t else None, work, out_m,
                     S, S)
    rows['aug_geometry'] = time_gpu(gather, a.warmup, a.iters, a.reps)
    for name, t in (('aug_warp affine', tables(affine=affine)),
                    ('aug_warp affine + elastic 4', tables(affine=affine, elastic=lattice(4))),
                    ('aug_warp affine + elastic 8', tables(affine=affine, elastic=lattice(8)))):
        rows[name] = time_gpu(lambda t=t: gather(t), a.warmup, a.iters, a.reps)
    gather()
    # in place: gamma stays near 1 so that repeated launches keep realistic values in the buffer
    for name, t, ops in (('aug_pointwise gamma', tables(gamma=0.999), DL.AUG_GAMMA),
                         ('aug_pointwise noise', tables(noise=lambda i: (5.0, 1000003 * i + 17)), DL.AUG_NOISE),
                         ('aug_pointwise gamma + noise',
                          tables(gamma=1.001, noise=lambda i: (5.0, 1000003 * i + 29)), DL.AUG_GAMMA | DL.AUG_NOISE)):
        rows[name] = time_gpu(lambda t=t, ops=ops: C.aug_pointwise(work, t[0], t[1], S * S, ops), a.warmup, a.iters,
                              a.reps)
    gather()
    for name, t in (('aug_blur r3', tables(blur=1.0)), ('aug_blur r8', tables(blur=2.5))):
        rows[name] = time_gpu(lambda t=t: C.aug_blur(work, work2, t[0], t[1], S, S), a.warmup, a.iters, a.reps)
    geo = rows['aug_geometry']['median_ms']
    for r in rows.values():
        r['vs_geometry'] = round(r['median_ms'] / geo, 2)

    # ---- whole batches, host side included
    batches = {}
    for name, loader in (('batch() every new option off', off), ('batch() every new option on, p = 1', on)):
        order = loader.stream()
        batches[name] = time_host(lambda: loader.batch(next(order), out=(out_x, out_m)), a.warmup, a.iters, a.reps)
        batches[name]['share_of_step'] = round(batches[name]['median_ms'] / STEP_MS, 4)
    assert off.ex_batches == 0 and on.ex_batches > 0
    out = {'tool': 'augment_bench', 'device': torch.cuda.get_device_name(0), 'batch': B, 'size': S, 'iters': a.iters,
           'reps': a.reps, 'step_ms': STEP_MS, 'kernels': rows, 'batches': batches}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
