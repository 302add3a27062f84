#!/usr/bin/env python3
"""Per-layer microbenchmark of the implicit-GEMM conv kernels (fwd / dgrad / wgrad) on the
DUCKNet-17 layer shapes at the headline config (batch 16, 352x352), vs MIOpen (torch bf16
channels_last).  Prints time, achieved TFLOP/s (useful FLOPs, unpadded) and a JSON summary.

    python tools/conv_bench.py [--batch 16] [--size 352] [--iters 20] [--miopen]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from medical_segmentation_pytorch_amd.ops.conv import Branch, ConvPlan, conv  # noqa: E402


def layers(b=17):
    L = []
    for lvl, c in enumerate([b, 2 * b, 4 * b, 8 * b, 16 * b]):
        L.append((f'L{lvl + 1} 3x3 {c}->{c}', lvl, c, c, (3, 3), 1, (1, 1), (1, 1), 1))
        L.append((f'L{lvl + 1} 3x3d3 {c}->{c}', lvl, c, c, (3, 3), 1, (3, 3), (3, 3), 1))
        L.append((f'L{lvl + 1} 1x7 {c}->{c}', lvl, c, c, (1, 7), 1, (0, 3), (1, 1), 1))
        L.append((f'L{lvl + 1} fused8 {c}->8x{c}', lvl, c, c, (3, 3), 1, (1, 1), (1, 1), 8))
        # DUCK first-conv decompositions: the 5 3x3 convs (in 1, 2 or 3 launches) + the 3 1x1 shortcuts
        for gsz in (5, 3, 2):
            L.append((f'L{lvl + 1} fused{gsz} {c}->{gsz}x{c}', lvl, c, c, (3, 3), 1, (1, 1), (1, 1), gsz))
        L.append((f'L{lvl + 1} fused3-1x1 {c}->3x{c}', lvl, c, c, (1, 1), 1, (0, 0), (1, 1), 3))
        L.append((f'L{lvl + 1} 3x3s2 {c}->{2 * c}', lvl, c, 2 * c, (3, 3), 2, (1, 1), (1, 1), 1))
    # the first DUCK reads the 3-channel image (in_bn(x)): its first convs at 3 -> b
    L.append((f'L1in fused8 3->8x{b}', 0, 3, b, (3, 3), 1, (1, 1), (1, 1), 8))
    L.append((f'L1in fused5 3->5x{b}', 0, 3, b, (3, 3), 1, (1, 1), (1, 1), 5))
    L.append((f'L1in fused3-1x1 3->3x{b}', 0, 3, b, (1, 1), 1, (0, 0), (1, 1), 3))
    L.append(('L6 3x3 544->544', 5, 32 * b, 32 * b, (3, 3), 1, (1, 1), (1, 1), 1))
    L.append(('L6 fused2 544->2x544', 5, 32 * b, 32 * b, (3, 3), 1, (1, 1), (1, 1), 2))
    return L


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def stamp_summary(C, buf, fn):
    """One stamped call (GK_STAMP build): per block the clock readings entry / first MFMA / last MFMA / exit
    (100-MHz ticks).  Returns the median fill, main-loop and drain time in us, the fill + drain share of the
    block lifetime and the number of blocks stamped."""
    buf.zero_()
    C.conv_gemm_stamp_buffer(buf)
    fn()
    torch.cuda.synchronize()
    C.conv_gemm_stamp_buffer(None)
    t = buf[buf[:, 3] > 0].double() * 0.01
    if t.shape[0] == 0:
        return None
    fill, loop, drain = t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 3] - t[:, 2]
    life = (t[:, 3] - t[:, 0]).sum().item()
    return {'fill_us': round(fill.median().item(), 2), 'loop_us': round(loop.median().item(), 2),
            'drain_us': round(drain.median().item(), 2), 'blocks': int(t.shape[0]),
            'fill_drain_share': round((fill.sum().item() + drain.sum().item()) / max(life, 1e-9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=352)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--miopen', action='store_true')
    ap.add_argument('--halo', type=int, default=1, help='1: halo-tiled stride-1 kernel where eligible, 0: gather only')
    ap.add_argument('--split', type=int, default=1, help='halo split-bank tile image: 0 never, 1 occupancy-preserving '
                    '(default), 2 wherever it fits (csrc/conv.hip halo_phys)')
    ap.add_argument('--gemm-cfg', type=int, default=-1, help='force one LDS-DMA GEMM tile configuration (A/B)')
    ap.add_argument('--gemm-stamps', action='store_true',
                    help='in-kernel clock stamps per block (needs a -DGK_STAMP side build loaded through MSP_C_SO): '
                    'median fill / main loop / drain per layer: forward, data-gradient, and the data-gradient '
                    'through the accumulate and the BN-backward epilogues')
    ap.add_argument('--wgrad-only', action='store_true', help='time the weight gradients only (knock-out / ring sweeps)')
    ap.add_argument('--wgrad-ring', default='', help="weight-gradient GEMM ring variants for this run, 'geometry:variant,...' "
                    "(configuration indices of csrc/conv_wgrad_gemm.hip kWgCfgs; 'base': every geometry on its 2 x 64 ring)")
    ap.add_argument('--only', default='', help='substring filter on layer names')
    ap.add_argument('--levels', default='', help='comma list of levels to run (e.g. 3,4,5,6)')
    ap.add_argument('--prologue', action='store_true',
                    help='input is a deferred BN(+ReLU) output: fwd / wgrad apply the BN prologue while staging')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    from medical_segmentation_pytorch_amd.ops import _ext
    C = _ext.require()
    C.conv_set_halo(bool(a.halo))
    C.conv_set_halo_split(a.split)
    C.conv_gemm_force_cfg(a.gemm_cfg)
    if a.wgrad_ring == 'base':
        for b in range(C.conv_wgrad_gemm_num_cfgs()):
            if C.conv_wgrad_gemm_cfg_info(b)[6] == b:
                C.conv_wgrad_gemm_set_ring(b, b)
    elif a.wgrad_ring:
        for pair in a.wgrad_ring.split(','):
            b, v = (int(t) for t in pair.split(':'))
            C.conv_wgrad_gemm_set_ring(b, v)
    sbuf = None
    if a.gemm_stamps:
        if not C.conv_gemm_stamp_buffer(None):
            sys.exit('--gemm-stamps: this extension was built without -DGK_STAMP')
        sbuf = torch.zeros(1 << 18, 4, device=dev, dtype=torch.int64)
    res = []
    tot = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}
    for name, lvl, ci, co, k, s, p, d, groups in layers():
        if a.only and a.only not in name:
            continue
        if a.levels and str(lvl + 1) not in a.levels.split(','):
            continue
        hw = a.size >> lvl
        n = a.batch
        convs = [nn.Conv2d(ci, co, k, s, p, d, bias=False).to(dev) for _ in range(groups)]
        br = [Branch(c.weight, g, 0, k[0] * k[1]) for g, c in enumerate(convs)]
        plan = ConvPlan(k[0], k[1], ci, co, br, stride=s, padding=p, dilation=d, Go=groups)
        x = torch.randn(n, hw, hw, plan.Cgi, device=dev).to(torch.bfloat16)
        x[..., ci:] = 0
        oh, ow = plan.out_hw(hw, hw)
        dims = plan.fwd_dims(n, hw, hw, oh, ow)
        dy, dx = [t[0] for t in plan.taps_fwd], [t[1] for t in plan.taps_fwd]
        wp = plan.pack_fwd(dev)
        ys = [torch.empty(n, oh, ow, plan.Cgo, device=dev, dtype=torch.bfloat16) for _ in range(groups)]
        nblk = C.conv_stat_blocks(dims, dy, dx)
        part = torch.empty(nblk, 2, plan.rows, device=dev)
        xc, xr = [], 0
        if a.prologue:   # BN stats rows (scale, shift, mean, invstd) of the input channels
            st = torch.zeros(4, plan.Cgi, device=dev)
            st[0, :ci] = torch.rand(ci, device=dev) + 0.5
            st[1, :ci] = torch.randn(ci, device=dev) * 0.1
            xc, xr = [st], 1
        if a.wgrad_only:
            gys = [torch.randn_like(y, dtype=torch.float32).to(torch.bfloat16) for y in ys]
            dwp = torch.empty(C.conv_wgrad_replicas(dims, dy, dx, False, False, bool(xc)) * plan.rows * plan.T * plan.Cip,
                              device=dev)
            t_w = timeit(lambda: C.conv_wgrad(gys, [x], dwp, dims, dy, dx, False, xc, xr), a.iters)
            cfg = C.conv_wgrad_gemm_plan_cfg(dims, dy, dx, bool(xc)) if hasattr(C, 'conv_wgrad_gemm_plan_cfg') else -1
            gemm = bool(C.conv_uses_wgrad_gemm(dims, dy, dx, False)) and not C.conv_wgrad_uses_halo(dims, dy, dx, False)
            flops = 2.0 * n * oh * ow * co * ci * k[0] * k[1] * groups
            res.append({'layer': name, 'wgrad_ms': round(t_w, 4), 'wgrad_tflops': round(flops / t_w / 1e9, 1),
                        'wgrad_cfg': cfg if gemm else None})
            tot['wgrad'] += t_w
            print(f"{name:28s} wgrad {t_w:7.3f} ({flops / t_w / 1e9:6.1f})  cfg {cfg if gemm else '-'}", flush=True)
            continue
        t_f = timeit(lambda: C.conv_fwd([x], wp, ys, None, part, dims, dy, dx, False, xc, xr), a.iters)
        wd, Kp_d = plan.pack_dgrad(dev)
        gys = [torch.randn_like(y, dtype=torch.float32).to(torch.bfloat16) for y in ys]
        dxs = [torch.empty_like(x)]
        dims_d = [n, oh, ow, plan.Go, plan.Cgo, hw, hw, 1, plan.Cgi, ci, plan.T, Kp_d, s]
        bdy, bdx = [t[0] for t in plan.taps_bwd], [t[1] for t in plan.taps_bwd]
        f_d = lambda: C.conv_fwd(gys, wd, dxs, None, None, dims_d, bdy, bdx, s > 1)   # noqa: E731
        t_d = timeit(f_d, a.iters)
        # the same data-gradient through the two other GEMM epilogues: accumulating into dL/dx, and (stride 1)
        # with the BN-backward partials of a BN(+ReLU) whose output this conv read (random y, coefficients as in
        # tests/test_gpu_conv_gemm.py)
        f_a = lambda: C.conv_fwd(gys, wd, dxs, None, None, dims_d, bdy, bdx, s > 1, accumulate=True)   # noqa: E731
        dxs[0].zero_()
        t_a = timeit(f_a, a.iters)
        f_b, t_b = None, None
        if s == 1:
            bn_y = torch.randn(n, hw, hw, plan.Cgi, device=dev).to(torch.bfloat16)
            coef = torch.zeros(3, plan.Cgi, device=dev)
            coef[0, :ci] = torch.rand(ci, device=dev) + 0.5
            coef[1, :ci] = torch.randn(ci, device=dev) * 0.2
            coef[2, :ci] = torch.randn(ci, device=dev) * 0.1
            part_d = torch.empty(C.conv_stat_blocks(dims_d, bdy, bdx, False, False, True), 2, plan.Cgi, device=dev)
            f_b = lambda: C.conv_fwd_bn(gys, wd, dxs, part_d, dims_d, bdy, bdx, bn_y, coef, True)   # noqa: E731
            t_b = timeit(f_b, a.iters)
        dwp = torch.empty(C.conv_wgrad_replicas(dims, dy, dx, False, False, bool(xc)) * plan.rows * plan.T * plan.Cip, device=dev)
        t_w = timeit(lambda: C.conv_wgrad(gys, [x], dwp, dims, dy, dx, False, xc, xr), a.iters)
        flops = 2.0 * n * oh * ow * co * ci * k[0] * k[1] * groups
        row = {'layer': name, 'fwd_ms': round(t_f, 4), 'dgrad_ms': round(t_d, 4), 'wgrad_ms': round(t_w, 4),
               'dgrad_acc_ms': round(t_a, 4), 'dgrad_bn_ms': round(t_b, 4) if t_b is not None else None,
               'fwd_tflops': round(flops / t_f / 1e9, 1), 'dgrad_tflops': round(flops / t_d / 1e9, 1),
               'wgrad_tflops': round(flops / t_w / 1e9, 1)}
        if a.miopen:
            xm = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
            wm = torch.randn(co * groups, ci, *k, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
            row['miopen_fwd_ms'] = round(timeit(lambda: F.conv2d(xm, wm, None, s, p, d), a.iters), 4)
        if sbuf is not None:
            row['stamps_fwd'] = stamp_summary(
                C, sbuf, lambda: C.conv_fwd([x], wp, ys, None, part, dims, dy, dx, False, xc, xr))
            row['stamps_dgrad'] = stamp_summary(C, sbuf, f_d)
            row['stamps_dgrad_acc'] = stamp_summary(C, sbuf, f_a)
            row['stamps_dgrad_bn'] = stamp_summary(C, sbuf, f_b) if f_b is not None else None
            for k in ('stamps_fwd', 'stamps_dgrad', 'stamps_dgrad_acc', 'stamps_dgrad_bn'):
                if row[k]:
                    print(f"    {k[7:]:9s} fill {row[k]['fill_us']:6.2f} us  loop {row[k]['loop_us']:7.2f}  drain "
                          f"{row[k]['drain_us']:6.2f}  fill+drain share {100 * row[k]['fill_drain_share']:5.1f} %  "
                          f"({row[k]['blocks']} blocks)", flush=True)
        row['halo_fwd'] = bool(C.conv_uses_halo(dims, dy, dx, False))
        row['halo_dgrad'] = bool(C.conv_uses_halo(dims_d, bdy, bdx, s > 1))
        res.append(row)
        tot['fwd'] += t_f; tot['dgrad'] += t_d; tot['wgrad'] += t_w
        print(f"{name:28s} fwd {t_f:7.3f} ms ({row['fwd_tflops']:6.1f} TF)  dgrad {t_d:7.3f} ({row['dgrad_tflops']:6.1f})"
              f"  wgrad {t_w:7.3f} ({row['wgrad_tflops']:6.1f})  dgrad+acc {t_a:7.3f}" +
              (f"  dgrad+bn {t_b:7.3f}" if t_b is not None else '') +
              (f"  miopen-fwd {row['miopen_fwd_ms']:7.3f}" if a.miopen else ''), flush=True)
    print(json.dumps({'batch': a.batch, 'size': a.size, 'halo': a.halo, 'split': a.split, 'layers': res, 'totals_ms': tot}))


if __name__ == '__main__':
    main()
