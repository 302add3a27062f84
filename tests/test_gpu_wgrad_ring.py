"""The weight-gradient GEMM's DMA ring and pixel cursor (csrc/conv_wgrad_gemm.hip) on blocks that run many stages:
every configuration, prologue off and on, under forced pixel splits, so that a block runs 1, 2, NS - 1, NS and
more than 2 NS stages, rings wrap, the cursor steps across rows and images, and last splits are uneven.  Against
fp32 torch; every ring variant bitwise equal to its tile geometry's 2 x 64 ring; every launch bitwise repeatable
(MI355X only)."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from medical_segmentation_pytorch_amd.ops.conv import Branch, ConvPlan
from medical_segmentation_pytorch_amd.ops.fm import from_fm_reference, to_fm_reference

pytestmark = pytest.mark.gpu

NUM_CFGS = 11   # every index of the kernel's configuration table (test_table_is_covered)
NO_PROLOGUE = (6, 7, 9)   # tiles wider than 128 k have no deferred-BN prologue: the planner never picks them for one

CASES = [
    # N, H, W, Cin, Cout, (kh, kw), stride, pad, dil, groups
    (9, 6, 6, 72, 72, (3, 3), 1, (1, 1), (1, 1), 1),        # OH*OW = 36 < a stage: every stage crosses an image; 4-pixel tail
    (2, 17, 19, 136, 136, (3, 3), 1, (3, 3), (3, 3), 1),    # OW 19, dilation 3; 11 stages
    (1, 16, 64, 72, 136, (1, 7), 1, (0, 3), (1, 1), 1),     # OW = 64; M an exact multiple of 64
    (2, 10, 70, 72, 72, (3, 3), 2, (1, 1), (1, 1), 1),      # stride 2, OW 35
    (2, 12, 11, 40, 40, (1, 7), 1, (0, 3), (1, 1), 5),      # fused groups; ragged stages
]
SPLITS = [1, 2, 3, 5, 0]   # 0: one split per 64-pixel stage


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture
def ext():
    from medical_segmentation_pytorch_amd.ops import _ext
    C = _ext.require()
    yield C
    C.conv_wgrad_gemm_force_cfg(-1)
    C.conv_wgrad_gemm_force_splits(-1)
    C.conv_set_wgrad_gemm(1)


@functools.lru_cache(maxsize=None)
def _setup(ci_, prologue):
    """Inputs of a case and its fp32 torch weight gradients: built once, shared by every configuration and split."""
    n, h, w, ci, co, (kh, kw), s, pad, dil, groups = CASES[ci_]
    gpu = torch.device('cuda', 0)
    torch.manual_seed(11 + ci_)
    ms = [nn.Conv2d(ci, co, (kh, kw), s, pad, dil, bias=False).to(gpu) for _ in range(groups)]
    plan = ConvPlan(kh, kw, ci, co, [Branch(m.weight, g, 0, kh * kw) for g, m in enumerate(ms)], stride=s,
                    padding=pad, dilation=dil, Go=groups)
    x = _bf(torch.randn(n, ci, h, w, device=gpu))
    xf = to_fm_reference(x)
    oh, ow = plan.out_hw(h, w)
    dims = plan.fwd_dims(n, h, w, oh, ow)
    dy = [t[0] for t in plan.taps_fwd]
    dx = [t[1] for t in plan.taps_fwd]
    gys = [to_fm_reference(_bf(torch.randn(n, co, oh, ow, device=gpu))) for _ in range(groups)]
    xc, xr, z = [], 0, x
    if prologue:
        st = torch.zeros(4, plan.Cgi, device=gpu)
        st[0, :ci] = torch.rand(ci, device=gpu) + 0.5
        st[1, :ci] = torch.randn(ci, device=gpu) * 0.3
        xc, xr = [st], 1
        z = _bf(torch.relu(x * st[0, :ci].view(1, -1, 1, 1) + st[1, :ci].view(1, -1, 1, 1)))
    refs = []
    for g_, m in enumerate(ms):
        wr = m.weight.detach().clone().requires_grad_(True)
        F.conv2d(z, wr, None, s, pad, dil).backward(from_fm_reference(gys[g_], co))
        refs.append(wr.grad.detach())
    return plan, xf, gys, xc, xr, dims, dy, dx, refs, n * oh * ow


def _slabs(C, cfg, nsplit, setup):
    plan, xf, gys, xc, xr, dims, dy, dx, _, _ = setup
    C.conv_wgrad_gemm_force_cfg(cfg)
    C.conv_wgrad_gemm_force_splits(nsplit)
    assert C.conv_uses_wgrad_gemm(dims, dy, dx, False)
    assert C.conv_wgrad_gemm_plan_cfg(dims, dy, dx, bool(xc)) == cfg   # the launch runs the configuration asked for
    nrep = C.conv_wgrad_replicas(dims, dy, dx, False, False, bool(xc))
    dwp = torch.full((nrep * plan.rows * plan.T * plan.Cip,), float('nan'), device=xf.device)
    C.conv_wgrad(gys, [xf], dwp, dims, dy, dx, False, xc, xr)
    return dwp, nrep


def test_table_is_covered(ext):
    assert ext.conv_wgrad_gemm_num_cfgs() == NUM_CFGS
    wide = tuple(c for c in range(NUM_CFGS) if 32 * ext.conv_wgrad_gemm_cfg_info(c)[1] * ext.conv_wgrad_gemm_cfg_info(c)[3] > 128)
    assert wide == NO_PROLOGUE


@pytest.mark.parametrize('nsplit', SPLITS)
@pytest.mark.parametrize('prologue,cfg', [(p, c) for p in (False, True) for c in range(NUM_CFGS)
                                          if not (p and c in NO_PROLOGUE)])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_wgrad_ring(gpu, ext, case, prologue, cfg, nsplit):
    C = ext
    setup = _setup(case, prologue)
    plan, _, _, _, _, _, _, _, refs, m = setup
    n, h, w, ci, co, (kh, kw), s, pad, dil, groups = CASES[case]
    nst = -(-m // 64)
    nsplit = nsplit or nst
    C.conv_set_wgrad_gemm(2)   # the GEMM kernel for every eligible shape
    dwp, nrep = _slabs(C, cfg, nsplit, setup)
    per = -(-nst // min(nsplit, nst))
    assert nrep == -(-nst // per)
    KT = plan.T * plan.Cip
    tot = dwp.view(nrep, plan.rows, KT).sum(0)   # [rows][t*Cip + c]
    for g_ in range(groups):
        got = tot[g_ * plan.Cgo:g_ * plan.Cgo + co].view(co, plan.T, plan.Cip)[:, :, :ci].permute(0, 2, 1)
        assert _rel(got.reshape(co, ci, kh, kw), refs[g_]) < 1e-2, g_
    again, _ = _slabs(C, cfg, nsplit, setup)
    assert torch.equal(dwp, again)   # (NaN-free: every slab element is written, and equal bit for bit)
    base = C.conv_wgrad_gemm_cfg_info(cfg)[6]
    if base != cfg:   # a ring variant: the same MFMAs on the same operands in the same order as its 2 x 64 ring
        ref_slabs, nrep_b = _slabs(C, base, nsplit, setup)
        assert nrep_b == nrep and torch.equal(dwp, ref_slabs)
