"""The epilogues of the LDS-tiled implicit-GEMM conv kernel (csrc/conv_gemm.hip) over every tile configuration:
the BN-backward epilogue (stored output and partials, per 128-pixel row), the forward statistics (per row), the
accumulating epilogue (+ bias, run-to-run bits) and the phase launches of a stride-2 data-gradient (MI355X only).
Tiny shapes: what can go wrong here is tails and index mix-ups (wave, half, row, group), not size."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from medical_segmentation_pytorch_amd.ops.conv import Branch, ConvPlan, check_parked_grads, conv, park_input_grad
from medical_segmentation_pytorch_amd.ops.fm import cpad, from_fm_reference, to_fm_reference

pytestmark = pytest.mark.gpu

CFGS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture
def ext():
    from medical_segmentation_pytorch_amd.ops import _ext
    C = _ext.require()
    yield C
    C.conv_gemm_force_cfg(-1)
    C.conv_set_gemm(True)


def _rows128(t):
    """[pixels, C] -> list of the 128-pixel statistic rows' slices."""
    return [t[i:i + 128] for i in range(0, t.shape[0], 128)]


def _launch(gpu, n, h, w, ci, co, k, pad, bias=False, seed=5):
    torch.manual_seed(seed)
    m = nn.Conv2d(ci, co, k, 1, pad, bias=bias).to(gpu)
    plan = ConvPlan(k[0], k[1], ci, co, [Branch(m.weight)], padding=pad, bias=m.bias if bias else None)
    x = to_fm_reference(_bf(torch.randn(n, ci, h, w, device=gpu)))
    dims = plan.fwd_dims(n, h, w, h, w)
    dy = [t[0] for t in plan.taps_fwd]
    dx = [t[1] for t in plan.taps_fwd]
    return m, plan, x, plan.pack_fwd(gpu), dims, dy, dx


def _bn_operands(gpu, n, h, w, co):
    y_bn = to_fm_reference(_bf(torch.randn(n, co, h, w, device=gpu)))
    coef = torch.zeros(3, cpad(co), device=gpu)
    coef[0, :co] = torch.rand(co, device=gpu) + 0.5
    coef[1, :co] = torch.randn(co, device=gpu) * 0.2
    coef[2, :co] = torch.randn(co, device=gpu) * 0.1
    return y_bn, coef


BN_SHAPE = (2, 11, 13, 72, 136)   # 286 pixels: two full 128-pixel statistic rows + a 30-pixel tail


@pytest.mark.parametrize('cfg', CFGS)
def test_bn_epilogue_stores_what_the_plain_launch_stores(gpu, ext, cfg):
    C = ext
    n, h, w, ci, co = BN_SHAPE
    C.conv_gemm_force_cfg(cfg)
    _, plan, x, wp, dims, dy, dx = _launch(gpu, n, h, w, ci, co, (3, 3), (1, 1))
    assert C.conv_uses_gemm(dims, dy, dx, False)
    y_bn, coef = _bn_operands(gpu, n, h, w, co)
    plain = torch.full((n, h, w, cpad(co)), 7.0, device=gpu, dtype=torch.bfloat16)
    out = torch.full_like(plain, -3.0)
    part = torch.empty(C.conv_stat_blocks(dims, dy, dx), 2, cpad(co), device=gpu)
    C.conv_fwd([x], wp, [plain], None, None, dims, dy, dx, False)
    C.conv_fwd_bn([x], wp, [out], part, dims, dy, dx, y_bn, coef, True)
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16))


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('cfg', CFGS)
def test_bn_epilogue_partials_per_row(gpu, ext, cfg, relu):
    """sum g and sum g*(y - mean), g = dz * relu'(y*scale + shift), against fp64 sums of the stored output: in
    total and for each 128-pixel row on its own (a wave or half mix-up keeps the total and moves a row)."""
    C = ext
    n, h, w, ci, co = BN_SHAPE
    C.conv_gemm_force_cfg(cfg)
    _, plan, x, wp, dims, dy, dx = _launch(gpu, n, h, w, ci, co, (3, 3), (1, 1))
    y_bn, coef = _bn_operands(gpu, n, h, w, co)
    out = torch.empty(n, h, w, cpad(co), device=gpu, dtype=torch.bfloat16)
    nblk = C.conv_stat_blocks(dims, dy, dx)
    assert nblk == 3
    part = torch.full((nblk, 2, cpad(co)), float('nan'), device=gpu)
    C.conv_fwd_bn([x], wp, [out], part, dims, dy, dx, y_bn, coef, relu)
    dz = out.double().reshape(-1, cpad(co))
    yb = y_bn.double().reshape(-1, cpad(co))
    sc, sh, mu = coef.double()
    g = torch.where((yb * sc + sh) > 0, dz, torch.zeros_like(dz)) if relu else dz
    gq = g * (yb - mu)
    tot = part.sum(0)
    print(f'cfg {cfg} relu {relu}: total rel {_rel(tot[0], g.sum(0)):.2e} {_rel(tot[1], gq.sum(0)):.2e}')
    assert _rel(tot[0], g.sum(0)) < 1e-4 and _rel(tot[1], gq.sum(0)) < 1e-4
    for r, (gr, gqr) in enumerate(zip(_rows128(g), _rows128(gq))):
        e0, e1 = _rel(part[r, 0], gr.sum(0)), _rel(part[r, 1], gqr.sum(0))
        print(f'  row {r}: rel {e0:.2e} {e1:.2e}')
        assert e0 < 1e-4 and e1 < 1e-4, r


STAT_CASES = [
    # N, H, W, Cin, Cout, (kh, kw), stride, pad, groups
    (1, 7, 9, 72, 72, (3, 3), 1, (1, 1), 1),      # A: 63 pixels -- less than one tile, not a multiple of 32
    (2, 10, 6, 136, 72, (7, 1), 1, (3, 0), 3),    # B: three output groups, a 32-row fragment straddles groups
    (3, 6, 6, 272, 272, (3, 3), 2, (1, 1), 1),    # C: stride 2, 27 pixels
]


@pytest.mark.parametrize('cfg', CFGS)
@pytest.mark.parametrize('case', STAT_CASES)
def test_forward_statistics_per_row(gpu, ext, case, cfg):
    """sum and sum of squares of the STORED bf16 output, per 128-pixel row and in total, against fp64."""
    n, h, w, ci, co, (kh, kw), s, pad, groups = case
    ext.conv_gemm_force_cfg(cfg)
    torch.manual_seed(0)
    ms = [nn.Conv2d(ci, co, (kh, kw), s, pad, bias=False).to(gpu) for _ in range(groups)]
    plan = ConvPlan(kh, kw, ci, co, [Branch(m.weight, g, 0, kh * kw) for g, m in enumerate(ms)], stride=s,
                    padding=pad, Go=groups)
    xf = to_fm_reference(_bf(torch.randn(n, ci, h, w, device=gpu)))
    oh, ow = plan.out_hw(h, w)
    assert ext.conv_uses_gemm(plan.fwd_dims(n, h, w, oh, ow), [t[0] for t in plan.taps_fwd],
                              [t[1] for t in plan.taps_fwd], False)
    with torch.no_grad():
        ys, part = conv(plan, [xf], want_stats=True)
    yv = torch.cat([y.double().reshape(-1, cpad(co)) for y in ys], 1)
    assert part.shape[0] == (yv.shape[0] + 127) // 128

    def check(p, v, what):
        e0 = ((p[0].double() - v.sum(0)).abs() / v.abs().sum(0).clamp_min(1e-6)).max().item()
        e1 = _rel(p[1], (v * v).sum(0))
        print(f'cfg {cfg} {what}: {e0:.2e} {e1:.2e}')
        assert e0 < 1e-4 and e1 < 1e-4, what

    check(part.sum(0), yv, 'total')
    for r, v in enumerate(_rows128(yv)):
        check(part[r], v, f'row {r}')


@pytest.mark.parametrize('cfg', CFGS)
def test_accumulate_epilogue(gpu, ext, cfg):
    C = ext
    n, h, w, ci, co = BN_SHAPE
    C.conv_gemm_force_cfg(cfg)
    m, plan, x, wp, dims, dy, dx = _launch(gpu, n, h, w, ci, co, (3, 3), (1, 1))
    base = to_fm_reference(_bf(torch.randn(n, co, h, w, device=gpu)))
    y, y2 = base.clone(), base.clone()
    C.conv_fwd([x], wp, [y], None, None, dims, dy, dx, False, accumulate=True)
    C.conv_fwd([x], wp, [y2], None, None, dims, dy, dx, False, accumulate=True)
    yr = F.conv2d(from_fm_reference(x, ci), _bf(m.weight.detach()), None, 1, 1)
    assert _rel(from_fm_reference(y, co), yr + from_fm_reference(base, co)) < 1e-2
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


@pytest.mark.parametrize('cfg', CFGS)
def test_accumulate_epilogue_with_bias(gpu, ext, cfg):
    """y += conv(x) + bias at 40 output channels (1 x 7): the bias row and the padded channels' zero."""
    C = ext
    n, h, w, ci, co = 1, 7, 19, 64, 40
    C.conv_gemm_force_cfg(cfg)
    m, plan, x, wp, dims, dy, dx = _launch(gpu, n, h, w, ci, co, (1, 7), (0, 3), bias=True)
    assert C.conv_uses_gemm(dims, dy, dx, False)
    base = to_fm_reference(_bf(torch.randn(n, co, h, w, device=gpu)))
    bias = m.bias.detach().float().contiguous()
    y, y2 = base.clone(), base.clone()
    C.conv_fwd([x], wp, [y], bias, None, dims, dy, dx, False, accumulate=True)
    C.conv_fwd([x], wp, [y2], bias, None, dims, dy, dx, False, accumulate=True)
    yr = F.conv2d(from_fm_reference(x, ci), _bf(m.weight.detach()), bias, 1, (0, 3))
    assert _rel(from_fm_reference(y, co), yr + from_fm_reference(base, co)) < 1e-2
    if co < cpad(co):
        assert y[..., co:].abs().max().item() == 0.0
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


@pytest.mark.parametrize('parked', [False, True])
@pytest.mark.parametrize('cfg', CFGS)
def test_strided_data_gradient_phases(gpu, ext, cfg, parked):
    """The stride-2 data-gradient through autograd (one launch per phase), alone and accumulating into the parked
    gradient of the input's other reader."""
    n, h, w, ci, co = 3, 6, 6, 272, 272
    ext.conv_gemm_force_cfg(cfg)
    torch.manual_seed(1)
    m = nn.Conv2d(ci, co, 3, 2, 1, bias=False).to(gpu)
    plan = ConvPlan(3, 3, ci, co, [Branch(m.weight)], stride=2, padding=(1, 1))
    x = _bf(torch.randn(n, ci, h, w, device=gpu))
    xf = to_fm_reference(x).requires_grad_(True)
    (y,), _ = conv(plan, [xf])
    xr = x.clone().requires_grad_(True)
    ref = F.conv2d(xr, _bf(m.weight.detach()), None, 2, 1)
    g = _bf(torch.randn_like(ref))
    ref.backward(g)
    want = xr.grad
    if parked:
        other = _bf(torch.randn_like(x))
        park_input_grad(xf, to_fm_reference(other))
        want = want + other
    try:
        y.backward(to_fm_reference(g))
    finally:
        try:
            check_parked_grads()   # (a failed backward must not leave its parked gradient to the next test)
        except RuntimeError:
            pass
    assert _rel(from_fm_reference(xf.grad, ci), want) < 2e-2
