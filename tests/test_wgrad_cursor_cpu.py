"""The weight-gradient GEMM's pixel cursor (csrc/wgrad_walk.h: wg_walk_make / wg_cursor_init / wg_cursor_advance /
wg_cursor_in, the functions the kernel itself steps its X addresses with) against divmod, on the host: for a lane
that starts at output pixel `row` and advances `step` pixels per stage, every stage's (inside the batch and the
image, input pixel index) must equal the per-stage division the kernel used to do.  Equality is exact.  Also the
host-side planner knobs the ring tests rely on."""
import itertools

import pytest

from medical_segmentation_pytorch_amd.ops import _ext

pytestmark = pytest.mark.skipif(not _ext.available(), reason='HIP extension not built')

NS_ = (1, 2, 9, 23)
OHS = (1, 3, 6, 11, 17)
OWS = (1, 5, 6, 19, 64, 70)
ROWS = (0, 7, 63, 141)                  # lanes of the first stage, and one of a later split
TAPS = ((-1, -1), (0, 1), (3, -3))      # 3x3 corner, 1x7-like, dilation 3


def _divmod_trace(n_, ih_, iw_, oh_, ow_, stride, row, tap, step, stages):
    out = []
    for s in range(stages):
        m = row + s * step
        n, r = divmod(m, oh_ * ow_)
        oh, ow = divmod(r, ow_)
        ih, iw = oh * stride + tap[0], ow * stride + tap[1]
        inside = n < n_ and 0 <= ih < ih_ and 0 <= iw < iw_
        out.append((inside, (n * ih_ + ih) * iw_ + iw if inside else -1))
    return out


@pytest.mark.parametrize('step', [16, 32, 64])   # pixels between a lane's consecutive DMA instructions / stages
@pytest.mark.parametrize('stride', [1, 2])
def test_cursor_matches_divmod(stride, step):
    C = _ext.require()
    checked = 0
    for n_, oh_, ow_, row, tap in itertools.product(NS_, OHS, OWS, ROWS, TAPS):
        ih_, iw_ = oh_ * stride, ow_ * stride   # a padded 3x3-like conv: OH = IH / stride
        m_tot = n_ * oh_ * ow_
        stages = max(0, -(-(m_tot - row) // step)) + 3   # to three stages past M
        got = C.wgrad_cursor_trace([n_, ih_, iw_, oh_, ow_, stride], row, list(tap), step, stages)
        want = _divmod_trace(n_, ih_, iw_, oh_, ow_, stride, row, tap, step, stages)
        assert [(bool(a), int(b)) for a, b in got] == want, (n_, oh_, ow_, stride, row, tap, step)
        checked += 1
    assert checked == len(NS_) * len(OHS) * len(OWS) * len(ROWS) * len(TAPS)


def test_cursor_unpadded_and_wide_inputs():
    """IW > OW*stride (no padding: the row carry moves base by more than the output row) and a walk that starts
    past the last image."""
    C = _ext.require()
    for (n_, ih_, iw_, oh_, ow_, stride), step in itertools.product(
            [(3, 9, 13, 7, 11, 1), (2, 11, 15, 5, 7, 2), (1, 4, 4, 4, 4, 1)], [16, 32, 64]):
        for row, tap in itertools.product((0, 5, 40, n_ * oh_ * ow_ + 3), ((0, 0), (2, 2), (1, 0))):
            got = C.wgrad_cursor_trace([n_, ih_, iw_, oh_, ow_, stride], row, list(tap), step, 12)
            want = _divmod_trace(n_, ih_, iw_, oh_, ow_, stride, row, tap, step, 12)
            assert [(bool(a), int(b)) for a, b in got] == want


def _dims(n, h, w, cin, cout, k, stride, pad):
    import torch
    from medical_segmentation_pytorch_amd.ops.conv import Branch, ConvPlan
    wt = torch.zeros(cout, cin, k, k)
    p = ConvPlan(k, k, cin, cout, [Branch(wt, 0, 0, k * k)], stride=stride, padding=(pad, pad))
    oh, ow = p.out_hw(h, w)
    return p.fwd_dims(n, h, w, oh, ow), [t[0] for t in p.taps_fwd], [t[1] for t in p.taps_fwd], n * oh * ow


def test_ring_table_and_forced_splits():
    C = _ext.require()
    ncfg = C.conv_wgrad_gemm_num_cfgs()
    infos = [C.conv_wgrad_gemm_cfg_info(i) for i in range(ncfg)]
    for i, (wm, wn, fm, fn, ns, bp, base) in enumerate(infos):
        assert infos[base][:4] == [wm, wn, fm, fn] and infos[base][4:] == [2, 64, base]   # the 2 x 64 ring, same tile
        assert ns >= 2 and bp in (32, 64)
        if i < 9:
            assert base == i   # the nine tile geometries keep their indices
    dims, dy, dx, m = _dims(2, 17, 19, 136, 136, 3, 1, 1)
    nst = -(-m // 64)
    try:
        for want in (1, 2, 3, 5, nst, 10 * nst):
            C.conv_wgrad_gemm_force_splits(want)
            per = -(-nst // min(want, nst))
            assert C.conv_wgrad_replicas(dims, dy, dx, False) == -(-nst // per)   # splits of 64-pixel stages, none empty
        C.conv_wgrad_gemm_force_splits(-1)
        planned = C.conv_wgrad_replicas(dims, dy, dx, False)
        # the ring a geometry runs on never changes the split count
        geom = C.conv_wgrad_gemm_plan_cfg(dims, dy, dx, False)
        base = infos[geom][6]
        for v in range(ncfg):
            if infos[v][6] == base:
                C.conv_wgrad_gemm_set_ring(base, v)
                assert C.conv_wgrad_gemm_plan_cfg(dims, dy, dx, False) == v
                assert C.conv_wgrad_replicas(dims, dy, dx, False) == planned
    finally:
        C.conv_wgrad_gemm_force_splits(-1)
        for b in range(9):
            C.conv_wgrad_gemm_set_ring(b, -1)


def test_gemm_refuses_inputs_past_the_32_bit_cursor():
    C = _ext.require()
    dims, dy, dx, _ = _dims(2, 64, 64, 64, 64, 3, 1, 1)
    assert C.conv_uses_wgrad_gemm(dims, dy, dx, False)
    big, dy, dx, _ = _dims(1 << 19, 64, 64, 64, 64, 3, 2, 1)   # N*IH*IW = 2^31, M = 2^29
    assert not C.conv_uses_wgrad_gemm(big, dy, dx, False)
