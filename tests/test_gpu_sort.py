"""Segmented radix sort (``csrc/sort.hip``) on the MI355X: bitwise against ``torch.sort(descending, stable)`` on
the CPU at every size around the wave and the tile, on key patterns that vary every digit position and that put
all keys into one digit; counter width, keys ordered by their bits, repeatability."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _tile():
    from medical_segmentation_pytorch_amd.ops._ext import require
    return require().sort_tile()


def _patterns(q, p, g):
    special = torch.tensor([0.0, 2.0 ** -149, 2.0 ** -126, 0.5, 1 - 2.0 ** -24, 1.0])
    asc = torch.linspace(0, 1, p).expand(q, p)
    low = (torch.full((q, p), 0.5).view(torch.int32) | torch.randint(0, 2, (q, p), generator=g, dtype=torch.int32))
    return {
        'uniform': torch.rand(q, p, generator=g),
        'all_equal': torch.full((q, p), 0.37),
        'two_values': torch.where(torch.rand(q, p, generator=g) < 0.5, 0.25, 0.75),
        'ascending': asc.clone(),
        'descending': asc.flip(1).clone(),
        'every_digit': special[torch.arange(q * p) % 6].reshape(q, p).clone(),
        'lowest_bit': low.view(torch.float32),
    }


def _check(keys, gpu):
    from medical_segmentation_pytorch_amd.ops.sort import sort_segments
    ref_v, ref_i = torch.sort(keys, dim=1, descending=True, stable=True)
    v, i = sort_segments(keys.to(gpu))
    assert v.dtype == torch.float32 and i.dtype == torch.int32 and v.shape == i.shape == keys.shape
    assert torch.equal(v.cpu().view(torch.int32), ref_v.view(torch.int32))
    assert torch.equal(i.cpu().long(), ref_i)


SIZES = {'1': lambda T: 1, '2': lambda T: 2, '63': lambda T: 63, '64': lambda T: 64, '65': lambda T: 65,
         'T-1': lambda T: T - 1, 'T': lambda T: T, 'T+1': lambda T: T + 1, '3T+17': lambda T: 3 * T + 17}


@pytest.mark.parametrize('q', [1, 3])
@pytest.mark.parametrize('size', list(SIZES))
def test_bitwise_against_torch_sort(gpu, size, q):
    p = SIZES[size](_tile())
    g = torch.Generator().manual_seed(p + q)
    for name, keys in _patterns(q, p, g).items():
        assert keys.shape == (q, p) and keys.dtype == torch.float32, name
        _check(keys, gpu)


def test_denormals_survive_the_host_sort():
    """The reference of the 'every_digit' pattern needs a host sort that does not flush denormals."""
    k = torch.tensor([[0.0, 2.0 ** -149, 0.0, 2.0 ** -126]])
    assert torch.sort(k, dim=1, descending=True, stable=True)[1].tolist() == [[3, 1, 0, 2]]


def test_counter_width(gpu):
    """70001 equal keys in one row: every key of a tile lands in one digit, every tile in one table row; a rank or
    an offset narrower than 32 bits wraps."""
    _check(torch.full((1, 70001), 0.625), gpu)


def test_any_bit_pattern_is_ordered_by_its_bits(gpu):
    """Negative, NaN and infinite keys: the result is a permutation, descending by the uint32 pattern, stable."""
    from medical_segmentation_pytorch_amd.ops.sort import sort_segments
    t = _tile()
    g = torch.Generator().manual_seed(11)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, t + 77), generator=g, dtype=torch.int64)
    bits[:, 1::2] = bits[:, 0:-1:2]                                  # every key twice (the row length is odd)
    keys = bits.to(torch.int32).view(torch.float32)
    v, i = sort_segments(keys.to(gpu))
    u = bits & 0xffffffff
    ref_u, ref_i = torch.sort(u, dim=1, descending=True, stable=True)
    assert torch.equal(v.cpu().view(torch.int32).long() & 0xffffffff, ref_u)
    assert torch.equal(i.cpu().long(), ref_i)


def test_repeatable_and_input_unchanged(gpu):
    from medical_segmentation_pytorch_amd.ops.sort import sort_segments
    keys = torch.rand(3, 2 * _tile() + 5, generator=torch.Generator().manual_seed(2)).to(gpu)
    keep = keys.clone()
    v1, i1 = sort_segments(keys)
    v2, i2 = sort_segments(keys)
    assert torch.equal(v1, v2) and torch.equal(i1, i2) and torch.equal(keys, keep)


def test_rejects_wrong_input(gpu):
    from medical_segmentation_pytorch_amd.ops.sort import sort_segments
    with pytest.raises(ValueError, match='fp32'):
        sort_segments(torch.zeros(4, device=gpu))
    with pytest.raises(ValueError, match='fp32'):
        sort_segments(torch.zeros(2, 4, device=gpu, dtype=torch.float64))
