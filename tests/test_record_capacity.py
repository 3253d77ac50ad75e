"""The capacity of a texel tile's record list (harp_shade_args.trec_cap): harp_shade_bwd and harp_texel_reduce refuse any value that is
no multiple of 4, so every caller takes it from ops.texel_record_capacity, which rounds the size-dependent rule up."""
import pytest

from harp_amd import ops


@pytest.mark.parametrize("B,S", [(1, 300), (1, 301), (1, 500), (27, 300), (3, 1000), (1, 128), (2, 512), (32, 512), (32, 1024)])
@pytest.mark.parametrize("div,floor", [(8, 4096), (32, 65536)])          # the reference-API backward (ops._Shade), FitEngine's defaults
def test_texel_record_capacity_is_a_multiple_of_4(B, S, div, floor):
    raw = max(floor, B * S * S // div)
    cap = ops.texel_record_capacity(B * S * S, div, floor)
    assert cap % 4 == 0 and raw <= cap < raw + 4, (B, S, div, floor, raw, cap)


def test_texel_record_capacity_rounds_the_sizes_that_were_refused():
    # B * S * S // div of these shapes is no multiple of 4: the capacity the kernels used to be handed as it stood
    assert ops.texel_record_capacity(1 * 300 * 300, 8, 4096) == 11252
    assert ops.texel_record_capacity(1 * 301 * 301, 8, 4096) == 11328
    assert ops.texel_record_capacity(1 * 500 * 500, 8, 4096) == 31252
    assert ops.texel_record_capacity(27 * 300 * 300, 32, 65536) == 75940
    assert ops.texel_record_capacity(3 * 1000 * 1000, 32, 65536) == 93752
    assert ops.texel_record_capacity(0, 1 << 30, 50) == 52 and ops.texel_record_capacity(0, 1 << 30, 65538) == 65540
    assert ops.texel_record_capacity(0, 1 << 30, 48) == 48 and ops.texel_record_capacity(3 * 128 * 128, 0, 4096) == 49152
