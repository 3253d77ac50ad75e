"""No GPU: harp_taubin_smooth refuses empty sizes before any launch, and harp_taubin_ws_bytes is pure host arithmetic (include/harp_hip.h).
As in tests/test_abi.py::test_building_blocks_refuse_empty_sizes_without_launch only sizes are tried, with fake pointers, for which an
entry point WITHOUT the check would reach no kernel either: B = 0 (an empty grid in both modes), V = 0 and V = -1 in mode 2 (grid x =
(V + 255) / 256 = 0) and num_iter = -1 in mode 2 (a loop of 2 * num_iter launches that never runs).  B = -1, V <= 0 in the LDS mode, whose
grid is the frame count, the null pointers and mode 1 past its capacity are refused with real buffers in tests/test_gpu_taubin.py."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_taubin_refuses_empty_sizes_without_launch(lib):
    f = 1 << 20                                                # a fake device pointer, never dereferenced
    for mode in (0, 1, 2):
        assert lib.harp_taubin_smooth(f, f, f, 0, 65, 0.53, -0.53, 10, mode, f, f, None) == 1, mode
    for V in (0, -1):
        assert lib.harp_taubin_smooth(f, f, f, 2, V, 0.53, -0.53, 10, 2, f, f, None) == 1, V
    assert lib.harp_taubin_smooth(f, f, f, 2, 65, 0.53, -0.53, -1, 2, f, f, None) == 1


def test_taubin_ws_bytes_is_host_arithmetic(lib):
    up = lambda n: (n + 255) // 256 * 256
    for B, V in [(1, 1), (1, 4), (3, 65), (32, 3093), (8, 4083), (1, 4160), (7, 1122)]:
        assert lib.harp_taubin_ws_bytes(B, V) == 2 * up(12 * B * V), (B, V)
    assert lib.harp_taubin_ws_bytes(1, 1) == 512
    assert lib.harp_taubin_ws_bytes(65535, 4083) == 2 * up(12 * 65535 * 4083)        # past 2^31 bytes: size_t throughout
    for B, V in [(0, 5), (5, 0), (-1, 5), (5, -1)]:
        assert lib.harp_taubin_ws_bytes(B, V) == 0, (B, V)
