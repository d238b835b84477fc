"""CPU checks of which instantiation of the recurrent-layer kernel a launch takes (skinny_pick in csrc/k_gemm.hip, through
bvc_test_skinny_pick: host arithmetic only, no device).  The rule is restated in tests/skinny_kernels.py from the comments of
launch_gemm_skinny; what the kernels then compute is tests/test_gpu_skinny_tiles.py's business."""
import ctypes

import pytest

import skinny_kernels as sk

ROWS = range(1, 131)
REQUESTS = (1, 2, 4, 3, 0, 8)
# (epilogue, gate-interleaved weights)
LAUNCHES = ((sk.EPI_LINEAR, 0), (sk.EPI_ELU, 0), (sk.EPI_SIGMOID, 0), (sk.EPI_CODE, 0), (sk.EPI_MEL, 0), (sk.EPI_GRU, 0), (sk.EPI_GRU, 1),
            (sk.EPI_GRU_PART, 0))


@pytest.fixture(scope="module")
def lib():
    from bvcodec import _abi
    return _abi.load()


@pytest.fixture(scope="module")
def picked(lib):
    """{(M, epi, gate_il, mtw, latency): (kernel, row tiles)} of the whole sweep, asked once."""
    out = {}
    for M in ROWS:
        for epi, il in LAUNCHES:
            for mtw in REQUESTS:
                for latency in (0, 1):
                    rc, got = sk.pick(lib, M, epi, il, mtw, latency)
                    assert rc == 0, (M, epi, il, mtw, latency)
                    out[(M, epi, il, mtw, latency)] = got
    return out


def test_pick_equals_the_rule(picked):
    assert len(picked) == 130 * 8 * 6 * 2
    bad = [(k, got, sk.rule(*k)) for k, got in picked.items() if got != sk.rule(*k)]
    assert not bad, bad[:8]
    seen = {got[0] for got in picked.values()}
    assert seen == set(range(sk.SK_COUNT)), seen                   # the sweep reaches every kernel of the table


def test_the_rule_at_its_edges(picked):
    """The statements of the issue, spelled out on the sweep's own answers."""
    for (M, epi, il, mtw, latency), (k, tiles_per_wg) in picked.items():
        tiles = (M + 15) // 16
        assert tiles_per_wg == sk.SHAPE[k][3] and tiles_per_wg <= max(tiles, 1)      # no workgroup is asked for more tiles than the launch has
        linear = epi not in (sk.EPI_GRU, sk.EPI_GRU_PART)
        assert (k in (sk.SK_LIN, sk.SK_LIN_LATENCY, sk.SK_LIN2, sk.SK_LIN4)) == linear
        if k == sk.SK_LIN_LATENCY:
            assert latency and linear and tiles_per_wg == 1
        if linear and latency:
            assert k != sk.SK_LIN
        if not latency:
            assert k != sk.SK_LIN_LATENCY
        if mtw in (0, 1) or (mtw in (3, 8) and mtw <= tiles):      # (a request above the tile count is mapped to 4, 2 or 1 FIRST)
            assert tiles_per_wg == 1
        if epi == sk.EPI_GRU:
            assert k == (sk.SK_GRU if not il else sk.SK_GRU_IL2 if tiles_per_wg == 2 else sk.SK_GRU_IL)
            assert tiles_per_wg <= 2                                # four sets of GRU partial tiles exceed the LDS
        if epi == sk.EPI_GRU_PART:
            assert k == sk.SK_GRU_PART
    # the clamp by the tile count: a request of 4 (or 8) on 1, 2 .. 3, >= 4 tiles
    for req in (4, 8):
        for M, want in ((1, sk.SK_LIN), (16, sk.SK_LIN), (17, sk.SK_LIN2), (48, sk.SK_LIN2), (49, sk.SK_LIN4), (112, sk.SK_LIN4)):
            assert picked[(M, sk.EPI_ELU, 0, req, 0)][0] == want, (req, M)
    # ... and a request that is neither 2 nor 4 and not above the tile count is 1
    assert picked[(128, sk.EPI_ELU, 0, 8, 0)][0] == sk.SK_LIN and picked[(130, sk.EPI_ELU, 0, 8, 0)][0] == sk.SK_LIN
    assert picked[(130, sk.EPI_ELU, 0, 4, 0)][0] == sk.SK_LIN4 and picked[(48, sk.EPI_ELU, 0, 3, 0)][0] == sk.SK_LIN
    assert picked[(16, sk.EPI_ELU, 0, 2, 0)][0] == sk.SK_LIN and picked[(17, sk.EPI_ELU, 0, 2, 0)][0] == sk.SK_LIN2
    assert picked[(33, sk.EPI_GRU, 1, 4, 0)] == (sk.SK_GRU_IL2, 2) and picked[(16, sk.EPI_GRU, 1, 4, 0)] == (sk.SK_GRU_IL, 1)


def test_lds_of_every_picked_kernel_fits_a_compute_unit(picked):
    for k in {got[0] for got in picked.values()}:
        assert sk.lds_kib(k) <= sk.LDS_KIB_PER_CU, (sk.NAMES[k], sk.lds_kib(k))
    assert sk.lds_kib(sk.SK_GRU_IL2) == 96 and sk.lds_kib(sk.SK_LIN4) == 32 and sk.lds_kib(sk.SK_LIN) == 8


def test_multi_frame_twins_exist_for_the_linear_kernels_only(picked):
    """launch_gemm_skinny refuses frames > 1 under a GRU epilogue and has a twin for every other kernel: a multi-frame request is
    served exactly where the picked kernel is none of the GRU-shaped ones."""
    for (M, epi, il, mtw, latency), (k, _) in picked.items():
        assert sk.SHAPE[k][4] == (epi not in (sk.EPI_GRU, sk.EPI_GRU_PART)), (M, epi, il, mtw, latency, sk.NAMES[k])


def test_pick_refusals_and_counts_without_a_device(lib):
    out = (ctypes.c_int32 * 2)()
    assert lib.bvc_test_skinny_pick(0, sk.EPI_ELU, 0, 1, 0, out) == sk.BVC_EINVAL
    assert lib.bvc_test_skinny_pick(5, 7, 0, 1, 0, out) == sk.BVC_EINVAL and lib.bvc_test_skinny_pick(5, -1, 0, 1, 0, out) == sk.BVC_EINVAL
    assert lib.bvc_test_skinny_pick(5, sk.EPI_ELU, 1, 1, 0, out) == sk.BVC_EINVAL      # gate-interleaved weights: the GRU launch only
    assert lib.bvc_test_skinny_pick(5, sk.EPI_ELU, 0, 1, 0, None) == sk.BVC_EINVAL
    assert b"bvc_test_skinny_pick" in lib.bvc_last_error()
    assert sk.pick(lib, 2 ** 31 - 1, sk.EPI_ELU, 0, 4, 0) == (0, (sk.SK_LIN4, 4))       # the largest row count an int32 holds
    assert lib.bvc_test_skinny_counts(None) == sk.BVC_EINVAL
    c = sk.counts(lib)
    assert c.shape == (2, sk.SK_COUNT) and (c >= 0).all()
    # the refusals of bvc_test_linear_tiles come before anything touches a device
    for M, N, K, frames in ((5, 24, 16, 1), (5, 16, 24, 1), (5, 16, 16, 0), (5, 16, 16, -1), (5, 0, 16, 1)):
        assert lib.bvc_test_linear_tiles(None, None, None, M, N, K, 0, 1, frames, None, None) == sk.BVC_EINVAL, (M, N, K, frames)
    assert (sk.counts(lib) == c).all()
