"""CPU checks of the tile cuts (tile_plan / gemm_batched_cut / amp_pair_cut) through bvc_test_tile_plan: host arithmetic only,
the library loads without a GPU."""
import ctypes

import pytest

GEMM, AMP64 = 0, 1
PLANNED, LEGACY = 0, 1
GEMM_SLOTS = 512
AMP_SLOTS = 512
AMP_HEIGHTS = (128, 112, 96, 80)
GEMM_HEIGHTS = (144, 128, 112)

# (utterances, frames per utterance): configs[1] 64 x 5 s, the 64 x 10 s target leg, 256 x 5 s in one call
SHAPES = [(64, 430), (64, 861), (256, 430)]


def cut(kind, rows, column_blocks, ks=0, mode=PLANNED):
    from bvcodec import _abi
    out = (ctypes.c_int64 * 6)()
    _abi.check(_abi.load().bvc_test_tile_plan(kind, rows, column_blocks, ks, mode, out))
    return dict(zip(("height", "blocks", "tail_height", "tiles", "rounds", "cost100"), out))


def gemm_rows_covered(c, M):
    """Rows the launches of a GEMM cut compute, as (first, last + 1) spans in order."""
    if c["tail_height"] == 0:
        return [(i * c["height"], (i + 1) * c["height"]) for i in range(c["blocks"])]
    spans = [(i * 128, (i + 1) * 128) for i in range(c["blocks"])]
    m_off = c["blocks"] * 128
    n_tail = -(-(M - m_off) // c["tail_height"])
    return spans + [(m_off + i * c["tail_height"], m_off + (i + 1) * c["tail_height"]) for i in range(n_tail)]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("column_blocks", [8, 24])
def test_gemm_cut_is_no_dearer_than_the_two_launch_cut_and_covers_every_row_once(B, T, column_blocks):
    M = B * T
    new, old = cut(GEMM, M, column_blocks), cut(GEMM, M, column_blocks, mode=LEGACY)
    assert new["height"] in GEMM_HEIGHTS and old["height"] == 128
    assert new["cost100"] <= old["cost100"], (new, old)
    for c in (new, old):
        spans = gemm_rows_covered(c, M)
        assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))     # each row exactly once
        assert spans[-1][0] < M <= spans[-1][1]
        last_height = c["tail_height"] or c["height"]
        assert spans[-1][1] - M < last_height                                               # padded rows per column block
        assert c["tiles"] == column_blocks * len(spans)
    assert new["rounds"] == -(-new["tiles"] // GEMM_SLOTS)
    # the benchmark shapes land on whole rounds in ONE launch
    assert new["tail_height"] == 0
    assert new["rounds"] * GEMM_SLOTS - new["tiles"] < 0.03 * new["tiles"], new


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("ks", [3, 7, 11])
def test_amp_cut_is_no_dearer_than_the_single_shape_and_covers_every_row_once(B, T, ks):
    L = 8 * (T + 1)                                        # rows of the C = 64 stage
    new, old = cut(AMP64, L, B, ks), cut(AMP64, L, B, ks, mode=LEGACY)
    assert old["height"] == AMP_HEIGHTS[0] and new["height"] in AMP_HEIGHTS
    assert new["cost100"] <= old["cost100"], (new, old)
    for c in (new, old):
        out_rows = c["height"] - (ks - 1)
        per_item = c["blocks"]
        assert (per_item - 1) * out_rows < L <= per_item * out_rows          # consecutive tiles of out_rows rows: once each
        assert per_item * out_rows - L < c["height"]
        assert c["tiles"] == per_item * B
        assert c["rounds"] == -(-c["tiles"] // AMP_SLOTS)


@pytest.mark.parametrize("height", GEMM_HEIGHTS)
@pytest.mark.parametrize("M", [27520, 11129, 300, 5])
def test_forced_gemm_heights_cover_the_rows(height, M):
    c = cut(GEMM, M, 8, mode=height)
    assert c["height"] == height and c["tail_height"] == 0
    assert (c["blocks"] - 1) * height < M <= c["blocks"] * height
    assert c["tiles"] == 8 * c["blocks"] and c["rounds"] == -(-c["tiles"] // GEMM_SLOTS)


def test_degenerate_inputs():
    assert cut(GEMM, 0, 8)["height"] == 0 and cut(GEMM, 0, 8)["tiles"] == 0                 # no rows: nothing to launch
    assert cut(AMP64, 0, 64, 7)["height"] == 0
    assert cut(GEMM, 27520, 8, mode=100)["height"] == 0                                     # not a compiled height
    assert cut(AMP64, 3448, 64, 7, mode=64)["height"] == 0
    for M in (1, 5, 111):                                                                    # fewer rows than any tile
        for column_blocks in (1, 8):
            c = cut(GEMM, M, column_blocks)
            assert c["blocks"] == 1 and c["tail_height"] == 0 and c["tiles"] == column_blocks and c["rounds"] == 1
            assert c["height"] == min(GEMM_HEIGHTS)        # one round either way: the shortest tile is the cheapest
    c = cut(AMP64, 5, 1, 11)
    assert c["blocks"] == 1 and c["tiles"] == 1 and c["rounds"] == 1
    c = cut(GEMM, 1 << 22, 1)                                                               # one column block, many rows
    assert c["tail_height"] == 0 or c["height"] == 128
    assert sum(b - a for a, b in gemm_rows_covered(c, 1 << 22)) >= 1 << 22
