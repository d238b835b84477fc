"""The case tables of tests/test_gpu_backward_shapes.py without a GPU: the row-count cases reach every path of the weight gradient, the
bias sums, the batched GEMM and the grid-stride loops that a training-sized call runs (backward_oracle.paths, restated from the code);
every new case finds a seed that keeps the margins among its 200, on the forward alone; the seeds of the old cases are the ones the
ledgers of profiles/backward_parity.md were measured at; the chunk sums of every weight gradient fit the workspace carve_backward
gives them, at every accepted size and every row count up to training's; every clipped branch of the KLD occurs under an active bit."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_oracle as bo  # noqa: E402
import bvrnn_draws as bd  # noqa: E402

# select()'s seed minus the case's base, for backward_oracle.CASES in order, as the search that took gradients at every seed found them
OLD_SEED_OFFSETS = (0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2, 0, 0, 0, 1, 2, 1, 1, 6, 1, 0, 0, 0, 0, 0, 1, 0,
                    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
NEW_TABLES = (("rows", bo.ROW_CASES), ("sizes", bo.SIZE_CASES), ("saturated", bo.SATURATED_CASES))


def state_dict(case):
    from bvcodec import synth
    return synth.bvrnn_state_dict(bd.conf_of(case[0], case[2], bo.z_of(case)), 1234, gains=bd.GAINS[case[1]])


def test_old_cases_keep_their_ids_and_seeds():
    assert len(bo.CASES) == len(OLD_SEED_OFFSETS) == 67 and all(len(c) == 7 for c in bo.CASES)
    assert zlib.crc32("|".join(bo.case_id(c) for c in bo.CASES).encode()) == 0x4856C269, "an old case's id changed"
    before = dict(bo.SEARCHED)
    fresh = [c for c in bo.CASES if (c, 64) not in bo._SELECTED]
    got = []
    for case in bo.CASES:
        s = bo.select(case, state_dict(case))
        got.append(s["seed"] - zlib.crc32(bo.case_id(case).encode()) % 100000)
        assert s["tried"] == got[-1] + 1
    assert tuple(got) == OLD_SEED_OFFSETS
    assert bo.SEARCHED["gradients"] - before["gradients"] == len(fresh)          # once per case, not once per seed tried


def test_inputs_take_the_case_z_dim():
    for z in (16, 96, 128):
        c = bo.draw_inputs((128, "default", True, 9, 31, 2, "random", z), 3)
        assert c["noise"].shape == (9, 31, z) and float(c["bits"].max()) == z and float(c["bits"].min()) == 0
        act = torch.arange(z)[None, None, :] < c["bits"][:, :, None]
        assert act.shape == (9, 31, z) and bool(act[:, :, z - 1].any())
    few = bo.draw_inputs((64, "default", True, 17, 16, 0, "upto8"), 3)
    assert set(few["bits"].unique().tolist()) == set(float(n) for n in range(9)) and few["noise"] is None
    old = bo.draw_inputs(bo.CASES[0], 3)
    assert torch.equal(old["bits"], bo.draw_inputs(bo.CASES[0], 3, z_dim=64)["bits"]) and bo.z_of(bo.CASES[0]) == 64
    f64 = dict(arg=torch.full((1, 1, 16), 0.25, dtype=torch.float64), prob=torch.full((1, 1, 16), 0.25, dtype=torch.float64),
               prior=torch.full((1, 1, 16), 0.5, dtype=torch.float64))
    f64["arg"][0, 0, 15] = 0.5                                 # a tie at the last position: seen exactly when that bit is active
    assert bo.margins(f64, torch.tensor([[15.0]]), 16)[0] == 0.25 and bo.margins(f64, torch.tensor([[16.0]]), 16)[0] == 0.0


def test_size_tables_are_the_size_classes():
    sizes = {(h, z): shapes for _, h, z, shapes in bd.SIZE_CLASSES}
    assert set(bo.SIZES) | set(bo.REFUSED_SIZES) == set(sizes) and not set(bo.SIZES) & set(bo.REFUSED_SIZES)
    assert all(bd.forward_runs(h, z) for h, z in bo.SIZES) and not any(bd.forward_runs(h, z) for h, z in bo.REFUSED_SIZES)
    for h, z in bo.SIZES:
        assert {(c[3], c[4]) for c in bo.SIZE_CASES if (c[0], c[7]) == (h, z)} == set(sizes[(h, z)])
        assert {c[1] for c in bo.SIZE_CASES if (c[0], c[7]) == (h, z)} == set(bd.SIZE_DRAWS)
    assert all(c[5] == 2 and c[2] for c in bo.SIZE_CASES)
    assert not bd.forward_fallback_runs(112, 96)              # forward without the caller's z is refused there; backward hands one over
    ids = [bo.case_id(c) for _, t in NEW_TABLES for c in t] + [bo.case_id(c) for c in bo.CASES]
    assert len(set(ids)) == len(ids)


def test_row_cases_reach_every_path():
    """Prints the path table of profiles/backward_parity.md."""
    reach = {bo.case_id(c): bo.paths(c) for c in bo.ROW_CASES}
    for path in bo.PATHS:
        who = [i for i, p in reach.items() if path in p]
        print(f"PATH {path}: {', '.join(who)}")
        assert who, f"no row case reaches: {path}"
    # the old cases: 17 x 7 stacked is 238 rows, one chunk of two blocks (phi_x and the GRU in mode 2) - and no chunked path at all
    old = set().union(*(bo.paths(c) for c in bo.CASES))
    print(f"PATH reached by backward_oracle.CASES: {', '.join(sorted(old))}")
    assert old == {"seam", "col_sum blocks"}
    assert any("seam" in bo.paths(c) and c[4] >= 48 for c in bo.ROW_CASES)            # the long-T form: many frames, many chain switches
    for mode in (0, 1):         # one chain only, above 256 rows: Mg = TB in chunks, r0 = 0 or TB
        assert any(c[5] == mode and c[3] * c[4] > 256 and "chunks ldo != K weight_ih[:, H:]" in bo.paths(c) for c in bo.ROW_CASES), mode
    # the worked examples: 17 x 16 at h_dim 64, 1024 and 1040
    cuts = lambda H: {n: bo.want_cut(M, N, K) + (ldo,) for n, M, N, K, ldo in bo.weight_grads(H, 64, 17, 16, 2)[0]}
    assert cuts(64)["phi_x.0"] == (3, 256, 80) and 544 - 2 * 256 == 32 and cuts(64)["enc.0[:, :H]"] == (2, 256, 128)
    assert cuts(1024)["enc.2"][:2] == (2, 256) and cuts(1024)["weight_hh"][:2] == (1, 640) and cuts(1024)["weight_ih[:, H:]"] == (1, 640, 2048)
    assert cuts(1040)["prior.2"][:2] == (2, 256) and 1040 * 1040 > bo.GRID_ELEMENTS
    # a size case reaches the batched GEMM's LDS path with N = Z (EL / QL): Z a multiple of 128, full tiles and a tail
    assert any(c[7] % 128 == 0 and c[0] % 256 == 0 and c[3] * c[4] > 144 and all((c[3] * c[4]) % h for h in bo.LDS_HEIGHTS) for c in bo.SIZE_CASES)


def test_want_cut_covers_the_rows():
    for M in (1, 128, 129, 255, 256, 257, 272, 544, 1056, 2112, bo.TRAINING_ROWS, 2 * bo.TRAINING_ROWS):
        for N, K in ((16, 16), (64, 64), (1024, 80), (3072, 1024), (1040, 1040)):
            chunks, rows = bo.want_cut(M, N, K)
            assert rows % bo.BLOCK == 0 and (chunks - 1) * rows < M <= chunks * rows
            assert bo.ws_floats(M, N, K) == (chunks * N * K if chunks > 1 else 0)


def test_chunk_sums_fit_the_workspace():
    """carve_backward's comment: chunks * N K <= 512 * 4096 + N K <= the floats of b.wg.  Every weight shape of every size of the tables
    (and of the row cases), every M from 1 to the stacked rows of a training batch."""
    M = np.arange(1, 2 * bo.TRAINING_ROWS + 1, dtype=np.int64)
    ceil = lambda a, b: -(-a // b)
    sizes = set(bo.SIZES) | set(bo.REFUSED_SIZES) | {(c[0], bo.z_of(c)) for c in bo.ROW_CASES + bo.CASES}
    worst = 0.0
    for H, Z in sorted(sizes):
        have = bo.wg_floats(H)
        for N, K in sorted({(N, K) for _, _, N, K, _ in bo.weight_grads(H, Z, 1, 1, 2)[0]}):
            tiles = ceil(N, bo.TILE) * ceil(K, bo.TILE)
            want = np.maximum(1, np.minimum(ceil(bo.TARGET, tiles), ceil(M, bo.MIN_CHUNK)))
            rows = ceil(ceil(M, want), bo.BLOCK) * bo.BLOCK
            chunks = ceil(M, rows)
            for m in (1, 257, 1056, bo.TRAINING_ROWS, 2 * bo.TRAINING_ROWS):          # the vector form is want_cut's
                assert (int(chunks[m - 1]), int(rows[m - 1])) == bo.want_cut(m, N, K)
            need = np.where(chunks > 1, chunks * N * K, 0)
            assert int(need.max()) <= 512 * 4096 + N * K <= have, (H, Z, N, K, int(need.max()), have)
            worst = max(worst, float(need.max()) / have)
    print(f"WORKSPACE largest share of b.wg used by one gradient's chunk sums: {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("table", [t for _, t in NEW_TABLES], ids=[n for n, _ in NEW_TABLES])
def test_new_cases_find_their_seeds(table):
    """Searched, never skipped, within the 200 seeds and at the margins of the old cases; the search takes no gradient."""
    before = bo.SEARCHED["gradients"]
    for case in table:
        s = bo.find_seed(case, state_dict(case))
        assert s["margins"][0] >= bo.ROUND_MARGIN and s["margins"][1] >= bo.CLIP_MARGIN and 1 <= s["tried"] <= 200
        act = torch.arange(bo.z_of(case))[None, None, :] < s["bits"][:, :, None]
        print(f"SEED {bo.case_id(case)}: seed {s['seed']} ({s['tried']} tried), {int(act.sum())} active bits, margins {s['margins'][0]:.2e} {s['margins'][1]:.2e}")
        use = s["r"] < s["p_use_gen"]
        assert case[5] != 2 or case[4] < 7 or (bool(use.any()) and not bool(use.all()))       # mode 2: frames conditioned on both chains
    assert bo.SEARCHED["gradients"] == before


def test_every_clipped_branch_occurs_under_an_active_bit():
    """code_bwd_kernel has a formula of its own where e, 1 - e, prior or 1 - prior is below 1e-3.  Among the active bits of the
    saturated cases each of the four occurs (and, counted apart, among those of the wide size cases); all keep CLIP_MARGIN."""
    for name, table in (("saturated", bo.SATURATED_CASES), ("sizes, wide", tuple(c for c in bo.SIZE_CASES if c[1] == "wide"))):
        count = np.zeros(4, dtype=np.int64)
        for case in table:
            s = bo.find_seed(case, state_dict(case))
            act = torch.arange(bo.z_of(case))[None, None, :] < s["bits"][:, :, None]
            e, q = s["f64"]["prob"][act], s["f64"]["prior"][act]
            for i, v in enumerate((e, 1 - e, q, 1 - q)):
                count[i] += int((v < bo.CLIP).sum())
                assert float((v - bo.CLIP).abs().min()) >= bo.CLIP_MARGIN
            if name == "saturated":
                assert all(int((v < bo.CLIP).sum()) > 0 for v in (e, 1 - e)) or case[6] != "random", bo.case_id(case)
        print(f"CLIPPED {name}: e {count[0]}, 1 - e {count[1]}, prior {count[2]}, 1 - prior {count[3]} active bits below 1e-3")
        assert (count > 0).all(), (name, count)
    assert any(c[0] == 1024 for c in bo.SATURATED_CASES) and sum(c[0] == 64 for c in bo.SATURATED_CASES) >= 2
