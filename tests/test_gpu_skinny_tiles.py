"""The row-tile variants of the recurrent-layer kernel alone (csrc/k_gemm.hip: SK_LIN2 / SK_LIN4, BVC_MTW=2|4, and the multi-frame twin
of every linear kernel), through bvc_test_linear_tiles: the same bits as one row tile per workgroup, as bvc_test_linear and as the
batched GEMM, at the shapes where the tile walk has an edge - a last group of row tiles with 1 or 3 tiles missing, a last tile of one
row, column tiles that are no multiple of the 8 per round, waves without a k-block, the unrolled loop against its remainder loop.
One row tile per workgroup is held to float64 at the project's bar (vocoder_layers.compare; measured ratios in
profiles/skinny_tiles_parity.md), and the launch counts prove that the kernel a case is written for is the one that ran.
BVC_LATENCY=1 and the variants inside the model: tests/test_gpu_mtw_model.py.  Needs the MI355X: run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import skinny_kernels as sk
from gpu_common import DEV

pytestmark = pytest.mark.gpu

# rows -> row tiles, and the kernel a request of 1 / 2 / 4 row tiles per workgroup has to run there, written out (not computed from the
# rule: a case that the clamp sends to another kernel than the one listed fails)
LIN, LIN2, LIN4 = sk.SK_LIN, sk.SK_LIN2, sk.SK_LIN4
WANT = {1: (1, (LIN, LIN, LIN)), 5: (1, (LIN, LIN, LIN)), 16: (1, (LIN, LIN, LIN)), 17: (2, (LIN, LIN2, LIN2)), 33: (3, (LIN, LIN2, LIN2)),
        48: (3, (LIN, LIN2, LIN2)), 49: (4, (LIN, LIN2, LIN4)), 65: (5, (LIN, LIN2, LIN4)), 130: (9, (LIN, LIN2, LIN4))}
MTWS = (1, 2, 4)
ROWS = (1, 16, 17, 33, 48, 49, 65, 130)
COLS = (16, 80, 144, 1024)                       # 1, 5, 9 and 64 column tiles against the rounds of 8
DEPTHS = (16, 80, 1024, 1152, 2048)              # 1, 5, 64, 72, 128 k-blocks over 8 waves: empty waves; remainder loop only (SK_LIN2's U = 8);
                                                 # one trip of U = 8; one trip and a remainder; several trips
# every M (so every (M, mtw) pair: a case runs all three mtw) at 9 column tiles and a trip plus a remainder; every (N, K) pair at five row
# tiles (the last group of 4 lacks 3 tiles, the last group of 2 lacks 1, the last tile holds one row); the largest operand on 3 and 9 tiles
CASES = tuple(sorted({(M, 144, 1152) for M in ROWS} | {(65, N, K) for N in COLS for K in DEPTHS}
                     | {(130, 1024, 2048), (33, 1024, 2048), (1, 16, 16), (17, 16, 16), (49, 80, 2048), (130, 16, 80)}))
CANARY_ROWS, CANARY = 16, 777.0
LEDGER = bd.Ledger("skinny tiles")


@pytest.fixture(scope="module")
def lib():
    from bvcodec import _abi
    return _abi.load()


def stream():
    from bvcodec import _abi
    return _abi.current_stream(torch.device(DEV))


def out_buffer(rows, N, frames=1):
    """(frames * rows + CANARY_ROWS, N): NaN where the launch has to write, the canary value in the rows behind."""
    buf = torch.full((frames * rows + CANARY_ROWS, N), float("nan"), device=DEV)
    buf[frames * rows:] = CANARY
    return buf


def written(buf, rows, N, frames=1):
    """The launch's output, after the checks every output gets: all of it written, nothing behind it."""
    torch.cuda.synchronize()
    y = buf[:frames * rows]
    assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} elements not written (or not finite)"
    assert bool((buf[frames * rows:] == CANARY).all()), "rows behind the output were written"
    return y.view(frames, rows, N) if frames > 1 else y


def tiles(lib, x, w, b, M, N, K, act, mtw, frames=1):
    from bvcodec import _abi
    buf = out_buffer(M, N, frames)
    _abi.check(lib.bvc_test_linear_tiles(_abi.ptr(x), _abi.ptr(w), _abi.ptr(b), M, N, K, act, mtw, frames, _abi.ptr(buf), stream()))
    return written(buf, M, N, frames)


def plain(lib, fn, x, w, b, M, N, K, act):
    from bvcodec import _abi
    buf = out_buffer(M, N)
    _abi.check(fn(_abi.ptr(x), _abi.ptr(w), _abi.ptr(b), M, N, K, act, _abi.ptr(buf), stream()))
    return written(buf, M, N)


def draw(M, N, K, seed, gain=1.0, frames=1):
    """N(0, 1) inputs, weights over sqrt(K) (as tests/test_gpu_parity.py), weight and bias times `gain`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames * M, K, generator=g)
    w = gain * torch.randn(N, K, generator=g) / np.sqrt(K)
    b = gain * torch.randn(N, generator=g)
    return x, w, b


def one_launch(lib, kernel, multi_frame, fn):
    """fn() must be ONE launch of the recurrent-layer kernel, and of `kernel` (its multi-frame twin if multi_frame)."""
    before = sk.counts(lib)
    out = fn()
    delta = sk.counts(lib) - before
    want = np.zeros_like(delta)
    want[1 if multi_frame else 0, kernel] = 1
    assert np.array_equal(delta, want), (f"wanted one {'multi-frame ' if multi_frame else ''}launch of {sk.NAMES[kernel]}; launched "
                                         + str({("frames " if f else "") + sk.NAMES[k]: int(delta[f, k]) for f in (0, 1) for k in range(sk.SK_COUNT) if delta[f, k]}))
    return out


def against_float64(y, x, w, b, act, what):
    ref64 = torch.nn.functional.linear(x.double(), w.double(), b.double())
    ref32 = torch.nn.functional.linear(x, w, b)
    if act:
        ref64, ref32 = torch.nn.functional.elu(ref64), torch.nn.functional.elu(ref32)
    v = bd.compare(bd.n64(y)[None], bd.n64(ref64)[None], bd.n64(ref32)[None], what)
    print(f"  ratio {v.ratio:.3f} e_hip {v.e_hip:.3e} e32 {v.e32:.3e} scale {v.scale:.3e} [{what}]", flush=True)
    LEDGER.add("elu" if act else "linear", v)
    assert v.ok, v.message


# ---------------------------------------------------------------------------------------------- 1: one frame
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "elu"])
@pytest.mark.parametrize("M,N,K", CASES)
def test_row_tile_variants_give_the_same_bits(lib, M, N, K, act):
    assert WANT[M][0] == (M + 15) // 16
    x, w, b = draw(M, N, K, 131 * M + N + K + act)
    xd, wd, bd_ = x.to(DEV), w.to(DEV), b.to(DEV)
    y = {mtw: one_launch(lib, WANT[M][1][i], False, lambda: tiles(lib, xd, wd, bd_, M, N, K, act, mtw)) for i, mtw in enumerate(MTWS)}
    against_float64(y[1], x, w, b, act, f"mtw 1 M {M} N {N} K {K} act {act}")
    for mtw in (2, 4):
        assert torch.equal(y[mtw], y[1]), (mtw, float((y[mtw] - y[1]).abs().max()))
    y_lin = one_launch(lib, LIN, False, lambda: plain(lib, lib.bvc_test_linear, xd, wd, bd_, M, N, K, act))
    y_bat = plain(lib, lib.bvc_test_linear_batched, xd, wd, bd_, M, N, K, act)
    for mtw in MTWS:
        assert torch.equal(y[mtw], y_lin) and torch.equal(y[mtw], y_bat), mtw


def test_cases_cover_the_edges():
    """What the module's docstring promises of CASES (host arithmetic; here because the cases are)."""
    assert {c[0] for c in CASES} == set(ROWS) and {c[1] for c in CASES} == set(COLS) and {c[2] for c in CASES} == set(DEPTHS)
    kernels = {(WANT[M][1][i], mtw) for M in ROWS for i, mtw in enumerate(MTWS)}
    assert kernels == {(LIN, 1), (LIN, 2), (LIN, 4), (LIN2, 2), (LIN2, 4), (LIN4, 4)}
    for M in ROWS:                                                  # WANT is the rule's answer, case by case
        assert WANT[M][1] == tuple(sk.linear_kernel(M, mtw) for mtw in MTWS), M
    t = [WANT[M][0] for M in ROWS]
    assert any(n % 4 == 1 for n in t if n > 4) and any(n % 2 == 1 for n in t if n > 2) and 130 % 16 == 2 and 65 % 16 == 1
    assert any(n // 16 % 8 for n in COLS) and any(n // 16 > 8 and n // 16 % 8 for n in COLS)
    kb = [k // 16 for k in DEPTHS]
    assert min(kb) < 8 and 64 in kb and 72 in kb and max(kb) >= 2 * 64


def test_saturated_weights_reach_the_elu_tail(lib):
    """Weights and biases of the size of the saturated draw's output layers: pre-activations far into the tail of the ELU."""
    M, N, K = 65, 144, 1152
    x, w, b = draw(M, N, K, 5, gain=bd.GAINS["saturated"][1])
    pre = torch.nn.functional.linear(x.double(), w.double(), b.double())
    assert float(pre.min()) < -25 and float(pre.max()) > 15
    xd, wd, bd_ = x.to(DEV), w.to(DEV), b.to(DEV)
    y = {mtw: one_launch(lib, WANT[M][1][i], False, lambda: tiles(lib, xd, wd, bd_, M, N, K, 1, mtw)) for i, mtw in enumerate(MTWS)}
    against_float64(y[1], x, w, b, 1, f"saturated mtw 1 M {M} N {N} K {K}")
    assert torch.equal(y[2], y[1]) and torch.equal(y[4], y[1])
    assert torch.equal(y[1], plain(lib, lib.bvc_test_linear_batched, xd, wd, bd_, M, N, K, 1))
    assert bool((y[1] >= -1).all()) and bool((y[1] == -1).any())


# ---------------------------------------------------------------------------------------------- 2: several frames in one launch
@pytest.mark.parametrize("N,K", [(144, 1152), (16, 80)])
@pytest.mark.parametrize("M", [5, 33, 65])
@pytest.mark.parametrize("frames", [2, 4])
def test_multi_frame_launch_equals_the_frames_alone(lib, frames, M, N, K):
    x, w, b = draw(M, N, K, 17 * M + N + K + frames, frames=frames)
    xd, wd, bd_ = x.to(DEV), w.to(DEV), b.to(DEV)
    alone = [tiles(lib, xd[f * M:(f + 1) * M].contiguous(), wd, bd_, M, N, K, 1, 1) for f in range(frames)]
    for i, mtw in enumerate(MTWS):
        y = one_launch(lib, WANT[M][1][i], True, lambda: tiles(lib, xd, wd, bd_, M, N, K, 1, mtw, frames))
        assert y.shape == (frames, M, N)
        for f in range(frames):
            assert torch.equal(y[f], alone[f]), (mtw, f, float((y[f] - alone[f]).abs().max()))
            one = one_launch(lib, WANT[M][1][i], False, lambda: tiles(lib, xd[f * M:(f + 1) * M].contiguous(), wd, bd_, M, N, K, 1, mtw))
            assert torch.equal(y[f], one), (mtw, f)


# ---------------------------------------------------------------------------------------------- 3: refusals
@pytest.mark.parametrize("M,N,K,frames", [(5, 24, 16, 1), (5, 16, 24, 1), (33, 1000, 1024, 2), (5, 16, 16, 0), (33, 16, 16, -3)])
def test_refusals_launch_nothing(lib, M, N, K, frames):
    from bvcodec import _abi
    rows = M * max(frames, 1)
    x, w, b = torch.zeros(rows, K, device=DEV), torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    buf = out_buffer(rows, N)
    before = sk.counts(lib)
    for mtw in MTWS:
        rc = lib.bvc_test_linear_tiles(_abi.ptr(x), _abi.ptr(w), _abi.ptr(b), M, N, K, 0, mtw, frames, _abi.ptr(buf), stream())
        assert rc == sk.BVC_EINVAL and b"bvc_test_linear_tiles" in lib.bvc_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(sk.counts(lib), before)
    assert bool(torch.isnan(buf[:rows]).all()) and bool((buf[rows:] == CANARY).all())


# ---------------------------------------------------------------------------------------------- the ledger
def test_every_variant_ran_and_parity_ledger(lib):
    """The counts of the process so far: both wider kernels and the three multi-frame twins this file is about were launched.  Prints
    the PARITY lines of the float64 comparisons (profiles/skinny_tiles_parity.md)."""
    c = sk.counts(lib)
    print({("frames " if f else "") + sk.NAMES[k]: int(c[f, k]) for f in (0, 1) for k in range(sk.SK_COUNT)}, flush=True)
    for f, k in ((0, LIN), (0, LIN2), (0, LIN4), (1, LIN), (1, LIN2), (1, LIN4)):
        assert c[f, k] > 0, (f, sk.NAMES[k])
    LEDGER.close()
