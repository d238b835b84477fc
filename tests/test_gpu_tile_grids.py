"""Every compiled tile height of the batched GEMM (BVC_GEMM_BM) and of the offline C = 64 AMP pair (BVC_AMP64_TR) gives the
bits of the cuts of before the plan (BVC_TILE_CUT=legacy: 128-row tiles plus a tail launch; one AMP tile shape), and the
default path is the planned one.  The switches are read at every launch, so one process runs them all.
Needs the MI355X: run with ``-m gpu``."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEMM_HEIGHTS = (144, 128, 112)
AMP64_HEIGHTS = (128, 112, 96, 80)
SWITCHES = ("BVC_TILE_CUT", "BVC_GEMM_BM", "BVC_AMP64_TR")


@contextlib.contextmanager
def switches(**env):
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def cut(lib, kind, rows=0, column_blocks=0, ks=0, mode=0):
    from bvcodec import _abi
    out = (ctypes.c_int64 * 6)()
    _abi.check(lib.bvc_test_tile_plan(kind, rows, column_blocks, ks, mode, out))
    return list(out)


@pytest.fixture(scope="module")
def lib():
    from bvcodec import _abi
    return _abi.load()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("N,K", [(1024, 1024), (3072, 1024)])
@pytest.mark.parametrize("M", [27520, 11129, 300, 5])
def test_every_gemm_height_gives_the_bits_of_the_two_launch_cut(lib, M, N, K, act):
    from bvcodec import _abi
    g = torch.Generator().manual_seed(3 * M + N + act)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    st = _abi.current_stream(torch.device(DEV))

    def run(**env):
        y = torch.full((M, N), float("nan"), device=DEV)
        with switches(**env):
            _abi.check(lib.bvc_test_linear_batched(_abi.ptr(x), _abi.ptr(w), _abi.ptr(b), M, N, K, act, _abi.ptr(y), st))
            torch.cuda.synchronize()
        return y, cut(lib, 0, mode=-1)

    ref, used = run(BVC_TILE_CUT="legacy")
    assert used == cut(lib, 0, M, N // 128, mode=1) and used[0] == 128
    assert not torch.isnan(ref).any()
    y, used = run()
    assert used == cut(lib, 0, M, N // 128), used                     # the default path is the planned one
    assert torch.equal(y, ref), (y - ref).abs().max().item()
    for h in GEMM_HEIGHTS:
        y, used = run(BVC_GEMM_BM=str(h))
        assert used[0] == h and used[2] == 0, used                     # one launch of that height
        assert torch.equal(y, ref), (h, (y - ref).abs().max().item())


@pytest.mark.parametrize("B,seconds", [(5, 1.0), (64, 5.0)])
def test_every_tile_height_gives_the_same_codes_and_waveform(lib, B, seconds):
    from gpu_common import make_model
    from bvcodec import synth
    model = make_model(True, 1024)[0]
    x = synth.synthetic_speech(B, int(22050 * seconds), seed=11, kind="speech").to(DEV)

    def run(**env):
        with switches(**env):
            codes = model.encode(x, 3000)
            wav = model.decode(codes, x.shape[1])
            torch.cuda.synchronize()
        return codes.clone(), wav.clone()

    ref_codes, ref_wav = run(BVC_TILE_CUT="legacy")
    assert cut(lib, 0, mode=-1)[0] == 128 and cut(lib, 1, mode=-1)[0] == 128
    forced = [{}] + [{"BVC_GEMM_BM": str(h)} for h in GEMM_HEIGHTS] + [{"BVC_AMP64_TR": str(h)} for h in AMP64_HEIGHTS]
    for env in forced:
        codes, wav = run(**env)
        if "BVC_GEMM_BM" in env:
            assert cut(lib, 0, mode=-1)[0] == int(env["BVC_GEMM_BM"])
        if "BVC_AMP64_TR" in env:
            assert cut(lib, 1, mode=-1)[0] == int(env["BVC_AMP64_TR"])
        assert torch.equal(codes, ref_codes), (env, int((codes != ref_codes).sum()))
        assert torch.equal(wav, ref_wav), (env, (wav - ref_wav).abs().max().item())


def test_default_path_is_the_planned_one(lib):
    """At the benchmark shape the default GEMM launch is ONE launch of 144-row tiles on whole rounds, and the C = 64 AMP pair
    runs the height the plan gives for its last launch - read back from the launch code, so that the switch cannot silently
    stay on the cuts of before."""
    from gpu_common import make_model
    from bvcodec import synth
    model = make_model(True, 1024)[0]
    x = synth.synthetic_speech(64, 110250, seed=0, kind="noise").to(DEV)
    with switches():
        wav = model.decode(model.encode(x, 3000), x.shape[1])
        torch.cuda.synchronize()
    assert torch.isfinite(wav).all()
    gemm, amp = cut(lib, 0, mode=-1), cut(lib, 1, mode=-1)
    assert gemm[0] == 144 and gemm[2] == 0 and gemm[3] % 512 == 0, gemm          # one launch, whole rounds of the 512 slots
    tiles_per_item = amp[3] // 64
    # the last C = 64 launch of decode(): recover its ks from nothing but the plan - one of the three must reproduce it
    L = 8 * 431
    assert any(cut(lib, 1, L, 64, ks)[0] == amp[0] and cut(lib, 1, L, 64, ks)[3] == amp[3] for ks in (3, 7, 11)), (amp, tiles_per_item)
    assert any(cut(lib, 1, L, 64, ks)[0] != 128 for ks in (3, 7, 11))            # the plan moves at least one of them
