"""Rate conversion at the session boundary, the host side: the output counts E(N), the filter's geometry and taps, the order of the
chunked sum (numpy float64 emulation of the kernel's walk), the finish plan, the s16 formulas and the refusals that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from resample_cases import ChunkedWalk, offline_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 22050
RATES = (8000, 16000, 24000, 32000, 44100, 48000)
PAIRS = [(r, FS) for r in RATES] + [(FS, r) for r in RATES]          # (rate_in, rate_out)
NEW_SYMBOLS = ("bvc_resampler_create", "bvc_resampler_destroy", "bvc_resampler_open", "bvc_resampler_close", "bvc_resampler_push",
               "bvc_resampler_flush", "bvc_resampler_count", "bvc_resampler_lag", "bvc_resampler_end", "bvc_resampler_set_taps",
               "bvc_resampler_taps")


def geometry(rate_in, rate_out):
    from bvcodec import preprocess
    return preprocess.design(rate_out, rate_in)                       # up, down, taps, n_pre_remove


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_counts_equal_brute_force(rate_in, rate_out):
    """E(N) for every N in 0 .. 3000 against counting the outputs m whose newest input floor((m + lag) down / up) has arrived; the counts
    of 20 ms pushes and the flush sum to ceil(N up / down), the length of the offline call."""
    from bvcodec.streaming import resampler_count
    up, down, _, lag = geometry(rate_in, rate_out)
    m = np.arange(0, 3000 * up // down + 64, dtype=np.int64)
    newest = (m + lag) * down // up                                   # ascending in m
    for N in range(0, 3001):
        assert resampler_count(rate_in, rate_out, N) == int(np.searchsorted(newest, N - 1, side="right")), N
    hop = rate_in // 50
    for pushes in (1, 2, 7, 50):
        N = pushes * hop
        per_push = [resampler_count(rate_in, rate_out, (p + 1) * hop) - resampler_count(rate_in, rate_out, p * hop) for p in range(pushes)]
        assert all(c >= 0 for c in per_push)
        flush = -(-N * up // down) - resampler_count(rate_in, rate_out, N)
        assert 0 <= flush <= lag and sum(per_push) + flush == -(-N * up // down)
    assert resampler_count(rate_in, rate_out, 2 ** 40) == -(-2 ** 40 * up // down) - lag        # 64-bit arithmetic
    with pytest.raises(ValueError):
        resampler_count(0, rate_out, 5)
    with pytest.raises(ValueError):
        resampler_count(rate_in, rate_out, -1)


@pytest.mark.parametrize("rate_in,rate_out", PAIRS + [(FS, FS)])
def test_lag_history_and_taps_equal_the_numpy_design(rate_in, rate_out):
    """bvc_resampler_lag gives preprocess.design's n_pre_remove and ceil(ntaps / up); the library's own taps are that design's within a few
    units in the last place of taps of size <= 1 (test_resample_cases_cpu.py holds them to equality at the rates it adds: both designs
    call the C library's exp and sin)."""
    from bvcodec import _abi
    from bvcodec.streaming import resampler_lag
    up, down, taps, lag = geometry(rate_in, rate_out)
    assert resampler_lag(rate_in, rate_out) == (lag, -(-len(taps) // up))
    lib = _abi.load()
    n = lib.bvc_resampler_taps(rate_in, rate_out, None, 0)
    assert n == len(taps)
    buf = (ctypes.c_double * n)()
    assert lib.bvc_resampler_taps(rate_in, rate_out, buf, n) == n
    got = np.frombuffer(buf, dtype=np.float64)
    if up == down:
        assert got.sum() == 1.0 and got[lag * down] == 1.0             # the unit impulse: resample_poly copies there
        return
    err = float(np.abs(got - taps).max())
    print(f"taps {rate_in} -> {rate_out}: {n} taps, max |C - numpy| = {err:.3e}, {int((got != taps).sum())} differ")
    assert err <= 8 * np.finfo(np.float64).eps * float(np.abs(taps).max())
    assert np.array_equal(got[:np.flatnonzero(taps)[0]], np.zeros(np.flatnonzero(taps)[0]))     # n_pre_pad zeros in front


def test_lag_of_the_usual_rates():
    from bvcodec.streaming import resampler_lag
    assert resampler_lag(16000, FS)[0] == 14 and resampler_lag(48000, FS)[0] == 11              # the send side's extra delay
    assert [resampler_lag(r, FS)[0] for r in RATES] == [28, 14, 11, 11, 11, 11]
    assert [resampler_lag(FS, r)[0] for r in RATES] == [11, 11, 11, 15, 21, 22]                 # the receive side's unflushed tail
    with pytest.raises(ValueError):
        resampler_lag(-8000, FS)


# ---------------------------------------------------------------------------------------------- the order of the sum
# (offline_walk and ChunkedWalk, the two kernels' walks in numpy float64, are resample_cases.py's)
@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_chunked_sum_equals_offline_sum(rate_in, rate_out):
    """Ragged chunks (1, 7, a hop, three hops and 5 samples) with a reset in the middle: every stream's chunked outputs are the offline
    walk's on its own signal with np.array_equal - the prefix E(N) before the flush, all of them after it - and the offline walk is
    scipy.signal.resample_poly to 1e-12."""
    import scipy.signal as ss
    hop = rate_in // 50
    chunks = [1, 7, hop, 3 * hop + 5]
    rng = np.random.default_rng(rate_in + 7 * rate_out)
    up, down, h, lag = geometry(rate_in, rate_out)
    w = ChunkedWalk(rate_in, rate_out)
    for order in (chunks, chunks[::-1]):                              # the second stream follows a reset of the same row
        x = rng.standard_normal(sum(order))
        ref = offline_walk(x, up, down, h, lag)
        assert np.abs(ref - ss.resample_poly(x, rate_out, rate_in)).max() < 1e-12
        w.reset()
        got, at = [], 0
        for n in order:
            got += w.push(x[at:at + n])
            at += n
            assert len(got) == w.E(at)
        assert np.array_equal(np.array(got), ref[:len(got)])
        got += w.flush()
        assert np.array_equal(np.array(got), ref)


# ---------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("fs", RATES)
def test_client_finish_plan(fs):
    """n_last in {0, 1, hop - 1, hop} after three whole pushes, and the stream lengths at which the flushed tail - the internal samples
    from the last push's start to the end of S - is exactly hop22 and hop22 + 1 long: the first fits its push, the second spills."""
    from bvcodec.streaming import client_finish_plan, resampler_lag
    hop = fs // 50
    hop22, lag = hop * FS // fs, resampler_lag(fs, FS)[0]
    assert hop22 == 441

    def brute(n):
        len_s = lag + math.ceil(n * FS / fs)
        last = max(0, math.ceil(n / hop) - 1)
        tail = len_s - last * hop22
        return len_s, last, tail

    for n_last in (0, 1, hop - 1, hop):
        n = 3 * hop + n_last
        len_s, push, n22 = client_finish_plan(n, hop, fs)
        assert len_s == lag + -(-n * FS // fs)
        assert 0 <= n22 <= hop22 and push * hop22 + n22 == len_s      # what the session's finish is handed, and when
        if n_last in (0, hop):                                        # a whole number of hops: the tail is the lag, one push later
            assert (push, n22) == (n // hop, lag)
        else:
            assert push == 3 + (1 if brute(n)[2] > hop22 else 0)
    seen = set()
    for n in range(3 * hop + 1, 4 * hop + 1):
        len_s, last, tail = brute(n)
        plan = client_finish_plan(n, hop, fs)
        if tail == hop22:
            assert plan == (len_s, last, hop22)
            seen.add("fits")
        elif tail == hop22 + 1:
            assert plan == (len_s, last + 1, 1)
            seen.add("spills")
        assert plan[1] * hop22 + plan[2] == len_s and plan[1] == last + (1 if tail > hop22 else 0)      # on both sides of the boundary
    if fs > FS:                                                       # a client sample is less than an internal one: no length is skipped
        assert seen == {"fits", "spills"}
    else:                                                             # (8 and 16 kHz step over some lengths; both are hit at 16 kHz)
        assert seen <= {"fits", "spills"}
    with pytest.raises(ValueError):
        client_finish_plan(100, 480, 48000)                           # 220.5 internal samples per hop


# ---------------------------------------------------------------------------------------------- s16
def test_s16_formulas():
    """in: x / 32768, exact; out: clamp(rint(y * 32768), -32768, 32767) with ties to even, NaN -> 0."""
    from bvcodec.streaming import pcm_f32_to_s16, pcm_s16_to_f32
    y = torch.tensor([-1.0, -0.5 / 32768, 0.5 / 32768, 1.5 / 32768, 1 - 2.0 ** -16, 1.0, 1.5, float("nan"), -1.5, float("inf"), float("-inf")])
    want = torch.tensor([-32768, 0, 0, 2, 32767, 32767, 32767, 0, -32768, 32767, -32768], dtype=torch.int16)
    got = pcm_f32_to_s16(y)
    assert got.dtype == torch.int16 and torch.equal(got, want)
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    f = pcm_s16_to_f32(every)
    assert f.dtype == torch.float32 and torch.equal(f.double() * 32768, every.double())          # exact
    assert torch.equal(pcm_f32_to_s16(f), every)


# ---------------------------------------------------------------------------------------------- refusals, ABI
def test_refusals_need_no_device(tmp_path, conf_var):
    from bvcodec import BVRNNCodecModel, config, synth
    from bvcodec.streaming import StreamingCodec, client_hop
    p1, p2 = synth.write_checkpoints(conf_var, str(tmp_path), seed=7)
    m = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2)
    with pytest.raises(ValueError, match=r"480.*220\.5|220\.5.*480"):
        StreamingCodec(m, 2, 3000, hop=480, client_rate=48000)
    for bad_rate in (0, -16000, 16000.5):
        with pytest.raises(ValueError, match="client_rate"):
            StreamingCodec(m, 2, 3000, hop=320, client_rate=bad_rate)
    for fmt in ("s24", "f64", None):
        with pytest.raises(ValueError, match="sample_format"):
            StreamingCodec(m, 2, 3000, hop=320, client_rate=16000, sample_format=fmt)
    for fs in RATES:                                                  # twenty-millisecond hops of the six usual rates pass
        assert client_hop(fs // 50, fs) == 441


def test_abi_has_the_resampler():
    from bvcodec import _abi
    hdr = open(os.path.join(ROOT, "include", "bvcodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(bvc_[a-z_0-9]+)\s*\(", hdr))
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"BVC_PCM_F32\s*=\s*0\s*,\s*BVC_PCM_S16\s*=\s*1", hdr)
    assert lib.bvc_abi_version() == 3
    r = ctypes.c_void_p()
    assert lib.bvc_resampler_create(2, 0, FS, 441, 0, 0, ctypes.byref(r)) == -1 and not r.value    # rates <= 0: BVC_EINVAL before any device
    assert lib.bvc_resampler_create(2, 16000, FS, 441, 2, 0, ctypes.byref(r)) == -1 and not r.value
