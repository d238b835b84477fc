"""What must hold without a device before the resamplers are compared with float64 (tests/test_gpu_resample.py): the pinned geometry of
the twenty rate pairs, the float64 walk rounded to float32 inside the bar against scipy at every case of the table, the closed form of
an impulse, the delayed form of the chunked walk, the library's own taps at the added rates, the refusal past the LDS limit and the
s16 formulas on the s16 case list."""
import ctypes

import numpy as np
import pytest
import torch

import resample_cases as rc


# ---------------------------------------------------------------------------------------------- geometry
def test_the_table_has_the_twenty_pairs():
    assert len(rc.PAIRS) == 20 and set(rc.GEOMETRY) == set(rc.PAIRS) and set(rc.USUAL_PAIRS) < set(rc.PAIRS)


@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_geometry_pins(rate_in, rate_out):
    from bvcodec import preprocess
    from bvcodec.streaming import resampler_lag
    up, down, h, lag = preprocess.design(rate_out, rate_in)
    H = -(-len(h) // up)
    assert rc.GEOMETRY[rate_in, rate_out] == (up, down, len(h), H, lag)
    assert resampler_lag(rate_in, rate_out) == (lag, H)
    assert rc.history(rate_in, rate_out) == H and {1, 2, H - 1, H, H + 1, 3000} <= set(rc.lengths(rate_in, rate_out))
    whole = [L for L in rc.lengths(rate_in, rate_out) if L * up % down == 0 and L > H + 1]
    assert whole and whole[0] + 1 in rc.lengths(rate_in, rate_out)


@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_zero_extension_is_never_taken(rate_in, rate_out):
    """preprocess.resample_poly appends zeros to the taps where need = (n_out + lag - 1) down - (L - 1) up + 1 exceeds len(h) (scipy's
    n_post_pad loop).  With r = n_out down - L up in [0, down) and lag down = half_len + n_pre_pad, need - len(h) is
    r + up - down - half_len <= up - 1 - 10 max(up, down) < 0: no length reaches that branch with the designed taps, so no case of the
    table can be one that takes it.  Checked for every length up to 3001 and at the grid cases' lengths."""
    up, down, h, lag = rc.geometry(rate_in, rate_out)
    half_len = 10 * max(up, down)
    for L in list(range(1, 3002)) + [g[3] for g in rc.GRID_CASES]:
        d = rc.zero_extension(rate_in, rate_out, L)
        r = rc.out_len(L, up, down) * down - L * up
        assert 0 <= r < down and d == r + up - down - half_len and d < 0, L


def test_grid_cases_take_a_second_trip():
    for rate_in, rate_out, B, L in rc.GRID_CASES:
        up, down, _, _ = rc.geometry(rate_in, rate_out)
        assert rc.GRID_OUTPUTS < rc.out_len(L, up, down) < 2 * rc.GRID_OUTPUTS and B == 2
    assert rc.out_len(1150000, 147, 320) == 528282


# ---------------------------------------------------------------------------------------------- the reference inside its own bar
@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_float64_walk_is_within_the_bar_of_scipy(rate_in, rate_out):
    """Every case of the table: float32 of the float64 walk against scipy under the bar the GPU is held to, the impulses' closed form
    with equality, and what the scaled and the Nyquist inputs are there for."""
    up, down, h, lag = rc.geometry(rate_in, rate_out)
    H = rc.history(rate_in, rate_out)
    failures, worst, seen = [], 0.0, 0
    for L in rc.lengths(rate_in, rate_out):
        blk = rc.block(rate_in, rate_out, L)
        assert list(blk) == list(rc.KINDS)
        for kind, (x, ref) in blk.items():
            seen += 1
            assert x.dtype == torch.float32 and ref.ref.shape == (x.shape[0], rc.out_len(L, up, down)) and np.isfinite(ref.ref).all()
            w = rc.walk(x.numpy(), up, down, h, lag)
            v = rc.compare(w.astype(np.float32), ref, f"{rate_in}->{rate_out} L {L} {kind}")
            worst = max(worst, v.ratio)
            if not v.ok:
                failures.append(v.message)
            if kind in rc.IMPULSES:
                want = rc.impulse_expected(rate_in, rate_out, L, rc.impulse_at(kind, L, H))
                assert np.array_equal(w.astype(np.float32), np.tile(want, (x.shape[0], 1))), (L, kind)
                assert np.count_nonzero(want) > 0 or L * up < down
            if kind == "zeros":
                assert not w.any() and not ref.ref.any()
            if kind in ("big", "small"):                             # the scale commutes with every rounding: nothing under- or overflows
                mag = np.abs(ref.ref[ref.ref != 0])
                assert mag.size and mag.min() >= 2 * rc.TINY and mag.max() < 2.0 ** 120, (L, kind, mag.min())
                scale = np.float32(rc.BIG if kind == "big" else rc.SMALL)
                assert np.array_equal(rc.make_input("noise", x.shape[0], L, H, seed=rate_in + rate_out).numpy() * scale, x.numpy())
    x, ref = rc.block(rate_in, rate_out, 3000)["nyquist"]
    if rate_out < rate_in:                 # the input's Nyquist is above the cut-off: attenuated, to nothing from a ratio of 4 : 3 on
        assert np.abs(ref.ref[:, 200:-200]).max() < (0.05 if 3 * rate_in >= 4 * rate_out else 1.0)
    else:                      # at the cut-off, where the tone and its image coincide: the two halves add up to (about) the tone
        assert 0.9 < np.abs(ref.ref[:, 200:-200]).max() < 1.1
    x, ref = rc.block(rate_in, rate_out, 3000)["dc"]
    assert np.abs(ref.ref[:, 200:-200] - 1.0).max() < 1e-3
    print(f"walk {rate_in} -> {rate_out}: {seen} cases, largest |float32(walk) - scipy| / bar = {worst:.3f}")
    assert not failures, "\n".join(failures[:12])


@pytest.mark.parametrize("rate_in,rate_out", [(8000, rc.FS), (rc.FS, 48000), (22051, rc.FS)])
def test_vector_walk_is_the_scalar_walk(rate_in, rate_out):
    up, down, h, lag = rc.geometry(rate_in, rate_out)
    H = rc.history(rate_in, rate_out)
    for L in (1, H, 2 * H + 5):
        x = rc.make_input("noise", 2, L, H, seed=1).numpy().astype(np.float64)
        w = rc.walk(x, up, down, h, lag)
        assert np.array_equal(w[0], rc.offline_walk(x[0], up, down, h, lag)) and np.array_equal(w[1], rc.offline_walk(x[1], up, down, h, lag))


@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_delayed_chunked_walk(rate_in, rate_out):
    """The delayed form: lag zeros in front, ceil(N up / down) samples after N inputs, the last lag of them in the flush - and behind
    the zeros the offline walk with np.array_equal; a stream shorter than the history, and one of no samples, too."""
    up, down, h, lag = rc.geometry(rate_in, rate_out)
    hop = rate_in // 50
    rng = np.random.default_rng(rate_in + 3 * rate_out)
    w = rc.ChunkedWalk(rate_in, rate_out, delayed=True)
    for chunks in ([1, 7, hop, hop + 5], [3], []):
        x = rng.standard_normal(sum(chunks))
        w.reset()
        got, at = [], 0
        for n in chunks:
            got += w.push(x[at:at + n])
            at += n
            assert len(got) == rc.out_len(at, up, down)
        tail = w.flush()
        assert len(tail) == lag
        got = np.array(got + tail)
        assert not got[:lag].any() and np.array_equal(got[lag:], rc.offline_walk(x, up, down, h, lag))


# ---------------------------------------------------------------------------------------------- the library's host side
@pytest.mark.parametrize("rate_in,rate_out", [p for p in rc.PAIRS if p not in rc.USUAL_PAIRS])
def test_library_taps_equal_the_design_at_the_added_rates(rate_in, rate_out):
    """bvc_resampler_taps (host only) against preprocess.design, bit for bit.  Both call the C library's exp and sin (numpy's own exp
    is a vector kernel on AVX-512 hosts, one unit in the last place off on 4 to 5 % of the window's arguments) and both add the
    window up as numpy does, 8192 elements at a time: the taps of 22051 <-> 22050 and 96000 <-> 22050 have more."""
    from bvcodec import _abi
    up, down, taps, lag = rc.geometry(rate_in, rate_out)
    lib = _abi.load()
    n = lib.bvc_resampler_taps(rate_in, rate_out, None, 0)
    assert n == len(taps)
    buf = (ctypes.c_double * n)()
    assert lib.bvc_resampler_taps(rate_in, rate_out, buf, n) == n
    got = np.frombuffer(buf, dtype=np.float64)
    differ = int((got != taps).sum())
    print(f"taps {rate_in} -> {rate_out}: {n} taps, {differ} differ, max |C - numpy| = {np.abs(got - taps).max():.3e}")
    assert np.array_equal(got, taps)


@pytest.mark.parametrize("rate_in,rate_out", [(48000, rc.FS), (rc.FS, 48000), (96000, rc.FS)])
def test_create_refuses_past_the_lds_limit(rate_in, rate_out):
    """H + max_in = 16385 floats do not fit the 64 KiB a push stages them in: BVC_EINVAL, in front of the device check."""
    from bvcodec import _abi
    lib = _abi.load()
    r = ctypes.c_void_p()
    over = rc.LDS_FLOATS - rc.history(rate_in, rate_out) + 1
    assert lib.bvc_resampler_create(2, rate_in, rate_out, over, 0, 0, ctypes.byref(r)) == -1 and not r.value
    assert b"64 KiB" in lib.bvc_last_error()


# ---------------------------------------------------------------------------------------------- s16
def test_s16_formulas_on_the_case_list():
    from bvcodec.streaming import pcm_f32_to_s16, pcm_s16_to_f32
    y = torch.tensor([p[0] for p in rc.S16_POINTS], dtype=torch.float32)
    want = torch.tensor([p[1] for p in rc.S16_POINTS], dtype=torch.int16)
    got = pcm_f32_to_s16(y)
    assert got.dtype == torch.int16 and torch.equal(got, want)
    kinds = {"tie": 0.5 / 32768, "full+": 1.0, "full-": -1.0, "over+": 1.5, "over-": -1.5}
    assert all(any(p[0] == v for p in rc.S16_POINTS) for v in kinds.values())
    assert {32767, -32768, 0} <= {p[1] for p in rc.S16_POINTS}
    finite = torch.isfinite(y)
    exact = rc.s16_expected(y[finite].double().numpy())               # within half a step of the clamped float64 value, none wraps
    assert np.abs(got[finite].double().numpy() - exact).max() <= 0.5
    sq = rc.square(3, 64, seed=1)
    assert set(np.unique(sq.numpy())) == {-1.0, 1.0} and not torch.equal(sq[0], sq[1])
    q = pcm_f32_to_s16(sq)
    assert set(np.unique(q.numpy())) == {-32768, 32767}
    for rate_in, rate_out in rc.S16_PAIRS:                            # the filter's overshoot on them is above full scale
        L = 4 * (rate_in // 50) + 17
        assert np.abs(rc.reference(pcm_s16_to_f32(pcm_f32_to_s16(rc.square(3, L, seed=rate_in % 7))).numpy(), rate_in, rate_out).ref).max(axis=1).min() > 1.05
    back = pcm_s16_to_f32(q)
    assert back.dtype == torch.float32 and torch.equal(back.double() * 32768, q.double()) and torch.equal(pcm_f32_to_s16(back), q)
