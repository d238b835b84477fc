"""What must hold on the oracle alone before the front end is compared with it (tests/test_gpu_frontend.py): the oracle equals a direct
statement of the operator at every bank and left padding used, the product's mel bank is the oracle's, each bank still has the
property it is in the list for, and no case can pass by looking at nothing.  Also the refusals of bvc_test_stft_logmel, which are
made on the host in front of everything that needs a device."""
import numpy as np
import pytest
import torch

import frontend_cases as fc


# ---------------------------------------------------------------------------------------------- the oracle
BANK_PADS = [(name, fc.BANK_PAD) for name in fc.BANKS] + [("default", p) for p in fc.PAD_LEFTS if p != fc.BANK_PAD]


@pytest.mark.parametrize("name,pad_left", BANK_PADS)
def test_oracle_equals_the_direct_statement(name, pad_left):
    """oracle.frontend.log_mel in float64 against an explicit reflect index, numpy's rfft and a dense matmul: 1e-12 relative in the
    linear domain, on noise and on tones, at lengths that reflect on both sides."""
    basis = fc.bank(name)
    lmin = fc.padding_lengths(pad_left)[0]
    for B, L, kind in ((2, lmin, "noise"), (3, lmin + 255, "tones"), (2, 2049, "noise"), (1, 2049, "tones")):
        x = fc.make_input(kind, B, L, pad_left, seed=1)
        m64 = fc.oracle_log_mel(x, pad_left, basis, torch.float64)
        lin = fc.direct_mel_linear(x, pad_left, basis)
        assert m64.shape == lin.shape == (B, fc.num_frames(L, pad_left), fc.NUM_MELS)
        want = np.maximum(lin, fc.CLAMP)
        assert np.abs(np.exp(m64) - want).max() <= 1e-12 * want.max(), (name, pad_left, L, kind)
        assert (np.abs(np.exp(m64) - want) <= 1e-12 * want + 1e-15 * want.max()).all()


def test_streaming_window_reads_no_padding():
    """The first k frames at pad_left = 0 of 256 (k - 1) + 1024 samples are the frames of the plain windows."""
    for k in fc.STREAM_KS:
        n = fc.stream_samples(k)
        i = fc.reflect_index(n, k, 0)
        assert np.array_equal(i, fc.HOP * np.arange(k)[:, None] + np.arange(fc.N_FFT)[None, :]) and i.max() == n - 1
        x, ref = fc.stream_case(k, 3, "noise")
        assert ref.m64.shape == ref.lin.shape == (3, k, fc.NUM_MELS) and bool(torch.isnan(x[:, n:]).all()) and x.shape[1] == n + fc.STREAM_TAIL
        want = np.maximum(ref.lin, fc.CLAMP)
        assert np.abs(np.exp(ref.m64) - want).max() <= 1e-12 * want.max()


# ---------------------------------------------------------------------------------------------- the banks
@pytest.mark.parametrize("name", list(fc.BANKS))
def test_product_bank_is_the_oracle_bank(name):
    from bvcodec import melbank
    fs, fmin, fmax = fc.BANKS[name]
    assert np.array_equal(melbank.slaney_mel_basis(fs, fc.N_FFT, fc.NUM_MELS, fmin, fmax), fc.bank(name))


@pytest.mark.parametrize("name", list(fc.BANKS))
def test_bank_still_exercises_what_it_is_listed_for(name):
    kmax, empty, w512 = fc.bank_tables(fc.bank(name))
    pin_kmax, pin_empty, pin_w512 = fc.BANK_PINS[name]
    assert (kmax, empty) == (pin_kmax, pin_empty)
    assert w512 == pytest.approx(pin_w512, rel=0.05) and (w512 > 0) == (pin_w512 > 0)
    if name == "default":
        assert int((fc.bank(name) != 0).sum()) == fc.NONZERO_DEFAULT
    if name == "fs44k":
        assert kmax < 3 * 64                                   # fewer than three turns of the k += 64 loop
    # a filter's weights are one run of bins: the sparse rows (mel_start, mel_len) hold no zero inside
    for row in fc.bank(name):
        nz = np.nonzero(row)[0]
        assert nz.size == 0 or nz.size == nz[-1] - nz[0] + 1


def test_tone_bins_take_every_digit():
    """Every value 0..7 of each radix-8 digit of the 512-point index, and bins 1, 255, 256, 510, 511."""
    bins = np.array(fc.TONE_BINS)
    assert {1, 255, 256, 510, 511} <= set(bins.tolist()) and bins.min() >= 0 and bins.max() < 512
    for shift in (0, 3, 6):
        assert set(((bins >> shift) & 7).tolist()) == set(range(8))


def test_shapes_reach_every_count_of_live_waves():
    assert {(B * fc.num_frames(L, fc.BANK_PAD)) % 4 for B, L in fc.BANK_SHAPES} == {0, 1, 2, 3}
    for p in fc.PAD_LEFTS:
        assert {(B * fc.num_frames(L, p)) % 4 for B, L, _ in fc.padding_cases(p)} >= {1, 2, 3}
        assert all(fc.num_frames(L, p) >= 1 for L in fc.padding_lengths(p)) and fc.num_frames(fc.padding_lengths(p)[0] - 1, p) == 0
    for B, L, p in fc.GRID_CASES:
        assert (B * fc.num_frames(L, p) + 3) // 4 > fc.GRID_LIMIT
    B, L, p = fc.GRID_CASES[2]
    assert (B * fc.num_frames(L, p) + 3) // 4 >= 2 * fc.GRID_LIMIT                     # (every workgroup takes a second turn)


def test_ragged_rows_cover_dead_and_clamped_lengths():
    x, rows = fc.ragged_case()
    assert x.shape == (len(fc.RAGGED_LENS), fc.RAGGED_L)
    assert [T for _, T, _ in rows] == [8, 8, 5, 5, 4, 3, 2, 0, 0, 0, 0, 0, 8]
    for b, (n, T, ref) in enumerate(rows):
        assert bool(torch.isnan(x[b, n:]).all()) and bool(torch.isfinite(x[b, :n]).all())
        assert (ref is None) == (T == 0) and (ref is None or ref.m64.shape == (1, T, fc.NUM_MELS))


# ---------------------------------------------------------------------------------------------- the caps
def test_no_case_passes_by_looking_at_nothing():
    """Per case, on the oracle: (1) noise and speech have at least half of their elements in the log-domain set; (2) fewer than 1 % of
    the elements are within the linear bar of the clamp, where either answer passes; (3) the tones put a filter of every non-empty
    third of the bank into the log-domain set."""
    bad, n = [], 0
    for family, label, kind, name, ref in fc.all_references():
        n += 1
        in_log, in_band = fc.conditions(ref)
        assert np.isfinite(ref.m64).all() and np.isfinite(ref.m32).all() and np.isfinite(ref.lin).all(), label
        if kind in ("noise", "speech") and in_log < 0.5:
            bad.append(f"{family} {label}: {in_log:.3f} of the elements in the log-domain set")
        if in_band >= 0.01:
            bad.append(f"{family} {label}: {in_band:.4f} of the elements within the bar of the clamp")
        if kind == "tones" and not all(fc.thirds_reached(ref, fc.bank(name))):
            bad.append(f"{family} {label}: thirds reached {fc.thirds_reached(ref, fc.bank(name))}")
        if kind == "zeros":
            assert (ref.lin < fc.CLAMP - fc.linear_bar(ref)).all() and (ref.m32 == fc.FLOOR).all(), label
    assert n > 400 and not bad, "\n".join(bad)


def test_empty_filters_and_silence_are_below_the_clamp():
    """What the floor test of the GPU file asserts bit for bit is the floor in the oracle too, and further from the clamp than the bar
    (a silent frame's narrowest filter of the narrow bank reaches 4.8e-6)."""
    for name in fc.BANKS:
        basis = fc.bank(name)
        empty = ~(basis != 0).any(axis=1)
        x = torch.cat([fc.make_input("zeros", 1, 1030), fc.make_input("noise", 1, 1030, seed=2)])
        ref = fc.reference(x, fc.BANK_PAD, basis)
        bar = fc.linear_bar(ref)
        assert (ref.lin[0] < fc.CLAMP - bar).all() and (ref.lin[1][:, empty] == 0).all() and (ref.m32[0] == fc.FLOOR).all()
        assert (ref.m32[1][:, empty] == fc.FLOOR).all() and (ref.lin[1][:, ~empty] > fc.CLAMP + bar).all()


# ---------------------------------------------------------------------------------------------- the test entry's refusals
def test_test_entry_refuses_on_the_host():
    """bvc_test_stft_logmel checks pad_left, T and the reach of the last frame before it looks at the model, so a null model shows
    every refusal without a device; a shape that passes them then meets the null argument."""
    from bvcodec import _abi
    lib = _abi.load()

    def call(B, L, T, pad_left, lengths=None):
        rc = lib.bvc_test_stft_logmel(None, None, lengths, B, L, T, pad_left, 1.0, None, None)
        return rc, lib.bvc_last_error().decode()

    for p in (-1, 769, 1 << 20):
        rc, msg = call(1, 2049, 8, p)
        assert rc == -1 and f"pad_left {p} outside [0, 768]" in msg, msg
    for T in (0, -3):
        rc, msg = call(1, 2049, T, 256)
        assert rc == -1 and "at least one frame" in msg, msg
    dummy = 4096                                                     # (any non-null address: never read)
    for p in fc.PAD_LEFTS:
        for L in fc.padding_lengths(p):
            T = fc.num_frames(L, p)
            # the last frame of T frames reads up to 256 (T - 1) - p + 1023, reflected to 2 (L - 1) - that: the largest T that fits
            tmax = (2 * (L - 1) - 1023 + p) // 256 + 1
            assert tmax >= T >= 1
            rc, msg = call(2, L, tmax + 1, p)
            assert rc == -1 and "outside [0, L" in msg, (p, L, msg)
            rc, msg = call(2, L, tmax, p)
            assert rc == -1 and msg.endswith("null argument"), (p, L, msg)
            rc, msg = call(2, L, T + 1, p, dummy)
            assert rc == -1 and ("exceeds" in msg or "outside [0, L" in msg), (p, L, msg)
            rc, msg = call(2, L, T, p, dummy)
            assert rc == -1 and msg.endswith("null argument"), (p, L, msg)
        if p:                                                        # a left padding that is not shorter than the row
            rc, msg = call(1, p, 1, p)
            assert rc == -1 and f"reflected sample {p} outside [0, L = {p})" in msg, (p, msg)
    rc, msg = call(1, 2049, 9, 256, dummy)
    assert rc == -1 and "exceeds the 8 frames of a full row" in msg, msg
