"""The STFT + log-mel front end (stft_logmel_kernel, csrc/k_frontend.hip) against float64 where its tables, reflect seams, frame
counts and grid have edges (profiles/frontend_parity.md): seven mel banks through the public path, eight left paddings at the
shortest rows each accepts, more workgroups' worth of frames than the grid has, a mixed-length batch and the streaming tick's
window through bvc_test_stft_logmel, which makes one launch with the caller's frame count and padding.  The cases, inputs, oracles
and the comparison are frontend_cases.py's; tests/test_frontend_cases_cpu.py holds what the oracle alone must satisfy.  The bar is
the suite's, in the linear domain on every element and in the log domain from ten times the clamp on, with
the unchanged MARGIN.  Needs the MI355X: run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import frontend_cases as fc
from gpu_common import DEV, make_model

pytestmark = pytest.mark.gpu

LEDGER = fc.Ledger("frontend")
H_DIM = 64                                                # the coder is not run: the cheapest one


def model_of(name="default", pad_left=None):
    fs, fmin, fmax = fc.BANKS[name]
    return make_model(True, H_DIM, frontend={"fs": fs, "fmin": fmin, "fmax": fmax, "mel_pad_left": pad_left})[0]


def entry(model, x, pad_left, T, lens=None):
    """One launch through bvc_test_stft_logmel into a buffer of NaN: (B, T, 80) on the device."""
    from bvcodec import _abi
    eng = model.engine()
    xd = x.to(DEV).contiguous()
    B, L = xd.shape
    out = torch.full((B, T, fc.NUM_MELS), float("nan"), device=DEV)
    ld = None if lens is None else torch.tensor(list(lens), dtype=torch.int64, device=DEV)
    with torch.cuda.device(eng.device):
        _abi.check(eng.lib.bvc_test_stft_logmel(eng.handle, _abi.ptr(xd), _abi.ptr(ld, torch.int64), B, L, T, pad_left, fc.SCALE,
                                                _abi.ptr(out), eng.stream()))
    return out


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- banks, through the public path
@pytest.mark.parametrize("name", list(fc.BANKS))
def test_banks_against_float64(name):
    model = model_of(name)
    assert [model.conf[k] for k in ("fs", "fmin", "fmax")] == list(fc.BANKS[name]) and model.conf["mel_pad_left"] == fc.BANK_PAD
    tally = fc.Tally(LEDGER, "banks")
    for B, L in fc.BANK_SHAPES:
        for kind in fc.BANK_INPUTS:
            x, ref = fc.bank_case(name, B, L, kind)
            mel = model.mel_spectrogram(x.to(DEV))
            assert tuple(mel.shape) == (B, fc.num_frames(L, fc.BANK_PAD), fc.NUM_MELS)
            tally.add(fc.judge(host(mel), ref, f"bank {name} B {B} L {L} {kind}"))
    tally.close()


def test_configured_left_padding_reaches_the_kernel():
    model = model_of("default", fc.OTHER_PAD)
    assert model.conf["mel_pad_left"] == fc.OTHER_PAD
    tally = fc.Tally(LEDGER, "banks")
    for B, L in fc.BANK_SHAPES:
        for kind in fc.BANK_INPUTS:
            x, ref = fc.bank_case("default", B, L, kind, fc.OTHER_PAD)
            mel = model.mel_spectrogram(x.to(DEV))
            assert tuple(mel.shape) == (B, fc.num_frames(L, fc.OTHER_PAD), fc.NUM_MELS)
            tally.add(fc.judge(host(mel), ref, f"mel_pad_left {fc.OTHER_PAD} B {B} L {L} {kind}"))
    tally.close()


@pytest.mark.parametrize("name", list(fc.BANKS))
def test_floor_is_the_same_float(name):
    """A silent row, and every empty filter of a loud one, hold float32(log(float32(1e-5))) bit for bit."""
    model = model_of(name)
    empty = torch.from_numpy(~(fc.bank(name) != 0).any(axis=1))
    assert int(empty.sum()) == fc.BANK_PINS[name][1]
    x = torch.cat([fc.make_input("zeros", 1, 1030), fc.make_input("noise", 1, 1030, seed=2)])
    mel = model.mel_spectrogram(x.to(DEV)).cpu()
    floor = torch.tensor(fc.FLOOR)
    assert bool((mel[0] == floor).all())
    assert bool((mel[1][:, empty] == floor).all()) and bool((mel[1][:, ~empty] > floor).all())


# ---------------------------------------------------------------------------------------------- left paddings, through the test entry
@pytest.mark.parametrize("pad_left", fc.PAD_LEFTS)
def test_paddings_against_float64(pad_left):
    model = model_of()
    tally = fc.Tally(LEDGER, "paddings")
    for B, L, kind in fc.padding_cases(pad_left):
        x, ref = fc.padding_case(pad_left, B, L, kind)
        mel = entry(model, x, pad_left, fc.num_frames(L, pad_left))
        tally.add(fc.judge(host(mel), ref, f"pad_left {pad_left} B {B} L {L} {kind}"))
    tally.close()


# ---------------------------------------------------------------------------------------------- more frames than the grid takes at once
@pytest.mark.parametrize("B,L,pad_left", fc.GRID_CASES)
def test_grid_stride_against_float64(B, L, pad_left):
    """Workgroups that take a second block of four frames re-use their LDS; every row is compared."""
    model = model_of()
    T = fc.num_frames(L, pad_left)
    nblocks = (B * T + 3) // 4
    assert nblocks > fc.GRID_LIMIT
    x, ref = fc.grid_case(B, L, pad_left)
    mel = entry(model, x, pad_left, T)
    tally = fc.Tally(LEDGER, "grid-stride")
    tally.add(fc.judge(host(mel), ref, f"grid-stride B {B} L {L} ({nblocks} blocks)"))
    tally.close()


# ---------------------------------------------------------------------------------------------- mixed-length batch
def test_ragged_rows_against_float64():
    model = model_of()
    x, rows = fc.ragged_case()
    L, T = fc.RAGGED_L, fc.num_frames(fc.RAGGED_L, fc.RAGGED_PAD)
    mel = host(entry(model, x, fc.RAGGED_PAD, T, fc.RAGGED_LENS))
    assert not np.isnan(mel).any() and np.isfinite(mel).all()
    tally = fc.Tally(LEDGER, "ragged")
    for b, (n, frames, ref) in enumerate(rows):
        assert (mel[b, frames:] == fc.FLOOR).all(), (b, n, frames)
        if frames:
            tally.add(fc.judge(mel[b:b + 1, :frames], ref, f"ragged row {b} len {fc.RAGGED_LENS[b]}"))
    tally.close()


def test_ragged_with_full_lengths_is_the_plain_launch():
    model = model_of()
    B, L = len(fc.RAGGED_LENS), fc.RAGGED_L
    T = fc.num_frames(L, fc.RAGGED_PAD)
    x = fc.make_input("noise", B, L, fc.RAGGED_PAD, seed=13)
    plain = entry(model, x, fc.RAGGED_PAD, T)
    assert bool(torch.isfinite(plain).all())
    assert torch.equal(entry(model, x, fc.RAGGED_PAD, T, [L] * B), plain)
    assert torch.equal(model.mel_spectrogram(x.to(DEV)), plain)


# ---------------------------------------------------------------------------------------------- the streaming tick's window
@pytest.mark.parametrize("k", fc.STREAM_KS)
@pytest.mark.parametrize("B", fc.STREAM_BATCHES)
def test_streaming_window_against_float64(k, B):
    """pad_left = 0 and T = k on a (B, cap) buffer whose samples behind the k frames are NaN: nothing of them is read."""
    model = model_of()
    tally = fc.Tally(LEDGER, "streaming window")
    for kind in ("noise", "tones"):
        x, ref = fc.stream_case(k, B, kind)
        mel = entry(model, x, 0, k)
        assert bool(torch.isfinite(mel).all())
        tally.add(fc.judge(host(mel), ref, f"window k {k} B {B} {kind}"))
    tally.close()


# ---------------------------------------------------------------------------------------------- refusals, with a model
def test_test_entry_refuses_with_a_model():
    from bvcodec import _abi
    model = model_of()
    x = fc.make_input("noise", 2, 2049)
    for pad_left, T, lens, text in ((769, 8, None, "pad_left 769 outside [0, 768]"), (256, 0, None, "at least one frame"),
                                    (256, 15, None, "outside [0, L = 2049)"), (256, 9, [2049, 2049], "exceeds the 8 frames of a full row")):
        with pytest.raises(_abi.BvcError, match=text.replace("[", r"\[").replace(")", r"\)")):
            entry(model, x, pad_left, T, lens)
    assert bool(torch.isfinite(entry(model, x, 256, 14)).all())      # the last T whose frames reflect once


# ---------------------------------------------------------------------------------------------- the ledger
def test_frontend_parity_ledger():
    """Prints the PARITY lines of everything this module compared so far (profiles/frontend_parity.md); fails if any comparison did."""
    print(flush=True)
    LEDGER.close()
