"""Repair window of a receive session (bvc_stream_codec_set_repair / _late), the parts that need no GPU: the acceptance and pass
arithmetic (bvcodec.streaming.repair_plan, the same as the library's), the premise of tests/test_gpu_late_repair.py - on the wide
weight draw one lost frame is still in the decoder's output 49 frames later, on the default draw it is not - and how far one mel frame
reaches through the generator."""
import numpy as np
import torch

import bvrnn_draws
import conceal_oracle as co
from bvcodec import synth
from bvcodec.streaming import CONTEXT_FRAMES, generator_reach, repair_plan
from oracle import bigvgan as obig

# ticks of 1, 2 and 3 frames: (first frame, count); 20 frames decoded
TICKS = [(0, 1), (1, 2), (3, 3), (6, 1), (7, 2), (9, 3), (12, 1), (13, 2), (15, 3), (18, 2)]


def test_window_edges():
    # W = 8: frames 12 .. 19 are the last eight; tick 6 = (12, 1) is the oldest retained, tick 5 = (9, 3) ends at frame 11
    taken, passes = repair_plan(TICKS, 8, [(0, 0, 12, True), (1, 0, 11, True), (2, 0, 19, True), (3, 0, 20, True)])
    assert taken == [True, False, True, False]                 # 11: one frame older than the window; 20: not decoded yet
    assert passes == [(6, [0]), (9, [2])]
    # W = 7: frames 13 .. 19; the oldest retained tick is (13, 2), frame 12 has left
    assert repair_plan(TICKS, 7, [(0, 0, 12, True), (0, 0, 13, True)])[0] == [False, True]
    # a tick is retained whole: W = 6 keeps frames 14 .. 19, and with them frame 13 of tick (13, 2)
    taken, passes = repair_plan(TICKS, 6, [(0, 0, 13, True)])
    assert taken == [True] and passes == [(7, [0])]
    # no window, nothing decoded
    assert repair_plan(TICKS, 0, [(0, 0, 19, True)]) == ([False], [])
    assert repair_plan([], 8, [(0, 0, 0, True)]) == ([False], [])
    # the replay never spans more than W + kmax - 1 frames
    for W in range(1, 21):
        done = 20
        oldest = min(i for i, (f0, k) in enumerate(TICKS) if f0 + k > done - W)
        assert done - TICKS[oldest][0] <= W + 3 - 1


def test_present_frames_duplicates_and_previous_occupants():
    req = [(0, 0, 15, False),            # arrived in time
           (0, 0, 16, True), (0, 0, 16, True),                  # the second late for one frame
           (1, None, 16, True),          # an idle (or waiting) slot
           (2, 14, 1, True),             # slot 2's stream began at session frame 14: its frame 1 is session frame 15
           (2, 14, -1, True),            # the previous occupant's last frame cannot be addressed
           (2, 14, 6, True)]             # session frame 20: not decoded yet
    taken, passes = repair_plan(TICKS, 8, req)
    assert taken == [False, True, False, False, True, False, False]
    assert passes == [(8, [0, 2])]                              # frames 15 and 16 both lie in tick (15, 3)


def test_rows_with_different_starts_fall_into_two_passes():
    req = [(0, 0, 19, True), (1, 0, 13, True), (2, 0, 18, True), (1, 0, 16, True), (3, 0, 14, True)]
    taken, passes = repair_plan(TICKS, 8, req)
    assert all(taken)
    assert passes == [(7, [1, 3]), (9, [0, 2])]                 # a row starts at its EARLIEST late frame


# ------------------------------------------------------------------------------------------------ the premise of the GPU tests
def delta_mel(draw, mode):
    sd = bvrnn_draws.state_dict(1024, draw)
    B, T, nb = 2, 60, 35
    rng = np.random.default_rng(3)
    codes = torch.from_numpy(rng.integers(0, 2, size=(B, T, 64)).astype(np.float32))
    codes[:, :, nb:] = 0.5
    bits = torch.full((B, T), float(nb))
    present = torch.ones(B, T, dtype=torch.bool)
    whole = co.decode_conceal(sd, codes, present, bits, torch.zeros(B, 1024), mode=mode)["mel"]
    present[:, 10] = False
    holed = co.decode_conceal(sd, codes, present, bits, torch.zeros(B, 1024), mode=mode)["mel"]
    return float((whole[:, 59] - holed[:, 59]).abs().max())


def test_the_wide_draw_remembers_a_lost_frame_and_the_default_draw_does_not():
    """|mel(frame 10 lost) - mel(not lost)| at frame 59, float32 oracle.  Wide draw: at least 2e-4, the project's bar for the GPU's mel
    (measured 7.5e-4 without concealment, 9.4e-4 with the prior) - "the repaired session equals the on-time one" is then a statement
    about the repair.  Default draw: below 1e-6, the state has forgotten, and the same statement would hold without any repair."""
    for mode in ("none", "prior"):
        wide, default = delta_mel("wide", mode), delta_mel("default", mode)
        print(f"conceal {mode}: |d mel| at frame 59: wide {wide:.2e}, default {default:.2e}")
        assert wide >= 2e-4
        assert default < 1e-6


# ------------------------------------------------------------------------------------------------ the generator's reach
def test_one_mel_frame_reaches_26_frames_ahead(conf_var):
    vcfg = conf_var["vocoder_config"]
    assert generator_reach(vcfg) == 26 == CONTEXT_FRAMES
    sd = synth.generator_state_dict(conf_var, 1235)
    T, f = 48, 12
    rng = np.random.default_rng(1)
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((1, 80, T))).astype(np.float32))
    other = mel.clone()
    other[:, :, f] += 0.5
    a, b = obig.forward(sd, vcfg, mel, 256 * T)[0, 0], obig.forward(sd, vcfg, other, 256 * T)[0, 0]
    assert torch.equal(a[:256 * f], b[:256 * f])                                   # causal
    assert torch.equal(a[256 * (f + 27):], b[256 * (f + 27):])
    assert not torch.equal(a[256 * (f + 26):256 * (f + 27)], b[256 * (f + 26):256 * (f + 27)])
