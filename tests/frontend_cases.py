"""Shared by test_frontend_cases_cpu.py and test_gpu_frontend.py; imports no GPU code.  The mel banks, left paddings and shapes at
which the STFT + log-mel front end (csrc/k_frontend.hip) is held to the suite's bar, the inputs, the float64 and float32 oracles of a
case (oracle/frontend.py with the padding and the bank given explicitly), a direct statement of the same operator that also gives the
values in front of the clamp, and the comparison (vocoder_layers.compare in the linear and in the log domain, and the rule of the
floor)."""
import collections
import functools

import numpy as np
import torch

from bvcodec import synth
from oracle import frontend as ofe
from oracle import melbank as omel
from vocoder_layers import MARGIN, U, Ledger, compare

N_FFT, HOP, NUM_MELS = 1024, 256, 80
PAD_MAX = N_FFT - HOP                                     # mel_pad_left in [0, 768]
SCALE = float(np.float32(ofe.SCALING))                    # the float the library is handed; both oracles multiply by it
CLAMP = 1e-5                                              # meldataset.py:38-39
FLOOR = np.float32(np.log(np.float32(1e-5)))              # what a clamped element holds
LOG_SET = 1e-4                                            # elements of at least ten times the clamp are also compared as logarithms

# ---------------------------------------------------------------------------------------------- banks: name -> (fs, fmin, fmax)
BANKS = {
    "default": (22050, 0, 8000),
    "nyquist": (22050, 0, 11025),                         # every bin below Nyquist
    "fs48k": (48000, 0, 24000),                           # bin 512 carries a weight of rounding's size: the split runs with k = 512
    "above_nyquist": (22050, 0, 12000),                   # fmax above Nyquist: bin 512 carries a weight that matters
    "fs44k": (44100, 0, 8000),                            # fewer than three turns of the magnitude loop
    "fmin80": (22050, 80, 7600),
    "narrow": (22050, 3000, 3500),                        # 34 empty filters
}
# what each bank is there for: kmax (highest bin with a weight, + 1), empty filters, the weight of bin 512 (largest over the filters)
BANK_PINS = {
    "default": (372, 0, 0.0), "nyquist": (512, 0, 0.0), "fs48k": (513, 0, 2.5e-18), "above_nyquist": (513, 0, 2.0e-3),
    "fs44k": (186, 0, 0.0), "fmin80": (353, 0, 0.0), "narrow": (163, 34, 0.0),
}
NONZERO_DEFAULT = 727                                     # non-zero weights of the default bank


@functools.lru_cache(maxsize=None)
def bank(name):
    fs, fmin, fmax = BANKS[name]
    b = omel.mel_filterbank(fs, N_FFT, NUM_MELS, fmin, fmax)
    b.setflags(write=False)
    return b


def bank_tables(b):
    """(kmax, empty filters, largest weight of bin 512), as build_frontend (csrc/model_build.hip) would find them."""
    nz = b != 0
    cols = np.nonzero(nz.any(axis=0))[0]
    return int(cols.max()) + 1, int((~nz.any(axis=1)).sum()), float(b[:, N_FFT // 2].max())


def num_frames(L, pad_left):
    """config.num_frames at another left padding."""
    pr = PAD_MAX - pad_left
    if L <= pad_left or L <= pr:
        return 0
    return (L + pad_left + pr - N_FFT) // HOP + 1


# ---------------------------------------------------------------------------------------------- inputs (B, L) float32
IMPULSES = ("imp_first", "imp_last", "imp_seam_left", "imp_seam_right")
KINDS = ("noise", "speech", "tones", "zeros") + IMPULSES
# on-bin sinusoids of the 1024-point spectrum.  Bin k < 512 is index k of the 512-point transform Z[k0 + 8 k1 + 64 k2]: 8 j + j % 8 has
# the digits (j % 8, j % 8, j // 8), so j = 0..63 takes every digit through 0..7; about one tone per 8 bins also reaches every filter
# that is wider than that, and every third of the narrow bank (bins 139..163).
TONE_BINS = tuple(sorted({8 * j + j % 8 for j in range(64)} | {1, 255, 256, 510, 511}))
TONE_LEVELS = (0.02, 0.006, 0.002)


def impulse_at(kind, L, pad_left):
    """Sample 0, the last sample, and the samples the two reflections turn around."""
    return {"imp_first": 0, "imp_last": L - 1, "imp_seam_left": pad_left, "imp_seam_right": L - 1 - (PAD_MAX - pad_left)}[kind]


def make_input(kind, B, L, pad_left=256, seed=0):
    rng = np.random.default_rng([seed, B, L, KINDS.index(kind)])
    if kind == "noise":
        x = 0.1 * rng.standard_normal((B, L))
    elif kind == "speech":
        return synth.synthetic_speech(B, L, seed=seed + 17 * B + L, kind="speech")
    elif kind == "tones":
        n = np.arange(L)[None, :]
        x = np.zeros((B, L))
        for i, k in enumerate(TONE_BINS):
            x += TONE_LEVELS[i % 3] * np.cos(2.0 * np.pi * k * n / N_FFT + rng.uniform(0.0, 2.0 * np.pi, size=(B, 1)))
    else:
        x = np.zeros((B, L))
        if kind != "zeros":
            pos = impulse_at(kind, L, pad_left)
            assert 0 <= pos < L, (kind, L, pad_left)
            x[:, pos] = 1.0 / (1.0 + np.arange(B))
    return torch.from_numpy(x.astype(np.float32))


# ---------------------------------------------------------------------------------------------- oracles
def oracle_log_mel(x, pad_left, basis, dtype, frames=None):
    """oracle.frontend.log_mel of x * SCALE, time-major (B, T, 80), as float64 numpy.  frames: keep the first ones only."""
    xs = torch.as_tensor(x).to(dtype) * torch.tensor(SCALE, dtype=dtype)
    m = ofe.log_mel(xs, padding_left=pad_left, mel_basis=torch.from_numpy(np.array(basis)), dtype=dtype)
    m = m.permute(0, 2, 1).to(torch.float64).numpy()
    return m if frames is None else m[:, :frames]


def reflect_index(L, T, pad_left):
    """(T, 1024) sample indices of the frames: 256 t - pad_left + n, turned around once at 0 and at L - 1."""
    i = HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :] - pad_left
    i = np.where(i < 0, -i, np.where(i >= L, 2 * (L - 1) - i, i))
    assert i.min() >= 0 and i.max() < L, (L, T, pad_left)
    return i


def direct_mel_linear(x, pad_left, basis, frames=None):
    """The operator stated directly in float64: explicit reflect index, numpy's rfft of the windowed frames, sqrt(re^2 + im^2 + 1e-9), a
    dense matmul.  (B, T, 80), linear and NOT clamped: what decides whether an element is the floor."""
    x = np.asarray(x, dtype=np.float64) * SCALE
    L = x.shape[1]
    T = num_frames(L, pad_left) if frames is None else frames
    win = torch.hann_window(N_FFT, dtype=torch.float32).numpy().astype(np.float64)
    spec = np.fft.rfft(x[:, reflect_index(L, T, pad_left)] * win, axis=-1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return mag @ np.asarray(basis, dtype=np.float64).T


Reference = collections.namedtuple("Reference", "m64 m32 lin")     # log-mel of both oracles and the unclamped linear float64 values


def reference(x, pad_left, basis, frames=None):
    """frames: the case runs that many leading frames of a buffer (the streaming window: none of them reads padding)."""
    return Reference(oracle_log_mel(x, pad_left, basis, torch.float64, frames), oracle_log_mel(x, pad_left, basis, torch.float32, frames),
                     direct_mel_linear(x, pad_left, basis, frames))


# ---------------------------------------------------------------------------------------------- the comparison
Judgement = collections.namedtuple("Judgement", "lin log floor_errors floor_message")


def linear_bar(ref):
    lin64, lin32 = np.exp(ref.m64), np.exp(ref.m32)
    return MARGIN * max(float(np.abs(lin32 - lin64).max()), U * float(lin64.max()))


def log_set(ref):
    return np.exp(ref.m64) >= LOG_SET


def judge(got, ref, what):
    """got (B, T, 80) float32 log-mel of the library.  Linear domain, every element: vocoder_layers.compare on exp of the three; log
    domain, the elements of LOG_SET and more: the same on the logarithms.  The floor: an element whose unclamped float64 value is
    further below the clamp than the linear bar is FLOOR exactly, one further above is not, between the two either."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.m64.shape, (what, got.dtype, got.shape, ref.m64.shape)
    g64 = got.astype(np.float64)
    lin = compare(np.exp(g64), np.exp(ref.m64), np.exp(ref.m32), what + " linear")
    sel = log_set(ref)
    log = None
    if sel.any():
        log = compare(g64[sel].reshape(1, -1, 1), ref.m64[sel].reshape(1, -1, 1), ref.m32[sel].reshape(1, -1, 1), what + " log")
    at_floor = got == FLOOR
    wrong = ((ref.lin < CLAMP - lin.bar) & ~at_floor) | ((ref.lin > CLAMP + lin.bar) & at_floor)
    msg = ""
    if wrong.any():
        b, t, j = (int(v) for v in np.argwhere(wrong)[0])
        msg = (f"{what}: {int(wrong.sum())} elements on the wrong side of the clamp; first (item {b}, frame {t}, filter {j}): got "
               f"{got[b, t, j]!r}, float64 value in front of the clamp {ref.lin[b, t, j]!r}, band {lin.bar:.3e}")
    return Judgement(lin, log, int(wrong.sum()), msg)


def conditions(ref):
    """What the oracle alone says about a case: the share of elements in the log-domain set, and the share whose float64 value is
    within the linear bar of the clamp (they may be the floor or not)."""
    return float(log_set(ref).mean()), float((np.abs(ref.lin - CLAMP) <= linear_bar(ref)).mean())


def thirds_reached(ref, basis):
    """Per third of the bank that has a non-empty filter: is one of its filters in the log-domain set somewhere?"""
    live = (np.asarray(basis) != 0).any(axis=1)
    hit = log_set(ref).any(axis=(0, 1))
    return [bool(hit[a:b].any()) for a, b in ((0, 27), (27, 54), (54, 80)) if live[a:b].any()]


class Tally:
    """The verdicts of one test: each goes to the family's line of the ledger, the failures are raised together."""

    def __init__(self, ledger, family):
        self.ledger, self.family, self.failures = ledger, family, []

    def add(self, j):
        for dom, v in (("linear", j.lin), ("log", j.log)):
            if v is not None:
                self.ledger.add(f"{self.family}/{dom}", v)
                if not v.ok:
                    self.failures.append(v.message)
        if j.floor_errors:
            self.failures.append(j.floor_message)

    def close(self):
        assert not self.failures, f"{len(self.failures)} comparisons failed; first ones:\n" + "\n".join(self.failures[:12])


# ---------------------------------------------------------------------------------------------- the case lists
# (B, L): 2, 4, 8 and 86 frames per row are 2, 12, 40 and 172 in all - one partly filled workgroup; (3, 769) and (5, 1793) are 9 and
# 35 frames, so that the last workgroup holds 2, 1 and 3 live waves
BANK_SHAPES = ((1, 513), (3, 1030), (5, 2049), (2, 22050), (3, 769), (5, 1793))
BANK_INPUTS = ("noise", "tones")
BANK_PAD = 256
OTHER_PAD = 384                                                    # the model that ties mel_pad_left to the kernel
PAD_LEFTS = (0, 1, 255, 256, 257, 384, 767, 768)
BATCHES = (1, 2, 3, 5)


def padding_lengths(pad_left):
    lmin = max(pad_left, PAD_MAX - pad_left) + 1
    return (lmin, lmin + 1, lmin + 255, lmin + 256, 2049)


def padding_cases(pad_left):
    """(B, L, kind): every input kind at every length, the batch sizes in rotation."""
    return [(BATCHES[(i + j) % 4], L, kind) for i, L in enumerate(padding_lengths(pad_left)) for j, kind in enumerate(KINDS)]


# (B, L, pad_left): 2050, 3075 and 4100 workgroups' worth of frames - two workgroups, half of them and all of them take a second turn
GRID_CASES = ((4099, 513, 256), (4100, 769, 256), (4100, 1025, 256))
GRID_LIMIT = 2048                                                  # launch_stft_logmel's grid

RAGGED_L = 2049
RAGGED_LENS = (2049, 2048, 1281, 1280, 1279, 1000, 513, 512, 257, 256, 0, -5, 2149)
RAGGED_PAD = 256

STREAM_KS = (1, 2, 3, 5)
STREAM_BATCHES = (1, 3, 6)
STREAM_TAIL = 300


def stream_samples(k):
    """Samples k frames read at pad_left = 0."""
    return HOP * (k - 1) + N_FFT


@functools.lru_cache(maxsize=None)
def bank_case(name, B, L, kind, pad_left=BANK_PAD):
    x = make_input(kind, B, L, pad_left, seed=3)
    return x, reference(x, pad_left, bank(name))


@functools.lru_cache(maxsize=None)
def padding_case(pad_left, B, L, kind):
    x = make_input(kind, B, L, pad_left, seed=5)
    return x, reference(x, pad_left, bank("default"))


@functools.lru_cache(maxsize=None)
def grid_case(B, L, pad_left):
    x = make_input("noise", B, L, pad_left, seed=7)
    return x, reference(x, pad_left, bank("default"))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """x (B, L) with NaN behind each row's clamped length; per row the clamped length, its frames and the reference of x[b, :len]
    (None for a row of no frames)."""
    B, L = len(RAGGED_LENS), RAGGED_L
    x = make_input("noise", B, L, RAGGED_PAD, seed=9)
    rows = []
    for b, n in enumerate(RAGGED_LENS):
        n = min(max(n, 0), L)
        x[b, n:] = float("nan")
        T = num_frames(n, RAGGED_PAD)
        rows.append((n, T, reference(x[b:b + 1, :n], RAGGED_PAD, bank("default")) if T else None))
    return x, rows


@functools.lru_cache(maxsize=None)
def stream_case(k, B, kind):
    """x (B, cap) with NaN in its last STREAM_TAIL samples; the reference of the k frames the tick computes."""
    n = stream_samples(k)
    x = make_input(kind, B, n + STREAM_TAIL, 0, seed=11)
    x[:, n:] = float("nan")
    return x, reference(x[:, :n], 0, bank("default"), frames=k)


def all_references():
    """(family, label, kind, bank name, Reference) of every case the GPU file compares."""
    for name in BANKS:
        for B, L in BANK_SHAPES:
            for kind in BANK_INPUTS:
                yield "banks", f"{name} B {B} L {L} {kind}", kind, name, bank_case(name, B, L, kind)[1]
    for B, L in BANK_SHAPES:
        for kind in BANK_INPUTS:
            yield "banks", f"default pad {OTHER_PAD} B {B} L {L} {kind}", kind, "default", bank_case("default", B, L, kind, OTHER_PAD)[1]
    for p in PAD_LEFTS:
        for B, L, kind in padding_cases(p):
            yield "paddings", f"pad {p} B {B} L {L} {kind}", kind, "default", padding_case(p, B, L, kind)[1]
    for B, L, p in GRID_CASES:
        yield "grid-stride", f"B {B} L {L}", "noise", "default", grid_case(B, L, p)[1]
    for b, (n, T, ref) in enumerate(ragged_case()[1]):
        if ref is not None:
            yield "ragged", f"row {b} len {n}", "noise", "default", ref
    for k in STREAM_KS:
        for B in STREAM_BATCHES:
            for kind in ("noise", "tones"):
                yield "streaming window", f"k {k} B {B} {kind}", kind, "default", stream_case(k, B, kind)[1]
