"""Shared by test_client_rate_cpu.py, test_resample_cases_cpu.py and test_gpu_resample.py; imports no GPU code.  The rate pairs at which
the resamplers (resample_poly_kernel in csrc/k_frontend.hip, resample_stream_kernel in csrc/k_resample_stream.hip) are held to float64,
their pinned geometry, the two walks in numpy float64, the inputs and lengths, the reference (scipy.signal.resample_poly in float64),
the per-element bar and the comparison, the closed form of an impulse's output, and the s16 case list."""
import collections
import functools

import numpy as np
import torch

from bvcodec import preprocess, synth
from vocoder_layers import U, Ledger  # noqa: F401  (Ledger is re-exported: the GPU file's ledger is this class)

FS = 22050
RATES = (8000, 16000, 24000, 32000, 44100, 48000)
ADDED_RATES = (11025, 12000, 96000, 22051)                # 22051 is coprime with 22050: 463k taps, 64-bit pos, a phase stride of 22050
ALL_RATES = RATES + ADDED_RATES
USUAL_PAIRS = [(r, FS) for r in RATES] + [(FS, r) for r in RATES]          # (rate_in, rate_out)
PAIRS = [(r, FS) for r in ALL_RATES] + [(FS, r) for r in ALL_RATES]

# (rate_in, rate_out): (up, down, ntaps, H = ceil(ntaps / up), lag = n_pre_remove); test_resample_cases_cpu.py re-derives every row
GEOMETRY = {
    (8000, 22050): (441, 160, 8891, 21, 28),
    (16000, 22050): (441, 320, 8891, 21, 14),
    (24000, 22050): (147, 160, 3361, 23, 11),
    (32000, 22050): (441, 640, 13441, 31, 11),
    (44100, 22050): (1, 2, 43, 43, 11),
    (48000, 22050): (147, 320, 6721, 46, 11),
    (11025, 22050): (2, 1, 42, 21, 21),
    (12000, 22050): (147, 80, 2991, 21, 19),
    (96000, 22050): (147, 640, 13441, 92, 11),
    (22051, 22050): (22050, 22051, 463072, 22, 11),
    (22050, 8000): (160, 441, 9262, 58, 11),
    (22050, 16000): (320, 441, 9262, 29, 11),
    (22050, 24000): (160, 147, 3218, 21, 11),
    (22050, 32000): (640, 441, 13016, 21, 15),
    (22050, 44100): (2, 1, 42, 21, 21),
    (22050, 48000): (320, 147, 6435, 21, 22),
    (22050, 11025): (1, 2, 43, 43, 11),
    (22050, 12000): (80, 147, 3088, 39, 11),
    (22050, 96000): (640, 147, 12869, 21, 44),
    (22050, 22051): (22051, 22050, 463061, 21, 11),
}
LDS_FLOATS = 16384                                        # H + max_in floats of a push: the 64 KiB bvc_resampler_create accepts


@functools.lru_cache(maxsize=None)
def geometry(rate_in, rate_out):
    """preprocess.design(rate_out, rate_in): up, down, taps (float64, not writable), n_pre_remove."""
    up, down, h, lag = preprocess.design(rate_out, rate_in)
    h.setflags(write=False)
    return up, down, h, lag


def history(rate_in, rate_out):
    up, _, h, _ = geometry(rate_in, rate_out)
    return -(-len(h) // up)


def out_len(n, up, down):
    return -(-n * up // down)


def family(rate_in, rate_out):
    return "offline-down" if rate_out < rate_in else "offline-up"


# ---------------------------------------------------------------------------------------------- the order of the sum
def offline_walk(x, up, down, h, lag):
    """resample_poly_kernel's walk (csrc/k_frontend.hip) in numpy float64."""
    n_out = -(-len(x) * up // down)
    y = np.zeros(n_out)
    for m in range(n_out):
        pos = (m + lag) * down
        i, k = pos // up, pos % up
        if i >= len(x):
            k += (i - (len(x) - 1)) * up
            i = len(x) - 1
        acc = 0.0
        while k < len(h) and i >= 0:
            acc += h[k] * x[i]
            k += up
            i -= 1
        y[m] = acc
    return y


class ChunkedWalk:
    """resample_stream_kernel's walk (csrc/k_resample_stream.hip) for one row in numpy float64: the history of ceil(ntaps / up) inputs
    and the chunk side by side, the outputs E(N) .. E(N + n) of a push, the rest with a clamp at the end in a flush.  delayed: the
    row's stream is zeros(lag) ++ y, ceil(N up / down) of its samples after N inputs, the last lag in the flush."""

    def __init__(self, rate_in, rate_out, delayed=False):
        self.rates = (rate_in, rate_out)
        self.up, self.down, self.h, self.lag = geometry(rate_in, rate_out)
        self.H = -(-len(self.h) // self.up)
        self.delayed = bool(delayed)
        self.reset()

    def reset(self):
        self.hist, self.N = np.zeros(self.H), 0

    def E(self, n):
        from bvcodec.streaming import resampler_count
        return resampler_count(*self.rates, n)

    def count(self, n):
        """Samples of the row's stream after n inputs."""
        return out_len(n, self.up, self.down) if self.delayed else self.E(n)

    def outputs(self, staged, N1, m0, m1):
        out = []
        lo = max(0, self.N - self.H)
        for m in range(m0, m1):
            pos = (m + self.lag) * self.down
            i, k = pos // self.up, pos % self.up
            if i >= N1:
                k += (i - (N1 - 1)) * self.up
                i = N1 - 1
            acc = 0.0
            while k < len(self.h) and i >= lo:
                acc += self.h[k] * staged[i - self.N + self.H]
                k += self.up
                i -= 1
            out.append(acc)
        return out

    def span(self, staged, N1, q0, q1):
        """Samples q0 .. q1 of the row's stream: when delayed, sample q is output q - lag, a zero in front of the first."""
        if not self.delayed:
            return self.outputs(staged, N1, q0, q1)
        zeros = max(0, min(q1, self.lag) - q0)
        return [0.0] * zeros + self.outputs(staged, N1, q0 + zeros - self.lag, q1 - self.lag)

    def push(self, chunk):
        staged = np.concatenate([self.hist, chunk])
        N1 = self.N + len(chunk)
        out = self.span(staged, N1, self.count(self.N), self.count(N1))
        self.hist, self.N = staged[len(chunk):], N1
        return out

    def flush(self):
        return self.span(self.hist, self.N, self.count(self.N), out_len(self.N, self.up, self.down) + (self.lag if self.delayed else 0))


def walk(x, up, down, h, lag):
    """offline_walk for the rows of x (R, L) at once: the same terms in the same order, one tap of every output per turn."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[1]
    pos = (np.arange(out_len(L, up, down), dtype=np.int64) + lag) * down
    i = pos // up
    k = pos - i * up
    skip = np.maximum(i - (L - 1), 0)
    i, k = i - skip, k + skip * up
    acc = np.zeros((x.shape[0], len(pos)))
    while True:
        ok = (k < len(h)) & (i >= 0)
        if not ok.any():
            return acc
        acc = np.where(ok, acc + h[np.where(ok, k, 0)] * x[:, np.where(ok, i, 0)], acc)
        k, i = k + up, i - 1


# ---------------------------------------------------------------------------------------------- inputs (B, L) float32
IMPULSES = ("imp_first", "imp_last", "imp_H")
KINDS = ("noise", "speech", "dc", "nyquist", "big", "small", "zeros") + IMPULSES
BATCHES = (1, 3, 5)
BIG, SMALL = 2.0 ** 100, 2.0 ** -100
TINY = 2.0 ** -126                                        # the smallest normal float32


def impulse_at(kind, L, H):
    """Sample 0, the last sample and sample H (the last one of a signal that has no sample H)."""
    return {"imp_first": 0, "imp_last": L - 1, "imp_H": min(H, L - 1)}[kind]


def make_input(kind, B, L, H, seed=0):
    """big and small are the noise of the same (B, L, seed) times 2^100 and 2^-100."""
    if kind in ("noise", "big", "small"):
        x = np.random.default_rng([seed, B, L]).standard_normal((B, L)).astype(np.float32)
        x = x * np.float32({"noise": 1.0, "big": BIG, "small": SMALL}[kind])
    elif kind == "speech":
        x = 0.9 * synth.synthetic_speech(B, L, seed=seed + 17 * B + L, kind="speech").numpy().astype(np.float64)
    elif kind == "dc":
        x = np.ones((B, L))
    elif kind == "nyquist":
        x = np.tile(1.0 - 2.0 * (np.arange(L) % 2), (B, 1))
    else:
        x = np.zeros((B, L))
        if kind != "zeros":
            x[:, impulse_at(kind, L, H)] = 1.0
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert np.isfinite(x).all()
    return torch.from_numpy(x)


def impulse_expected(rate_in, rate_out, L, p):
    """What a unit impulse at sample p of L gives: float32(h[k]) at the outputs m whose walk meets it, k = (m + lag) down - p up, exact
    zeros elsewhere."""
    up, down, h, lag = geometry(rate_in, rate_out)
    k = (np.arange(out_len(L, up, down), dtype=np.int64) + lag) * down - p * up
    ok = (k >= 0) & (k < len(h))
    return np.where(ok, h[np.where(ok, k, 0)], 0.0).astype(np.float32)


def zero_extension(rate_in, rate_out, L):
    """need - len(h) of preprocess.resample_poly: positive where it appends zeros to the taps."""
    up, down, h, lag = geometry(rate_in, rate_out)
    return (out_len(L, up, down) + lag - 1) * down - (L - 1) * up + 1 - len(h)


def lengths(rate_in, rate_out):
    """1 and 2, the history's length and its neighbours, a length whose outputs end on an input (L up % down == 0), the next one, 3000."""
    up, down, _, _ = geometry(rate_in, rate_out)
    H = history(rate_in, rate_out)
    whole = down * -(-(2 * H + 3) // down)
    return tuple(sorted({1, 2, H - 1, H, H + 1, whole, whole + 1, 3000}))


def cases(rate_in, rate_out):
    """(L, kind, B): every kind at every length, the batch sizes in rotation."""
    return [(L, kind, BATCHES[(a + b) % 3]) for a, L in enumerate(lengths(rate_in, rate_out)) for b, kind in enumerate(KINDS)]


# (rate_in, rate_out, B, L): more than 2048 x 256 outputs per row - the offline kernel's grid takes a second trip
GRID_CASES = ((48000, 22050, 2, 1150000), (22050, 48000, 2, 241000))
GRID_OUTPUTS = 2048 * 256


# ---------------------------------------------------------------------------------------------- reference and bar
Reference = collections.namedtuple("Reference", "ref tol")


def reference(x, rate_in, rate_out):
    """x (R, L) -> scipy.signal.resample_poly of x in float64, and per element the bar
    U |ref| + 4 (H + 1) 2^-53 S + 2^-149 with S = sum |h_k| |x_i| over the output's own terms: at most H double products and adds on
    either side (2 H 2^-53 S each, fused or not), then one rounding to float32."""
    import scipy.signal as ss
    up, down, h, lag = geometry(rate_in, rate_out)
    x = np.asarray(x, dtype=np.float64)
    if up == down:
        return Reference(x.copy(), U * np.abs(x) + 2.0 ** -149)
    ref = ss.resample_poly(x, rate_out, rate_in, axis=1)
    n_out = out_len(x.shape[1], up, down)
    assert ref.shape == (x.shape[0], n_out)
    S = ss.upfirdn(np.abs(h), np.abs(x), up, down, axis=1)[:, lag:lag + n_out]
    assert S.shape == ref.shape
    H = -(-len(h) // up)
    return Reference(ref, U * np.abs(ref) + 4.0 * (H + 1) * 2.0 ** -53 * S + 2.0 ** -149)


@functools.lru_cache(maxsize=None)
def block(rate_in, rate_out, L):
    """kind -> (x (B, L) float32 tensor, Reference) of every case of that length; one reference call for all of them."""
    H = history(rate_in, rate_out)
    todo = [(kind, B) for l, kind, B in cases(rate_in, rate_out) if l == L]
    xs = [make_input(kind, B, L, H, seed=rate_in + rate_out) for kind, B in todo]
    r = reference(np.concatenate([x.numpy() for x in xs]), rate_in, rate_out)
    out, at = {}, 0
    for (kind, B), x in zip(todo, xs):
        out[kind] = (x, Reference(r.ref[at:at + B], r.tol[at:at + B]))
        at += B
    return out


@functools.lru_cache(maxsize=None)
def grid_case(rate_in, rate_out, B, L):
    x = make_input("noise", B, L, history(rate_in, rate_out), seed=3)
    return x, reference(x.numpy(), rate_in, rate_out)


# ---------------------------------------------------------------------------------------------- the comparison
Verdict = collections.namedtuple("Verdict", "ok ratio worst e32 scale differ count message")


def compare(got, r, what):
    """got (R, n) float32 against a Reference of the same shape: the largest |got - ref| / bar and where; an element that is not finite
    is the worst there is.  differ / count: elements that are not float32(ref)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == r.ref.shape, (what, got.dtype, got.shape, r.ref.shape)
    if got.size == 0:
        return Verdict(True, 0.0, None, 0.0, 0.0, 0, 0, f"{what}: nothing to compare")
    with np.errstate(over="ignore", invalid="ignore"):
        ratio = np.where(np.isfinite(got), np.abs(got.astype(np.float64) - r.ref) / r.tol, np.inf)
    ref32 = r.ref.astype(np.float32)
    b, m = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    worst = float(ratio[b, m])
    msg = (f"{what}: largest |got - ref| / bar = {worst:.3f} at (row {b}, output {m}): got {got[b, m]!r}, float64 {r.ref[b, m]!r}, bar "
           f"{r.tol[b, m]:.3e}; {int((ratio > 1).sum())} of {got.size} above the bar")
    return Verdict(worst <= 1.0, worst, (b, m), float(np.abs(ref32.astype(np.float64) - r.ref).max()), float(np.abs(r.ref).max()),
                   int((got != ref32).sum()), got.size, msg)


class Tally:
    """The verdicts of one test: each goes to the family's line of the ledger, the failures are raised together."""

    def __init__(self, ledger, fam):
        self.ledger, self.family, self.failures, self.differ, self.count, self.worst = ledger, fam, [], 0, 0, 0.0

    def add(self, v):
        self.ledger.add(self.family, v)
        self.differ, self.count, self.worst = self.differ + v.differ, self.count + v.count, max(self.worst, v.ratio)
        if not v.ok:
            self.failures.append(v.message)

    def check(self, ok, message):
        if not ok:
            self.failures.append(message)

    def close(self, label):
        print(f"RESAMPLE {label} family={self.family} elements={self.count} not_float32_of_ref={self.differ} max_ratio={self.worst:.3f}", flush=True)
        assert not self.failures, f"{len(self.failures)} comparisons failed; first ones:\n" + "\n".join(self.failures[:12])


# ---------------------------------------------------------------------------------------------- streams
def ragged(total, hop):
    """Chunks of 1, 7, a hop, three hops and 5, over and over, up to total samples."""
    out, at, i = [], 0, 0
    while at < total:
        n = min((1, 7, hop, 3 * hop + 5)[i % 4], total - at)
        out.append(n)
        at, i = at + n, i + 1
    return out


# ---------------------------------------------------------------------------------------------- s16
# float32 y -> the s16 a resampler stores: ties go to even, both ends saturate, NaN is 0
S16_POINTS = (
    (0.0, 0), (-0.0, 0), (0.5 / 32768, 0), (-0.5 / 32768, 0), (1.5 / 32768, 2), (-1.5 / 32768, -2), (2.5 / 32768, 2), (-2.5 / 32768, -2),
    (0.75 / 32768, 1), (32766.5 / 32768, 32766), (32767.0 / 32768, 32767), (32767.5 / 32768, 32767), (-32767.5 / 32768, -32768),
    (1.0, 32767), (-1.0, -32768), (1.0 + 2.0 ** -23, 32767), (1.5, 32767), (-1.5, -32768), (3.0e38, 32767), (-3.0e38, -32768),
    (float("inf"), 32767), (float("-inf"), -32768), (float("nan"), 0), (2.0 ** -140, 0), (-2.0 ** -140, 0),
)
S16_PAIRS = ((16000, FS), (FS, 48000))


def square(B, L, seed=0):
    """+-1 square waves with periods of a few samples, every row its own: the filter's overshoot is above full scale."""
    n = np.arange(L)
    rows = [np.where((n + seed + b) // (3 + (seed + b) % 4) % 2 == 0, 1.0, -1.0) for b in range(B)]
    return torch.from_numpy(np.array(rows, dtype=np.float32))


def s16_expected(ref):
    """clamp(32768 ref, -32768, 32767) in float64: what a stored s16 is within half a step (and the bar) of."""
    return np.clip(32768.0 * np.asarray(ref, dtype=np.float64), -32768.0, 32767.0)
