"""The resamplers and the PCM conversion at the client-rate boundary against float64 (profiles/resample_parity.md): the offline kernel
(resample_poly_kernel, csrc/k_frontend.hip) through preprocess.resample_poly and the streaming one (resample_stream_kernel and
rs_update_kernel, csrc/k_resample_stream.hip, with the host book of csrc/resampler.hip) through StreamResampler, each against
scipy.signal.resample_poly in float64 on the stream's own signal - not against one another, which test_gpu_client_rate.py does.  Twenty
rate pairs, the inputs, lengths, reference and the per-element bar are resample_cases.py's; tests/test_resample_cases_cpu.py holds what
must be true of them without a device.  Also s16 in and out, the rows' book past one update launch, strides and offset of a push, the
largest push the LDS takes, and peak_normalize_kernel.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import resample_cases as rc
from gpu_common import DEV

pytestmark = pytest.mark.gpu

LEDGER = rc.Ledger("resample")
NAN = float("nan")


def host(t):
    return t.cpu().numpy()


def offline(x, rate_in, rate_out):
    from bvcodec import preprocess
    return host(preprocess.resample_poly(x.to(DEV), rate_out, rate_in))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------- the offline kernel
@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_offline_against_float64(rate_in, rate_out):
    """Every input at every length under the bar; an impulse gives float32(h[k]) and exact zeros; x 2^100 and x 2^-100 give the
    noise's bits times that scale."""
    H = rc.history(rate_in, rate_out)
    tally = rc.Tally(LEDGER, rc.family(rate_in, rate_out))
    for L in rc.lengths(rate_in, rate_out):
        for kind, (x, ref) in rc.block(rate_in, rate_out, L).items():
            what = f"{rate_in}->{rate_out} L {L} {kind} B {x.shape[0]}"
            got = offline(x, rate_in, rate_out)
            tally.add(rc.compare(got, ref, what))
            if kind in rc.IMPULSES:
                want = np.tile(rc.impulse_expected(rate_in, rate_out, L, rc.impulse_at(kind, L, H)), (x.shape[0], 1))
                tally.check(np.array_equal(got, want), f"{what}: {int((got != want).sum())} outputs are not float32(h[k]) / zero")
            if kind == "zeros":
                tally.check(not got.any(), f"{what}: not zeros")
            if kind in ("big", "small"):
                base = offline(rc.make_input("noise", x.shape[0], L, H, seed=rate_in + rate_out), rate_in, rate_out)
                want = base * np.float32(rc.BIG if kind == "big" else rc.SMALL)
                tally.check(np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} outputs are not the scaled bits")
    tally.close(f"offline {rate_in}->{rate_out}")


@pytest.mark.parametrize("rate_in,rate_out,B,L", rc.GRID_CASES)
def test_offline_grid_stride_against_float64(rate_in, rate_out, B, L):
    """More than 2048 x 256 outputs per row: every thread of the first workgroups takes a second output."""
    x, ref = rc.grid_case(rate_in, rate_out, B, L)
    assert ref.ref.shape[1] > rc.GRID_OUTPUTS
    tally = rc.Tally(LEDGER, rc.family(rate_in, rate_out))
    tally.add(rc.compare(offline(x, rate_in, rate_out), ref, f"grid-stride {rate_in}->{rate_out} B {B} L {L}"))
    tally.close(f"grid-stride {rate_in}->{rate_out}")


# ---------------------------------------------------------------------------------------------- the streaming kernel
class Stream:
    """What one row has been given since it was opened, and what it gave."""

    def __init__(self, row, label):
        self.row, self.label, self.x, self.y, self.n = row, label, [], [], 0

    def signal(self):
        return torch.cat(self.x) if self.x else torch.empty(0)

    def output(self):
        return np.concatenate(self.y) if self.y else np.empty(0, dtype=np.float32)


def stream_count(rs, n):
    from bvcodec.streaming import resampler_count
    return rc.out_len(n, rs.up, rs.down) if rs.delayed else resampler_count(rs.rate_in, rs.rate_out, n)


def push(rs, chunk, live, offsets=None, valid=None):
    """One push of chunk (B, n) - NaN goes wherever no row may read: in front of a row's offset, behind its n_valid, in idle rows - with
    the counts checked against resampler_count, zeros behind every row's count and in idle rows.  live: row -> Stream."""
    offsets, valid = offsets or {}, valid or {}
    chunk = chunk.clone()
    n = chunk.shape[1]
    for row in range(rs.B):
        if row not in live:
            chunk[row] = NAN
            continue
        chunk[row, :offsets.get(row, 0)] = NAN
        chunk[row, valid.get(row, n):] = NAN
    y, counts = rs.push(chunk.to(DEV))
    y = host(y)
    assert y.shape == (rs.B, rc.out_len(n, rs.up, rs.down))
    for row in range(rs.B):
        s = live.get(row)
        if s is None:
            assert counts[row] == 0 and not y[row].any(), ("idle row", row)
            continue
        part = chunk[row, offsets.get(row, 0):valid.get(row, n)]
        c = stream_count(rs, s.n + len(part)) - stream_count(rs, s.n)
        assert int(counts[row]) == c, (s.label, int(counts[row]), c)
        assert bits(y[row, c:]).any() == 0, (s.label, "not zeros behind the count")
        s.x.append(part)
        s.y.append(y[row, :c].copy())
        s.n += len(part)


def flush(rs, s):
    tail = host(rs.flush(s.row))
    assert len(tail) == rc.out_len(s.n, rs.up, rs.down) + (rs.lag if rs.delayed else 0) - stream_count(rs, s.n), s.label
    s.y.append(tail)


def judge_stream(rs, s, tally, what):
    """The stream's whole output: when delayed lag exact zeros, then its own signal's float64 resampling under the bar."""
    got = s.output()
    lead = rs.lag if rs.delayed else 0
    assert got.dtype == np.float32 and len(got) == lead + rc.out_len(s.n, rs.up, rs.down), (what, s.label, len(got))
    tally.check(not bits(got[:lead]).any(), f"{what} {s.label}: the leading {lead} samples are not zeros")
    if s.n:
        x = s.signal().numpy()[None]
        assert np.isfinite(x).all()
        tally.add(rc.compare(got[None, lead:], rc.reference(x, rs.rate_in, rs.rate_out), f"{what} {s.label} ({s.n} inputs)"))


@pytest.mark.parametrize("delayed", (False, True), ids=("plain", "delayed"))
@pytest.mark.parametrize("rate_in,rate_out", rc.PAIRS)
def test_stream_against_float64(rate_in, rate_out, delayed):
    """Chunks of 1, 7, a hop, three hops and 5, twice.  Row 0 runs throughout; row 1 opens 3 samples into the third chunk, ends with 4
    samples of the sixth, is flushed and runs again from the seventh; row 2 is opened and flushed with nothing pushed, then runs for 5
    samples of the second chunk - a stream shorter than the history - and is flushed; row 3 stays idle."""
    from bvcodec.streaming import StreamResampler
    hop = rate_in // 50
    H = rc.history(rate_in, rate_out)
    chunks = rc.ragged(2 * (4 * hop + 13), hop)
    assert chunks == [1, 7, hop, 3 * hop + 5] * 2 and H > 5
    X = torch.randn(4, sum(chunks), generator=torch.Generator().manual_seed(rate_in + 2 * rate_out))
    rs = StreamResampler(4, rate_in, rate_out, 3 * hop + 5, delayed=delayed)
    assert (rs.up, rs.down, rs.lag) == rc.GEOMETRY[rate_in, rate_out][:2] + rc.GEOMETRY[rate_in, rate_out][4:]
    tally = rc.Tally(LEDGER, "stream-delayed" if delayed else "stream")
    what = f"{rate_in}->{rate_out}" + (" delayed" if delayed else "")
    done, live = [], {}

    def start(row, label, offset=0):
        rs.open(row, offset)
        live[row] = Stream(row, label)

    def finish(row):
        s = live.pop(row)
        flush(rs, s)
        done.append(s)

    start(0, "row 0 throughout")
    start(2, "row 2 never pushed")
    finish(2)
    assert len(done[0].output()) == (rs.lag if delayed else 0)
    at = 0
    for i, n in enumerate(chunks):
        offsets, valid = {}, {}
        if i == 1:
            start(2, "row 2 shorter than the history")
            rs.end(2, 5)
            valid[2] = 5
        if i == 2:
            start(1, "row 1 opened mid-chunk", 3)
            offsets[1] = 3
        if i == 5:
            rs.end(1, 4)
            valid[1] = 4
        if i == 6:
            start(1, "row 1 reopened")
        push(rs, X[:, at:at + n], live, offsets, valid)
        at += n
        for row in valid:
            finish(row)
    for row in sorted(live):
        finish(row)
    assert [s.n for s in done] == [0, 5, 3 * hop + 5 + 1 + 4 + hop - 3, sum(chunks), hop + 3 * hop + 5]
    for s in done:
        judge_stream(rs, s, tally, what)
    tally.close(f"stream {what}")


def run_all_rows(rs, X, n):
    """Every row opened at once, X (B, L) pushed n samples at a time, every row flushed: (B, all of it) on the host."""
    for row in range(rs.B):
        rs.open(row)
    out = [[] for _ in range(rs.B)]
    for at in range(0, X.shape[1], n):
        y, counts = rs.push(X[:, at:at + n].to(DEV))
        for row in range(rs.B):
            out[row].append(host(y[row, :counts[row]]))
    return np.stack([np.concatenate(out[row] + [host(rs.flush(row))]) for row in range(rs.B)])


def library_taps(batch, rate_in, rate_out, max_in):
    """A StreamResampler on the taps the library designs itself: created through the C call, bvc_resampler_set_taps left out."""
    from bvcodec import _abi
    from bvcodec.streaming import StreamResampler
    rs = StreamResampler.__new__(StreamResampler)
    rs.lib, rs.dev = _abi.load(), torch.device(DEV)
    rs.B, rs.rate_in, rs.rate_out, rs.max_in = batch, rate_in, rate_out, max_in
    rs.fmt_in, rs.fmt_out, rs.delayed = "f32", "f32", False
    rs.up, rs.down, _, rs.lag = rc.geometry(rate_in, rate_out)
    rs.max_out, rs.running = rc.out_len(max_in, rs.up, rs.down), set()
    rs.handle = _abi.Handle(rs.lib.bvc_resampler_destroy)
    with torch.cuda.device(rs.dev):
        _abi.check_arg(rs.lib.bvc_resampler_create(batch, rate_in, rate_out, max_in, 0, 0, ctypes.byref(rs.handle)))
    rs._counts, rs._out = (ctypes.c_int32 * batch)(), None
    return rs


@pytest.mark.parametrize("rate_in,rate_out", ((16000, rc.FS), (rc.FS, 48000)))
def test_library_taps_give_the_handed_in_bits(rate_in, rate_out):
    """design_taps (csrc/resampler.hip) is numpy's design to a few units in the last place of a double: the float32 outputs are the
    same, and under the bar."""
    from bvcodec.streaming import StreamResampler
    hop = rate_in // 50
    X = torch.randn(3, 6 * hop, generator=torch.Generator().manual_seed(rate_in))
    want = run_all_rows(StreamResampler(3, rate_in, rate_out, hop), X, hop)
    got = run_all_rows(library_taps(3, rate_in, rate_out, hop), X, hop)
    v = rc.compare(got, rc.reference(X.numpy(), rate_in, rate_out), f"library taps {rate_in}->{rate_out}")
    LEDGER.add("stream", v)
    assert v.ok, v.message
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("B", (64, 65, 130))
def test_many_rows_open_at_once(B):
    """All rows opened in front of one push, each b % 5 samples into it: one, two and three update launches (64 rows each).  Then every
    third row is closed and NaN is what its input holds: the others go on as in a resampler where those rows never ran."""
    from bvcodec.streaming import StreamResampler
    rate_in, rate_out, n = 16000, rc.FS, 400
    X = torch.randn(B, 2 * n, generator=torch.Generator().manual_seed(B))
    tally = rc.Tally(LEDGER, "stream")
    closed = [b for b in range(B) if b % 3 == 0]
    runs = []
    for without in (False, True):
        rs = StreamResampler(B, rate_in, rate_out, n)
        live = {}
        for b in range(B):
            if not (without and b in closed):
                rs.open(b, b % 5)
                live[b] = Stream(b, f"row {b} of {B}")
        push(rs, X[:, :n], live, {b: b % 5 for b in live})
        for b in closed:
            rs.close(b)
            live.pop(b, None)
        push(rs, X[:, n:], live)
        runs.append(live)
    full, never = runs
    assert sorted(full) == sorted(never) == [b for b in range(B) if b % 3]
    for b, s in full.items():
        assert s.n == 2 * n - b % 5 and len(s.y) == 2
        tally.check(all(np.array_equal(bits(p), bits(q)) for p, q in zip(s.y, never[b].y)), f"row {b} of {B}: not what it is without rows {closed[:3]}...")
    for off in range(5):                                              # one reference per offset: rows of one length
        rows = [b for b in full if b % 5 == off]
        ref = rc.reference(np.stack([full[b].signal().numpy() for b in rows]), rate_in, rate_out)
        got = np.stack([full[b].output() for b in rows])
        tally.add(rc.compare(got, rc.Reference(ref.ref[:, :got.shape[1]], ref.tol[:, :got.shape[1]]), f"{B} rows, offset {off}"))
    tally.close(f"many rows B {B}")


def test_push_strides_and_offset():
    """x rows wider than n_in, y rows wider than n_fill and an offset into them: cells [y_offset, y_offset + n_fill) of each row are
    the plain push's, every other cell of the buffer keeps its NaN."""
    from bvcodec import _abi
    from bvcodec.streaming import StreamResampler
    rate_in, rate_out, B, n_in, xs, yoff = rc.FS, 48000, 3, 100, 107, 3
    up, down, _, lag = rc.geometry(rate_in, rate_out)
    n_fill = rc.out_len(n_in, up, down)
    ys = n_fill + yoff + 5
    x = torch.randn(B, n_in, generator=torch.Generator().manual_seed(9))
    plain = StreamResampler(B, rate_in, rate_out, n_in)
    rs = StreamResampler(B, rate_in, rate_out, n_in)
    for r in (plain, rs):
        for b in range(B):
            r.open(b)
    want, counts = plain.push(x.to(DEV))
    assert tuple(want.shape) == (B, n_fill) and int(counts[0]) == n_fill - lag
    X = torch.full((B, xs), NAN)
    X[:, :n_in] = x
    X = X.to(DEV)
    Y = torch.full((B * ys,), NAN, device=DEV)
    got_counts = rs.push_raw(_abi.addr(X), xs, n_in, _abi.addr(Y), ys, yoff, torch.cuda.current_stream(DEV).cuda_stream)
    assert got_counts == [int(c) for c in counts]
    Y = Y.view(B, ys)
    assert torch.equal(Y[:, yoff:yoff + n_fill], want) and bool(torch.isfinite(want).all()) and bool(want.any())
    assert bool(torch.isnan(Y[:, :yoff]).all()) and bool(torch.isnan(Y[:, yoff + n_fill:]).all())
    with pytest.raises(ValueError):
        rs.push_raw(_abi.addr(X), n_in - 1, n_in, _abi.addr(Y), ys, yoff, torch.cuda.current_stream(DEV).cuda_stream)
    with pytest.raises(ValueError):
        rs.push_raw(_abi.addr(X), xs, n_in, _abi.addr(Y), n_fill - 1, 0, torch.cuda.current_stream(DEV).cuda_stream)


@pytest.mark.parametrize("rate_in,rate_out", ((48000, rc.FS), (rc.FS, 48000)))
def test_largest_push_the_lds_takes(rate_in, rate_out):
    """max_in = 16384 - H: history and chunk fill the 64 KiB exactly.  One full chunk against float64; one sample more is refused."""
    from bvcodec.streaming import StreamResampler
    H = rc.history(rate_in, rate_out)
    max_in = rc.LDS_FLOATS - H
    with pytest.raises(ValueError, match="64 KiB"):
        StreamResampler(2, rate_in, rate_out, max_in + 1)
    rs = StreamResampler(2, rate_in, rate_out, max_in)
    X = torch.randn(2, max_in, generator=torch.Generator().manual_seed(H))
    live = {}
    for b in range(2):
        rs.open(b)
        live[b] = Stream(b, f"row {b}")
    push(rs, X, live)
    tally = rc.Tally(LEDGER, "stream")
    for s in live.values():
        flush(rs, s)
        judge_stream(rs, s, tally, f"LDS limit {rate_in}->{rate_out}")
    tally.close(f"LDS limit {rate_in}->{rate_out}")


# ---------------------------------------------------------------------------------------------- s16
def s16_runs(rate_in, rate_out, delayed, x16, n):
    """The four format combinations on the same signal: (f32 -> f32, f32 -> s16, s16 -> f32, s16 -> s16) outputs, whole streams."""
    from bvcodec.streaming import StreamResampler, pcm_s16_to_f32
    xf = pcm_s16_to_f32(x16)
    out = []
    for fi, fo in (("f32", "f32"), ("f32", "s16"), ("s16", "f32"), ("s16", "s16")):
        rs = StreamResampler(x16.shape[0], rate_in, rate_out, n, fmt_in=fi, fmt_out=fo, delayed=delayed)
        out.append(run_all_rows(rs, xf if fi == "f32" else x16, n))
    return xf, out


@pytest.mark.parametrize("delayed", (False, True), ids=("plain", "delayed"))
@pytest.mark.parametrize("rate_in,rate_out", rc.S16_PAIRS)
def test_s16_in_and_out(rate_in, rate_out, delayed):
    """+-full-scale square waves, whose overshoot saturates: the s16 a resampler stores is pcm_f32_to_s16 of the float32 it would have
    stored, s16 input is x / 32768, and against float64 |q - clamp(32768 ref, -32768, 32767)| <= 0.5 + 32768 bar; no sample wraps."""
    from bvcodec.streaming import pcm_f32_to_s16
    hop = rate_in // 50
    lag = rc.GEOMETRY[rate_in, rate_out][4] if delayed else 0
    x16 = pcm_f32_to_s16(rc.square(3, 4 * hop + 17, seed=rate_in % 7))
    assert set(np.unique(x16.numpy())) == {-32768, 32767}
    xf, (ff, fs, sf, ss) = s16_runs(rate_in, rate_out, delayed, x16, hop)
    assert ff.dtype == sf.dtype == np.float32 and fs.dtype == ss.dtype == np.int16
    assert np.array_equal(fs, pcm_f32_to_s16(torch.from_numpy(ff)).numpy())
    assert np.array_equal(bits(sf), bits(ff)) and np.array_equal(ss, fs)
    assert not ff[:, :lag].any() and not fs[:, :lag].any()
    ref = rc.reference(xf.numpy(), rate_in, rate_out)
    tally = rc.Tally(LEDGER, "s16")
    what = f"s16 {rate_in}->{rate_out}" + (" delayed" if delayed else "")
    tally.add(rc.compare(ff[:, lag:], ref, what + " f32"))
    q = fs[:, lag:].astype(np.float64)
    want = rc.s16_expected(ref.ref)
    ratio = np.abs(q - want) / (0.5 + 32768.0 * ref.tol)
    b, m = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    tally.check(ratio[b, m] <= 1.0, f"{what}: |q - clamp(32768 ref)| / (0.5 + 32768 bar) = {ratio[b, m]:.4f} at (row {b}, output {m}): q {q[b, m]}, "
                                    f"float64 {32768.0 * ref.ref[b, m]!r}")
    print(f"RESAMPLE {what} largest |q - clamp(32768 ref)| / (0.5 + 32768 bar) = {ratio.max():.4f}; {int((q == 32767).sum())} at 32767, "
          f"{int((q == -32768).sum())} at -32768 of {q.size}", flush=True)
    assert (q == 32767).any() and (q == -32768).any() and np.abs(ref.ref).max() > 1.0
    loud = np.abs(32768.0 * ref.ref) > 1.0
    tally.check(np.array_equal(np.sign(q[loud]), np.sign(ref.ref[loud])), f"{what}: a sample has the wrong sign (wrapped)")
    tally.close(what)


@pytest.mark.parametrize("delayed", (False, True), ids=("plain", "delayed"))
@pytest.mark.parametrize("rate_in,rate_out", rc.S16_PAIRS)
def test_s16_of_what_is_not_finite(rate_in, rate_out, delayed):
    """NaN, +Inf and -Inf in the input, further apart than the history: the stored s16 is 0, 32767 and -32768 where the float64 walk is
    NaN, +Inf and -Inf (the taps have both signs, and zeros in front), finite and under the s16 bar everywhere else."""
    from bvcodec.streaming import StreamResampler
    up, down, h, lag = rc.geometry(rate_in, rate_out)
    H, hop = rc.history(rate_in, rate_out), rate_in // 50
    L = 4 * hop
    x = 0.2 * torch.randn(2, L, generator=torch.Generator().manual_seed(rate_out))
    spots = (hop // 2, hop // 2 + 3 * H, hop // 2 + 6 * H)
    assert spots[2] + 3 * H < L
    x[:, spots[0]], x[0, spots[1]], x[0, spots[2]], x[1, spots[1]], x[1, spots[2]] = NAN, float("inf"), float("-inf"), float("-inf"), float("inf")
    got = run_all_rows(StreamResampler(2, rate_in, rate_out, hop, fmt_out="s16", delayed=delayed), x, hop)
    lead = lag if delayed else 0
    assert got.dtype == np.int16 and not got[:, :lead].any()
    q = got[:, lead:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = rc.walk(x.numpy(), up, down, h, lag)
    assert q.shape == w.shape and np.isnan(w).any() and (w == np.inf).any() and (w == -np.inf).any()
    assert (q[np.isnan(w)] == 0).all() and (q[w == np.inf] == 32767).all() and (q[w == -np.inf] == -32768).all()
    fin = np.isfinite(w)
    tol = rc.reference(np.nan_to_num(x.numpy(), nan=0.0, posinf=0.0, neginf=0.0), rate_in, rate_out).tol
    assert fin.mean() > 0.5 and (np.abs(q[fin] - rc.s16_expected(w[fin])) <= 0.5 + 32768.0 * tol[fin]).all()


# ---------------------------------------------------------------------------------------------- peak normalisation
@pytest.mark.parametrize("L", (1, 1023, 1024, 1025, 5000))
def test_peak_normalize_is_the_rounded_quotient(L):
    """Rows with the peak at the first, the last and a middle sample, a negative peak, zeros, the 2^-100 scale and plain noise: numpy's
    float32 x / max|x| with equality (the correctly rounded quotient), the peak itself exactly +-1, zeros stay zeros."""
    from bvcodec import preprocess
    x = np.random.default_rng(L).standard_normal((7, L)).astype(np.float32)
    peak = np.float32(np.abs(x).max() + 1.0)
    x[0, 0], x[1, L - 1], x[2, L // 2], x[3, L // 2] = peak, peak, peak, -peak
    x[4] = 0.0
    x[5] *= np.float32(rc.SMALL)
    mx = np.abs(x).max(axis=1, keepdims=True)
    want = np.where(mx > 0, x / np.where(mx > 0, mx, np.float32(1.0)), x).astype(np.float32)
    got = host(preprocess.peak_normalize(torch.from_numpy(x).to(DEV)))
    differ = bits(got) != bits(want)
    print(f"RESAMPLE peak_normalize L {L}: {int(differ.sum())} of {got.size} elements are not numpy's float32 quotient", flush=True)
    assert not differ.any(), (np.argwhere(differ)[:5], got[differ][:5], want[differ][:5])
    assert got[0, 0] == 1.0 and got[1, L - 1] == 1.0 and got[2, L // 2] == 1.0 and got[3, L // 2] == -1.0 and not got[4].any()
    assert (np.abs(got).max(axis=1)[[0, 1, 2, 3, 5, 6]] == 1.0).all()


def test_peak_normalize_keeps_a_nan_in_place():
    """fmaxf drops a NaN: the row is divided by its largest finite magnitude, and the NaN stays where it was."""
    from bvcodec import preprocess
    x = np.random.default_rng(3).standard_normal((2, 2049)).astype(np.float32)
    x[0, 1500] = np.nan
    fin = np.where(np.isnan(x), np.float32(0.0), x)
    want = (x / np.abs(fin).max(axis=1, keepdims=True)).astype(np.float32)
    got = host(preprocess.peak_normalize(torch.from_numpy(x).to(DEV)))
    assert np.isnan(got[0, 1500]) and int(np.isnan(got).sum()) == 1
    keep = ~np.isnan(x)
    assert np.array_equal(bits(got[keep]), bits(want[keep])) and np.abs(got[keep]).max() == 1.0


# ---------------------------------------------------------------------------------------------- the ledger
def test_resample_parity_ledger():
    """Prints the PARITY lines of everything this module compared so far (profiles/resample_parity.md); fails if any comparison did."""
    print(flush=True)
    LEDGER.close()
