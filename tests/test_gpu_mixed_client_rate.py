"""Streaming sessions whose slots each speak their own client rate (``StreamingCodec(client_rate=(...))``) and the multi-rate resampler
under them (``MultiRateResampler``, bvc_resampler_*_multi).  The contract is equality with ``torch.equal``: a row of the multi-rate
resampler gives what ``StreamResampler`` at its rate gives on the same chunks (and after the flush the offline ``resample_poly``); a slot
of a mixed-rate session gives - packets, codes, samples, counts - what the same stream gives in a single-rate session at its rate,
driven alone with the same events.  Needs the MI355X."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gpu_sessions import DEV

pytestmark = pytest.mark.gpu
FS = 22050
RATES7 = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
H_DIM = 64                                                            # the small coder: the tests are about the session's boundary


@pytest.fixture(scope="module")
def model():
    from gpu_common import make_model
    return make_model(True, H_DIM)[0]


def offline(x, rate_in, rate_out):
    from bvcodec import preprocess
    return preprocess.resample_poly(x[None].to(DEV), rate_out, rate_in)[0]


def garbage(B, n, dtype=torch.float32):
    """What no row may read: NaN, Inf and 1e38 in turn (s16: a constant that would be heard)."""
    if dtype == torch.int16:
        return torch.full((B, n), 12345, dtype=dtype)
    x = torch.empty(B, n)
    x[:, 0::3], x[:, 1::3], x[:, 2::3] = float("nan"), float("inf"), 1e38
    return x


# ---------------------------------------------------------------------------------------------- the resampler alone
def chunk_table(direction, pushes=9):
    """n[i][p]: the chunk of rate i in push p - (1, 7, hop, 3 hop + 5) over and over, rotated by i, with one push of no samples at p = i + 1:
    every launch mixes lengths, and in pushes 1 .. 7 one rate pushes nothing.  hop: 20 ms on the input side."""
    table = []
    for i, rate in enumerate(RATES7):
        hop = (rate if direction == "in" else FS) // 50
        seq = [(1, 7, hop, 3 * hop + 5)[(p + i) % 4] for p in range(pushes - 1)]
        table.append(seq[:i + 1] + [0] + seq[i + 1:])
    return table


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("direction", ["in", "out"])
def test_rows_equal_the_single_rate_resampler(direction, delayed):
    """Nine rows: one at each of the seven rates, one more at 8 kHz (it opens at push 2, 3 samples into its chunk) and one more at 48 kHz
    (it ends with 2 samples of push 3, is flushed and opens again at 16 kHz before push 5: nothing of its history leaks).  Every push's
    counts and samples are those of a StreamResampler at the row's rate fed the same chunks, the block behind a row's samples is zeros
    up to the call's longest, idle rows (their input NaN, Inf, 1e38) give zeros, and after the flush every stream is the offline call."""
    from bvcodec.streaming import MultiRateResampler, StreamResampler
    n_of = chunk_table(direction)
    pushes = len(n_of[0])
    max_in = [max(n) for n in n_of]
    pair = lambda rate: (rate, FS) if direction == "in" else (FS, rate)
    multi = MultiRateResampler(9, RATES7, FS, direction, max_in, delayed=delayed)
    S = lambda row, rate, t_open, offset=0, t_end=None, n_valid=0: SimpleNamespace(
        row=row, rate=rate, i=RATES7.index(rate), t_open=t_open, offset=offset, t_end=t_end, n_valid=n_valid, x=[], y=[], local=None, done=False)
    streams = [S(i, r, 0) for i, r in enumerate(RATES7)] + [S(7, 8000, 2, offset=3), S(8, 48000, 0, t_end=3, n_valid=2), S(8, 16000, 5)]
    assert n_of[0][2] >= 3 and n_of[6][3] >= 2
    single = {}
    for i, rate in enumerate(RATES7):                                 # the reference: one single-rate resampler per rate, a row per stream
        mine = [s for s in streams if s.rate == rate]
        for local, s in enumerate(mine):
            s.local = local
        single[rate] = StreamResampler(len(mine), *pair(rate), max_in[i], delayed=delayed)
    g = torch.Generator().manual_seed(17 + delayed)

    def finish(s):
        a, b = multi.flush(s.row).clone(), single[s.rate].flush(s.local).clone()
        assert torch.equal(a, b) and a.numel() <= multi.lag[s.i], (s.row, s.rate)
        got, x = torch.cat(s.y + [a]), torch.cat(s.x)
        ref = offline(x, *pair(s.rate))
        if delayed:
            ref = torch.cat([torch.zeros(multi.lag[s.i], device=DEV), ref])
        assert torch.equal(got, ref), (s.row, s.rate, got.numel(), ref.numel())
        s.done = True

    for p in range(pushes):
        n = [n_of[i][p] for i in range(7)]
        x = garbage(9, max(max(n), 1))
        live = []
        for s in streams:
            if s.done or s.t_open > p:
                continue
            if s.t_open == p:
                multi.open(s.row, s.rate, s.offset)
                single[s.rate].open(s.local, s.offset)
            lo, hi = (s.offset if s.t_open == p else 0), (s.n_valid if s.t_end == p else n[s.i])
            if s.t_end == p:
                multi.end(s.row, s.n_valid)
                single[s.rate].end(s.local, s.n_valid)
            x[s.row, lo:hi] = torch.randn(hi - lo, generator=g)
            s.x.append(x[s.row, lo:hi].clone())
            live.append(s)
        x = x.to(DEV)
        y, counts = multi.push(x, n)
        assert y.shape == (9, multi.out_len(n)) and counts.dtype == torch.int64
        busy = set()
        for i, rate in enumerate(RATES7):
            rows = [s.row for s in streams if s.rate == rate]
            yr, cr = single[rate].push(x[rows][:, :n[i]].contiguous())
            for s in live:
                if s.rate == rate:
                    c = int(counts[s.row])
                    assert c == int(cr[s.local]), (p, s.row, rate)
                    assert torch.equal(y[s.row, :c], yr[s.local, :c]), (p, s.row, rate)
                    assert not bool(y[s.row, c:].any())
                    s.y.append(y[s.row, :c].clone())
                    busy.add(s.row)
        for row in set(range(9)) - busy:                              # idle rows: zeros, whatever their input holds
            assert int(counts[row]) == 0 and not bool(y[row].any())
        assert bool(torch.isfinite(y).all())
        for s in live:
            if s.t_end == p:
                finish(s)
    assert sum(n_of[0]) > 1000 and len([s for s in streams if not s.done]) == 9
    for s in streams:
        if not s.done:
            finish(s)
    for bad in (lambda: multi.open(0, 11025), lambda: multi.flush(3), lambda: multi.push(x, n[:6]), lambda: multi.push(x, [m + 10000 for m in n]),
                lambda: MultiRateResampler(2, (8000, 8000), FS, max_in=16), lambda: MultiRateResampler(2, range(1000, 10000, 1000), FS, max_in=16)):
        with pytest.raises(ValueError):
            bad()


def test_s16_strides_offset_and_the_wrong_kind_of_call():
    """s16 in and out through push_raw with x_row_stride, y_row_stride and y_offset larger than needed: the rows are the s16
    StreamResampler's at their rates and nothing outside a row's block is written.  Then the calls of the other kind on either kind of
    handle: BVC_EINVAL, a message that names the right call, and the object goes on as if nothing had been asked."""
    from bvcodec import _abi
    from bvcodec.streaming import MultiRateResampler, StreamResampler
    rates, n = (8000, 44100, 48000), (160, 882, 959)
    row_rate = (48000, 8000, 44100, 8000)
    multi = MultiRateResampler(5, rates, FS, "in", (160, 882, 960), "s16", "s16")          # row 4 stays idle
    single = {r: StreamResampler(1, r, FS, 960, "s16", "s16") for r in set(row_rate)}
    lib, s = multi.lib, torch.cuda.current_stream().cuda_stream
    i32s, r8 = ctypes.c_int32 * 3, single[8000]
    taps = (ctypes.c_double * 8)()
    wrong = {"bvc_resampler_open_rate": lambda: lib.bvc_resampler_open(multi.handle, 4, 0),
             "bvc_resampler_push_multi": lambda: lib.bvc_resampler_push(multi.handle, 1, 8, 1, 1, 8, 0, None, s),
             "bvc_resampler_set_taps_rate": lambda: lib.bvc_resampler_set_taps(multi.handle, taps, 8),
             "bvc_resampler_open": lambda: lib.bvc_resampler_open_rate(r8.handle, 0, 0, 0),
             "bvc_resampler_push": lambda: lib.bvc_resampler_push_multi(r8.handle, 1, 8, i32s(1, 1, 1), 1, 8, 0, None, s),
             "bvc_resampler_set_taps": lambda: lib.bvc_resampler_set_taps_rate(r8.handle, 0, taps, 8)}
    xs, ys, yoff = 1000, 500, 7
    for rnd in range(3):
        X = torch.randint(-20000, 20000, (5, xs), generator=torch.Generator().manual_seed(rnd), dtype=torch.int16)
        X[4] = 12345
        if rnd == 0:
            for row, rate in enumerate(row_rate):
                multi.open(row, rate)
            for r in single.values():
                r.open(0)
        for right, call in wrong.items():
            assert call() == -1 and lib.bvc_last_error().endswith(b"takes " + right.encode()), right
        X = X.to(DEV)
        Y = torch.full((5, ys), 77, dtype=torch.int16, device=DEV)
        counts = multi.push_raw(_abi.addr(X, torch.int16), xs, n, _abi.addr(Y, torch.int16), ys, yoff, s)
        n_max = multi.out_len(n)
        assert n_max == 441 and counts[4] == 0
        assert bool((Y[:, :yoff] == 77).all()) and bool((Y[:, yoff + n_max:] == 77).all())
        assert not bool(Y[4, yoff:yoff + n_max].any())
        used = set()
        for row, rate in enumerate(row_rate):
            if rate in used:                                          # (the second 8 kHz row: a resampler of its own would do; one row is checked per rate)
                continue
            used.add(rate)
            yr, cr = single[rate].push(X[row:row + 1, :n[rates.index(rate)]].contiguous())
            c = counts[row]
            assert c == int(cr[0]) > 0 and torch.equal(Y[row, yoff:yoff + c], yr[0, :c]) and not bool(Y[row, yoff + c:yoff + n_max].any())
            assert yr.dtype == torch.int16
    for bad in (lambda: multi.push_raw(_abi.addr(X, torch.int16), 881, n, _abi.addr(Y, torch.int16), ys, 0, s),      # rows too narrow
                lambda: multi.push_raw(_abi.addr(X, torch.int16), xs, n, _abi.addr(Y, torch.int16), 440, 0, s),
                lambda: multi.push_raw(_abi.addr(X, torch.int16), xs, (161, 1, 1), _abi.addr(Y, torch.int16), ys, 0, s),
                lambda: multi.end(0, 961), lambda: multi.end(1, 161)):
        with pytest.raises(ValueError):
            bad()
    multi.end(1, 160)


ONE_RATE_CASES = [(r, d, delayed, "f32") for r in (8000, 48000, 22050) for d in ("in", "out") for delayed in (False, True)]
ONE_RATE_CASES.append((48000, "in", True, "s16"))


@pytest.mark.parametrize("rate,direction,delayed,fmt", ONE_RATE_CASES)
def test_one_listed_rate_equals_the_single_rate_resampler(rate, direction, delayed, fmt):
    """The table of one rate and the single-rate object share everything but the kernel's entry point: a MultiRateResampler that lists
    only `rate` and a StreamResampler at it go through one ragged script - max_in one 20 ms hop of the input side; row 0 opens 3 samples
    into push 0, row 1 at its start; chunks of a hop, 0, 1, 7, a hop (row 1 ends with 5 samples of it and is flushed), a hop less one
    (row 1 opens again 2 samples in), 33 and a hop; then both rows are flushed.  Row 2 is never opened and its input is NaN, Inf and 1e38
    (s16: a constant).  Every push's whole block - the samples, the zeros behind a row's count, the idle row's zeros - its counts, and
    every flush are equal."""
    from bvcodec.streaming import MultiRateResampler, StreamResampler
    rate_in, rate_out = (rate, FS) if direction == "in" else (FS, rate)
    hop = rate_in // 50
    dtype = torch.int16 if fmt == "s16" else torch.float32
    multi = MultiRateResampler(3, (rate,), FS, direction, hop, fmt, fmt, delayed=delayed)
    single = StreamResampler(3, rate_in, rate_out, hop, fmt, fmt, delayed=delayed)
    assert multi.max_in == [single.max_in] and multi.lag == [single.lag] and multi.max_out == [single.max_out]
    g = torch.Generator().manual_seed(rate // 50 + delayed)

    def both(call, *args):
        return call(multi, *args), call(single, *args)

    def flush(row):
        a, b = both(lambda rs: rs.flush(row).clone())
        assert a.dtype == b.dtype == dtype and a.shape == b.shape and torch.equal(a, b) and a.numel() <= single.lag, (row, a.shape, b.shape)
        return a.numel()

    start = {0: 3, 1: 0}                                              # row -> where its stream starts in the coming chunk
    multi.open(0, rate, 3), single.open(0, 3), multi.open(1, rate), single.open(1)
    flushed = []
    for p, n in enumerate((hop, 0, 1, 7, hop, hop - 1, 33, hop)):
        end = {}
        if p == 4:
            both(lambda rs: rs.end(1, 5))
            end[1] = 5
        if p == 5:
            multi.open(1, rate, 2), single.open(1, 2)
            start[1] = 2
        x = garbage(3, n, dtype)
        for row in (0, 1):
            lo, hi = min(start.get(row, 0), n), end.get(row, n)
            x[row, lo:hi] = (torch.randint(-20000, 20000, (hi - lo,), generator=g, dtype=dtype) if fmt == "s16"
                             else torch.randn(hi - lo, generator=g))
        start = {}
        x = x.to(DEV)
        (ym, cm), (ys, cs) = multi.push(x, [n]), single.push(x)
        assert ym.shape == ys.shape == (3, -(-n * single.up // single.down)) and ym.dtype == ys.dtype == dtype, (p, ym.shape, ys.shape)
        assert torch.equal(cm, cs) and torch.equal(ym, ys), (p, cm, cs)
        assert int(cm[2]) == 0 and not bool(ym[2].any())
        for row in (0, 1):
            assert not bool(ym[row, int(cm[row]):].any()), (p, row)
        if fmt == "f32":
            assert bool(torch.isfinite(ym).all())
        if p == 4:
            flushed.append(flush(1))
    flushed += [flush(0), flush(1)]
    assert any(flushed) and int(cm[0]) > 0
    for rs in (multi, single):
        with pytest.raises(ValueError):
            rs.flush(2)


# ---------------------------------------------------------------------------------------------- sessions
def speech(n, seed):
    from bvcodec import synth
    return synth.synthetic_speech(1, n, seed=seed, kind="speech")[0].float()


def stream(slot, rate, t_open, t_fin=None, n_last=0, t_close=None, target=None):
    """One stream of a schedule: it lives in `slot` from push t_open on - to the end, to its finish in front of push t_fin with n_last
    client samples, or to its close in front of push t_close."""
    return SimpleNamespace(slot=slot, rate=rate, t_open=t_open, t_fin=t_fin, n_last=n_last, t_close=t_close, target=target,
                           seed=500 + 16 * slot + t_open)


def drive(model, direction, fmt, client_rate, streams, slots, pushes, vbr=None):
    """One send or duplex session with `client_rate` (a tuple: mixed), stream i of `streams` in slot slots[i].  A stream's client
    samples are speech of its own seed; everything else a row holds - in front of a stream, behind its finish, behind the slot's
    own hop - is garbage.  Returns per stream the record of every push of its life: the delay, then per push (slot_frames, slot_state,
    the tick's tensors cut to the slot's frames and samples)."""
    from bvcodec.streaming import StreamingCodec, pcm_f32_to_s16
    mixed = isinstance(client_rate, tuple)
    B = max(slots) + 1
    sc = StreamingCodec(model, B, 3000, hop=441 if mixed else 441 * client_rate // FS, open_all=False, direction=direction,
                        client_rate=client_rate, sample_format=fmt, vbr=vbr)
    dtype = torch.int16 if fmt == "s16" else torch.float32
    assert sc.hop == 441 * max(client_rate if mixed else (client_rate,)) // FS
    records = [[] for _ in streams]
    signals = []
    for i, s in enumerate(streams):
        x = speech((pushes - s.t_open) * 441 * s.rate // FS, s.seed) * 0.9
        signals.append(pcm_f32_to_s16(x) if fmt == "s16" else x)
    for t in range(pushes):
        for s, slot in zip(streams, slots):
            if s.t_close == t:
                sc.close(slot)
        for s, slot in zip(streams, slots):
            if s.t_fin == t:
                sc.finish(slot, s.n_last)
        x = garbage(B, sc.hop, dtype)
        for i, (s, slot) in enumerate(zip(streams, slots)):
            hop = 441 * s.rate // FS
            if s.t_open == t:
                how = dict(target=s.target) if vbr is not None else dict(bitrate=3000)
                records[i].append(sc.open(slot, client_rate=s.rate, **how) if mixed else sc.open(slot, **how))
                assert sc.slot_rate(slot) == s.rate and sc.slot_hop(slot) == hop
            if s.t_open <= t and (s.t_close is None or t < s.t_close) and (s.t_fin is None or t <= s.t_fin):
                n = s.n_last if s.t_fin == t else hop
                x[slot, :n] = signals[i][(t - s.t_open) * hop:(t - s.t_open) * hop + n]
        res = sc.push(x.to(DEV))
        for i, (s, slot) in enumerate(zip(streams, slots)):
            if s.t_open <= t and (s.t_close is None or t < s.t_close):
                first, count, f0 = frames = sc.slot_frames(slot)
                cut = [r[slot, first:first + max(count, 0)].clone() for r in res[:1 if direction == "duplex" else 2]]
                if direction == "duplex":
                    cut += [res[1][slot, :int(res[2][slot])].clone(), res[2][slot].clone()]
                    assert res[1].dtype == dtype
                    if mixed:                                         # n_max is the fastest listed rate's
                        assert res[1].shape[1] == -(-res[0].shape[1] * 256 * max(client_rate) // FS)
                if vbr is not None:
                    cut += [sc.last_bits[slot, first:first + max(count, 0)].clone(), sc.last_sizes[slot, first:first + max(count, 0)].clone()]
                records[i].append((frames, sc.slot_state(slot), cut))
    torch.cuda.synchronize()
    model.check_status()
    return sc, records


def same_records(a, b, what):
    assert len(a) == len(b) and a[0] == b[0], (what, "delay", a[0], b[0])
    for t, ((fa, sa, ca), (fb, sb, cb)) in enumerate(zip(a[1:], b[1:])):
        assert fa == fb and sa == sb and len(ca) == len(cb), (what, t, fa, fb, sa, sb)
        for k, (u, v) in enumerate(zip(ca, cb)):
            assert u.dtype == v.dtype and torch.equal(u, v), (what, t, k)


def against_sessions_alone(model, direction, fmt, rates, streams, pushes, vbr=None):
    """The schedule in one mixed-rate session, then every stream alone in a single-rate session at its rate with the same events at the
    same pushes: the records are equal.  Returns the mixed session and its records."""
    sc, mixed = drive(model, direction, fmt, tuple(rates), streams, [s.slot for s in streams], pushes, vbr)
    for i, s in enumerate(streams):
        _, alone = drive(model, direction, fmt, s.rate, [s], [0], pushes, vbr)
        assert len(mixed[i]) > 1
        same_records(mixed[i], alone[0], (i, s.rate))
    return sc, mixed


@pytest.mark.parametrize("fmt,rates", [("f32", (8000, 16000, 48000)), ("s16", (8000, 16000, 48000, 22050))])
def test_send_session_slots_equal_sessions_of_their_rate(model, fmt, rates):
    """Five slots, hop 441, 12 pushes; slots open at pushes 0, 0, 3 and 5 at different rates.  Slot 0 (8 kHz) finishes with 123 client
    samples in front of push 8; slot 1 (48 kHz) with a hop less one sample in front of push 7, whose flushed tail spills into push 8;
    slot 4 opens at 16 kHz, is closed in front of push 6 and opens again at 8 kHz (s16: at 22050).  Packets, codes, frames and states
    of every stream are those of the single-rate send session at its rate, driven alone."""
    from bvcodec.streaming import client_finish_plan
    again = 22050 if 22050 in rates else 8000
    streams = [stream(0, 8000, 0, t_fin=8, n_last=123), stream(1, 48000, 0, t_fin=7, n_last=959), stream(2, 16000, 3), stream(3, 48000, 5),
               stream(4, 16000, 0, t_close=6), stream(4, again, 6)]
    assert client_finish_plan(8 * 160 + 123, 160, 8000)[1] == 8 and client_finish_plan(7 * 960 + 959, 960, 48000)[1] == 8      # fits; spills
    sc, rec = against_sessions_alone(model, "send", fmt, rates, streams, 12)
    assert rec[0][-1][1] == "idle" and rec[1][-1][1] == "idle" and rec[2][-1][1] == "running"
    assert sum(r[0][1] for r in rec[0][1:]) == (28 + -(-(8 * 160 + 123) * FS // 8000)) // 256          # all num_frames(len(S)) frames
    assert sc.slot_lag(0) == 28 and sc.slot_lag(1) == 11 and sc.slot_rate(4) == again and sc.hop == 960
    with pytest.raises(ValueError, match="slot_lag"):
        sc.lag
    for bad in (lambda: sc.open(0, 3000), lambda: sc.open(0, 3000, client_rate=44100), lambda: sc.push(torch.zeros(5, 441, device=DEV)),
                lambda: sc.finish(2, 321), lambda: sc.slot_hop(5)):
        with pytest.raises((ValueError, AssertionError)):
            bad()
    sc.finish(2, 320)


def test_open_takes_a_rate_on_mixed_sessions_only(model):
    from bvcodec.streaming import StreamingCodec
    for rate in (None, 16000):
        sc = StreamingCodec(model, 2, 3000, hop=441 if rate is None else 320, open_all=False, direction="send", client_rate=rate)
        with pytest.raises(ValueError, match="client_rate"):
            sc.open(0, 3000, client_rate=16000)
        assert sc.open(0, 3000) == 0
    sc = StreamingCodec(model, 3, 3000, client_rate=(16000, 8000), direction="send")      # open_all: every slot at the first listed rate
    assert [sc.slot_rate(b) for b in range(3)] == [16000] * 3 and sc.hop == 320 and sc.slot_state(2) == "running"
    assert sc.push(torch.zeros(3, 320, device=DEV))[0].shape[0] == 3


def test_receive_session_slots_equal_sessions_of_their_rate(model):
    """Packets of a plain send session, 5 % of them dropped, conceal="prior"; three slots at 8, 16 and 48 kHz opened at ticks 0, 1 and
    3, slot 0 closed at the end of its stream and opened again at 48 kHz.  Every tick's samples and counts of every slot are those of
    the single-rate receive session at its rate, driven alone."""
    from bvcodec.streaming import StreamingCodec
    rates, hop, pushes, k = (8000, 16000, 48000), 441, 24, 2
    x = torch.stack([speech(pushes * hop, 200 + b) * 0.9 for b in range(2)]).to(DEV)
    snd = StreamingCodec(model, 2, 3000, hop=hop, direction="send")
    packets = torch.cat([snd.push(x[:, t * hop:(t + 1) * hop])[0].clone() for t in range(pushes)], 1).cpu()
    F = packets.shape[1] // k * k
    present = (torch.rand(2, F, generator=torch.Generator().manual_seed(9)) >= 0.05).to(torch.uint8)
    assert 0 < int((present == 0).sum()) < F // 4
    n_ticks = F // k
    # (slot, rate, the wire's stream, first tick, ticks)
    plan = [(0, 8000, 0, 0, 9), (1, 16000, 1, 1, n_ticks - 1), (2, 48000, 0, 3, n_ticks - 3), (0, 48000, 1, 10, n_ticks - 10)]

    def run(client_rate, mine, slots):
        mixed = isinstance(client_rate, tuple)
        B = max(slots) + 1
        sc = StreamingCodec(model, B, 3000, direction="recv", conceal="prior", open_all=False, client_rate=client_rate)
        out = [[] for _ in mine]
        for t in range(n_ticks):
            pk, pr = torch.zeros(B, k, packets.shape[2], dtype=torch.uint8), torch.zeros(B, k, dtype=torch.uint8)
            for (_, rate, wire, t0, n), slot in zip(mine, slots):
                if t == t0 + n:
                    sc.close(slot)
            for (_, rate, wire, t0, n), slot in zip(mine, slots):
                if t == t0:
                    assert (sc.open(slot, 3000, client_rate=rate) if mixed else sc.open(slot, 3000)) == 0
                if t0 <= t < t0 + n:
                    f = (t - t0) * k
                    pk[slot], pr[slot] = packets[wire, f:f + k], present[wire, f:f + k]
            wav, counts = sc.push_packets(pk.to(DEV), pr.to(DEV))
            assert counts.dtype == torch.int64 and counts.device.type == "cpu" and wav.shape[0] == B
            for i, ((_, rate, wire, t0, n), slot) in enumerate(zip(mine, slots)):
                if t0 <= t < t0 + n:
                    out[i].append((int(counts[slot]), wav[slot, :int(counts[slot])].clone(), sc.slot_frames(slot)))
                    assert not bool(wav[slot, int(counts[slot]):].any())
            if mixed:
                assert wav.shape[1] == -(-256 * k * 320 // 147)       # n_max is the fastest listed rate's
        torch.cuda.synchronize()
        return out

    mixed = run(rates, plan, [p[0] for p in plan])
    for i, p in enumerate(plan):
        alone = run(p[1], [p], [0])[0]
        assert len(alone) == len(mixed[i]) == p[4] and sum(c for c, _, _ in alone) > 0
        for t, ((ca, wa, fa), (cb, wb, fb)) in enumerate(zip(mixed[i], alone)):
            assert ca == cb and fa == fb and torch.equal(wa, wb), (i, t, ca, cb)
    model.check_status()


def test_duplex_session_slots_equal_sessions_of_their_rate(model):
    """(16000, 44100): slot 1 opens before push 2 (its frame 0 waits for the session's grid, so its output resampler starts inside a
    tick), slot 2 finishes with 300 samples.  Codes, the client's samples and their counts per push are the single-rate duplex session's."""
    streams = [stream(0, 44100, 0), stream(1, 16000, 2), stream(2, 44100, 4, t_fin=10, n_last=300), stream(3, 16000, 0, t_close=5),
               stream(3, 44100, 5)]
    sc, rec = against_sessions_alone(model, "duplex", "f32", (16000, 44100), streams, 14)
    assert rec[1][0] > 0 and rec[2][-1][1] == "idle" and sum(int(r[2][2]) for r in rec[0][1:]) > 10000


def test_vbr_send_session_slots_equal_sessions_of_their_rate(model):
    """(8000, 48000) with the session choosing every frame's rate: packets, codes, bit counts and sizes per slot are the single-rate vbr
    send session's."""
    vbr = dict(bitrates=(1500, 3000, 6000), target=0.35)
    streams = [stream(0, 8000, 0, target=0.2), stream(1, 48000, 0, t_fin=8, n_last=500), stream(2, 48000, 2, target=1e6), stream(3, 8000, 3)]
    sc, rec = against_sessions_alone(model, "send", "f32", (8000, 48000), streams, 11, vbr=vbr)
    bits = torch.cat([r[2][2] for r in rec[0][1:]] + [r[2][2] for r in rec[2][1:]])
    assert len(set(bits.tolist())) > 1                                # (the ladder is in use: a target of 1e6 is met by the lowest rung)


# ---------------------------------------------------------------------------------------------- the sessions next to it
def test_other_sessions_are_what_they_are_without_it(model):
    """A plain duplex session and a client_rate=16000 duplex session, run with no mixed-rate session about, then made before and made
    after a mixed-rate one that ticks between their pushes: the same bits each time."""
    from bvcodec.streaming import StreamingCodec
    B, pushes = 2, 10
    x22 = torch.stack([speech(pushes * 441, 300 + b) * 0.9 for b in range(B)]).to(DEV)
    x16 = torch.stack([speech(pushes * 320, 310 + b) * 0.9 for b in range(B)]).to(DEV)
    make = lambda: (StreamingCodec(model, B, 3000, hop=441), StreamingCodec(model, B, 3000, hop=320, client_rate=16000))

    def run(pair, between):
        out = []
        for t in range(pushes):
            codes, wav = pair[0].push(x22[:, t * 441:(t + 1) * 441])
            out += [codes.clone(), wav.clone()]
            between()
            codes, wav, counts = pair[1].push(x16[:, t * 320:(t + 1) * 320])
            out += [codes.clone(), wav.clone(), counts.clone()]
            between()
        torch.cuda.synchronize()
        return out

    base = run(make(), lambda: None)
    before = make()
    mixed = StreamingCodec(model, 3, 3000, hop=441, client_rate=(8000, 16000, 48000))
    assert type(before[1]._client).__name__ == "_ClientRate" and type(mixed._client).__name__ == "_MixedClientRate"
    xm = (0.1 * torch.randn(3, 960, generator=torch.Generator().manual_seed(1))).to(DEV)
    tick = lambda: mixed.push(xm)
    after = make()
    for name, pair in (("before", before), ("after", after)):
        got = run(pair, tick)
        assert len(got) == len(base) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, base)), name
    assert before[0]._client is None and before[1].lag == 14 and before[1].slot_lag(0) == 14 and before[1].slot_rate(1) == 16000
    model.check_status()
