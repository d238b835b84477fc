"""Streaming sessions at the client's sample rate: the streaming resampler alone, and send, receive and duplex sessions with
``client_rate``, each against the offline call on the stream's own signal - ``preprocess.resample_poly`` then ``encode``, or the plain
session's samples then ``preprocess.resample_poly`` - with ``torch.equal``.  Needs the MI355X."""
import pytest
import torch

from gpu_sessions import DEV

pytestmark = pytest.mark.gpu
FS = 22050
RATES = (8000, 16000, 24000, 32000, 44100, 48000)
PAIRS = [(r, FS) for r in RATES] + [(FS, r) for r in RATES]          # (rate_in, rate_out)
H_DIM = 64                                                            # the small coder: the tests are about the session's boundary


@pytest.fixture(scope="module")
def model():
    from gpu_common import make_model
    return make_model(True, H_DIM)[0]


def offline(x, rate_in, rate_out):
    """preprocess.resample_poly of ONE signal x (n,) -> (ceil(n up / down),)."""
    from bvcodec import preprocess
    return preprocess.resample_poly(x[None].to(DEV), rate_out, rate_in)[0]


def ragged(total, hop):
    out, at, i = [], 0, 0
    while at < total:
        n = min((1, 7, hop, 3 * hop + 5)[i % 4], total - at)
        out.append(n)
        at, i = at + n, i + 1
    return out


# ---------------------------------------------------------------------------------------------- the resampler alone
@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_resampler_equals_offline_on_ragged_chunks(rate_in, rate_out):
    """Three rows, 6000 inputs each, pushed in chunks of 1, 7, a hop, three hops and 5: row 0 runs throughout, row 1 opens two pushes
    late and 3 samples into its chunk, row 2 is flushed after four pushes and opened again two pushes later.  Every stream's samples
    are the offline call on its own signal: the prefix E(N) before the flush, everything after it; the counts are E's."""
    from bvcodec.streaming import StreamResampler, resampler_count
    hop, L = rate_in // 50, 6000
    chunks = ragged(L, hop)
    X = torch.randn(3, L, generator=torch.Generator().manual_seed(rate_in + rate_out)).to(DEV)
    rs = StreamResampler(3, rate_in, rate_out, 3 * hop + 5)
    E = lambda n: resampler_count(rate_in, rate_out, n)
    streams = []                                                      # [row, first sample, samples so far, [outputs]]
    live = {}

    def start(row, at, offset=0):
        rs.open(row, offset)
        live[row] = [row, at + offset, 0, []]
        streams.append(live[row])

    def check(s, whole):
        ref = offline(X[s[0], s[1]:s[1] + s[2]], rate_in, rate_out)
        got = torch.cat(s[3]) if s[3] else torch.empty(0, device=DEV)
        assert got.numel() == (ref.numel() if whole else E(s[2]))
        assert torch.equal(got, ref[:got.numel()]), (s[0], s[1], whole)

    start(0, 0)
    start(2, 0)
    at = 0
    for i, n in enumerate(chunks):
        if i == 2:
            start(1, at, 3)
        if i == 4:
            s = live.pop(2)
            check(s, False)
            s[3].append(rs.flush(2).clone())
            check(s, True)
        if i == 6:
            start(2, at)
        y, counts = rs.push(X[:, at:at + n])
        for row in range(3):
            s = live.get(row)
            if s is None:
                assert counts[row] == 0 and not bool(y[row].any())
                continue
            took = n - (s[1] - at if s[2] == 0 and s[1] > at else 0)
            assert counts[row] == E(s[2] + took) - E(s[2])
            assert not bool(y[row, counts[row]:].any())               # zeros behind a row's samples
            s[3].append(y[row, :counts[row]].clone())
            s[2] += took
        at += n
    for s in live.values():
        check(s, False)
        s[3].append(rs.flush(s[0]).clone())
        check(s, True)
    assert len(streams) == 4 and sorted(live) == [0, 1, 2]
    rs.open(0)                                                        # (every row is idle after its flush)
    for bad in (lambda: rs.open(0), lambda: rs.open(3), lambda: rs.close(-1), lambda: rs.flush(1), lambda: rs.end(1, 0),
                lambda: rs.push(torch.zeros(3, 3 * hop + 6, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        StreamResampler(3, 0, rate_out, 16)


def test_idle_rows_are_never_read():
    """NaN, Inf and 1e38 in the idle row's input: its output is zeros and the other rows are what they are without it."""
    from bvcodec.streaming import StreamResampler
    x = torch.randn(3, 2000, generator=torch.Generator().manual_seed(5)).to(DEV)
    bad = x.clone()
    bad[1, 0::3], bad[1, 1::3], bad[1, 2::3] = float("nan"), float("inf"), 1e38
    outs = []
    for inp in (x, bad):
        rs = StreamResampler(3, 16000, FS, 500)
        rs.open(0)
        rs.open(2, 17)
        got = []
        for at in range(0, 2000, 500):
            y, counts = rs.push(inp[:, at:at + 500])
            assert counts[1] == 0 and not bool(y[1].any()) and bool(torch.isfinite(y).all())
            got.append(y.clone())
        outs.append(torch.cat(got, 1))
    assert torch.equal(outs[0], outs[1])                              # (every push's whole output block, the zeros behind the counts included)
    assert bool(outs[0][0].any()) and bool(outs[0][2].any())


# ---------------------------------------------------------------------------------------------- sessions
def speech(n, seed):
    from bvcodec import synth
    return synth.synthetic_speech(1, n, seed=seed, kind="speech")[0].float()


def internal_signal(x, fs, lag):
    """S = zeros(lag) ++ resample_poly(x, 22050, fs): what a rate-converting send side codes."""
    return torch.cat([torch.zeros(lag, device=DEV), offline(x, fs, FS)])


def drive_send(model, fs, fmt, plan, pushes, direction="send", rate=3000, quantize=False):
    """plan: [(slot, open push, finish push or None, n_last)].  Returns per slot (x, codes, packets, client samples, frames, state)."""
    from bvcodec.streaming import StreamingCodec, pcm_f32_to_s16
    hop, B = fs // 50, len(plan)
    sc = StreamingCodec(model, B, rate, hop=hop, open_all=False, direction=direction, client_rate=fs, sample_format=fmt)
    X = torch.full((B, pushes * hop), float("nan"))
    out = {}
    for slot, t_open, t_fin, n_last in plan:
        n = ((t_fin if t_fin is not None else pushes) - t_open) * hop + (n_last if t_fin is not None else 0)
        x = speech(n, 100 + slot) * 0.9
        if fmt == "s16" or quantize:
            x = pcm_f32_to_s16(x).float() / 32768
        X[slot, t_open * hop:t_open * hop + n] = x                    # NaN behind a stream's last sample and in front of its first
        out[slot] = dict(x=x, codes=[], packets=[], wav=[], first=[], delay=None)
    X = X.to(DEV)
    feed = torch.nan_to_num(X * 32768).round().to(torch.int16) if fmt == "s16" else X
    for t in range(pushes):
        for slot, t_open, t_fin, n_last in plan:
            if t_fin == t:
                sc.finish(slot, n_last)
            if t_open == t:
                out[slot]["delay"] = sc.open(slot, rate)
        res = sc.push(feed[:, t * hop:(t + 1) * hop])
        for slot in out:
            first, count, f0 = sc.slot_frames(slot)
            o = out[slot]
            if count:
                assert f0 == sum(c.shape[0] for c in o["codes"])
                o["first"].append(first)
                if direction == "send":
                    o["packets"].append(res[0][slot, first:first + count].clone())
                    o["codes"].append(res[1][slot, first:first + count].clone())
                else:
                    o["codes"].append(res[0][slot, first:first + count].clone())
            if direction == "duplex":
                o["wav"].append(res[1][slot, :int(res[2][slot])].clone())
    torch.cuda.synchronize()
    for slot in out:
        out[slot]["state"] = sc.slot_state(slot)
    return sc, out


@pytest.mark.parametrize("fs", [16000, 48000])
def test_send_session_codes_the_resampled_signal(model, fs):
    """Four slots opened at pushes 0, 0, 3 and 5; slot 0 finished with 123 client samples in its last push, slot 1 with a hop less one
    sample, whose flushed tail spills into the next push.  Every slot's codes are model.encode(S) on the frames the session gave it, S =
    zeros(lag) ++ resample_poly(x, 22050, fs); its packets are model.pack of them; the finished slots have all num_frames(len(S))."""
    from bvcodec.streaming import client_finish_plan, resampler_lag
    hop, lag, pushes = fs // 50, resampler_lag(fs, FS)[0], 34
    assert lag == {16000: 14, 48000: 11}[fs]
    plan = [(0, 0, 20, 123), (1, 0, 22, hop - 1), (2, 3, None, 0), (3, 5, None, 0)]
    assert client_finish_plan(20 * hop + 123, hop, fs)[1] == 20 and client_finish_plan(22 * hop + hop - 1, hop, fs)[1] == 23
    sc, out = drive_send(model, fs, "f32", plan, pushes)
    assert sc.lag == lag
    nb = (model.active_bits(3000) + 7) // 8
    for slot, t_open, t_fin, n_last in plan:
        o = out[slot]
        S = internal_signal(o["x"], fs, lag)
        ref = model.encode(S[None], 3000)[0]
        got = torch.cat(o["codes"])
        T = got.shape[0]
        if t_fin is not None:
            assert o["state"] == "idle" and T == S.numel() // 256 == ref.shape[0], (slot, T, S.numel())
        else:
            assert o["state"] == "running" and T == ((pushes - t_open) * 441 - o["delay"] - 768) // 256 + 1
        assert torch.equal(got, ref[:T]), slot
        packets = torch.cat(o["packets"])
        assert torch.equal(packets[:, :nb], model.pack(got[None], 3000)[0]) and not bool(packets[:, nb:].any())


@pytest.mark.parametrize("fs", [8000, 48000])
def test_receive_session_gives_the_resampled_samples(model, fs):
    """Packets of a plain send session, 5 % of them dropped, conceal="prior": per slot the client's samples are resample_poly of what a
    receive session without client_rate returned for the same packets, cut at E(N).  Slots 0 and 2 get the same stream from pushes 0
    and 3: the late one does not differ."""
    from bvcodec.streaming import StreamingCodec, resampler_count
    hop, pushes = 441, 30
    x = torch.stack([speech(pushes * hop, 200 + b) * 0.9 for b in range(2)]).to(DEV)
    snd = StreamingCodec(model, 2, 3000, hop=hop, direction="send")
    packets = torch.cat([snd.push(x[:, t * hop:(t + 1) * hop])[0].clone() for t in range(pushes)], 1)     # (2, F, 8)
    F = packets.shape[1]
    present = (torch.rand(2, F, generator=torch.Generator().manual_seed(fs)) >= 0.05).to(torch.uint8)
    assert 0 < int((present == 0).sum()) < F // 4
    stream_of, t_open, k = (0, 1, 0), (0, 1, 3), 2                    # slot -> stream, the push that brings its frame 0; frames per push
    ticks = F // k + 3
    sessions = [StreamingCodec(model, 3, 3000, direction="recv", conceal="prior", open_all=False, client_rate=rate) for rate in (None, fs)]
    wav22, client, n22 = [[] for _ in range(3)], [[] for _ in range(3)], [0] * 3
    for t in range(ticks):
        pk = torch.zeros(3, k, packets.shape[2], dtype=torch.uint8)
        pr = torch.zeros(3, k, dtype=torch.uint8)
        live = []
        for slot in range(3):
            f = (t - t_open[slot]) * k
            if t == t_open[slot]:
                for sc in sessions:
                    assert sc.open(slot, 3000) == 0
            if 0 <= f and f + k <= F:
                pk[slot], pr[slot] = packets[stream_of[slot], f:f + k].cpu(), present[stream_of[slot], f:f + k]
                live.append(slot)
            elif f >= 0 and f < F + k:                                # the stream is over: the slot is closed
                for sc in sessions:
                    if sc.slot_state(slot) != "idle":
                        sc.close(slot)
        w = sessions[0].push_packets(pk.to(DEV), pr.to(DEV))
        cw, counts = sessions[1].push_packets(pk.to(DEV), pr.to(DEV))
        assert counts.dtype == torch.int64 and counts.device.type == "cpu" and cw.shape[0] == 3
        for slot in range(3):
            if slot in live:
                wav22[slot].append(w[slot].clone())
                n22[slot] += w.shape[1]
                assert int(counts[slot]) == resampler_count(FS, fs, n22[slot]) - resampler_count(FS, fs, n22[slot] - w.shape[1])
                client[slot].append(cw[slot, :int(counts[slot])].clone())
            else:
                assert int(counts[slot]) == 0
    torch.cuda.synchronize()
    for slot in range(3):
        w22, got = torch.cat(wav22[slot]), torch.cat(client[slot])
        assert w22.numel() == 256 * (F // k) * k and got.numel() == resampler_count(FS, fs, w22.numel())
        assert torch.equal(got, offline(w22, FS, fs)[:got.numel()]), slot
    if torch.equal(torch.cat(wav22[0]), torch.cat(wav22[2])):         # (the plain session's rows agree: then so do the client's)
        assert torch.equal(torch.cat(client[0]), torch.cat(client[2]))
    model.check_status()


def test_duplex_session_holds_both_contracts(model):
    """44.1 kHz, slot 1 opened before push 2 (its frame 0 waits for the session's grid: the resampler behind d_wav starts at that
    frame, 256 * first samples into its push): the codes are encode(S)'s, the client's samples resample_poly of the samples a plain
    duplex session returns for S, cut at E(N)."""
    from bvcodec.streaming import StreamingCodec, resampler_count, resampler_lag
    fs, pushes = 44100, 30
    lag = resampler_lag(fs, FS)[0]
    plan = [(0, 0, None, 0), (1, 2, None, 0), (2, 4, 24, 300)]
    sc, out = drive_send(model, fs, "f32", plan, pushes, direction="duplex")
    plain = StreamingCodec(model, 3, 3000, hop=441, open_all=False)
    S = {slot: internal_signal(out[slot]["x"], fs, lag) for slot, *_ in plan}
    X22 = torch.full((3, (pushes + 1) * 441), float("nan"), device=DEV)
    for slot, t_open, t_fin, n_last in plan:
        X22[slot, t_open * 441:t_open * 441 + S[slot].numel()] = S[slot]
    wav22 = {slot: [] for slot in S}
    for t in range(pushes):
        for slot, t_open, t_fin, n_last in plan:
            if t_open == t:
                assert plain.open(slot, 3000) == out[slot]["delay"]
            if t_fin is not None and t == (t_open * 441 + S[slot].numel()) // 441:
                plain.finish(slot, S[slot].numel() - (t - t_open) * 441)
        codes, w = plain.push(X22[:, t * 441:(t + 1) * 441])
        for slot in S:
            first, count, _ = plain.slot_frames(slot)
            if count:
                wav22[slot].append(w[slot, 256 * first:256 * (first + count)].clone())
    torch.cuda.synchronize()
    assert out[1]["delay"] > 0 and out[2]["state"] == "idle"
    print("first frame of each slot's ticks:", {slot: sorted(set(out[slot]["first"])) for slot in S})
    for slot in S:
        got = torch.cat(out[slot]["codes"])
        assert torch.equal(got, model.encode(S[slot][None], 3000)[0][:got.shape[0]]), slot
        if plan[slot][2] is not None:
            assert got.shape[0] == S[slot].numel() // 256
        w22, client = torch.cat(wav22[slot]), torch.cat(out[slot]["wav"])
        assert w22.numel() == 256 * got.shape[0] and client.numel() == resampler_count(FS, fs, w22.numel())
        assert torch.equal(client, offline(w22, FS, fs)[:client.numel()]), slot
    model.check_status()


def test_s16_is_a_function_of_f32(model):
    """s16 in: the session that is fed x / 32768 as float32 gives the same codes; s16 out: the samples are the f32 session's through
    clamp(rint(y * 32768)).  Exact in both directions."""
    from bvcodec.streaming import StreamingCodec, pcm_f32_to_s16
    fs, pushes = 16000, 12
    plan = [(0, 0, None, 0), (1, 1, None, 0)]
    _, a = drive_send(model, fs, "s16", plan, pushes)
    _, b = drive_send(model, fs, "f32", plan, pushes, quantize=True)  # fed the s16 samples / 32768
    for slot in (0, 1):
        assert torch.equal(a[slot]["x"], b[slot]["x"]) and torch.equal(torch.cat(a[slot]["codes"]), torch.cat(b[slot]["codes"]))
        assert torch.cat(a[slot]["codes"]).shape[0] >= 10
    packets = torch.cat(a[0]["packets"])[None]
    sessions = [StreamingCodec(model, 1, 3000, direction="recv", client_rate=fs, sample_format=fmt) for fmt in ("f32", "s16")]
    for f in range(0, packets.shape[1] - 1, 2):
        (w, n), (q, m) = [sc.push_packets(packets[:, f:f + 2]) for sc in sessions]
        assert q.dtype == torch.int16 and w.dtype == torch.float32 and int(n[0]) == int(m[0]) > 0
        assert torch.equal(q[0, :int(m[0])], pcm_f32_to_s16(w[0, :int(n[0])]))
    for bad in (torch.zeros(2, fs // 50), torch.zeros(2, fs // 50, dtype=torch.float64)):
        with pytest.raises(ValueError):
            StreamingCodec(model, 2, 3000, hop=fs // 50, direction="send", client_rate=fs, sample_format="s16").push(bad)


def test_session_without_client_rate_is_unchanged(model):
    """A plain duplex session next to a rate-converting one in the same process: two-value returns, codes bit for bit the offline
    encode's, samples within 2e-6 of the offline decode's, as tests/test_gpu_streaming.py holds them."""
    from bvcodec.streaming import StreamingCodec
    B, hop, pushes = 3, 441, 40
    x = torch.stack([speech(pushes * hop, 300 + b) * 0.9 for b in range(B)]).to(DEV)
    other = StreamingCodec(model, B, 3000, hop=960, client_rate=48000)
    sc = StreamingCodec(model, B, 3000, hop=hop)
    assert sc.client_rate is None and sc._client is None and sc.hop == hop                # (no resampler on either side)
    codes, wavs = [], []
    for t in range(pushes):
        res = sc.push(x[:, t * hop:(t + 1) * hop])
        assert len(res) == 2
        codes.append(res[0].clone())
        wavs.append(res[1].clone())
        assert len(other.push(torch.zeros(B, 960, device=DEV))) == 3
    torch.cuda.synchronize()
    codes, wav = torch.cat(codes, 1), torch.cat(wavs, 1)
    F = codes.shape[1]
    assert F == (pushes * hop - 768) // 256 + 1 and wav.shape[1] == 256 * F
    off = model.encode(x, 3000)
    assert torch.equal(codes, off[:, :F])
    assert (wav - model.decode(off, pushes * hop)[:, :256 * F]).abs().max().item() <= 2e-6
    same = StreamingCodec(model, B, 3000, hop=hop, client_rate=FS)    # the session's own rate: the session it is today
    assert same._client is None and len(same.push(x[:, :hop])) == 2
    model.check_status()
