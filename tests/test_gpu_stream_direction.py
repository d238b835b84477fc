"""Streaming sessions by direction: a send session (samples -> packets), a receive session (packets -> samples, lost frames included)
and the end-of-stream flush, each against the duplex session, the offline calls and the CPU oracle.  Needs the MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gpu_sessions as gs
from gpu_sessions import DEV, RATES, chunked, churn_schedule

pytestmark = pytest.mark.gpu
BAR = 2e-6                                                   # streaming waveform against the offline launch-per-layer model


@pytest.fixture(scope="module")
def model():
    return gs.product_model()


@pytest.fixture(scope="module")
def ref_model():
    return gs.reference_model()


def nbits_of(model, rate):
    return model.active_bits(rate)


def host_pack(codes, nbits):
    """codes (..., z) of {0, 1, 0.5} -> uint8 (..., 8): the nbits leading bits in numpy's little bit order, zeros behind."""
    bits = (codes[..., :nbits].cpu().numpy() > 0.75).astype(np.uint8)
    out = np.zeros(bits.shape[:-1] + (8,), np.uint8)
    if nbits:
        p = np.packbits(bits, axis=-1, bitorder="little")
        out[..., :p.shape[-1]] = p
    return out


def sent(model, schedule, B, monkeypatch):
    """The duplex and the send session of test 1 on one input, per tick schedule and batch (shared with the receive tests)."""
    from bvcodec import synth
    gs.set_schedule(monkeypatch, schedule)

    def make():
        hop, ticks = 441, 120
        x = synth.synthetic_speech(B, hop * ticks, seed=60 + B, kind="speech").to(DEV)
        rates = [RATES[b % 4] for b in range(B)]
        d, s = gs.drive_sender(model, "duplex", x, hop, rates), gs.drive_sender(model, "send", x, hop, rates)
        return SimpleNamespace(x=x, rates=rates, ks=s.ks, ks_d=d.ks, codes_d=d.first, wav_d=d.second, packets=s.first, codes=s.second)
    return gs.memo(("direction", schedule, B), make)


@pytest.mark.parametrize("B", [3, 40])
def test_send_equals_duplex_and_offline(model, B, monkeypatch):
    """The send session's codes equal the duplex session's; each row's packets unpack to exactly those codes,
    equal numpy's little-order packing of the offline encode() on the emitted frames, and are 0 behind the row's bytes and bits."""
    r = sent(model, "flow", B, monkeypatch)
    assert r.ks == r.ks_d and sum(r.ks) == (441 * 120 - 768) // 256 + 1
    assert r.packets.dtype == torch.uint8 and r.packets.shape == (B, sum(r.ks), 8)
    assert torch.equal(r.codes, r.codes_d)
    F = r.codes.shape[1]
    for b in range(B):
        rate = r.rates[b]
        nbits = nbits_of(model, rate)
        used = (nbits + 7) // 8
        pk = r.packets[b:b + 1]
        assert torch.equal(model.unpack(pk[:, :, :used].contiguous(), rate), r.codes[b:b + 1]), b
        off = model.encode(r.x[b:b + 1], rate)[:, :F]
        assert torch.equal(off, r.codes[b:b + 1]), b
        want = np.packbits((off[0, :, :nbits].cpu().numpy() > 0.75).astype(np.uint8), axis=-1, bitorder="little")
        got = pk[0].cpu().numpy()
        assert np.array_equal(got[:, :used], want), b
        assert not got[:, used:].any(), b
        if nbits % 8:
            assert not (got[:, used - 1] >> (nbits % 8)).any(), b
    assert {nbits_of(model, q) for q in r.rates} == ({26, 35, 64} if B == 3 else {17, 26, 35, 64})
    model.check_status()


def receive(model, B, rates, packets, chunks, present=None):
    """A receive session fed `packets` (B, F, 8) in ticks of `chunks` frames; returns wav (B, 256 F)."""
    assert packets.shape[0] == B
    r = gs.drive_receiver(model, packets, chunks, rates, present, on_tick=gs.every_row_runs)
    return r.wav, r.sc


@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("schedule", ["flow", "graph", "eager"])
def test_receive_equals_duplex_and_offline(model, ref_model, schedule, B, monkeypatch):
    """The packets of the send session, fed in ticks of the frame counts that session emitted, give the duplex
    session's waveform bit for bit; one frame per tick and max_frames_per_tick frames per tick are within 2e-6 of the offline decode."""
    r = sent(model, schedule, B, monkeypatch)
    F = r.codes.shape[1]
    wav, sc = receive(model, B, r.rates, r.packets, [k for k in r.ks if k])
    assert 4 <= sc.kmax <= 7 and sc.bytes_per_frame == 8
    assert torch.equal(wav, r.wav_d)
    off = torch.cat([ref_model.decode(ref_model.encode(r.x[b:b + 1], r.rates[b])[:, :F].contiguous(), 256 * F) for b in range(B)], 0)
    for name, chunks in (("as sent", None), ("one frame", chunked(F, 1)), ("max frames", chunked(F, sc.kmax))):
        w = wav if chunks is None else receive(model, B, r.rates, r.packets, chunks)[0]
        assert bool(torch.isfinite(w).all())
        err = (w - off).abs().max().item()
        print(f"receive {schedule} B={B} {name}: max |err| against the offline decode {err:.3e}")
        assert err <= BAR, (name, err)
    model.check_status()


def loss_patterns(T):
    rng = np.random.default_rng(7)
    present = np.ones((8, T), np.uint8)
    present[0, [5, 17, 60]] = 0                                               # single frames
    present[1, 30:40] = 0                                                     # a burst of 10
    present[2, 0] = 0                                                         # the very first frame of a stream
    present[3, 1::2] = 0                                                      # every other frame
    #        4: nothing lost
    present[5, rng.random(T) < 0.1] = 0                                       # a seeded 10 %
    present[6, 0:3] = 0
    present[6, 50:60] = 0
    present[7, rng.random(T) < 0.3] = 0
    return present


def test_lost_frames(model, ref_model):
    """Seeded loss patterns on 8 rows; lost frames carry 0xFF bytes.  Row 1 is the reference case of DESIGN.md section 6: 1 s of
    synthetic_speech(seed=41) at 3000 bit/s, frames 30-39 lost."""
    from gpu_common import make_model
    from bvcodec import synth
    from oracle import codec as ocodec
    n, T = 22050, 86
    x = synth.synthetic_speech(8, n, seed=43, kind="speech")
    x[1] = synth.synthetic_speech(1, n, seed=41, kind="speech")[0]
    x = x.to(DEV)
    rates = [1500, 3000, 6000, 2200, 3000, 6000, 1500, 3000]
    codes = torch.cat([ref_model.encode(x[b:b + 1], rates[b]) for b in range(8)], 0)
    assert codes.shape == (8, T, 64)
    present = loss_patterns(T)
    assert present[4].all() and not present[1, 30:40].any() and present[1].sum() == T - 10
    packets = np.stack([host_pack(codes[b], nbits_of(model, rates[b])) for b in range(8)], 0)
    lossy = packets.copy()
    lossy[present == 0] = 0xFF                                                # what a lost frame's bytes hold must reach nothing
    lost = codes.clone()
    lost[torch.from_numpy(present == 0).to(DEV)] = 0.5
    chunks = [(1, 2, 7, 3, 2, 1, 4)[i % 7] for i in range(200)]
    cut, f = [], 0
    for k in chunks:
        cut.append(min(k, T - f))
        f += cut[-1]
        if f == T:
            break
    wav, _ = receive(model, 8, rates, torch.from_numpy(lossy).to(DEV), cut, torch.from_numpy(present).to(DEV))
    clean, _ = receive(model, 8, rates, torch.from_numpy(packets).to(DEV), cut)
    assert bool(torch.isfinite(wav).all())
    assert torch.equal(wav[4], clean[4])                                      # rows do not leak into each other
    ref_lost = torch.cat([ref_model.decode(lost[b:b + 1].contiguous(), 256 * T) for b in range(8)], 0)
    ref_full = torch.cat([ref_model.decode(codes[b:b + 1].contiguous(), 256 * T) for b in range(8)], 0)
    for b in range(8):
        err = (wav[b] - ref_lost[b]).abs().max().item()
        print(f"lost frames row {b}: {int((present[b] == 0).sum())} lost, max |err| against the offline decode of the holed codes {err:.3e}")
        assert err <= BAR, (b, err)
    assert (clean - ref_full).abs().max().item() <= BAR
    # ignoring `present` cannot pass: the two references differ, from the first lost frame on
    diff = (ref_lost[1] - ref_full[1]).pow(2).mean().sqrt().item()
    print(f"burst row: rms difference between the offline decodes with and without the loss {diff:.3e}")
    assert diff > 2e-5
    # ... and the burst row against the CPU oracle decoding the same holed code tensor
    _, conf, vr, ge = make_model(True, 1024)
    torch.set_num_threads(16)
    oc = ocodec.OracleCodec(conf, vr, ge)
    ref = oc.decode(lost[1:2].cpu(), n)[:, :256 * T]
    rms = float((wav[1:2].cpu() - ref).pow(2).mean().sqrt())
    print(f"burst row: waveform rms error against the oracle {rms:.3e}")
    assert rms <= 1e-4, rms
    model.check_status()


def test_receive_side_churn(model, ref_model):
    """The shape of churn_schedule() on a receive session of 8 rows - rows opened, closed, re-opened and re-rated
    between ticks, idle rows' bytes 0xFF with present = 1; a tick takes 1, 2 or 3 frames.  The packets of an utterance carry all 64
    bits of its 6000 bit/s encode, so a row that runs at fewer bits has to ignore what lies behind them: the reference is the offline
    decode of the codes with 0.5 behind each frame's bit count.  Misuse is refused and changes nothing."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    B, ticks = 8, 300
    kt = [(1, 2, 2, 1, 2, 3)[t % 6] for t in range(ticks)]
    utts = churn_schedule()
    rerate = {(1, 30): 6000, (0, 60): 1500, (0, 200): 3000}                   # (slot, tick) -> new rate from that tick on
    for u in utts:
        u.F = sum(kt[u.t_open:u.t_close])
        u.x = synth.synthetic_speech(u.batch, 256 * u.F, seed=u.seed, kind="speech")[u.row].float()
        full = ref_model.encode(u.x[None].to(DEV), 6000)[0]                   # every bit active
        assert full.shape == (u.F, 64) and not bool((full == 0.5).any())
        u.bytes = torch.from_numpy(host_pack(full, 64)).to(DEV)
        u.full, u.nb, u.wav, u.frames = full, [], [], 0
    sc = StreamingCodec(model, B, 3000, open_all=False, direction="recv")
    send = StreamingCodec(model, 2, 3000, hop=441, direction="send")
    xs = synth.synthetic_speech(2, 441 * 40, seed=77, kind="speech").to(DEV)
    sent_codes = []
    live = {}
    for t in range(ticks):
        for u in utts:
            if u.t_close == t:
                sc.close(u.slot)
                del live[u.slot]
                assert sc.slot_state(u.slot) == "idle"
        for u in utts:
            if u.t_open == t:
                assert sc.open(u.slot, u.rate) == 0
                assert sc.slot_state(u.slot) == "waiting"
                live[u.slot] = u
        for s in [s for s in live if (s, t) in rerate]:
            sc.set_bitrate(s, rerate[(s, t)])
            live[s].rate = rerate[(s, t)]
        k = kt[t]
        pk = torch.full((B, k, 8), 0xFF, dtype=torch.uint8, device=DEV)
        for s, u in live.items():
            pk[s] = u.bytes[u.frames:u.frames + k]
        if t in (0, 33, 150):                                                 # misuse: refused, the session untouched
            for bad in (lambda: sc.push(torch.zeros(B, 441, device=DEV)), lambda: sc.push_packets(pk[:, :0]),
                        lambda: sc.push_packets(torch.zeros(B, sc.kmax + 1, 8, dtype=torch.uint8, device=DEV)),
                        lambda: sc.open(next(iter(live)), 3000), lambda: sc.finish(next(iter(live)), 0),
                        lambda: send.push_packets(pk[:2])):
                with pytest.raises(ValueError):
                    bad()
        if t < 40:
            sent_codes.append(send.push(xs[:, t * 441:(t + 1) * 441])[1].clone())
        w = sc.push_packets(pk, torch.ones(B, k, dtype=torch.uint8, device=DEV))
        assert bool(torch.isfinite(w).all()), t
        for b in range(B):
            first, count, f0 = sc.slot_frames(b)
            if b not in live:
                assert count == 0 and sc.slot_state(b) == "idle"
                continue
            u = live[b]
            assert (first, count, f0) == (0, k, u.frames) and sc.slot_state(b) == "running"
            u.wav.append(w[b].clone())
            u.nb += [nbits_of(model, u.rate)] * k
            u.frames += k
    torch.cuda.synchronize()
    assert sc.slot_state(7) == "idle"
    for u in utts:
        assert u.frames == u.F
        ref_codes = u.full.clone()
        for i, nb in enumerate(u.nb):
            ref_codes[i, nb:] = 0.5
        off = ref_model.decode(ref_codes[None].contiguous(), 256 * u.F)[0]
        err = (torch.cat(u.wav) - off).abs().max().item()
        assert err <= BAR, (u.slot, u.t_open, err)
    assert len({tuple(sorted(set(u.nb))) for u in utts}) >= 5                 # several bit counts, some changed mid-stream
    assert any(len(set(u.nb)) > 1 for u in utts)
    sent_codes = torch.cat(sent_codes, 1)                                     # the send session that refused tick_recv three times
    assert torch.equal(sent_codes, model.encode(xs, 3000)[:, :sent_codes.shape[1]]) and sent_codes.shape[1] == (441 * 40 - 768) // 256 + 1
    model.check_status()


def stream(slot, t_open, t_fin, residue, rate, seed, hop, n_last=None):
    """A stream that lives in `slot` from push t_open on and is finished before push t_fin; n_last is chosen so that its sample count
    n = (t_fin - t_open) * hop + n_last has n % 256 == residue (or given).  t_fin None: it runs to the end of the session."""
    if t_fin is not None and n_last is None:
        n_last = (residue - (t_fin - t_open) * hop) % 256
    return SimpleNamespace(slot=slot, t_open=t_open, t_fin=t_fin, n_last=n_last, rate=rate, seed=seed)


def flush_schedule(hop):
    late = 254 if hop == 441 else 3                                           # hop 441: tick 254 has the largest delay, 370
    return [
        stream(0, 0, 40, 0, 3000, 501, hop),                                  # n a multiple of 256 ...
        stream(1, 0, 40, 1, 1500, 502, hop),                                  # ... plus 1, finished in the same tick
        stream(2, late, late + 36, 255, 6000, 503, hop),                      # ... plus 255
        stream(3, 0, None, 0, 2200, 504, hop),                                # keeps running throughout
        stream(4, 40, 100, 0, 3000, 505, hop, n_last=0),                      # opens in the tick in which two others finish; ends with a whole hop
        stream(0, 46, 120, 0, 6000, 506, hop, n_last=hop),                    # slot 0 again once it is idle; n_last = the whole hop
        stream(1, 60, 130, 77, 2200, 507, hop),
    ]                                                                         # slot 5 stays idle


@pytest.mark.parametrize("hop", [441, 700])
@pytest.mark.parametrize("direction", ["duplex", "send"])
def test_flush(model, ref_model, direction, hop):
    """Streams that end with bvc_stream_codec_finish in a duplex and in a send session: n a multiple of 256, plus 1, plus 255, with n_last 0
    and a whole hop among them, one opened with the largest delay, two finished in the tick in which another opens, a slot opened again once
    it is idle; NaN behind every stream's last sample.  Every stream gets ALL frames of the offline encode.  (A running slot has at least
    768 samples, so the n <= 512 refusal cannot be reached through a running slot: the waiting slot, where such a stream still is, is
    refused instead.)"""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec, finish_plan, join_plan
    B = 6
    ss = flush_schedule(hop)
    ticks = max((s.t_fin or 0) for s in ss) + 12
    X = torch.full((B, ticks * hop), float("nan"))
    for s in ss:
        s.n = ((s.t_fin if s.t_fin is not None else ticks) - s.t_open) * hop + (s.n_last or 0)
        s.x = synth.synthetic_speech(1, s.n, seed=s.seed, kind="speech")[0].float()
        X[s.slot, s.t_open * hop:s.t_open * hop + s.n] = s.x                  # behind it, the rest of its last hop included: NaN
        s.codes, s.wav, s.frames, s.plan = [], [], 0, None
    assert {s.n % 256 for s in ss if s.t_fin is not None} >= {0, 1, 255}
    X = X.to(DEV)
    sc = StreamingCodec(model, B, 3000, hop=hop, open_all=False, direction=direction)
    live = {}
    for t in range(ticks):
        for s in ss:
            if s.t_fin == t:
                assert sc.slot_state(s.slot) == "running"
                for bad in (lambda: sc.finish(s.slot, -1), lambda: sc.finish(s.slot, hop + 1), lambda: sc.finish(5, 0)):
                    with pytest.raises(ValueError):
                        bad()
                sc.finish(s.slot, None if s.n_last == hop else s.n_last)
                assert sc.slot_state(s.slot) == "draining"
                for bad in (lambda: sc.finish(s.slot, 0), lambda: sc.open(s.slot, 3000)):
                    with pytest.raises(ValueError):
                        bad()
                n, total, plan = finish_plan(s.t_open, t, s.n_last, hop)
                assert (n, total) == (s.n, s.n // 256)
                s.plan = dict(plan)
        for s in ss:
            if s.t_open == t:
                assert sc.slot_state(s.slot) == "idle"
                s.delay = sc.open(s.slot, s.rate)
                assert s.delay == join_plan(t * hop, hop)[0]
                if s.delay:
                    assert sc.slot_state(s.slot) == "waiting"
                    with pytest.raises(ValueError):
                        sc.finish(s.slot, 0)
                live[s.slot] = s
        a, c = sc.push(X[:, t * hop:(t + 1) * hop])
        codes, wav = (c, None) if direction == "send" else (a, c)
        k = codes.shape[1]
        assert bool(torch.isfinite(codes).all()) and (wav is None or bool(torch.isfinite(wav).all())), t
        for b in range(B):
            first, count, f0 = sc.slot_frames(b)
            s = live.get(b)
            if s is None:
                assert count == 0 and sc.slot_state(b) == "idle"
                continue
            assert first == 0 and count <= k
            if s.plan is not None:                                            # draining: the plan says what each tick gives, and when it is over
                assert count == s.plan[t], (b, t, count, s.plan)
                assert sc.slot_state(b) == ("idle" if t == max(s.plan) else "draining")
            else:
                assert count == (k if sc.slot_state(b) == "running" else 0)
            if count:
                assert f0 == s.frames
                s.codes.append(codes[b, :count].clone())
                if wav is not None:
                    s.wav.append(wav[b, :256 * count].clone())
                s.frames += count
            if s.plan is not None and t == max(s.plan):
                del live[b]
    torch.cuda.synchronize()
    if hop == 441:
        assert max(s.delay for s in ss) == 370
    for s in ss:
        x = s.x[None].to(DEV)
        off = ref_model.encode(x, s.rate)
        T = s.n // 256
        assert off.shape[1] == T
        if s.t_fin is None:
            T = (s.n - s.delay - 768) // 256 + 1                              # never finished: what its samples complete
        else:
            assert s.frames == T, (s.slot, s.t_open, s.frames, T)             # ALL frames of the offline call
        got = torch.cat(s.codes, 0)[None]
        assert torch.equal(got, off[:, :T]), (s.slot, s.t_open)
        assert torch.equal(got, model.encode(x, s.rate)[:, :T]), (s.slot, s.t_open)
        if direction == "duplex":
            err = (torch.cat(s.wav)[None] - ref_model.decode(off, s.n)[:, :256 * T]).abs().max().item()
            print(f"flush hop {hop} slot {s.slot} from tick {s.t_open}: n = {s.n}, {T} frames, max |err| {err:.3e}")
            assert err <= BAR, (s.slot, s.t_open, err)
    model.check_status()


def test_close_on_a_draining_slot_drops_the_rest(model):
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec, join_plan
    hop = 441
    x = synth.synthetic_speech(2, hop * 60, seed=88, kind="speech").to(DEV)
    sc = StreamingCodec(model, 2, 3000, hop=hop, direction="send")
    codes, again = [], []
    for t in range(60):
        if t == 20:
            sc.finish(1, 400)
        if t == 21:
            assert sc.slot_state(1) == "draining"
            sc.close(1)
            assert sc.slot_state(1) == "idle"
        if t == 22:
            assert sc.open(1, 6000) == join_plan(22 * hop, hop)[0]
        pk, c = sc.push(x[:, t * hop:(t + 1) * hop])
        codes.append(c.clone())
        if t >= 22:
            again.append(c[1:2, :sc.slot_frames(1)[1]].clone())
    codes, again = torch.cat(codes, 1), torch.cat(again, 1)
    assert again.shape[1] > 20 and torch.equal(again, model.encode(x[1:2, 22 * hop:], 6000)[:, :again.shape[1]])     # the slot is as good as new
    assert torch.equal(codes[:1], model.encode(x[:1], 3000)[:, :codes.shape[1]])     # the neighbour never noticed
    model.check_status()


def test_over_the_wire(model, ref_model):
    """A send session's packets go to the host and back into a receive session; 40 rows at mixed rates, two
    streams finished on the way and their rows opened again."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    B, hop, ticks = 40, 441, 100
    ss = [stream(b, 0, None, 0, RATES[b % 4], 700 + b, hop) for b in range(B) if b not in (5, 17)]
    ss += [stream(5, 0, 30, 0, 3000, 705, hop, n_last=100), stream(5, 40, None, 0, 1500, 745, hop),
           stream(17, 2, 50, 0, 2200, 717, hop, n_last=0), stream(17, 60, None, 0, 6000, 757, hop)]
    X = torch.full((B, ticks * hop), float("nan"))
    for s in ss:
        s.n = ((s.t_fin if s.t_fin is not None else ticks) - s.t_open) * hop + (s.n_last or 0)
        s.x = synth.synthetic_speech(1, s.n, seed=s.seed, kind="speech")[0].float()
        X[s.slot, s.t_open * hop:s.t_open * hop + s.n] = s.x
        s.codes, s.wav, s.frames = [], [], 0
    X = X.to(DEV)
    tx = StreamingCodec(model, B, 3000, hop=hop, open_all=False, direction="send")
    rx = StreamingCodec(model, B, 3000, open_all=False, direction="recv")
    live, rx_open = {}, set()
    for t in range(ticks):
        for s in ss:
            if s.t_fin == t:
                tx.finish(s.slot, s.n_last)
            if s.t_open == t:
                assert tx.slot_state(s.slot) == "idle"
                s.delay = tx.open(s.slot, s.rate)
                live[s.slot] = s
        pk, codes = tx.push(X[:, t * hop:(t + 1) * hop])
        k = pk.shape[1]
        if k == 0:
            continue
        wire = pk.cpu().numpy().tobytes()                                     # the wire: bytes on the host
        present = torch.zeros(B, k, dtype=torch.uint8)
        counts = {}
        for b, s in live.items():
            first, count, f0 = tx.slot_frames(b)
            counts[b] = count
            if count:
                assert first == 0 and f0 == s.frames
                if f0 == 0:                                                   # the receiver learns of the stream with its first packet
                    assert rx.open(b, s.rate) == 0
                    rx_open.add(b)
                present[b, :count] = 1                                        # nothing arrives for a row without a stream (or behind its end)
                s.codes.append(codes[b, :count].clone())
        back = torch.from_numpy(np.frombuffer(wire, np.uint8).reshape(B, k, 8).copy()).to(DEV)
        w = rx.push_packets(back, present)
        assert bool(torch.isfinite(w).all())
        for b, s in list(live.items()):
            if counts[b]:
                assert rx.slot_frames(b) == (0, k, s.frames)
                s.wav.append(w[b, :256 * counts[b]].clone())
                s.frames += counts[b]
            if tx.slot_state(b) == "idle":                                    # drained: the stream is over on both sides
                rx.close(b)
                rx_open.discard(b)
                del live[b]
    torch.cuda.synchronize()
    assert len(ss) == 42 and all(s.frames > 0 for s in ss)
    for s in ss:
        x = s.x[None].to(DEV)
        off = ref_model.encode(x, s.rate)
        T = s.n // 256 if s.t_fin is not None else (s.n - s.delay - 768) // 256 + 1
        assert s.frames == T, (s.slot, s.t_open, s.frames, T)
        assert torch.equal(torch.cat(s.codes, 0)[None], off[:, :T]), (s.slot, s.t_open)
        err = (torch.cat(s.wav)[None] - ref_model.decode(off, s.n)[:, :256 * T]).abs().max().item()
        assert err <= BAR, (s.slot, s.t_open, err)
    model.check_status()


def test_fixed_rate_model_sends_and_receives_all_bits():
    """var_bit = 0: every frame carries all z_dim bits whatever bitrate the slot was opened with."""
    from bvcodec import synth
    fixed, ref = gs.product_model(False), gs.reference_model(False)
    B, hop, ticks = 3, 441, 60
    x = synth.synthetic_speech(B, hop * ticks, seed=91, kind="speech").to(DEV)
    s = gs.drive_sender(fixed, "send", x, hop, [1500, 3000, 6000])
    ks, packets, codes = s.ks, s.first, s.second
    F = codes.shape[1]
    off = ref.encode(x, 3000)[:, :F]
    assert torch.equal(codes, off) and not bool((codes == 0.5).any())
    assert np.array_equal(packets.cpu().numpy(), host_pack(off, 64))
    wav, _ = receive(fixed, B, [1500, 3000, 6000], packets, [k for k in ks if k])
    err = (wav - ref.decode(off.contiguous(), 256 * F)).abs().max().item()
    assert err <= BAR, err
    fixed.check_status()
