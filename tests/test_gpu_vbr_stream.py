"""Streaming sessions that choose their own rates (``StreamingCodec(vbr=...)``, bvc_stream_codec_create_vbr): every stream of a send
session against ``model.encode_vbr`` of its own signal alone - codes, bits, packets, sizes - on both tick schedules, under slot churn,
under the rate cap, at a client rate; the duplex session; the receive session on the wire with a bit count per frame, lost frames
included; the refusals; and plain sessions in the same process.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_sessions as gs
import vbr_cap_oracle as vc
import vbr_oracle as vo
from gpu_sessions import DEV, chunked

pytestmark = pytest.mark.gpu
BAR = 2e-6                                                   # streaming waveform against the offline launch-per-layer model
BITRATES = (1500, 3000, 6000)                                # 17, 35 and 64 bits per frame
CAP_BITRATES = (689, 1378, 2756, 5513)                       # 8, 16, 32 and 64 bits per frame
HOP, TICKS = 441, 60
INF = float("inf")


@pytest.fixture(scope="module")
def model():
    return gs.product_model()


@pytest.fixture(scope="module")
def ref_model():
    return gs.reference_model()


def set_schedule(monkeypatch, schedule):
    gs.set_schedule(monkeypatch, schedule, flow_stays=True)


def signals(model, B, bitrates=BITRATES):
    """x (B, TICKS * HOP) and every row's target: +inf (always rung 0), -inf (always the top rung), or the median over frames of the
    second rung's distortion in one offline probe call - in rotation."""
    from bvcodec import synth

    def make():
        x = synth.synthetic_speech(B, HOP * TICKS, seed=80 + B, kind="speech").to(DEV)
        ladder = [model.active_bits(r) for r in bitrates]
        mel = model.mel_spectrogram(x)
        extra = model.bvrnn.encode_vbr(mel, ladder, -INF, torch.zeros(1, B, 1024, device=DEV), return_all=True)[3]
        med = extra["dist"][:, :, 1].median(dim=1).values.cpu()
        return x, [(INF, -INF, float(med[b]))[b % 3] for b in range(B)]
    return gs.memo(("vbr signals", B, bitrates), make)


def drive(model, direction, x, targets, vbr, ticks=TICKS):
    """One vbr session on x, row b opened with targets[b].  Returns ks, per tick outputs concatenated: first (packets or codes), second
    (codes or wav), bits (B, F), sizes (B, F), and the session."""
    r = gs.drive_sender(model, direction, x, HOP, targets=targets, vbr=vbr, ticks=ticks)
    return r.ks, r.first, r.second, r.bits, r.sizes, r.sc


def check_wire(packets, sizes, codes, bits):
    """The session's packets and sizes are vbr_oracle.pack_vbr of its codes and bits; the bytes behind sizes are zero."""
    ref_p, ref_s = vo.pack_vbr(codes.cpu().numpy(), bits.cpu().numpy())
    got_p, got_s = packets.cpu().numpy(), sizes.cpu().numpy()
    assert np.array_equal(got_p, ref_p) and np.array_equal(got_s, ref_s)
    behind = np.arange(got_p.shape[2])[None, None, :] >= got_s[:, :, None]
    assert not got_p[behind].any()


def sent(model, schedule, B, monkeypatch):
    set_schedule(monkeypatch, schedule)
    x, targets = signals(model, B)
    return gs.memo(("vbr sent", schedule, B), lambda: (x, targets) + drive(model, "send", x, targets, dict(bitrates=BITRATES, target=0.35)))


# ---------------------------------------------------------------------------------------------- 1: every stream is its own offline call
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("schedule", ["graph", "eager"])
def test_send_streams_equal_their_offline_calls(model, schedule, B, monkeypatch):
    x, targets, ks, packets, codes, bits, sizes, sc = sent(model, schedule, B, monkeypatch)
    F = sum(ks)
    assert F == (HOP * TICKS - 768) // 256 + 1 and sc.bytes_per_frame == 9 and packets.shape == (B, F, 9)
    for b in range(B):
        off_c, off_b = model.encode_vbr(x[b:b + 1], targets[b], BITRATES)
        assert torch.equal(codes[b:b + 1], off_c[:, :F]), b
        assert torch.equal(bits[b:b + 1], off_b[:, :F]), b
        if targets[b] == -INF:
            assert torch.equal(codes[b:b + 1], model.encode(x[b:b + 1], 6000)[:, :F]) and bool((bits[b] == 64).all())
        elif targets[b] == INF:
            assert bool((bits[b] == 17).all())
        else:                                                         # not vacuous: two rungs at least twice each
            counts = [int((off_b[0, :F] == n).sum()) for n in (17, 35, 64)]
            assert sum(c >= 2 for c in counts) >= 2, (b, counts)
    check_wire(packets, sizes, codes, bits)
    model.check_status()


def test_both_schedules_give_the_same_bits(model, monkeypatch):
    g = sent(model, "graph", 3, monkeypatch)
    e = sent(model, "eager", 3, monkeypatch)
    assert g[2] == e[2] and all(torch.equal(a, b) for a, b in zip(g[3:7], e[3:7]))


# ---------------------------------------------------------------------------------------------- 2: churn
def test_churn(model):
    """Slot 0 runs throughout and is re-targeted twice; slot 1 opens late; slot 2 is finished (all num_frames(n) frames), re-opened
    with another signal and target, and starts with zero state and a full bucket (the session is capped, so a stale bucket would
    show); slot 3 stays idle.  Each stream equals its own offline capped call with the per-frame target that results."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    B, ticks = 4, 64
    x = synth.synthetic_speech(B, HOP * ticks, seed=91, kind="speech").to(DEV)
    _, (_, _, med) = signals(model, 3)
    vbr = dict(bitrates=BITRATES, target=med, rate_cap=4000, burst=100)
    sc = StreamingCodec(model, B, 3000, hop=HOP, open_all=False, direction="send", vbr=vbr)
    events = {0: [("open", 0, None)], 5: [("open", 1, -INF)], 3: [("open", 2, INF)], 20: [("target", 0, -INF)], 41: [("target", 0, med / 2)],
              25: [("finish", 2, 200)], 40: [("open", 2, -INF)]}
    target = {}
    streams, live = [], {}
    for t in range(ticks):
        for what, slot, val in events.get(t, ()):
            if what == "open":
                sc.open(slot, target=val)
                target[slot] = med if val is None else val
                live[slot] = dict(slot=slot, t0=t, t1=None, n_last=0, codes=[], bits=[], tau=[], packets=[], sizes=[])
                streams.append(live[slot])
            elif what == "target":
                sc.set_target(slot, val)
                target[slot] = val
            else:
                sc.finish(slot, val)
                live[slot]["t1"], live[slot]["n_last"] = t, val
        packets, codes = sc.push(x[:, t * HOP:(t + 1) * HOP])
        bits, sizes = sc.last_bits, sc.last_sizes
        for slot, s in list(live.items()):
            first, count, f0 = sc.slot_frames(slot)
            if count:
                assert f0 == sum(c.shape[0] for c in s["codes"])
                s["codes"].append(codes[slot, first:first + count].clone()); s["bits"].append(bits[slot, first:first + count].clone())
                s["packets"].append(packets[slot, first:first + count].clone()); s["sizes"].append(sizes[slot, first:first + count].clone())
                s["tau"] += [target[slot]] * count
            if s["t1"] is not None and sc.slot_state(slot) == "idle":
                del live[slot]
        assert bool(torch.isfinite(codes).all())                      # idle and draining rows included
    torch.cuda.synchronize()
    assert len(streams) == 4 and sc.slot_state(3) == "idle"
    for s in streams:
        t1 = ticks if s["t1"] is None else s["t1"]
        sig = x[s["slot"], s["t0"] * HOP:t1 * HOP + s["n_last"]]
        got_c, got_b = torch.cat(s["codes"]), torch.cat(s["bits"])
        T = got_c.shape[0]
        if s["t1"] is not None:
            assert T == sig.numel() // 256                            # all num_frames(n) of them
        tau = torch.tensor([s["tau"] + [s["tau"][-1]] * (sig.numel() // 256 - T)])
        off_c, off_b = model.encode_vbr(sig[None], tau, BITRATES, rate_cap=4000, burst=100)
        assert torch.equal(got_c, off_c[0, :T]) and torch.equal(got_b, off_b[0, :T]), (s["slot"], s["t0"])
        check_wire(torch.cat(s["packets"])[None], torch.cat(s["sizes"])[None], got_c[None], got_b[None])
    assert len({tuple(s["tau"]) for s in streams}) == 4 and len(set(streams[0]["tau"])) == 3
    model.check_status()


# ---------------------------------------------------------------------------------------------- 3: the cap
@pytest.mark.parametrize("schedule", ["graph", "eager"])
def test_capped_session(model, schedule, monkeypatch):
    from bvcodec.model import cap_q8
    set_schedule(monkeypatch, schedule)
    B = 3
    x, _ = signals(model, B)
    _, tg = signals(model, B, CAP_BITRATES)
    targets = [-INF, tg[2], -INF]
    vbr = dict(bitrates=CAP_BITRATES, target=0.35, rate_cap=2600, burst=96)
    ks, packets, codes, bits, sizes, sc = drive(model, "send", x, targets, vbr)
    F = sum(ks)
    rate_q8, burst_q8 = cap_q8(model.conf, [8, 16, 32, 64], 2600, 96)
    assert 8 * 256 <= rate_q8                                         # the premise of the guarantee
    for b in range(B):
        off_c, off_b = model.encode_vbr(x[b:b + 1], targets[b], CAP_BITRATES, rate_cap=2600, burst=96)
        assert torch.equal(codes[b:b + 1], off_c[:, :F]) and torch.equal(bits[b:b + 1], off_b[:, :F]), b
    slack = vc.check_windows(bits.cpu().numpy(), rate_q8, burst_q8)
    binds = int((bits[0] < 64).sum())                                 # a target of -inf asks for the top rung in every frame
    print(f"capped session {schedule}: the cap binds on {binds} of {F} frames of row 0; tightest window slack {slack / 256:g} bits")
    assert binds >= 2
    check_wire(packets, sizes, codes, bits)
    model.check_status()


# ---------------------------------------------------------------------------------------------- 4: duplex, and over the wire
def receive(model, B, packets, chunks, present=None, conceal="none", bitrate=3000):
    r = gs.drive_receiver(model, packets, chunks, [bitrate] * B, present, bitrate=bitrate, on_tick=gs.every_row_runs, vbr=True, conceal=conceal)
    assert r.sc.bytes_per_frame == 9 and r.sc.B == B
    return r.wav, r.codes, r.bits, r.sc


@pytest.mark.parametrize("B", [3, 17])
def test_duplex_and_over_the_wire(model, ref_model, B, monkeypatch):
    x, targets, ks, packets, codes, bits, sizes, _ = sent(model, "graph", B, monkeypatch)
    F = sum(ks)
    ks_d, codes_d, wav_d, bits_d, sizes_d, _ = drive(model, "duplex", x, targets, dict(bitrates=BITRATES, target=0.35))
    assert ks_d == ks and torch.equal(codes_d, codes) and torch.equal(bits_d, bits) and torch.equal(sizes_d, sizes)
    monkeypatch.setenv("BVC_STREAM_FLOW", "0")                        # bit for bit on the duplex session's schedule, launch per layer
    wav, got_c, got_b, sc = receive(model, B, packets, [k for k in ks if k])
    monkeypatch.delenv("BVC_STREAM_FLOW")                             # (the chunked receivers below: the default schedule)
    assert torch.equal(got_c, codes) and torch.equal(got_b, bits)
    assert torch.equal(wav, wav_d)
    off = torch.cat([ref_model.decode(codes[b:b + 1].contiguous(), 256 * F) for b in range(B)], 0)
    for name, chunks in (("as sent", None), ("one frame", chunked(F, 1)), ("max frames", chunked(F, sc.kmax))):
        w, c = (wav, got_c) if chunks is None else receive(model, B, packets, chunks)[:2]
        err = (w - off).abs().max().item()
        print(f"vbr wire B={B} {name}: max |err| against the offline decode {err:.3e}")
        assert torch.equal(c, codes) and err <= BAR, (name, err)
    model.check_status()


def test_lost_frames_on_the_vbr_wire(model, ref_model, monkeypatch):
    """5 % of the frames lost, their bytes junk (a lost frame has no header): without concealment the frames are frames of no bits,
    with conceal="prior" they are generated at the slot's count; both against the offline calls on the same codes."""
    B = 3
    x, targets, ks, packets, codes, bits, sizes, _ = sent(model, "graph", B, monkeypatch)
    F = sum(ks)
    rng = np.random.default_rng(17)
    present = torch.from_numpy(rng.random((B, F)) >= 0.05).to(DEV)
    present[0, 0] = False
    assert int((~present).sum()) >= 5
    lossy = packets.clone()
    lossy[~present] = 0xFF
    chunks = [(1, 2, 7, 3, 2, 1, 4)[i % 7] for i in range(F)]
    cut, f = [], 0
    while f < F:
        cut.append(min(chunks[len(cut)], F - f)); f += cut[-1]
    holed = codes.clone()
    holed[~present] = 0.5
    wav, got_c, got_b, _ = receive(model, B, lossy, cut, present)
    assert torch.equal(got_c, holed) and torch.equal(got_b, bits * present)
    for b in range(B):
        err = (wav[b:b + 1] - ref_model.decode(holed[b:b + 1].contiguous(), 256 * F)).abs().max().item()
        print(f"vbr wire, lost frames, row {b}: max |err| against the offline decode of the holed codes {err:.3e}")
        assert err <= BAR, (b, err)
    wav_p, filled, _, _ = receive(model, B, lossy, cut, present, conceal="prior", bitrate=3000)
    for b in range(B):
        nan = codes[b:b + 1].clone()
        nan[0][~present[b]] = float("nan")
        off_w, off_c = model.decode(nan, 256 * F, lost=~present[b:b + 1], bitrate=3000, return_codes=True)
        assert torch.equal(filled[b:b + 1], off_c), b
        assert torch.equal(wav_p[b:b + 1], off_w), (b, float((wav_p[b:b + 1] - off_w).abs().max()))
    assert not torch.equal(wav_p, wav)
    model.check_status()


# ---------------------------------------------------------------------------------------------- 5: at the client's rate
def test_client_rate_send(model):
    from bvcodec.streaming import StreamingCodec, resampler_lag
    from test_gpu_client_rate import FS, internal_signal, speech
    fs, pushes = 16000, 40
    hop, lag = fs // 50, resampler_lag(fs, FS)[0]
    x = (speech(pushes * hop, 123) * 0.9).to(DEV)
    _, (_, _, med) = signals(model, 3)
    sc = StreamingCodec(model, 1, 3000, hop=hop, open_all=False, direction="send", client_rate=fs,
                        vbr=dict(bitrates=BITRATES, target=med))
    sc.open(0)
    codes, bits = [], []
    for t in range(pushes):
        _, c = sc.push(x[None, t * hop:(t + 1) * hop])
        first, count, f0 = sc.slot_frames(0)
        codes.append(c[0, first:first + count].clone()); bits.append(sc.last_bits[0, first:first + count].clone())
    codes, bits = torch.cat(codes), torch.cat(bits)
    S = internal_signal(x, fs, lag)
    off_c, off_b = model.encode_vbr(S[None], med, BITRATES)
    T = codes.shape[0]
    assert T > 40 and torch.equal(codes, off_c[0, :T]) and torch.equal(bits, off_b[0, :T])
    assert len(set(bits.tolist())) >= 2


# ---------------------------------------------------------------------------------------------- 6: refusals, and plain sessions
def test_refusals_leave_the_session_usable(model):
    from bvcodec import _abi
    from bvcodec.streaming import StreamingCodec
    from gpu_common import make_model
    eng = model.engine()
    lib = eng.lib

    def create(m, ladder, direction=1, rate_q8=0, burst_q8=-1):
        h = ctypes.c_void_p()
        lad = (ctypes.c_int32 * max(len(ladder), 1))(*ladder) if ladder is not None else None
        with torch.cuda.device(DEV):
            rc = lib.bvc_stream_codec_create_vbr(m.engine().handle, 2, HOP, lad, len(ladder or ()), 0.35, rate_q8, burst_q8, 35.0, 32768.0,
                                                 32768.0, direction, ctypes.byref(h))
        if rc == 0:
            lib.bvc_stream_codec_destroy(h)
        return rc, lib.bvc_last_error().decode()

    assert create(model, (17, 35, 64))[0] == 0
    fix = make_model(False, 1024)[0]
    rc, msg = create(fix, (17, 35, 64))
    assert rc == -1 and "fixed-rate" in msg
    for ladder in (tuple(range(1, 10)), (35, 17), (17, 17), (17, 65), ()):
        rc, msg = create(model, ladder)
        assert rc == -1 and "rung" in msg, (ladder, msg)
    assert create(model, (17, 35), burst_q8=17 * 256 - 1)[0] == -1 and create(model, (17, 35), rate_q8=-1, burst_q8=9000)[0] == -1
    assert create(model, (17, 35), direction=2)[0] == -1 and create(model, None, direction=2)[0] == 0

    x, targets = signals(model, 3)
    send = StreamingCodec(model, 3, 3000, hop=HOP, direction="send", vbr=dict(bitrates=BITRATES, target=targets[2]))
    recv = StreamingCodec(model, 3, 3000, direction="recv", vbr=True)
    plain = StreamingCodec(model, 3, 3000, hop=HOP, direction="send")
    with pytest.raises(ValueError, match="chooses its own rates"):
        send.set_bitrate(0, 1500)
    with pytest.raises(ValueError, match="chooses its own rates"):
        send.open(0, 3000)
    for sc in (recv, plain):
        with pytest.raises(ValueError, match="set_target"):
            sc.set_target(0, 0.3)
    with pytest.raises(ValueError, match="set_repair"):
        recv.set_repair(8)
    with pytest.raises(ValueError, match="late"):
        recv.late(0, 0, bytes(9))
    with pytest.raises(ValueError, match="last_bits"):
        plain.last_bits
    # ... and every one of them still works: the send session's packets through the receive session
    got = []
    for t in range(12):
        p, c = send.push(x[:, t * HOP:(t + 1) * HOP])
        if p.shape[1]:
            recv.push_packets(p)
            assert torch.equal(recv.filled_codes(p.shape[1]), c)
            got.append(c[2].clone())
    got = torch.cat(got)
    off_c, _ = model.encode_vbr(x[2:3], targets[2], BITRATES)
    assert got.shape[0] > 10 and torch.equal(got, off_c[0, :got.shape[0]])


def test_plain_sessions_before_and_after(model):
    """A plain send session made before and after a vbr one in the same process gives model.encode's bits, on its default schedule."""
    from bvcodec.streaming import StreamingCodec
    x, targets = signals(model, 3)

    def plain():
        sc = StreamingCodec(model, 3, 3000, hop=HOP, direction="send")
        out = [tuple(a.clone() for a in sc.push(x[:, t * HOP:(t + 1) * HOP])) for t in range(TICKS)]
        assert sc.bytes_per_frame == 8
        return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1)

    p0, c0 = plain()
    drive(model, "send", x, targets, dict(bitrates=BITRATES, target=0.35), ticks=20)
    p1, c1 = plain()
    F = c0.shape[1]
    assert torch.equal(c0, model.encode(x, 3000)[:, :F]) and torch.equal(c1, c0) and torch.equal(p1, p0)
    assert torch.equal(p0[:, :, :5], model.pack(c0, 3000)) and not bool(p0[:, :, 5:].any())
