"""Helpers shared by the GPU tests of the streaming sessions (test_gpu_streaming, _stream_slots, _stream_direction, _conceal,
_late_repair, _client_rate, _vbr_stream): the models, the tick schedules, the churn schedule, and one driver for each side of the wire.
The cases and what they assert are the test files' own."""
from types import SimpleNamespace

import torch

from gpu_common import DEV, make_model

RATES = (2200, 3000, 6000, 1500)                             # 26, 35, 64 and 17 bits per frame (26: a frame that ends inside a byte)
_MEMO = {}


def product_model(var_bit=True):
    return make_model(var_bit, 1024)[0]


def reference_model(var_bit=True):
    """The launch-per-layer model: the ticks' own recurrence kernels, offline."""
    return make_model(var_bit, 1024, env={"BVC_RECURRENCE": "layers"})[0]


def set_schedule(monkeypatch, schedule, flow_stays=False):
    """How the sessions created from here on run their ticks.  "flow": the recurrences on the persistent kernel (the default); "graph":
    launch-per-layer kernels, replayed from the session's graph table once the streams are warm; "eager": the same launches without
    the graph.  flow_stays: only "eager" sets anything (tests/test_gpu_vbr_stream.py)."""
    if schedule != "flow" and not flow_stays:
        monkeypatch.setenv("BVC_STREAM_FLOW", "0")
    if schedule == "eager":
        monkeypatch.setenv("BVC_STREAM_NO_GRAPH", "1")


def memo(key, make):
    """make() once per key and test process: what several tests of a file share and leave unchanged."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def chunked(total, k):
    return [k] * (total // k) + ([total % k] if total % k else [])


def utt(slot, t_open, t_close, rate, seed, row=0, batch=1):
    """One utterance of a schedule: it lives in `slot` for the pushes t_open .. t_close - 1; its signal is row `row` of
    synth.synthetic_speech(batch, n, seed) with n = (t_close - t_open) * hop (filled in by the test that runs the schedule)."""
    return SimpleNamespace(slot=slot, t_open=t_open, t_close=t_close, rate=rate, seed=seed, row=row, batch=batch)


# hop 441: the delay of a stream that joins at tick t is 0 at t = 0 and 256, 368 at 16, 369 at 135 and the largest, 370, at 254
ORACLE_A = dict(rate=1500, seed=41, row=1, batch=2)       # 50 ticks = 22050 samples: the CPU oracle has no probability within 1e-5 of 0.5
ORACLE_B = dict(rate=6000, seed=42, row=0, batch=2)       # 50 ticks: the oracle's first such probability (active bits) is in frame 69


def churn_schedule():
    return [
        utt(0, 0, 37, 3000, 101), utt(1, 0, 90, 1500, 102),                  # two slots open in one tick, delay 0
        utt(2, 5, 55, **ORACLE_B),                                            # delay 355
        utt(3, 16, 70, 2200, 104),                                            # delay 368, an odd bitrate (26 bits per frame)
        utt(0, 37, 120, 6000, 105),                                           # closed and re-opened between the same two pushes
        utt(4, 45, 110, 3000, 106), utt(5, 45, 95, **ORACLE_A),               # two slots open in one tick of a running session
        utt(2, 63, 135, 3000, 108),
        utt(4, 117, 180, 1500, 109),
        utt(3, 128, 190, 6000, 110),                                          # delay 128
        utt(0, 135, 230, 1500, 111),                                          # slot 0 for the third time; delay 369
        utt(6, 254, 300, 3000, 112),                                          # the largest delay, 370
        utt(1, 256, 300, 4100, 113),                                          # delay 0 in a warm session; another odd bitrate
    ]                                                                         # slot 7 stays idle throughout


def drive_sender(model, direction, x, hop, rates=None, targets=None, vbr=None, ticks=None):
    """One send or duplex session on x (B, ticks * hop), every row opened before the first push: row b at rates[b], or on a vbr session
    with targets[b].  Returns sc, ks (the frame count of every tick) and the ticks' outputs concatenated: first (B, F, ...) and second -
    (packets, codes) on a send session, (codes, wav) on a duplex one - and on a vbr session bits and sizes (B, F)."""
    from bvcodec.streaming import StreamingCodec
    B = x.shape[0]
    sc = StreamingCodec(model, B, 3000, hop=hop, open_all=False, direction=direction, vbr=vbr)
    for b in range(B):
        assert (sc.open(b, rates[b]) if vbr is None else sc.open(b, target=targets[b])) == 0
    ks, first, second, bits, sizes = [], [], [], [], []
    for t in range(x.shape[1] // hop if ticks is None else ticks):
        a, c = sc.push(x[:, t * hop:(t + 1) * hop])
        k = a.shape[1]
        ks.append(k)
        first.append(a.clone())
        second.append(c.clone())
        assert all(sc.slot_frames(b)[:2] == (0, k) for b in (0, B - 1))
        if vbr is not None:
            bits.append(sc.last_bits.clone())
            sizes.append(sc.last_sizes.clone())
            assert bits[-1].shape == (B, k) and sizes[-1].shape == (B, k)
    torch.cuda.synchronize()
    return SimpleNamespace(sc=sc, ks=ks, first=torch.cat(first, 1), second=torch.cat(second, 1),
                           bits=torch.cat(bits, 1) if bits else None, sizes=torch.cat(sizes, 1) if sizes else None)


def send_packets(model, B, ticks, hop=441, seed=70):
    """(ks, packets (B, F, 8)) of a send session on a short seeded signal, row b at RATES[b % 4]; ks without the ticks of no frame."""
    from bvcodec import synth
    x = synth.synthetic_speech(B, hop * ticks, seed=seed + B, kind="speech").to(DEV)
    r = drive_sender(model, "send", x, hop, [RATES[b % 4] for b in range(B)])
    return [k for k in r.ks if k], r.first


def every_row_runs(sc, i, f, k):
    """on_tick of drive_receiver for a session whose rows all run from the first tick to the last."""
    assert sc.slot_frames(0) == (0, k, f) and sc.slot_state(sc.B - 1) == "running"


def drive_receiver(model, packets, chunks, rates, present=None, actions=None, opened=None, bitrate=3000, on_tick=None, **session):
    """One receive session (session: conceal=, repair=, vbr=) fed packets (B, F, bytes) in ticks of `chunks` frames, the rows of
    `opened` (None: all) opened before the first push at rates[b].  present (B, F): 0 marks a frame pushed as not arrived.  actions
    {tick index: [(what, ...), ...]}, carried out in front of that push: ("late", row, stream_frame, the frame's bytes), ("open", row,
    rate), ("close", row), ("rate", row, rate), ("conceal", mode).  on_tick(sc, tick index, first frame, count) behind every push.
    Returns sc, wav (B, 256 F), codes (B, F, z) (``filled_codes``), bits (B, F) (vbr), taken (late's answers)."""
    from bvcodec.streaming import StreamingCodec
    B = packets.shape[0]
    sc = StreamingCodec(model, B, bitrate, open_all=False, direction="recv", **session)
    for b in range(B) if opened is None else sorted(opened):
        assert sc.open(b, rates[b]) == 0
        assert sc.slot_state(b) == "waiting"
    act = {"late": sc.late, "open": sc.open, "close": sc.close, "rate": sc.set_bitrate, "conceal": sc.set_conceal}
    wav, codes, bits, taken, f = [], [], [], [], 0
    for i, k in enumerate(chunks):
        for what, *args in (actions or {}).get(i, ()):
            answer = act[what](*args)
            if what == "late":
                taken.append(answer)
        w = sc.push_packets(packets[:, f:f + k], None if present is None else present[:, f:f + k])
        assert w.shape == (B, 256 * k)
        wav.append(w.clone())
        codes.append(sc.filled_codes(k).clone())
        if session.get("vbr"):
            bits.append(sc.last_bits.clone())
        if on_tick is not None:
            on_tick(sc, i, f, k)
        f += k
    assert f == packets.shape[1]
    torch.cuda.synchronize()
    return SimpleNamespace(sc=sc, wav=torch.cat(wav, 1), codes=torch.cat(codes, 1), bits=torch.cat(bits, 1) if bits else None, taken=taken)
