"""Repair window of a receive session (bvc_stream_codec_set_repair / _late): a packet that arrives a few ticks late puts the decoder
back on the state of a session that got it in time.  Every case runs receive sessions over the same packets - ON-TIME (the packet is
present in its own push), LATE (lost in its push, handed in with ``late`` some ticks afterwards) and NEVER (lost for good) - on the
WIDE weight draw: on the default draw the state forgets a lost frame within about 30 frames and "repaired equals on-time" would hold
without any repair (tests/test_late_repair_cpu.py keeps both figures).  Needs the MI355X."""
import pytest
import torch

import bvrnn_draws
import gpu_sessions as gs
from gpu_common import make_model
from gpu_sessions import DEV, RATES

pytestmark = pytest.mark.gpu
REACH = 26                                                      # bvcodec.streaming.generator_reach: frames one mel frame reaches ahead


def mk(var_bit=True):
    return make_model(var_bit, 1024, gains=bvrnn_draws.GAINS["wide"])[0]


def send_packets(model, var_bit, B, ticks, hop=441):
    """(B, F, 8) uint8: a send session of the same model on a short seeded signal, row b at RATES[b % 4]; computed once per case."""
    return gs.memo(("late_repair", var_bit, B, ticks), lambda: gs.send_packets(model, B, ticks, hop)[1])


def chunks(F):
    """Ticks of 1, 2 and 3 frames mixed: [(first frame, count), ...] over F frames."""
    out, f, i = [], 0, 0
    while f < F:
        k = min((1, 2, 3, 2, 3, 1, 1, 3)[i % 8], F - f)
        out.append((f, k))
        f += k
        i += 1
    return out


def tick_of(ticks, f):
    return next(i for i, (f0, k) in enumerate(ticks) if f0 <= f < f0 + k)


def lossy(packets, lost, seed=5):
    """The packets as a push sees them: the bytes of frames that are not present are random."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    junk = torch.randint(0, 256, packets.shape, generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
    out = packets.clone()
    out[lost] = junk[lost]
    return out


def run(model, packets, ticks, lost, actions=None, conceal="none", repair=0, opened=None):
    """One receive session.  lost (B, F) bool: frames pushed as not present.  actions {tick index: [(what, ...), ...]}, carried out in
    front of that push: ("late", row, stream_frame, session frame whose bytes are handed in), ("open", row, rate), ("close", row),
    ("rate", row, rate), ("conceal", mode).  Returns (wav (B, 256 F), filled codes (B, F, 64), [late's answers])."""
    actions = {i: [a[:3] + (packets[a[1], a[3]],) if a[0] == "late" else a for a in acts] for i, acts in (actions or {}).items()}
    r = gs.drive_receiver(model, lossy(packets, lost), [k for _, k in ticks], [RATES[b % 4] for b in range(packets.shape[0])],
                          (~lost).to(torch.uint8), actions, opened, conceal=conceal, repair=repair)
    return r.wav, r.codes, r.taken


def mask(B, F, frames):
    m = torch.zeros(B, F, dtype=torch.bool, device=DEV)
    for b, f in frames:
        m[b, f] = True
    return m


def assert_repaired(late, ontime, never, rows, f_r, B, f_first=None):
    """From the tick after the last ``late`` on (first frame f_r): codes equal ON-TIME's at once, samples from f_r + REACH on; before the
    first repair (first frame f_first, f_r if there is one repair) the session is NEVER's; rows that got nothing never differ; and NEVER
    does not get there (the control)."""
    (lw, lc, _), (ow, oc, _), (nw, nc, _) = late, ontime, never
    f_first = f_r if f_first is None else f_first
    assert torch.equal(lc[:, f_r:], oc[:, f_r:])
    assert torch.equal(lw[:, 256 * (f_r + REACH):], ow[:, 256 * (f_r + REACH):])
    assert torch.equal(lw[:, :256 * f_first], nw[:, :256 * f_first]) and torch.equal(lc[:, :f_first], nc[:, :f_first])
    for b in range(B):
        if b not in rows:
            assert torch.equal(lw[b], ow[b]) and torch.equal(lc[b], oc[b]) and torch.equal(nw[b], ow[b]), b
        else:
            assert ow.shape[1] > 256 * (f_r + REACH + 2)
            assert not torch.equal(nw[b, 256 * (f_r + REACH):], ow[b, 256 * (f_r + REACH):]), b


# ------------------------------------------------------------------------------------------------ 4: one late frame
@pytest.mark.parametrize("schedule", ["flow", "graph"])
@pytest.mark.parametrize("var_bit", [True, False])
@pytest.mark.parametrize("conceal", ["none", "prior"])
@pytest.mark.parametrize("d", [1, 2, 5])
def test_one_late_frame(d, conceal, var_bit, schedule, monkeypatch):
    """Frame 34 of row 1 is lost in its push and handed in d ticks later ("graph": launch-per-layer ticks replayed from the session's
    graph table from frame 33 on, so the repair happens between two replayed ticks).  With conceal="prior" frame 54 is lost for good in
    all three sessions: what LATE generates for it are ON-TIME's bits."""
    gs.set_schedule(monkeypatch, schedule)
    model = mk(var_bit)
    B, FL, GONE = 3, 34, 54
    packets = send_packets(model, var_bit, B, 52)
    F = packets.shape[1]
    ticks = chunks(F)
    i_l = tick_of(ticks, FL)
    f_r = ticks[i_l + d][0]
    gone = [(1, GONE)] if conceal == "prior" else []
    kw = dict(conceal=conceal, repair=24)
    ontime = run(model, packets, ticks, mask(B, F, gone), **kw)
    late = run(model, packets, ticks, mask(B, F, gone + [(1, FL)]), {i_l + d: [("late", 1, FL, FL)]}, **kw)
    never = run(model, packets, ticks, mask(B, F, gone + [(1, FL)]), **kw)
    assert late[2] == [True]
    assert_repaired(late, ontime, never, {1}, f_r, B)
    if conceal == "prior":
        nb = model.active_bits(RATES[1])
        assert torch.equal(late[1][1, GONE], ontime[1][1, GONE]) and bool((late[1][1, GONE, :nb] != 0.5).all())
        assert bool((late[1][1, FL, :nb] != 0.5).all())                              # (generated when it was pushed as lost)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 5: against the offline call
def test_against_the_offline_call():
    """Independent of any other session: LATE's filled codes of the frames from f_r on are those of the offline concealing decode of the
    stream's own packets with what is STILL lost (two frames behind the repair, whose generated bits hang on the repaired state)."""
    model = mk(True)
    B, FL = 3, 20
    packets = send_packets(model, True, B, 52)
    F = packets.shape[1]
    ticks = chunks(F)
    i_l = tick_of(ticks, FL)
    f_r = ticks[i_l + 3][0]
    still = [(b, f) for b in range(B) for f in (8, f_r + 4, f_r + 21)]
    lost = mask(B, F, still + [(b, FL) for b in range(B)])
    late = run(model, packets, ticks, lost, {i_l + 3: [("late", b, FL, FL) for b in range(B)]}, conceal="prior", repair=16)
    assert late[2] == [True] * B
    for b in range(B):
        used = (model.active_bits(RATES[b]) + 7) // 8
        codes = model.unpack(packets[b:b + 1, :, :used].contiguous(), RATES[b])
        gone = mask(B, F, still)[b:b + 1]
        codes[gone] = float("nan")
        _, filled = model.decode(codes, 256 * F, lost=gone, bitrate=RATES[b], return_codes=True)
        assert torch.equal(late[1][b, f_r:], filled[0, f_r:]), b
        assert not torch.equal(late[1][b, FL], filled[0, FL])                        # (pushed as lost: generated, not the packet)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 6: several at once
@pytest.mark.parametrize("conceal", ["none", "prior"])
def test_a_burst_of_which_two_arrive(conceal):
    """Frames 20, 21, 22 of row 1 are lost; 20 and 21 arrive late between the same two ticks, 22 never: the session that lost only 22."""
    model = mk(True)
    B = 3
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    at = tick_of(ticks, 22) + 2
    kw = dict(conceal=conceal, repair=16)
    ontime = run(model, packets, ticks, mask(B, F, [(1, 22)]), **kw)
    burst = mask(B, F, [(1, 20), (1, 21), (1, 22)])
    late = run(model, packets, ticks, burst, {at: [("late", 1, 21, 21), ("late", 1, 20, 20)]}, **kw)
    never = run(model, packets, ticks, burst, **kw)
    assert late[2] == [True, True]
    assert_repaired(late, ontime, never, {1}, ticks[at][0], B)
    model.check_status()


@pytest.mark.parametrize("conceal", ["none", "prior"])
def test_two_rows_with_different_starts_and_a_second_packet_for_a_repaired_row(conceal):
    """Rows 0 and 2 lose frames of different ticks (14 and 19) and get them in front of the same push: two passes.  Row 0 has lost frame
    17 as well, which arrives three ticks after that repair: its replay starts at a snapshot behind the first repair's start, one that
    the first replay has rewritten."""
    model = mk(True)
    B = 3
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    assert len({tick_of(ticks, f) for f in (14, 17, 19)}) == 3
    first = tick_of(ticks, 19) + 1
    second = first + 3
    kw = dict(conceal=conceal, repair=24)
    lost = mask(B, F, [(0, 14), (0, 17), (2, 19)])
    ontime = run(model, packets, ticks, mask(B, F, []), **kw)
    late = run(model, packets, ticks, lost, {first: [("late", 2, 19, 19), ("late", 0, 14, 14)], second: [("late", 0, 17, 17)]}, **kw)
    never = run(model, packets, ticks, lost, **kw)
    assert late[2] == [True, True, True]
    assert_repaired(late, ontime, never, {0, 2}, ticks[second][0], B, ticks[first][0])
    # between the two repairs row 2 is ON-TIME's already, row 0 is neither's
    a, e = ticks[first][0], ticks[second][0]
    assert torch.equal(late[1][2, a:e], ontime[1][2, a:e])
    model.check_status()


def test_forty_rows_twelve_of_them_late_in_one_tick():
    model = mk(True)
    B = 40
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    rows = list(range(1, 37, 3))
    assert len(rows) == 12
    frames = {b: 16 + (b % 5) for b in rows}                                         # five different frames, three ticks
    at = tick_of(ticks, 20) + 2
    lost = mask(B, F, [(b, f) for b, f in frames.items()])
    kw = dict(conceal="prior", repair=16)
    ontime = run(model, packets, ticks, mask(B, F, []), **kw)
    late = run(model, packets, ticks, lost, {at: [("late", b, f, f) for b, f in frames.items()]}, **kw)
    never = run(model, packets, ticks, lost, **kw)
    assert late[2] == [True] * 12
    assert_repaired(late, ontime, never, set(rows), ticks[at][0], B)
    model.check_status()


def test_more_late_rows_than_one_list_holds():
    """Every per-tick list of the library holds 64 entries; here each kind is sent as two.  All 80 slots are opened in front of the first
    push: 80 pending slot updates and 80 row starts.  66 rows lose frame 20 (one pass of 66 rows: two gather groups, and two scatter groups
    behind each of its ticks), 4 others lose frame 17 of an earlier tick (a second pass), and all 70 packets are handed in in front of one
    push two ticks later (two patch lists)."""
    model = mk(True)
    B = 80
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    early = [3, 28, 53, 78]                                                          # one row of every rate
    many = [b for b in range(B) if b % 8 != 7 and b not in early]
    assert len(many) == 66 and tick_of(ticks, 17) < tick_of(ticks, 20)
    frames = {b: 20 for b in many}
    frames.update({b: 17 for b in early})
    at = tick_of(ticks, 20) + 2
    lost = mask(B, F, [(b, f) for b, f in frames.items()])
    kw = dict(conceal="prior", repair=16)
    ontime = run(model, packets, ticks, mask(B, F, []), **kw)
    late = run(model, packets, ticks, lost, {at: [("late", b, f, f) for b, f in sorted(frames.items())]}, **kw)
    never = run(model, packets, ticks, lost, **kw)
    assert late[2] == [True] * 70
    assert_repaired(late, ontime, never, set(frames), ticks[at][0], B)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 7: slot life
@pytest.mark.parametrize("conceal", ["none", "prior"])
def test_slot_life(conceal):
    """Row 1 is opened in the running session and its stream's frame 1 arrives late: the replay starts from its zero state.  Row 0 is
    re-rated between its lost frame and the repair: the replay unpacks with the old bit count.  Row 2 loses its frame 5, is closed and
    opened again: a ``late`` for frame 5 is not taken until the NEW stream has decoded its own frame 5 (as lost), and then repairs that."""
    model = mk(True)
    B = 3
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    T_OPEN1, T_CLOSE2, T_OPEN2 = 8, 9, 11
    f1, f2 = ticks[T_OPEN1][0], ticks[T_OPEN2][0]                                    # session frames that are frame 0 of the new streams
    assert ticks[T_CLOSE2][0] > 5
    lost0 = f1 + 2
    t_rate, t_fix = tick_of(ticks, lost0) + 1, tick_of(ticks, lost0) + 3
    assert ticks[t_fix][0] < f2 + 5
    t_new = tick_of(ticks, f2 + 5) + 2
    life = {T_CLOSE2: [("close", 2)], T_OPEN2: [("open", 2, 3000)], T_OPEN1: [("open", 1, RATES[1])], t_rate: [("rate", 0, 1500)]}
    lates = {t_fix: [("late", 1, 1, f1 + 1), ("late", 0, lost0, lost0), ("late", 2, 5, 5)],     # the last: the old stream's frame, the new one is not there yet
             t_new: [("late", 2, 5, f2 + 5)]}
    both = {i: life.get(i, []) + lates.get(i, []) for i in set(life) | set(lates)}
    lost = mask(B, F, [(1, f1 + 1), (0, lost0), (2, 5), (2, f2 + 5)])
    kw = dict(conceal=conceal, repair=16, opened={0, 2})
    ontime = run(model, packets, ticks, mask(B, F, [(2, 5)]), life, **kw)
    late = run(model, packets, ticks, lost, both, **kw)
    never = run(model, packets, ticks, lost, life, **kw)
    assert late[2] == [True, True, False, True]
    assert_repaired(late, ontime, never, {0, 1, 2}, ticks[t_new][0], B, ticks[t_fix][0])
    a, e = ticks[t_fix][0], ticks[t_new][0]                                          # rows 0 and 1 are ON-TIME's from the first repair on
    assert torch.equal(late[1][:2, a:e], ontime[1][:2, a:e])
    model.check_status()


# ------------------------------------------------------------------------------------------------ 8: not taken
def test_refused_packets_leave_the_session_untouched():
    """One frame older than the window, a frame that arrived in time, a frame that has not been decoded, an idle slot: False each, and the
    whole session is NEVER's.  A second ``late`` for a frame is False, and the session is that of the first alone."""
    model = mk(True)
    B, W = 3, 8
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    at = 20
    done = ticks[at][0]                                                              # frames decoded in front of push `at`
    oldest = min(f0 for f0, k in ticks[:at] if f0 + k > done - W)                    # first frame of the oldest retained tick
    lost = mask(B, F, [(0, oldest - 1), (0, oldest), (1, done)])
    refused = {at: [("late", 0, oldest - 1, oldest - 1), ("late", 0, done - 1, done - 1), ("late", 1, done, done), ("late", 2, done - 1, done - 1)]}
    kw = dict(conceal="prior", repair=W, opened={0, 1})
    never = run(model, packets, ticks, lost, **kw)
    got = run(model, packets, ticks, lost, refused, **kw)
    assert got[2] == [False, False, False, False]
    assert torch.equal(got[0], never[0]) and torch.equal(got[1], never[1])
    once = run(model, packets, ticks, lost, {at: [("late", 0, oldest, oldest)]}, **kw)
    twice = run(model, packets, ticks, lost, {at: [("late", 0, oldest, oldest), ("late", 0, oldest, oldest)], at + 1: [("late", 0, oldest, oldest)]}, **kw)
    assert once[2] == [True] and twice[2] == [True, False, False]
    assert torch.equal(once[0], twice[0]) and torch.equal(once[1], twice[1])
    assert not torch.equal(once[0][0, 256 * done:], never[0][0, 256 * done:])        # (the edge of the window itself is repaired)
    model.check_status()


def test_set_conceal_empties_the_window():
    model = mk(True)
    B = 3
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    at = 20
    f = ticks[at - 2][0]
    lost = mask(B, F, [(1, f)])
    switch = {at - 1: [("conceal", "prior")]}
    never = run(model, packets, ticks, lost, switch, repair=16)
    got = run(model, packets, ticks, lost, {at - 1: [("conceal", "prior")], at: [("late", 1, f, f)]}, repair=16)
    assert got[2] == [False]
    assert torch.equal(got[0], never[0]) and torch.equal(got[1], never[1])
    model.check_status()


def test_errors_and_a_window_without_late_packets():
    from bvcodec.streaming import StreamingCodec
    model = mk(True)
    B = 3
    packets = send_packets(model, True, B, 42)
    F = packets.shape[1]
    ticks = chunks(F)
    for direction in ("duplex", "send"):
        with pytest.raises(ValueError):
            StreamingCodec(model, B, 3000, direction=direction, repair=8)
        sc = StreamingCodec(model, B, 3000, direction=direction)
        with pytest.raises(ValueError, match="not a receive session"):
            sc.late(0, 0, packets[0, 0])
        with pytest.raises(ValueError, match="not a receive session"):
            sc.set_repair(8)
    recv = StreamingCodec(model, B, 3000, direction="recv", repair=8)
    for bad in (-1, B):
        with pytest.raises(ValueError, match="outside"):
            recv.late(bad, 0, packets[0, 0])
    with pytest.raises(ValueError, match="outside"):
        recv.set_repair(65)
    assert recv.late(0, 0, packets[0, 0]) is False                                   # nothing decoded yet
    assert recv.late(0, 0, bytes(3)) is False                                        # (fewer bytes: the leading ones)
    recv.set_repair(0)
    assert recv.late(0, 0, packets[0, 0]) is False                                   # no window
    for conceal in ("none", "prior"):
        lost = mask(B, F, [(0, 9), (1, 30), (2, 31)])
        plain = run(model, packets, ticks, lost, conceal=conceal)
        kept = run(model, packets, ticks, lost, conceal=conceal, repair=8)
        assert torch.equal(plain[0], kept[0]) and torch.equal(plain[1], kept[1])
    model.check_status()
