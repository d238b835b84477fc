"""Slots of the whole-hop streaming codec: rows of a session are opened, closed, re-used and re-rated while the others keep running,
and whatever a slot emits is bit for bit the offline call on that stream's own signal alone.  Needs the MI355X."""
import pytest
import torch

import gpu_sessions as gs
from gpu_sessions import DEV, churn_schedule, utt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return gs.product_model()


def run_session(model, B, hop, ticks, utts, rate_changes=(), check_finite=True):
    """Drives one session through a schedule.  Rows without a stream hold NaN and 1e30 in every push.  Fills in, per utterance:
    x (n,), delay, codes (F, z), wav (256 F,), bits (F,) (the bits per frame in force for each of its frames)."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec, join_plan
    X = torch.full((B, ticks * hop), float("nan"))
    X[:, 1::2] = 1e30
    taken = torch.zeros(B, ticks, dtype=torch.bool)
    for u in utts:
        u.n = (u.t_close - u.t_open) * hop
        u.x = synth.synthetic_speech(u.batch, u.n, seed=u.seed, kind="speech")[u.row].float()
        assert not taken[u.slot, u.t_open:u.t_close].any(), "schedule: two utterances overlap in a slot"
        taken[u.slot, u.t_open:u.t_close] = True
        X[u.slot, u.t_open * hop:u.t_close * hop] = u.x
        u.codes, u.wav, u.bits, u.frames = [], [], [], 0
    X = X.to(DEV)
    sc = StreamingCodec(model, B, 3000, hop=hop, open_all=False)
    live = {}
    for t in range(ticks):
        for u in utts:
            if u.t_close == t:
                sc.close(u.slot)
                del live[u.slot]
        for u in utts:
            if u.t_open == t:
                u.delay = sc.open(u.slot, u.rate)
                assert u.delay == join_plan(t * hop, hop)[0]
                live[u.slot] = u
        for tt, slot, rate in rate_changes:
            if tt == t:
                sc.set_bitrate(slot, rate)
                live[slot].rate = rate
        c, w = sc.push(X[:, t * hop:(t + 1) * hop])
        k = c.shape[1]
        if check_finite and k:
            assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(w).all()), f"tick {t}: output not finite"
        for b in range(B):
            first, count, f0 = sc.slot_frames(b)
            if b not in live:
                assert count == 0
                continue
            u = live[b]
            assert 0 <= first and first + count <= k
            if count:
                assert f0 == u.frames
                u.codes.append(c[b, first:first + count].clone())
                u.wav.append(w[b, 256 * first:256 * (first + count)].clone())
                u.bits += [model.bits_per_frame(u.rate)] * count
                u.frames += count
    torch.cuda.synchronize()
    for u in utts:
        assert u.frames == (u.n - u.delay - 768) // 256 + 1 and u.frames > 0, (u.slot, u.t_open, u.frames, u.delay)
        u.codes, u.wav = torch.cat(u.codes, 0), torch.cat(u.wav, 0)
    return sc


def check_against_offline(model, utts):
    """Every utterance against the offline call on its own signal alone: the launch-per-layer reference model (the bar of
    test_whole_hop_codec_equals_offline_and_oracle: codes equal, waveform within 2e-6) and the default model (codes equal)."""
    ref_model = gs.reference_model()
    for u in utts:
        F = u.frames
        x = u.x[None].to(DEV)
        codes_off = ref_model.encode(x, u.rate)
        assert torch.equal(u.codes[None], codes_off[:, :F]), (u.slot, u.t_open)
        assert torch.equal(model.encode(x, u.rate)[:, :F], u.codes[None]), (u.slot, u.t_open)
        wav_off = ref_model.decode(codes_off, u.n)
        err = (u.wav[None] - wav_off[:, :256 * F]).abs().max().item()
        assert err <= 2e-6, (u.slot, u.t_open, err)


def churn_run(model, schedule):
    def make():
        utts = churn_schedule()
        run_session(model, 8, 441, 300, utts)
        assert {u.delay for u in utts} >= {0, 355, 368, 369, 370, 128}
        return utts
    return gs.memo(("slots churn", schedule), make)


@pytest.mark.parametrize("schedule", ["flow", "graph", "eager"])
def test_churn_equals_offline(model, schedule, monkeypatch):
    """8 slots, 441-sample hops, 300 ticks, 13 utterances of different lengths and bitrates that come and go (delays 0 .. 370, a slot
    used three times, two opened in one tick, a slot closed and re-opened between the same two pushes), slot 7 idle throughout with
    NaN / 1e30 in its input row: every utterance equals the offline call on its own signal, on each of the tick's schedules."""
    gs.set_schedule(monkeypatch, schedule)
    utts = churn_run(model, schedule)
    check_against_offline(model, utts)
    model.check_status()


def test_churn_256_slots_equals_offline(model):
    """Joins into a warm, full-width session on the default schedule: 256 rows, 40 utterances spread over 150 ticks (the sliding
    generator windows stand at a non-zero cursor when most of them start, and the histories move back to the front of their
    buffers several times during each of them)."""
    import random
    rng = random.Random(5)
    rates = (1500, 3000, 6000, 2200)
    utts, busy = [], {}
    for i in range(40):
        slot = rng.choice([0, 1, 17, 100, 254, 255] + list(range(256)))
        t_open = max(busy.get(slot, 0), rng.randrange(0, 110))
        t_close = min(150, t_open + rng.randrange(12, 45))
        if t_close - t_open < 8:
            continue
        busy[slot] = t_close + rng.randrange(0, 3)
        utts.append(utt(slot, t_open, t_close, rates[i % 4], 200 + i))
    assert len(utts) >= 36 and len({u.slot for u in utts}) < len(utts)       # some slots are used more than once
    run_session(model, 256, 441, 150, utts)
    check_against_offline(model, utts)
    model.check_status()


@pytest.mark.parametrize("hop", [700, 1100])
def test_other_hops_with_joins_equal_offline(model, hop):
    """Three and five frames per tick, 5 slots, streams that join and leave."""
    ticks = 70 if hop == 700 else 50
    utts = [utt(0, 0, ticks, 3000, 301), utt(1, 3, 40, 1500, 302),           # hop 700, tick 3: delay 716
            utt(2, 7, ticks - 5, 6000, 303), utt(1, 40, ticks, 3000, 304), utt(3, 15, 45, 2200, 305), utt(3, 46, ticks, 1500, 306)]
    run_session(model, 5, hop, ticks, utts)                                   # slot 4 idle
    assert max(u.delay for u in utts) >= (716 if hop == 700 else 540)
    check_against_offline(model, utts)
    model.check_status()


def test_bitrate_change_mid_stream(model):
    """One slot switched 3000 -> 1500 -> 6000 at two ticks: its codes equal bvc_bvrnn_encode with the per-frame bits the switches
    imply; its neighbours are untouched."""
    utts = [utt(0, 0, 120, 3000, 401), utt(1, 4, 120, 3000, 402), utt(2, 9, 120, 6000, 403)]
    run_session(model, 3, 441, 120, utts, rate_changes=[(40, 1, 1500), (83, 1, 6000)])
    u = utts[1]
    assert [b for i, b in enumerate(u.bits) if i == 0 or b != u.bits[i - 1]] == [35.0, 17.0, 70.0]
    mel = model.mel_spectrogram(u.x[None].to(DEV))[:, :u.frames].contiguous()
    bits = torch.tensor(u.bits, device=DEV)[None]
    ref, _ = model.bvrnn.encode_stateful(mel, bits, torch.zeros(1, 1, model.conf["h_dim"], device=DEV))
    assert torch.equal(u.codes[None], ref)
    assert not torch.equal(u.codes[None], model.encode(u.x[None].to(DEV), 3000)[:, :u.frames])     # the switches did something
    check_against_offline(model, [utts[0], utts[2]])
    model.check_status()


def test_churn_against_the_oracle(model):
    """Two utterances of the churn schedule (default tick schedule) against the CPU oracle directly.  Waveform: the oracle decoding the
    STREAMED codes, RMS < 1e-4.  Codes: the free-running oracle encode; a differing bit is excused only where the oracle's probability
    is within 1e-5 of 0.5, and the comparison of an utterance ends with the first frame that holds an excused bit (behind it the two
    recurrences code different streams); at least 60 % of each utterance's frames must have been compared.  The two utterances were
    picked with the CPU oracle: seed 41 row 1 at 1500 bit/s has no active probability within 1e-5 of 0.5 in its 86 frames, seed 42
    row 0 at 6000 bit/s has its first in frame 69 (of the 82 frames the stream gets)."""
    from gpu_common import make_model
    from oracle import codec as ocodec
    _, conf, vr, ge = make_model(True, 1024)
    utts = [u for u in churn_run(model, "flow") if (u.seed, u.row) in ((41, 1), (42, 0))]
    assert len(utts) == 2
    torch.set_num_threads(16)
    oc = ocodec.OracleCodec(conf, vr, ge)
    for u in utts:
        F = u.frames
        r = oc.encode(u.x[None], u.rate, full=True)
        mism = u.codes[None].cpu() != r["codes"][:, :F]
        margin = (r["prob"][:, :F] - 0.5).abs()
        differing = mism.any(2)[0].nonzero().flatten()
        compared = int(differing[0]) if len(differing) else F                  # frames before the first differing bit
        assert not bool((mism & (margin > 1e-5))[:, :compared + 1].any()), (u.seed, compared)     # ... which must be a near-tie
        print(f"oracle: seed {u.seed} rate {u.rate}: {compared} of {F} frames compared, {int(mism[:, :compared + 1].sum())} excused bits")
        assert compared >= 0.6 * F, (u.seed, compared, F)
        ref_wav = oc.decode(u.codes[None].cpu(), u.n)[:, :256 * F]
        rms = float((u.wav[None].cpu() - ref_wav).pow(2).mean().sqrt())
        print(f"oracle: seed {u.seed}: waveform rms error {rms:.3e}")
        assert rms < 1e-4, (u.seed, rms)
    model.check_status()


def test_slot_errors_leave_the_session_untouched(model):
    """Misuse of the slot calls is refused (BVC_EINVAL -> ValueError) and changes nothing: the following ticks still match."""
    from gpu_common import make_model
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    B, hop, ticks = 3, 441, 60
    x = synth.synthetic_speech(B, hop * ticks, seed=51, kind="speech").to(DEV)
    sc = StreamingCodec(model, B, 3000, hop=hop)
    sc.close(2)
    codes = []
    for t in range(ticks):
        if t in (0, 20, 41):
            for bad in (lambda: sc.open(-1, 3000), lambda: sc.open(B, 3000), lambda: sc.close(B), lambda: sc.set_bitrate(-1, 3000),
                        lambda: sc.slot_frames(B), lambda: sc.open(0, 1500), lambda: sc.close(2), lambda: sc.set_bitrate(2, 1500)):
                with pytest.raises(ValueError):
                    bad()
        c, w = sc.push(x[:, t * hop:(t + 1) * hop])
        codes.append(c.clone())
        assert sc.slot_frames(2)[1] == 0 and sc.slot_frames(0)[:2] == (0, c.shape[1])
        assert c.shape[1] == 0 or sc.slot_frames(0)[2] == sum(cc.shape[1] for cc in codes[:-1])
    codes = torch.cat(codes, 1)
    F = codes.shape[1]
    assert F == (hop * ticks - 768) // 256 + 1
    assert torch.equal(codes[:2], model.encode(x[:2], 3000)[:, :F])
    fixed = make_model(False, 1024)[0]                                        # var_bit = 0: the bitrate cannot be changed
    sf = StreamingCodec(fixed, 2, 3000, hop=hop)
    with pytest.raises(ValueError, match="var_bit"):
        sf.set_bitrate(0, 1500)
    model.check_status()
