"""Host arithmetic of the streaming codec's slots (no GPU): where a stream that joins a running session starts."""
import pytest

FRAME, PAD, NFFT = 256, 256, 1024


def simulate(hop, ticks):
    """The library's own schedule, tick by tick (bvc_stream_codec_tick: a fill level that starts at the left padding, takes a hop per
    tick and gives up one frame per 256 samples beyond the window): (frames emitted before tick t, frames tick t emits)."""
    fill, emitted, out = PAD, 0, []
    for _ in range(ticks):
        fill += hop
        k = (fill - NFFT) // FRAME + 1 if fill >= NFFT else 0
        out.append((emitted, k))
        emitted += k
        fill -= FRAME * k
    return out


@pytest.mark.parametrize("hop,max_tick_aligned", [(300, 388), (441, 370), (512, 0), (700, 764), (1000, 488), (1100, 588), (1500, 988)])
def test_join_plan_against_simulated_schedule(hop, max_tick_aligned):
    from bvcodec.streaming import join_plan
    ticks = 3000
    sched = simulate(hop, ticks + 16)
    kmax = max(k for _, k in sched)
    first_frames = {}                                        # first frame of a tick -> that tick
    for t, (f0, k) in enumerate(sched):
        if k:
            first_frames[f0] = t
    worst = 0
    for t in range(ticks + 1):                               # the stream's first hop goes into tick t
        arrived = t * hop                                    # session samples before it
        delay, frame, tick = join_plan(arrived, hop)
        assert 0 <= delay < FRAME * kmax
        assert arrived + delay == FRAME * frame              # sample 0 on a session frame boundary, not before its arrival
        assert frame >= sched[t][0]                          # the start frame has not been emitted yet
        assert first_frames.get(frame) == tick and tick >= t  # ... and is the first frame of the tick that emits it
        worst = max(worst, delay)
    assert worst == max_tick_aligned


def test_join_plan_at_session_start_and_frame_count():
    from bvcodec.streaming import join_plan
    assert join_plan(0, 441) == (0, 0, 1)                    # 441 samples complete no frame: frame 0 comes with the second tick
    assert join_plan(0, 1100) == (0, 0, 0)
    # frames a stream has after n samples: (n - delay - 768) // 256 + 1, from the schedule
    hop = 441
    sched = simulate(hop, 400)
    for t in (1, 7, 58, 123):
        delay, frame, tick = join_plan(t * hop, hop)
        for life in (3, 40, 200):                            # ticks pushed before close
            emitted = sched[t + life][0]                     # session frames emitted by ticks t .. t + life - 1 and all before
            n = life * hop
            want = (n - delay - 768) // 256 + 1 if n - delay >= 768 else 0
            assert max(0, emitted - frame) == want
