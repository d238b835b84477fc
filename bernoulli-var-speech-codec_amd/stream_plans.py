"""Host arithmetic of the streaming sessions: where a stream joins and ends, what a late packet repairs, how a client's hop maps to
the model's rate.  Each function mirrors the library's own arithmetic and touches no device."""
import math

CONTEXT_FRAMES = 26      # ceil(6 + 1 + 15 + 1/8 + 120/64 + 1/64 + 120/128 + 1/128 + 120/256 + 6/256)


def join_plan(samples_so_far, hop, frame=256, pad_left=256, n_fft=1024):
    """Where a stream that joins a running ``StreamingCodec`` session starts: ``(delay, start_frame, start_tick)``.

    The session has taken ``samples_so_far`` samples per row (ticks so far * hop).  Session frame f reads the samples
    [frame f - pad_left, frame f - pad_left + n_fft), so it is emitted by the first tick whose samples reach that far (ticks count
    from 0).  A stream's frame grid is fixed by its sample 0, the session's by tick 0: the library delays the row by ``delay`` samples
    so that the stream's sample 0 becomes session sample frame * start_frame, where start_frame is the first frame at or behind the
    stream's arrival that is the FIRST frame of its tick (the row's reset then lies between two ticks).  Pure host arithmetic, the
    same as the library's (csrc/stream_codec.hip: join_plan)."""
    def tick_of(f):
        return -(-(frame * f - pad_left + n_fft) // hop) - 1
    f = -(-samples_so_far // frame)
    while f > 0 and tick_of(f - 1) == tick_of(f):
        f += 1
    return frame * f - samples_so_far, f, tick_of(f)


def finish_plan(open_tick, finish_tick, n_last, hop, frame=256, pad_left=256, n_fft=1024):
    """What a stream that is finished (``StreamingCodec.finish``) still gets: ``(n, total_frames, [(tick, count), ...])``.

    The stream's first hop went into tick ``open_tick`` (``open`` was called before that push), ``finish(slot, n_last)`` is called
    before the push of tick ``finish_tick``, whose hop holds the stream's last ``n_last`` samples: n = (finish_tick - open_tick) * hop
    + n_last samples in all, total_frames = n // frame = the frames of the offline ``encode``.  The list says for tick finish_tick
    and every later one up to the tick that emits the last frame how many of that tick's frames are the stream's (``slot_frames``'s
    count); after the last entry the slot is idle.  Frames the stream got before tick finish_tick: total_frames minus the counts.
    Pure host arithmetic, the same as the library's (csrc/stream_codec.hip: stream_finish_rows and the end of bvc_stream_codec_tick)."""
    def emitted_before(t):                                  # session frames emitted by the ticks before tick t
        have = pad_left + t * hop
        return (have - n_fft) // frame + 1 if have >= n_fft else 0
    n = (finish_tick - open_tick) * hop + n_last
    if not 0 <= n_last <= hop or n <= n_fft - frame - pad_left:
        raise ValueError("finish_plan: n_last out of range or the stream is too short for the right reflect padding")
    _, f0, _ = join_plan(open_tick * hop, hop, frame, pad_left, n_fft)
    end = f0 + n // frame
    out, t = [], finish_tick
    while True:
        lo, hi = emitted_before(t), emitted_before(t + 1)
        out.append((t, max(0, min(hi, end) - max(lo, f0))))
        if hi >= end:
            return n, n // frame, out
        t += 1


def generator_reach(vocoder_config):
    """Frames behind mel frame f whose samples frame f still reaches through the causal generator: conv_pre looks 6 frames back, every
    stage one input row through its upsampler and (ks - 1) * (d + 1) rows through each AMP pair of its widest block, conv_post 6 samples -
    6 + sum_stages (1 / rate_in + max_ks (ks - 1) * sum_d (d + 1) / rate_out) + 6 / 256 = 25.45 for the shipped generator, so frame f
    changes samples of the frames f .. f + 26 and none later (``CONTEXT_FRAMES``)."""
    reach, rate = 6.0, 1
    for r in vocoder_config["upsample_rates"]:
        rate_in, rate = rate, rate * r
        reach += 1.0 / rate_in + max((ks - 1) * sum(d + 1 for d in ds) for ks, ds in
                                     zip(vocoder_config["resblock_kernel_sizes"], vocoder_config["resblock_dilation_sizes"])) / rate
    return math.ceil(reach + 6.0 / rate)


def repair_plan(ticks, window, requests):
    """What a receive session with a repair window of ``window`` frames does with late packets: ``(taken, passes)``.

    ``ticks``: ``[(first_frame, count), ...]``, the session's ticks in order since the ring was last cleared (creation, ``set_repair``,
    ``set_conceal``), in session frames; the session has decoded ``first_frame + count`` of the last entry.  A tick is *retained* while
    it holds any of the last ``window`` decoded frames.  ``requests``: ``[(row, stream_frame0, stream_frame, lost), ...]``, the ``late``
    calls since the last tick in order: the slot, the session frame that is frame 0 of the slot's current stream (None: the slot is not
    running), the frame's index in that stream, and whether the tick that decoded it was given it as not present.

    ``taken[i]``: the frame belongs to the running stream (index >= 0), has been decoded, lies in a retained tick, was lost and has not
    been handed in by an earlier request.  ``passes``: ``[(tick_index, [rows]), ...]``, oldest first: every row with a taken packet is
    decoded again from the snapshot in front of the tick that holds its earliest late frame - the newest retained tick whose first
    frame is not behind it - through the last tick; rows that start at the same tick share a pass.  Pure host arithmetic, the same as
    the library's (csrc/stream_codec.hip: bvc_stream_codec_late and stream_apply_late)."""
    done = ticks[-1][0] + ticks[-1][1] if ticks else 0
    retained = [i for i, (f0, k) in enumerate(ticks) if f0 + k > done - window] if window > 0 else []
    taken, seen, first = [], set(), {}
    for row, frame0, stream_frame, lost in requests:
        ok = frame0 is not None and stream_frame >= 0 and frame0 + stream_frame < done
        at = None
        if ok:
            f = frame0 + stream_frame
            at = next((i for i in retained if ticks[i][0] <= f < ticks[i][0] + ticks[i][1]), None)
            ok = at is not None and bool(lost) and (row, f) not in seen
        if ok:
            seen.add((row, f))
            first[row] = min(first.get(row, at), at)
        taken.append(ok)
    passes = [(t, sorted(r for r in first if first[r] == t)) for t in sorted(set(first.values()))]
    return taken, passes


def client_hop(hop, client_rate, fs=22050):
    """The internal samples of a hop of client samples; ValueError where that is no whole number."""
    if int(client_rate) <= 0 or int(hop) <= 0:
        raise ValueError(f"client_rate {client_rate} and hop {hop} must be positive")
    if hop * fs % client_rate:
        raise ValueError(f"a hop of {hop} samples at {client_rate} Hz is {hop * fs / client_rate:g} samples at {fs} Hz: not a whole number")
    return hop * fs // client_rate


def client_finish_plan(n_client, hop, fs, fs_internal=22050):
    """Where the internal stream of a rate-converting send session ends: ``(len_S, push, n_last)``.

    The stream has ``n_client`` client samples in all, pushed ``hop`` at a time from its push 0 on.  Its internal stream S =
    zeros(lag) ++ resample_poly(x, fs_internal, fs) has ``len_S = lag + ceil(n_client * fs_internal / fs)`` samples, of which every push
    writes hop22 = hop * fs_internal / fs.  The session's ``finish`` takes the internal ``n_last`` (0 .. hop22) in front of push ``push``
    of the stream: the push that holds the client's last sample where the flushed tail still fits its hop, else the next one (the tail
    spills: at most ``lag`` samples).  Pure host arithmetic."""
    from .resampling import resampler_lag                       # (the filter's lag is the library's arithmetic)
    hop22 = client_hop(hop, fs, fs_internal)
    lag = resampler_lag(fs, fs_internal)[0]
    if n_client < 0:
        raise ValueError("client_finish_plan: n_client must not be negative")
    len_s = lag + -(-n_client * fs_internal // fs)
    last = max(0, -(-n_client // hop) - 1)                      # the push that holds the client's last sample
    tail = len_s - last * hop22
    return (len_s, last, tail) if tail <= hop22 else (len_s, last + 1, tail - hop22)
