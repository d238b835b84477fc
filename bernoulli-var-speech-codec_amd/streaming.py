"""Stateful chunked (streaming) encode / decode on top of the same kernels (SURVEY.md 8f rank 1,
BASELINE.json configs[4]).

The reference facade has no streaming mode: it zero-initialises the GRU state on every call
(bvrnn_codec_model.py:60,69) and never returns the state after the last frame (bvrnn.py:205).  The
primitives are causal, though, so chunked processing reproduces the offline result (code bits identical; waveform
to rounding, <= 1e-6 - long offline decodes batch two dot-product halves over all frames, short hops do not):

* front-end: frame t reads samples [256t-256, 256t+768) -> it is emitted as soon as those samples
  have arrived (algorithmic look-ahead 768 samples = 34.8 ms, README.md:19); the last frames of an
  utterance, which need the right reflect padding, are emitted by ``flush()``;
* BVRNN: the GRU state is carried from chunk to chunk (``bvc_bvrnn_encode/decode`` take h0, return hT);
* vocoder: the generator is causal, so the library keeps the last 64 rows of every activation tensor
  (``bvc_vocoder_stream_*``, include/bvcodec.h) and a hop computes only the rows of its new frames -
  256 samples per frame, bit-for-bit the kernels of the offline path.  ``incremental=False`` selects
  the older, stateless scheme instead: every output sample depends on at most ``CONTEXT_FRAMES`` past
  mel frames (conv_pre 6 frames + per stage 12*(k-1) = 120 samples of AMP halo + 1 sample of
  transposed conv), so each hop re-runs the generator over [context | new frames] and keeps the new
  samples (≈4x the work per 20 ms hop).  The tail beyond the last full frame (``flush``) always uses
  the context scheme.

``tests/test_gpu_streaming.py`` checks that any chunking reproduces the offline encode()/decode().
"""
import ctypes
import math

import torch

from . import _abi
from .config import is_causal, not_causal_message
from .model import SCALING

CONTEXT_FRAMES = 26      # ceil(6 + 1 + 15 + 1/8 + 120/64 + 1/64 + 120/128 + 1/128 + 120/256 + 6/256)


class StreamingEncoder:
    def __init__(self, model, batch, bitrate, device=None):
        self.m = model
        self.B = batch
        self.bits = model.bits_per_frame(bitrate)
        eng = model.engine(None if device is None else torch.empty(0, device=device))
        self.dev = eng.device
        c = model.conf
        self.hop, self.win, self.pl = c["hopsize"], c["winsize"], c["mel_pad_left"]
        self.h = torch.zeros(1, batch, c["h_dim"], device=self.dev)
        self.buf = torch.empty(batch, 0, device=self.dev)      # samples from index self.s0 on
        self.s0 = 0                                            # global index of buf[:, 0] (multiple of hop)
        self.n = 0                                             # samples received
        self.frames = 0                                        # frames emitted

    def _emit(self, upto, total_len=None):
        """Encode frames [self.frames, upto); total_len: utterance length when flushing."""
        k = upto - self.frames
        if k <= 0:
            return torch.empty(self.B, 0, self.m.conf["z_dim"], device=self.dev)
        mel = self.m.mel_spectrogram(self.buf)                 # local frames; reflect pads only matter at the ends
        f0 = self.frames - self.s0 // self.hop
        mel = mel[:, f0:f0 + k].contiguous()
        bits = torch.full((self.B, k), self.bits, device=self.dev)
        codes, self.h = self.m.bvrnn.encode_stateful(mel, bits, self.h)
        self.frames = upto
        # keep what later frames still read: from sample hop*frames - 2*hop (so the next frame is local frame 2)
        keep_from = max(0, self.hop * self.frames - 2 * self.hop)
        if keep_from > self.s0:
            self.buf = self.buf[:, keep_from - self.s0:].contiguous()
            self.s0 = keep_from
        return codes

    @torch.no_grad()
    def push(self, x):
        """x (B, n) new samples -> codes (B, k, z_dim) of the frames completed by them (k may be 0)."""
        x = x.to(self.dev, torch.float32)
        self.buf = torch.cat([self.buf, x], 1)
        self.n += x.shape[1]
        pr = self.win - self.pl - self.hop                     # right look-ahead beyond the hop (512)
        complete = 0 if self.n < self.hop + pr else (self.n - self.hop - pr) // self.hop + 1
        if self.buf.shape[1] <= 2 * self.hop:                  # the front-end kernel needs L > 512
            complete = self.frames
        return self._emit(complete)

    @torch.no_grad()
    def flush(self):
        """End of utterance: the remaining floor(L/hop) - emitted frames (right reflect padding)."""
        total = self.n // self.hop
        if self.buf.shape[1] <= 2 * self.hop and total > self.frames:
            raise RuntimeError("utterance too short for the reflect padding of the STFT front-end")
        return self._emit(total)


class VocoderStream:
    """Handle of the library's incremental generator state for `batch` parallel streams."""

    def __init__(self, engine, batch, max_frames_per_push):
        if not is_causal(engine.conf):
            raise ValueError("VocoderStream: " + not_causal_message(engine.conf))
        self.eng = engine
        self.B = batch
        self.kmax = max_frames_per_push
        self.spf = math.prod(engine.conf["vocoder_config"]["upsample_rates"])
        h = ctypes.c_void_p()
        with torch.cuda.device(engine.device):
            _abi.check(engine.lib.bvc_vocoder_stream_create(engine.handle, batch, max_frames_per_push, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.eng.lib.bvc_vocoder_stream_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def reset(self):
        with torch.cuda.device(self.eng.device):
            _abi.check(self.eng.lib.bvc_vocoder_stream_reset(self.handle, self.eng.stream()))

    def push(self, mel, scale_div=1.0):
        """mel (B, k, num_mels) time-major on the engine's device -> wav (B, k*256)."""
        B, k, _ = mel.shape
        assert B == self.B
        out = torch.empty(B, k * self.spf, device=self.eng.device)
        with torch.cuda.device(self.eng.device):
            for f in range(0, k, self.kmax):                   # longer chunks go through in kmax-frame pieces
                n = min(self.kmax, k - f)
                piece = mel[:, f:f + n].contiguous()
                dst = out if n == k else torch.empty(B, n * self.spf, device=self.eng.device)
                _abi.check(self.eng.lib.bvc_vocoder_stream_push(self.handle, _abi.ptr(piece), n, float(scale_div),
                                                                _abi.ptr(dst), self.eng.stream()))
                if dst is not out:
                    out[:, f * self.spf:(f + n) * self.spf] = dst
        return out


class StreamingDecoder:
    def __init__(self, model, batch, device=None, incremental=True, max_frames_per_push=8):
        if not is_causal(model.conf):                          # (the context scheme counts on the same causality)
            raise ValueError("StreamingDecoder: " + not_causal_message(model.conf))
        self.m = model
        self.B = batch
        eng = model.engine(None if device is None else torch.empty(0, device=device))
        self.dev = eng.device
        c = model.conf
        self.h = torch.zeros(1, batch, c["h_dim"], device=self.dev)
        self.ctx = torch.empty(batch, 0, c["num_mels"], device=self.dev)     # last CONTEXT_FRAMES mel frames
        self.spf = math.prod(c["vocoder_config"]["upsample_rates"])         # samples per frame (256)
        self.tail = None
        self.voc = VocoderStream(eng, batch, max_frames_per_push) if incremental else None

    @torch.no_grad()
    def push(self, codes):
        """codes (B, k, z_dim) -> wav (B, 256*k): the samples of exactly those frames."""
        k = codes.shape[1]
        if k == 0:
            return torch.empty(self.B, 0, device=self.dev)
        mel, self.h = self.m.bvrnn.decode(codes.to(self.dev, torch.float32), self.h)
        allmel = torch.cat([self.ctx, mel], 1)
        nctx = self.ctx.shape[1]
        self.ctx = allmel[:, -CONTEXT_FRAMES:].contiguous()
        if self.voc is not None:
            self.tail = None
            return self.voc.push(mel, SCALING)
        wav = self.m.vocoder(allmel, 10 ** 12, _scale_div=SCALING, _time_major=True)[:, 0]
        out = wav[:, self.spf * nctx: self.spf * (nctx + k)]
        self.tail = wav[:, self.spf * (nctx + k):]             # partial sums beyond the last frame (models.py:238)
        return out

    @torch.no_grad()
    def flush(self, n_extra):
        """Up to 294 samples beyond the last full frame (what decode(codes, length) returns past 256*T)."""
        if n_extra <= 0 or self.ctx.shape[1] == 0:
            return torch.empty(self.B, 0, device=self.dev)
        if self.tail is None:                                  # incremental mode: the tail comes from the context
            wav = self.m.vocoder(self.ctx, 10 ** 12, _scale_div=SCALING, _time_major=True)[:, 0]
            self.tail = wav[:, self.spf * self.ctx.shape[1]:]
        return self.tail[:, :max(0, n_extra)]


class _DeviceView:
    """Raw device memory owned by the library, exposed to torch through the CUDA array interface."""

    def __init__(self, ptr, shape, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


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


PCM_FORMATS = {"f32": 0, "s16": 1}                              # BVC_PCM_F32 / BVC_PCM_S16
PCM_DTYPES = {"f32": torch.float32, "s16": torch.int16}
PCM_DELAYED = 16                                                # BVC_PCM_DELAYED


def pcm_s16_to_f32(x):
    """What a resampler does with s16 input: x / 32768 in float32 (exact)."""
    return x.to(torch.float32) / 32768.0


def pcm_f32_to_s16(y):
    """What a resampler does with s16 output: clamp(rint(y * 32768), -32768, 32767) of the float32 it would have stored; NaN gives 0."""
    q = torch.clamp(torch.round(y.to(torch.float32) * 32768.0), -32768.0, 32767.0)
    return torch.nan_to_num(q, nan=0.0).to(torch.int16)


def resampler_count(rate_in, rate_out, n_inputs):
    """E(N) = max(0, ceil(N up / down) - n_pre_remove): the outputs of ``resample_poly(x, rate_out, rate_in)`` that the first N inputs
    complete.  The library's arithmetic (``bvc_resampler_count``); no device."""
    n = _abi.load().bvc_resampler_count(int(rate_in), int(rate_out), int(n_inputs))
    if n < 0:
        raise ValueError("resampler_count: rates must be positive, n_inputs not negative")
    return int(n)


def resampler_lag(rate_in, rate_out):
    """(n_pre_remove, history) of the filter between two rates: the lag in output samples, and the inputs a row keeps.  No device."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    if _abi.load().bvc_resampler_lag(int(rate_in), int(rate_out), ctypes.byref(a), ctypes.byref(b)) != 0:
        raise ValueError("resampler_lag: rates must be positive")
    return a.value, b.value


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
    hop22 = client_hop(hop, fs, fs_internal)
    lag = resampler_lag(fs, fs_internal)[0]
    if n_client < 0:
        raise ValueError("client_finish_plan: n_client must not be negative")
    len_s = lag + -(-n_client * fs_internal // fs)
    last = max(0, -(-n_client // hop) - 1)                      # the push that holds the client's last sample
    tail = len_s - last * hop22
    return (len_s, last, tail) if tail <= hop22 else (len_s, last + 1, tail - hop22)


class StreamResampler:
    """``batch`` independent rows resampled from ``rate_in`` to ``rate_out`` a chunk at a time (``bvc_resampler_*``): what a row has
    got is a bit-exact prefix of ``preprocess.resample_poly(row, rate_out, rate_in)`` on its own signal, whatever the chunking.

    Rows start idle.  ``open(row, offset)`` resets a row and starts it at sample ``offset`` of the next chunk, ``close(row)`` idles it,
    ``end(row, n_valid)`` ends its stream with the first ``n_valid`` samples of the next chunk, ``flush(row)`` returns the rest.  ``push(x)``
    with x (batch, n <= max_in) returns ``(y (batch, ceil(n up / down)) view, counts (batch,) int64 CPU tensor)``; row b's samples are
    ``y[b, :counts[b]]``, zeros behind them; an idle row's input is never read.  The counts are host arithmetic (``resampler_count``): a
    push does not synchronise.  ``fmt_in`` / ``fmt_out``: "f32" or "s16".  ``delayed=True``: the row's output is zeros(lag) followed by
    the resampled signal, ``ceil(N up / down)`` samples after N inputs - a fixed hop in, a fixed hop out."""

    def __init__(self, batch, rate_in, rate_out, max_in, fmt_in="f32", fmt_out="f32", delayed=False, device=None):
        from . import preprocess
        if fmt_in not in PCM_FORMATS or fmt_out not in PCM_FORMATS:
            raise ValueError(f"sample formats are {sorted(PCM_FORMATS)}")
        if int(rate_in) <= 0 or int(rate_out) <= 0:
            raise ValueError("StreamResampler: rates must be positive")
        self.lib = _abi.load()
        self.dev = torch.device("cuda" if device is None else device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.B, self.rate_in, self.rate_out, self.max_in = batch, int(rate_in), int(rate_out), int(max_in)
        self.fmt_in, self.fmt_out, self.delayed = fmt_in, fmt_out, bool(delayed)
        self.up, self.down, taps, self.lag = preprocess.design(rate_out, rate_in)
        self.max_out = -(-self.max_in * self.up // self.down)
        self.running = set()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            rc = self.lib.bvc_resampler_create(batch, self.rate_in, self.rate_out, self.max_in, PCM_FORMATS[fmt_in],
                                               PCM_FORMATS[fmt_out] | (PCM_DELAYED if delayed else 0), ctypes.byref(h))
            self._call(rc)
            self.handle = h
            if self.up != self.down:        # the offline call's taps are numpy's: hand them in, whatever the C library's exp and sin round to
                taps = taps.astype("float64")
                self._call(self.lib.bvc_resampler_set_taps(h, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(taps)))
        self._counts = (ctypes.c_int32 * batch)()
        self._out = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.bvc_resampler_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _call(self, rc):
        if rc == -1:                                           # BVC_EINVAL: a misuse, the object is untouched
            msg = self.lib.bvc_last_error()
            raise ValueError(msg.decode() if msg else "bvcodec: invalid argument")
        _abi.check(rc)

    def open(self, row, offset=0):
        self._call(self.lib.bvc_resampler_open(self.handle, int(row), int(offset)))
        self.running.add(int(row))

    def close(self, row):
        self._call(self.lib.bvc_resampler_close(self.handle, int(row)))
        self.running.discard(int(row))

    def end(self, row, n_valid):
        self._call(self.lib.bvc_resampler_end(self.handle, int(row), int(n_valid)))

    def push_raw(self, x_ptr, x_row_stride, n_in, y_ptr, y_row_stride, y_offset, stream):
        """The C call on raw device addresses (strides and offset in elements); returns the rows' counts as a list."""
        self._call(self.lib.bvc_resampler_push(self.handle, ctypes.c_void_p(x_ptr), int(x_row_stride), int(n_in), ctypes.c_void_p(y_ptr),
                                               int(y_row_stride), int(y_offset), self._counts, ctypes.c_void_p(stream)))
        return list(self._counts)

    def flush_raw(self, row, y_ptr, stream):
        n = ctypes.c_int32()
        self._call(self.lib.bvc_resampler_flush(self.handle, int(row), ctypes.c_void_p(y_ptr), ctypes.byref(n), ctypes.c_void_p(stream)))
        self.running.discard(int(row))
        return n.value

    @torch.no_grad()
    def push(self, x):
        if x.dim() != 2 or x.shape[0] != self.B or x.shape[1] > self.max_in or x.dtype != PCM_DTYPES[self.fmt_in]:
            raise ValueError(f"StreamResampler.push: expected a {PCM_DTYPES[self.fmt_in]} tensor ({self.B}, n <= {self.max_in})")
        x = x.to(self.dev).contiguous()
        n = x.shape[1]
        if self._out is None:
            self._out = torch.empty(self.B, max(1, self.max_out), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            counts = self.push_raw(x.data_ptr() if n else self._out.data_ptr(), max(n, 1), n, self._out.data_ptr(), self._out.shape[1], 0,
                                   torch.cuda.current_stream(self.dev).cuda_stream)
        return self._out[:, :-(-n * self.up // self.down)], torch.tensor(counts, dtype=torch.int64)

    @torch.no_grad()
    def flush(self, row):
        """The rest of the row's outputs (at most ``lag`` samples, a new tensor); the row is idle afterwards."""
        y = torch.empty(max(1, self.lag), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            n = self.flush_raw(row, y.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream)
        return y[:n]


class StreamingCodec:
    """BASELINE configs[4]: `batch` parallel streams, a fixed hop of new samples per tick, encode + decode of the frames
    each hop completes in ONE library call (``bvc_stream_codec_tick``: one persistent launch per recurrence where that
    kernel is available, else a hipGraph of launch-per-layer kernels replayed once the streams are warm).  State (sample buffer, both GRU states, the generator's activation history) lives in the library.

    ``push(x)`` with x (batch, hop) returns (codes (batch, k, z_dim), wav (batch, 256 k)) for the k frames completed;
    they equal the offline ``encode`` / ``decode`` of the whole signal on those frames (tests/test_gpu_streaming.py).
    The returned tensors are views of the state's output buffers: valid until the next push.

    Every row is a *slot* with a life of its own.  Between two pushes ``open(slot, bitrate)`` starts a new stream in an idle row
    (the samples pushed into that row from then on are its samples 0, 1, 2, ...; the returned delay says how many samples the
    library holds the row back so that the stream's frames fall on the session's), ``close(slot)`` ends it, ``set_bitrate(slot,
    bitrate)`` changes its bits per frame from the next push on, and ``slot_frames(slot)`` tells which frames of the last push
    belong to the slot's stream.  Those frames are bit for bit the offline ``encode`` / ``decode`` of that stream's own signal alone.
    A stream that is closed has got the frames its samples complete (``(n - delay - 768) // 256 + 1`` after n samples); the last
    two frames of the offline call need the right reflect padding: end the stream with ``finish`` instead to get them.  Idle rows of
    ``x`` are never read.  ``open_all=False`` starts with every slot idle.

    ``finish(slot, n_last)`` ends a stream completely where ``close`` cuts it off: the next push's row holds the stream's last
    ``n_last`` samples, the library writes the right reflect padding behind them and the slot *drains* - this and the next pushes
    emit its remaining frames (``slot_frames`` says which, ``finish_plan`` predicts them), ALL ``num_frames(n)`` frames of the offline
    ``encode``, and then the slot is idle (``slot_state``).

    ``direction`` splits the loopback into the two halves a deployment runs in different places.  ``"send"``: ``push(x)`` returns
    ``(packets (batch, k, bytes_per_frame) uint8, codes)``: the front-end and the encoder only; row b's frames hold its own
    ``active_bits`` leading bits in the layout of ``model.pack`` and zeros behind them.  ``"recv"``: ``push_packets(packets,
    present=None)`` with packets ``(batch, k, bytes_per_frame)``, 1 <= k <= ``kmax``, returns wav ``(batch, 256 k)``: the decoder and
    the generator only.  ``present (batch, k)``: 0 marks a frame that did not arrive; it is decoded as a frame of no bits (codes all
    0.5) and the state moves on.  ``hop`` means nothing to a receive session, ``open`` always returns 0 there.

    ``conceal="prior"`` (receive sessions only; ``set_conceal`` switches between two pushes): a lost frame of an open slot is generated
    from the model's prior net at the decoder's own state instead, with the slot's current bit count, and ``filled_codes()`` gives the
    codes with the gaps filled; every stream equals ``model.decode(codes, n, lost=..., bitrate=...)`` of its own packets alone.

    ``repair=W`` (receive sessions only, 0 .. 64 frames, 0 = off; ``set_repair`` changes it between two pushes): a network mostly
    reorders, and a frame decoded without its bits leaves the decoder's state off the sender's for as long as the model remembers.
    With a window the session keeps the decoder state in front of, and the input of, every push that holds one of its last W frames.
    ``late(slot, stream_frame, packet)`` hands in a frame that was pushed as not present (``stream_frame`` counts as the third value of
    ``slot_frames`` does) and returns whether it was taken: the slot is running, the frame is its current stream's, still within the
    window and still marked lost (``repair_plan`` states the rule).  The next push first decodes every such row again from the kept
    state in front of its earliest late frame - with the bit counts those frames had, generating again what is still lost - and
    continues from a state that is bit for bit that of a session which got the packet in time: its ``filled_codes`` equal that
    session's from this push on, its samples once the generator's history has flushed (``CONTEXT_FRAMES`` later).  What was
    returned before is not touched.  ``set_conceal`` and ``set_repair`` empty the window.

    ``client_rate=fs`` (8000 .. 48000 Hz; None or the model's own 22050: the session as above), ``sample_format="f32"`` or ``"s16"``:
    the session speaks the client's rate and format on both sides.  ``hop`` then counts client samples and must be a whole number of
    internal ones (``hop * 22050 % fs == 0``, else ``ValueError``: 480 samples at 48 kHz would be 220.5; 20 ms hops of the six usual
    rates pass).  One ``StreamResampler`` sits in front of the session's input buffer (send, duplex) and one behind its output buffer
    (recv, duplex), both on the session's stream, writing into and reading from the session's own buffers.  Send side: with ``lag`` =
    ``self.lag`` (``n_pre_remove`` of ``design(22050, fs)``: 14 samples at 16 kHz, 11 at 48 kHz) a slot's internal stream is S =
    zeros(lag) ++ resample_poly(x, 22050, fs) - the offline resampling of the client's signal, ``lag`` samples late because the filter
    looks that far ahead; ``open`` returns the session's delay as before, in internal samples, and the stream is ``lag`` later than
    that.  The slot's packets and codes equal ``model.encode(S[None], bitrate)`` on the frames the session emits, bit for bit, and
    ``finish(slot, n_last)`` (``n_last`` in client samples) ends the slot with all ``num_frames(len(S))`` of them.  Receive side: after
    N internal samples of a stream the client has ``resample_poly(wav22[:N], fs, 22050)[:E(N)]`` (``resampler_count``), ``wav22`` what
    the same session without ``client_rate`` returns; the last ``lag'`` (11 .. 22) client samples of a stream stay inside - receive
    sessions have no ``finish``.  ``push_packets`` then returns ``(wav (batch, n_max) view, counts (batch,) int64 CPU tensor)`` - row
    b's samples are ``wav[b, :counts[b]]`` - and a duplex ``push`` ``(codes, wav, counts)``; a send ``push`` returns what it returned
    before.  ``"s16"`` takes and returns int16 tensors (in: x / 32768; out: clamp(rint(y * 32768)) of the float32 result, NaN 0).
    Concealment, repair, ``set_bitrate`` and ``late`` act on the inner session unchanged; ``close`` also idles the row's resamplers.

    ``vbr=dict(bitrates=(1500, 3000, 6000), target=0.35, rate_cap=None, burst=None)`` (send and duplex sessions; ``bitrate`` is then
    ignored): the session chooses every frame's rate itself, as ``model.encode_vbr(x, target, bitrates, rate_cap=, burst=)`` does -
    the lowest of ``bitrates`` at which the decoded mel lies within the slot's ``target``, under the slot's own token bucket where
    ``rate_cap`` [bit/s] is given.  ``open(slot, target=None)`` starts a stream with that (None: the session's) target, zero state
    and a full bucket, ``set_target(slot, target)`` changes it from the next push on; ``set_bitrate`` is refused.  ``push`` returns
    what it returns without ``vbr``, the packets on the wire of ``model.pack_vbr``: ``bytes_per_frame = 1 + ceil(z_dim / 8)``, byte 0
    the frame's bit count.  ``last_bits`` (batch, k) float and ``last_sizes`` (batch, k) int32 - the bytes of each frame worth sending -
    are views valid until the next push.  Every stream equals ``model.encode_vbr`` of its own signal alone, bit for bit.  On a receive
    session ``vbr=True`` selects that wire: every present frame says how many bits it holds, ``bitrate`` is the count a lost frame is
    concealed with (``conceal="prior"``), ``last_bits`` what the last push read.  Not with ``repair``, not on a fixed-rate model."""

    DIRECTIONS = {"duplex": 0, "send": 1, "recv": 2}
    CONCEAL = {"none": 0, "prior": 1}

    def __init__(self, model, batch, bitrate, hop=441, device=None, open_all=True, direction="duplex", conceal="none", repair=0,
                 client_rate=None, sample_format="f32", vbr=None):
        self.vbr = self._check_vbr(model, direction, repair, vbr)     # ValueError before anything is created
        if sample_format not in PCM_FORMATS:
            raise ValueError(f"sample_format must be one of {sorted(PCM_FORMATS)}")
        if client_rate is None and sample_format != "f32":
            raise ValueError("sample_format: a session without client_rate speaks float32")
        fs = model.conf["fs"]
        if client_rate is not None and (client_rate != int(client_rate) or client_rate <= 0):
            raise ValueError(f"client_rate must be a positive number of Hz, not {client_rate}")
        converting = client_rate is not None and (int(client_rate) != fs or sample_format != "f32")
        self.client_rate, self.sample_format, self.client_hop = (int(client_rate) if converting else None), sample_format, hop
        if converting and direction != "recv":
            hop = client_hop(hop, int(client_rate), fs)         # ValueError before anything is created
        if direction not in self.DIRECTIONS:
            raise ValueError(f"direction must be one of {sorted(self.DIRECTIONS)}")
        if conceal not in self.CONCEAL:
            raise ValueError(f"conceal must be one of {sorted(self.CONCEAL)}")
        if conceal != "none" and direction != "recv":
            raise ValueError("conceal: only a receive session has lost frames to conceal")
        if repair and direction != "recv":
            raise ValueError("repair: only a receive session has late packets to repair from")
        if direction != "send" and not is_causal(model.conf):
            raise ValueError("StreamingCodec: " + not_causal_message(model.conf))
        self.direction = direction
        eng = model.engine(None if device is None else torch.empty(0, device=device))
        if direction == "recv":
            hop = 0
        self.eng, self.B, self.hop = eng, batch, hop
        self.dev = eng.device
        self.z = model.conf["z_dim"]
        self.spf = math.prod(model.conf["vocoder_config"]["upsample_rates"])
        self.stream = torch.cuda.Stream(self.dev)          # a tick may be captured into a hipGraph: not possible on the default stream
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            if self.vbr is not None:
                v = self.vbr
                lad = (ctypes.c_int32 * len(v["ladder"]))(*v["ladder"]) if v["ladder"] else None
                _abi.check(eng.lib.bvc_stream_codec_create_vbr(
                    eng.handle, batch, hop, lad, len(v["ladder"]), float(v["target"]), v["rate_q8"], v["burst_q8"],
                    float(model.bits_per_frame(bitrate)), float(SCALING), float(SCALING), self.DIRECTIONS[direction], ctypes.byref(h)))
            elif direction == "duplex":
                _abi.check(eng.lib.bvc_stream_codec_create(eng.handle, batch, hop, float(model.bits_per_frame(bitrate)), float(SCALING),
                                                           float(SCALING), ctypes.byref(h)))
            else:
                _abi.check(eng.lib.bvc_stream_codec_create_dir(eng.handle, batch, hop, float(model.bits_per_frame(bitrate)),
                                                               float(SCALING), float(SCALING), self.DIRECTIONS[direction], ctypes.byref(h)))
        self.handle = h
        pin, pc, pw, kmax = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        _abi.check(eng.lib.bvc_stream_codec_buffers(h, ctypes.byref(pin), ctypes.byref(pc), ctypes.byref(pw), ctypes.byref(kmax)))
        self.kmax = kmax.value
        self._in = torch.as_tensor(_DeviceView(pin.value, (batch, hop)), device=self.dev) if pin.value else None
        self._codes_ptr, self._wav_ptr = pc.value, pw.value
        pp, pr, bpf = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        _abi.check(eng.lib.bvc_stream_codec_packets(h, ctypes.byref(pp), ctypes.byref(pr), ctypes.byref(bpf)))
        self.bytes_per_frame = bpf.value
        self._packets = self._present = None
        if pp.value:                                           # (batch, kmax, bytes_per_frame) / (batch, kmax) whatever a tick's frame count
            self._packets = torch.as_tensor(_DeviceView(pp.value, (batch, self.kmax, bpf.value), "|u1"), device=self.dev)
            self._present = torch.as_tensor(_DeviceView(pr.value, (batch, self.kmax), "|u1"), device=self.dev)
        self._sizes_ptr = self._bits_ptr = None
        self._last_k = 0
        if self.vbr is not None:
            ps, pb = ctypes.c_void_p(), ctypes.c_void_p()
            _abi.check(eng.lib.bvc_stream_codec_sizes(h, ctypes.byref(ps)))
            _abi.check(eng.lib.bvc_stream_codec_bits(h, ctypes.byref(pb)))
            self._sizes_ptr, self._bits_ptr = ps.value, pb.value
        self.frames = 0
        self._model = model
        self._rs_in = self._rs_out = None
        if converting:
            self._client_setup(fs, open_all)
        if not open_all:
            for b in range(batch):
                self.close(b)
        self.conceal = "none"
        if conceal != "none":
            self.set_conceal(conceal)
        self.repair = 0
        if repair:
            self.set_repair(repair)

    VBR_KEYS = ("bitrates", "target", "rate_cap", "burst")

    @classmethod
    def _check_vbr(cls, model, direction, repair, vbr):
        """The ``vbr`` keyword as what bvc_stream_codec_create_vbr takes - dict(ladder, target, rate_q8, burst_q8), burst_q8 = -1
        without a cap - or None for a session without it; ValueError for what the library would refuse."""
        if vbr is None or vbr is False:
            return None
        from .model import _check_ladder, cap_q8
        conf = model.conf
        if not conf["var_bit"]:
            raise ValueError("vbr: a fixed-rate model (var_bit = false) has no bit mask to choose")
        if direction == "recv":
            if vbr is not True:
                raise ValueError("vbr: a receive session takes vbr=True (the wire with a bit count per frame); the sender chooses the rates")
            if repair:
                raise ValueError("vbr: no repair window on the wire with a bit count per frame")
            return dict(ladder=[], target=0.0, rate_q8=0, burst_q8=-1)
        if not isinstance(vbr, dict):
            raise ValueError("vbr: a send or duplex session takes dict(bitrates=, target=, rate_cap=, burst=)")
        unknown = sorted(set(vbr) - set(cls.VBR_KEYS))
        if unknown:
            raise ValueError(f"vbr: unknown keys {unknown}; known: {list(cls.VBR_KEYS)}")
        z = conf["z_dim"]
        rungs = [int(min(z, max(0.0, model.bits_per_frame(r)))) for r in vbr.get("bitrates", (1500, 3000, 6000))]
        _check_ladder(rungs, z, True)
        target = float(vbr.get("target", 0.35))
        cap = cap_q8(conf, rungs, vbr.get("rate_cap"), vbr.get("burst"))
        return dict(ladder=rungs, target=target, rate_q8=cap[0] if cap else 0, burst_q8=cap[1] if cap else -1)

    @property
    def last_bits(self):
        """vbr sessions: the bit count of every frame of the last push, (batch, k) float; a view valid until the next push."""
        return self._vbr_view(self._bits_ptr, "<f4")

    @property
    def last_sizes(self):
        """vbr sessions: 1 + ceil(bits / 8) of every frame of the last push - the bytes worth sending - (batch, k) int32; a view."""
        return self._vbr_view(self._sizes_ptr, "<i4")

    def _vbr_view(self, ptr, typestr):
        if not ptr:
            raise ValueError("last_bits / last_sizes: not a vbr session")
        return torch.as_tensor(_DeviceView(ptr, (self.B, self.kmax), typestr), device=self.dev)[:, :self._last_k]

    def set_target(self, slot, target):
        """vbr send / duplex sessions: the distortion target of an open slot from the next push on."""
        self._slot_call(self.eng.lib.bvc_stream_codec_set_target(self.handle, int(slot), float(target)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.eng.lib.bvc_stream_codec_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _client_setup(self, fs, open_all):
        """The resamplers of a rate-converting session: one in front of d_in (delayed: a fixed hop in, a fixed hop out), one behind
        d_wav, both on the session's stream, writing into / reading from the session's own buffers."""
        rate, fmt, B = self.client_rate, self.sample_format, self.B
        self._n_push = 0                                       # pushes so far
        self._open_push = [0] * B                              # the push that took a slot's first client samples
        self._ending = {}                                      # slot -> (internal n_last, spills) of a finish the next push carries out
        self._carry = {}                                       # slot -> (from, count): the part of a flushed tail that goes into the next push
        self._out_wait, self._out_drain = set(), set()         # slots whose samples have yet to start / are about to end on the wav side
        if self.direction != "recv":
            self._rs_in = StreamResampler(B, rate, fs, self.client_hop, fmt, "f32", delayed=True, device=self.dev)
            self.lag = self._rs_in.lag
            self._tail = torch.zeros(B, max(1, self.lag), device=self.dev)
            self.hop, self._hop_in = self.client_hop, self.hop  # ``hop`` counts client samples from here on
        if self.direction != "send":
            self._rs_out = StreamResampler(B, fs, rate, self.kmax * self.spf, "f32", fmt, device=self.dev)
            self._cwav = torch.zeros(B, max(1, self._rs_out.max_out), dtype=PCM_DTYPES[fmt], device=self.dev)
        if open_all:
            for b in range(B):
                self._client_open(b)

    def _client_open(self, slot):
        if self._rs_in is not None:
            self._rs_in.close(slot)
            self._rs_in.open(slot, 0)
            self._open_push[slot] = self._n_push
            self._ending.pop(slot, None)
            self._carry.pop(slot, None)
        if self._rs_out is not None:
            self._rs_out.close(slot)
            self._out_wait.add(slot)
            self._out_drain.discard(slot)

    def _client_close(self, slot):
        if self._rs_in is not None:
            self._rs_in.close(slot)
            self._ending.pop(slot, None)
            self._carry.pop(slot, None)
        if self._rs_out is not None:
            self._rs_out.close(slot)
            self._out_wait.discard(slot)
            self._out_drain.discard(slot)

    def _client_in(self, x):
        """A hop of client samples -> d_in, inside the session's stream: one resampler push for all rows, and for a row that ends the
        flush of its last ``lag`` samples - straight into d_in where they fit the hop, else through a buffer into this hop and the next."""
        if tuple(x.shape) != (self.B, self.hop) or x.dtype != PCM_DTYPES[self.sample_format]:
            raise ValueError(f"push: expected a {PCM_DTYPES[self.sample_format]} tensor ({self.B}, {self.hop})")
        x = x.to(self.dev).contiguous()
        rs, hop22, s = self._rs_in, self._hop_in, self.stream.cuda_stream
        counts = rs.push_raw(x.data_ptr(), self.hop, self.hop, self._in.data_ptr(), hop22, 0, s)
        for slot, (frm, n) in list(self._carry.items()):       # the rest of a tail that spilled: the row is idle, its hop zeros
            self._in[slot, :n].copy_(self._tail[slot, frm:frm + n], non_blocking=True)
            self._slot_call(self.eng.lib.bvc_stream_codec_finish(self.handle, slot, n))
            self._out_drain.add(slot)
            del self._carry[slot]
        for slot, (n22, spills) in list(self._ending.items()):
            e = counts[slot]                                   # what the row's last client samples completed
            if not spills:
                rs.flush_raw(slot, self._in.data_ptr() + 4 * (slot * hop22 + e), s)
                self._slot_call(self.eng.lib.bvc_stream_codec_finish(self.handle, slot, n22))
                self._out_drain.add(slot)
            else:
                rs.flush_raw(slot, self._tail.data_ptr() + 4 * slot * self._tail.shape[1], s)
                self._in[slot, e:].copy_(self._tail[slot, :hop22 - e], non_blocking=True)
                self._carry[slot] = (hop22 - e, n22)
            del self._ending[slot]
        self._n_push += 1

    def _client_out(self, k):
        """The tick's k frames of d_wav -> client samples: (wav (B, n_max) view, counts (B,) int64 CPU tensor)."""
        rs = self._rs_out
        for slot in list(self._out_wait):                      # a row's resampler starts with its stream's frame 0
            first, count, frame0 = self.slot_frames(slot)
            if count > 0 and frame0 == 0:
                rs.open(slot, self.spf * first)
                self._out_wait.discard(slot)
        for slot in list(self._out_drain):                     # ... and ends with its last one (the last lag' samples stay inside)
            if self.slot_state(slot) == "idle":
                first, count, _ = self.slot_frames(slot)
                if slot in rs.running:
                    rs.end(slot, self.spf * (first + max(0, count)))
                    rs.running.discard(slot)
                self._out_drain.discard(slot)
                self._out_wait.discard(slot)                   # (a stream that ended before its frame 0 came out)
        n = k * self.spf
        counts = rs.push_raw(self._wav_ptr, n, n, self._cwav.data_ptr(), self._cwav.shape[1], 0, self.stream.cuda_stream)
        return self._cwav[:, :-(-n * rs.up // rs.down)], torch.tensor(counts, dtype=torch.int64)

    def _slot_call(self, rc):
        if rc == -1:                                           # BVC_EINVAL: a misuse of the slot calls, the session is untouched
            msg = self.eng.lib.bvc_last_error()
            raise ValueError(msg.decode() if msg else "bvcodec: invalid argument")
        _abi.check(rc)

    def open(self, slot, bitrate=None, target=None):
        """Start a new stream in idle row `slot` from the next push on; returns its delay in (internal) samples.  A rate-converting
        send side delays the stream by ``lag`` more: its filter looks that far ahead (``self.lag`` internal samples).  A vbr send or
        duplex session takes ``target`` (None: the session's) instead of ``bitrate``."""
        choosing = self.vbr is not None and self.direction != "recv"
        if choosing and bitrate is not None:
            raise ValueError("open: a vbr session chooses its own rates (open(slot, target=...))")
        if not choosing and (bitrate is None or target is not None):
            raise ValueError("open: open(slot, bitrate)" if bitrate is None else "open: target belongs to a vbr send or duplex session")
        d = ctypes.c_int32()
        self._slot_call(self.eng.lib.bvc_stream_codec_open(self.handle, int(slot), 0.0 if choosing else float(self._model.bits_per_frame(bitrate)),
                                                           ctypes.byref(d)))
        if choosing and target is not None:
            self.set_target(slot, target)
        if self.client_rate is not None:
            self._client_open(int(slot))
        return d.value

    def close(self, slot):
        """The row is idle from the next push on (ask ``slot_frames`` first)."""
        self._slot_call(self.eng.lib.bvc_stream_codec_close(self.handle, int(slot)))
        if self.client_rate is not None:
            self._client_close(int(slot))

    def set_bitrate(self, slot, bitrate):
        """Bits per frame of an open slot from the next push on (variable-bitrate models only)."""
        self._slot_call(self.eng.lib.bvc_stream_codec_set_bits(self.handle, int(slot), float(self._model.bits_per_frame(bitrate))))

    def slot_frames(self, slot):
        """(first, count, stream_frame0): frames [first, first + count) of the last push are the slot's stream's frames
        stream_frame0, stream_frame0 + 1, ...; count is 0 for an idle slot and before the stream's frame 0."""
        f, n, s0 = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._slot_call(self.eng.lib.bvc_stream_codec_slot_frames(self.handle, int(slot), ctypes.byref(f), ctypes.byref(n),
                                                                  ctypes.byref(s0)))
        return f.value, n.value, s0.value

    def finish(self, slot, n_last=None):
        """The stream in `slot` ends with the first `n_last` samples of the next push's row (None: the whole hop; 0: it ended with
        the last push).  The slot drains from that push on and is idle once its last frame is out.  On a rate-converting session `n_last`
        counts client samples; the stream's internal signal S = zeros(lag) ++ resample_poly(x, 22050, client_rate) ends ``lag`` samples
        later, so the drain starts with the next push, or the one after it where the flushed tail does not fit the hop
        (``client_finish_plan``); the slot ends with all ``num_frames(len(S))`` frames."""
        if self._rs_in is not None:
            return self._client_finish(int(slot), self.hop if n_last is None else int(n_last))
        self._slot_call(self.eng.lib.bvc_stream_codec_finish(self.handle, int(slot), int(self.hop if n_last is None else n_last)))

    def _client_finish(self, slot, n_last):
        if not 0 <= slot < self.B or self.slot_state(slot) != "running" or slot in self._ending or slot in self._carry:
            raise ValueError(f"finish: slot {slot} is not a running stream")
        if not 0 <= n_last <= self.hop:
            raise ValueError(f"finish: n_last {n_last} outside 0..{self.hop}")
        push = self._n_push - self._open_push[slot]            # the coming push, counted from the stream's first
        c = self._model.conf
        len_s, at, n22 = client_finish_plan(push * self.hop + n_last, self.hop, self.client_rate, c["fs"])
        if len_s <= c["winsize"] - c["hopsize"] - c["mel_pad_left"]:
            raise ValueError(f"finish: a stream of {len_s} internal samples is too short for the right reflect padding")
        self._rs_in.end(slot, n_last)
        self._ending[slot] = (n22, at > push)

    def set_conceal(self, mode):
        """What the next pushes do with a lost frame: "none" (a frame of no bits) or "prior" (generated from the prior net).
        Receive sessions only."""
        if mode not in self.CONCEAL:
            raise ValueError(f"conceal must be one of {sorted(self.CONCEAL)}")
        self._slot_call(self.eng.lib.bvc_stream_codec_set_conceal(self.handle, self.CONCEAL[mode]))
        self.conceal = mode

    def set_repair(self, window):
        """The repair window in frames (0 .. 64, 0: off) from the next push on; empties the window.  Receive sessions only."""
        with torch.cuda.device(self.dev):
            self._slot_call(self.eng.lib.bvc_stream_codec_set_repair(self.handle, int(window)))
        self.repair = int(window)

    def late(self, slot, stream_frame, packet):
        """A frame of the stream in `slot` that was pushed as not present: its index in the stream and its bytes (uint8 tensor or
        bytes; fewer than ``bytes_per_frame`` are taken as the leading ones).  True if the next push repairs the row with it."""
        raw = bytes(packet) if isinstance(packet, (bytes, bytearray)) else bytes(packet.detach().to("cpu", torch.uint8).reshape(-1).tolist())
        if len(raw) > self.bytes_per_frame:
            raise ValueError(f"late: a frame has at most {self.bytes_per_frame} bytes")
        buf = (ctypes.c_uint8 * self.bytes_per_frame)(*raw)
        taken = ctypes.c_int32()
        with torch.cuda.device(self.dev):
            self._slot_call(self.eng.lib.bvc_stream_codec_late(self.handle, int(slot), int(stream_frame), ctypes.cast(buf, ctypes.c_void_p),
                                                               ctypes.byref(taken)))
        return bool(taken.value)

    def filled_codes(self, k):
        """Receive session: the codes (batch, k, z_dim) the last push of k frames decoded - unpacked, and with ``conceal="prior"`` with
        the lost frames filled; a view of the session's buffer, valid until the next push."""
        return torch.as_tensor(_DeviceView(self._codes_ptr, (self.B, k, self.z)), device=self.dev)

    def slot_state(self, slot):
        """"idle", "waiting" (open, frame 0 still to come), "running" or "draining" (finished, frames still to come)."""
        v = ctypes.c_int32()
        self._slot_call(self.eng.lib.bvc_stream_codec_slot_state(self.handle, int(slot), ctypes.byref(v)))
        return ("idle", "waiting", "running", "draining")[v.value]

    @torch.no_grad()
    def push_packets(self, packets, present=None):
        """Receive session: packets (batch, k, bytes_per_frame) uint8 (fewer bytes per frame are taken as the leading ones),
        present (batch, k) (None: everything arrived) -> wav (batch, 256 k), a view of the session's buffer, valid until the next push."""
        if packets.dim() != 3 or packets.shape[0] != self.B or packets.shape[2] > self.bytes_per_frame or packets.dtype != torch.uint8:
            raise ValueError(f"push_packets: expected uint8 packets ({self.B}, k, <= {self.bytes_per_frame})")
        k = packets.shape[1]
        if self.direction != "recv" or not 1 <= k <= self.kmax:    # the library's refusal (BVC_EINVAL), session untouched
            self._slot_call(self.eng.lib.bvc_stream_codec_tick_recv(self.handle, k, ctypes.c_void_p(self.stream.cuda_stream)))
            raise ValueError("push_packets: refused")
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream), torch.cuda.device(self.dev):
            self._packets[:, :k, :packets.shape[2]].copy_(packets.to(self.dev), non_blocking=True)
            if present is None:
                self._present[:, :k].fill_(1)
            else:
                self._present[:, :k].copy_(present.to(self.dev).ne(0).to(torch.uint8).reshape(self.B, k), non_blocking=True)
            self._slot_call(self.eng.lib.bvc_stream_codec_tick_recv(self.handle, k, ctypes.c_void_p(self.stream.cuda_stream)))
            if self._rs_out is not None:
                out = self._client_out(k)
        cur.wait_stream(self.stream)
        self.frames += k
        self._last_k = k
        if self._rs_out is not None:
            return out
        return torch.as_tensor(_DeviceView(self._wav_ptr, (self.B, k * self.spf)), device=self.dev)

    @torch.no_grad()
    def push(self, x):
        if self.direction == "recv":                           # the library's refusal (BVC_EINVAL), session untouched
            self._slot_call(self.eng.lib.bvc_stream_codec_tick(self.handle, None, ctypes.c_void_p(self.stream.cuda_stream)))
            raise ValueError("push: a receive session takes packets (push_packets)")
        assert tuple(x.shape) == (self.B, self.hop)
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        k = ctypes.c_int32()
        out = None
        with torch.cuda.stream(self.stream), torch.cuda.device(self.dev):
            if self._rs_in is not None:
                self._client_in(x)
            else:
                self._in.copy_(x.to(self.dev, torch.float32), non_blocking=True)
            _abi.check(self.eng.lib.bvc_stream_codec_tick(self.handle, ctypes.byref(k), ctypes.c_void_p(self.stream.cuda_stream)))
            if self._rs_out is not None and k.value > 0:
                out = self._client_out(k.value)
        cur.wait_stream(self.stream)
        k = k.value
        self.frames += k
        self._last_k = k
        send = self.direction == "send"
        if self._rs_out is not None:                           # a rate-converting duplex session: (codes, wav, counts)
            codes = torch.as_tensor(_DeviceView(self._codes_ptr, (self.B, k, self.z)), device=self.dev) if k else \
                torch.empty(self.B, 0, self.z, device=self.dev)
            if out is None:
                out = (torch.empty(self.B, 0, dtype=PCM_DTYPES[self.sample_format], device=self.dev), torch.zeros(self.B, dtype=torch.int64))
            return codes, out[0], out[1]
        if k == 0:
            first = torch.empty(self.B, 0, self.bytes_per_frame, dtype=torch.uint8, device=self.dev) if send else \
                torch.empty(self.B, 0, self.z, device=self.dev)
            return first, (torch.empty(self.B, 0, self.z, device=self.dev) if send else torch.empty(self.B, 0, device=self.dev))
        codes = torch.as_tensor(_DeviceView(self._codes_ptr, (self.B, k, self.z)), device=self.dev)
        if send:
            return self._packets[:, :k], codes
        wav = torch.as_tensor(_DeviceView(self._wav_ptr, (self.B, k * self.spf)), device=self.dev)
        return codes, wav
