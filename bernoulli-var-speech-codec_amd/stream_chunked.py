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
  the context scheme.  A generator with symmetric layers is not causal, but its look-ahead is bounded
  (``config.generator_lookahead``): ``lookahead=True`` runs the library's state behind that delay
  (``bvc_vocoder_stream_create_lookahead``) - a push returns the samples that became final, ``flush`` /
  ``finish`` the rest, bit for bit the offline call.

``tests/test_gpu_streaming.py`` checks that any chunking reproduces the offline encode()/decode().
"""
import ctypes
import math

import torch

from . import _abi
from .config import generator_lookahead, is_antialiased, is_causal, not_causal_message
from .model import SCALING
from .stream_plans import CONTEXT_FRAMES


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
    """Handle of the library's incremental generator state for `batch` parallel streams.

    ``lookahead=True``: the state behind a look-ahead window (``bvc_vocoder_stream_create_lookahead``), which also runs generators
    with symmetric layers.  ``.lookahead`` is the delay in samples (0 for a causal generator); ``push`` then returns the samples that
    became final with its frames - ``(B, n)``, ``n`` possibly 0 - and ``flush`` the rest up to the generator's length.  The pushes and
    the flush concatenated are the offline call's bits."""

    def __init__(self, engine, batch, max_frames_per_push, lookahead=False):
        if is_antialiased(engine.conf) if lookahead else not is_causal(engine.conf):
            raise ValueError("VocoderStream: " + not_causal_message(engine.conf)
                             + ("" if lookahead or is_antialiased(engine.conf) else
                                f"; lookahead=True streams it behind {generator_lookahead(engine.conf)} samples of delay"))
        self.eng = engine
        self.B = batch
        self.kmax = max_frames_per_push
        self.spf = math.prod(engine.conf["vocoder_config"]["upsample_rates"])
        self.windowed = bool(lookahead)
        self.lookahead = generator_lookahead(engine.conf) if lookahead else 0
        self.handle = _abi.Handle(engine.lib.bvc_vocoder_stream_destroy, engine)
        engine.call("bvc_vocoder_stream_create_lookahead" if lookahead else "bvc_vocoder_stream_create", engine.handle, batch,
                    max_frames_per_push, ctypes.byref(self.handle), stream=False)

    def reset(self):
        self.eng.call("bvc_vocoder_stream_reset", self.handle)

    def samples(self, k):
        """Samples per row the next push of k frames (1 <= k <= max_frames_per_push) writes, or with k = -1 the flush."""
        return int(self.eng.lib.bvc_vocoder_stream_samples(self.handle, k))

    def _windowed(self, mel, scale_div):
        """One library call of a look-ahead state: a push of mel's frames, or with mel None the flush.  A misuse (a push after the
        flush) is the library's BVC_EINVAL: ValueError."""
        out = torch.empty(self.B, self.samples(-1 if mel is None else mel.shape[1]), device=self.eng.device)
        with torch.cuda.device(self.eng.device):
            if mel is None:
                _abi.check_arg(self.eng.lib.bvc_vocoder_stream_flush(self.handle, float(scale_div), _abi.ptr(out), self.eng.stream()))
            else:
                _abi.check_arg(self.eng.lib.bvc_vocoder_stream_push(self.handle, _abi.ptr(mel), mel.shape[1], float(scale_div), _abi.ptr(out),
                                                                    self.eng.stream()))
        return out

    def flush(self, scale_div=1.0):
        """End of the signal (look-ahead states): the samples no push has returned, up to the generator's length; afterwards only
        ``reset`` is legal."""
        if not self.windowed:
            raise ValueError("VocoderStream.flush: a state made with lookahead=True has a flush")
        return self._windowed(None, scale_div)

    def push(self, mel, scale_div=1.0):
        """mel (B, k, num_mels) time-major on the engine's device -> wav (B, k*256); behind a look-ahead window the samples that
        became final, (B, n)."""
        B, k, _ = mel.shape
        assert B == self.B
        if self.windowed:                                      # longer chunks go through in kmax-frame pieces
            pieces = [self._windowed(mel[:, f:f + self.kmax].contiguous(), scale_div) for f in range(0, k, self.kmax)]
            return torch.cat(pieces, 1) if pieces else torch.empty(B, 0, device=self.eng.device)
        out = torch.empty(B, k * self.spf, device=self.eng.device)
        for f in range(0, k, self.kmax):                       # longer chunks go through in kmax-frame pieces
            n = min(self.kmax, k - f)
            piece = mel[:, f:f + n].contiguous()
            dst = out if n == k else torch.empty(B, n * self.spf, device=self.eng.device)
            self.eng.call("bvc_vocoder_stream_push", self.handle, _abi.ptr(piece), n, float(scale_div), _abi.ptr(dst))
            if dst is not out:
                out[:, f * self.spf:(f + n) * self.spf] = dst
        return out


class StreamingDecoder:
    """``lookahead=True``: the generator runs behind its look-ahead window (``VocoderStream(lookahead=True)``), which admits
    symmetric layers: ``push`` returns the samples that became final - ``.lookahead`` samples behind the frames pushed - and
    ``finish(length)`` the rest, so that ``cat(pushes + [finish(length)])`` is ``model.decode(codes, length)``."""

    def __init__(self, model, batch, device=None, incremental=True, max_frames_per_push=8, lookahead=False):
        if lookahead and not incremental:                      # the context scheme counts on causality
            raise ValueError("StreamingDecoder: lookahead=True runs the incremental generator; incremental=False counts on a causal one")
        if is_antialiased(model.conf) if lookahead else not is_causal(model.conf):
            raise ValueError("StreamingDecoder: " + not_causal_message(model.conf)
                             + ("" if lookahead or is_antialiased(model.conf) else
                                f"; lookahead=True streams it behind {generator_lookahead(model.conf)} samples of delay"))
        self.m = model
        self.B = batch
        eng = model.engine(None if device is None else torch.empty(0, device=device))
        self.dev = eng.device
        c = model.conf
        self.h = torch.zeros(1, batch, c["h_dim"], device=self.dev)
        self.ctx = torch.empty(batch, 0, c["num_mels"], device=self.dev)     # last CONTEXT_FRAMES mel frames
        self.spf = math.prod(c["vocoder_config"]["upsample_rates"])         # samples per frame (256)
        self.tail = None
        self.voc = VocoderStream(eng, batch, max_frames_per_push, lookahead=lookahead) if incremental else None
        self.windowed = bool(lookahead)
        self.lookahead = self.voc.lookahead if lookahead else 0
        self.emitted = 0                                       # samples the pushes have returned (look-ahead window)

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
        if self.windowed:
            out = self.voc.push(mel, SCALING)
            self.emitted += out.shape[1]
            return out
        if self.voc is not None:
            self.tail = None
            return self.voc.push(mel, SCALING)
        wav = self.m.vocoder(allmel, 10 ** 12, _scale_div=SCALING, _time_major=True)[:, 0]
        out = wav[:, self.spf * nctx: self.spf * (nctx + k)]
        self.tail = wav[:, self.spf * (nctx + k):]             # partial sums beyond the last frame (models.py:238)
        return out

    @torch.no_grad()
    def finish(self, length=None):
        """End of the utterance (look-ahead window): the samples no push has returned, up to the generator's length, or up to
        ``length`` samples of the whole utterance as ``decode(codes, length)`` cuts it (what the pushes returned stays returned).
        Afterwards the decoder is done."""
        if not self.windowed:
            raise ValueError("StreamingDecoder.finish: a decoder made with lookahead=True has a finish (see flush)")
        rest = self.voc.flush(SCALING)
        return rest if length is None else rest[:, :max(0, int(length) - self.emitted)]

    @torch.no_grad()
    def flush(self, n_extra):
        """Up to 294 samples beyond the last full frame (what decode(codes, length) returns past 256*T)."""
        if self.windowed:
            raise ValueError("StreamingDecoder.flush: a decoder made with lookahead=True ends with finish()")
        if n_extra <= 0 or self.ctx.shape[1] == 0:
            return torch.empty(self.B, 0, device=self.dev)
        if self.tail is None:                                  # incremental mode: the tail comes from the context
            wav = self.m.vocoder(self.ctx, 10 ** 12, _scale_div=SCALING, _time_major=True)[:, 0]
            self.tail = wav[:, self.spf * self.ctx.shape[1]:]
        return self.tail[:, :max(0, n_extra)]
