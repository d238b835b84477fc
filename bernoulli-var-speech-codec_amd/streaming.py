"""Streaming sessions: ``StreamingCodec``, one library call per hop for a batch of streams that come and go.

The rest of the streaming layer lives beside it, one concern per module, and is importable from here as before: the stateless chunked
classes and the account of the chunked scheme (``stream_chunked``), the host arithmetic (``stream_plans``), the PCM formats and the
streaming resampler (``resampling``), and the client-rate side of a session (``client_rate``).
"""
import ctypes
import math

import torch

from . import _abi
from .client_rate import _ClientRate, _MixedClientRate
from .config import is_causal, not_causal_message
from .model import SCALING
from .resampling import (PCM_DELAYED, PCM_DTYPES, PCM_FORMATS, MultiRateResampler, StreamResampler, pcm_f32_to_s16, pcm_s16_to_f32,  # noqa: F401
                         resampler_count, resampler_lag)
from .stream_chunked import StreamingDecoder, StreamingEncoder, VocoderStream  # noqa: F401
from .stream_plans import (CONTEXT_FRAMES, client_finish_plan, client_hop, finish_plan, generator_reach, join_plan,  # noqa: F401
                           repair_plan)
from .vbr_args import _check_ladder, cap_q8


class _DeviceView:
    """Raw device memory owned by the library, exposed to torch through the CUDA array interface."""

    def __init__(self, ptr, shape, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


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

    ``client_rate=fs``, ``sample_format="f32"`` or ``"s16"``: the session speaks the client's rate and format on both sides, through
    the adapter in ``self._client``; ``client_rate._ClientRate`` holds that contract (what ``hop``, ``finish`` and ``lag`` then mean,
    and the three-value returns).  ``client_rate=(8000, 16000, 48000)`` - a tuple or list of 1 to 8 distinct rates - makes a mixed-rate
    session: every slot speaks one of them, given to ``open(slot, ..., client_rate=fs)`` (``open_all``: the first listed), ``hop``
    counts internal samples, ``push`` takes (batch, the largest client hop) and ``slot_rate`` / ``slot_hop`` / ``slot_lag`` tell a
    slot's values; ``client_rate._MixedClientRate`` holds that contract: a slot gives what it gives in a session of its rate alone.

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
    VBR_KEYS = ("bitrates", "target", "rate_cap", "burst")

    def __init__(self, model, batch, bitrate, hop=441, device=None, open_all=True, direction="duplex", conceal="none", repair=0,
                 client_rate=None, sample_format="f32", vbr=None):
        # ValueError before anything is created
        self.vbr, self.client_rate, self._hop_in = self._check_args(model, hop, direction, conceal, repair, client_rate, sample_format, vbr)
        self.sample_format, self.client_hop, self.direction = sample_format, hop, direction
        self.hop = 0 if direction == "recv" else hop           # the samples per row that push takes
        self.eng = model.engine(None if device is None else torch.empty(0, device=device))
        self.B, self.dev, self._model = batch, self.eng.device, model
        self.z = model.conf["z_dim"]
        self.spf = math.prod(model.conf["vocoder_config"]["upsample_rates"])
        self.stream = torch.cuda.Stream(self.dev)          # a tick may be captured into a hipGraph: not possible on the default stream
        self.handle = self._create(model.bits_per_frame(bitrate))
        self._map_buffers()
        self.frames = 0
        self._client = None
        if isinstance(self.client_rate, tuple):
            self._client = _MixedClientRate(self, model.conf, self.client_rate, sample_format, self._hop_in, open_all)
            self.hop = 0 if direction == "recv" else self._client.hop
        elif self.client_rate is not None:
            self._client = _ClientRate(self, model.conf, self.client_rate, sample_format, hop, self._hop_in, open_all)
        if not open_all:
            for b in range(batch):
                self.close(b)
        self.conceal = "none"
        if conceal != "none":
            self.set_conceal(conceal)
        self.repair = 0
        if repair:
            self.set_repair(repair)

    @classmethod
    def _check_args(cls, model, hop, direction, conceal, repair, client_rate, sample_format, vbr):
        """Every refusal of the constructor's arguments, before anything is created: ``(vbr as _check_vbr gives it, the client's rate
        where the session converts (a tuple of rates for a mixed-rate session) else None, the internal hop)``."""
        vbr = cls._check_vbr(model, direction, repair, vbr)
        if sample_format not in PCM_FORMATS:
            raise ValueError(f"sample_format must be one of {sorted(PCM_FORMATS)}")
        if client_rate is None and sample_format != "f32":
            raise ValueError("sample_format: a session without client_rate speaks float32")
        fs = model.conf["fs"]
        mixed = isinstance(client_rate, (tuple, list))
        if mixed:
            converting, client_rate = True, cls._check_rates(client_rate, hop, fs, direction)
        else:
            if client_rate is not None and (client_rate != int(client_rate) or client_rate <= 0):
                raise ValueError(f"client_rate must be a positive number of Hz, not {client_rate}")
            converting = client_rate is not None and (int(client_rate) != fs or sample_format != "f32")
            if converting and direction != "recv":
                hop = client_hop(hop, int(client_rate), fs)
        if direction not in cls.DIRECTIONS:
            raise ValueError(f"direction must be one of {sorted(cls.DIRECTIONS)}")
        if conceal not in cls.CONCEAL:
            raise ValueError(f"conceal must be one of {sorted(cls.CONCEAL)}")
        if conceal != "none" and direction != "recv":
            raise ValueError("conceal: only a receive session has lost frames to conceal")
        if repair and direction != "recv":
            raise ValueError("repair: only a receive session has late packets to repair from")
        if direction != "send" and not is_causal(model.conf):
            raise ValueError("StreamingCodec: " + not_causal_message(model.conf))
        return vbr, (client_rate if mixed else int(client_rate) if converting else None), (0 if direction == "recv" else hop)

    @staticmethod
    def _check_rates(rates, hop, fs, direction):
        """The rates of a mixed-rate session as a tuple of ints: 1 to 8, positive whole numbers, distinct, and (send and duplex) each with
        a whole client hop for ``hop`` internal samples."""
        if not 1 <= len(rates) <= 8:
            raise ValueError(f"client_rate: a mixed-rate session lists 1 to 8 rates, not {len(rates)}")
        if direction != "recv" and int(hop) <= 0:
            raise ValueError(f"hop {hop} must be positive")
        out = []
        for r in rates:
            if r != int(r) or r <= 0:
                raise ValueError(f"client_rate lists positive numbers of Hz, not {r}")
            if int(r) in out:
                raise ValueError(f"client_rate lists {int(r)} Hz twice")
            if direction != "recv" and hop * int(r) % fs:
                raise ValueError(f"client_rate {int(r)}: a hop of {hop} internal samples is {hop * int(r) / fs:g} samples at {int(r)} Hz: "
                                 "not a whole number")
            out.append(int(r))
        return tuple(out)

    @classmethod
    def _check_vbr(cls, model, direction, repair, vbr):
        """The ``vbr`` keyword as what bvc_stream_codec_create_vbr takes - dict(ladder, target, rate_q8, burst_q8), burst_q8 = -1
        without a cap - or None for a session without it; ValueError for what the library would refuse."""
        if vbr is None or vbr is False:
            return None
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

    def _create(self, bits):
        """The library's session: ``bvc_stream_codec_create_vbr`` for a vbr session, else ``bvc_stream_codec_create_dir``."""
        eng, v, d = self.eng, self.vbr, self.DIRECTIONS[self.direction]
        h = _abi.Handle(eng.lib.bvc_stream_codec_destroy, eng)
        with torch.cuda.device(self.dev):
            if v is not None:
                lad = (ctypes.c_int32 * len(v["ladder"]))(*v["ladder"]) if v["ladder"] else None
                _abi.check(eng.lib.bvc_stream_codec_create_vbr(
                    eng.handle, self.B, self._hop_in, lad, len(v["ladder"]), float(v["target"]), v["rate_q8"], v["burst_q8"],
                    float(bits), float(SCALING), float(SCALING), d, ctypes.byref(h)))
            else:
                _abi.check(eng.lib.bvc_stream_codec_create_dir(eng.handle, self.B, self._hop_in, float(bits), float(SCALING),
                                                               float(SCALING), d, ctypes.byref(h)))
        return h

    def _map_buffers(self):
        """Views and addresses of the session's own device buffers."""
        lib, h, B = self.eng.lib, self.handle, self.B
        pin, pc, pw, kmax = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        _abi.check(lib.bvc_stream_codec_buffers(h, ctypes.byref(pin), ctypes.byref(pc), ctypes.byref(pw), ctypes.byref(kmax)))
        self.kmax = kmax.value
        self._in = self._view(pin.value, (B, self._hop_in)) if pin.value else None
        self._codes_ptr, self._wav_ptr = pc.value, pw.value
        pp, pr, bpf = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        _abi.check(lib.bvc_stream_codec_packets(h, ctypes.byref(pp), ctypes.byref(pr), ctypes.byref(bpf)))
        self.bytes_per_frame = bpf.value
        self._packets = self._present = None
        if pp.value:                                           # (batch, kmax, bytes_per_frame) / (batch, kmax) whatever a tick's frame count
            self._packets = self._view(pp.value, (B, self.kmax, bpf.value), "|u1")
            self._present = self._view(pr.value, (B, self.kmax), "|u1")
        self._sizes_ptr = self._bits_ptr = None
        self._last_k = 0
        if self.vbr is not None:
            ps, pb = ctypes.c_void_p(), ctypes.c_void_p()
            _abi.check(lib.bvc_stream_codec_sizes(h, ctypes.byref(ps)))
            _abi.check(lib.bvc_stream_codec_bits(h, ctypes.byref(pb)))
            self._sizes_ptr, self._bits_ptr = ps.value, pb.value

    def _view(self, ptr, shape, typestr="<f4"):
        return torch.as_tensor(_DeviceView(ptr, shape, typestr), device=self.dev)

    @property
    def lag(self):
        """Rate-converting send and duplex sessions: the internal samples a stream is late by (``client_rate._ClientRate``)."""
        if isinstance(self._client, _MixedClientRate):
            raise ValueError("lag: a mixed-rate session has a lag per slot (slot_lag(slot))")
        return self._client.lag

    def slot_rate(self, slot):
        """Rate-converting sessions: the client rate of a slot - on a mixed-rate session the one it was last opened with."""
        return self._slot_value("slot_rate", slot)

    def slot_hop(self, slot):
        """Rate-converting send and duplex sessions: the client samples of a slot that a push takes."""
        return self._slot_value("slot_hop", slot)

    def slot_lag(self, slot):
        """Rate-converting send and duplex sessions: the internal samples the slot's stream is late by."""
        return self._slot_value("slot_lag", slot)

    def _slot_value(self, what, slot):
        if self._client is None or (what != "slot_rate" and self.direction == "recv"):
            raise ValueError(f"{what}: not a rate-converting {'send or duplex ' if what != 'slot_rate' else ''}session")
        if not 0 <= int(slot) < self.B:
            raise ValueError(f"{what}: slot {slot} outside 0..{self.B - 1}")
        return getattr(self._client, what)(int(slot))

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
        return self._view(ptr, (self.B, self.kmax), typestr)[:, :self._last_k]

    def set_target(self, slot, target):
        """vbr send / duplex sessions: the distortion target of an open slot from the next push on."""
        _abi.check_arg(self.eng.lib.bvc_stream_codec_set_target(self.handle, int(slot), float(target)))

    def open(self, slot, bitrate=None, target=None, client_rate=None):
        """Start a new stream in idle row `slot` from the next push on; returns its delay in (internal) samples.  A rate-converting
        send side delays the stream by ``lag`` more: its filter looks that far ahead (``self.lag`` internal samples).  A vbr send or
        duplex session takes ``target`` (None: the session's) instead of ``bitrate``.  A mixed-rate session takes the slot's
        ``client_rate``, one of the session's; no other session does."""
        mixed = isinstance(self._client, _MixedClientRate)
        if mixed and client_rate not in self.client_rate:
            raise ValueError(f"open: client_rate must be one of the session's rates {self.client_rate}, not {client_rate}")
        if not mixed and client_rate is not None:
            raise ValueError("open: client_rate belongs to a mixed-rate session (StreamingCodec(client_rate=(...)))")
        choosing = self.vbr is not None and self.direction != "recv"
        if choosing and bitrate is not None:
            raise ValueError("open: a vbr session chooses its own rates (open(slot, target=...))")
        if not choosing and (bitrate is None or target is not None):
            raise ValueError("open: open(slot, bitrate)" if bitrate is None else "open: target belongs to a vbr send or duplex session")
        d = ctypes.c_int32()
        _abi.check_arg(self.eng.lib.bvc_stream_codec_open(self.handle, int(slot), 0.0 if choosing else float(self._model.bits_per_frame(bitrate)),
                                                          ctypes.byref(d)))
        if choosing and target is not None:
            self.set_target(slot, target)
        if mixed:
            self._client.opened(int(slot), int(client_rate))
        elif self._client is not None:
            self._client.opened(int(slot))
        return d.value

    def close(self, slot):
        """The row is idle from the next push on (ask ``slot_frames`` first)."""
        _abi.check_arg(self.eng.lib.bvc_stream_codec_close(self.handle, int(slot)))
        if self._client is not None:
            self._client.closed(int(slot))

    def set_bitrate(self, slot, bitrate):
        """Bits per frame of an open slot from the next push on (variable-bitrate models only)."""
        _abi.check_arg(self.eng.lib.bvc_stream_codec_set_bits(self.handle, int(slot), float(self._model.bits_per_frame(bitrate))))

    def slot_frames(self, slot):
        """(first, count, stream_frame0): frames [first, first + count) of the last push are the slot's stream's frames
        stream_frame0, stream_frame0 + 1, ...; count is 0 for an idle slot and before the stream's frame 0."""
        f, n, s0 = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        _abi.check_arg(self.eng.lib.bvc_stream_codec_slot_frames(self.handle, int(slot), ctypes.byref(f), ctypes.byref(n),
                                                                 ctypes.byref(s0)))
        return f.value, n.value, s0.value

    def finish(self, slot, n_last=None):
        """The stream in `slot` ends with the first `n_last` samples of the next push's row (None: the whole hop; 0: it ended with
        the last push).  The slot drains from that push on and is idle once its last frame is out.  On a rate-converting session `n_last`
        counts client samples, and the drain starts ``lag`` internal samples later (``client_rate._ClientRate.finish``)."""
        if n_last is None:
            n_last = self.slot_hop(slot) if isinstance(self._client, _MixedClientRate) and self.direction != "recv" else self.hop
        if self._client is not None:
            return self._client.finish(slot, n_last)
        self._finish(slot, n_last)

    def _finish(self, slot, n_last):
        _abi.check_arg(self.eng.lib.bvc_stream_codec_finish(self.handle, int(slot), int(n_last)))

    def set_conceal(self, mode):
        """What the next pushes do with a lost frame: "none" (a frame of no bits) or "prior" (generated from the prior net).
        Receive sessions only."""
        if mode not in self.CONCEAL:
            raise ValueError(f"conceal must be one of {sorted(self.CONCEAL)}")
        _abi.check_arg(self.eng.lib.bvc_stream_codec_set_conceal(self.handle, self.CONCEAL[mode]))
        self.conceal = mode

    def set_repair(self, window):
        """The repair window in frames (0 .. 64, 0: off) from the next push on; empties the window.  Receive sessions only."""
        with torch.cuda.device(self.dev):
            _abi.check_arg(self.eng.lib.bvc_stream_codec_set_repair(self.handle, int(window)))
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
            _abi.check_arg(self.eng.lib.bvc_stream_codec_late(self.handle, int(slot), int(stream_frame), ctypes.cast(buf, ctypes.c_void_p),
                                                              ctypes.byref(taken)))
        return bool(taken.value)

    def filled_codes(self, k):
        """Receive session: the codes (batch, k, z_dim) the last push of k frames decoded - unpacked, and with ``conceal="prior"`` with
        the lost frames filled; a view of the session's buffer, valid until the next push."""
        return self._view(self._codes_ptr, (self.B, k, self.z))

    def slot_state(self, slot):
        """"idle", "waiting" (open, frame 0 still to come), "running" or "draining" (finished, frames still to come)."""
        v = ctypes.c_int32()
        _abi.check_arg(self.eng.lib.bvc_stream_codec_slot_state(self.handle, int(slot), ctypes.byref(v)))
        return ("idle", "waiting", "running", "draining")[v.value]

    @torch.no_grad()
    def push_packets(self, packets, present=None):
        """Receive session: packets (batch, k, bytes_per_frame) uint8 (fewer bytes per frame are taken as the leading ones),
        present (batch, k) (None: everything arrived) -> wav (batch, 256 k), a view of the session's buffer, valid until the next push."""
        if packets.dim() != 3 or packets.shape[0] != self.B or packets.shape[2] > self.bytes_per_frame or packets.dtype != torch.uint8:
            raise ValueError(f"push_packets: expected uint8 packets ({self.B}, k, <= {self.bytes_per_frame})")
        k = packets.shape[1]
        if self.direction != "recv" or not 1 <= k <= self.kmax:    # the library's refusal (BVC_EINVAL), session untouched
            _abi.check_arg(self.eng.lib.bvc_stream_codec_tick_recv(self.handle, k, ctypes.c_void_p(self.stream.cuda_stream)))
            raise ValueError("push_packets: refused")
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        out = None
        with torch.cuda.stream(self.stream), torch.cuda.device(self.dev):
            self._packets[:, :k, :packets.shape[2]].copy_(packets.to(self.dev), non_blocking=True)
            if present is None:
                self._present[:, :k].fill_(1)
            else:
                self._present[:, :k].copy_(present.to(self.dev).ne(0).to(torch.uint8).reshape(self.B, k), non_blocking=True)
            _abi.check_arg(self.eng.lib.bvc_stream_codec_tick_recv(self.handle, k, ctypes.c_void_p(self.stream.cuda_stream)))
            if self._client is not None:
                out = self._client.drain(k)
        cur.wait_stream(self.stream)
        self.frames += k
        self._last_k = k
        return self._view(self._wav_ptr, (self.B, k * self.spf)) if out is None else out

    @torch.no_grad()
    def push(self, x):
        if self.direction == "recv":                           # the library's refusal (BVC_EINVAL), session untouched
            _abi.check_arg(self.eng.lib.bvc_stream_codec_tick(self.handle, None, ctypes.c_void_p(self.stream.cuda_stream)))
            raise ValueError("push: a receive session takes packets (push_packets)")
        assert tuple(x.shape) == (self.B, self.hop)
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        k = ctypes.c_int32()
        client, out = self._client, None
        with torch.cuda.stream(self.stream), torch.cuda.device(self.dev):
            if client is not None:
                client.feed(x)
            else:
                self._in.copy_(x.to(self.dev, torch.float32), non_blocking=True)
            _abi.check(self.eng.lib.bvc_stream_codec_tick(self.handle, ctypes.byref(k), ctypes.c_void_p(self.stream.cuda_stream)))
            if client is not None:
                out = client.drain(k.value)
        cur.wait_stream(self.stream)
        k = k.value
        self.frames += k
        self._last_k = k
        return self._pushed(k, out)

    def _pushed(self, k, client_out):
        """What ``push`` returns for a tick of k frames: (packets, codes) on a send session, else (codes, wav) - views of the library's
        buffers, empty tensors where k is 0 - or (codes, wav, counts) with the client-rate adapter's samples."""
        codes = self._view(self._codes_ptr, (self.B, k, self.z)) if k else torch.empty(self.B, 0, self.z, device=self.dev)
        if self.direction == "send":
            return self._packets[:, :k], codes
        if client_out is not None:
            return (codes,) + client_out
        return codes, (self._view(self._wav_ptr, (self.B, k * self.spf)) if k else torch.empty(self.B, 0, device=self.dev))
