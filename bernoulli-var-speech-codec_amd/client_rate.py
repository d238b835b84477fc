"""The client-rate side of a ``StreamingCodec`` session: the resamplers in front of and behind the session's own buffers."""
import weakref

import torch

from . import _abi
from .resampling import PCM_DTYPES, MultiRateResampler, StreamResampler
from .stream_plans import client_finish_plan


class _ClientRate:
    """What ``StreamingCodec(client_rate=fs, sample_format=...)`` adds to a session (8000 .. 48000 Hz; None or the model's own 22050:
    no adapter), ``sample_format="f32"`` or ``"s16"``: the session speaks the client's rate and format on both sides.  ``hop`` then
    counts client samples and must be a whole number of internal ones (``hop * 22050 % fs == 0``, else ``ValueError``: 480 samples at
    48 kHz would be 220.5; 20 ms hops of the six usual rates pass).  One ``StreamResampler`` sits in front of the session's input
    buffer (send, duplex) and one behind its output buffer (recv, duplex), both on the session's stream, writing into and reading from
    the session's own buffers.  Send side: with ``lag`` = ``self.lag`` (``n_pre_remove`` of ``design(22050, fs)``: 14 samples at
    16 kHz, 11 at 48 kHz) a slot's internal stream is S = zeros(lag) ++ resample_poly(x, 22050, fs) - the offline resampling of the
    client's signal, ``lag`` samples late because the filter looks that far ahead; ``open`` returns the session's delay as before, in
    internal samples, and the stream is ``lag`` later than that.  The slot's packets and codes equal ``model.encode(S[None],
    bitrate)`` on the frames the session emits, bit for bit, and ``finish(slot, n_last)`` (``n_last`` in client samples) ends the slot
    with all ``num_frames(len(S))`` of them.  Receive side: after N internal samples of a stream the client has
    ``resample_poly(wav22[:N], fs, 22050)[:E(N)]`` (``resampler_count``), ``wav22`` what the same session without ``client_rate``
    returns; the last ``lag'`` (11 .. 22) client samples of a stream stay inside - receive sessions have no ``finish``.
    ``push_packets`` then returns ``(wav (batch, n_max) view, counts (batch,) int64 CPU tensor)`` - row b's samples are
    ``wav[b, :counts[b]]`` - and a duplex ``push`` ``(codes, wav, counts)``; a send ``push`` returns what it returned before.
    ``"s16"`` takes and returns int16 tensors (in: x / 32768; out: clamp(rint(y * 32768)) of the float32 result, NaN 0).
    Concealment, repair, ``set_bitrate`` and ``late`` act on the inner session unchanged; ``close`` also idles the row's resamplers.

    The session calls ``opened`` / ``closed`` behind its own open / close, ``finish`` in place of its own, ``feed`` in place of the
    copy into d_in and ``drain`` behind the tick.  Of the session the adapter uses ``_finish``, ``slot_frames`` and ``slot_state``,
    the d_in view, the address of d_wav, the stream, ``spf`` and ``kmax``."""

    def __init__(self, session, conf, rate, fmt, hop, hop_in, open_all):
        self.rate = rate
        self._attach(session, conf, fmt, hop, hop, hop_in)
        if open_all:
            for b in range(self.B):
                self.opened(b)

    def _attach(self, session, conf, fmt, hop, n_in, hop_in):
        """The adapter's book and its resamplers (``_resampler``).  ``hop``: the row a push takes; ``n_in``: what the input side's push
        is told of it - the hop, or ``_MixedClientRate``'s hop per rate; ``lag`` follows ``n_in`` (a number, or one per rate)."""
        sc = self.sc = weakref.proxy(session)                  # (the session owns the adapter: no cycle)
        self.conf, self.fmt, self.hop, self.n_in, self.hop_in = conf, fmt, hop, n_in, hop_in
        self.B, self.dev, self.spf, self.stream, self.d_in, self.wav_ptr = sc.B, sc.dev, sc.spf, sc.stream, sc._in, sc._wav_ptr
        self.n_push = 0                                        # pushes so far
        self.open_push = [0] * self.B                          # the push that took a slot's first client samples
        self.ending = {}                                       # slot -> (internal n_last, spills) of a finish the next push carries out
        self.carry = {}                                        # slot -> (from, count): the part of a flushed tail that goes into the next push
        self.out_wait, self.out_drain = set(), set()           # slots whose samples have yet to start / are about to end on the wav side
        self.rs_in = self.rs_out = None
        if sc.direction != "recv":                             # in front of d_in (delayed: a fixed hop in, a fixed hop out)
            self.rs_in = self._resampler("in", n_in, fmt, "f32", delayed=True)
            self.lag = self.rs_in.lag
            self.tail = torch.zeros(self.B, max(1, self.rs_in.widths()[1]), device=self.dev)
        if sc.direction != "send":                             # behind d_wav
            self.rs_out = self._resampler("out", sc.kmax * self.spf, "f32", fmt)
            self.cwav = torch.zeros(self.B, max(1, self.rs_out.widths()[0]), dtype=PCM_DTYPES[fmt], device=self.dev)

    def _resampler(self, direction, max_in, fmt_in, fmt_out, delayed=False):
        fs = self.conf["fs"]
        rate_in, rate_out = (self.rate, fs) if direction == "in" else (fs, self.rate)
        return StreamResampler(self.B, rate_in, rate_out, max_in, fmt_in, fmt_out, delayed=delayed, device=self.dev)

    def _out_chunk(self, n):
        """n internal samples for every row of the output side: what its push is told, and the width of what comes back."""
        return n, -(-n * self.rs_out.up // self.rs_out.down)

    def slot_rate(self, slot):
        """The client rate, the client hop and the send side's lag of a slot: the session's (``_MixedClientRate``: the slot's own)."""
        return self.rate

    def slot_hop(self, slot):
        return self.hop

    def slot_lag(self, slot):
        return self.lag

    def _open_in(self, slot):
        self.rs_in.open(slot, 0)

    def _open_out(self, slot, offset):
        self.rs_out.open(slot, offset)

    def opened(self, slot):
        if self.rs_in is not None:
            self.rs_in.close(slot)
            self._open_in(slot)
            self.open_push[slot] = self.n_push
            self.ending.pop(slot, None)
            self.carry.pop(slot, None)
        if self.rs_out is not None:
            self.rs_out.close(slot)
            self.out_wait.add(slot)
            self.out_drain.discard(slot)

    def closed(self, slot):
        if self.rs_in is not None:
            self.rs_in.close(slot)
            self.ending.pop(slot, None)
            self.carry.pop(slot, None)
        if self.rs_out is not None:
            self.rs_out.close(slot)
            self.out_wait.discard(slot)
            self.out_drain.discard(slot)

    def finish(self, slot, n_last):
        """``n_last`` counts client samples; the stream's internal signal S = zeros(lag) ++ resample_poly(x, 22050, client_rate) ends
        ``lag`` samples later, so the drain starts with the next push, or the one after it where the flushed tail does not fit the hop
        (``client_finish_plan``); the slot ends with all ``num_frames(len(S))`` frames."""
        if self.rs_in is None:                                 # a receive session: the library's refusal
            return self.sc._finish(slot, n_last)
        slot, n_last = int(slot), int(n_last)
        if not 0 <= slot < self.B or self.sc.slot_state(slot) != "running" or slot in self.ending or slot in self.carry:
            raise ValueError(f"finish: slot {slot} is not a running stream")
        hop = self.slot_hop(slot)
        if not 0 <= n_last <= hop:
            raise ValueError(f"finish: n_last {n_last} outside 0..{hop}")
        push = self.n_push - self.open_push[slot]              # the coming push, counted from the stream's first
        c = self.conf
        len_s, at, n22 = client_finish_plan(push * hop + n_last, hop, self.slot_rate(slot), c["fs"])
        if len_s <= c["winsize"] - c["hopsize"] - c["mel_pad_left"]:
            raise ValueError(f"finish: a stream of {len_s} internal samples is too short for the right reflect padding")
        self.rs_in.end(slot, n_last)
        self.ending[slot] = (n22, at > push)

    def feed(self, x):
        """A hop of client samples -> d_in, inside the session's stream: one resampler push for all rows, and for a row that ends the
        flush of its last ``lag`` samples - straight into d_in where they fit the hop, else through a buffer into this hop and the next.
        (``_MixedClientRate``: row b's first ``slot_hop(b)`` samples are read, every row gets a whole internal hop.)"""
        if tuple(x.shape) != (self.B, self.hop) or x.dtype != PCM_DTYPES[self.fmt]:
            raise ValueError(f"push: expected a {PCM_DTYPES[self.fmt]} tensor ({self.B}, {self.hop})")
        x = x.to(self.dev).contiguous()
        self._end_streams(self.rs_in.push_raw(_abi.addr(x, PCM_DTYPES[self.fmt]), self.hop, self.n_in, _abi.addr(self.d_in), self.hop_in, 0,
                                              self.stream.cuda_stream))
        self.n_push += 1

    def _end_streams(self, counts):
        """Behind the input side's push (``counts``: what it gave every row): the tails of the rows that end."""
        rs, hop22, s = self.rs_in, self.hop_in, self.stream.cuda_stream
        for slot, (frm, n) in list(self.carry.items()):        # the rest of a tail that spilled: the row is idle, its hop zeros
            self.d_in[slot, :n].copy_(self.tail[slot, frm:frm + n], non_blocking=True)
            self.sc._finish(slot, n)
            self.out_drain.add(slot)
            del self.carry[slot]
        for slot, (n22, spills) in list(self.ending.items()):
            e = counts[slot]                                   # what the row's last client samples completed
            if not spills:
                rs.flush_raw(slot, _abi.addr(self.d_in) + 4 * (slot * hop22 + e), s)
                self.sc._finish(slot, n22)
                self.out_drain.add(slot)
            else:
                rs.flush_raw(slot, _abi.addr(self.tail) + 4 * slot * self.tail.shape[1], s)
                self.d_in[slot, e:].copy_(self.tail[slot, :hop22 - e], non_blocking=True)
                self.carry[slot] = (hop22 - e, n22)
            del self.ending[slot]

    def drain(self, k):
        """The tick's k frames of d_wav -> client samples: (wav (B, n_max) view, counts (B,) int64 CPU tensor); None on a send session.
        (``_MixedClientRate``: n_max is the fastest listed rate's.)"""
        rs = self.rs_out
        if rs is None:
            return None
        if k == 0:
            return torch.empty(self.B, 0, dtype=PCM_DTYPES[self.fmt], device=self.dev), torch.zeros(self.B, dtype=torch.int64)
        self._start_and_end_out()
        n = k * self.spf
        n_in, n_out = self._out_chunk(n)
        counts = rs.push_raw(self.wav_ptr, n, n_in, _abi.addr(self.cwav, PCM_DTYPES[self.fmt]), self.cwav.shape[1], 0, self.stream.cuda_stream)
        return self.cwav[:, :n_out], torch.tensor(counts, dtype=torch.int64)

    def _start_and_end_out(self):
        """In front of the output side's push: the rows whose stream starts or ends inside the tick's frames."""
        rs = self.rs_out
        for slot in list(self.out_wait):                       # a row's resampler starts with its stream's frame 0
            first, count, frame0 = self.sc.slot_frames(slot)
            if count > 0 and frame0 == 0:
                self._open_out(slot, self.spf * first)
                self.out_wait.discard(slot)
        for slot in list(self.out_drain):                      # ... and ends with its last one (the last lag' samples stay inside)
            if self.sc.slot_state(slot) == "idle":
                first, count, _ = self.sc.slot_frames(slot)
                if slot in rs.running:
                    rs.end(slot, self.spf * (first + max(0, count)))
                    rs.running.discard(slot)
                self.out_drain.discard(slot)
                self.out_wait.discard(slot)                    # (a stream that ended before its frame 0 came out)


class _MixedClientRate(_ClientRate):
    """What ``StreamingCodec(client_rate=(8000, 16000, 48000))`` adds to a session: ``_ClientRate`` with a client rate PER SLOT, one of
    the 1 .. 8 listed, given to ``open(slot, ..., client_rate=fs)`` and fixed until the slot is opened again (``open_all``: the first
    listed).  One ``MultiRateResampler`` on either side resamples all rows in the one launch per direction the single-rate session
    has.  ``hop`` counts INTERNAL samples - there is no single client rate to count in - and every listed rate must give a whole client
    hop (``hop * rate % 22050 == 0``); slot b's client hop is ``slot_hop(b) = hop * slot_rate(b) / 22050`` and its send-side lag
    ``slot_lag(b)``.  ``push(x)`` takes (batch, the largest client hop) and reads the first ``slot_hop(b)`` samples of row b;
    ``finish(slot, n_last)`` counts the slot's own client samples (``client_finish_plan`` at its rate); on the receive side ``n_max``
    is the fastest listed rate's.  The format is the session's.  The contract: a slot at rate r gives - packets, codes, samples and
    counts, bit for bit - what the same stream gives in a session ``client_rate=r`` of the same format, whatever the other slots
    speak, so ``_ClientRate``'s offline contracts hold per slot.  (A listed 22050 goes through the resampler like any other rate -
    the unit impulse, 11 samples of lag - as ``client_rate=22050, sample_format="s16"`` does.)

    Per slot the adapter keeps the index of the rate, and what ``_ClientRate`` keeps: the tail buffer (as wide as the largest lag) and
    the carry."""

    def __init__(self, session, conf, rates, fmt, hop, open_all):
        self.rates = tuple(rates)
        self.rate_of = [0] * session.B                         # slot -> the index of its rate
        self.hops = [hop * r // conf["fs"] for r in rates]     # the client hop at every rate; the row that push takes is the longest
        self._attach(session, conf, fmt, max(self.hops), self.hops, hop)
        if open_all:
            for b in range(self.B):
                self.opened(b, self.rates[0])

    def _resampler(self, direction, max_in, fmt_in, fmt_out, delayed=False):
        return MultiRateResampler(self.B, self.rates, self.conf["fs"], direction, max_in, fmt_in, fmt_out, delayed=delayed, device=self.dev)

    def _out_chunk(self, n):
        n = [n] * len(self.rates)
        return n, self.rs_out.out_len(n)

    def slot_rate(self, slot):
        return self.rates[self.rate_of[slot]]

    def slot_hop(self, slot):
        return self.hops[self.rate_of[slot]]

    def slot_lag(self, slot):
        return self.lag[self.rate_of[slot]]

    def _open_in(self, slot):
        self.rs_in.open(slot, self.slot_rate(slot), 0)

    def _open_out(self, slot, offset):
        self.rs_out.open(slot, self.slot_rate(slot), offset)

    def opened(self, slot, rate):
        self.rate_of[slot] = self.rates.index(rate)
        super().opened(slot)
