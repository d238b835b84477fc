"""PCM formats and the streaming resampler (``bvc_resampler_*``): what stands between a client's sample rate and the model's."""
import ctypes

import torch

from . import _abi

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
        self.rate_in, self.rate_out, self.max_in = int(rate_in), int(rate_out), int(max_in)
        design = preprocess.design(rate_out, rate_in)
        self.up, self.down, _, self.lag = design
        self.max_out = -(-self.max_in * self.up // self.down)
        self._create(batch, fmt_in, fmt_out, delayed, device, [design], "bvc_resampler_create", (batch, self.rate_in, self.rate_out, self.max_in))

    def _create(self, batch, fmt_in, fmt_out, delayed, device, designs, create, args):
        """What a constructor does once its arguments and geometry stand: the device, the library's object (the call named ``create``:
        ``args``, the two formats, the handle), the taps of ``designs`` - the offline call's, ``preprocess.design``'s - handed in one by
        one (``_set_taps``; the library designs the same ones), the counts."""
        self.lib = _abi.load()
        self.dev = torch.device("cuda" if device is None else device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.B, self.fmt_in, self.fmt_out, self.delayed = batch, fmt_in, fmt_out, bool(delayed)
        self.running = set()
        self.handle = _abi.Handle(self.lib.bvc_resampler_destroy)
        with torch.cuda.device(self.dev):
            _abi.check_arg(getattr(self.lib, create)(*args, PCM_FORMATS[fmt_in], PCM_FORMATS[fmt_out] | (PCM_DELAYED if delayed else 0), ctypes.byref(self.handle)))
            for i, (up, down, taps, _) in enumerate(designs):
                if up != down:
                    taps = taps.astype("float64")
                    _abi.check_arg(self._set_taps(i, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(taps)))
        self._counts = (ctypes.c_int32 * batch)()
        self._out = None

    def _set_taps(self, i, taps, ntaps):
        return self.lib.bvc_resampler_set_taps(self.handle, taps, ntaps)

    def widths(self):
        """(columns of the out buffer, length of a flush's tensor): ``max_out`` and ``lag`` (``MultiRateResampler``: the largest)."""
        return self.max_out, self.lag

    def open(self, row, offset=0):
        _abi.check_arg(self.lib.bvc_resampler_open(self.handle, int(row), int(offset)))
        self.running.add(int(row))

    def close(self, row):
        _abi.check_arg(self.lib.bvc_resampler_close(self.handle, int(row)))
        self.running.discard(int(row))

    def end(self, row, n_valid):
        _abi.check_arg(self.lib.bvc_resampler_end(self.handle, int(row), int(n_valid)))

    def push_raw(self, x_ptr, x_row_stride, n_in, y_ptr, y_row_stride, y_offset, stream):
        """The C call on raw device addresses (strides and offset in elements); returns the rows' counts as a list."""
        _abi.check_arg(self.lib.bvc_resampler_push(self.handle, ctypes.c_void_p(x_ptr), int(x_row_stride), int(n_in), ctypes.c_void_p(y_ptr),
                                                   int(y_row_stride), int(y_offset), self._counts, ctypes.c_void_p(stream)))
        return list(self._counts)

    def flush_raw(self, row, y_ptr, stream):
        n = ctypes.c_int32()
        _abi.check_arg(self.lib.bvc_resampler_flush(self.handle, int(row), ctypes.c_void_p(y_ptr), ctypes.byref(n), ctypes.c_void_p(stream)))
        self.running.discard(int(row))
        return n.value

    @torch.no_grad()
    def push(self, x):
        if x.dim() != 2 or x.shape[0] != self.B or x.shape[1] > self.max_in or x.dtype != PCM_DTYPES[self.fmt_in]:
            raise ValueError(f"StreamResampler.push: expected a {PCM_DTYPES[self.fmt_in]} tensor ({self.B}, n <= {self.max_in})")
        return self._push(x, x.shape[1], -(-x.shape[1] * self.up // self.down))

    def _push(self, x, n_in, n_out):
        """A checked push: ``n_in`` as ``push_raw`` takes it, ``n_out`` the width of the view that is returned."""
        x = x.to(self.dev).contiguous()
        if self._out is None:
            self._out = torch.empty(self.B, max(1, self.widths()[0]), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            out = _abi.addr(self._out, PCM_DTYPES[self.fmt_out])
            counts = self.push_raw(_abi.addr(x, PCM_DTYPES[self.fmt_in]) if x.shape[1] else out, max(x.shape[1], 1), n_in, out,
                                   self._out.shape[1], 0, torch.cuda.current_stream(self.dev).cuda_stream)
        return self._out[:, :n_out], torch.tensor(counts, dtype=torch.int64)

    @torch.no_grad()
    def flush(self, row):
        """The rest of the row's outputs (at most ``lag`` samples - its rate's - in a new tensor); the row is idle afterwards."""
        y = torch.empty(max(1, self.widths()[1]), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            n = self.flush_raw(row, _abi.addr(y, PCM_DTYPES[self.fmt_out]), torch.cuda.current_stream(self.dev).cuda_stream)
        return y[:n]


class MultiRateResampler(StreamResampler):
    """``StreamResampler`` with a rate per row (``bvc_resampler_create_multi``): ``batch`` rows, each converted between one of ``rates``
    (1 .. 8 distinct ones) and ``fixed_rate`` - ``direction="in"``: from its rate to ``fixed_rate``, ``"out"``: from ``fixed_rate`` to
    its rate - all rows in the one launch of a push.  What a row at rate r has got after any chunking is a bit-exact prefix of
    ``preprocess.resample_poly`` of its own signal between r and ``fixed_rate``: what ``StreamResampler`` at that rate gives.

    ``open(row, rate, offset=0)`` starts an idle row at ``rate`` (one of ``rates``, in Hz); the rate is the row's until it is idle again.
    ``close``, ``end`` and ``flush`` are inherited.  ``max_in``: the longest chunk per rate on the input side (a number: the
    same for all).  ``push(x, n)``: ``n`` has one chunk length per rate, in the order of ``rates`` (rows of one rate share the chunk
    length of a push, different rates do not; 0 is allowed); x is (batch, >= max(n)) and row b's first ``n[its rate]`` samples are read.
    Returns ``(y (batch, n_max) view, counts)``, n_max the call's largest ``ceil(n up / down)``; row b's samples are ``y[b, :counts[b]]``,
    zeros behind them up to n_max for every row."""

    def __init__(self, batch, rates, fixed_rate, direction="in", max_in=None, fmt_in="f32", fmt_out="f32", delayed=False, device=None):
        from . import preprocess
        if fmt_in not in PCM_FORMATS or fmt_out not in PCM_FORMATS:
            raise ValueError(f"sample formats are {sorted(PCM_FORMATS)}")
        if direction not in ("in", "out"):
            raise ValueError('MultiRateResampler: direction is "in" or "out"')
        rates = [int(r) for r in rates]
        if not 1 <= len(rates) <= 8 or len(set(rates)) != len(rates) or min(rates) <= 0 or int(fixed_rate) <= 0:
            raise ValueError("MultiRateResampler: 1 to 8 distinct positive rates and a positive fixed_rate")
        n = len(rates)
        self.max_in = [int(max_in)] * n if isinstance(max_in, int) else [int(m) for m in max_in]
        if len(self.max_in) != n:
            raise ValueError("MultiRateResampler: max_in is a number or one number per rate")
        self.rates, self.fixed_rate, self.direction = tuple(rates), int(fixed_rate), direction
        pairs = [(r, self.fixed_rate) if direction == "in" else (self.fixed_rate, r) for r in rates]      # (rate_in, rate_out)
        designs = [preprocess.design(rate_out, rate_in) for rate_in, rate_out in pairs]
        self.up, self.down, self.lag = ([d[i] for d in designs] for i in (0, 1, 3))
        self.max_out = [-(-m * u // d) for m, u, d in zip(self.max_in, self.up, self.down)]
        self.row_rate = [None] * batch                          # the index of a row's rate, from open until it is idle again
        i32s = ctypes.c_int32 * n
        self._n = i32s()
        self._create(batch, fmt_in, fmt_out, delayed, device, designs, "bvc_resampler_create_multi",
                     (batch, n, i32s(*rates), self.fixed_rate, 0 if direction == "in" else 1, i32s(*self.max_in)))

    def _set_taps(self, i, taps, ntaps):
        return self.lib.bvc_resampler_set_taps_rate(self.handle, i, taps, ntaps)

    def widths(self):
        return max(self.max_out), max(self.lag)

    def index(self, rate):
        if rate not in self.rates:
            raise ValueError(f"MultiRateResampler: rate {rate} is not one of {self.rates}")
        return self.rates.index(rate)

    def open(self, row, rate, offset=0):
        i = self.index(rate)
        _abi.check_arg(self.lib.bvc_resampler_open_rate(self.handle, int(row), i, int(offset)))
        self.running.add(int(row))
        self.row_rate[int(row)] = i

    def out_len(self, n):
        """The call's largest block: max over the rates of ceil(n[i] up / down)."""
        return max(-(-int(m) * u // d) for m, u, d in zip(n, self.up, self.down))

    def push_raw(self, x_ptr, x_row_stride, n_in, y_ptr, y_row_stride, y_offset, stream):
        """The C call on raw device addresses (strides and offset in elements, n_in per rate); returns the rows' counts as a list."""
        self._n[:] = [int(m) for m in n_in]
        _abi.check_arg(self.lib.bvc_resampler_push_multi(self.handle, ctypes.c_void_p(x_ptr), int(x_row_stride), self._n, ctypes.c_void_p(y_ptr),
                                                         int(y_row_stride), int(y_offset), self._counts, ctypes.c_void_p(stream)))
        return list(self._counts)

    @torch.no_grad()
    def push(self, x, n):
        n = [int(m) for m in n]
        if (x.dim() != 2 or x.shape[0] != self.B or x.dtype != PCM_DTYPES[self.fmt_in] or len(n) != len(self.rates)
                or x.shape[1] < max(n) or any(not 0 <= m <= lim for m, lim in zip(n, self.max_in))):
            raise ValueError(f"MultiRateResampler.push: expected a {PCM_DTYPES[self.fmt_in]} tensor ({self.B}, >= max(n)) and one chunk "
                             f"length per rate, at most {self.max_in}")
        return self._push(x, n, self.out_len(n))
