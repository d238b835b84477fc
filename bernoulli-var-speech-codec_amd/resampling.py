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
        self.lib = _abi.load()
        self.dev = torch.device("cuda" if device is None else device)
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.B, self.rate_in, self.rate_out, self.max_in = batch, int(rate_in), int(rate_out), int(max_in)
        self.fmt_in, self.fmt_out, self.delayed = fmt_in, fmt_out, bool(delayed)
        self.up, self.down, taps, self.lag = preprocess.design(rate_out, rate_in)
        self.max_out = -(-self.max_in * self.up // self.down)
        self.running = set()
        h = self.handle = _abi.Handle(self.lib.bvc_resampler_destroy)
        with torch.cuda.device(self.dev):
            _abi.check_arg(self.lib.bvc_resampler_create(batch, self.rate_in, self.rate_out, self.max_in, PCM_FORMATS[fmt_in],
                                                         PCM_FORMATS[fmt_out] | (PCM_DELAYED if delayed else 0), ctypes.byref(h)))
            if self.up != self.down:        # the offline call's taps are preprocess.design's: hand them in (the library designs the same ones)
                taps = taps.astype("float64")
                _abi.check_arg(self.lib.bvc_resampler_set_taps(h, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(taps)))
        self._counts = (ctypes.c_int32 * batch)()
        self._out = None

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
        x = x.to(self.dev).contiguous()
        n = x.shape[1]
        if self._out is None:
            self._out = torch.empty(self.B, max(1, self.max_out), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            out = _abi.addr(self._out, PCM_DTYPES[self.fmt_out])
            counts = self.push_raw(_abi.addr(x, PCM_DTYPES[self.fmt_in]) if n else out, max(n, 1), n, out, self._out.shape[1], 0,
                                   torch.cuda.current_stream(self.dev).cuda_stream)
        return self._out[:, :-(-n * self.up // self.down)], torch.tensor(counts, dtype=torch.int64)

    @torch.no_grad()
    def flush(self, row):
        """The rest of the row's outputs (at most ``lag`` samples, a new tensor); the row is idle afterwards."""
        y = torch.empty(max(1, self.lag), dtype=PCM_DTYPES[self.fmt_out], device=self.dev)
        with torch.cuda.device(self.dev):
            n = self.flush_raw(row, _abi.addr(y, PCM_DTYPES[self.fmt_out]), torch.cuda.current_stream(self.dev).cuda_stream)
        return y[:n]
