"""Drop-in facade: ``BVRNNCodecModel(config_path, bvrnn_chkpt_path, vocoder_chkpt_path)`` with
``encode(x, bitrate)``, ``decode(codes, length)``, ``forward(x, bitrate)`` - same names, argument
meaning and error behaviour as the reference class (bvrnn_codec_model.py:19-76) - plus the two
sub-operators the reference exposes as attributes (``model.bvrnn.encode/decode`` bvrnn.py:163-229,
``model.vocoder(x, length)`` models.py:207-238) and ``mel_spectrogram`` (meldataset.py:60-95).

All arithmetic runs in the gfx950 HIP library behind include/bvcodec.h; PyTorch only provides device
memory and streams.  Inference only: outputs carry no autograd graph.  Tensors that live on another
device (e.g. the CPU tensors of the reference's example.py) are moved to the model's GPU for the
call and the result is returned on the caller's device.
"""
import ctypes
import os

import numpy as np
import torch
from torch import nn

from . import _abi, ragged, weights
from .config import DEFAULT_CONFIG, is_causal, load_config, not_causal_message

_ROOT = os.path.abspath(os.path.dirname(__file__))
default_config = DEFAULT_CONFIG
# The reference resolves its default checkpoints next to its module file (bvrnn_codec_model.py:11-15: ./chkpts/...).
# Same file names here, looked up in $BVC_CHKPT_DIR if set, else in ./chkpts next to the drop-in shim
# (bvrnn_codec_model.py at the repository root).  The files themselves are Git-LFS objects of the reference and are
# not shipped: the constructor names the path it looked at when one is missing.
_CHKPT_DIR = os.environ.get("BVC_CHKPT_DIR") or os.path.join(os.path.dirname(_ROOT), "chkpts")
default_chkpt_bvrnn = os.path.join(_CHKPT_DIR, "bvrnn_var_bitrate_step200000")
default_chkpt_vocoder = os.path.join(_CHKPT_DIR, "bigvgan_causal_tiny_ftbvrnn_g_step3500000")

SCALING = 10 ** (-10 / 20)      # bvrnn_codec_model.py:17


def _as_device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("bvcodec needs an AMD GPU (gfx950): torch.cuda.is_available() is False and "
                               "there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"bvcodec runs on the GPU only (got device '{device}')")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Engine:
    """One device-resident copy of the weights (a bvc_model handle) + its workspace."""

    def __init__(self, conf, tensors, device):
        self.lib = _abi.load()
        self.device = device
        self.conf = conf
        v = conf["vocoder_config"]
        cfg = _abi.BvcConfig()
        cfg.num_mels, cfg.h_dim, cfg.z_dim = conf["num_mels"], conf["h_dim"], conf["z_dim"]
        cfg.var_bit = 1 if conf["var_bit"] else 0
        cfg.n_fft, cfg.hop, cfg.pad_left = conf["winsize"], conf["hopsize"], conf["mel_pad_left"]
        cfg.sample_rate, cfg.fmin, cfg.fmax = conf["fs"], float(conf["fmin"]), float(conf["fmax"])
        cfg.upsample_initial_channel = v["upsample_initial_channel"]
        cfg.n_up = len(v["upsample_rates"])
        for i, (u, k) in enumerate(zip(v["upsample_rates"], v["upsample_kernel_sizes"])):
            cfg.up_rates[i], cfg.up_kernels[i] = u, k
        cfg.n_resk = len(v["resblock_kernel_sizes"])
        for j, (k, ds) in enumerate(zip(v["resblock_kernel_sizes"], v["resblock_dilation_sizes"])):
            cfg.res_kernels[j] = k
            for d in range(3):
                cfg.res_dilations[j][d] = ds[d]
        names = list(tensors)
        arr = (_abi.BvcTensor * len(names))()
        for i, n in enumerate(names):
            t = tensors[n]
            arr[i].name, arr[i].h_data, arr[i].numel = n.encode(), t.data_ptr(), t.numel()
        handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _abi.check(self.lib.bvc_model_create(ctypes.byref(cfg), arr, len(names), ctypes.byref(handle)))
        self.handle = handle
        self._ws = {}            # one workspace per stream: calls on different streams may overlap

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.bvc_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def workspace(self, B, T):
        """Scratch for one call, owned by the CURRENT stream (the C ABI allows one in-flight call per
        (model, workspace); independent batches issued on different streams therefore overlap)."""
        need = self.lib.bvc_workspace_bytes(self.handle, B, T)
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws[key] = None
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ctypes.c_void_p(ws.data_ptr()), ws.numel()

    def vbr_workspace(self, B, T, K):
        """Scratch of a closed-loop call (bvc_vbr_workspace_bytes): the current stream's buffer, grown if need be."""
        need = self.lib.bvc_vbr_workspace_bytes(self.handle, B, T, K)
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws[key] = None
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ctypes.c_void_p(ws.data_ptr()), ws.numel()

    def stream(self):
        return _abi.current_stream(self.device)

    def set_option(self, name, value):
        _abi.check(self.lib.bvc_model_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name):
        v = ctypes.c_int32(0)
        _abi.check(self.lib.bvc_model_get_option(self.handle, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def check_status(self):
        """Synchronises the device and raises if a persistent recurrence kernel of this model ever gave up waiting
        (its results were then invalid); see bvc_model_status in include/bvcodec.h.  (Every compute call also looks at
        the status word, without synchronising, and raises on the first call after a time-out.)"""
        code = ctypes.c_uint32(0)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.bvc_model_status(self.handle, ctypes.byref(code)))

    def poll_status(self):
        """The same check without synchronising (bvc_model_poll_status): for right after a blocking copy of an output."""
        _abi.check(self.lib.bvc_model_poll_status(self.handle, None))

    def deliver(self, out, out_dev):
        """An output tensor on the caller's device.  A copy to the CPU blocks until the call has finished: the recurrence's status word is
        then final for THIS call, and a time-out is raised here rather than by the next call."""
        res = out.to(out_dev)
        if torch.device(out_dev).type == "cpu":
            self.poll_status()
        return res

    def num_frames(self, L):
        return int(self.lib.bvc_num_frames(self.handle, L))

    def vocoder_length(self, T):
        return int(self.lib.bvc_vocoder_length(self.handle, T))


def _trimmed(total, length):
    """Samples that ``x[:, :, :length]`` keeps of ``total`` (models.py:238): Python slice semantics, so 0 keeps nothing and a
    negative length cuts from the end."""
    return len(range(int(total))[:int(length)])


def _prep(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


_MAX_RUNGS = 8                   # VBR_MAX_RUNGS of the library


def _check_ladder(ladder, z_dim, var_bit):
    """The ladder of a closed-loop call as a ctypes int32 array, or ValueError: 1 to 8 integer bit counts in [0, z_dim], strictly
    ascending, on a variable-rate model."""
    if not var_bit:
        raise ValueError("encode_vbr: a fixed-rate model (var_bit = false) has no bit mask to choose")
    rungs = [int(n) for n in ladder]
    if any(float(a) != float(b) for a, b in zip(rungs, ladder)):
        raise ValueError(f"encode_vbr: the rungs must be integer bit counts, got {list(ladder)}")
    if not 1 <= len(rungs) <= _MAX_RUNGS:
        raise ValueError(f"encode_vbr: the ladder takes 1 to {_MAX_RUNGS} rungs, got {len(rungs)}: {rungs}")
    if any(n < 0 or n > z_dim for n in rungs) or any(b <= a for a, b in zip(rungs, rungs[1:])):
        raise ValueError(f"encode_vbr: the rungs must lie in [0, {z_dim}] and ascend strictly, got {rungs}")
    return (ctypes.c_int32 * len(rungs))(*rungs), len(rungs)


_Q8 = 256                        # the token bucket of a capped closed-loop call counts 1/256 bit
_I32_MAX = 2 ** 31 - 1


def _check_cap_q8(rungs, rate_q8, burst_q8):
    """The bucket of a capped closed-loop call as two ints, or ValueError (what the library refuses with BVC_EINVAL): neither negative,
    both int32, and a full bucket holds rung 0."""
    if rate_q8 is None or burst_q8 is None:
        raise ValueError("encode_vbr: a rate cap takes both rate_q8 and burst_q8")
    if int(rate_q8) != rate_q8 or int(burst_q8) != burst_q8:
        raise ValueError(f"encode_vbr: rate_q8 and burst_q8 are integers (1/256 bit), got {rate_q8!r}, {burst_q8!r}")
    rate_q8, burst_q8 = int(rate_q8), int(burst_q8)
    if rate_q8 < 0 or burst_q8 < 0 or rate_q8 > _I32_MAX or burst_q8 > _I32_MAX:
        raise ValueError(f"encode_vbr: rate_q8 = {rate_q8} and burst_q8 = {burst_q8} must lie in [0, 2^31)")
    if burst_q8 < int(rungs[0]) * _Q8:
        raise ValueError(f"encode_vbr: a bucket of {burst_q8 / _Q8:g} bits never holds rung 0 ({int(rungs[0])} bits)")
    return rate_q8, burst_q8


def cap_q8(conf, rungs, rate_cap, burst):
    """``rate_cap`` [bit/s] and ``burst`` [bits] of a capped closed-loop call as (rate_q8, burst_q8), None without a cap; ValueError as
    ``_check_cap_q8``.  rate_q8 = round(rate_cap * hopsize / fs * 256), burst_q8 = round(burst * 256), the default burst four times the
    top rung."""
    if rate_cap is None:
        if burst is not None:
            raise ValueError("encode_vbr: burst without rate_cap")
        return None
    if not (rate_cap >= 0) or (burst is not None and not (burst >= 0)) or rate_cap == float("inf") or burst == float("inf"):
        raise ValueError(f"encode_vbr: rate_cap = {rate_cap} and burst = {burst} must be finite and not negative")
    if burst is None:
        burst = 4 * int(rungs[-1])
    return _check_cap_q8(rungs, round(rate_cap * conf["hopsize"] / conf["fs"] * _Q8), round(burst * _Q8))


def _broadcast_target(target, B, T, device):
    """A scalar, (B,) or (B,T) distortion target as a contiguous float32 (B,T) tensor on ``device``."""
    t = torch.as_tensor(target, dtype=torch.float32).detach()
    if t.dim() == 0:
        t = t.reshape(1, 1)
    elif tuple(t.shape) == (B,) and t.dim() == 1:
        t = t.reshape(B, 1)
    elif tuple(t.shape) != (B, T):
        raise ValueError(f"encode_vbr: target must be a scalar, ({B},) or ({B}, {T}), got {tuple(t.shape)}")
    return t.to(device).expand(B, T).contiguous()


class _OnDevice(nn.Module):
    """Shared plumbing: lazily creates the engine on the module's device."""

    def __init__(self, conf, tensors):
        super().__init__()
        self.conf = conf
        self._tensors = tensors
        self._engines = {}
        self._device = None

    def _apply(self, fn, *a, **k):              # follow .to('cuda:N') / .cuda(); there is no CPU residence
        # probe where a tensor that lives where this module lives would end up: a dtype-only conversion (.float(), .half(),
        # .to(torch.float32)) leaves the device alone and must not forget the residence
        here = torch.empty(0, device=self._device) if self._device is not None else torch.empty(0)
        probe = fn(here)
        if probe.device.type == "cuda":
            self._device = _as_device(probe.device)
        elif probe.device.type == "cpu" and here.device.type != "cpu":    # .cpu() / .to('cpu'): the next call follows its input again
            self._device = None
        return super()._apply(fn, *a, **k)

    _SCHEDULES = {"persistent": 0, "layers": 1, "auto": 2}

    def set_recurrence(self, schedule):
        """'auto' (default): every frame of a call in one persistent kernel launch while calls come one at a time, one launch
        per layer (hipGraph replay) while calls issued on several streams overlap - the library watches whether the previous
        call, issued on another stream, is still running when a new one starts;
        'persistent' / 'layers': that schedule for every call.  Applies to the engines created so far and to later ones.
        Not while a call is in flight."""
        if schedule not in self._SCHEDULES:
            raise ValueError("schedule must be 'auto', 'persistent' or 'layers'")
        self._recurrence = schedule
        for eng in list(self._engines.values()):
            eng.set_option("recurrence", self._SCHEDULES[schedule])

    def check_status(self):
        """Device-synchronising health check of the engines this module has created (bvc_model_status)."""
        for eng in list(self._engines.values()):
            eng.check_status()

    def engine(self, like=None):
        dev = self._device
        if dev is None and like is not None and like.device.type == "cuda":
            dev = like.device
        dev = _as_device(dev)
        if dev not in self._engines:
            self._engines[dev] = _Engine(self.conf, self._tensors, dev)
            if getattr(self, "_recurrence", None) is not None:
                self._engines[dev].set_option("recurrence", self._SCHEDULES[self._recurrence])
        return self._engines[dev]


class BVRNN(_OnDevice):
    """``BVRNN.encode`` / ``BVRNN.decode`` (bvrnn.py:163-229) on the HIP recurrent kernels."""

    def __init__(self, conf, tensors, shared=None):
        super().__init__(conf, tensors)
        self.h_dim, self.z_dim, self.x_dim = conf["h_dim"], conf["z_dim"], conf["num_mels"]
        self.varBit = bool(conf["var_bit"])
        if shared is not None:
            self._engines = shared

    @torch.no_grad()
    def forward(self, y, p_use_gen, greedy, varBitrate, *, r=None, noise=None, return_all=False):
        """``BVRNN.forward(y, p_use_gen, greedy, varBitrate)`` (bvrnn.py:86-160), forward values only (this build
        has no autograd): stochastic Bernoulli sampler ``round(u - 0.5 + enc_t)``, prior net, KL term and the
        teacher-forcing mix.  Returns (all_dec_mean (B,T,x_dim), kld scalar) like the reference.

        Randomness: the reference draws, per frame, ``torch.rand([])`` (compared with p_use_gen) and - unless
        greedy - ``torch.rand_like(enc_t)``.  By default the same numbers are drawn here, in the same order, from
        torch's global CPU generator, so ``torch.manual_seed(s)`` followed by this call reproduces the reference
        run on CPU after the same seed.  ``r`` (T,) / ``noise`` (B,T,z_dim) override them.
        ``return_all=True`` adds a dict with z (forward value of the sample), prob (enc_t), prior, kld_frames."""
        eng = self.engine(y)
        out_dev = y.device
        y = _prep(y, eng.device)
        B, T, _ = y.shape
        if r is None or (noise is None and not greedy):
            rs, ns = [], []
            for _ in range(T):                                    # the reference's draw order (bvrnn.py:111,126)
                rs.append(torch.rand([]))
                if not greedy:
                    ns.append(torch.rand(B, self.z_dim))
            r = torch.stack(rs) if r is None else r
            if not greedy and noise is None:
                noise = torch.stack(ns, 1)
        use_gen = (torch.as_tensor(r).detach().cpu().float() < p_use_gen).to(torch.uint8).contiguous()
        assert use_gen.numel() == T
        bits = _prep(varBitrate, eng.device) if (varBitrate is not None and self.varBit) else None
        un = None if greedy else _prep(noise, eng.device)
        dec = torch.empty(B, T, self.x_dim, device=eng.device)
        kld = torch.empty(T, device=eng.device)
        extra = {k: torch.empty(B, T, self.z_dim, device=eng.device) for k in ("z", "prob", "prior")} if return_all else {}
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_bvrnn_forward(
                eng.handle, _abi.ptr(y), _abi.ptr(bits), ctypes.c_void_p(use_gen.data_ptr()), int(p_use_gen < 1),
                int(p_use_gen > 0), _abi.ptr(un), B, T, _abi.ptr(dec), _abi.ptr(kld), _abi.ptr(extra.get("z")),
                _abi.ptr(extra.get("prob")), _abi.ptr(extra.get("prior")), ws, nws, eng.stream()))
        out = (dec.to(out_dev), torch.mean(kld).to(out_dev))     # torch.mean(torch.stack(kld_loss)), bvrnn.py:160
        if return_all:
            extra["kld_frames"] = kld
            return out + ({k: v.to(out_dev) for k, v in extra.items()},)
        return out

    @torch.no_grad()
    def encode(self, y, varBitrate, h, return_prob=False):
        """y (B,T,x_dim), varBitrate (B,T) bits/frame, h (1,B,h_dim) -> (codes (B,T,z), all_h (B,T,h))."""
        eng = self.engine(y)
        out_dev = y.device
        y = _prep(y, eng.device)
        B, T, _ = y.shape
        bits = _prep(varBitrate, eng.device) if varBitrate is not None else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        all_h = torch.empty(B, T, self.h_dim, device=eng.device)
        prob = torch.empty(B, T, self.z_dim, device=eng.device) if return_prob else None
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_bvrnn_encode(eng.handle, _abi.ptr(y), _abi.ptr(bits), _abi.ptr(h0), B, T,
                                                _abi.ptr(codes), _abi.ptr(all_h), None, _abi.ptr(prob), ws, nws,
                                                eng.stream()))
        if return_prob:
            return codes.to(out_dev), all_h.to(out_dev), eng.deliver(prob, out_dev)
        return codes.to(out_dev), eng.deliver(all_h, out_dev)

    @torch.no_grad()
    def encode_vbr(self, y, ladder, target, h, return_all=False, rate_q8=None, burst_q8=None, tok=None):
        """``encode`` with the bits of every frame chosen inside the frame (``bvc_bvrnn_encode_vbr``): y (B,T,x_dim), ``ladder`` up to 8
        ascending bit counts, ``target`` a scalar, (B,) or (B,T) bound on the mean absolute log-mel error of the frame as the receiver
        will decode it, h (1,B,h_dim).  A frame gets the first rung of the ladder that meets its target, the last one if none does.
        Returns (codes (B,T,z), bits (B,T), all_h (B,T,h)); ``return_all=True`` adds a dict with prob (B,T,z), dist (B,T,K) - the error
        of every rung -, dec (B,T,x_dim) - the chosen rung's decoded mel - and h_next (1,B,h_dim).

        ``rate_q8`` and ``burst_q8`` (ints, 1/256 bit; both or neither) put a token bucket per row under the choice
        (``bvc_bvrnn_encode_vbr_capped``): per frame tok = min(burst_q8, tok + rate_q8), the frame gets the lower of its rung and the
        highest rung with ladder[k] * 256 <= tok (rung 0 if none), tok = max(0, tok - 256 bits).  ``tok`` (B,) int32: the buckets in
        front of the first frame (None: full); the dict then carries ``tok_next`` (B,) int32, which the next chunk takes as ``tok``."""
        lad, K = _check_ladder(ladder, self.z_dim, self.varBit)
        capped = rate_q8 is not None or burst_q8 is not None
        if capped:
            rate_q8, burst_q8 = _check_cap_q8(list(lad), rate_q8, burst_q8)
        elif tok is not None:
            raise ValueError("encode_vbr: tok without rate_q8 and burst_q8")
        if y.dim() != 3:
            raise ValueError("encode_vbr: y must be (B, T, num_mels)")
        B, T, _ = y.shape
        tau = _broadcast_target(target, B, T, "cpu")
        eng = self.engine(y)
        out_dev = y.device
        y = _prep(y, eng.device)
        tau = tau.to(eng.device)
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        all_h = torch.empty(B, T, self.h_dim, device=eng.device)
        extra = {}
        if return_all:
            extra = {"prob": torch.empty(B, T, self.z_dim, device=eng.device), "dist": torch.empty(B, T, K, device=eng.device),
                     "dec": torch.empty(B, T, self.x_dim, device=eng.device), "h_next": torch.empty(B, self.h_dim, device=eng.device)}
        ws, nws = eng.vbr_workspace(B, T, K)
        args = (eng.handle, _abi.ptr(y), _abi.ptr(tau), lad, K, _abi.ptr(h0), B, T, _abi.ptr(codes), _abi.ptr(bits), _abi.ptr(all_h),
                _abi.ptr(extra.get("h_next")), _abi.ptr(extra.get("prob")), _abi.ptr(extra.get("dist")), _abi.ptr(extra.get("dec")),
                ws, nws, eng.stream())
        tok_next = None
        with torch.cuda.device(eng.device):
            if capped:
                tok0 = None
                if tok is not None:
                    tok0 = torch.as_tensor(tok).detach().to(device=eng.device, dtype=torch.int32).contiguous()
                    if tuple(tok0.shape) != (B,):
                        raise ValueError(f"encode_vbr: tok must be ({B},), got {tuple(tok0.shape)}")
                tok_next = torch.empty(B, dtype=torch.int32, device=eng.device)
                _abi.check(eng.lib.bvc_bvrnn_encode_vbr_capped(
                    *args, rate_q8, burst_q8, ctypes.c_void_p(tok0.data_ptr()) if tok0 is not None else None,
                    ctypes.c_void_p(tok_next.data_ptr())))
            else:
                _abi.check(eng.lib.bvc_bvrnn_encode_vbr(*args))
        out = (codes.to(out_dev), bits.to(out_dev), eng.deliver(all_h, out_dev))
        if return_all:
            if capped:
                extra["tok_next"] = tok_next
            extra["h_next"] = extra["h_next"].unsqueeze(0)
            return out + ({k: v.to(out_dev) for k, v in extra.items()},)
        return out

    @torch.no_grad()
    def encode_stateful(self, y, varBitrate, h):
        """Like encode() but returns the state AFTER the last frame instead of the per-frame states:
        (codes (B,T,z), h_next (1,B,h_dim)).  This is what chunked / streaming encoding needs (the
        reference's encode() only exposes the state before each frame, bvrnn.py:205,209)."""
        eng = self.engine(y)
        out_dev = y.device
        y = _prep(y, eng.device)
        B, T, _ = y.shape
        bits = _prep(varBitrate, eng.device) if varBitrate is not None else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_bvrnn_encode(eng.handle, _abi.ptr(y), _abi.ptr(bits), _abi.ptr(h0), B, T,
                                                _abi.ptr(codes), None, _abi.ptr(hT), None, ws, nws, eng.stream()))
        return codes.to(out_dev), eng.deliver(hT.unsqueeze(0), out_dev)

    @torch.no_grad()
    def decode(self, z, h, present=None, bits=None, return_codes=False):
        """z (B,T,z_dim), h (1,B,h_dim) -> (mel (B,T,x_dim), h (1,B,h_dim)).

        ``present`` (B,T) turns concealment on (``bvc_bvrnn_decode_conceal``): a frame whose entry is 0 did not arrive and is generated
        from the prior net at the decoder's own state - round(prior(h_t)), masked to ``bits[b, t]`` leading bits on a variable-rate
        model (``bits`` (B,T) is then required) - whatever ``z`` holds there.  ``return_codes=True`` adds the codes with the gaps
        filled and the prior's probabilities of every frame: (mel, h, codes_out, prior)."""
        if present is not None:
            return self._decode_conceal(z, h, present, bits, return_codes)
        if return_codes or bits is not None:
            raise ValueError("decode: bits / return_codes belong to concealment (pass present)")
        eng = self.engine(z)
        out_dev = z.device
        z = _prep(z, eng.device)
        B, T, _ = z.shape
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        mel = torch.empty(B, T, self.x_dim, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_bvrnn_decode(eng.handle, _abi.ptr(z), _abi.ptr(h0), B, T, _abi.ptr(mel),
                                                _abi.ptr(hT), ws, nws, eng.stream()))
        return mel.to(out_dev), eng.deliver(hT.unsqueeze(0), out_dev)


    @torch.no_grad()
    def _decode_conceal(self, z, h, present, bits, return_codes):
        if self.varBit and bits is None:
            raise ValueError("decode: a variable-rate model needs bits (B,T) to generate lost frames")
        if z.dim() != 3 or tuple(present.shape) != tuple(z.shape[:2]) or (bits is not None and tuple(bits.shape) != tuple(z.shape[:2])):
            raise ValueError("decode: z (B,T,z_dim) with present (B,T) and bits (B,T)")
        eng = self.engine(z)
        out_dev = z.device
        z = _prep(z, eng.device)
        B, T, _ = z.shape
        pres = present.detach().to(eng.device).ne(0).to(torch.uint8).contiguous()
        d_bits = _prep(bits, eng.device) if (bits is not None and self.varBit) else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        mel = torch.empty(B, T, self.x_dim, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device) if return_codes else None
        prior = torch.empty(B, T, self.z_dim, device=eng.device) if return_codes else None
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_bvrnn_decode_conceal(eng.handle, _abi.ptr(z), ctypes.c_void_p(pres.data_ptr()), _abi.ptr(d_bits),
                                                        _abi.ptr(h0), B, T, _abi.ptr(mel), _abi.ptr(hT), _abi.ptr(codes),
                                                        _abi.ptr(prior), ws, nws, eng.stream()))
        if return_codes:
            return mel.to(out_dev), hT.unsqueeze(0).to(out_dev), codes.to(out_dev), eng.deliver(prior, out_dev)
        return mel.to(out_dev), eng.deliver(hT.unsqueeze(0), out_dev)


class BigVGAN(_OnDevice):
    """``BigVGAN.forward(x, length)`` (models.py:207-238): x (B, num_mels, T) -> (B, 1, n)."""

    def __init__(self, conf, tensors, shared=None):
        super().__init__(conf, tensors)
        if shared is not None:
            self._engines = shared

    @torch.no_grad()
    def forward(self, x, length, _scale_div=1.0, _time_major=False):
        eng = self.engine(x)
        out_dev = x.device
        mel = _prep(x if _time_major else x.permute(0, 2, 1), eng.device)        # kernels are time-major
        B, T, _ = mel.shape
        n = _trimmed(eng.vocoder_length(T), length)
        wav = torch.empty(B, n, device=eng.device)
        if n:
            ws, nws = eng.workspace(B, T)
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_bigvgan(eng.handle, _abi.ptr(mel), B, T, n, float(_scale_div),
                                               _abi.ptr(wav), ws, nws, eng.stream()))
        return wav.unsqueeze(1).to(out_dev)


class BVRNNCodecModel(_OnDevice):
    def __init__(self, config_path=default_config, bvrnn_chkpt_path=default_chkpt_bvrnn,
                 vocoder_chkpt_path=default_chkpt_vocoder):
        """Same three arguments as the reference constructor (bvrnn_codec_model.py:20-42): the TOML file that describes
        front-end, coder and vocoder, and the two ``torch.save`` dicts holding the coder's ``'vrnn'`` and the vocoder's
        ``'generator'`` state dict.  Both checkpoints are loaded strictly; nothing touches the GPU until the first call."""
        for what, path in (("BVRNN", bvrnn_chkpt_path), ("vocoder", vocoder_chkpt_path)):
            if not os.path.exists(path):
                raise FileNotFoundError(f"{what} checkpoint not found at '{path}'.  Pass the path explicitly, or place the "
                                        f"reference's chkpts/ files (Git-LFS objects, not shipped) in '{_CHKPT_DIR}' "
                                        "(override with BVC_CHKPT_DIR)")
        conf = load_config(config_path)
        vrnn_sd = weights.load_checkpoint(bvrnn_chkpt_path, "vrnn")
        gen_sd = weights.load_checkpoint(vocoder_chkpt_path, "generator")
        super().__init__(conf, weights.host_tensors(conf, vrnn_sd, gen_sd))
        _abi.load()                                   # fail at construction if the HIP library is absent
        self.bvrnn = BVRNN(conf, self._tensors, shared=self._engines)
        self.vocoder = BigVGAN(conf, self._tensors, shared=self._engines)

    def bits_per_frame(self, bitrate):
        return float(np.round(bitrate * self.conf['hopsize'] / self.conf['fs']))   # bvrnn_codec_model.py:58

    @torch.no_grad()
    def mel_spectrogram(self, x, scale=SCALING):
        """log-mel of x*scale as the facade computes it (bvrnn_codec_model.py:49-56): (B,L) -> (B,T,80)."""
        eng = self.engine(x)
        out_dev = x.device
        x = _prep(x, eng.device)
        if x.dim() != 2:
            raise RuntimeError("expected a (batch, length) waveform")
        B, L = x.shape
        T = eng.num_frames(L)
        if T <= 0:
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                               f"(length {L} is too short for the reflect padding of the STFT front-end)")
        mel = torch.empty(B, T, self.conf["num_mels"], device=eng.device)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_stft_logmel(eng.handle, _abi.ptr(x), B, L, float(scale), _abi.ptr(mel),
                                               eng.stream()))
        return mel.to(out_dev)

    @torch.no_grad()
    def encode(self, x, bitrate, lengths=None):
        """Waveforms ``x`` (batch, samples), expected in [-1, 1], to codes (batch, samples // hop, z_dim) with values in
        {0, 1} and 0.5 at masked positions.  ``bitrate`` [bit/s] selects round(bitrate * hop / fs) leading bits per frame
        (saturating at z_dim; ignored by fixed-rate configs) - bvrnn_codec_model.py:44-62.

        Mixed-length batch: ``lengths`` (batch,) gives the valid samples of each row (the rest of the row is never read), and
        ``bitrate`` may be one value per row.  Row b then equals ``encode(x[b:b+1, :lengths[b]], bitrate[b])`` bit for bit in
        its first num_frames(lengths[b]) frames and is 0.5 after them."""
        if lengths is not None or ragged.per_row(bitrate, x.shape[0], "bitrate") is not None:
            return self._encode_ragged(x, bitrate, lengths)
        eng = self.engine(x)
        out_dev = x.device
        x = _prep(x, eng.device)
        if x.dim() != 2:
            raise RuntimeError("expected a (batch, length) waveform")
        B, L = x.shape
        T = eng.num_frames(L)
        if T <= 0:
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                               f"(length {L} is too short for the reflect padding of the STFT front-end)")
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device)
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_encode(eng.handle, _abi.ptr(x), B, L, float(SCALING), self.bits_per_frame(bitrate),
                                          _abi.ptr(codes), ws, nws, eng.stream()))
        return eng.deliver(codes, out_dev)

    @torch.no_grad()
    def encode_vbr(self, x, target, bitrates=(1500, 3000, 6000), return_bits=True, lengths=None, rate_cap=None, burst=None):
        """Closed-loop variable-rate ``encode`` (``bvc_encode_vbr``): every frame gets the lowest of ``bitrates`` at which the mel the
        receiver will decode lies within ``target`` - the mean absolute error over the bands of the natural-log mel; a scalar, (batch,)
        or (batch, frames) - of the input's, the highest where none does.  ``bitrates`` [bit/s] become bits per frame as in ``encode``
        (saturating at z_dim) and must still ascend strictly after that.  Returns (codes, bits (batch, frames)); ``decode`` takes the
        codes as they are, ``pack_vbr`` puts them on the wire.  Equal-length batches only.

        ``rate_cap`` [bit/s] caps the rate of every row for good (``bvc_encode_vbr_capped``): a token bucket that gains
        ``rate_cap * hopsize / fs`` bits per frame, holds at most ``burst`` bits (default: four times the top rung) and starts full; a
        frame never gets a rung the bucket does not hold.  If the lowest rung is within the rate, any L consecutive frames of a row
        carry at most ``burst + L * rate_cap * hopsize / fs`` bits.  ``target=-inf`` then spends whatever the bucket allows."""
        if lengths is not None:
            raise ValueError("encode_vbr: mixed-length batches (lengths=) are not supported")
        z = self.conf["z_dim"]
        rungs = [int(min(z, max(0.0, self.bits_per_frame(r)))) for r in bitrates]
        lad, K = _check_ladder(rungs, z, self.conf["var_bit"])
        cap = cap_q8(self.conf, rungs, rate_cap, burst)
        if x.dim() != 2:
            raise RuntimeError("expected a (batch, length) waveform")
        B, L = x.shape
        c = self.conf
        pr = c["winsize"] - c["mel_pad_left"] - c["hopsize"]          # bvc_num_frames
        T = 0 if (L <= c["mel_pad_left"] or L <= pr) else (L + c["mel_pad_left"] + pr - c["winsize"]) // c["hopsize"] + 1
        if T <= 0:
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                               f"(length {L} is too short for the reflect padding of the STFT front-end)")
        tau = _broadcast_target(target, B, T, "cpu")
        eng = self.engine(x)
        out_dev = x.device
        x = _prep(x, eng.device)
        tau = tau.to(eng.device)
        codes = torch.empty(B, T, z, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        ws, nws = eng.vbr_workspace(B, T, K)
        with torch.cuda.device(eng.device):
            args = (eng.handle, _abi.ptr(x), B, L, float(SCALING), _abi.ptr(tau), lad, K, _abi.ptr(codes), _abi.ptr(bits), ws, nws, eng.stream())
            _abi.check(eng.lib.bvc_encode_vbr(*args) if cap is None else eng.lib.bvc_encode_vbr_capped(*args, *cap))
        if return_bits:
            return codes.to(out_dev), eng.deliver(bits, out_dev)
        return eng.deliver(codes, out_dev)

    @torch.no_grad()
    def _encode_ragged(self, x, bitrate, lengths):
        eng = self.engine(x)
        out_dev = x.device
        x = _prep(x, eng.device)
        if x.dim() != 2:
            raise RuntimeError("expected a (batch, length) waveform")
        B, L = x.shape
        lens = ragged.per_row_ints(L if lengths is None else lengths, B, "lengths")
        if (lens > L).any():
            raise RuntimeError(f"lengths must not exceed the row length {L} (got {int(lens.max())})")
        for n in [L] + sorted(set(lens.tolist())):            # the equal-length path's check, for the row and for every utterance
            if eng.num_frames(int(n)) <= 0:
                raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                                   f"(length {int(n)} is too short for the reflect padding of the STFT front-end)")
        T = eng.num_frames(L)
        rates = ragged.per_row(bitrate, B, "bitrate")
        bits = None
        if rates is not None:                                  # bits_per_frame per row, the reference's rounding in float64
            bits = torch.from_numpy(np.round(rates * self.conf['hopsize'] / self.conf['fs']).astype(np.float32)).to(eng.device)
        d_lens = torch.from_numpy(lens).to(eng.device)
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device)
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_encode_ragged(eng.handle, _abi.ptr(x), ctypes.c_void_p(d_lens.data_ptr()), B, L, float(SCALING),
                                                 _abi.ptr(bits), self.bits_per_frame(bitrate) if rates is None else 0.0,
                                                 _abi.ptr(codes), ws, nws, eng.stream()))
        return eng.deliver(codes, out_dev)

    @torch.no_grad()
    def decode(self, codes, length, frames=None, lost=None, bitrate=None, return_codes=False):
        """Codes (batch, frames, z_dim) back to waveforms (batch, min(length, 256 * frames + 294)): coder decode from a
        zero state, vocoder, output gain undone - bvrnn_codec_model.py:64-71.  (A generator with symmetric stages makes
        ``config.generator_length(conf, frames)`` samples instead of 256 * frames + 294: 256 * frames when every stage is symmetric.)

        Mixed-length batch: ``length`` (batch,) per row, and optionally ``frames`` (batch,) valid code frames per row (default
        min(frames, num_frames(length[b])), the frame count encode gives for that length).  Returns (batch, max n_b): row b equals
        ``decode(codes[b:b+1, :frames[b]], length[b])`` in its first n_b = min(length[b], 256 * frames[b] + 294) samples and is 0
        after them (n_b = 0 for a row without frames).

        Lost frames: ``lost`` (batch, frames) bool marks the frames that did not arrive; they are generated from the model's prior
        net at the decoder's own state (``bvc_decode_conceal``), whatever ``codes`` holds there, with the bits per frame of
        ``bitrate`` (required on a variable-rate model).  ``return_codes=True`` then returns (wav, codes with the gaps filled).  Not
        together with a mixed-length batch."""
        if lost is not None:
            return self._decode_conceal(codes, length, frames, lost, bitrate, return_codes)
        if return_codes:
            raise ValueError("decode: return_codes belongs to concealment (pass lost)")
        if frames is not None or ragged.per_row(length, codes.shape[0], "length") is not None:
            if not is_causal(self.conf):
                raise ValueError("decode: " + not_causal_message(self.conf))
            return self._decode_ragged(codes, length, frames)
        eng = self.engine(codes)
        out_dev = codes.device
        codes = _prep(codes, eng.device)
        B, T, Z = codes.shape
        if Z != self.conf["z_dim"]:
            raise RuntimeError(f"codes must have {self.conf['z_dim']} values per frame, got {Z}")
        n = _trimmed(eng.vocoder_length(T), length)       # `[:, :, :length]`, models.py:238
        wav = torch.empty(B, n, device=eng.device)
        if n:                                             # (length 0 keeps nothing: an empty (B, 0) tensor like the reference's)
            ws, nws = eng.workspace(B, T)
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_decode(eng.handle, _abi.ptr(codes), B, T, n, float(SCALING),
                                              _abi.ptr(wav), ws, nws, eng.stream()))
        return eng.deliver(wav, out_dev)

    @torch.no_grad()
    def _decode_conceal(self, codes, length, frames, lost, bitrate, return_codes):
        if frames is not None or ragged.per_row(length, codes.shape[0], "length") is not None:
            raise ValueError("decode: lost frames in a mixed-length batch are not supported (decode the rows on their own)")
        if self.conf["var_bit"] and bitrate is None:
            raise ValueError("decode: a variable-rate model needs the bitrate to generate lost frames")
        if codes.dim() != 3 or tuple(lost.shape) != tuple(codes.shape[:2]):
            raise ValueError("decode: lost must be (batch, frames) like the codes")
        eng = self.engine(codes)
        out_dev = codes.device
        codes = _prep(codes, eng.device)
        B, T, Z = codes.shape
        if Z != self.conf["z_dim"]:
            raise RuntimeError(f"codes must have {self.conf['z_dim']} values per frame, got {Z}")
        present = lost.detach().to(eng.device).eq(0).to(torch.uint8).contiguous()
        n = _trimmed(eng.vocoder_length(T), length)
        wav = torch.empty(B, n, device=eng.device)
        filled = torch.empty(B, T, Z, device=eng.device) if return_codes else None
        if n:
            ws, nws = eng.workspace(B, T)
            bits = self.bits_per_frame(bitrate) if self.conf["var_bit"] else float(Z)
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_decode_conceal(eng.handle, _abi.ptr(codes), ctypes.c_void_p(present.data_ptr()), float(bits), B, T,
                                                      n, float(SCALING), _abi.ptr(wav), _abi.ptr(filled), ws, nws, eng.stream()))
        elif return_codes:
            raise ValueError("decode: the filled codes need a non-empty output (length > 0)")
        if return_codes:
            return eng.deliver(wav, out_dev), filled.to(out_dev)
        return eng.deliver(wav, out_dev)

    @torch.no_grad()
    def _decode_ragged(self, codes, length, frames):
        eng = self.engine(codes)
        out_dev = codes.device
        codes = _prep(codes, eng.device)
        B, T, Z = codes.shape
        if Z != self.conf["z_dim"]:
            raise RuntimeError(f"codes must have {self.conf['z_dim']} values per frame, got {Z}")
        lens = ragged.per_row_ints(length, B, "length")
        if (lens < 0).any():
            raise RuntimeError("per-row lengths must not be negative")
        if frames is None:
            fr = np.array([min(T, max(eng.num_frames(int(n)), 0)) for n in lens], dtype=np.int64)
        else:
            fr = ragged.per_row_ints(frames, B, "frames")
            if (fr < 0).any() or (fr > T).any():
                raise RuntimeError(f"frames must lie in [0, {T}]")
        n = [min(int(l), eng.vocoder_length(int(f))) if f > 0 else 0 for l, f in zip(lens, fr)]
        n_max = max(n) if n else 0
        wav = torch.empty(B, n_max, device=eng.device)
        if n_max:
            d_fr = torch.from_numpy(fr).to(eng.device)
            d_lens = torch.from_numpy(lens).to(eng.device)
            ws, nws = eng.workspace(B, T)
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_decode_ragged(eng.handle, _abi.ptr(codes), ctypes.c_void_p(d_fr.data_ptr()), B, T,
                                                     ctypes.c_void_p(d_lens.data_ptr()), n_max, float(SCALING), _abi.ptr(wav),
                                                     ws, nws, eng.stream()))
        return eng.deliver(wav, out_dev)

    def forward(self, x, bitrate, lengths=None):
        """decode(encode(x, bitrate)) trimmed to the input length (bvrnn_codec_model.py:73-76); with ``lengths`` (batch,),
        decode(encode(x, bitrate, lengths), lengths): row b is forward(x[b:b+1, :lengths[b]]) followed by zeros."""
        length = x.shape[1]
        codes = self.encode(x, bitrate, lengths)
        return self.decode(codes, length if lengths is None else lengths)

    # ---- corpora: lists of utterances of any lengths, coded in mixed-length batches
    @torch.no_grad()
    def encode_many(self, waves, bitrate, max_batch=64):
        """1-D waveforms of any lengths -> their codes, a list of (num_frames(len_i), z_dim) tensors in input order.
        ``bitrate``: one value, or one per item.  The items are sorted by length and coded in mixed-length calls of at most
        ``max_batch`` rows (ragged.batch_plan); item i equals ``encode(waves[i][None], bitrate_i)[0]`` bit for bit."""
        waves = list(waves)
        if not waves:
            return []
        rates = ragged.per_row(bitrate, len(waves), "bitrate")
        lens = [int(w.shape[-1]) for w in waves]
        eng = self.engine(waves[0])
        out_dev = waves[0].device
        perm, bounds, inv = ragged.batch_plan(lens, max_batch)
        done = []
        for a, e in bounds:
            idx = perm[a:e]
            x = nn.utils.rnn.pad_sequence([_prep(waves[i].reshape(-1), eng.device) for i in idx], batch_first=True)
            br = bitrate if rates is None else rates[idx]
            codes = self.encode(x, br, lengths=[lens[i] for i in idx]).to(out_dev)
            done += [codes[r, :eng.num_frames(lens[i])] for r, i in enumerate(idx)]
        return [done[k] for k in inv]

    @torch.no_grad()
    def decode_many(self, codes_list, lengths, max_batch=64):
        """(frames_i, z_dim) codes of any frame counts -> waveforms, a list of (min(len_i, 256 * frames_i + 294),) tensors in
        input order.  ``lengths``: one value, or one per item.  Item i equals ``decode(codes_list[i][None], lengths_i)[0]``."""
        codes_list = list(codes_list)
        if not codes_list:
            return []
        lens = ragged.per_row_ints(lengths, len(codes_list), "lengths")
        frames = [int(c.shape[0]) for c in codes_list]
        eng = self.engine(codes_list[0])
        out_dev = codes_list[0].device
        if not is_causal(self.conf):                      # equal-length items only: plain batches of at most max_batch rows
            if len(set(frames)) > 1 or len(set(int(n) for n in lens)) > 1:
                raise ValueError("decode_many: " + not_causal_message(self.conf))
            done = []
            for a in range(0, len(codes_list), max(int(max_batch), 1)):
                c = torch.stack([_prep(ci, eng.device) for ci in codes_list[a:a + max(int(max_batch), 1)]])
                done += list(self.decode(c, int(lens[0])).to(out_dev))
            return done
        perm, bounds, inv = ragged.batch_plan(frames, max_batch)
        done = []
        for a, e in bounds:
            idx = perm[a:e]
            c = nn.utils.rnn.pad_sequence([_prep(codes_list[i], eng.device) for i in idx], batch_first=True, padding_value=0.5)
            wav = self.decode(c, lens[idx], frames=[frames[i] for i in idx]).to(out_dev)
            done += [wav[r, :(min(int(lens[i]), eng.vocoder_length(frames[i])) if frames[i] > 0 else 0)] for r, i in enumerate(idx)]
        return [done[k] for k in inv]

    @torch.no_grad()
    def forward_fused(self, x, bitrate, return_codes=False):
        """``forward(x, bitrate)`` with ONE recurrence instead of two (``bvc_forward``): the encoder's frame loop already runs the
        decoder on every frame (bvrnn.py:198-204) from the states ``decode`` would visit again, so its outputs go to the vocoder
        directly.  Same codes as ``encode``; the waveform agrees with ``forward`` to rounding (the halves of dec.0 and of the GRU's
        input gates are summed in another order).  ``forward`` itself stays the reference's decode(encode(x))."""
        eng = self.engine(x)
        out_dev = x.device
        x = _prep(x, eng.device)
        if x.dim() != 2:
            raise RuntimeError("expected a (batch, length) waveform")
        B, L = x.shape
        T = eng.num_frames(L)
        if T <= 0:
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                               f"(length {L} is too short for the reflect padding of the STFT front-end)")
        n = _trimmed(eng.vocoder_length(T), L)
        wav = torch.empty(B, n, device=eng.device)
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device) if return_codes else None
        ws, nws = eng.workspace(B, T)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_forward(eng.handle, _abi.ptr(x), B, L, float(SCALING), self.bits_per_frame(bitrate), n, float(SCALING),
                                           _abi.ptr(codes), _abi.ptr(wav), ws, nws, eng.stream()))
        if return_codes:
            return codes.to(out_dev), eng.deliver(wav, out_dev)
        return eng.deliver(wav, out_dev)

    # ---- wire format (not in the reference, which has no bit stream: SURVEY.md 8f rank 2)
    def active_bits(self, bitrate):
        z = self.conf["z_dim"]
        return z if not self.conf["var_bit"] else int(min(z, max(0.0, self.bits_per_frame(bitrate))))

    @torch.no_grad()
    def pack(self, codes, bitrate):
        """codes (B,T,z_dim) from encode(x, bitrate) -> uint8 (B,T,ceil(n/8)), n active bits per frame."""
        eng = self.engine(codes)
        out_dev = codes.device
        codes = _prep(codes, eng.device)
        B, T, Z = codes.shape
        n = self.active_bits(bitrate)
        out = torch.empty(B, T, (n + 7) // 8, dtype=torch.uint8, device=eng.device)
        if out.numel():
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_pack_codes(_abi.ptr(codes), B, T, Z, n, ctypes.c_void_p(out.data_ptr()),
                                                  eng.stream()))
        return out.to(out_dev)

    @torch.no_grad()
    def unpack(self, packed, bitrate):
        """Inverse of pack(): uint8 (B,T,ceil(n/8)) -> float32 codes (B,T,z_dim) with 0.5 in masked positions."""
        eng = self.engine(packed)
        out_dev = packed.device
        packed = packed.to(eng.device).contiguous()
        B, T, _ = packed.shape
        n = self.active_bits(bitrate)
        Z = self.conf["z_dim"]
        codes = torch.empty(B, T, Z, device=eng.device)
        with torch.cuda.device(eng.device):
            _abi.check(eng.lib.bvc_unpack_codes(ctypes.c_void_p(packed.data_ptr()) if packed.numel() else None, B, T, Z,
                                                n, _abi.ptr(codes), eng.stream()))
        return codes.to(out_dev)

    @torch.no_grad()
    def pack_vbr(self, codes, bits):
        """codes (B,T,z_dim) and bits (B,T) from encode_vbr -> (bytes uint8 (B,T,1 + ceil(z_dim/8)), sizes int32 (B,T)): a frame is its
        bit count n, ceil(n/8) bytes of bits, zeros; sizes = 1 + ceil(n/8) are the bytes of the frame worth sending."""
        if codes.dim() != 3 or tuple(bits.shape) != tuple(codes.shape[:2]) or codes.shape[2] != self.conf["z_dim"]:
            raise ValueError("pack_vbr: codes (B, T, z_dim) with bits (B, T)")
        eng = self.engine(codes)
        out_dev = codes.device
        codes = _prep(codes, eng.device)
        bits = _prep(bits, eng.device)
        B, T, Z = codes.shape
        out = torch.empty(B, T, 1 + (Z + 7) // 8, dtype=torch.uint8, device=eng.device)
        sizes = torch.empty(B, T, dtype=torch.int32, device=eng.device)
        if sizes.numel():
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_pack_codes_vbr(_abi.ptr(codes), _abi.ptr(bits), B, T, Z, ctypes.c_void_p(out.data_ptr()),
                                                      ctypes.c_void_p(sizes.data_ptr()), eng.stream()))
        return out.to(out_dev), sizes.to(out_dev)

    @torch.no_grad()
    def unpack_vbr(self, packed):
        """Inverse of pack_vbr(): uint8 (B,T,1 + ceil(z_dim/8)) -> (codes (B,T,z_dim) with 0.5 behind each frame's bits, bits (B,T))."""
        Z = self.conf["z_dim"]
        if packed.dim() != 3 or packed.shape[2] != 1 + (Z + 7) // 8 or packed.dtype != torch.uint8:
            raise ValueError(f"unpack_vbr: uint8 (B, T, {1 + (Z + 7) // 8}) expected")
        eng = self.engine(packed)
        out_dev = packed.device
        packed = packed.to(eng.device).contiguous()
        B, T, _ = packed.shape
        codes = torch.empty(B, T, Z, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        if bits.numel():
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_unpack_codes_vbr(ctypes.c_void_p(packed.data_ptr()), B, T, Z, _abi.ptr(codes), _abi.ptr(bits),
                                                        eng.stream()))
        return codes.to(out_dev), bits.to(out_dev)
