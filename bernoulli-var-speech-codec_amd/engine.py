"""What every operator of the facade stands on: ``_Engine``, one device-resident copy of the weights with the one path every library
call takes and the one way outputs go back to the caller; ``_OnDevice``, the module that creates engines where its inputs live; and
the checks of the two arguments most calls take, a waveform and a tensor of codes.
"""
import ctypes

import torch
from torch import nn

from . import _abi


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


def grad_layout(conf):
    """``bvc_bvrnn_grad_layout``: ([(name, offset, numel)], total floats) of the flat buffer of the coder's 36 trainable tensors - the
    gradients of ``BVRNN.backward``, the parameters and the optimiser's moments (needs no GPU)."""
    lib = _abi.load()
    cfg = _abi.BvcConfig()
    cfg.num_mels, cfg.h_dim, cfg.z_dim, cfg.var_bit = conf["num_mels"], conf["h_dim"], conf["z_dim"], int(bool(conf["var_bit"]))
    n, total = ctypes.c_int32(0), ctypes.c_int64(0)
    _abi.check(lib.bvc_bvrnn_grad_layout(ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), ctypes.byref(total)))
    names, offs, nums = (ctypes.c_char_p * n.value)(), (ctypes.c_int64 * n.value)(), (ctypes.c_int64 * n.value)()
    _abi.check(lib.bvc_bvrnn_grad_layout(ctypes.byref(cfg), names, offs, nums, n.value, None, None))
    return [(names[i].decode(), int(offs[i]), int(nums[i])) for i in range(n.value)], int(total.value)


class _Tensors(dict):
    """The host tensors a model was loaded with, by name: what an engine is created from.  ``stale``: the engine whose coder weights
    were updated in place (``load_parameters``, an optimiser step) since these copies were made, or None; ``_OnDevice._live_tensors``
    fetches them when somebody reads the copies."""
    stale = None


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
            arr[i].name, arr[i].h_data, arr[i].numel = n.encode(), _abi.ptr(t), t.numel()
        # destroyed with the engine: whatever the library creates on this model keeps the engine alive (_abi.Handle's ``keep``)
        self.handle = _abi.Handle(self.lib.bvc_model_destroy)
        with torch.cuda.device(device):
            _abi.check(self.lib.bvc_model_create(ctypes.byref(cfg), arr, len(names), ctypes.byref(self.handle)))
        self._ws = {}            # one workspace per stream: calls on different streams may overlap

    def workspace(self, B, T, K=None):
        """Scratch for one call, owned by the CURRENT stream (the C ABI allows one in-flight call per
        (model, workspace); independent batches issued on different streams therefore overlap): the stream's buffer, grown if
        need be.  ``K``: the rungs of a closed-loop call, which takes ``bvc_vbr_workspace_bytes``, or "entropy" for a call of the
        entropy-coded wire format, which takes ``bvc_entropy_workspace_bytes``, or "backward" for ``bvc_bvrnn_backward``."""
        if K is None:
            need = self.lib.bvc_workspace_bytes(self.handle, B, T)
        elif K == "entropy":
            need = self.lib.bvc_entropy_workspace_bytes(self.handle, B, T)
        elif K == "backward":
            need = self.lib.bvc_bvrnn_backward_workspace_bytes(self.handle, B, T)
        else:
            need = self.lib.bvc_vbr_workspace_bytes(self.handle, B, T, K)
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws[key] = None
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return _abi.ptr(ws, torch.uint8), ws.numel()

    def stream(self):
        return _abi.current_stream(self.device)

    def call(self, name, *args, scratch=None, after=(), stream=True):
        """The library call ``name(*args[, workspace, bytes][, stream], *after)`` on this engine's device and the current stream; raises
        unless it returns BVC_OK.  ``scratch``: the (B, T) or (B, T, K) the call takes scratch for (``workspace``).  ``after``: what
        the entry point takes behind its stream.  Nothing here synchronises: a call may be captured into the caller's graph."""
        ws = () if scratch is None else self.workspace(*scratch)
        with torch.cuda.device(self.device):
            _abi.check(getattr(self.lib, name)(*args, *ws, *((self.stream(),) if stream else ()), *after))

    def to_caller(self, out_dev, *outs, poll=True):
        """The outputs of one call on the caller's device: one tensor, or a tuple of them.  A copy to the CPU blocks until the call
        has finished: the recurrence's status word is then final for THIS call, and it is looked at once, behind the copy of the
        last output - a time-out is raised here rather than by the next call.  ``poll=False``: the calls that do not look (front-end,
        vocoder and wire format run no recurrence; ``BVRNN.forward``)."""
        res = tuple(o.to(out_dev) for o in outs)
        if poll and torch.device(out_dev).type == "cpu":
            self.poll_status()
        return res[0] if len(res) == 1 else res

    def params_get(self, total):
        """``bvc_bvrnn_params_get``: the coder's trainable tensors as this engine holds them, one flat device tensor (``grad_layout``)."""
        flat = torch.empty(total, device=self.device)
        self.call("bvc_bvrnn_params_get", self.handle, _abi.ptr(flat))
        return flat

    def params_set(self, flat):
        """``bvc_bvrnn_params_set``: every form of the coder's weights rewritten in place from the flat device tensor ``flat``."""
        self.call("bvc_bvrnn_params_set", self.handle, _abi.ptr(flat))

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


def _wave_dims(x):
    """(batch, samples) of a waveform argument."""
    if x.dim() != 2:
        raise RuntimeError("expected a (batch, length) waveform")
    return x.shape


def _wave_frames(L, num_frames):
    """The frames of a waveform of L samples, ``num_frames(L)``; the reference's error where the reflect padding does not fit."""
    T = num_frames(L)
    if T <= 0:
        raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension "
                           f"(length {L} is too short for the reflect padding of the STFT front-end)")
    return T


def _codes_dims(codes, z_dim):
    """(batch, frames, z_dim) of a codes argument."""
    B, T, Z = codes.shape
    if Z != z_dim:
        raise RuntimeError(f"codes must have {z_dim} values per frame, got {Z}")
    return B, T, Z


class _OnDevice(nn.Module):
    """Shared plumbing: lazily creates the engine on the module's device.  ``shared``: the engine table of the module this one is a
    part of, so that the whole model holds one engine per device."""

    def __init__(self, conf, tensors, shared=None):
        super().__init__()
        self.conf = conf
        self._tensors = tensors if isinstance(tensors, _Tensors) else _Tensors(tensors)
        self._engines = {} if shared is None else shared
        self._device = None

    def _live_tensors(self):
        """``self._tensors`` with the coder's trainable tensors as the model holds them NOW: after ``load_parameters`` or an
        optimiser step the CPU copies are refreshed here, once, from the engine that was updated (``bvc_bvrnn_params_get``)."""
        eng, self._tensors.stale = self._tensors.stale, None
        if eng is not None:
            layout, total = grad_layout(self.conf)
            flat = eng.params_get(total).cpu()
            for name, off, numel in layout:
                self._tensors[name] = flat[off:off + numel].view(self._tensors[name].shape).clone()
        return self._tensors

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
            self._engines[dev] = _Engine(self.conf, self._live_tensors(), dev)     # (a new engine starts from the updated weights)
            if getattr(self, "_recurrence", None) is not None:
                self._engines[dev].set_option("recurrence", self._SCHEDULES[self._recurrence])
        return self._engines[dev]

    def _enter(self, t):
        """(engine, the caller's device, ``t`` as float32 on the engine's device) for a call whose first tensor is ``t``."""
        eng = self.engine(t)
        return eng, t.device, _prep(t, eng.device)
