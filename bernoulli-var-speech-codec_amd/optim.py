"""``AdamW`` for the mel coder, on the device (``bvc_optimizer_*``, include/bvcodec.h): the parameters, the two moments and the update
live in device memory; ``step`` takes the gradients ``BVRNN.backward`` writes and ends with every form of the weights the model's
kernels read rewritten in place, so the next ``encode`` / ``decode`` / ``forward`` / ``backward`` - on any schedule, a captured graph
included - runs on the new values without a host copy or a new model.  Obtained through ``model.bvrnn.optimizer(...)``.

    opt = model.bvrnn.optimizer(lr=1e-4, max_grad_norm=1000.0)
    for y, bits in batches:
        flat, fwd = model.bvrnn.backward(y, p, False, bits, grad_dec, grad_kld, return_forward=True, flat=True)
        opt.step(flat)

The arithmetic is torch.optim.AdamW's (no amsgrad, no maximize) in float32; ``weight_decay=0`` gives Adam.  One parameter group: the
36 trainable tensors.  A step is ordered on the current stream of the model's device; a call in flight on another stream while the
weights change is the caller's to serialise, and a step cannot be captured into a graph (its scalars change with every step)."""
import ctypes
import numbers

import torch

from . import _abi
from ._abi import ptr


def _check_hyper(lr, betas, eps, weight_decay, max_grad_norm):
    num = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool) and v == v
    if not num(lr) or lr < 0:
        raise ValueError(f"AdamW: invalid learning rate: {lr!r}")
    if not isinstance(betas, (tuple, list)) or len(betas) != 2 or not all(num(b) and 0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"AdamW: invalid betas (two values in [0, 1)): {betas!r}")
    if not num(eps) or eps <= 0:
        raise ValueError(f"AdamW: invalid epsilon value: {eps!r}")
    if not num(weight_decay) or weight_decay < 0:
        raise ValueError(f"AdamW: invalid weight_decay value: {weight_decay!r}")
    if not num(max_grad_norm) or max_grad_norm < 0:
        raise ValueError(f"AdamW: invalid max_grad_norm (0: no clipping): {max_grad_norm!r}")


class AdamW:
    """``lr``, ``betas``, ``eps``, ``weight_decay`` and ``max_grad_norm`` are plain attributes, read (and checked) at every step: a
    schedule is an assignment between two steps.  Nothing touches the GPU before the first ``step`` / ``state_dict`` /
    ``load_state_dict``."""

    def __init__(self, bvrnn, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0):
        _check_hyper(lr, betas, eps, weight_decay, max_grad_norm)
        self.bvrnn = bvrnn
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = lr, tuple(betas), eps, weight_decay, max_grad_norm
        self._layout, self._total = bvrnn.grad_layout()
        self._shapes = {n: tuple(bvrnn._tensors[n].shape) for n, _, _ in self._layout}
        self._eng = self._handle = None

    def _engine(self):
        """The engine of the model's device and this optimiser's handle on it (created at the first use)."""
        if self._handle is None:
            eng = self.bvrnn.engine()
            handle = _abi.Handle(eng.lib.bvc_optimizer_destroy, eng)
            with torch.cuda.device(eng.device):
                _abi.check(eng.lib.bvc_optimizer_create(eng.handle, ctypes.byref(handle)))
            self._eng, self._handle = eng, handle
        return self._eng

    def _flatten(self, named, who, device):
        """A dict of tensors keyed by some of the trainable names (a missing name or None: zeros) as one flat device tensor."""
        self.bvrnn._check_named(named, who)
        flat = torch.zeros(self._total, device=device)
        for name, off, numel in self._layout:
            if named.get(name) is not None:
                flat[off:off + numel].copy_(named[name].detach().reshape(-1))
        return flat

    def _split(self, flat):
        return {name: flat[off:off + numel].view(self._shapes[name]) for name, off, numel in self._layout}

    @torch.no_grad()
    def step(self, grads, params=None):
        """One step from ``grads``: the dict ``backward`` returns (or ``{name: p.grad}`` of ``forward_train``'s leaves; a name that is
        missing or None has a zero gradient), or the flat device tensor of ``backward(..., flat=True)``.  Returns the gradients'
        2-norm before clipping, a scalar on the device (what clip_grad_norm_ returns).  ``params``: a dict of leaf tensors keyed like
        ``grad_parameters()``; each is overwritten with the model's new values, so that it keeps holding them as ``forward_train``
        demands."""
        _check_hyper(self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm)
        if params is not None:
            self.bvrnn._check_named(params, "AdamW.step: params")
        if isinstance(grads, dict):
            grads = {k: v for k, v in grads.items() if k != "y"}          # backward(grad_input=True) adds the input's gradient
            self.bvrnn._check_named(grads, "AdamW.step")
        elif not torch.is_tensor(grads) or grads.dim() != 1 or grads.numel() != self._total:
            raise ValueError(f"AdamW.step: a dict of gradients or a flat tensor of {self._total} floats expected")
        eng = self._engine()
        flat = self._flatten(grads, "AdamW.step", eng.device) if isinstance(grads, dict) else grads.detach().to(device=eng.device, dtype=torch.float32).contiguous()
        cfg = _abi.BvcAdamWConfig(float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                                  float(self.max_grad_norm))
        norm = torch.empty((), device=eng.device)
        eng.call("bvc_optimizer_step", self._handle, ctypes.byref(cfg), ptr(flat), ptr(norm))
        self.bvrnn._tensors.stale = eng
        if params:
            new = self._split(eng.params_get(self._total))
            for name, p in params.items():
                p.copy_(new[name])
        return norm

    @torch.no_grad()
    def state_dict(self):
        """{"step": steps taken, "state": {name: {"exp_avg", "exp_avg_sq"}}} with CPU tensors of the parameters' shapes."""
        eng = self._engine()
        step = ctypes.c_int64(0)
        m, v = torch.empty(self._total, device=eng.device), torch.empty(self._total, device=eng.device)
        eng.call("bvc_optimizer_state_get", self._handle, ctypes.byref(step), ptr(m), ptr(v))
        m, v = self._split(m.cpu()), self._split(v.cpu())
        return {"step": int(step.value), "state": {n: {"exp_avg": m[n].clone(), "exp_avg_sq": v[n].clone()} for n in m}}

    @torch.no_grad()
    def load_state_dict(self, state):
        """The inverse of ``state_dict``: every one of the 36 names with both moments, and the step count."""
        if not isinstance(state, dict) or "step" not in state or not isinstance(state.get("state"), dict):
            raise ValueError("AdamW.load_state_dict: {'step': n, 'state': {name: {'exp_avg', 'exp_avg_sq'}}} expected")
        step = state["step"]
        if isinstance(step, bool) or int(step) != step or step < 0:
            raise ValueError(f"AdamW.load_state_dict: step must be a non-negative integer, got {step!r}")
        moments = []
        for key in ("exp_avg", "exp_avg_sq"):
            missing = [n for n, _, _ in self._layout if not isinstance(state["state"].get(n), dict) or state["state"][n].get(key) is None]
            if missing:
                raise ValueError(f"AdamW.load_state_dict: {key} of {missing[:4]} is missing")
            moments.append({n: s[key] for n, s in state["state"].items()})
            self.bvrnn._check_named(moments[-1], "AdamW.load_state_dict")
        eng = self._engine()
        m, v = (self._flatten(d, "AdamW.load_state_dict", eng.device) for d in moments)
        eng.call("bvc_optimizer_state_set", self._handle, ctypes.byref(ctypes.c_int64(int(step))), ptr(m), ptr(v))
