"""The two sub-operators the reference exposes as attributes of its facade: ``BVRNN`` (``model.bvrnn.encode/decode``, bvrnn.py:163-229)
and ``BigVGAN`` (``model.vocoder(x, length)``, models.py:207-238), each on the engines of the model it is a part of."""
import numpy as np
import torch

from ._abi import ptr
from .engine import _OnDevice, _prep, _trimmed, grad_layout as _grad_layout
from .vbr_args import _check_cap_q8, _check_ladder


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


def _entropy_segments(frames, segment, who):
    """(S, nseg) of a call of ``frames`` frames cut into segments of ``segment`` (None: the whole call)."""
    if isinstance(frames, bool) or int(frames) != frames or frames < 1:
        raise ValueError(f"{who}: frames must be a positive integer, got {frames!r}")
    segment = frames if segment is None else segment
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or segment < 1:
        raise ValueError(f"{who}: segment must be an integer of at least 1 (frames per independently coded segment), got {segment!r}")
    S = min(int(segment), int(frames))
    return S, -(-int(frames) // S)


def _check_stream(data, sizes, nseg, who):
    """The shapes of an entropy-coded stream: data uint8 (B, nseg, stride), sizes an integer tensor (B, nseg)."""
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 3:
        raise ValueError(f"{who}: data must be a uint8 tensor (batch, segments, stride)")
    if not torch.is_tensor(sizes) or sizes.is_floating_point() or tuple(sizes.shape) != tuple(data.shape[:2]):
        raise ValueError(f"{who}: sizes must be an integer tensor {tuple(data.shape[:2])} like data's first two dimensions")
    if data.shape[0] < 1 or data.shape[1] != nseg:
        raise ValueError(f"{who}: {data.shape[1]} segments given, the frames and the segment length make {nseg}")


def _check_frame_bits(bits, B, T, var_bit, who):
    if var_bit and bits is None:
        raise ValueError(f"{who}: a variable-rate model needs the bits of every frame (a bitrate, or bits (batch, frames))")
    if bits is not None and (not torch.is_tensor(bits) or tuple(bits.shape) != (B, T)):
        raise ValueError(f"{who}: bits must be a tensor ({B}, {T})")


def _draw_randomness(B, T, z_dim, greedy, r, noise):
    """The random numbers of ``BVRNN.forward`` that the caller did not give, in the reference's draw order (bvrnn.py:111,126) from
    torch's global CPU generator: per frame ``torch.rand([])`` and - unless greedy - ``torch.rand(B, z_dim)``."""
    if r is None or (noise is None and not greedy):
        rs, ns = [], []
        for _ in range(T):
            rs.append(torch.rand([]))
            if not greedy:
                ns.append(torch.rand(B, z_dim))
        r = torch.stack(rs) if r is None else r
        if not greedy and noise is None:
            noise = torch.stack(ns, 1)
    return r, noise


class BVRNN(_OnDevice):
    """``BVRNN.encode`` / ``BVRNN.decode`` (bvrnn.py:163-229) on the HIP recurrent kernels."""

    def __init__(self, conf, tensors, shared=None):
        super().__init__(conf, tensors, shared)
        self.h_dim, self.z_dim, self.x_dim = conf["h_dim"], conf["z_dim"], conf["num_mels"]
        self.varBit = bool(conf["var_bit"])

    @torch.no_grad()
    def forward(self, y, p_use_gen, greedy, varBitrate, *, r=None, noise=None, return_all=False):
        """``BVRNN.forward(y, p_use_gen, greedy, varBitrate)`` (bvrnn.py:86-160), forward values only (their gradients:
        ``backward``, or ``forward_train`` for torch.autograd): stochastic Bernoulli sampler ``round(u - 0.5 + enc_t)``, prior net, KL term and the
        teacher-forcing mix.  Returns (all_dec_mean (B,T,x_dim), kld scalar) like the reference.

        Randomness: the reference draws, per frame, ``torch.rand([])`` (compared with p_use_gen) and - unless
        greedy - ``torch.rand_like(enc_t)``.  By default the same numbers are drawn here, in the same order, from
        torch's global CPU generator, so ``torch.manual_seed(s)`` followed by this call reproduces the reference
        run on CPU after the same seed.  ``r`` (T,) / ``noise`` (B,T,z_dim) override them.
        ``return_all=True`` adds a dict with z (forward value of the sample), prob (enc_t), prior, kld_frames."""
        eng, out_dev, y = self._enter(y)
        B, T, _ = y.shape
        r, noise = _draw_randomness(B, T, self.z_dim, greedy, r, noise)
        use_gen = (torch.as_tensor(r).detach().cpu().float() < p_use_gen).to(torch.uint8).contiguous()
        assert use_gen.numel() == T
        bits = _prep(varBitrate, eng.device) if (varBitrate is not None and self.varBit) else None
        un = None if greedy else _prep(noise, eng.device)
        dec = torch.empty(B, T, self.x_dim, device=eng.device)
        kld = torch.empty(T, device=eng.device)
        extra = {k: torch.empty(B, T, self.z_dim, device=eng.device) for k in ("z", "prob", "prior")} if return_all else {}
        eng.call("bvc_bvrnn_forward", eng.handle, ptr(y), ptr(bits), ptr(use_gen, torch.uint8), int(p_use_gen < 1), int(p_use_gen > 0),
                 ptr(un), B, T, ptr(dec), ptr(kld), ptr(extra.get("z")), ptr(extra.get("prob")), ptr(extra.get("prior")), scratch=(B, T))
        if return_all:
            extra["kld_frames"] = kld
        # torch.mean(torch.stack(kld_loss)), bvrnn.py:160
        out = eng.to_caller(out_dev, dec, torch.mean(kld), *extra.values(), poll=False)
        return out[:2] + (dict(zip(extra, out[2:])),) if return_all else out

    def grad_parameters(self):
        """The trainable tensors of ``BVRNN.forward`` as this model holds them NOW - after ``load_parameters`` or an optimiser step, the
        updated values: a dict of float32 CPU copies keyed by the reference's state-dict names (36 tensors; not mean_mel / std_mel,
        which are buffers, nor log_sigma, which does not enter forward)."""
        tensors = self._live_tensors()
        names = [n for n in tensors if n.split(".")[0] in ("phi_x", "phi_z", "enc", "prior", "dec", "rnn")]
        return {n: tensors[n].detach().clone() for n in names}

    def grad_layout(self):
        """``bvc_bvrnn_grad_layout``: ([(name, offset, numel)], total floats) of the flat gradient buffer of ``backward`` (needs no GPU)."""
        return _grad_layout(self.conf)

    def _check_named(self, tensors, who):
        """A dict of tensors keyed by some of the 36 trainable names, each of its state-dict shape."""
        if not isinstance(tensors, dict):
            raise ValueError(f"{who}: a dict keyed by state-dict names expected, got {type(tensors).__name__}")
        known = {n for n, _, _ in self.grad_layout()[0]}
        unknown = [n for n in tensors if n not in known]
        if unknown:
            raise ValueError(f"{who}: {unknown} are no trainable tensors of BVRNN.forward")
        for n, t in tensors.items():
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != tuple(self._tensors[n].shape)):
                raise ValueError(f"{who}: '{n}' must be a tensor {tuple(self._tensors[n].shape)}, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")

    @torch.no_grad()
    def load_parameters(self, tensors):
        """New values for some of the 36 trainable tensors (a dict keyed like ``grad_parameters()``), written into the LIVE model
        (``bvc_bvrnn_params_get``, patch, ``bvc_bvrnn_params_set``): every form of the weights the kernels read is rewritten in
        place on the device, stream-ordered on the current stream, and the next call - on any schedule, a captured graph included -
        runs on them; the model is then bit for bit the one a checkpoint with these values loads.  It applies to the engine of the
        model's device (engines on other devices keep their values); a call in flight on another stream is the caller's to
        serialise."""
        self._check_named(tensors, "load_parameters")
        eng = self.engine()
        layout, total = self.grad_layout()
        flat = eng.params_get(total)
        for name, off, numel in layout:
            if tensors.get(name) is not None:
                flat[off:off + numel].copy_(_prep(tensors[name], eng.device).reshape(-1))
        eng.params_set(flat)
        self._tensors.stale = eng

    def optimizer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0):
        """An AdamW optimiser of this model's trainable tensors (``bvcodec.optim.AdamW``; torch.optim.AdamW's defaults): its ``step``
        takes what ``backward`` returns and updates the live model in place.  ``max_grad_norm > 0`` clips the gradients' 2-norm first
        (torch.nn.utils.clip_grad_norm_)."""
        from .optim import AdamW
        return AdamW(self, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)

    def _check_backward_args(self, y, greedy, varBitrate, grad_dec, grad_kld, r, noise):
        if not torch.is_tensor(y) or y.dim() != 3 or y.shape[2] != self.x_dim or y.shape[0] < 1 or y.shape[1] < 1:
            raise ValueError(f"backward: y must be (B, T, {self.x_dim})")
        B, T, _ = y.shape
        if not torch.is_tensor(grad_dec) or tuple(grad_dec.shape) != (B, T, self.x_dim):
            raise ValueError(f"backward: grad_dec must be ({B}, {T}, {self.x_dim}) like all_dec_mean, got "
                             f"{tuple(grad_dec.shape) if torch.is_tensor(grad_dec) else type(grad_dec).__name__}")
        if torch.is_tensor(grad_kld):
            if grad_kld.numel() != 1 or grad_kld.dim() > 0:
                raise ValueError(f"backward: grad_kld must be a scalar, got a tensor {tuple(grad_kld.shape)}")
        elif isinstance(grad_kld, bool) or not isinstance(grad_kld, (int, float, np.floating, np.integer)):
            raise ValueError(f"backward: grad_kld must be a scalar, got {type(grad_kld).__name__}")
        if r is not None and tuple(torch.as_tensor(r).shape) != (T,):
            raise ValueError(f"backward: r must be ({T},), got {tuple(torch.as_tensor(r).shape)}")
        if noise is not None and not greedy and tuple(torch.as_tensor(noise).shape) != (B, T, self.z_dim):
            raise ValueError(f"backward: noise must be ({B}, {T}, {self.z_dim}), got {tuple(torch.as_tensor(noise).shape)}")
        if self.varBit and (varBitrate is None or not torch.is_tensor(varBitrate) or tuple(varBitrate.shape) != (B, T)):
            raise ValueError(f"backward: a variable-rate model needs varBitrate ({B}, {T})")
        return B, T

    @torch.no_grad()
    def backward(self, y, p_use_gen, greedy, varBitrate, grad_dec, grad_kld, *, r=None, noise=None, grad_input=False,
                 return_forward=False, flat=False):
        """The vector-Jacobian product of ``forward`` (``bvc_bvrnn_backward``): given ``grad_dec`` (B,T,x_dim), the gradient of a
        loss with respect to all_dec_mean, and the scalar ``grad_kld``, its gradient with respect to the returned kld, a dict of the
        loss's gradients keyed by the reference's state-dict names, each of its state-dict shape (``grad_parameters`` has the same
        keys); ``grad_input=True`` adds "y", the gradient with respect to the input mel.  The call runs its own forward, with the
        randomness of ``forward``: the same draws in the same order from the global CPU generator unless ``r`` / ``noise`` are
        given.  ``return_forward=True``: (grads, dict(dec, kld, kld_frames, z, prob, prior)), that forward's values - the bits
        ``forward`` returns for the same inputs.  ``flat=True``: instead of the dict, the flat device buffer the library wrote
        (``grad_layout``), on the model's device - what ``optimizer().step`` takes as it is; not together with ``grad_input``.  The
        call leaves the model's weights alone: ``optimizer()`` updates them in place."""
        B, T = self._check_backward_args(y, greedy, varBitrate, grad_dec, grad_kld, r, noise)
        if flat and grad_input:
            raise ValueError("backward: flat=True returns the parameters' gradients only (not together with grad_input)")
        eng, out_dev, y = self._enter(y)
        r, noise = _draw_randomness(B, T, self.z_dim, greedy, r, noise)
        use_gen = (torch.as_tensor(r).detach().cpu().float() < p_use_gen).to(torch.uint8).contiguous()
        bits = _prep(varBitrate, eng.device) if (varBitrate is not None and self.varBit) else None
        un = None if greedy else _prep(noise, eng.device)
        gdec = _prep(grad_dec, eng.device)
        layout, total = self.grad_layout()
        want_flat, flat = flat, torch.empty(total, device=eng.device)
        gy = torch.empty(B, T, self.x_dim, device=eng.device) if grad_input else None
        fwd = {}
        if return_forward:
            fwd = {"dec": torch.empty(B, T, self.x_dim, device=eng.device), "kld_frames": torch.empty(T, device=eng.device)}
            fwd.update({k: torch.empty(B, T, self.z_dim, device=eng.device) for k in ("z", "prob", "prior")})
        eng.call("bvc_bvrnn_backward", eng.handle, ptr(y), ptr(bits), ptr(use_gen, torch.uint8), int(p_use_gen < 1), int(p_use_gen > 0),
                 ptr(un), B, T, ptr(gdec), float(grad_kld), ptr(flat), ptr(gy), ptr(fwd.get("dec")), ptr(fwd.get("kld_frames")),
                 ptr(fwd.get("z")), ptr(fwd.get("prob")), ptr(fwd.get("prior")), scratch=(B, T, "backward"))
        grads = flat if want_flat else {name: flat[off:off + numel].view(self._tensors[name].shape).to(out_dev) for name, off, numel in layout}
        if grad_input:
            grads["y"] = gy.to(out_dev)
        if not return_forward:
            return grads
        fwd["kld"] = torch.mean(fwd["kld_frames"])
        return grads, {k: v.to(out_dev) for k, v in fwd.items()}

    def forward_train(self, y, p_use_gen, greedy, varBitrate, params, *, r=None, noise=None):
        """``forward`` attached to torch.autograd (``bvcodec.autograd``): (all_dec_mean, kld) whose ``.backward()`` fills ``.grad`` of
        ``y``, if it requires grad, and of the leaf tensors in ``params`` - a dict like ``grad_parameters()``.  The values are
        computed with the MODEL's weights: ``params`` must hold the model's values, nothing checks it."""
        from .autograd import forward_train
        return forward_train(self, y, p_use_gen, greedy, varBitrate, params, r=r, noise=noise)

    def _encode(self, y, varBitrate, h, want_all_h=False, want_h_next=False, want_prob=False):
        """``bvc_bvrnn_encode``: the codes and those of its three optional outputs that are asked for, in the order of the arguments."""
        eng, out_dev, y = self._enter(y)
        B, T, _ = y.shape
        bits = _prep(varBitrate, eng.device) if varBitrate is not None else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        all_h = torch.empty(B, T, self.h_dim, device=eng.device) if want_all_h else None
        hT = torch.empty(B, self.h_dim, device=eng.device) if want_h_next else None
        prob = torch.empty(B, T, self.z_dim, device=eng.device) if want_prob else None
        eng.call("bvc_bvrnn_encode", eng.handle, ptr(y), ptr(bits), ptr(h0), B, T, ptr(codes), ptr(all_h), ptr(hT), ptr(prob),
                 scratch=(B, T))
        outs = [codes] + ([all_h] if want_all_h else []) + ([hT.unsqueeze(0)] if want_h_next else []) + ([prob] if want_prob else [])
        return eng.to_caller(out_dev, *outs)

    @torch.no_grad()
    def encode(self, y, varBitrate, h, return_prob=False):
        """y (B,T,x_dim), varBitrate (B,T) bits/frame, h (1,B,h_dim) -> (codes (B,T,z), all_h (B,T,h))."""
        return self._encode(y, varBitrate, h, want_all_h=True, want_prob=return_prob)

    @torch.no_grad()
    def encode_stateful(self, y, varBitrate, h):
        """Like encode() but returns the state AFTER the last frame instead of the per-frame states:
        (codes (B,T,z), h_next (1,B,h_dim)).  This is what chunked / streaming encoding needs (the
        reference's encode() only exposes the state before each frame, bvrnn.py:205,209)."""
        return self._encode(y, varBitrate, h, want_h_next=True)

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
        eng, out_dev, y = self._enter(y)
        tau = tau.to(eng.device)
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        all_h = torch.empty(B, T, self.h_dim, device=eng.device)
        extra = {}
        if return_all:
            extra = {"prob": torch.empty(B, T, self.z_dim, device=eng.device), "dist": torch.empty(B, T, K, device=eng.device),
                     "dec": torch.empty(B, T, self.x_dim, device=eng.device), "h_next": torch.empty(B, self.h_dim, device=eng.device)}
        args = (eng.handle, ptr(y), ptr(tau), lad, K, ptr(h0), B, T, ptr(codes), ptr(bits), ptr(all_h), ptr(extra.get("h_next")),
                ptr(extra.get("prob")), ptr(extra.get("dist")), ptr(extra.get("dec")))
        if capped:
            tok0 = None
            if tok is not None:
                tok0 = torch.as_tensor(tok).detach().to(device=eng.device, dtype=torch.int32).contiguous()
                if tuple(tok0.shape) != (B,):
                    raise ValueError(f"encode_vbr: tok must be ({B},), got {tuple(tok0.shape)}")
            tok_next = torch.empty(B, dtype=torch.int32, device=eng.device)
            eng.call("bvc_bvrnn_encode_vbr_capped", *args, scratch=(B, T, K),
                     after=(rate_q8, burst_q8, ptr(tok0, torch.int32), ptr(tok_next, torch.int32)))
        else:
            eng.call("bvc_bvrnn_encode_vbr", *args, scratch=(B, T, K))
        if return_all:
            extra["h_next"] = extra["h_next"].unsqueeze(0)
            if capped:
                extra["tok_next"] = tok_next
        out = eng.to_caller(out_dev, codes, bits, all_h, *extra.values())
        return out[:3] + (dict(zip(extra, out[3:])),) if return_all else out

    @torch.no_grad()
    def decode(self, z, h, present=None, bits=None, return_codes=False):
        """z (B,T,z_dim), h (1,B,h_dim) -> (mel (B,T,x_dim), h (1,B,h_dim)).

        ``present`` (B,T) turns concealment on (``bvc_bvrnn_decode_conceal``): a frame whose entry is 0 did not arrive and is generated
        from the prior net at the decoder's own state - round(prior(h_t)), masked to ``bits[b, t]`` leading bits on a variable-rate
        model (``bits`` (B,T) is then required) - whatever ``z`` holds there.  ``return_codes=True`` adds the codes with the gaps
        filled and the prior's probabilities of every frame: (mel, h, codes_out, prior)."""
        if present is None:
            if return_codes or bits is not None:
                raise ValueError("decode: bits / return_codes belong to concealment (pass present)")
        elif self.varBit and bits is None:
            raise ValueError("decode: a variable-rate model needs bits (B,T) to generate lost frames")
        elif z.dim() != 3 or tuple(present.shape) != tuple(z.shape[:2]) or (bits is not None and tuple(bits.shape) != tuple(z.shape[:2])):
            raise ValueError("decode: z (B,T,z_dim) with present (B,T) and bits (B,T)")
        eng, out_dev, z = self._enter(z)
        B, T, _ = z.shape
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        mel = torch.empty(B, T, self.x_dim, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        if present is None:
            eng.call("bvc_bvrnn_decode", eng.handle, ptr(z), ptr(h0), B, T, ptr(mel), ptr(hT), scratch=(B, T))
            return eng.to_caller(out_dev, mel, hT.unsqueeze(0))
        pres = present.detach().to(eng.device).ne(0).to(torch.uint8).contiguous()
        d_bits = _prep(bits, eng.device) if (bits is not None and self.varBit) else None
        codes = torch.empty(B, T, self.z_dim, device=eng.device) if return_codes else None
        prior = torch.empty(B, T, self.z_dim, device=eng.device) if return_codes else None
        eng.call("bvc_bvrnn_decode_conceal", eng.handle, ptr(z), ptr(pres, torch.uint8), ptr(d_bits), ptr(h0), B, T, ptr(mel), ptr(hT),
                 ptr(codes), ptr(prior), scratch=(B, T))
        return eng.to_caller(out_dev, mel, hT.unsqueeze(0), *((codes, prior) if return_codes else ()))

    # ---- entropy-coded wire format (include/bvcodec.h): the codes range-coded under the prior net at the decoder's own states
    @torch.no_grad()
    def entropy_pack(self, z, bits, h, segment=None, return_prior=False):
        """z (B,T,z_dim), bits (B,T) or None on a fixed-rate model, h (1,B,h_dim) -> (data uint8 (B, nseg, stride), sizes int32
        (B, nseg), h_next (1,B,h_dim)) (``bvc_bvrnn_entropy_pack``): segment s of row b is data[b, s, :sizes[b, s]], the frames
        [s S, (s + 1) S) coded on their own coder, S = ``segment`` (None: all T frames), stride = the safe stride that no segment
        exceeds.  ``return_prior=True`` adds the probabilities the bits were coded under, (B,T,z_dim)."""
        if z.dim() != 3 or z.shape[2] != self.z_dim or z.shape[0] < 1:
            raise ValueError(f"entropy_pack: z must be (B, T, {self.z_dim})")
        B, T, _ = z.shape
        S, nseg = _entropy_segments(T, segment, "entropy_pack")
        _check_frame_bits(bits, B, T, self.varBit, "entropy_pack")
        eng, out_dev, z = self._enter(z)
        d_bits = _prep(bits, eng.device) if (bits is not None and self.varBit) else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        stride = int(eng.lib.bvc_entropy_stride(self.z_dim, S))
        data = torch.empty(B, nseg, stride, dtype=torch.uint8, device=eng.device)
        sizes = torch.empty(B, nseg, dtype=torch.int32, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        prior = torch.empty(B, T, self.z_dim, device=eng.device) if return_prior else None
        eng.call("bvc_bvrnn_entropy_pack", eng.handle, ptr(z), ptr(d_bits), ptr(h0), B, T, S, ptr(data, torch.uint8), stride,
                 ptr(sizes, torch.int32), ptr(hT), ptr(prior), scratch=(B, T, "entropy"))
        return eng.to_caller(out_dev, data, sizes, hT.unsqueeze(0), *((prior,) if return_prior else ()))

    @torch.no_grad()
    def entropy_unpack(self, data, sizes, frames, bits, h, segment=None, return_prior=False):
        """The inverse, and the decoder in one recurrence (``bvc_bvrnn_entropy_unpack``): data (B, nseg, any stride >= max size), sizes
        (B, nseg), ``frames`` = T, bits (B,T) or None on a fixed-rate model, h (1,B,h_dim) -> (codes (B,T,z_dim), mel (B,T,x_dim),
        h_next (1,B,h_dim)); with ``return_prior=True`` also the prior's probabilities.  Same ``segment`` as the sender's."""
        S, nseg = _entropy_segments(frames, segment, "entropy_unpack")
        _check_stream(data, sizes, nseg, "entropy_unpack")
        B, T = data.shape[0], int(frames)
        _check_frame_bits(bits, B, T, self.varBit, "entropy_unpack")
        eng, out_dev = self.engine(data), data.device
        data = data.to(eng.device).contiguous()
        sizes = sizes.detach().to(device=eng.device, dtype=torch.int32).contiguous()
        d_bits = _prep(bits, eng.device) if (bits is not None and self.varBit) else None
        h0 = _prep(h.reshape(B, self.h_dim), eng.device)
        codes = torch.empty(B, T, self.z_dim, device=eng.device)
        mel = torch.empty(B, T, self.x_dim, device=eng.device)
        hT = torch.empty(B, self.h_dim, device=eng.device)
        prior = torch.empty(B, T, self.z_dim, device=eng.device) if return_prior else None
        eng.call("bvc_bvrnn_entropy_unpack", eng.handle, ptr(data, torch.uint8) if data.numel() else None, data.shape[2],
                 ptr(sizes, torch.int32), ptr(d_bits), ptr(h0), B, T, S, ptr(codes), ptr(mel), ptr(hT), ptr(prior), scratch=(B, T, "entropy"))
        return eng.to_caller(out_dev, codes, mel, hT.unsqueeze(0), *((prior,) if return_prior else ()))


class BigVGAN(_OnDevice):
    """``BigVGAN.forward(x, length)`` (models.py:207-238): x (B, num_mels, T) -> (B, 1, n)."""

    @torch.no_grad()
    def forward(self, x, length, _scale_div=1.0, _time_major=False):
        eng, out_dev, mel = self._enter(x if _time_major else x.permute(0, 2, 1))        # kernels are time-major
        B, T, _ = mel.shape
        n = _trimmed(eng.vocoder_length(T), length)
        wav = torch.empty(B, n, device=eng.device)
        if n:
            eng.call("bvc_bigvgan", eng.handle, ptr(mel), B, T, n, float(_scale_div), ptr(wav), scratch=(B, T))
        return eng.to_caller(out_dev, wav.unsqueeze(1), poll=False)
