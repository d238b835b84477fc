"""Drop-in facade: ``BVRNNCodecModel(config_path, bvrnn_chkpt_path, vocoder_chkpt_path)`` with
``encode(x, bitrate)``, ``decode(codes, length)``, ``forward(x, bitrate)`` - same names, argument
meaning and error behaviour as the reference class (bvrnn_codec_model.py:19-76) - plus the two
sub-operators the reference exposes as attributes (``model.bvrnn.encode/decode`` bvrnn.py:163-229,
``model.vocoder(x, length)`` models.py:207-238; ``coder``) and ``mel_spectrogram`` (meldataset.py:60-95).

All arithmetic runs in the gfx950 HIP library behind include/bvcodec.h; PyTorch only provides device
memory and streams.  Inference only: outputs carry no autograd graph.  Tensors that live on another
device (e.g. the CPU tensors of the reference's example.py) are moved to the model's GPU for the
call and the result is returned on the caller's device (``engine``: the one path of every library call).
"""
import os

import numpy as np
import torch
from torch import nn

from . import _abi, ragged, weights
from ._abi import ptr
from .coder import BVRNN, BigVGAN, _broadcast_target, _check_stream, _entropy_segments
from .config import DEFAULT_CONFIG, is_causal, load_config, not_causal_message, num_frames
from .engine import _Engine  # noqa: F401  (importable from here as before)
from .engine import _codes_dims, _OnDevice, _prep, _trimmed, _wave_dims, _wave_frames
from .vbr_args import _check_ladder, cap_q8

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
        eng, out_dev, x = self._enter(x)
        B, L = _wave_dims(x)
        T = _wave_frames(L, eng.num_frames)
        mel = torch.empty(B, T, self.conf["num_mels"], device=eng.device)
        eng.call("bvc_stft_logmel", eng.handle, ptr(x), B, L, float(scale), ptr(mel))
        return eng.to_caller(out_dev, mel, poll=False)

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
        eng, out_dev, x = self._enter(x)
        B, L = _wave_dims(x)
        T = _wave_frames(L, eng.num_frames)
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device)
        eng.call("bvc_encode", eng.handle, ptr(x), B, L, float(SCALING), self.bits_per_frame(bitrate), ptr(codes), scratch=(B, T))
        return eng.to_caller(out_dev, codes)

    def _encode_ragged(self, x, bitrate, lengths):
        """``encode`` of a mixed-length batch (``bvc_encode_ragged``)."""
        eng, out_dev, x = self._enter(x)
        B, L = _wave_dims(x)
        lens = ragged.per_row_ints(L if lengths is None else lengths, B, "lengths")
        if (lens > L).any():
            raise RuntimeError(f"lengths must not exceed the row length {L} (got {int(lens.max())})")
        for n in [L] + sorted(set(lens.tolist())):            # the equal-length path's check, for the row and for every utterance
            _wave_frames(int(n), eng.num_frames)
        T = eng.num_frames(L)
        rates = ragged.per_row(bitrate, B, "bitrate")
        bits = None
        if rates is not None:                                  # bits_per_frame per row, the reference's rounding in float64
            bits = torch.from_numpy(np.round(rates * self.conf['hopsize'] / self.conf['fs']).astype(np.float32)).to(eng.device)
        d_lens = torch.from_numpy(lens).to(eng.device)
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device)
        eng.call("bvc_encode_ragged", eng.handle, ptr(x), ptr(d_lens, torch.int64), B, L, float(SCALING), ptr(bits),
                 self.bits_per_frame(bitrate) if rates is None else 0.0, ptr(codes), scratch=(B, T))
        return eng.to_caller(out_dev, codes)

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
        B, L = _wave_dims(x)
        T = _wave_frames(L, lambda n: num_frames(self.conf, n))
        tau = _broadcast_target(target, B, T, "cpu")
        eng, out_dev, x = self._enter(x)
        tau = tau.to(eng.device)
        codes = torch.empty(B, T, z, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        eng.call("bvc_encode_vbr" if cap is None else "bvc_encode_vbr_capped", eng.handle, ptr(x), B, L, float(SCALING), ptr(tau), lad, K,
                 ptr(codes), ptr(bits), scratch=(B, T, K), after=cap or ())
        return eng.to_caller(out_dev, codes, *((bits,) if return_bits else ()))

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
        if lost is None and return_codes:
            raise ValueError("decode: return_codes belongs to concealment (pass lost)")
        mixed = frames is not None or ragged.per_row(length, codes.shape[0], "length") is not None
        if lost is None and mixed:
            if not is_causal(self.conf):
                raise ValueError("decode: " + not_causal_message(self.conf))
            return self._decode_ragged(codes, length, frames)
        if lost is not None:
            if mixed:
                raise ValueError("decode: lost frames in a mixed-length batch are not supported (decode the rows on their own)")
            if self.conf["var_bit"] and bitrate is None:
                raise ValueError("decode: a variable-rate model needs the bitrate to generate lost frames")
            if codes.dim() != 3 or tuple(lost.shape) != tuple(codes.shape[:2]):
                raise ValueError("decode: lost must be (batch, frames) like the codes")
        eng, out_dev, codes = self._enter(codes)
        B, T, Z = _codes_dims(codes, self.conf["z_dim"])
        n = _trimmed(eng.vocoder_length(T), length)       # `[:, :, :length]`, models.py:238
        wav = torch.empty(B, n, device=eng.device)
        filled = torch.empty(B, T, Z, device=eng.device) if return_codes else None
        if n and lost is None:                            # (length 0 keeps nothing: an empty (B, 0) tensor like the reference's)
            eng.call("bvc_decode", eng.handle, ptr(codes), B, T, n, float(SCALING), ptr(wav), scratch=(B, T))
        elif n:
            present = lost.detach().to(eng.device).eq(0).to(torch.uint8).contiguous()
            bits = self.bits_per_frame(bitrate) if self.conf["var_bit"] else float(Z)
            eng.call("bvc_decode_conceal", eng.handle, ptr(codes), ptr(present, torch.uint8), float(bits), B, T, n, float(SCALING),
                     ptr(wav), ptr(filled), scratch=(B, T))
        elif return_codes:
            raise ValueError("decode: the filled codes need a non-empty output (length > 0)")
        return eng.to_caller(out_dev, wav, *((filled,) if return_codes else ()))

    def _decode_ragged(self, codes, length, frames):
        """``decode`` of a mixed-length batch (``bvc_decode_ragged``)."""
        eng, out_dev, codes = self._enter(codes)
        B, T, Z = _codes_dims(codes, self.conf["z_dim"])
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
            eng.call("bvc_decode_ragged", eng.handle, ptr(codes), ptr(d_fr, torch.int64), B, T, ptr(d_lens, torch.int64), n_max,
                     float(SCALING), ptr(wav), scratch=(B, T))
        return eng.to_caller(out_dev, wav)

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
        eng, out_dev, x = self._enter(x)
        B, L = _wave_dims(x)
        T = _wave_frames(L, eng.num_frames)
        n = _trimmed(eng.vocoder_length(T), L)
        wav = torch.empty(B, n, device=eng.device)
        codes = torch.empty(B, T, self.conf["z_dim"], device=eng.device) if return_codes else None
        eng.call("bvc_forward", eng.handle, ptr(x), B, L, float(SCALING), self.bits_per_frame(bitrate), n, float(SCALING), ptr(codes),
                 ptr(wav), scratch=(B, T))
        return eng.to_caller(out_dev, *((codes,) if return_codes else ()), wav)

    # ---- wire format (not in the reference, which has no bit stream: SURVEY.md 8f rank 2)
    def active_bits(self, bitrate):
        z = self.conf["z_dim"]
        return z if not self.conf["var_bit"] else int(min(z, max(0.0, self.bits_per_frame(bitrate))))

    @torch.no_grad()
    def pack(self, codes, bitrate):
        """codes (B,T,z_dim) from encode(x, bitrate) -> uint8 (B,T,ceil(n/8)), n active bits per frame."""
        eng, out_dev, codes = self._enter(codes)
        B, T, Z = codes.shape
        n = self.active_bits(bitrate)
        out = torch.empty(B, T, (n + 7) // 8, dtype=torch.uint8, device=eng.device)
        if out.numel():
            eng.call("bvc_pack_codes", ptr(codes), B, T, Z, n, ptr(out, torch.uint8))
        return eng.to_caller(out_dev, out, poll=False)

    @torch.no_grad()
    def unpack(self, packed, bitrate):
        """Inverse of pack(): uint8 (B,T,ceil(n/8)) -> float32 codes (B,T,z_dim) with 0.5 in masked positions."""
        eng, out_dev = self.engine(packed), packed.device
        packed = packed.to(eng.device).contiguous()
        B, T, _ = packed.shape
        Z = self.conf["z_dim"]
        codes = torch.empty(B, T, Z, device=eng.device)
        eng.call("bvc_unpack_codes", ptr(packed, torch.uint8) if packed.numel() else None, B, T, Z, self.active_bits(bitrate), ptr(codes))
        return eng.to_caller(out_dev, codes, poll=False)

    # ---- entropy-coded wire format: the codes range-coded under the model's prior net (lossless; storage and reliable transport)
    def _frame_bits(self, who, B, T, bitrate, bits):
        """The bits of every frame of an entropy-coded call, (B, T) on the CPU, or None on a fixed-rate model: ``bits`` as encode_vbr
        returns them, or the constant of ``bitrate``."""
        if bitrate is not None and np.ndim(bitrate.detach().cpu().numpy() if hasattr(bitrate, "detach") else bitrate) != 0:
            raise ValueError(f"{who}: one bitrate for the whole batch (mixed-length and mixed-rate batches are not supported)")
        if bits is not None and bitrate is not None:
            raise ValueError(f"{who}: bitrate or bits, not both")
        if not self.conf["var_bit"]:
            return None
        if bits is None and bitrate is None:
            raise ValueError(f"{who}: a variable-rate model needs the bitrate (or bits (batch, frames)) the codes were made with")
        if bits is not None:
            if not torch.is_tensor(bits) or tuple(bits.shape) != (B, T):
                raise ValueError(f"{who}: bits must be a tensor ({B}, {T})")
            return bits
        return torch.full((B, T), float(self.active_bits(bitrate)))

    def _state(self, h0, B):
        return torch.zeros(1, B, self.conf["h_dim"]) if h0 is None else h0

    @torch.no_grad()
    def pack_entropy(self, codes, bitrate=None, bits=None, segment=None, h0=None, return_state=False):
        """codes (B,T,z_dim) from encode(x, bitrate) - or from encode_vbr, with its ``bits`` - -> (data uint8 (B, nseg, n), sizes int32
        (B, nseg)): every bit coded under the probability the prior net gives it at the decoder's own state, so a bit costs about
        -log2 p instead of one stored bit (``bvc_bvrnn_entropy_pack``).  Segment s of row b is data[b, s, :sizes[b, s]]; a segment
        holds ``segment`` frames (None: the whole call) and is decodable on its own coder, though not without the decoder state its
        first frame starts from.  n = the largest size in use.  ``h0`` (1,B,h_dim): the decoder's state in front of the first frame
        (None: zero); ``return_state=True`` adds the state behind the last.  Lossless, for storage and reliable transport: a receiver
        that misses a segment cannot decode the rest of the row.  The gain depends on the checkpoint's prior and has not been measured
        on trained weights; an untrained prior can make the stream longer than ``pack``'s."""
        if codes.dim() != 3 or codes.shape[2] != self.conf["z_dim"] or codes.shape[0] < 1 or codes.shape[1] < 1:
            raise ValueError(f"pack_entropy: codes must be (batch, frames, {self.conf['z_dim']})")
        B, T, _ = codes.shape
        fb = self._frame_bits("pack_entropy", B, T, bitrate, bits)
        data, sizes, hT = self.bvrnn.entropy_pack(codes, fb, self._state(h0, B), segment=segment)
        if bool((sizes < 0).any()):
            raise RuntimeError("pack_entropy: a segment did not fit the safe stride")      # (cannot happen: the stride is a bound)
        data = data[:, :, :int(sizes.max())].contiguous()
        return (data, sizes, hT) if return_state else (data, sizes)

    @torch.no_grad()
    def unpack_entropy(self, data, sizes, frames, bitrate=None, bits=None, segment=None, h0=None, return_mel=False):
        """Inverse of pack_entropy(): (data, sizes) of ``frames`` frames -> float32 codes (B, frames, z_dim) with 0.5 at the positions
        without a bit; same ``bitrate`` / ``bits``, ``segment`` and ``h0`` as the sender's (``bvc_bvrnn_entropy_unpack``).  The
        decoder runs its recurrence to do so: ``return_mel=True`` adds the decoded mel (B, frames, num_mels) and the state behind the
        last frame (1,B,h_dim)."""
        if not torch.is_tensor(data) or data.dim() != 3:
            raise ValueError("unpack_entropy: data must be a uint8 tensor (batch, segments, stride)")
        _entropy_segments(frames, segment, "unpack_entropy")
        fb = self._frame_bits("unpack_entropy", data.shape[0], int(frames), bitrate, bits)
        codes, mel, hT = self.bvrnn.entropy_unpack(data, sizes, frames, fb, self._state(h0, data.shape[0]), segment=segment)
        return (codes, mel, hT) if return_mel else codes

    @torch.no_grad()
    def encode_entropy(self, x, bitrate, segment=None):
        """``encode(x, bitrate)`` followed by ``pack_entropy``: waveforms (batch, samples) -> (data, sizes)."""
        return self.pack_entropy(self.encode(x, bitrate), bitrate=bitrate, segment=segment)

    @torch.no_grad()
    def decode_entropy(self, data, sizes, frames, length, bitrate=None, segment=None, return_codes=False):
        """(data, sizes) of pack_entropy / encode_entropy back to waveforms, as ``decode(unpack_entropy(...), length)`` gives them but
        with ONE recurrence (``bvc_decode_entropy``): the receive program decodes the codes and the mel in the same frame loop.
        ``return_codes=True`` returns (wav, codes)."""
        S, nseg = _entropy_segments(frames, segment, "decode_entropy")
        _check_stream(data, sizes, nseg, "decode_entropy")
        B, T, Z = data.shape[0], int(frames), self.conf["z_dim"]
        if np.ndim(length.detach().cpu().numpy() if hasattr(length, "detach") else length) != 0:
            raise ValueError("decode_entropy: one length for the whole batch (mixed-length batches are not supported)")
        self._frame_bits("decode_entropy", B, T, bitrate, None)
        eng, out_dev = self.engine(data), data.device
        data = data.to(eng.device).contiguous()
        sizes = sizes.detach().to(device=eng.device, dtype=torch.int32).contiguous()
        n = _trimmed(eng.vocoder_length(T), length)
        if not n:
            raise ValueError("decode_entropy: a non-empty output is needed (length > 0)")
        wav = torch.empty(B, n, device=eng.device)
        codes = torch.empty(B, T, Z, device=eng.device) if return_codes else None
        bpf = float(self.active_bits(bitrate)) if self.conf["var_bit"] else float(Z)
        eng.call("bvc_decode_entropy", eng.handle, ptr(data, torch.uint8) if data.numel() else None, data.shape[2], ptr(sizes, torch.int32),
                 bpf, B, T, S, n, float(SCALING), ptr(wav), ptr(codes), scratch=(B, T, "entropy"))
        return eng.to_caller(out_dev, wav, *((codes,) if return_codes else ()))

    @torch.no_grad()
    def pack_vbr(self, codes, bits):
        """codes (B,T,z_dim) and bits (B,T) from encode_vbr -> (bytes uint8 (B,T,1 + ceil(z_dim/8)), sizes int32 (B,T)): a frame is its
        bit count n, ceil(n/8) bytes of bits, zeros; sizes = 1 + ceil(n/8) are the bytes of the frame worth sending."""
        if codes.dim() != 3 or tuple(bits.shape) != tuple(codes.shape[:2]) or codes.shape[2] != self.conf["z_dim"]:
            raise ValueError("pack_vbr: codes (B, T, z_dim) with bits (B, T)")
        eng, out_dev, codes = self._enter(codes)
        bits = _prep(bits, eng.device)
        B, T, Z = codes.shape
        out = torch.empty(B, T, 1 + (Z + 7) // 8, dtype=torch.uint8, device=eng.device)
        sizes = torch.empty(B, T, dtype=torch.int32, device=eng.device)
        if sizes.numel():
            eng.call("bvc_pack_codes_vbr", ptr(codes), ptr(bits), B, T, Z, ptr(out, torch.uint8), ptr(sizes, torch.int32))
        return eng.to_caller(out_dev, out, sizes, poll=False)

    @torch.no_grad()
    def unpack_vbr(self, packed):
        """Inverse of pack_vbr(): uint8 (B,T,1 + ceil(z_dim/8)) -> (codes (B,T,z_dim) with 0.5 behind each frame's bits, bits (B,T))."""
        Z = self.conf["z_dim"]
        if packed.dim() != 3 or packed.shape[2] != 1 + (Z + 7) // 8 or packed.dtype != torch.uint8:
            raise ValueError(f"unpack_vbr: uint8 (B, T, {1 + (Z + 7) // 8}) expected")
        eng, out_dev = self.engine(packed), packed.device
        packed = packed.to(eng.device).contiguous()
        B, T, _ = packed.shape
        codes = torch.empty(B, T, Z, device=eng.device)
        bits = torch.empty(B, T, device=eng.device)
        if bits.numel():
            eng.call("bvc_unpack_codes_vbr", ptr(packed, torch.uint8), B, T, Z, ptr(codes), ptr(bits))
        return eng.to_caller(out_dev, codes, bits, poll=False)
