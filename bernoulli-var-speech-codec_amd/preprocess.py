"""GPU pre-processing of the reference's example script (example.py:12-17): first channel, rational-rate
polyphase resampling to 22.05 kHz (``scipy.signal.resample_poly(speech, 22050, fs)``) and peak
normalisation (``speech / np.max(np.abs(speech))``).  SURVEY.md 8(f) rank 3.

The low-pass design restates scipy's defaults (``firwin(2*10*max(up,down)+1, 1/max(up,down),
window=('kaiser', 5.0))``, unit DC gain, scaled by ``up``, zero-padded so the output is centred) in numpy
float64; the filtering itself (upfirdn + slicing) runs in ``bvc_resample_poly`` on the GPU.
"""
import functools
import math

import numpy as np
import torch

from . import _abi


# numpy.i0 on [0, 8]: Clenshaw's recurrence over the Chebyshev coefficients of Cephes' i0, in numpy's order (csrc/resampler.hip: I0A)
_I0A = (
    -4.4153416464793395e-18, 3.3307945188222384e-17, -2.431279846547955e-16, 1.715391285555133e-15, -1.1685332877993451e-14,
    7.676185498604936e-14, -4.856446783111929e-13, 2.95505266312964e-12, -1.726826291441556e-11, 9.675809035373237e-11,
    -5.189795601635263e-10, 2.6598237246823866e-09, -1.300025009986248e-08, 6.046995022541919e-08, -2.670793853940612e-07,
    1.1173875391201037e-06, -4.4167383584587505e-06, 1.6448448070728896e-05, -5.754195010082104e-05, 0.00018850288509584165,
    -0.0005763755745385824, 0.0016394756169413357, -0.004324309995050576, 0.010546460394594998, -0.02373741480589947,
    0.04930528423967071, -0.09490109704804764, 0.17162090152220877, -0.3046826723431984, 0.6767952744094761)
# exp and sin of the C library, element by element.  numpy's own are vector kernels on some hosts (AVX-512: np.exp is a unit in the
# last place off the C library's on a few per cent of the window's arguments), so taps made with them depend on the host that designs
# them and are not the ones bvc_resampler_taps designs; with these the design is the same everywhere, and the library's bit for bit.
_exp = np.frompyfunc(math.exp, 1, 1)
_sin = np.frompyfunc(math.sin, 1, 1)


def _i0_small(x):
    """numpy.i0(x) for 0 <= x <= 8, operation for operation, with the C library's exp."""
    x = np.asarray(x, dtype=np.float64)
    y = x / 2.0 - 2.0
    b0, b1, b2 = np.full_like(y, _I0A[0]), np.zeros_like(y), np.zeros_like(y)
    for a in _I0A[1:]:
        b2, b1 = b1, b0
        b0 = y * b1 - b2 + a
    return np.asarray(_exp(x)).astype(np.float64) * (0.5 * (b0 - b2))


@functools.lru_cache(maxsize=16)
def _kaiser_lowpass(numtaps, cutoff, beta):
    """kaiser_lowpass's taps, kept per design (a 20 ms hop's resampler is designed again at every call of resample_poly); read-only."""
    alpha = (numtaps - 1) / 2.0
    m = np.arange(numtaps, dtype=np.float64) - alpha
    cm = cutoff * m
    y = np.pi * np.where(cm == 0.0, 1.0e-20, cm)
    q = m / alpha
    kaiser = _i0_small(np.abs(beta * np.sqrt(1.0 - q * q))) / _i0_small(beta)
    h = cutoff * (_sin(y).astype(np.float64) / y) * kaiser
    h = h / h.sum()                          # unit gain at DC
    h.setflags(write=False)
    return h


def kaiser_lowpass(numtaps, cutoff, beta=5.0):
    """scipy.signal.firwin(numtaps, cutoff, window=('kaiser', beta)) for a low-pass (cutoff rel. to Nyquist): numpy's sinc and kaiser
    restated operation for operation, so that the C library's exp and sin are the ones called (design_taps in csrc/resampler.hip
    is the same statement)."""
    if not 0.0 <= beta <= 8.0:
        raise ValueError("kaiser_lowpass: beta outside [0, 8]")
    if numtaps == 1:
        return np.ones(1)
    return _kaiser_lowpass(int(numtaps), float(cutoff), float(beta)).copy()


def design(up, down):
    """-> (up, down, h_padded float64, n_pre_remove) exactly as scipy.signal.resample_poly arranges them."""
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = kaiser_lowpass(2 * half_len + 1, 1.0 / max_rate) * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return up, down, np.concatenate([np.zeros(n_pre_pad), h]), n_pre_remove


def resample_poly(x, up, down):
    """x (B, L) float tensor on the GPU -> (B, ceil(L*up/down)) float32."""
    if x.device.type != "cuda":
        raise RuntimeError("bvcodec.preprocess runs on the GPU only")
    up, down, h, n_pre_remove = design(up, down)
    x = x.detach().to(torch.float32).contiguous()
    if up == down == 1:
        return x.clone()
    B, L = x.shape
    n_out = (L * up + down - 1) // down
    # the filter tail must cover every kept output (scipy's n_post_pad loop)
    need = (n_out + n_pre_remove - 1) * down - (L - 1) * up + 1
    if need > len(h):
        h = np.concatenate([h, np.zeros(need - len(h))])
    hd = torch.from_numpy(h).to(x.device)
    y = torch.empty(B, n_out, device=x.device)
    lib = _abi.load()
    with torch.cuda.device(x.device):
        _abi.check(lib.bvc_resample_poly(_abi.ptr(x), B, L, _abi.ptr(hd, torch.float64), len(h), up, down,
                                         n_pre_remove, _abi.ptr(y), n_out, _abi.current_stream(x.device)))
    return y


def peak_normalize(x):
    """x (B, L) -> x / max|x| per utterance (new tensor); a row of zeros stays zeros.  The peak is taken with ``fmaxf``, which
    drops a NaN: a row that holds one is divided by its largest finite magnitude, and the NaN stays where it was."""
    y = x.detach().to(torch.float32).contiguous().clone()
    lib = _abi.load()
    with torch.cuda.device(y.device):
        _abi.check(lib.bvc_peak_normalize(_abi.ptr(y), y.shape[0], y.shape[1], _abi.current_stream(y.device)))
    return y


def prepare_speech(x, fs_in, fs_out=22050):
    """example.py:12-17 for a batch: resample fs_in -> fs_out and peak-normalise."""
    return peak_normalize(resample_poly(x, fs_out, fs_in))
