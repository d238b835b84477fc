"""Oracle: causal-tiny BigVGAN generator forward (test infrastructure, see __init__).

Follows ``BigVGAN.forward`` third_party/BigVGAN/models.py:207-238 (ctor :132-205),
``AMPBlock1.forward`` models.py:103-121 (causal paddings :41-44, ``get_padding_causal``
:19-20), ``SnakeBeta.forward`` third_party/BigVGAN/activations.py:107-120 with
``alpha_logscale=True``, and old-style ``weight_norm`` (``weight_g``/``weight_v``,
norm over every dim but 0; models.py:47-62,140,164,200).  Only the configuration the two
shipped TOMLs select is covered: resblock "1", snakebeta, no anti-aliasing, all layers
causal (configs/config_varBitRate.toml:39-56).
"""
import torch
import torch.nn.functional as F


def fold_weight_norm(g, v):
    """w = g * v / ||v||, norm over all dims except 0 (torch._weight_norm, dim=0)."""
    norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v.dim() - 1))
    return v * (g / norm)


def snakebeta(x, alpha, beta):
    a = torch.exp(alpha)[None, :, None]                      # activations.py:111-115
    b = torch.exp(beta)[None, :, None]
    return x + (1.0 / (b + 0.000000001)) * torch.pow(torch.sin(x * a), 2)   # :116


def _cast(sd, names, dtype):
    return [sd[n].to(dtype) for n in names]


def amp_pair(sd, pre, m, x, ksize, d, dtype=torch.float32):
    """One iteration of AMPBlock1.forward, models.py:106-119: x + conv2(S2(conv1_dil(S1(x)))), x (B, C, L).
    ``m``: index of the iteration (its convs and activations), ``d``: its dilation."""
    x = torch.as_tensor(x).to(dtype)
    a1 = _cast(sd, (f"{pre}.activations.{2 * m}.alpha", f"{pre}.activations.{2 * m}.beta"), dtype)
    a2 = _cast(sd, (f"{pre}.activations.{2 * m + 1}.alpha", f"{pre}.activations.{2 * m + 1}.beta"), dtype)
    g1, v1, b1 = _cast(sd, [f"{pre}.convs1.{m}.{k}" for k in ("weight_g", "weight_v", "bias")], dtype)
    g2, v2, b2 = _cast(sd, [f"{pre}.convs2.{m}.{k}" for k in ("weight_g", "weight_v", "bias")], dtype)
    xt = snakebeta(x, *a1)
    xt = F.pad(xt, (ksize * d - d, 0))
    xt = F.conv1d(xt, fold_weight_norm(g1, v1), b1, dilation=d)
    xt = snakebeta(xt, *a2)
    xt = F.pad(xt, (ksize - 1, 0))
    xt = F.conv1d(xt, fold_weight_norm(g2, v2), b2)
    return xt + x


def amp_block(sd, pre, x, ksize, dilations=(1, 3, 5)):
    """AMPBlock1.forward, models.py:103-121 (symmetric=False)."""
    for m, d in enumerate(dilations):
        x = amp_pair(sd, pre, m, x, ksize, d, dtype=x.dtype)
    return x


def conv_pre(sd, mel, dtype=torch.float32):
    """mel (B, num_mels, T) -> (B, upsample_initial_channel, T), models.py:212-213."""
    x = torch.as_tensor(mel).to(dtype)
    g, v, b = _cast(sd, ("conv_pre.weight_g", "conv_pre.weight_v", "conv_pre.bias"), dtype)
    x = F.pad(x, [6, 0])                                             # models.py:212
    return F.conv1d(x, fold_weight_norm(g, v), b)                    # :213


def upsample(sd, cfg, i, x, dtype=torch.float32):
    """Upsampler i, models.py:216-217: (B, Cin, L) -> (B, Cin / 2, (L + 1) * rate) (kernel = 2 * rate, no padding)."""
    x = torch.as_tensor(x).to(dtype)
    g, v, b = _cast(sd, [f"ups.{i}.1.{k}" for k in ("weight_g", "weight_v", "bias")], dtype)
    return F.conv_transpose1d(x, fold_weight_norm(g, v), b, stride=cfg["upsample_rates"][i], padding=0)


def conv_post(sd, x, length, dtype=torch.float32):
    """activation_post -> conv_post -> tanh -> [:length], models.py:228-238: (B, C, L) -> (B, 1, min(length, L))."""
    x = torch.as_tensor(x).to(dtype)
    al, be = _cast(sd, ("activation_post.alpha", "activation_post.beta"), dtype)
    g, v, b = _cast(sd, ("conv_post.weight_g", "conv_post.weight_v", "conv_post.bias"), dtype)
    x = snakebeta(x, al, be)                                         # :228
    x = F.pad(x, [6, 0])                                             # :233
    x = F.conv1d(x, fold_weight_norm(g, v), b)                       # :235
    x = torch.tanh(x)                                                # :236
    return x[:, :, :length]                                          # :238


@torch.no_grad()
def forward(sd, cfg, mel, length, dtype=torch.float32, taps=None):
    """mel (B, num_mels, T) -> (B, 1, min(length, 256T+294)).

    ``cfg``: the ``vocoder_config`` table of the TOML.  ``taps``: optional dict that is
    filled with the intermediate tensors (conv_pre, up{i}, stage{i}) for bisecting.
    """
    sd = {k: v.to(dtype) for k, v in sd.items()}
    rates = cfg["upsample_rates"]
    rks, rds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(rks)
    x = conv_pre(sd, mel, dtype)
    if taps is not None:
        taps["conv_pre"] = x
    for i in range(len(rates)):                                      # :214
        x = upsample(sd, cfg, i, x, dtype)
        if taps is not None:
            taps[f"up{i}"] = x
        xs = None
        for j in range(nk):                                          # :219-224
            r = amp_block(sd, f"resblocks.{i * nk + j}", x, rks[j], tuple(rds[j]))
            xs = r if xs is None else xs + r
        x = xs / nk                                                  # :225
        if taps is not None:
            taps[f"stage{i}"] = x
    return conv_post(sd, x, length, dtype)
