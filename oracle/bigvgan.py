"""Oracle: BigVGAN generator forward (test infrastructure, see __init__).

Follows ``BigVGAN.forward`` third_party/BigVGAN/models.py:207-238 (ctor :132-205),
``AMPBlock1.forward`` models.py:103-121 (paddings :35-44, ``get_padding_causal`` :19-20,
``utils.get_padding``), ``SnakeBeta.forward`` third_party/BigVGAN/activations.py:107-120 with
``alpha_logscale=True``, ``Activation1d`` third_party/BigVGAN/alias_free_torch/act.py:8-28 and
old-style ``weight_norm`` (``weight_g``/``weight_v``, norm over every dim but 0;
models.py:47-62,140,164,200).  Every configuration the product loads is covered: resblock "1",
snakebeta, any ``upsample_initial_channel``, and any mix of causal, symmetric and anti-aliased stages.

Symmetric layers (``layers_sym`` / ``pre_sym`` / ``post_sym`` of the ``vocoder_config`` table; no switch adds a checkpoint key):
    pre_sym         conv_pre is padded [3, 3] instead of [6, 0]                                              :209-213
    layers_sym[i]   upsampler i is ConvTranspose1d(padding = (k - u) // 2): with k = 2u, rows [u/2, u/2 + L u) of the causal
                    result, L u rows instead of (L + 1) u                                                    :151-155,164-167
                    the stage's AMP blocks pad conv1 (ks-1) d / 2 and conv2 (ks-1) / 2 on BOTH sides, after the activations
                    (utils.get_padding): out[t] of one iteration reads x[t - h .. t + h], h = (ks-1)(d+1)/2   :35-44,106-119
    post_sym        conv_post is padded [3, 3]                                                               :230-233

Anti-aliased activations (``layers_antialias`` / ``antialias_post``).  ``Activation1d`` wraps a SnakeBeta S on a signal x (B, C, L),
with the two 12-tap filters f (``upsample.filter``) and g (``downsample.lowpass.filter``) of the checkpoint:
    up  = 2 * conv_transpose1d(replicate_pad(x, 5, 5), f, stride 2)[15:-15]          resample.py:10-33   -> 2L samples
    a   = S(up)                                                                      act.py:25
    y   = conv1d(replicate_pad(a, 5, 6), g, stride 2)                                filter.py:86-95, resample.py:36-49 -> L samples
i.e. up[2t] = 2 sum_k f[2k+1] x[c(t+2-k)], up[2t+1] = 2 sum_k f[2k] x[c(t+3-k)] (k = 0..5, c = clamp to [0, L-1]) and
y[t] = sum_j g[j] a[clamp(2t-5+j, 0, 2L-1)]: two clamps, and y[t] reads x[t-5 .. t+5].
State-dict keys of activation K: ``...activations.K.act.alpha / .act.beta / .upsample.filter / .downsample.lowpass.filter``
(a plain one: ``...activations.K.alpha / .beta``); which layout a stage has is read from the keys.

``fold``: how weight_g / weight_v become the weight.  The default is ``fold_weight_norm`` (any dtype: the float64 truth).  It
rounds v * (g / ||v||) where the reference's forward pre-hook, ``torch._weight_norm``, rounds v * g / ||v||: weights that differ in
the last bit (3.7e-9 on conv_pre), outputs 8e-7 apart.  ``REFERENCE_FOLD`` is the hook's function; with it the float32 oracle gives
the reference's bits (tests/test_antialias_cpu.py, test_symmetric_cpu.py, test_wide_generator_cpu.py).
"""
import torch
import torch.nn.functional as F

REACH = 5            # y[t] of one Activation1d reads x[t - 5 .. t + 5]


def fold_weight_norm(g, v):
    """w = g * v / ||v||, norm over all dims except 0 (torch._weight_norm, dim=0)."""
    norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v.dim() - 1))
    return v * (g / norm)


def REFERENCE_FOLD(g, v):
    return torch._weight_norm(v, g, 0)


def snakebeta(x, alpha, beta):
    a = torch.exp(alpha)[None, :, None]                      # activations.py:111-115
    b = torch.exp(beta)[None, :, None]
    return x + (1.0 / (b + 0.000000001)) * torch.pow(torch.sin(x * a), 2)   # :116


def activation1d(x, alpha, beta, f_up, f_down):
    """x (B, C, L); alpha, beta (C,); f_up, f_down (1, 1, 12), all of x's dtype."""
    C = x.shape[1]
    up = F.pad(x, (5, 5), mode="replicate")                                          # resample.py:27
    up = 2 * F.conv_transpose1d(up, f_up.expand(C, -1, -1), stride=2, groups=C)      # :28-29
    up = up[..., 15:-15]                                                             # :30
    a = snakebeta(up, alpha, beta)                                                   # act.py:25
    a = F.pad(a, (5, 6), mode="replicate")                                           # filter.py:89-90
    return F.conv1d(a, f_down.expand(C, -1, -1), stride=2, groups=C)                 # :91-92


def is_filtered(sd, name):
    return f"{name}.act.alpha" in sd


def activation(sd, name, x, dtype):
    """Activation ``name`` of the state dict on x: Activation1d where the checkpoint carries its keys, a plain SnakeBeta else."""
    if not is_filtered(sd, name):
        return snakebeta(x, sd[f"{name}.alpha"].to(dtype), sd[f"{name}.beta"].to(dtype))
    return activation1d(x, sd[f"{name}.act.alpha"].to(dtype), sd[f"{name}.act.beta"].to(dtype),
                        sd[f"{name}.upsample.filter"].to(dtype), sd[f"{name}.downsample.lowpass.filter"].to(dtype))


def _conv(sd, name, dtype):
    return [sd[f"{name}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias")]


def amp_pair(sd, pre, m, x, ksize, d, dtype=torch.float32, fold=fold_weight_norm, sym=False):
    """One iteration of AMPBlock1.forward, models.py:106-119: x + conv2(S2(conv1_dil(S1(x)))), x (B, C, L).
    ``m``: index of the iteration (its convs and activations), ``d``: its dilation.  The zero paddings follow the activations."""
    x = torch.as_tensor(x).to(dtype)
    g1, v1, b1 = _conv(sd, f"{pre}.convs1.{m}", dtype)
    g2, v2, b2 = _conv(sd, f"{pre}.convs2.{m}", dtype)
    p1, p2 = ksize * d - d, ksize - 1
    xt = activation(sd, f"{pre}.activations.{2 * m}", x, dtype)
    xt = F.pad(xt, (p1 // 2, p1 // 2) if sym else (p1, 0))
    xt = F.conv1d(xt, fold(g1, v1), b1, dilation=d)
    xt = activation(sd, f"{pre}.activations.{2 * m + 1}", xt, dtype)
    xt = F.pad(xt, (p2 // 2, p2 // 2) if sym else (p2, 0))
    xt = F.conv1d(xt, fold(g2, v2), b2)
    return xt + x


def amp_block(sd, pre, x, ksize, dilations=(1, 3, 5), fold=fold_weight_norm, sym=False):
    """AMPBlock1.forward, models.py:103-121."""
    for m, d in enumerate(dilations):
        x = amp_pair(sd, pre, m, x, ksize, d, x.dtype, fold, sym)
    return x


def conv_pre(sd, mel, dtype=torch.float32, fold=fold_weight_norm, sym=False):
    """mel (B, num_mels, T) -> (B, upsample_initial_channel, T), models.py:209-213."""
    g, v, b = _conv(sd, "conv_pre", dtype)
    x = F.pad(torch.as_tensor(mel).to(dtype), [3, 3] if sym else [6, 0])             # models.py:212
    return F.conv1d(x, fold(g, v), b)                                                # :213


def upsample(sd, cfg, i, x, dtype=torch.float32, fold=fold_weight_norm, sym=False):
    """Upsampler i, models.py:151-167,216-217: (B, Cin, L) -> (B, Cin / 2, (L + 1) * rate) (kernel = 2 * rate, no padding), or
    L * rate where it is symmetric."""
    g, v, b = _conv(sd, f"ups.{i}.1", dtype)
    u = cfg["upsample_rates"][i]
    return F.conv_transpose1d(torch.as_tensor(x).to(dtype), fold(g, v), b, stride=u,
                              padding=(cfg["upsample_kernel_sizes"][i] - u) // 2 if sym else 0)


def conv_post(sd, x, length, dtype=torch.float32, fold=fold_weight_norm, sym=False):
    """activation_post -> pad [6, 0] (or [3, 3]) -> conv_post -> tanh -> [:length], models.py:228-238: (B, C, L) -> (B, 1, min(length, L))."""
    x = torch.as_tensor(x).to(dtype)
    g, v, b = _conv(sd, "conv_post", dtype)
    x = activation(sd, "activation_post", x, dtype)                  # :228
    x = F.pad(x, [3, 3] if sym else [6, 0])                          # :233
    x = F.conv1d(x, fold(g, v), b)                                   # :235
    x = torch.tanh(x)                                                # :236
    return x[:, :, :length]                                          # :238


def flags(cfg):
    """(layers_sym, pre_sym, post_sym) of a ``vocoder_config`` table."""
    n = len(cfg["upsample_rates"])
    return [bool(f) for f in cfg.get("layers_sym", [False] * n)], bool(cfg.get("pre_sym", False)), bool(cfg.get("post_sym", False))


@torch.no_grad()
def forward(sd, cfg, mel, length, dtype=torch.float32, taps=None, fold=fold_weight_norm):
    """mel (B, num_mels, T) -> (B, 1, min(length, generator length of T)): 256T+294 samples from a causal generator.

    ``cfg``: the ``vocoder_config`` table of the TOML; its symmetric switches are read here, the filtered stages from the state
    dict's keys.  ``taps``: optional dict that is filled with the intermediate tensors (conv_pre, up{i}, stage{i}) for bisecting.
    """
    sd = {k: v.to(dtype) for k, v in sd.items()}
    rates = cfg["upsample_rates"]
    rks, rds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(rks)
    stages, pre, post = flags(cfg)
    x = conv_pre(sd, mel, dtype, fold, pre)
    if taps is not None:
        taps["conv_pre"] = x
    for i in range(len(rates)):                                      # :214
        x = upsample(sd, cfg, i, x, dtype, fold, stages[i])
        if taps is not None:
            taps[f"up{i}"] = x
        xs = None
        for j in range(nk):                                          # :219-224
            r = amp_block(sd, f"resblocks.{i * nk + j}", x, rks[j], tuple(rds[j]), fold, stages[i])
            xs = r if xs is None else xs + r
        x = xs / nk                                                  # :225
        if taps is not None:
            taps[f"stage{i}"] = x
    return conv_post(sd, x, length, dtype, fold, post)
