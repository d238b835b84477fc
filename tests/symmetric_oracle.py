"""The generator with symmetric layers (``layers_sym`` / ``pre_sym`` / ``post_sym``), in any mix with causal and filtered stages,
composed from the CPU oracle's pieces (oracle/bigvgan.py, tests/antialias_oracle.py); test infrastructure, float32 or float64.

What the switches do (third_party/BigVGAN/models.py):
    pre_sym         conv_pre is padded [3, 3] instead of [6, 0]                                              :209-213
    layers_sym[i]   upsampler i is ConvTranspose1d(padding = (k - u) // 2): with k = 2u, rows [u/2, u/2 + L u) of the causal
                    result, L u rows instead of (L + 1) u                                                    :151-155,164-167
                    the stage's AMP blocks pad conv1 (ks-1) d / 2 and conv2 (ks-1) / 2 on BOTH sides, after the activations
                    (utils.get_padding): out[t] of one iteration reads x[t - h .. t + h], h = (ks-1)(d+1)/2   :35-44,106-119
    post_sym        conv_post is padded [3, 3]                                                               :230-233
No switch adds a checkpoint key.  ``fold``: see antialias_oracle (``REFERENCE_FOLD`` gives the reference's bits).
"""
import torch
import torch.nn.functional as F

import antialias_oracle as aao

FOLD = aao.FOLD
REFERENCE_FOLD = aao.REFERENCE_FOLD


def reach(ks, d):
    """A symmetric pair's out[t] reads x[t - reach .. t + reach] (test_symmetric_cpu.py measures it)."""
    return (ks - 1) * (d + 1) // 2


def amp_pair(sd, pre, m, x, ksize, d, dtype=torch.float32, fold=FOLD, sym=True):
    """One iteration of AMPBlock1.forward, models.py:106-119, x (B, C, L); the zero paddings follow the activations."""
    x = torch.as_tensor(x).to(dtype)
    g1, v1, b1 = (sd[f"{pre}.convs1.{m}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    g2, v2, b2 = (sd[f"{pre}.convs2.{m}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    p1, p2 = ksize * d - d, ksize - 1
    xt = aao.activation(sd, f"{pre}.activations.{2 * m}", x, dtype)
    xt = F.pad(xt, (p1 // 2, p1 // 2) if sym else (p1, 0))
    xt = F.conv1d(xt, fold(g1, v1), b1, dilation=d)
    xt = aao.activation(sd, f"{pre}.activations.{2 * m + 1}", xt, dtype)
    xt = F.pad(xt, (p2 // 2, p2 // 2) if sym else (p2, 0))
    xt = F.conv1d(xt, fold(g2, v2), b2)
    return xt + x


def conv_pre(sd, mel, dtype=torch.float32, fold=FOLD, sym=True):
    """mel (B, num_mels, T) -> (B, upsample_initial_channel, T), models.py:209-213."""
    g, v, b = (sd[f"conv_pre.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    return F.conv1d(F.pad(torch.as_tensor(mel).to(dtype), [3, 3] if sym else [6, 0]), fold(g, v), b)


def upsample(sd, cfg, i, x, dtype=torch.float32, fold=FOLD, sym=True):
    """Upsampler i, models.py:151-167,216-217: (B, Cin, L) -> (B, Cin / 2, L * rate), or (L + 1) * rate without padding."""
    g, v, b = (sd[f"ups.{i}.1.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    u, k = cfg["upsample_rates"][i], cfg["upsample_kernel_sizes"][i]
    return F.conv_transpose1d(torch.as_tensor(x).to(dtype), fold(g, v), b, stride=u, padding=(k - u) // 2 if sym else 0)


def conv_post(sd, x, length, dtype=torch.float32, fold=FOLD, sym=True):
    """activation_post -> pad [3, 3] (or [6, 0]) -> conv_post -> tanh -> [:length], models.py:228-238."""
    x = torch.as_tensor(x).to(dtype)
    g, v, b = (sd[f"conv_post.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    x = aao.activation(sd, "activation_post", x, dtype)
    x = F.pad(x, [3, 3] if sym else [6, 0])
    x = torch.tanh(F.conv1d(x, fold(g, v), b))
    return x[:, :, :length]


def flags(cfg):
    """(layers_sym, pre_sym, post_sym) of a ``vocoder_config`` table."""
    n = len(cfg["upsample_rates"])
    return [bool(f) for f in cfg.get("layers_sym", [False] * n)], bool(cfg.get("pre_sym", False)), bool(cfg.get("post_sym", False))


@torch.no_grad()
def forward(sd, cfg, mel, length, dtype=torch.float32, taps=None, fold=FOLD):
    """BigVGAN.forward (models.py:207-238) for any mix of causal, symmetric and filtered stages (the filtered ones are read from the
    state dict's keys); ``taps``: conv_pre, up{i}, stage{i}."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    rks, rds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(rks)
    stages, pre, post = flags(cfg)
    x = conv_pre(sd, mel, dtype, fold, pre)
    if taps is not None:
        taps["conv_pre"] = x
    for i in range(len(cfg["upsample_rates"])):
        x = upsample(sd, cfg, i, x, dtype, fold, stages[i])
        if taps is not None:
            taps[f"up{i}"] = x
        xs = None
        for j in range(nk):
            r = x
            for m, d in enumerate(rds[j]):
                r = amp_pair(sd, f"resblocks.{i * nk + j}", m, r, rks[j], d, dtype, fold, stages[i])
            xs = r if xs is None else xs + r
        x = xs / nk
        if taps is not None:
            taps[f"stage{i}"] = x
    return conv_post(sd, x, length, dtype, fold, post)


def _c(layers_sym, pre_sym, post_sym, layers_antialias=(False,) * 4, antialias_post=False):
    return dict(layers_sym=list(layers_sym), pre_sym=pre_sym, post_sym=post_sym, layers_antialias=list(layers_antialias),
                antialias_post=antialias_post)


T_, F_ = True, False
CONFIGS = {
    "all": _c([T_, T_, T_, T_], True, True),
    # symmetric C = 32 and C = 8 stages around the causal persistent C = 16 kernel
    "mixed": _c([F_, T_, F_, T_], False, True),
    "with_aa": _c([T_, F_, T_, F_], True, False, [F_, T_, F_, T_], True),
}


def with_switches(conf, tag_or_dict):
    """A copy of the configuration with the five switches of one of CONFIGS (or of a dict like them) set."""
    sw = CONFIGS[tag_or_dict] if isinstance(tag_or_dict, str) else tag_or_dict
    c = dict(conf)
    c["vocoder_config"] = dict(conf["vocoder_config"], **{k: (list(v) if isinstance(v, (list, tuple)) else bool(v)) for k, v in sw.items()})
    return c


def sym_lengths(cfg, T):
    """Rows after every stage: L * u behind a symmetric upsampler, (L + 1) * u behind a causal one; the last is the waveform's."""
    out, L = [], T
    for u, s in zip(cfg["upsample_rates"], flags(cfg)[0]):
        L = L * u if s else (L + 1) * u
        out.append(L)
    return out


# ---------------------------------------------------------------------------------------------- shared by the two test files
def write_config(path, tag, h_dim=None):
    """The shipped variable-rate TOML with the switches of CONFIGS[tag] set (and, for cheap models, another h_dim); returns the
    loaded config."""
    from bvcodec import config
    sw = CONFIGS[tag]
    txt = open(config.DEFAULT_CONFIG).read()
    for key, value in sw.items():
        off = "[false, false, false, false]" if isinstance(value, list) else "false"
        old = f"{key} = {off}"
        assert txt.count(old) == 1, key
        new = "[" + ", ".join("true" if f else "false" for f in value) + "]" if isinstance(value, list) else ("true" if value else "false")
        txt = txt.replace(old, f"{key} = {new}")
    if h_dim is not None:
        assert "h_dim = 1024" in txt
        txt = txt.replace("h_dim = 1024", f"h_dim = {h_dim}")
    with open(path, "w") as f:
        f.write(txt)
    return config.load_config(path)


SYM_TILE_HEIGHT = {64: 128, 32: 256, 16: 128, 8: 256}     # launch_amp_pair's tile (rows both convs sweep) of a symmetric stage


def sym_tile_rows(C, ks):
    """Valid output rows per tile: conv2 spends ks - 1 of the tile's rows, (ks-1)/2 on each side."""
    return SYM_TILE_HEIGHT[C] - (ks - 1)


def amp_lengths(TT, ks, d):
    """Rows per item: signals shorter than the reach on both sides at once, both sides of every seam, the last tile's end anywhere."""
    p2, h = (ks - 1) // 2, reach(ks, d)
    return sorted({1, 2, p2, p2 + 1, h, h + 1, 2 * h + 1, TT - 1, TT, TT + 1, 2 * TT + 1, 3 * TT + 17})
