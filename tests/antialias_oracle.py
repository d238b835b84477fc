"""The generator with anti-aliased activations (``layers_antialias`` / ``antialias_post``) composed from the CPU oracle's own
pieces (oracle/bigvgan.py: ``snakebeta``, ``fold_weight_norm``); test infrastructure, float32 or float64.

``Activation1d`` (third_party/BigVGAN/alias_free_torch/act.py:8-28) wraps a SnakeBeta S on a signal x (B, C, L), with the two
12-tap filters f (``upsample.filter``) and g (``downsample.lowpass.filter``) of the checkpoint:
    up  = 2 * conv_transpose1d(replicate_pad(x, 5, 5), f, stride 2)[15:-15]          resample.py:10-33   -> 2L samples
    a   = S(up)                                                                      act.py:25
    y   = conv1d(replicate_pad(a, 5, 6), g, stride 2)                                filter.py:86-95, resample.py:36-49 -> L samples
i.e. up[2t] = 2 sum_k f[2k+1] x[c(t+2-k)], up[2t+1] = 2 sum_k f[2k] x[c(t+3-k)] (k = 0..5, c = clamp to [0, L-1]) and
y[t] = sum_j g[j] a[clamp(2t-5+j, 0, 2L-1)]: two clamps, and y[t] reads x[t-5 .. t+5].

State-dict keys of activation K: ``...activations.K.act.alpha / .act.beta / .upsample.filter / .downsample.lowpass.filter``
(a plain one: ``...activations.K.alpha / .beta``); which layout a stage has is read from the keys.

``fold``: how weight_g / weight_v become the weight.  The default is the oracle's ``fold_weight_norm`` (any dtype: the float64
truth).  It rounds v * (g / ||v||) where the reference's forward pre-hook, ``torch._weight_norm``, rounds v * g / ||v||: weights
that differ in the last bit (3.7e-9 on conv_pre), outputs 8e-7 apart.  ``REFERENCE_FOLD`` is the hook's function; with it the float32
oracle gives the reference's bits (tests/test_antialias_cpu.py).
"""
import torch
import torch.nn.functional as F

from oracle import bigvgan as obig

FOLD = obig.fold_weight_norm


def REFERENCE_FOLD(g, v):
    return torch._weight_norm(v, g, 0)


REACH = 5            # y[t] of one Activation1d reads x[t - 5 .. t + 5]


def activation1d(x, alpha, beta, f_up, f_down):
    """x (B, C, L); alpha, beta (C,); f_up, f_down (1, 1, 12), all of x's dtype."""
    C = x.shape[1]
    up = F.pad(x, (5, 5), mode="replicate")                                          # resample.py:27
    up = 2 * F.conv_transpose1d(up, f_up.expand(C, -1, -1), stride=2, groups=C)      # :28-29
    up = up[..., 15:-15]                                                             # :30
    a = obig.snakebeta(up, alpha, beta)                                              # act.py:25
    a = F.pad(a, (5, 6), mode="replicate")                                           # filter.py:89-90
    return F.conv1d(a, f_down.expand(C, -1, -1), stride=2, groups=C)                 # :91-92


def is_filtered(sd, name):
    return f"{name}.act.alpha" in sd


def activation(sd, name, x, dtype):
    """Activation ``name`` of the state dict on x: Activation1d where the checkpoint carries its keys, a plain SnakeBeta else."""
    if not is_filtered(sd, name):
        return obig.snakebeta(x, sd[f"{name}.alpha"].to(dtype), sd[f"{name}.beta"].to(dtype))
    return activation1d(x, sd[f"{name}.act.alpha"].to(dtype), sd[f"{name}.act.beta"].to(dtype),
                        sd[f"{name}.upsample.filter"].to(dtype), sd[f"{name}.downsample.lowpass.filter"].to(dtype))


def amp_pair(sd, pre, m, x, ksize, d, dtype=torch.float32, fold=FOLD):
    """One iteration of AMPBlock1.forward, models.py:106-119, x (B, C, L): the causal zero paddings follow the activations."""
    x = torch.as_tensor(x).to(dtype)
    g1, v1, b1 = (sd[f"{pre}.convs1.{m}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    g2, v2, b2 = (sd[f"{pre}.convs2.{m}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    xt = activation(sd, f"{pre}.activations.{2 * m}", x, dtype)
    xt = F.pad(xt, (ksize * d - d, 0))
    xt = F.conv1d(xt, fold(g1, v1), b1, dilation=d)
    xt = activation(sd, f"{pre}.activations.{2 * m + 1}", xt, dtype)
    xt = F.pad(xt, (ksize - 1, 0))
    xt = F.conv1d(xt, fold(g2, v2), b2)
    return xt + x


def conv_post(sd, x, length, dtype=torch.float32, fold=FOLD):
    """activation_post -> pad [6, 0] -> conv_post -> tanh -> [:length], models.py:228-238."""
    x = torch.as_tensor(x).to(dtype)
    g, v, b = (sd[f"conv_post.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    x = activation(sd, "activation_post", x, dtype)
    x = F.pad(x, [6, 0])
    x = torch.tanh(F.conv1d(x, fold(g, v), b))
    return x[:, :, :length]


@torch.no_grad()
def forward(sd, cfg, mel, length, dtype=torch.float32, taps=None, fold=FOLD):
    """BigVGAN.forward (models.py:207-238) for any mix of filtered and plain stages; ``taps``: conv_pre, up{i}, stage{i}."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    rks, rds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(rks)
    wn = lambda name: (fold(sd[f"{name}.weight_g"], sd[f"{name}.weight_v"]), sd[f"{name}.bias"])
    x = F.conv1d(F.pad(torch.as_tensor(mel).to(dtype), [6, 0]), *wn("conv_pre"))                 # models.py:212-213
    if taps is not None:
        taps["conv_pre"] = x
    for i in range(len(cfg["upsample_rates"])):
        x = F.conv_transpose1d(x, *wn(f"ups.{i}.1"), stride=cfg["upsample_rates"][i], padding=0)   # :216-217
        if taps is not None:
            taps[f"up{i}"] = x
        xs = None
        for j in range(nk):
            r = x
            for m, d in enumerate(rds[j]):
                r = amp_pair(sd, f"resblocks.{i * nk + j}", m, r, rks[j], d, dtype, fold)
            xs = r if xs is None else xs + r
        x = xs / nk
        if taps is not None:
            taps[f"stage{i}"] = x
    return conv_post(sd, x, length, dtype, fold)


def with_antialias(conf, layers, post):
    """A copy of the configuration with the two switches set."""
    c = dict(conf)
    c["vocoder_config"] = dict(conf["vocoder_config"], layers_antialias=list(layers), antialias_post=bool(post))
    return c


CONFIGS = {"all": ([True, True, True, True], True), "mixed": ([True, False, True, False], False)}


# ---------------------------------------------------------------------------------------------- shared by the two test files
def write_config(path, layers, post, h_dim=None):
    """The shipped variable-rate TOML with the two switches set (and, for cheap models, another h_dim); returns the loaded config."""
    from bvcodec import config
    txt = open(config.DEFAULT_CONFIG).read()
    old_l, old_p = "layers_antialias = [false, false, false, false]", "antialias_post = false"
    assert old_l in txt and old_p in txt
    txt = txt.replace(old_l, "layers_antialias = [" + ", ".join("true" if f else "false" for f in layers) + "]")
    txt = txt.replace(old_p, "antialias_post = " + ("true" if post else "false"))
    if h_dim is not None:
        assert "h_dim = 1024" in txt
        txt = txt.replace("h_dim = 1024", f"h_dim = {h_dim}")
    with open(path, "w") as f:
        f.write(txt)
    return config.load_config(path)


AA_TILE_HEIGHT = {64: 96, 32: 128, 16: 128, 8: 256}     # launch_amp_pair's tile (rows both convs sweep) of a filtered stage


def halo(ks, d):
    """An anti-aliased pair's out[t] reads x[t - halo .. t + 10] (test_antialias_cpu.py measures it)."""
    return (ks - 1) * (d + 1) + 2 * REACH


def aa_tile_rows(C, ks):
    """Valid output rows per tile: conv1 runs on the tile's rows, 10 of which feed A2's reach, ks - 1 conv2's."""
    return AA_TILE_HEIGHT[C] - (ks - 1) - 2 * REACH


def aa_lengths(TT, ks, d):
    """Rows per item: signals shorter than the filter's reach (both clamps at once), and both sides of every seam."""
    return sorted({1, 2, 5, 6, 10, 11, (ks - 1) * d + 10, TT - 1, TT, TT + 1, 2 * TT + 1, 3 * TT + 17})
