"""TOML configuration of the codec path.

Reads the same file format and key names the reference facade reads at
bvrnn_codec_model.py:27-36,49-59 (configs/config_varBitRate.toml / config_64bit.toml load
unchanged); training-only keys are ignored.  ``AttrDict`` mirrors
third_party/BigVGAN/env.py:8-11 (attribute-style access to ``vocoder_config``).
"""
import os

try:                        # Python >= 3.11
    import tomllib as _toml
except ModuleNotFoundError:  # this image: Python 3.10 + tomli
    import tomli as _toml

_HERE = os.path.abspath(os.path.dirname(__file__))
DEFAULT_CONFIG = os.path.join(_HERE, "configs", "codec_varbitrate.toml")
DEFAULT_CONFIG_64BIT = os.path.join(_HERE, "configs", "codec_64bit.toml")

_REQUIRED = ("var_bit", "fs", "winsize", "hopsize", "num_mels", "fmin", "fmax", "mel_pad_left",
             "h_dim", "z_dim", "vocoder_config")
_REQUIRED_VOC = ("num_mels", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel",
                 "resblock_kernel_sizes", "resblock_dilation_sizes")


class AttrDict(dict):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def load_config(path):
    with open(path, "rb") as f:
        conf = _toml.load(f)
    for k in _REQUIRED:
        if k not in conf:
            raise KeyError(f"config {path}: missing key '{k}'")
    for k in _REQUIRED_VOC:
        if k not in conf["vocoder_config"]:
            raise KeyError(f"config {path}: missing key 'vocoder_config.{k}'")
    check_supported(conf)
    return conf


def antialias_flags(conf):
    """(per-stage list, post switch): where the generator wraps its SnakeBeta in ``Activation1d``
    (third_party/BigVGAN/models.py:172-192; absent keys: nowhere)."""
    v = conf["vocoder_config"]
    n = len(v["upsample_rates"])
    return [bool(f) for f in v.get("layers_antialias", [False] * n)], bool(v.get("antialias_post", False))


def is_antialiased(conf):
    stages, post = antialias_flags(conf)
    return any(stages) or post


NOT_CAUSAL = ("this generator has anti-aliased activations: every filtered AMP block looks 30 rows ahead, so it cannot run "
              "incrementally or on mixed-length batches (decode equal-length batches offline)")
NOT_CAUSAL_SYM = ("this generator has symmetric layers: a symmetric layer reads as many rows ahead as behind, so it cannot run "
                  "incrementally or on mixed-length batches (decode equal-length batches offline)")


def symmetric_flags(conf):
    """(per-stage list, pre switch, post switch): where the generator pads symmetrically instead of causally - ``layers_sym[i]``
    upsampler i and the stage's AMP blocks, ``pre_sym`` conv_pre, ``post_sym`` conv_post (third_party/BigVGAN/models.py:35-44,
    151-155,209-213,230-233; absent keys: nowhere)."""
    v = conf["vocoder_config"]
    n = len(v["upsample_rates"])
    return [bool(f) for f in v.get("layers_sym", [False] * n)], bool(v.get("pre_sym", False)), bool(v.get("post_sym", False))


def is_symmetric(conf):
    stages, pre, post = symmetric_flags(conf)
    return any(stages) or pre or post


def is_causal(conf):
    """Every output sample depends on earlier frames only: what streaming and mixed-length decoding count on."""
    return not (is_antialiased(conf) or is_symmetric(conf))


def not_causal_message(conf):
    """Why a non-causal generator is refused: a filtered one keeps its text, a symmetric, unfiltered one says so."""
    return NOT_CAUSAL if is_antialiased(conf) else NOT_CAUSAL_SYM


def num_frames(conf, L):
    """Frames the front-end makes of L samples, the count ``bvc_num_frames`` gives; 0 where a reflect padding is not shorter than the
    signal (the library answers BVC_EINVAL there)."""
    pr = conf["winsize"] - conf["mel_pad_left"] - conf["hopsize"]
    if L <= conf["mel_pad_left"] or L <= pr:
        return 0
    return (L + conf["mel_pad_left"] + pr - conf["winsize"]) // conf["hopsize"] + 1


def generator_length(conf, T, stages=False):
    """Samples the generator makes of T frames: L_0 = T, L_{i+1} = L_i * u_i behind a symmetric upsampler (ConvTranspose1d with
    padding (k - u) / 2, k = 2u), (L_i + 1) * u_i behind a causal one.  ``stages``: the list of the stage lengths instead."""
    sym = symmetric_flags(conf)[0]
    L, out = int(T), []
    for u, s in zip(conf["vocoder_config"]["upsample_rates"], sym):
        L = L * u if s else (L + 1) * u
        out.append(L)
    return out if stages else L


def stream_lags(conf):
    """The frontier arithmetic of the incremental generator behind a look-ahead window (csrc/generator.hip keeps the same table):
    after n frames, rows [0, rate * n - lag) of a tensor are final.  By the paddings: conv_pre lags 3 frames where it is symmetric;
    upsampler i multiplies the lag by its rate and, symmetric, adds rate / 2 (it is the view [u/2, u/2 + L u) of the causal rows); an
    iteration of a symmetric AMP block adds its reach (ks - 1)(d + 1) / 2, so a stage adds the longest block's sum; conv_post adds 3.
    Keys: "mel", "conv_pre", "up<i>", "stage<i>" (the oracle's tap names), "wav", and "P" / "Q": per stage, per block, the lag of the
    block's first and second iteration's result.  A filtered generator has no such table: ValueError with its text."""
    if is_antialiased(conf):
        raise ValueError("stream_lags: " + NOT_CAUSAL)
    v = conf["vocoder_config"]
    stages, pre, post = symmetric_flags(conf)
    lags = {"mel": 0, "conv_pre": 3 if pre else 0, "P": [], "Q": []}
    lag = lags["conv_pre"]
    for i, u in enumerate(v["upsample_rates"]):
        lag = lag * u + (u // 2 if stages[i] else 0)
        lags[f"up{i}"] = lag
        reaches = [[(ks - 1) * (d + 1) // 2 if stages[i] else 0 for d in ds]
                   for ks, ds in zip(v["resblock_kernel_sizes"], v["resblock_dilation_sizes"])]
        lags["P"].append([lag + r[0] for r in reaches])
        lags["Q"].append([lag + r[0] + r[1] for r in reaches])
        lag += max(sum(r) for r in reaches)
        lags[f"stage{i}"] = lag
    lags["wav"] = lag + (3 if post else 0)
    return lags


def generator_lookahead(conf):
    """Samples the generator looks ahead: sample t is final once frame (t + this) / 256 has arrived.  0 for a causal generator, -1
    for one that cannot stream (anti-aliased), as ``bvc_vocoder_lookahead`` answers."""
    return -1 if is_antialiased(conf) else stream_lags(conf)["wav"]


GENERATOR_WIDTHS = (16, 32, 64, 128, 256, 512)     # vocoder_config.upsample_initial_channel (check_config in csrc/model_build.hip)
FINAL_CHANNELS = (8, 16, 32)                       # channels in front of conv_post: the width halved once per upsampling stage
WIDEST_SWITCHED_STAGE = 64                         # layers_sym / layers_antialias: stages of more channels have the causal kernels only


def check_supported(conf):
    """The HIP path covers the snakebeta generator with causal or symmetric layers, and anti-aliased activations on causal stages;
    anything else fails loudly."""
    v = conf["vocoder_config"]
    bad = []
    if v.get("resblock", "1") != "1":
        bad.append("vocoder_config.resblock must be '1'")
    if v.get("activation", "snakebeta") != "snakebeta" or not v.get("snake_logscale", True):
        bad.append("only activation='snakebeta' with snake_logscale=true is implemented")
    aa = v.get("layers_antialias")
    if aa is not None and len(aa) != len(v["upsample_rates"]):
        bad.append(f"layers_antialias must have one entry per upsampling stage ({len(v['upsample_rates'])}), got {len(aa)}")
    sym = v.get("layers_sym")
    if sym is not None and len(sym) != len(v["upsample_rates"]):
        bad.append(f"layers_sym must have one entry per upsampling stage ({len(v['upsample_rates'])}), got {len(sym)}")
    elif sym is not None and any(sym):
        if any(k % 2 == 0 for k in v["resblock_kernel_sizes"]):
            bad.append("a symmetric stage (layers_sym) needs odd resblock_kernel_sizes")
        if aa is not None and len(aa) == len(sym) and any(a and s for a, s in zip(aa, sym)):
            bad.append("filtered (anti-aliased) stages are implemented as causal stages only: layers_sym and layers_antialias "
                       "are set on the same stage")
    if v.get("post_sym", False) and v.get("antialias_post", False):
        bad.append("a filtered (anti-aliased) activation_post is implemented in front of a causal conv_post only: post_sym and "
                   "antialias_post are both set")
    c0, n_up = v["upsample_initial_channel"], len(v["upsample_rates"])
    if c0 not in GENERATOR_WIDTHS:
        bad.append(f"vocoder_config.upsample_initial_channel must be one of {list(GENERATOR_WIDTHS)}, got {c0}")
    elif (c0 >> n_up) not in FINAL_CHANNELS:
        bad.append(f"vocoder_config.upsample_initial_channel = {c0} with {n_up} upsampling stages leaves {c0 >> n_up} channels in "
                   f"front of conv_post: must be one of {list(FINAL_CHANNELS)}")
    else:
        for key, what in (("layers_sym", "symmetric layers"), ("layers_antialias", "anti-aliased activations")):
            flags = v.get(key)
            wide = [i for i in range(n_up) if flags is not None and len(flags) == n_up and flags[i] and (c0 >> (i + 1)) > WIDEST_SWITCHED_STAGE]
            if wide:
                bad.append(f"{what} ({key}) are implemented on stages of {WIDEST_SWITCHED_STAGE} channels at most: with "
                           f"upsample_initial_channel = {c0}, stage {wide[0]} has {c0 >> (wide[0] + 1)}")
    for u, k in zip(v["upsample_rates"], v["upsample_kernel_sizes"]):
        if k != 2 * u:
            bad.append(f"transposed conv kernel {k} must be 2 x stride {u}")
    if conf["winsize"] != 1024 or conf["hopsize"] != 256:
        bad.append("front-end kernel is specialised for winsize=1024, hopsize=256")
    if conf["mel_pad_left"] < 0 or conf["mel_pad_left"] > conf["winsize"] - conf["hopsize"]:
        bad.append("mel_pad_left out of range")
    if any(conf[k] % 16 or conf[k] < 16 for k in ("z_dim", "h_dim", "num_mels")):
        bad.append("z_dim, h_dim and num_mels must be positive multiples of 16")
    if bad:
        raise ValueError("unsupported configuration: " + "; ".join(bad))
