"""Shared by test_wide_generator_cpu.py, test_gpu_wide_generator.py and tests/golden/make_golden_wide.py: generators of 256 and
512 initial channels (``vocoder_config.upsample_initial_channel``; the shipped one has 128).  The configuration helpers, and a
restatement of the tile geometry launch_amp_pair / launch_conv_mfma / launch_conv_post (k_vocoder.hip) pick for the channel counts
only a wide generator has - every GPU case checks it against what the launch reports, as vocoder_layers.amp_tile_rows is."""
import vocoder_layers as vl

WIDTHS = (256, 512)
LDS_LIMIT = 160 * 1024
WIDE_CHANNELS = (256, 128)                 # stages on the wide forms of the AMP-pair kernel
AMP_HEIGHT = {256: 64, 128: 64}            # rows both convs of a tile sweep, offline and in windows of more than one short tile
AMP_HEIGHTS = {256: (64, 96), 128: (64, 128)}      # every compiled height (BVC_AMP256_TR / BVC_AMP128_TR; the first is the default)
AMP_SHORT = 32                             # a streaming window of at most one such tile takes it
ROW_GUARD = 512                            # rows the host keeps between L and the 32-bit byte offset's end


def with_width(conf, c0):
    """A copy of the configuration whose generator starts with c0 channels."""
    c = dict(conf)
    c["vocoder_config"] = dict(conf["vocoder_config"], upsample_initial_channel=int(c0))
    return c


def write_config(path, c0, h_dim=64, switches=None):
    """The shipped variable-rate TOML with ``upsample_initial_channel = c0`` (and, for cheap models, another h_dim); ``switches``:
    a dict like symmetric_oracle.CONFIGS' entries.  Returns the loaded config (config.load_config checks it)."""
    from bvcodec import config
    txt = open(config.DEFAULT_CONFIG).read()
    old = "upsample_initial_channel = 128"
    assert txt.count(old) == 1, old
    txt = txt.replace(old, f"upsample_initial_channel = {int(c0)}")
    for key, value in (switches or {}).items():
        off = "[false, false, false, false]" if isinstance(value, (list, tuple)) else "false"
        assert txt.count(f"{key} = {off}") == 1, key
        new = "[" + ", ".join("true" if f else "false" for f in value) + "]" if isinstance(value, (list, tuple)) else ("true" if value else "false")
        txt = txt.replace(f"{key} = {off}", f"{key} = {new}")
    if h_dim is not None:
        assert txt.count("h_dim = 1024") == 1
        txt = txt.replace("h_dim = 1024", f"h_dim = {h_dim}")
    with open(path, "w") as f:
        f.write(txt)
    return config.load_config(path)


def stage_channels(conf):
    v = conf["vocoder_config"]
    return [v["upsample_initial_channel"] >> (i + 1) for i in range(len(v["upsample_rates"]))]


# ---------------------------------------------------------------------------------------------- tile geometry (k_vocoder.hip)
def amp_tile_rows(C, ks, d, new_rows, window, height=None):
    """Valid output rows per tile and the family name of the AMP pair launch_amp_pair picks; the narrow channel counts are
    vocoder_layers.amp_tile_rows' (planned C = 64 heights excepted: pass them there)."""
    if C not in WIDE_CHANNELS:
        return vl.amp_tile_rows(C, ks, d, new_rows, window)
    if window and new_rows <= AMP_SHORT - (ks - 1):
        return AMP_SHORT - (ks - 1), f"amp{C}/window{AMP_SHORT}"
    h = AMP_HEIGHT[C] if (window or height is None) else height
    return h - (ks - 1), f"amp{C}/{h}" + ("/window" if window else "")


def amp_lds_bytes(C, ks, d, height):
    """amp_pair_kernel<C, ..., ALIAS = true>: the S1 rows (tile + conv1's halo); the S2 tile (height + ks - 1 rows) and the output
    staging (height rows) re-use them."""
    rows1 = height + (ks - 1) * d
    assert rows1 >= height + ks - 1
    return rows1 * (C + 2) * 4


def conv_tile_rows(cin):
    """launch_one's rows per workgroup, row-split tiles (offline)."""
    return {512: 64, 256: 128}.get(cin) or vl.conv_tile_rows(cin)


def conv_lds_bytes(cin, ks, d, rows):
    return (rows + (ks - 1) * d) * (cin + 2) * 4


def post_lds_bytes(C, ks, antialias=False):
    return (2 * (256 + ks - 1) + 10 if antialias else 256 + ks - 1) * C * 4


def max_rows(C):
    """Rows per item the wide AMP pair accepts: rows_load4's byte offset is a 32-bit integer."""
    return 0x7FFFFFFF // C // 4 - ROW_GUARD


def window_new_rows(ks):
    """New rows of a streaming window: one row, one frame of stage 0, one short tile, one more, and past the tall tiles."""
    return sorted({1, 8, AMP_SHORT - (ks - 1), AMP_SHORT - (ks - 1) + 1, 129})
