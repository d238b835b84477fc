"""Shared by every generator test (the four test_*_cpu.py / test_gpu_*.py pairs of the plain, anti-aliased, symmetric and wide
generators), tests/golden/make_golden_*.py and the tools/*_cost.py scripts; imports no GPU code.  The named configurations and the
TOML writer, the weight draws, the inputs and case lists, the tile geometry of the generator's launchers (a restatement of
k_vocoder*.hip that every GPU case checks against what the launch reports) and the elementwise comparison with the float64 oracle
(oracle/bigvgan.py)."""
import collections

import numpy as np
import torch

from bvcodec import synth
from oracle import bigvgan as obig

U = 2.0 ** -24                       # unit roundoff of float32
MARGIN = 8.0                         # e_hip <= MARGIN * max(e32, U * max|oracle64|), see DESIGN.md section 2
NARROW_DRAWS = ("seed1235", "seed8", "seed100")
DRAWS = NARROW_DRAWS + ("wide",)
BATCHES = (2, 3, 5, 9)               # tile counts that are not multiples of 8 (the grids are padded to 8 and dealt per XCD)
CHANNELS = (64, 32, 16, 8)           # per stage of the shipped width
WIDTHS = (256, 512)                  # upsample_initial_channel of the wide generators (the shipped one has 128)
KSIZES = (3, 7, 11)                  # per AMP block
DILATIONS = (1, 3, 5)                # per iteration
CE_RES, CE_RES_ACC, CE_RES_ACC_DIV = 1, 2, 3


# ---------------------------------------------------------------------------------------------- configurations
def _c(layers_sym=(False,) * 4, pre_sym=False, post_sym=False, layers_antialias=(False,) * 4, antialias_post=False):
    return dict(layers_sym=list(layers_sym), pre_sym=pre_sym, post_sym=post_sym, layers_antialias=list(layers_antialias),
                antialias_post=antialias_post)


T_, F_ = True, False
AA_CONFIGS = {"all": _c(layers_antialias=[T_, T_, T_, T_], antialias_post=True), "mixed": _c(layers_antialias=[T_, F_, T_, F_])}
SYM_CONFIGS = {
    "all": _c([T_, T_, T_, T_], True, True),
    # symmetric C = 32 and C = 8 stages around the causal persistent C = 16 kernel
    "mixed": _c([F_, T_, F_, T_], False, True),
    "with_aa": _c([T_, F_, T_, F_], True, False, [F_, T_, F_, T_], True),
}


def with_switches(conf, switches=None, width=None):
    """A copy of the configuration with some of the five switches (a dict like the CONFIGS' entries, or a part of one) and / or
    the generator's initial channel count set."""
    v = dict(conf["vocoder_config"], **{k: (list(f) if isinstance(f, (list, tuple)) else bool(f)) for k, f in (switches or {}).items()})
    if width is not None:
        v["upsample_initial_channel"] = int(width)
    return dict(conf, vocoder_config=v)


def write_config(path, *, width=None, switches=None, h_dim=None):
    """The shipped variable-rate TOML with another ``upsample_initial_channel``, the given switches set and, for cheap models,
    another h_dim.  Returns the loaded config (config.load_config checks it)."""
    from bvcodec import config
    txt = open(config.DEFAULT_CONFIG).read()

    def put(old, new):
        nonlocal txt
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    if width is not None:
        put("upsample_initial_channel = 128", f"upsample_initial_channel = {int(width)}")
    for key, value in (switches or {}).items():
        if isinstance(value, (list, tuple)):
            put(f"{key} = [false, false, false, false]", f"{key} = [" + ", ".join("true" if f else "false" for f in value) + "]")
        else:
            put(f"{key} = false", f"{key} = " + ("true" if value else "false"))
    if h_dim is not None:
        put("h_dim = 1024", f"h_dim = {h_dim}")
    with open(path, "w") as f:
        f.write(txt)
    return config.load_config(path)


def stage_channels(conf):
    v = conf["vocoder_config"]
    return [v["upsample_initial_channel"] >> (i + 1) for i in range(len(v["upsample_rates"]))]


def generator_draw(conf, name):
    """The generator state dict of a draw.  'wide': seed 1235 with every alpha and beta redrawn ~ N(0, 1) (exp(alpha) up to about 20;
    the synthetic draws have sd 0.3).  sd 1.5 and more is not used: there the float32 oracle itself is 1e-3 from the float64 one."""
    if name != "wide":
        return synth.generator_state_dict(conf, int(name[4:]))
    sd = synth.generator_state_dict(conf, 1235)
    rng = np.random.default_rng(77)
    for k in sd:
        if k.endswith(".alpha") or k.endswith(".beta"):
            sd[k] = torch.from_numpy(rng.standard_normal(size=tuple(sd[k].shape)).astype(np.float32))
    return sd


def pairs(conf):
    """(stage, block, iteration, C, ks, d, state-dict prefix) of all AMP pairs."""
    v = conf["vocoder_config"]
    nk = len(v["resblock_kernel_sizes"])
    out = []
    for i in range(len(v["upsample_rates"])):
        C = v["upsample_initial_channel"] >> (i + 1)
        for j, ks in enumerate(v["resblock_kernel_sizes"]):
            for m, d in enumerate(v["resblock_dilation_sizes"][j]):
                out.append((i, j, m, C, ks, d, f"resblocks.{i * nk + j}"))
    return out


# ---------------------------------------------------------------------------------------------- tile geometry (k_vocoder*.hip)
LDS_LIMIT = 160 * 1024
WIDE_CHANNELS = (256, 128)                 # stages on the wide forms of the AMP-pair kernel
# every compiled offline height (rows both convs of a tile sweep; BVC_AMP256_TR / BVC_AMP128_TR / BVC_AMP64_TR force one); the first
# is the default of the wide ones, offline and in windows of more than one short tile - C = 64 takes the planned one
AMP_HEIGHTS = {256: (64, 96), 128: (64, 128), 64: (128, 112, 96, 80)}
AMP_HEIGHT = {C: AMP_HEIGHTS[C][0] for C in WIDE_CHANNELS}
AMP_SHORT = 32                             # a streaming window of at most one such tile takes it
AA_TILE_HEIGHT = {64: 96, 32: 128, 16: 128, 8: 256}       # launch_amp_pair's tile of a filtered stage
SYM_TILE_HEIGHT = {64: 128, 32: 256, 16: 128, 8: 256}     # and of a symmetric one
ROW_GUARD = 512                            # rows the host keeps between L and the 32-bit byte offset's end
REACH = obig.REACH


def amp8_tile_rows(ks, d, mt2):
    """Amp8Geom<KS, D, MT2>::TT: NP = 64 * MT2 row pairs, whole blocks of d pairs, two rows per pair."""
    npairs = 4 * mt2 * 16
    return 2 * (npairs // d) * d - (ks - 1)


def amp_tile_rows(C, ks, d, new_rows, window, height=None, c8=True, c16=True, form="causal"):
    """Valid output rows per tile of the kernel launch_amp_pair picks.  height: the offline tile height of C = 256, 128 and 64 (forced,
    or for C = 64 planned; None: the default, 128 at C = 64); c8 / c16: the model's vocoder_full_tiles / vocoder_c16_kernel options;
    form: 'causal', 'filtered' or 'symmetric', the stage's.  Returns (TT, family name)."""
    if form == "filtered":     # conv1 runs on the tile's rows, 10 of which feed A2's reach, ks - 1 conv2's
        return AA_TILE_HEIGHT[C] - (ks - 1) - 2 * REACH, f"amp{C}/filtered"
    if form == "symmetric":    # conv2 spends ks - 1 of the tile's rows, (ks-1)/2 on each side
        return SYM_TILE_HEIGHT[C] - (ks - 1), f"amp{C}/symmetric"
    if C in WIDE_CHANNELS:
        if window and new_rows <= AMP_SHORT - (ks - 1):
            return AMP_SHORT - (ks - 1), f"amp{C}/window{AMP_SHORT}"
        h = AMP_HEIGHT[C] if (window or height is None) else height
        return h - (ks - 1), f"amp{C}/{h}" + ("/window" if window else "")
    if window and C == 64 and new_rows <= 32 - (ks - 1):
        return 32 - (ks - 1), "amp64/window32"
    if window and C == 64 and new_rows <= 2 * (64 - (ks - 1)):
        return 64 - (ks - 1), "amp64/window64"
    if window and C == 32 and new_rows <= 3 * (64 - (ks - 1)):
        return 64 - (ks - 1), "amp32/window64"
    if C == 8 and c8:
        if window and new_rows <= 128:
            return amp8_tile_rows(ks, d, 1), "amp8/full<1,4>"
        return amp8_tile_rows(ks, d, 2), "amp8/full<2,2>" + ("/window" if window else "")
    if C == 64:
        h = 128 if (window or height is None) else height
        return h - (ks - 1), f"amp64/{h}" + ("/window" if window else "")
    if C == 32:
        return 256 - (ks - 1), "amp32/256" + ("/window" if window else "")
    if C == 16:
        if c16 and not window:
            return 256 - (ks - 1), "amp16/persistent"
        return 128 - (ks - 1), "amp16/generic" + ("/window" if window else "")
    return 256 - (ks - 1), "amp8/generic" + ("/window" if window else "")


def conv_tile_rows(cin):
    """launch_one's rows per workgroup for the row-split tiles of launch_conv_mfma (conv_pre and the upsamplers, offline)."""
    return {512: 64, 256: 128, 128: 128, 80: 128, 64: 128, 32: 256, 16: 256, 8: 256}[cin]


POST_TILE_ROWS = 256                 # conv_post_kernel: one output sample per thread


def amp_lds_bytes(C, ks, d, height):
    """amp_pair_kernel<C, ..., ALIAS = true>: the S1 rows (tile + conv1's halo); the S2 tile (height + ks - 1 rows) and the output
    staging (height rows) re-use them."""
    rows1 = height + (ks - 1) * d
    assert rows1 >= height + ks - 1
    return rows1 * (C + 2) * 4


def conv_lds_bytes(cin, ks, d, rows):
    return (rows + (ks - 1) * d) * (cin + 2) * 4


def post_lds_bytes(C, ks, antialias=False):
    return (2 * (256 + ks - 1) + 10 if antialias else 256 + ks - 1) * C * 4


def max_rows(C):
    """Rows per item the wide AMP pair accepts: rows_load4's byte offset is a 32-bit integer."""
    return 0x7FFFFFFF // C // 4 - ROW_GUARD


# ---------------------------------------------------------------------------------------------- the case lists
def lengths(TT, ks, d):
    """Rows per item: the shortest signals, both halo depths, and the seams of the first tiles."""
    ls = {1, 2, ks - 1, (ks - 1) * d, (ks - 1) * d + 1, TT - 1, TT, TT + 1, 2 * TT, 2 * TT + 1, 3 * TT + 17}
    return sorted(l for l in ls if l >= 1)


def window_new_rows(ks):
    return sorted({1, 8, 32 - (ks - 1), 32 - (ks - 1) + 1, 2 * (64 - (ks - 1)), 2 * (64 - (ks - 1)) + 1,
                   3 * (64 - (ks - 1)), 3 * (64 - (ks - 1)) + 1, 128, 129, 400})


def wide_window_new_rows(ks):
    """New rows of a streaming window: one row, one frame of stage 0, one short tile, one more, and past the tall tiles."""
    return sorted({1, 8, AMP_SHORT - (ks - 1), AMP_SHORT - (ks - 1) + 1, 129})


def halo(ks, d):
    """An anti-aliased pair's out[t] reads x[t - halo .. t + 10] (test_antialias_cpu.py measures it)."""
    return (ks - 1) * (d + 1) + 2 * REACH


def aa_lengths(TT, ks, d):
    """Rows per item: signals shorter than the filter's reach (both clamps at once), and both sides of every seam."""
    return sorted({1, 2, 5, 6, 10, 11, (ks - 1) * d + 10, TT - 1, TT, TT + 1, 2 * TT + 1, 3 * TT + 17})


def reach(ks, d):
    """A symmetric pair's out[t] reads x[t - reach .. t + reach] (test_symmetric_cpu.py measures it)."""
    return (ks - 1) * (d + 1) // 2


def sym_amp_lengths(TT, ks, d):
    """Rows per item: signals shorter than the reach on both sides at once, both sides of every seam, the last tile's end anywhere."""
    p2, h = (ks - 1) // 2, reach(ks, d)
    return sorted({1, 2, p2, p2 + 1, h, h + 1, 2 * h + 1, TT - 1, TT, TT + 1, 2 * TT + 1, 3 * TT + 17})


def sym_lengths(cfg, T):
    """Rows after every stage: L * u behind a symmetric upsampler, (L + 1) * u behind a causal one; the last is the waveform's."""
    out, L = [], T
    for u, s in zip(cfg["upsample_rates"], obig.flags(cfg)[0]):
        L = L * u if s else (L + 1) * u
        out.append(L)
    return out


# ---------------------------------------------------------------------------------------------- inputs, channels-first (B, C, L)
INPUTS = ("n1", "n6", "zeros", "row_first", "row_last", "row_tile2")


def make_input(kind, B, C, L, TT, seed):
    rng = np.random.default_rng(seed)
    if kind in ("n1", "n6"):
        x = rng.standard_normal((B, C, L)) * (1.0 if kind == "n1" else 6.0)
    else:
        x = np.zeros((B, C, L))
        if kind != "zeros":
            row = {"row_first": 0, "row_last": L - 1, "row_tile2": TT if TT < L else L - 1}[kind]
            x[:, :, row] = rng.standard_normal((B, C)) * 2.0           # every item its own values
    return torch.from_numpy(x.astype(np.float32))


# ---------------------------------------------------------------------------------------------- oracle units with the epilogues
def oracle_pair(sd, pair, x, dtype, epi=CE_RES, acc=None, n_blocks=3, sym=False):
    i, j, m, C, ks, d, pre = pair
    y = obig.amp_pair(sd, pre, m, x, ks, d, dtype=dtype, sym=sym)
    if epi >= CE_RES_ACC:
        y = acc.to(dtype) + y                                           # xs += resblock   (models.py:224)
    if epi == CE_RES_ACC_DIV:
        y = y / n_blocks                                                # xs / num_kernels (models.py:225)
    return y


def cl(t):
    """(B, C, L) -> channels-last float64 numpy (B, L, C)."""
    return t.detach().cpu().permute(0, 2, 1).contiguous().to(torch.float64).numpy()


# ---------------------------------------------------------------------------------------------- the comparison
Verdict = collections.namedtuple("Verdict", "ok e_hip e32 scale bar ratio worst row_in_tile message")


def compare(got, ref64, ref32, what, tile_rows=None, row0=0, margin=MARGIN):
    """got / ref64 / ref32: (B, L, C) arrays (or (B, L) for a waveform) of the same rows.  Every element, maximum norm:
    e_hip = max|got - ref64| <= margin * max(e32, U * max|ref64|), e32 = max|ref32 - ref64|.  row0: position of the arrays' first row
    inside the launch's output rows (for the row's place in its tile, row % tile_rows)."""
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape, ref32.shape)
    if got.ndim == 2:
        got, ref64, ref32 = got[:, :, None], ref64[:, :, None], ref32[:, :, None]
    assert np.isfinite(ref64).all() and np.isfinite(ref32).all(), what
    e32 = float(np.abs(ref32 - ref64).max())
    scale = float(np.abs(ref64).max())
    floor = max(e32, U * scale)
    bar = margin * floor
    err = np.abs(got - ref64)
    err = np.where(np.isfinite(got), err, np.inf)                       # a NaN (an element nobody wrote) is the worst element
    b, row, c = (int(k) for k in np.unravel_index(int(np.argmax(err)), err.shape))
    e_hip = float(err[b, row, c])
    rit = (row + row0) % tile_rows if tile_rows else None
    ok = e_hip <= bar
    msg = (f"{what}: max|hip - oracle64| = {e_hip:.3e} at (item {b}, row {row + row0}, channel {c})"
           + (f", row % TT = {rit} of TT = {tile_rows}" if tile_rows else "")
           + f"; got {got[b, row, c]!r} expected {ref64[b, row, c]!r}; bar {bar:.3e} = {margin:g} x max(e32 = {e32:.3e}, "
           f"u x max|oracle64| = {U * scale:.3e}); shape {got.shape}")
    return Verdict(ok, e_hip, e32, scale, bar, e_hip / floor if floor > 0 else (0.0 if e_hip == 0 else float("inf")), (b, row + row0, c), rit, msg)


class Ledger:
    """Largest e_hip / max(e32, floor) per kernel family, and the failures of a sweep (all of them are reported, not the first)."""

    def __init__(self, draw):
        self.draw, self.stats, self.failures, self.cases = draw, {}, [], 0

    def add(self, family, v):
        self.cases += 1
        s = self.stats.get(family)
        if s is None or v.ratio > s[0]:
            self.stats[family] = (v.ratio, v.e32 / v.scale if v.scale else 0.0, v.message)
        if not v.ok:
            self.failures.append(v.message)

    def close(self):
        for fam in sorted(self.stats):
            r, e32rel, msg = self.stats[fam]
            print(f"PARITY draw={self.draw} family={fam} max_ratio={r:.3f} e32_rel={e32rel:.3e} case=[{msg.split(':')[0]}]", flush=True)
        print(f"PARITY draw={self.draw} cases={self.cases} failures={len(self.failures)}", flush=True)
        assert not self.failures, f"{len(self.failures)} of {self.cases} cases failed; first ones:\n" + "\n".join(self.failures[:12])
