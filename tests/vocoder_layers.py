"""Shared by test_vocoder_layers_cpu.py and test_gpu_vocoder_layers.py: the weight draws, the inputs, the tile geometry of the
generator's launchers (a restatement of k_vocoder.hip that every GPU case checks against what the launch reports) and the
elementwise comparison with the float64 oracle."""
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
CHANNELS = (64, 32, 16, 8)           # per stage
KSIZES = (3, 7, 11)                  # per AMP block
DILATIONS = (1, 3, 5)                # per iteration
AMP64_HEIGHTS = (128, 112, 96, 80)
CE_RES, CE_RES_ACC, CE_RES_ACC_DIV = 1, 2, 3


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


# ---------------------------------------------------------------------------------------------- tile geometry (k_vocoder.hip)
def amp8_tile_rows(ks, d, mt2):
    """Amp8Geom<KS, D, MT2>::TT: NP = 64 * MT2 row pairs, whole blocks of d pairs, two rows per pair."""
    npairs = 4 * mt2 * 16
    return 2 * (npairs // d) * d - (ks - 1)


def amp_tile_rows(C, ks, d, new_rows, window, height64=128, c8=True, c16=True):
    """Valid output rows per tile of the kernel launch_amp_pair picks.  height64: the offline C = 64 tile height (forced or planned);
    c8 / c16: the model's vocoder_full_tiles / vocoder_c16_kernel options.  Returns (TT, family name)."""
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
        h = 128 if window else height64
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
    return {128: 128, 80: 128, 64: 128, 32: 256, 16: 256, 8: 256}[cin]


POST_TILE_ROWS = 256                 # conv_post_kernel: one output sample per thread


def lengths(TT, ks, d):
    """Rows per item: the shortest signals, both halo depths, and the seams of the first tiles."""
    ls = {1, 2, ks - 1, (ks - 1) * d, (ks - 1) * d + 1, TT - 1, TT, TT + 1, 2 * TT, 2 * TT + 1, 3 * TT + 17}
    return sorted(l for l in ls if l >= 1)


def window_new_rows(ks):
    return sorted({1, 8, 32 - (ks - 1), 32 - (ks - 1) + 1, 2 * (64 - (ks - 1)), 2 * (64 - (ks - 1)) + 1,
                   3 * (64 - (ks - 1)), 3 * (64 - (ks - 1)) + 1, 128, 129, 400})


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
def oracle_pair(sd, pair, x, dtype, epi=CE_RES, acc=None, n_blocks=3):
    i, j, m, C, ks, d, pre = pair
    y = obig.amp_pair(sd, pre, m, x, ks, d, dtype=dtype)
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
