"""Shared by test_lookahead_cpu.py and test_gpu_lookahead_stream.py; imports no GPU code.  The frontiers of the incremental generator
behind a look-ahead window as config.stream_lags gives them, an emulation of that stream built from the oracle's own layer functions
(oracle/bigvgan.py: conv_pre, upsample, amp_pair, conv_post), and the tile geometry of a symmetric AMP pair in a look-ahead window
(a restatement of amp_symmetric_window in k_vocoder_amp.hip that every GPU case checks against what the launch reports)."""
import torch

import vocoder_layers as vl
from bvcodec import config
from oracle import bigvgan as obig

CUTS_24 = ([1] * 24, [2, 1, 4, 8, 8, 1], [24])


def rates(conf):
    """Rows per frame of every tensor config.stream_lags names."""
    v = conf["vocoder_config"]
    out, r = {"mel": 1, "conv_pre": 1}, 1
    for i, u in enumerate(v["upsample_rates"]):
        r *= u
        out[f"up{i}"] = out[f"stage{i}"] = r
    out["wav"] = r
    return out


def frontier(rate, lag, n):
    """Rows of a tensor that are final after n frames."""
    return max(0, rate * n - lag)


def push_samples(conf, n_old, n_new):
    """Samples a look-ahead stream returns for the frames [n_old, n_new): the issue's [max(0, 256 n_old - D), max(0, 256 n_new - D))."""
    spf, D = rates(conf)["wav"], config.generator_lookahead(conf)
    return frontier(spf, D, n_new) - frontier(spf, D, n_old)


class StreamEmulation:
    """The stream in the oracle's arithmetic (any dtype; the tests use float64).  Every tensor is a buffer of its true length (T frames
    are announced up front, for the buffers' sizes alone) whose rows [0, frontier) are final and whose other rows are ZERO: rows that
    do not exist yet read as zeros, as in the kernels.  A push computes each tensor's new final rows from the tensor before it as it
    stands - final rows and zeros - and keeps only the output rows before the output's own frontier.  If a lag of config.stream_lags
    were too small, a kept row would have consumed such a zero and differ from the offline run.  The flush runs every layer on its
    complete input and keeps the rest.  (Full-length buffers, not truncated ones, also for the bits: the CPU's conv1d sums in an order
    that depends on the signal's length, 1 ulp apart in float64; with the offline shapes the kept rows are the offline run's exactly.)"""

    def __init__(self, sd, conf, T, dtype=torch.float64):
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.conf, self.v, self.dtype, self.T = conf, conf["vocoder_config"], dtype, T
        self.lags, self.rates = config.stream_lags(conf), rates(conf)
        self.sym, self.pre, self.post = obig.flags(self.v)
        self.n = 0
        self.done, self.front = {}, {}                         # tensor name -> its buffer (B, C, true length), its frontier
        self.nk = len(self.v["resblock_kernel_sizes"])

    def _keep(self, name, rows, rate, lag, flush):
        """Move into ``name`` the rows of ``rows`` (the layer's output on its input as it stands) between the old and the new
        frontier; returns (the buffer, the rows moved)."""
        if name not in self.done:
            self.done[name], self.front[name] = torch.zeros_like(rows), 0
        old = self.front[name]
        new = rows.shape[2] if flush else min(frontier(rate, lag, self.n), rows.shape[2])
        assert old <= new and self.done[name].shape == rows.shape, (name, old, new, rows.shape)
        self.done[name][:, :, old:new] = rows[:, :, old:new]
        self.front[name] = new
        return self.done[name], rows[:, :, old:new]

    def _advance(self, flush):
        sd, v, dt = self.sd, self.v, self.dtype
        x, _ = self._keep("conv_pre", obig.conv_pre(sd, self.done["mel"], dt, sym=self.pre), 1, self.lags["conv_pre"], flush)
        for i in range(len(v["upsample_rates"])):
            r = self.rates[f"up{i}"]
            x, _ = self._keep(f"up{i}", obig.upsample(sd, v, i, x, dt, sym=self.sym[i]), r, self.lags[f"up{i}"], flush)
            xs = None
            for j, ks in enumerate(v["resblock_kernel_sizes"]):
                pre = f"resblocks.{i * self.nk + j}"
                ds = v["resblock_dilation_sizes"][j]
                p, _ = self._keep(f"P{i}.{j}", obig.amp_pair(sd, pre, 0, x, ks, ds[0], dt, sym=self.sym[i]), r, self.lags["P"][i][j], flush)
                q, _ = self._keep(f"Q{i}.{j}", obig.amp_pair(sd, pre, 1, p, ks, ds[1], dt, sym=self.sym[i]), r, self.lags["Q"][i][j], flush)
                # the block's last iteration: kept up to the stage's frontier, where all blocks meet
                o, _ = self._keep(f"R{i}.{j}", obig.amp_pair(sd, pre, 2, q, ks, ds[2], dt, sym=self.sym[i]), r, self.lags[f"stage{i}"], flush)
                xs = o if xs is None else xs + o
            x = xs / self.nk
            self.done[f"stage{i}"] = x
        return self._keep("wav", obig.conv_post(sd, x, 10 ** 9, dt, sym=self.post), self.rates["wav"], self.lags["wav"], flush)[1]

    def push(self, mel):
        """mel (B, num_mels, k) -> (B, 1, samples that became final)."""
        if "mel" not in self.done:
            self.done["mel"] = torch.zeros(mel.shape[0], mel.shape[1], self.T, dtype=self.dtype)
        self.done["mel"][:, :, self.n:self.n + mel.shape[2]] = mel.to(self.dtype)
        self.n += mel.shape[2]
        assert self.n <= self.T
        return self._advance(False)

    def flush(self):
        assert self.n == self.T
        return self._advance(True)


def run_cuts(sd, conf, mel, cuts, dtype=torch.float64):
    """The emulated stream over mel (B, num_mels, T) cut into pushes of ``cuts`` frames and flushed: (pieces, emulation)."""
    assert sum(cuts) == mel.shape[2]
    em, pieces, t = StreamEmulation(sd, conf, mel.shape[2], dtype), [], 0
    with torch.no_grad():
        for k in cuts:
            pieces.append(em.push(mel[:, :, t:t + k]))
            t += k
        pieces.append(em.flush())
    return pieces, em


# ---------------------------------------------------------------------------------------------- tile geometry (amp_symmetric_window)
SYM_WINDOW_TILE = {64: (32, 64), 32: (64,), 16: (64,), 8: (128,)}        # the short tiles' heights per channel count
SYM_WINDOW_TILES = {64: (1, 2), 32: (3,), 16: (3,), 8: (3,)}              # and how many of them a window may take


def sym_window_tile_rows(C, ks, new_rows):
    """Valid output rows per tile of the kernel launch_amp_pair picks for a symmetric pair in a look-ahead window, and its name."""
    for height, count in zip(SYM_WINDOW_TILE[C], SYM_WINDOW_TILES[C]):
        if new_rows <= count * (height - (ks - 1)):
            return height - (ks - 1), f"amp{C}/lookahead{height}"
    return vl.SYM_TILE_HEIGHT[C] - (ks - 1), f"amp{C}/lookahead-offline"


def sym_window_new_rows(C, ks):
    """New rows of a look-ahead window: one, one frame of stage 0, the short tile's height and one more row, 129, and 400 - past the
    short tiles of every channel count, where the window takes the offline shape (129 rows are past them at C = 64 only)."""
    short = SYM_WINDOW_TILE[C][0] - (ks - 1)
    return sorted({1, 8, short, short + 1, 129, 400})
