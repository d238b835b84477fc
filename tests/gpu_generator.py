"""The GPU harness of the generator tests (test_gpu_vocoder_layers.py, test_gpu_antialias.py, test_gpu_symmetric.py,
test_gpu_wide_generator.py): the product model of one configuration and one weight draw with the library's test entry points, one
AMP pair against the float64 oracle in every form (causal narrow and wide, filtered, symmetric; offline and in streaming windows),
the conv_post sweep of the switched generators and the comparison with a reference fixture.  The cases and their lists are the test
files'; the geometry they are held to is vocoder_layers' restatement."""
import contextlib
import ctypes
import os
import zlib

import numpy as np
import torch

import vocoder_layers as vl
from conftest import load_golden
from oracle import bigvgan as obig

DEV = "cuda:0"
KIND_PRE, KIND_UP, KIND_AMP, KIND_POST = 0, 1, 2, 3
H_DIM = 64                                   # a small coder, where the tests are about the generator
TILE_SWITCHES = ("BVC_TILE_CUT", "BVC_AMP64_TR", "BVC_AMP128_TR", "BVC_AMP256_TR")
TAPS = ["conv_pre"] + [f"{k}{i}" for i in range(4) for k in ("up", "stage")]         # bvc_test_vocoder_tap's `which`, in order


@contextlib.contextmanager
def switches(names, **env):
    """The environment with the switches ``names`` unset, but for those given."""
    old = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def to_dev(t):
    """(B, C, L) CPU tensor -> contiguous channels-last device tensor (B, L, C)."""
    return t.permute(0, 2, 1).contiguous().to(DEV)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV)


class Model:
    """The product model of one configuration and one generator draw on the GPU (checkpoints written into ``directory``) and the
    draw's state dict.  name None: the shipped variable-rate TOML; else the TOML vl.write_config(**config) writes as <name>.toml."""

    def __init__(self, directory, draw="seed1235", name=None, **config):
        from bvcodec import BVRNNCodecModel, _abi, synth
        from bvcodec import config as bconfig
        self.draw = draw
        if name is None:
            cfg, self.conf = bconfig.DEFAULT_CONFIG, bconfig.load_config(bconfig.DEFAULT_CONFIG)
        else:
            cfg = os.path.join(directory, f"{name}.toml")
            self.conf = vl.write_config(cfg, **config)
        self.width = self.conf["vocoder_config"]["upsample_initial_channel"]
        self.sd = vl.generator_draw(self.conf, draw)
        self.vr = synth.bvrnn_state_dict(self.conf, 1234)
        p1, p2 = os.path.join(directory, f"bvrnn_{self.conf['h_dim']}"), os.path.join(directory, f"bigvgan_{name or 'shipped'}_{draw}")
        if not os.path.exists(p1):
            torch.save({"vrnn": self.vr}, p1)
        torch.save({"generator": self.sd}, p2)
        self.model = BVRNNCodecModel(cfg, p1, p2).to(DEV)
        self.eng = self.model.engine(torch.empty(0, device=DEV))
        self.lib, self.abi = _abi.load(), _abi

    def layer_rc(self, kind, x, out, stage=0, block=0, iteration=0, epi=vl.CE_RES, acc=None, window=None, length=0, div=1.0):
        """ONE launch of the path.  x (B, L, Cin), out: device tensors, channels-last; window: None or (row_begin, t_origin).
        Returns (rc, out_info)."""
        info = (ctypes.c_int64 * 5)()
        rb, t0 = window if window else (0, 0)
        B, L = x.shape[0], x.shape[1]
        rc = self.lib.bvc_test_vocoder_layer(self.eng.handle, kind, stage, block, iteration, self.abi.ptr(x), B, L, self.abi.ptr(out),
                                             epi, self.abi.ptr(acc), 1 if window else 0, rb, t0, length, div, info, self.eng.stream())
        return rc, list(info)

    def layer(self, *a, **k):
        rc, info = self.layer_rc(*a, **k)
        self.abi.check(rc)
        return info

    def tap(self, mel_tm, which):
        """Tap TAPS[which] of the whole chain on mel_tm (B, T, num_mels): a flat (B, rows * channels) device tensor."""
        B, T = mel_tm.shape[0], mel_tm.shape[1]
        ws, nws = self.eng.workspace(B, T)
        n, out = ctypes.c_int64(), None
        for _ in range(2):                                           # the first call asks for the size
            self.abi.check(self.lib.bvc_test_vocoder_tap(self.eng.handle, self.abi.ptr(mel_tm), B, T, which, self.abi.ptr(out), ctypes.byref(n),
                                                         ws, nws, self.eng.stream()))
            out = nan_like(B, n.value) if out is None else out
        torch.cuda.synchronize()
        return out

    def planned_height(self, rows, B, ks):
        out = (ctypes.c_int64 * 6)()
        self.abi.check(self.lib.bvc_test_tile_plan(1, rows, B, ks, 0, out))
        return int(out[0])


def cached(make):
    """(get, close) for a module's fixture: get(*key) makes each model once, close() checks the status of every model made."""
    cache = {}

    def get(*key):
        if key not in cache:
            cache[key] = make(*key)
        return cache[key]

    def close():
        for m in cache.values():
            m.model.check_status()
    return get, close


# ---------------------------------------------------------------------------------------------- one AMP pair
def amp_case(mo, ledger, pair, B, L, kind, epi, window=None, height=None, c8=True, c16=True):
    """One launch of one AMP pair against the float64 oracle, with the tiles of vl.amp_tile_rows asserted; returns out_info.
    window: None, or (mode, row_begin, t_origin) with mode 'start' (history all zero, t_origin = -row_begin: global time 0 is the
    first new row, inside the tile conv1 sweeps, and the S2 rows before it are zero) or 'mid' (the buffer is cut out of a longer
    signal).  L counts the buffer's rows (history included).  height: a compiled tile height to force (C = 256, 128, 64), or None for
    the launcher's own - at C = 64 offline the planned one; c8 / c16: the engine's options, which the caller has set.  Whether the
    stage is symmetric is read from the model's configuration, whether it is filtered from its state dict's keys, as the oracle does."""
    i, j, m, C, ks, d, pre = pair
    sym = obig.flags(mo.conf["vocoder_config"])[0][i]
    form = "symmetric" if sym else "filtered" if obig.is_filtered(mo.sd, f"{pre}.activations.0") else "causal"
    rb = window[1] if window else 0
    new_rows = L - rb
    planned = form == "causal" and C == 64 and not window and height is None
    TT, family = vl.amp_tile_rows(C, ks, d, new_rows, window is not None, mo.planned_height(new_rows, B, ks) if planned else height, c8, c16, form)
    if planned:
        family = "amp64/plan"
    # the texts and seeds every family has had from its first day: they name the ledgers' worst cases and draw their inputs
    title = {"causal": "amp pair" + (f" width {mo.width}" if C in vl.WIDE_CHANNELS else ""), "filtered": "filtered amp pair",
             "symmetric": "symmetric amp pair"}[form]
    what = f"{title} stage {i} block {j} iteration {m} (C={C} ks={ks} d={d}) epi={epi} B={B} L={L} input={kind}"
    key = (mo.draw,) + ((mo.width,) if C in vl.WIDE_CHANNELS else ()) + (i, j, m, B, L, kind, epi)
    if form == "causal":
        what += f" variant={family}" + (f" window={window}" if window else "")
        key += (family, window)
    seed = seed_of(*key)
    if window and window[0] == "mid":
        t0 = window[2]
        x_full = vl.make_input(kind, B, C, t0 + L, t0 + rb + TT, seed)
        buf, x_ref, lo = x_full[:, :, t0:], x_full, t0 + rb
    elif window:
        t0 = -rb
        x_new = vl.make_input(kind, B, C, new_rows, TT, seed)
        buf, x_ref, lo = torch.cat([torch.zeros(B, C, rb), x_new], 2), x_new, 0
    else:
        t0 = 0
        buf = x_ref = vl.make_input(kind, B, C, L, TT, seed)
        lo = 0
    acc = acc_ref = None
    if epi >= vl.CE_RES_ACC:
        acc = vl.make_input("n1", B, C, L, TT, seed + 1)
        acc_ref = torch.zeros_like(x_ref)
        acc_ref[:, :, lo:] = acc[:, :, rb:]
    with torch.no_grad():
        r64 = vl.cl(vl.oracle_pair(mo.sd, pair, x_ref, torch.float64, epi, acc_ref, sym=sym))[:, lo:]
        r32 = vl.cl(vl.oracle_pair(mo.sd, pair, x_ref, torch.float32, epi, acc_ref, sym=sym))[:, lo:]
    x_dev = to_dev(buf)
    if acc is None:
        out, acc_dev, before = nan_like(B, L, C), None, None
    else:
        out = to_dev(acc)                                            # the running sum IS the output buffer, as in run_vocoder (w.XS)
        acc_dev, before = out, out.clone()
    with switches(TILE_SWITCHES, **({f"BVC_AMP{C}_TR": str(height)} if height is not None else {})):
        info = mo.layer(KIND_AMP, x_dev, out, i, j, m, epi, acc_dev, (rb, t0) if window else None)
    tiles = B * -(-new_rows // TT)
    padded = info[3] if ("persistent" in family or "full" in family) else (tiles + 7) // 8 * 8
    assert info == [L, C, tiles, padded, TT], (what, info, "assumed tiles / rows per tile", tiles, TT)
    got = out.cpu().numpy()
    if rb:                                                           # history rows are nobody's to write
        hist = got[:, :rb]
        assert np.isnan(hist).all() if before is None else np.array_equal(hist, before.cpu().numpy()[:, :rb]), what + ": history rows written"
    ledger.add(family, vl.compare(got[:, rb:], r64, r32, what, tile_rows=TT))
    return info


def every_channel_count_meets_every_epilogue(conf):
    """The rotation (q + stage) % 3 of the filtered and the symmetric AMP sweeps gives every (C, epilogue)."""
    seen = set()
    for stage in range(4):
        for q, pair in enumerate(p for p in vl.pairs(conf) if p[0] == stage):
            seen.add((pair[3], (q + stage) % 3))
    assert seen == {(C, e) for C in vl.CHANNELS for e in range(3)}


# ---------------------------------------------------------------------------------------------- conv_post behind a switch
def conv_post_sweep(mo, ledger, word, rows, all_inputs_at, inputs):
    """conv_post of a filtered or symmetric (``word``) generator from 8 channels: L of ``rows`` with ``length`` below, equal to and
    above L, N(0, 36) input - and ``inputs`` at the two L of ``all_inputs_at``; B and the divisor rotate."""
    sym = obig.flags(mo.conf["vocoder_config"])[2]
    n = 0
    for L in rows:
        for length in sorted({L, max(1, L - 3), 10 ** 9}):
            for kind in (("n6",) if L not in all_inputs_at else inputs):
                n += 1
                B, div = 2 + n % 2, (1.0, 0.95)[n % 2]
                x = vl.make_input(kind, B, 8, L, vl.POST_TILE_ROWS, seed_of(mo.draw, "post", L, length, kind))
                n_out = min(L, length)
                out = nan_like(B, n_out)
                info = mo.layer(KIND_POST, to_dev(x), out, length=length, div=div)
                assert info[:2] == [n_out, 1]
                with torch.no_grad():
                    r64 = obig.conv_post(mo.sd, x, length, torch.float64, sym=sym)[:, 0].numpy() / np.float64(np.float32(div))
                    r32 = (obig.conv_post(mo.sd, x, length, torch.float32, sym=sym)[:, 0].numpy() / np.float32(div)).astype(np.float64)
                ledger.add(f"conv_post/{word}", vl.compare(out.cpu().numpy(), r64, r32,
                                                           f"{word} conv_post B={B} L={L} length={length} div={div} input={kind}",
                                                           tile_rows=vl.POST_TILE_ROWS))


# ---------------------------------------------------------------------------------------------- the reference's run
def check_fixture(mo, golden, label, taps, rms_bar, max_bar=None, tap_bar=2e-5):
    """BigVGAN.forward against the waveform of tests/golden/<golden>.npz (rms <= rms_bar, and every sample < max_bar) and
    bvc_test_vocoder_tap against its stored ``taps`` (<= tap_bar x max(1, max|tap|)).  Returns the fixture."""
    g = load_golden(golden)
    mel = torch.from_numpy(g["mel"]).to(DEV)
    wav = mo.model.vocoder(mel, 10 ** 9).cpu().numpy()
    assert wav.shape == g["wav"].shape
    rms = float(np.sqrt(((wav - g["wav"]) ** 2).mean()))
    print(f"FIXTURE {label}: waveform rms error {rms:.3e} max {np.abs(wav - g['wav']).max():.3e}")
    assert rms <= rms_bar and (max_bar is None or np.abs(wav - g["wav"]).max() < max_bar)
    mel_tm = mel.permute(0, 2, 1).contiguous()
    for nm in taps:
        ref = g[nm]
        got = mo.tap(mel_tm, TAPS.index(nm)).cpu().numpy().reshape(ref.shape[0], -1, ref.shape[1]).transpose(0, 2, 1)
        assert got.shape == ref.shape
        err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
        print(f"FIXTURE {label}: {nm} max error {err:.3e} (scale {scale:.3f})")
        assert err <= tap_bar * scale, (label, nm, err, scale)
    return g
