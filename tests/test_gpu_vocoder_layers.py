"""The generator's kernels one layer at a time against the float64 oracle (bvc_test_vocoder_layer runs ONE launch of the path on a
given input): every AMP pair (C, ks, dilation) x epilogue x tile shape - the four compiled C = 64 heights and the planned one, the
persistent C = 16 and C = 8 kernels and the generic kernel behind their options, the streaming window shapes - at lengths on both
sides of every tile seam, on four weight draws (one with alpha, beta ~ N(0, 1)); conv_pre, the upsamplers and conv_post the same
way; the whole chain at sizes with seams.  Every element, maximum norm: e_hip = max|hip - oracle64| <= MARGIN x max(e32,
2^-24 max|oracle64|) with e32 = max|oracle32 - oracle64| on the identical input (vocoder_layers.compare; DESIGN.md section 2;
measured ratios in profiles/vocoder_layer_parity.md).  Every AMP case also asserts that the launch was cut into the tiles this file
assumes.  Needs the MI355X: run with ``-m gpu``."""
import contextlib
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import vocoder_layers as vl
from oracle import bigvgan as obig

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCHES = ("BVC_TILE_CUT", "BVC_AMP64_TR")
KIND_PRE, KIND_UP, KIND_AMP, KIND_POST = 0, 1, 2, 3


@contextlib.contextmanager
def switches(**env):
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Draw:
    """One weight draw: the product model on the GPU (checkpoints written into a temporary directory) and its state dict."""

    def __init__(self, conf, name, directory):
        from bvcodec import BVRNNCodecModel, _abi, config, synth
        self.name, self.conf, self.sd = name, conf, vl.generator_draw(conf, name)
        p1 = os.path.join(directory, "bvrnn")
        if not os.path.exists(p1):
            torch.save({"vrnn": synth.bvrnn_state_dict(conf, 1234)}, p1)
        p2 = os.path.join(directory, f"bigvgan_{name}")
        torch.save({"generator": self.sd}, p2)
        self.model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
        self.eng = self.model.engine(torch.empty(0, device=DEV))
        self.lib, self.abi = _abi.load(), _abi

    def layer(self, kind, x, out, stage=0, block=0, iteration=0, epi=vl.CE_RES, acc=None, window=None, length=0, div=1.0):
        """x (B, L, Cin), out: device tensors, channels-last.  Returns out_info."""
        info = (ctypes.c_int64 * 5)()
        rb, t0 = window if window else (0, 0)
        B, L = x.shape[0], x.shape[1]
        self.abi.check(self.lib.bvc_test_vocoder_layer(self.eng.handle, kind, stage, block, iteration, self.abi.ptr(x), B, L, self.abi.ptr(out),
                                                       epi, self.abi.ptr(acc), 1 if window else 0, rb, t0, length, div, info, self.eng.stream()))
        return list(info)

    def planned_height(self, rows, B, ks):
        out = (ctypes.c_int64 * 6)()
        self.abi.check(self.lib.bvc_test_tile_plan(1, rows, B, ks, 0, out))
        return int(out[0])


@pytest.fixture(scope="module")
def draws(conf_var, tmp_path_factory):
    directory, cache = str(tmp_path_factory.mktemp("vocoder_layers")), {}

    def get(name):
        if name not in cache:
            cache[name] = Draw(conf_var, name, directory)
        return cache[name]
    yield get
    for d in cache.values():
        d.model.check_status()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def to_dev(t):
    """(B, C, L) CPU tensor -> contiguous channels-last device tensor (B, L, C)."""
    return t.permute(0, 2, 1).contiguous().to(DEV)


def nan_like(shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------------------------------------------------------------------------------------- one AMP pair
def amp_case(dr, ledger, pair, B, L, kind, epi, variant, window=None):
    """variant: dict(height64=int or 'plan', c8=bool, c16=bool) - the engine's options are set by the caller; height64 is forced here.
    window: None, or (mode, row_begin, t_origin) with mode 'start' (history all zero, t_origin = -row_begin) or 'mid' (the buffer is
    cut out of a longer signal).  L counts the buffer's rows (history included)."""
    i, j, m, C, ks, d, pre = pair
    rb = window[1] if window else 0
    new_rows = L - rb
    h64 = variant.get("height64", "plan")
    height = dr.planned_height(new_rows, B, ks) if h64 == "plan" else h64
    TT, family = vl.amp_tile_rows(C, ks, d, new_rows, window is not None, height64=height, c8=variant.get("c8", True), c16=variant.get("c16", True))
    if C == 64 and not window and h64 == "plan":
        family = "amp64/plan"
    what = (f"amp pair stage {i} block {j} iteration {m} (C={C} ks={ks} d={d}) epi={epi} B={B} L={L} input={kind} variant={family}"
            + (f" window={window}" if window else ""))
    seed = seed_of(dr.name, i, j, m, B, L, kind, epi, family, window)
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
        r64 = vl.cl(vl.oracle_pair(dr.sd, pair, x_ref, torch.float64, epi, acc_ref))[:, lo:]
        r32 = vl.cl(vl.oracle_pair(dr.sd, pair, x_ref, torch.float32, epi, acc_ref))[:, lo:]
    x_dev = to_dev(buf)
    if acc is None:
        out, acc_dev, before = nan_like((B, L, C)), None, None
    else:
        out = to_dev(acc)                                            # the running sum IS the output buffer, as in run_vocoder (w.XS)
        acc_dev, before = out, out.clone()
    env = {"BVC_AMP64_TR": str(h64)} if (C == 64 and h64 != "plan") else {}
    with switches(**env):
        info = dr.layer(KIND_AMP, x_dev, out, i, j, m, epi, acc_dev, (rb, t0) if window else None)
    tiles = B * -(-new_rows // TT)
    assert info[:2] == [L, C] and info[2] == tiles and info[4] == TT, (what, info, "assumed tiles / rows per tile", tiles, TT)
    if "persistent" not in family and "full" not in family:
        assert info[3] == (tiles + 7) // 8 * 8, (what, info)
    got = out.cpu().numpy()
    if rb:                                                           # history rows are nobody's to write
        hist = got[:, :rb]
        assert np.isnan(hist).all() if before is None else np.array_equal(hist, before.cpu().numpy()[:, :rb]), what + ": history rows written"
    v = vl.compare(got[:, rb:], r64, r32, what, tile_rows=TT)
    ledger.add(family, v)
    return info


def amp_variants(C):
    if C == 64:
        return [dict(height64=h) for h in vl.AMP64_HEIGHTS] + [dict(height64="plan")]
    if C == 16:
        return [dict(c16=True), dict(c16=False)]
    if C == 8:
        return [dict(c8=True), dict(c8=False)]
    return [dict()]


@contextlib.contextmanager
def options(dr, variant):
    try:
        dr.eng.set_option("vocoder_full_tiles", 1 if variant.get("c8", True) else 0)
        dr.eng.set_option("vocoder_c16_kernel", 1 if variant.get("c16", True) else 0)
        yield
    finally:
        dr.eng.set_option("vocoder_full_tiles", 1)
        dr.eng.set_option("vocoder_c16_kernel", 1)


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("draw", vl.DRAWS)
def test_amp_pairs_offline_against_float64(draws, conf_var, draw, stage):
    """All nine (ks, dilation) pairs of a stage, every tile shape: the full length list with the residual epilogue on N(0, 1) input;
    the other inputs (N(0, 36), zeros, one non-zero row at row 0 / the last row / the first row of the second tile) at TT, 2 TT + 1
    and 3 TT + 17; the two accumulating epilogues, the running sum aliased to the output, at TT and 2 TT + 1."""
    dr, ledger, n = draws(draw), vl.Ledger(draw), 0
    for pair in [p for p in vl.pairs(conf_var) if p[0] == stage]:
        C, ks, d = pair[3:6]
        for variant in amp_variants(C):
            h64 = variant.get("height64", "plan")
            TT = vl.amp_tile_rows(C, ks, d, 10 ** 6, False, height64=128 if h64 == "plan" else h64, c8=variant.get("c8", True),
                                  c16=variant.get("c16", True))[0]
            with options(dr, variant):
                for L in vl.lengths(TT, ks, d):
                    n += 1
                    amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, "n1", vl.CE_RES, variant)
                for kind in vl.INPUTS[1:]:
                    for L in (TT, 2 * TT + 1, 3 * TT + 17):
                        n += 1
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, kind, vl.CE_RES, variant)
                for epi in (vl.CE_RES_ACC, vl.CE_RES_ACC_DIV):
                    for L in (TT, 2 * TT + 1):
                        n += 1
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, "n1", epi, variant)
    ledger.close()


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("draw", vl.DRAWS)
def test_amp_pairs_in_streaming_windows_against_float64(draws, conf_var, draw, stage):
    """The window shapes of a streaming hop: new rows behind a history, on both sides of every threshold at the top of
    launch_amp_pair.  'mid': the buffer is rows [t_origin, t_origin + L) of a longer signal, history 64 rows (what a hop keeps) and
    (ks - 1) (d + 1) rows (just deep enough for both halos); 'start': t_origin = -row_begin, the history all zero - the new rows
    are the first rows of a signal and see the causal zero padding."""
    dr, ledger, n = draws(draw), vl.Ledger(draw), 0
    for pair in [p for p in vl.pairs(conf_var) if p[0] == stage]:
        C, ks, d = pair[3:6]
        deep = (ks - 1) * (d + 1)
        for variant in ([dict(c8=True), dict(c8=False)] if C == 8 else [dict()]):
            with options(dr, variant):
                for new in vl.window_new_rows(ks):
                    for window in (("start", 64, -64), ("mid", 64, 0), ("mid", 64, 37), ("mid", deep, 5)):
                        n += 1
                        kind = ("n1", "n6", "row_first", "n1", "zeros", "row_tile2", "n1", "row_last")[n % 8]
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], window[1] + new, kind, vl.CE_RES, variant, window)
                for new in (8, 400):
                    for epi in (vl.CE_RES_ACC, vl.CE_RES_ACC_DIV):
                        for window in (("start", 64, -64), ("mid", 64, 37)):
                            n += 1
                            amp_case(dr, ledger, pair, vl.BATCHES[n % 4], 64 + new, "n1", epi, variant, window)
    ledger.close()


@pytest.mark.parametrize("ks_index", [0, 1, 2])
@pytest.mark.parametrize("stage", [2, 3])
def test_persistent_kernels_walk_over_several_tiles_per_workgroup(draws, conf_var, stage, ks_index):
    """amp_pair16_kernel / amp_pair8_kernel with at least three times as many tiles as workgroups - read back from the launch, not
    assumed: every workgroup walks over at least two tiles (the next tile's rows travel under the current tile's convs)."""
    dr, ledger = draws("seed1235"), vl.Ledger("seed1235")
    pair = next(p for p in vl.pairs(conf_var) if p[0] == stage and p[1] == ks_index and p[2] == ks_index)
    B, L = (48, 12000) if stage == 2 else (64, 16000)         # (the C = 8 kernel fits four workgroups per CU: 1,024 of them)
    info = amp_case(dr, ledger, pair, B, L, "n1", vl.CE_RES_ACC_DIV, dict())
    print(f"persistent C={pair[3]} ks={pair[4]} d={pair[5]}: {info[2]} tiles on {info[3]} workgroups", flush=True)
    assert info[3] > 0 and info[2] >= 3 * info[3], info
    ledger.close()


# ---------------------------------------------------------------------------------------------- conv_pre, upsamplers, conv_post
@pytest.mark.parametrize("draw", vl.DRAWS)
def test_conv_pre_upsamplers_conv_post_against_float64(draws, conf_var, draw):
    dr, ledger, n = draws(draw), vl.Ledger(draw), 0
    vcfg = conf_var["vocoder_config"]

    def cases(TT, ks):
        for L in vl.lengths(TT, ks, 1):
            yield L, "n1"
        for kind in vl.INPUTS[1:]:
            for L in (TT, 2 * TT + 1):
                yield L, kind

    with torch.no_grad():
        TT = vl.conv_tile_rows(80)
        for L, kind in cases(TT, 7):
            n += 1
            B = vl.BATCHES[n % 4]
            x = vl.make_input(kind, B, 80, L, TT, seed_of(draw, "pre", L, kind))
            out = nan_like((B, L, 128))
            info = dr.layer(KIND_PRE, to_dev(x), out)
            assert info[:2] == [L, 128]
            ledger.add("conv_pre", vl.compare(out.cpu().numpy(), vl.cl(obig.conv_pre(dr.sd, x, torch.float64)), vl.cl(obig.conv_pre(dr.sd, x, torch.float32)),
                                              f"conv_pre B={B} L={L} input={kind}", tile_rows=TT))
        for i, rate in enumerate(vcfg["upsample_rates"]):
            cin = 128 >> i
            TT = vl.conv_tile_rows(cin)                              # rows of the 2-tap view: L + 1 of them, `rate` output rows each
            for rows, kind in cases(TT, 2):
                L = rows - 1
                if L < 1:
                    continue
                n += 1
                B = vl.BATCHES[n % 4]
                x = vl.make_input(kind, B, cin, L, TT - 1, seed_of(draw, "up", i, L, kind))
                out = nan_like((B, rows * rate, cin // 2))
                info = dr.layer(KIND_UP, to_dev(x), out, stage=i)
                assert info[:2] == [rows * rate, cin // 2]
                ledger.add(f"up{i}", vl.compare(out.cpu().numpy(), vl.cl(obig.upsample(dr.sd, vcfg, i, x, torch.float64)),
                                                vl.cl(obig.upsample(dr.sd, vcfg, i, x, torch.float32)),
                                                f"upsampler {i} B={B} L={L} input={kind}", tile_rows=TT * rate))
        TT = vl.POST_TILE_ROWS
        for L, kind in cases(TT, 7):
            for length, div in ((L, 1.0), (L + 50, 32768.0), (max(1, L - 3), 32768.0), (max(1, L // 2), 0.95)):
                n += 1
                B = vl.BATCHES[n % 4]
                x = vl.make_input(kind, B, 8, L, TT, seed_of(draw, "post", L, kind))
                n_out = min(length, L)
                out = nan_like((B, n_out))
                info = dr.layer(KIND_POST, to_dev(x), out, length=length, div=div)
                assert info[:2] == [n_out, 1]
                r64 = obig.conv_post(dr.sd, x, length, torch.float64)[:, 0].numpy() / np.float64(np.float32(div))
                r32 = (obig.conv_post(dr.sd, x, length, torch.float32)[:, 0].numpy() / np.float32(div)).astype(np.float64)
                ledger.add("conv_post", vl.compare(out.cpu().numpy(), r64, r32, f"conv_post B={B} L={L} length={length} div={div} input={kind}",
                                                   tile_rows=TT))
    ledger.close()


# ---------------------------------------------------------------------------------------------- the whole chain, with seams
@pytest.mark.parametrize("B,T", [(8, 130), (3, 257)])
@pytest.mark.parametrize("draw", vl.NARROW_DRAWS)
def test_whole_chain_taps_and_waveform_against_float64(draws, conf_var, draw, B, T):
    """All nine taps and the waveform at sizes where every stage has several tiles per item (the golden fixtures are below one tile
    at C = 64).  Only the narrow draws: through four stages the float32 oracle of the wide draw is itself 1e-2 from the float64 one."""
    dr, ledger = draws(draw), vl.Ledger(draw)
    vcfg = conf_var["vocoder_config"]
    rng = np.random.default_rng(seed_of(draw, B, T))
    mel = torch.from_numpy((-4 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32))
    t64, t32 = {}, {}
    w64 = obig.forward(dr.sd, vcfg, mel, 10 ** 9, dtype=torch.float64, taps=t64)
    w32 = obig.forward(dr.sd, vcfg, mel, 10 ** 9, dtype=torch.float32, taps=t32)
    mel_cl = to_dev(mel)
    ws, nws = dr.eng.workspace(B, T)
    names = ["conv_pre"] + [f"{k}{i}" for i in range(4) for k in ("up", "stage")]
    for which, nm in enumerate(names):
        n = ctypes.c_int64()
        dr.abi.check(dr.lib.bvc_test_vocoder_tap(dr.eng.handle, dr.abi.ptr(mel_cl), B, T, which, None, ctypes.byref(n), ws, nws, dr.eng.stream()))
        out = nan_like((B, n.value))
        dr.abi.check(dr.lib.bvc_test_vocoder_tap(dr.eng.handle, dr.abi.ptr(mel_cl), B, T, which, dr.abi.ptr(out), ctypes.byref(n), ws, nws,
                                                 dr.eng.stream()))
        torch.cuda.synchronize()
        r64 = vl.cl(t64[nm])
        ledger.add(f"chain/{nm}", vl.compare(out.cpu().numpy().reshape(r64.shape), r64, vl.cl(t32[nm]), f"chain tap {nm} B={B} T={T}"))
    wav = dr.model.vocoder(mel.to(DEV), 10 ** 9)
    assert wav.shape == w64.shape
    ledger.add("chain/waveform", vl.compare(wav[:, 0].cpu().numpy(), w64[:, 0].numpy(), w32[:, 0].numpy(), f"chain waveform B={B} T={T}"))
    ledger.close()
