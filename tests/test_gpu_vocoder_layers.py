"""The generator's kernels one layer at a time against the float64 oracle (bvc_test_vocoder_layer runs ONE launch of the path on a
given input): every AMP pair (C, ks, dilation) x epilogue x tile shape - the four compiled C = 64 heights and the planned one, the
persistent C = 16 and C = 8 kernels and the generic kernel behind their options, the streaming window shapes - at lengths on both
sides of every tile seam, on four weight draws (one with alpha, beta ~ N(0, 1)); conv_pre, the upsamplers and conv_post the same
way; the whole chain at sizes with seams.  Every element, maximum norm: e_hip = max|hip - oracle64| <= MARGIN x max(e32,
2^-24 max|oracle64|) with e32 = max|oracle32 - oracle64| on the identical input (vocoder_layers.compare; DESIGN.md section 2;
measured ratios in profiles/vocoder_layer_parity.md).  Every AMP case also asserts that the launch was cut into the tiles this file
assumes.  Needs the MI355X: run with ``-m gpu``."""
import contextlib

import numpy as np
import pytest
import torch

import gpu_generator as gg
import vocoder_layers as vl
from gpu_generator import KIND_POST, KIND_PRE, KIND_UP, amp_case, nan_like, seed_of, to_dev
from oracle import bigvgan as obig

pytestmark = pytest.mark.gpu

DEV = gg.DEV


@pytest.fixture(scope="module")
def draws(tmp_path_factory):
    """draws(name): the shipped model with the generator of one weight draw."""
    directory = str(tmp_path_factory.mktemp("vocoder_layers"))
    get, close = gg.cached(lambda name: gg.Model(directory, name))
    yield get
    close()


# ---------------------------------------------------------------------------------------------- one AMP pair
def amp_variants(C):
    if C == 64:
        return [dict(height=h) for h in vl.AMP_HEIGHTS[64]] + [dict()]             # each compiled height forced, and the planned one
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
            TT = vl.amp_tile_rows(C, ks, d, 10 ** 6, False, **variant)[0]
            with options(dr, variant):
                for L in vl.lengths(TT, ks, d):
                    n += 1
                    amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, "n1", vl.CE_RES, **variant)
                for kind in vl.INPUTS[1:]:
                    for L in (TT, 2 * TT + 1, 3 * TT + 17):
                        n += 1
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, kind, vl.CE_RES, **variant)
                for epi in (vl.CE_RES_ACC, vl.CE_RES_ACC_DIV):
                    for L in (TT, 2 * TT + 1):
                        n += 1
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], L, "n1", epi, **variant)
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
                        amp_case(dr, ledger, pair, vl.BATCHES[n % 4], window[1] + new, kind, vl.CE_RES, window, **variant)
                for new in (8, 400):
                    for epi in (vl.CE_RES_ACC, vl.CE_RES_ACC_DIV):
                        for window in (("start", 64, -64), ("mid", 64, 37)):
                            n += 1
                            amp_case(dr, ledger, pair, vl.BATCHES[n % 4], 64 + new, "n1", epi, window, **variant)
    ledger.close()


@pytest.mark.parametrize("ks_index", [0, 1, 2])
@pytest.mark.parametrize("stage", [2, 3])
def test_persistent_kernels_walk_over_several_tiles_per_workgroup(draws, conf_var, stage, ks_index):
    """amp_pair16_kernel / amp_pair8_kernel with at least three times as many tiles as workgroups - read back from the launch, not
    assumed: every workgroup walks over at least two tiles (the next tile's rows travel under the current tile's convs)."""
    dr, ledger = draws("seed1235"), vl.Ledger("seed1235")
    pair = next(p for p in vl.pairs(conf_var) if p[0] == stage and p[1] == ks_index and p[2] == ks_index)
    B, L = (48, 12000) if stage == 2 else (64, 16000)         # (the C = 8 kernel fits four workgroups per CU: 1,024 of them)
    info = amp_case(dr, ledger, pair, B, L, "n1", vl.CE_RES_ACC_DIV)
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
            out = nan_like(B, L, 128)
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
                out = nan_like(B, rows * rate, cin // 2)
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
                out = nan_like(B, n_out)
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
    for which, nm in enumerate(gg.TAPS):
        out = dr.tap(mel_cl, which)
        r64 = vl.cl(t64[nm])
        ledger.add(f"chain/{nm}", vl.compare(out.cpu().numpy().reshape(r64.shape), r64, vl.cl(t32[nm]), f"chain tap {nm} B={B} T={T}"))
    wav = dr.model.vocoder(mel.to(DEV), 10 ** 9)
    assert wav.shape == w64.shape
    ledger.add("chain/waveform", vl.compare(wav[:, 0].cpu().numpy(), w64[:, 0].numpy(), w32[:, 0].numpy(), f"chain waveform B={B} T={T}"))
    ledger.close()
