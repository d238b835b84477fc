"""Symmetric layers on the GPU: every symmetric AMP pair, conv_pre, upsampler and conv_post one launch at a time against the
float64 oracle (oracle/bigvgan.py) with the project's bar, vocoder_layers.compare: e_hip = max|hip - oracle64| <= 8 x
max(e32, 2^-24 max|oracle64|); the three reference fixtures through BigVGAN.forward and the facade's decode; batch invariance; the
refusals of everything that counts on a causal generator; and the tile cuts of a causal model beside the symmetric ones.
Measured ratios: profiles/symmetric_parity.md.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_generator as gg
import vocoder_layers as vl
from gpu_generator import DEV, H_DIM, KIND_AMP, KIND_PRE, KIND_UP, amp_case, nan_like, seed_of, to_dev
from oracle import bigvgan as obig

pytestmark = pytest.mark.gpu

CAUSAL = "causal"                            # the shipped switches (all off), for the last test


def make_model(directory, tag, draw):
    return gg.Model(directory, draw, tag, switches=None if tag == CAUSAL else vl.SYM_CONFIGS[tag], h_dim=H_DIM)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """models(tag, draw): the product model of one of vl.SYM_CONFIGS (or the shipped switches) and one generator draw."""
    directory = str(tmp_path_factory.mktemp("symmetric"))
    get, close = gg.cached(lambda tag, draw: make_model(directory, tag, draw))
    yield lambda tag, draw="seed1235": get(tag, draw)
    close()


def check_fixture(mo, tag):
    gg.check_fixture(mo, f"g11_bigvgan_sym_{tag}", tag, ("stage0", "stage1", "stage2", "stage3"), rms_bar=1e-4)


# ----------------------------------------------------------------------------------------------- 1. symmetric AMP pairs
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_symmetric_amp_pairs_against_float64(models, stage):
    """The nine (ks, d) pairs of the stage, each with one of the three epilogues (rotating, so that every (C, epilogue) occurs; the
    running sums aliased to the output), at every length of amp_lengths - signals shorter than the reach on both sides at once,
    both sides of every seam, the last tile's end anywhere - with N(0, 36) input, the draws and B in {2, 3} rotating; and the
    inputs whose only non-zero row is the first, the last or the second tile's first, and zeros.  The items of a batch lie back to
    back: the rows right behind item b's end are item b + 1's, so a missing zero at the end shows."""
    conf = models("all").conf
    ledgers = {draw: vl.Ledger(draw) for draw in vl.DRAWS}
    n = 0
    for q, pair in enumerate(p for p in vl.pairs(conf) if p[0] == stage):
        C, ks, d = pair[3:6]
        TT = vl.amp_tile_rows(C, ks, d, 10 ** 6, False, form="symmetric")[0]
        assert TT == vl.SYM_TILE_HEIGHT[C] - (ks - 1)
        h = vl.reach(ks, d)
        epi = (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(q + stage) % 3]
        for L in vl.sym_amp_lengths(TT, ks, d):
            n += 1
            draw = vl.DRAWS[n % 4]
            amp_case(models("all", draw), ledgers[draw], pair, 2 + (n // 4) % 2, L, "n6", epi)
        for kind in ("row_first", "row_last", "row_tile2", "zeros"):
            for L in (1, h + 1, TT + 1, 2 * TT + 1):
                n += 1
                draw = vl.DRAWS[n % 4]
                amp_case(models("all", draw), ledgers[draw], pair, 2 + (n // 4) % 2, L, kind, epi)
    for ledger in ledgers.values():
        ledger.close()


def test_every_channel_count_meets_every_epilogue(models):
    gg.every_channel_count_meets_every_epilogue(models("all").conf)


# ----------------------------------------------------------------------------------------------- 2. conv_pre, upsamplers, conv_post
def seams(tile):
    return (1, 3, 4, 7, tile - 1, tile, tile + 1, 2 * tile + 5)


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_symmetric_conv_pre_against_float64(models, draw):
    mo, ledger = models("all", draw), vl.Ledger(draw)
    tile = vl.conv_tile_rows(80)
    for n, L in enumerate(seams(tile)):
        B = 2 + n % 2
        x = vl.make_input("n6", B, 80, L, tile, seed_of(draw, "pre", L))
        out = nan_like(B, L, 128)
        assert mo.layer(KIND_PRE, to_dev(x), out)[:2] == [L, 128]
        with torch.no_grad():
            r64, r32 = vl.cl(obig.conv_pre(mo.sd, x, torch.float64, sym=True)), vl.cl(obig.conv_pre(mo.sd, x, torch.float32, sym=True))
        ledger.add("conv_pre/symmetric", vl.compare(out.cpu().numpy(), r64, r32, f"symmetric conv_pre B={B} L={L}", tile_rows=tile))
    ledger.close()


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_symmetric_upsamplers_against_float64(models, stage):
    """Output rows = L * rate: the view of the causal rows that the stage works on, against conv_transpose1d(padding = u / 2)."""
    conf = models("all").conf
    v = conf["vocoder_config"]
    cin, rate = v["upsample_initial_channel"] >> stage, v["upsample_rates"][stage]
    tile = vl.conv_tile_rows(cin)
    ledgers = {draw: vl.Ledger(draw) for draw in vl.DRAWS}
    for n, L in enumerate(seams(tile)):
        draw, B = vl.DRAWS[n % 4], 2 + (n // 4) % 2
        mo = models("all", draw)
        x = vl.make_input("n6", B, cin, L, tile, seed_of(draw, "up", stage, L))
        out = nan_like(B, L * rate, cin // 2)
        assert mo.layer(KIND_UP, to_dev(x), out, stage)[:2] == [L * rate, cin // 2]
        with torch.no_grad():
            r64, r32 = vl.cl(obig.upsample(mo.sd, v, stage, x, torch.float64, sym=True)), vl.cl(obig.upsample(mo.sd, v, stage, x, torch.float32, sym=True))
        assert r64.shape == (B, L * rate, cin // 2)
        ledgers[draw].add(f"upsample{cin}/symmetric", vl.compare(out.cpu().numpy(), r64, r32, f"symmetric upsampler {stage} B={B} L={L}",
                                                                  tile_rows=tile * rate))
    for ledger in ledgers.values():
        ledger.close()


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_symmetric_conv_post_against_float64(models, draw):
    mo, ledger = models("all", draw), vl.Ledger(draw)
    gg.conv_post_sweep(mo, ledger, "symmetric", (1, 3, 4, 255, 256, 257, 600), (4, 257), ("n6", "row_first", "row_last", "row_tile2", "zeros"))
    ledger.close()


# ----------------------------------------------------------------------------------------------- 3. the reference's run
@pytest.mark.parametrize("tag", sorted(vl.SYM_CONFIGS))
def test_reference_fixture_through_forward_and_decode(models, tag):
    """BigVGAN.forward against the reference's waveform (rms <= 1e-4) and stage taps (<= 2e-5), the bars test_gpu_parity.py has for
    g5.  The fixture starts at the mel, so the facade's decode is held against forward on the mel its own coder decodes, with the
    waveform bar; the waveforms are min(length, generator_length(T)) samples long, with and without lost frames."""
    from bvcodec import config
    from bvcodec.model import SCALING
    mo = models(tag)
    check_fixture(mo, tag)
    rng = np.random.default_rng(3)
    codes = torch.from_numpy(rng.integers(0, 2, size=(2, 12, 64)).astype(np.float32)).to(DEV)
    n = min(3000, config.generator_length(mo.conf, 12))
    assert mo.eng.vocoder_length(12) == config.generator_length(mo.conf, 12) == vl.sym_lengths(mo.conf["vocoder_config"], 12)[-1]
    wav = mo.model.decode(codes, 3000)
    mel, _ = mo.model.bvrnn.decode(codes, torch.zeros(1, 2, H_DIM, device=DEV))
    ref = mo.model.vocoder(mel, 3000, _scale_div=float(SCALING), _time_major=True)[:, 0]
    assert wav.shape == (2, n) and bool(torch.isfinite(wav).all())
    rms = float((wav - ref).pow(2).mean().sqrt())
    print(f"FIXTURE {tag}: decode against forward on its own mel, rms {rms:.3e}, equal bits {torch.equal(wav, ref)}")
    assert rms <= 1e-4
    lost = torch.zeros(2, 12, dtype=torch.bool, device=DEV)
    lost[0, 5:7] = True
    lost[1, 11] = True
    wav_l = mo.model.decode(codes, 3000, lost=lost, bitrate=3000)
    assert wav_l.shape == (2, n) and bool(torch.isfinite(wav_l).all())


# ----------------------------------------------------------------------------------------------- 4. invariance
def test_item_of_a_batch_equals_the_item_alone(models):
    """64 + 3 frames: workgroups serve several tiles and items from stage 0 on; an all-symmetric generator makes 256 T samples."""
    mo = models("all")
    rng = np.random.default_rng(4)
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((5, 80, 67))).astype(np.float32)).to(DEV)
    full = mo.model.vocoder(mel, 10 ** 9)
    assert full.shape == (5, 1, 256 * 67) and bool(torch.isfinite(full).all())
    assert torch.equal(mo.model.vocoder(mel, 10 ** 9), full)
    for b in (0, 3, 4):
        assert torch.equal(mo.model.vocoder(mel[b:b + 1].contiguous(), 10 ** 9), full[b:b + 1]), b


# ----------------------------------------------------------------------------------------------- 5. refusals
def refusals(mo, word):
    from bvcodec.streaming import StreamingCodec, StreamingDecoder, VocoderStream
    with pytest.raises(ValueError, match=word):
        StreamingCodec(mo.model, 2, 3000)
    with pytest.raises(ValueError, match=word):
        StreamingCodec(mo.model, 2, 3000, direction="recv")
    with pytest.raises(ValueError, match=word):
        StreamingDecoder(mo.model, 2)
    with pytest.raises(ValueError, match=word):
        StreamingDecoder(mo.model, 2, incremental=False)
    with pytest.raises(ValueError, match=word):
        VocoderStream(mo.eng, 2, 4)
    codes = torch.full((2, 12, 64), 0.5, device=DEV)
    with pytest.raises(ValueError, match=word):
        mo.model.decode(codes, 3000, frames=[12, 7])
    with pytest.raises(ValueError, match=word):
        mo.model.decode(codes, [3000, 2000])
    with pytest.raises(ValueError, match=word):
        mo.model.decode_many([codes[0], codes[1, :7]], 3000)
    n = min(3000, mo.eng.vocoder_length(12))
    assert [tuple(w.shape) for w in mo.model.decode_many([codes[0], codes[1]], 3000, max_batch=1)] == [(n,), (n,)]
    # the library itself: BVC_EINVAL (-1) from the entry points under those classes, and from the windowed test entry
    h = ctypes.c_void_p()
    w = word.encode()
    assert mo.lib.bvc_vocoder_stream_create(mo.eng.handle, 2, 4, ctypes.byref(h)) == -1 and w in mo.lib.bvc_last_error()
    assert mo.lib.bvc_stream_codec_create(mo.eng.handle, 2, 441, 35.0, 0.95, 0.95, ctypes.byref(h)) == -1 and w in mo.lib.bvc_last_error()
    x = torch.zeros(2, 40, 64, device=DEV)
    rc, _ = mo.layer_rc(KIND_AMP, x, torch.empty_like(x), 0, 0, 0, window=(0, 0))
    assert rc == -1 and w in mo.lib.bvc_last_error()
    ws, nws = mo.eng.workspace(2, 12)
    frames = torch.tensor([12, 7], device=DEV)
    lens = torch.tensor([3000, 2000], device=DEV)
    wav = torch.zeros(2, 3000, device=DEV)
    rc = mo.lib.bvc_decode_ragged(mo.eng.handle, mo.abi.ptr(codes), ctypes.c_void_p(frames.data_ptr()), 2, 12, ctypes.c_void_p(lens.data_ptr()),
                                  3000, 1.0, mo.abi.ptr(wav),
                                  ws, nws, mo.eng.stream())
    assert rc == -1 and w in mo.lib.bvc_last_error()


def test_everything_causal_is_refused_and_offline_decode_goes_on(models):
    mo = models("mixed")
    refusals(mo, "symmetric")
    # a send-only session needs no generator
    from bvcodec.streaming import StreamingCodec
    StreamingCodec(mo.model, 2, 3000, direction="send")
    check_fixture(mo, "mixed")                                            # a following offline call is untouched


def test_a_filtered_and_symmetric_generator_keeps_the_filtered_text(models):
    mo = models("with_aa")
    refusals(mo, "anti-aliased")
    check_fixture(mo, "with_aa")


def test_an_unfused_library_refuses_a_symmetric_stage(tmp_path, monkeypatch):
    """BVC_UNFUSED_AMP runs the pairs as two plain causal convolutions: a symmetric stage is refused at creation, like a filtered one."""
    from bvcodec import _abi
    monkeypatch.setenv("BVC_UNFUSED_AMP", "1")
    with pytest.raises(_abi.BvcError, match="symmetric stages run in the fused AMP kernels only"):
        make_model(str(tmp_path), "mixed", "seed1235")


# ----------------------------------------------------------------------------------------------- 6. causal tile cuts
def test_a_causal_model_keeps_its_tile_cuts(models):
    """A causal model of the same draw, created after the symmetric ones in the same process: one AMP pair per stage launches what
    vl.amp_tile_rows predicts - the persistent C = 16 kernel, the full-tile C = 8 kernel - and meets the float64 oracle."""
    models("all"), models("mixed")
    mo = models(CAUSAL)
    ledger = vl.Ledger(mo.draw)
    families = []
    for stage in range(4):
        pair = next(p for p in vl.pairs(mo.conf) if p[0] == stage and p[4] == 7 and p[5] == 3)
        i, j, m, C, ks, d, pre = pair
        B, L = 3, 700
        TT, family = vl.amp_tile_rows(C, ks, d, L, False, height=mo.planned_height(L, B, ks))
        families.append(family.split("/")[1] if C in (16, 8) else family)
        x = vl.make_input("n6", B, C, L, TT, seed_of("causal", stage))
        out = nan_like(B, L, C)
        info = mo.layer(KIND_AMP, to_dev(x), out, i, j, m)
        tiles = B * -(-L // TT)
        assert info[:3] == [L, C, tiles] and info[4] == TT, (family, info, tiles, TT)
        if C in (64, 32):
            assert info[3] == (tiles + 7) // 8 * 8, (family, info)
        with torch.no_grad():
            r64 = vl.cl(vl.oracle_pair(mo.sd, pair, x, torch.float64))
            r32 = vl.cl(vl.oracle_pair(mo.sd, pair, x, torch.float32))
        ledger.add(family, vl.compare(out.cpu().numpy(), r64, r32, f"causal amp pair stage {stage} beside symmetric models", tile_rows=TT))
    assert families[2:] == ["persistent", "full<2,2>"], families
    ledger.close()
