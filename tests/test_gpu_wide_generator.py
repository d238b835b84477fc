"""Wide generators (``upsample_initial_channel`` 256 and 512) on the GPU.  The AMP pairs of the wide stages (C = 256, 128) one launch
at a time against the float64 oracle, offline and in streaming windows, with the project's bar, vocoder_layers.compare: e_hip =
max|hip - oracle64| <= 8 x max(e32, 2^-24 max|oracle64|); conv_pre, the upsamplers out of 512 / 256 / 128 / 64 channels and conv_post
from 16 / 32 channels the same way; the reference's own run (tests/golden/g12_bigvgan_wide_*.npz); the whole chain with seams; the
facade, mixed-length batches and the streaming classes with the assertions the shipped width is held to; and what stays refused.
Every AMP case also asserts that the launch was cut into the tiles tests/vocoder_layers.py restates.  Measured ratios:
profiles/wide_generator_parity.md.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_generator as gg
import vocoder_layers as vl
from gpu_generator import DEV, H_DIM, KIND_AMP, KIND_POST, KIND_PRE, KIND_UP, amp_case, nan_like, seed_of, to_dev
from oracle import bigvgan as obig

pytestmark = pytest.mark.gpu

WIDE_STAGES = ((256, 0), (512, 0), (512, 1))                 # (width, stage): C = 128, 256, 128
T_, F_ = True, False
# symmetric and filtered narrow stages (C <= 64) behind the causal wide ones, per width
MIXED = {256: dict(layers_sym=[F_, T_, F_, T_], layers_antialias=[F_, F_, T_, F_], post_sym=True),
         512: dict(layers_sym=[F_, F_, T_, F_], layers_antialias=[F_, F_, F_, T_], antialias_post=True)}


def make_model(directory, width, draw="seed1235", tag="causal", h_dim=H_DIM):
    return gg.Model(directory, draw, f"wide{width}_{tag}_{h_dim}", width=width, switches=None if tag == "causal" else MIXED[width], h_dim=h_dim)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """models(width, draw, tag, h_dim): the product model of one width, one set of switches and one generator draw."""
    directory = str(tmp_path_factory.mktemp("wide_generator"))
    get, close = gg.cached(lambda *key: make_model(directory, *key))
    yield lambda width, draw="seed1235", tag="causal", h_dim=H_DIM: get(width, draw, tag, h_dim)
    close()


# ----------------------------------------------------------------------------------------------- 1, 2. one AMP pair of a wide stage
def wide_pairs(mo, stage, block):
    return [p for p in vl.pairs(mo.conf) if p[0] == stage and p[1] == block]


@pytest.mark.parametrize("block", [0, 1, 2])
@pytest.mark.parametrize("draw", ["seed1235", "wide"])
@pytest.mark.parametrize("width,stage", WIDE_STAGES)
def test_wide_amp_pairs_offline_against_float64(models, width, stage, draw, block):
    """The three dilations of one AMP block (ks = 3, 7, 11 by block) of a wide stage.  B = 3, N(0, 1) input, the residual epilogue:
    every length of vl.lengths - 1, 2, both halo depths, TT - 1, TT, TT + 1, 2 TT, 2 TT + 1, 3 TT + 17; the seam length 2 TT + 1 at
    B = 2, 5, 9 (tile counts that are no multiples of 8: the padded grid and the per-XCD renumbering); at TT + 1 the other inputs
    (N(0, 36), zeros, one non-zero row at row 0 / the last row / the second tile's first); the two accumulating epilogues, the
    running sum aliased to the output, at TT and 2 TT + 1; and the other compiled tile height on both sides of its seams."""
    mo, ledger = models(width, draw), vl.Ledger(draw)
    for pair in wide_pairs(mo, stage, block):
        C, ks, d = pair[3:6]
        assert C in vl.WIDE_CHANNELS
        TT = vl.amp_tile_rows(C, ks, d, 10 ** 6, False)[0]
        assert TT == vl.AMP_HEIGHT[C] - (ks - 1)
        for L in vl.lengths(TT, ks, d):
            amp_case(mo, ledger, pair, 3, L, "n1", vl.CE_RES)
        for B in (2, 5, 9):
            amp_case(mo, ledger, pair, B, 2 * TT + 1, "n1", vl.CE_RES)
        for kind in vl.INPUTS[1:]:
            amp_case(mo, ledger, pair, 3, TT + 1, kind, vl.CE_RES)
        for epi in (vl.CE_RES_ACC, vl.CE_RES_ACC_DIV):
            for L in (TT, 2 * TT + 1):
                amp_case(mo, ledger, pair, 3, L, "n1", epi)
        other = vl.AMP_HEIGHTS[C][1]
        for n, L in enumerate((other - (ks - 1), other - (ks - 1) + 1, 2 * (other - (ks - 1)) + 1)):
            amp_case(mo, ledger, pair, (3, 5, 2)[n], L, "n6", (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[n], height=other)
    ledger.close()


@pytest.mark.parametrize("draw", ["seed1235", "wide"])
@pytest.mark.parametrize("width,stage", WIDE_STAGES)
def test_wide_amp_pairs_in_streaming_windows_against_float64(models, width, stage, draw):
    """window = 1, row_begin = 64 (what a hop keeps): 1, 8, one short tile, one short tile + 1 and 129 new rows - the short-tile and
    the tall-tile choice at each wide width - with t_origin 0 and 37 ('mid': the buffer is rows [t_origin, t_origin + L) of a longer
    signal) and -64 ('start': global time 0 is the first new row, the S2 rows before it are zero).  Inputs, epilogues and B rotate."""
    mo, ledger, n = models(width, draw), vl.Ledger(draw), 0
    for pair in [p for p in vl.pairs(mo.conf) if p[0] == stage]:
        C, ks, d = pair[3:6]
        families = set()
        for new in vl.wide_window_new_rows(ks):
            for window in (("start", 64, -64), ("mid", 64, 0), ("mid", 64, 37)):
                n += 1
                kind = ("n1", "n6", "row_first", "n1", "zeros", "row_tile2", "n1", "row_last")[n % 8]
                epi = (vl.CE_RES, vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(n // 3) % 4]
                amp_case(mo, ledger, pair, vl.BATCHES[n % 4], 64 + new, kind, epi, window)
            families.add(vl.amp_tile_rows(C, ks, d, new, True)[1])
        assert families == {f"amp{C}/window32", f"amp{C}/{vl.AMP_HEIGHT[C]}/window"}, families
    ledger.close()


def test_a_wide_pair_refuses_rows_beyond_its_index(models):
    """rows_load4's byte offset is a 32-bit integer: the host refuses L + 512 > 2^31 / (4 C) before anything is launched (the
    buffers are never touched, so small ones do)."""
    for width, stage in WIDE_STAGES[1:]:
        mo = models(width)
        C = vl.stage_channels(mo.conf)[stage]
        x = torch.zeros(1, 8, C, device=DEV)
        info = (ctypes.c_int64 * 5)()
        L = vl.max_rows(C) + 1
        rc = mo.lib.bvc_test_vocoder_layer(mo.eng.handle, KIND_AMP, stage, 0, 0, mo.abi.ptr(x), 1, L, mo.abi.ptr(x), 1, None, 0, 0, 0, 0, 1.0,
                                           info, mo.eng.stream())
        assert rc == -1 and b"row index" in mo.lib.bvc_last_error(), (C, L, rc, mo.lib.bvc_last_error())


# ----------------------------------------------------------------------------------------------- 3. conv_pre, upsamplers, conv_post
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_wide_conv_pre_and_upsamplers_against_float64(models, width):
    """conv_pre 80 -> width and every upsampler of the model (out of 256 / 128 / 64 / 32 channels, or 512 / 256 / 128 / 64) at
    L = 1, 6, 63, 64, 65, 129 input rows - both sides of the 64-row tiles of the 512-channel upsampler and of the 128-row ones."""
    ledgers = {draw: vl.Ledger(draw) for draw in ("seed1235", "wide")}
    n = 0
    for L in (1, 6, 63, 64, 65, 129):
        n += 1
        draw, B = ("seed1235", "wide")[n % 2], 2 + n % 2
        mo = models(width, draw)
        vcfg = mo.conf["vocoder_config"]
        x = vl.make_input("n6" if n % 3 else "n1", B, 80, L, 128, seed_of(draw, width, "pre", L))
        out = nan_like(B, L, width)
        assert mo.layer(KIND_PRE, to_dev(x), out)[:2] == [L, width]
        with torch.no_grad():
            r64, r32 = vl.cl(obig.conv_pre(mo.sd, x, torch.float64)), vl.cl(obig.conv_pre(mo.sd, x, torch.float32))
        ledgers[draw].add(f"conv_pre/{width}", vl.compare(out.cpu().numpy(), r64, r32, f"conv_pre width {width} B={B} L={L}", tile_rows=128))
        for i, rate in enumerate(vcfg["upsample_rates"]):
            cin = width >> i
            tile = vl.conv_tile_rows(cin)
            x = vl.make_input("n6" if (n + i) % 3 else "n1", B, cin, L, tile - 1, seed_of(draw, width, "up", i, L))
            out = nan_like(B, (L + 1) * rate, cin // 2)
            assert mo.layer(KIND_UP, to_dev(x), out, stage=i)[:2] == [(L + 1) * rate, cin // 2]
            with torch.no_grad():
                r64, r32 = vl.cl(obig.upsample(mo.sd, vcfg, i, x, torch.float64)), vl.cl(obig.upsample(mo.sd, vcfg, i, x, torch.float32))
            ledgers[draw].add(f"up/cin{cin}", vl.compare(out.cpu().numpy(), r64, r32, f"upsampler {i} (cin {cin}) width {width} B={B} L={L}",
                                                         tile_rows=tile * rate))
    for ledger in ledgers.values():
        ledger.close()


@pytest.mark.parametrize("width", vl.WIDTHS)
def test_wide_conv_post_against_float64(models, width):
    """conv_post from 16 and 32 channels: L on both sides of the 256-sample tiles, ``length`` below, equal to and above L."""
    C = width >> 4
    ledgers = {draw: vl.Ledger(draw) for draw in ("seed1235", "wide")}
    n = 0
    for L in (1, 6, 255, 256, 257, 600):
        for length in sorted({max(1, L - 3), L, L + 50}):
            n += 1
            draw, B, div = ("seed1235", "wide")[n % 2], 2 + (n // 2) % 2, (1.0, 32768.0, 0.95)[n % 3]
            mo = models(width, draw)
            kind = ("n6", "n1", "row_first", "row_last", "row_tile2")[n % 5]
            x = vl.make_input(kind, B, C, L, vl.POST_TILE_ROWS, seed_of(draw, width, "post", L, length))
            rows = min(L, length)
            out = nan_like(B, rows)
            assert mo.layer(KIND_POST, to_dev(x), out, length=length, div=div)[:2] == [rows, 1]
            with torch.no_grad():
                r64 = obig.conv_post(mo.sd, x, length, torch.float64)[:, 0].numpy() / np.float64(np.float32(div))
                r32 = (obig.conv_post(mo.sd, x, length, torch.float32)[:, 0].numpy() / np.float32(div)).astype(np.float64)
            ledgers[draw].add(f"conv_post/{C}", vl.compare(out.cpu().numpy(), r64, r32, f"conv_post C={C} B={B} L={L} length={length} div={div} "
                                                           f"input={kind}", tile_rows=vl.POST_TILE_ROWS))
    for ledger in ledgers.values():
        ledger.close()


# ----------------------------------------------------------------------------------------------- 4. the reference's run
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_reference_fixture_taps_and_waveform(models, width):
    """bvc_test_vocoder_tap against the five stored taps (<= 2e-5) and BigVGAN.forward against the stored waveform (rms <= 1e-5):
    the bars test_gpu_parity.py holds the shipped width's fixtures g5 to."""
    g = gg.check_fixture(models(width), f"g12_bigvgan_wide_{width}", f"width {width}", ("conv_pre", "stage0", "stage1", "stage2", "stage3"),
                         rms_bar=1e-5, max_bar=1e-4)
    assert int(g["width"]) == width and int(g["seed"]) == 1235


# ----------------------------------------------------------------------------------------------- 5. the whole chain, with seams
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_wide_whole_chain_taps_and_waveform_against_float64(models, width):
    """All nine taps and the waveform at (B, T) = (3, 130): several tiles per item at every stage (the fixtures are below one)."""
    mo, ledger = models(width), vl.Ledger("seed1235")
    vcfg = mo.conf["vocoder_config"]
    B, T = 3, 130
    rng = np.random.default_rng(seed_of(width, B, T))
    mel = torch.from_numpy((-4 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32))
    t64, t32 = {}, {}
    w64 = obig.forward(mo.sd, vcfg, mel, 10 ** 9, dtype=torch.float64, taps=t64)
    w32 = obig.forward(mo.sd, vcfg, mel, 10 ** 9, dtype=torch.float32, taps=t32)
    mel_cl = to_dev(mel)
    for which, nm in enumerate(gg.TAPS):
        r64 = vl.cl(t64[nm])
        out = mo.tap(mel_cl, which)
        ledger.add(f"chain{width}/{nm}", vl.compare(out.cpu().numpy().reshape(r64.shape), r64, vl.cl(t32[nm]), f"chain tap {nm} width {width} B={B} T={T}"))
    wav = mo.model.vocoder(mel.to(DEV), 10 ** 9)
    assert wav.shape == w64.shape
    ledger.add(f"chain{width}/waveform", vl.compare(wav[:, 0].cpu().numpy(), w64[:, 0].numpy(), w32[:, 0].numpy(), f"chain waveform width {width} B={B} T={T}"))
    ledger.close()


# ----------------------------------------------------------------------------------------------- 6. facade
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_facade_encode_decode(models, tmp_path, width):
    """encode -> decode, B = 3, 1 s: the codes are the same coder's with the shipped generator (the generator does not enter encode);
    the waveform against the oracle's decode, rms < 1e-4 (the facade's bar); forward and forward_fused; lost frames: the filled codes
    are the shipped generator's model's too, and the waveform is the plain decode's of those codes - to the facade's bar, as
    forward_fused against forward: the concealing recurrence sums the coder's layers in another order than the plain one, and the
    generator is a function of the mel alone."""
    from bvcodec import BVRNNCodecModel, config, synth
    from oracle import codec as ocodec
    mo = models(width)
    B, L = 3, 22050
    x = synth.synthetic_speech(B, L, seed=29, kind="speech").to(DEV)
    codes = mo.model.encode(x, 3000)
    cfg128 = str(tmp_path / "shipped.toml")
    with open(cfg128, "w") as f:
        f.write(open(config.DEFAULT_CONFIG).read().replace("h_dim = 1024", f"h_dim = {H_DIM}"))
    conf128 = config.load_config(cfg128)
    p1, p2 = str(tmp_path / "bvrnn"), str(tmp_path / "bigvgan")
    torch.save({"vrnn": mo.vr}, p1)
    torch.save({"generator": synth.generator_state_dict(conf128, 1235)}, p2)
    shipped = BVRNNCodecModel(cfg128, p1, p2).to(DEV)
    assert torch.equal(codes, shipped.encode(x, 3000))
    wav = mo.model.decode(codes, L)
    assert wav.shape == (B, L) and bool(torch.isfinite(wav).all())
    torch.set_num_threads(16)
    oc = ocodec.OracleCodec(mo.conf, mo.vr, mo.sd)
    ref = oc.decode(codes.cpu(), L)
    rms = float((wav.cpu() - ref).pow(2).mean().sqrt())
    print(f"FACADE width {width}: decode against the oracle, rms {rms:.3e}")
    assert rms < 1e-4
    assert torch.equal(mo.model.forward(x, 3000), wav)
    fcodes, fused = mo.model.forward_fused(x, 3000, return_codes=True)
    assert torch.equal(fcodes, codes) and float((fused - wav).pow(2).mean().sqrt()) < 1e-4
    lost = torch.zeros(B, codes.shape[1], dtype=torch.bool, device=DEV)
    lost[0, 5:7] = True
    lost[2, 40] = True
    wav_l, codes_l = mo.model.decode(codes, L, lost=lost, bitrate=3000, return_codes=True)
    assert wav_l.shape == (B, L) and bool(torch.isfinite(wav_l).all())
    assert torch.equal(codes_l, shipped.decode(codes, L, lost=lost, bitrate=3000, return_codes=True)[1])
    again = mo.model.decode(codes_l, L)
    print(f"FACADE width {width}: concealing decode against decode of its filled codes, rms {float((again - wav_l).pow(2).mean().sqrt()):.3e} "
          f"max {float((again - wav_l).abs().max()):.3e}, equal bits {torch.equal(again, wav_l)}")
    assert float((again - wav_l).pow(2).mean().sqrt()) < 1e-4
    shipped.check_status()


# ----------------------------------------------------------------------------------------------- 7. mixed lengths
def test_ragged_decode_equals_single_calls(models):
    """decode(codes, LENGTHS) and decode_many at width 256, rows of 7 / 20 / 33 / 40 frames: each row equals its own single-utterance
    decode bit for bit, zeros behind each row's end (test_gpu_ragged.py's assertions; one order of summation per output)."""
    mo = models(256)
    frames = [7, 20, 33, 40]
    lengths = [256 * f + (0, 13, 100, 255)[b] for b, f in enumerate(frames)]
    rng = np.random.default_rng(41)
    codes = torch.from_numpy(rng.integers(0, 2, size=(4, 40, 64)).astype(np.float32)).to(DEV)
    wav = mo.model.decode(codes, lengths)
    assert wav.shape == (4, max(lengths)) and bool(torch.isfinite(wav).all())
    many = mo.model.decode_many([codes[b, :f] for b, f in enumerate(frames)], lengths)
    for b, (f, n) in enumerate(zip(frames, lengths)):
        one = mo.model.decode(codes[b:b + 1, :f].contiguous(), n)
        assert one.shape == (1, n)
        assert torch.equal(wav[b:b + 1, :n], one), (b, n)
        assert bool((wav[b, n:] == 0).all()), (b, n)
        assert torch.equal(many[b], one[0]), (b, n)


# ----------------------------------------------------------------------------------------------- 8. streaming
@pytest.mark.parametrize("width,B", [(256, 3), (512, 2)])
def test_streaming_codec_equals_offline(models, width, B):
    """StreamingCodec, loopback, 30 hops of 441 samples: codes identical to the offline call, waveform within 2e-6 of it (the bar
    test_gpu_streaming.py holds the shipped width to)."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    mo = models(width)
    hop, hops = 441, 30
    L = hop * hops
    x = synth.synthetic_speech(B, L, seed=23, kind="speech").to(DEV)
    sc = StreamingCodec(mo.model, B, 3000, hop=hop)
    codes, wavs = [], []
    for i in range(hops):
        c, w = sc.push(x[:, i * hop:(i + 1) * hop])
        codes.append(c.clone())
        wavs.append(w.clone())
    torch.cuda.synchronize()
    codes, wav = torch.cat(codes, 1), torch.cat(wavs, 1)
    F = codes.shape[1]
    assert F == (L - 768) // 256 + 1 and wav.shape[1] == 256 * F
    codes_off = mo.model.encode(x, 3000)
    assert torch.equal(codes, codes_off[:, :F])
    wav_off = mo.model.decode(codes_off, L)
    err = (wav - wav_off[:, :256 * F]).abs().max().item()
    print(f"STREAMING width {width}: max |streamed - offline| = {err:.3e}")
    assert err <= 2e-6
    mo.model.check_status()


def test_vocoder_stream_equals_offline_for_any_chunking(models):
    """bvc_vocoder_stream_push at width 256 over ragged chunks == the matching slice of the offline generator."""
    from bvcodec.streaming import VocoderStream
    mo = models(256)
    B, T = 2, 37
    g = torch.Generator().manual_seed(5)
    mel = (torch.randn(B, T, 80, generator=g) * 1.5 - 4.0).to(DEV)
    ref = mo.model.vocoder(mel, 10 ** 12, _time_major=True)[:, 0]
    vs = VocoderStream(mo.eng, B, 5)
    chunks, t = [], 0
    for k in [1, 5, 2, 1, 1, 4, 3, 5, 5, 5, 5]:
        k = min(k, T - t)
        if k == 0:
            break
        chunks.append(vs.push(mel[:, t:t + k].contiguous()))
        t += k
    assert t == T
    wav = torch.cat(chunks, 1)
    assert wav.shape == (B, 256 * T)
    err = (wav - ref[:, :256 * T]).abs().max().item()
    print(f"VOCODER STREAM width 256: max |streamed - offline| = {err:.3e}")
    assert err <= 2e-6


# ----------------------------------------------------------------------------------------------- 9. refusals, and what works beside them
@pytest.mark.parametrize("key", ["layers_sym", "layers_antialias"])
def test_switches_on_a_wide_stage_are_refused(tmp_path, conf_var, key):
    """ValueError from the configuration, BVC_EINVAL from bvc_model_create - with the stage named."""
    from bvcodec import _abi, config, synth, weights
    from bvcodec.model import _Engine
    for width, stage in WIDE_STAGES:
        flags = [k == stage for k in range(4)]
        with pytest.raises(ValueError, match=key):
            vl.write_config(str(tmp_path / f"{key}_{width}_{stage}.toml"), width=width, switches={key: flags}, h_dim=H_DIM)
        # the library itself, handed the tensors such a checkpoint would carry
        conf = vl.with_switches(vl.write_config(str(tmp_path / f"plain_{width}.toml"), width=width, h_dim=H_DIM), {key: flags})
        tensors = weights.host_tensors(conf, synth.bvrnn_state_dict(conf, 1234), synth.generator_state_dict(conf, 1235))
        with pytest.raises(_abi.BvcError, match=f"stage {stage} has {width >> (stage + 1)} channels") as e:
            _Engine(conf, tensors, torch.device(DEV))
        assert key in str(e.value)
    assert config.check_supported(vl.with_switches(conf_var, {key: [True] * 4})) is None


def test_an_unfused_library_refuses_a_wide_stage(tmp_path, monkeypatch):
    from bvcodec import _abi
    monkeypatch.setenv("BVC_UNFUSED_AMP", "1")
    with pytest.raises(_abi.BvcError, match="wide stages run in the fused AMP kernels only"):
        make_model(str(tmp_path), 256)


@pytest.mark.parametrize("width", vl.WIDTHS)
def test_switches_on_the_narrow_stages_of_a_wide_generator(models, width):
    """Symmetric and filtered stages of 64 channels and fewer, a symmetric or filtered conv_post from 16 / 32 channels, behind
    causal wide stages: the waveform and the stage taps against the oracle in float64."""
    mo, ledger = models(width, tag="mixed"), vl.Ledger("seed1235")
    vcfg = mo.conf["vocoder_config"]
    B, T = 2, 40
    rng = np.random.default_rng(seed_of("mixed", width))
    mel = torch.from_numpy((-4 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32))
    t64, t32 = {}, {}
    w64 = obig.forward(mo.sd, vcfg, mel, 10 ** 9, dtype=torch.float64, taps=t64)
    w32 = obig.forward(mo.sd, vcfg, mel, 10 ** 9, dtype=torch.float32, taps=t32)
    mel_cl = to_dev(mel)
    for i in range(4):
        r64 = vl.cl(t64[f"stage{i}"])
        out = mo.tap(mel_cl, 2 + 2 * i)
        ledger.add(f"mixed{width}/stage{i}", vl.compare(out.cpu().numpy().reshape(r64.shape), r64, vl.cl(t32[f"stage{i}"]), f"mixed width {width} stage {i}"))
    wav = mo.model.vocoder(mel.to(DEV), 10 ** 9)
    assert wav.shape == w64.shape
    ledger.add(f"mixed{width}/waveform", vl.compare(wav[:, 0].cpu().numpy(), w64[:, 0].numpy(), w32[:, 0].numpy(), f"mixed waveform width {width}"))
    ledger.close()
    from bvcodec.streaming import VocoderStream
    with pytest.raises(ValueError, match="anti-aliased"):
        VocoderStream(mo.eng, 2, 4)
