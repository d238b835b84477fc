"""Symmetric layers on the GPU: every symmetric AMP pair, conv_pre, upsampler and conv_post one launch at a time against the
float64 oracle (tests/symmetric_oracle.py) with the project's bar, vocoder_layers.compare: e_hip = max|hip - oracle64| <= 8 x
max(e32, 2^-24 max|oracle64|); the three reference fixtures through BigVGAN.forward and the facade's decode; batch invariance; the
refusals of everything that counts on a causal generator; and the tile cuts of a causal model beside the symmetric ones.
Measured ratios: profiles/symmetric_parity.md.  Needs the MI355X: run with ``-m gpu``."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import symmetric_oracle as symo
import vocoder_layers as vl
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIND_PRE, KIND_UP, KIND_AMP, KIND_POST = 0, 1, 2, 3
H_DIM = 64                                   # a small coder: these tests are about the generator
CAUSAL = "causal"                            # the shipped switches (all off), for the last test


class Model:
    """The product model of one configuration and one generator draw on the GPU."""

    def __init__(self, directory, tag, draw):
        from bvcodec import BVRNNCodecModel, _abi, config, synth
        self.tag, self.draw = tag, draw
        cfg = os.path.join(directory, f"{tag}.toml")
        if tag == CAUSAL:
            with open(cfg, "w") as f:
                f.write(open(config.DEFAULT_CONFIG).read().replace("h_dim = 1024", f"h_dim = {H_DIM}"))
            self.conf = config.load_config(cfg)
        else:
            self.conf = symo.write_config(cfg, tag, h_dim=H_DIM)
        self.sd = vl.generator_draw(self.conf, draw)
        self.vr = synth.bvrnn_state_dict(self.conf, 1234)
        p1, p2 = os.path.join(directory, "bvrnn"), os.path.join(directory, f"bigvgan_{tag}_{draw}")
        torch.save({"vrnn": self.vr}, p1)
        torch.save({"generator": self.sd}, p2)
        self.model = BVRNNCodecModel(cfg, p1, p2).to(DEV)
        self.eng = self.model.engine(torch.empty(0, device=DEV))
        self.lib, self.abi = _abi.load(), _abi

    def layer_rc(self, kind, x, out, stage=0, block=0, iteration=0, epi=vl.CE_RES, acc=None, window=0, length=0, div=1.0):
        info = (ctypes.c_int64 * 5)()
        B, L = x.shape[0], x.shape[1]
        rc = self.lib.bvc_test_vocoder_layer(self.eng.handle, kind, stage, block, iteration, self.abi.ptr(x), B, L, self.abi.ptr(out),
                                             epi, self.abi.ptr(acc), window, 0, 0, length, div, info, self.eng.stream())
        return rc, list(info)

    def layer(self, *a, **k):
        rc, info = self.layer_rc(*a, **k)
        self.abi.check(rc)
        return info

    def planned_height(self, rows, B, ks):
        out = (ctypes.c_int64 * 6)()
        self.abi.check(self.lib.bvc_test_tile_plan(1, rows, B, ks, 0, out))
        return int(out[0])


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    directory, cache = str(tmp_path_factory.mktemp("symmetric")), {}

    def get(tag, draw="seed1235"):
        if (tag, draw) not in cache:
            cache[(tag, draw)] = Model(directory, tag, draw)
        return cache[(tag, draw)]
    yield get
    for m in cache.values():
        m.model.check_status()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def to_dev(t):
    return t.permute(0, 2, 1).contiguous().to(DEV)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ----------------------------------------------------------------------------------------------- 1. symmetric AMP pairs
def amp_case(mo, ledger, pair, B, L, kind, epi):
    i, j, m, C, ks, d, pre = pair
    TT = symo.sym_tile_rows(C, ks)
    what = f"symmetric amp pair stage {i} block {j} iteration {m} (C={C} ks={ks} d={d}) epi={epi} B={B} L={L} input={kind}"
    seed = seed_of(mo.draw, i, j, m, B, L, kind, epi)
    x = vl.make_input(kind, B, C, L, TT, seed)
    acc = vl.make_input("n1", B, C, L, TT, seed + 1) if epi >= vl.CE_RES_ACC else None

    def oracle(dtype):
        y = symo.amp_pair(mo.sd, pre, m, x, ks, d, dtype=dtype)
        if epi >= vl.CE_RES_ACC:
            y = acc.to(dtype) + y
        if epi == vl.CE_RES_ACC_DIV:
            y = y / 3
        return vl.cl(y)
    with torch.no_grad():
        r64, r32 = oracle(torch.float64), oracle(torch.float32)
    if acc is None:
        out, acc_dev = nan_like(B, L, C), None
    else:
        out = to_dev(acc)                                            # the running sum IS the output buffer, as in the path
        acc_dev = out
    info = mo.layer(KIND_AMP, to_dev(x), out, i, j, m, epi, acc_dev)
    tiles = B * -(-L // TT)
    assert info == [L, C, tiles, (tiles + 7) // 8 * 8, TT], (what, info, "assumed tiles / rows per tile", tiles, TT)
    ledger.add(f"amp{C}/symmetric", vl.compare(out.cpu().numpy(), r64, r32, what, tile_rows=TT))


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
        TT = symo.sym_tile_rows(C, ks)
        assert TT == symo.SYM_TILE_HEIGHT[C] - (ks - 1)
        h = symo.reach(ks, d)
        epi = (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(q + stage) % 3]
        for L in symo.amp_lengths(TT, ks, d):
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
    conf = models("all").conf
    seen = set()
    for stage in range(4):
        for q, pair in enumerate(p for p in vl.pairs(conf) if p[0] == stage):
            seen.add((pair[3], (q + stage) % 3))
    assert seen == {(C, e) for C in vl.CHANNELS for e in range(3)}


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
            r64, r32 = vl.cl(symo.conv_pre(mo.sd, x, torch.float64)), vl.cl(symo.conv_pre(mo.sd, x, torch.float32))
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
            r64, r32 = vl.cl(symo.upsample(mo.sd, v, stage, x, torch.float64)), vl.cl(symo.upsample(mo.sd, v, stage, x, torch.float32))
        assert r64.shape == (B, L * rate, cin // 2)
        ledgers[draw].add(f"upsample{cin}/symmetric", vl.compare(out.cpu().numpy(), r64, r32, f"symmetric upsampler {stage} B={B} L={L}",
                                                                  tile_rows=tile * rate))
    for ledger in ledgers.values():
        ledger.close()


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_symmetric_conv_post_against_float64(models, draw):
    mo, ledger = models("all", draw), vl.Ledger(draw)
    n = 0
    for L in (1, 3, 4, 255, 256, 257, 600):
        for length in sorted({L, max(1, L - 3), 10 ** 9}):
            for kind in (("n6",) if L not in (4, 257) else ("n6", "row_first", "row_last", "row_tile2", "zeros")):
                n += 1
                B, div = 2 + n % 2, (1.0, 0.95)[n % 2]
                x = vl.make_input(kind, B, 8, L, vl.POST_TILE_ROWS, seed_of(draw, "post", L, length, kind))
                rows = min(L, length)
                out = nan_like(B, rows)
                info = mo.layer(KIND_POST, to_dev(x), out, length=length, div=div)
                assert info[:2] == [rows, 1]
                with torch.no_grad():
                    r64 = symo.conv_post(mo.sd, x, length, torch.float64)[:, 0].numpy() / np.float64(np.float32(div))
                    r32 = (symo.conv_post(mo.sd, x, length, torch.float32)[:, 0].numpy() / np.float32(div)).astype(np.float64)
                ledger.add("conv_post/symmetric", vl.compare(out.cpu().numpy(), r64, r32,
                                                             f"symmetric conv_post B={B} L={L} length={length} div={div} input={kind}",
                                                             tile_rows=vl.POST_TILE_ROWS))
    ledger.close()


# ----------------------------------------------------------------------------------------------- 3. the reference's run
def stage_tap(mo, mel_tm, i):
    B, T = mel_tm.shape[0], mel_tm.shape[1]
    ws, nws = mo.eng.workspace(B, T)
    n = ctypes.c_int64()
    mo.abi.check(mo.lib.bvc_test_vocoder_tap(mo.eng.handle, mo.abi.ptr(mel_tm), B, T, 2 + 2 * i, None, ctypes.byref(n), ws, nws, mo.eng.stream()))
    out = nan_like(B, n.value)
    mo.abi.check(mo.lib.bvc_test_vocoder_tap(mo.eng.handle, mo.abi.ptr(mel_tm), B, T, 2 + 2 * i, mo.abi.ptr(out), ctypes.byref(n), ws, nws,
                                             mo.eng.stream()))
    torch.cuda.synchronize()
    return out


def check_fixture(mo, tag):
    g = load_golden(f"g11_bigvgan_sym_{tag}")
    mel = torch.from_numpy(g["mel"]).to(DEV)
    wav = mo.model.vocoder(mel, 10 ** 9).cpu().numpy()
    assert wav.shape == g["wav"].shape
    rms = float(np.sqrt(((wav - g["wav"]) ** 2).mean()))
    print(f"FIXTURE {tag}: waveform rms error {rms:.3e} max {np.abs(wav - g['wav']).max():.3e}")
    assert rms <= 1e-4
    mel_tm = mel.permute(0, 2, 1).contiguous()
    for i in range(4):
        ref = g[f"stage{i}"]
        got = stage_tap(mo, mel_tm, i).cpu().numpy().reshape(ref.shape[0], -1, ref.shape[1]).transpose(0, 2, 1)
        assert got.shape == ref.shape
        err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
        print(f"FIXTURE {tag}: stage{i} max error {err:.3e} (scale {scale:.3f})")
        assert err <= 2e-5 * scale, (tag, i, err, scale)


@pytest.mark.parametrize("tag", sorted(symo.CONFIGS))
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
    assert mo.eng.vocoder_length(12) == config.generator_length(mo.conf, 12) == symo.sym_lengths(mo.conf["vocoder_config"], 12)[-1]
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
    rc, _ = mo.layer_rc(KIND_AMP, x, torch.empty_like(x), 0, 0, 0, window=1)
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
        Model(str(tmp_path), "mixed", "seed1235")


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
        TT, family = vl.amp_tile_rows(C, ks, d, L, False, height64=mo.planned_height(L, B, ks))
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
