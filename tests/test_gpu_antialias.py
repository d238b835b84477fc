"""Anti-aliased activations on the GPU: every filtered AMP pair and the filtered conv_post one launch at a time against the
float64 oracle (tests/antialias_oracle.py) with the project's bar, vocoder_layers.compare: e_hip = max|hip - oracle64| <= 8 x
max(e32, 2^-24 max|oracle64|); the two reference fixtures through BigVGAN.forward and the facade's decode; batch invariance; and
the refusals of everything that counts on a causal generator.  Measured ratios: profiles/antialias_parity.md.
Needs the MI355X: run with ``-m gpu``."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import antialias_oracle as aao
import vocoder_layers as vl
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIND_AMP, KIND_POST = 2, 3
H_DIM = 64                                   # a small coder: these tests are about the generator


class Model:
    """The product model of one configuration and one generator draw on the GPU."""

    def __init__(self, directory, tag, draw):
        from bvcodec import BVRNNCodecModel, _abi, synth
        layers, post = aao.CONFIGS[tag]
        self.tag, self.draw = tag, draw
        cfg = os.path.join(directory, f"{tag}.toml")
        self.conf = aao.write_config(cfg, layers, post, h_dim=H_DIM)
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


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    directory, cache = str(tmp_path_factory.mktemp("antialias")), {}

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


# ----------------------------------------------------------------------------------------------- 5. layer parity
def amp_case(mo, ledger, pair, B, L, kind, epi):
    i, j, m, C, ks, d, pre = pair
    TT = aao.aa_tile_rows(C, ks)
    what = f"filtered amp pair stage {i} block {j} iteration {m} (C={C} ks={ks} d={d}) epi={epi} B={B} L={L} input={kind}"
    seed = seed_of(mo.draw, i, j, m, B, L, kind, epi)
    x = vl.make_input(kind, B, C, L, TT, seed)
    acc = vl.make_input("n1", B, C, L, TT, seed + 1) if epi >= vl.CE_RES_ACC else None

    def oracle(dtype):
        y = aao.amp_pair(mo.sd, pre, m, x, ks, d, dtype=dtype)
        if epi >= vl.CE_RES_ACC:
            y = acc.to(dtype) + y
        if epi == vl.CE_RES_ACC_DIV:
            y = y / 3
        return vl.cl(y)
    with torch.no_grad():
        r64, r32 = oracle(torch.float64), oracle(torch.float32)
    if acc is None:
        out, acc_dev = torch.full((B, L, C), float("nan"), device=DEV), None
    else:
        out = to_dev(acc)                                            # the running sum IS the output buffer, as in the path
        acc_dev = out
    info = mo.layer(KIND_AMP, to_dev(x), out, i, j, m, epi, acc_dev)
    tiles = B * -(-L // TT)
    assert info == [L, C, tiles, (tiles + 7) // 8 * 8, TT], (what, info, "assumed tiles / rows per tile", tiles, TT)
    ledger.add(f"amp{C}/filtered", vl.compare(out.cpu().numpy(), r64, r32, what, tile_rows=TT))


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_filtered_amp_pairs_against_float64(models, stage):
    """The nine (ks, d) pairs of the stage, each with one of the three epilogues (rotating, so that every (C, epilogue) occurs; the
    running sums aliased to the output), at every length of aa_lengths - the two clamps on signals shorter than the filter's
    reach, both sides of every seam - with N(0, 36) input, the draws and B in {2, 3} rotating; and the inputs whose replicated
    ends carry the only non-zero row, and zeros, at 1, 6, TT + 1 and 2 TT + 1 rows."""
    conf = models("all").conf
    ledgers = {draw: vl.Ledger(draw) for draw in vl.DRAWS}
    n = 0
    for q, pair in enumerate(p for p in vl.pairs(conf) if p[0] == stage):
        C, ks, d = pair[3:6]
        TT = aao.aa_tile_rows(C, ks)
        assert TT == aao.AA_TILE_HEIGHT[C] - (ks - 1) - 10
        epi = (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(q + stage) % 3]
        for L in aao.aa_lengths(TT, ks, d):
            n += 1
            draw = vl.DRAWS[n % 4]
            amp_case(models("all", draw), ledgers[draw], pair, 2 + (n // 4) % 2, L, "n6", epi)
        for kind in ("row_first", "row_last", "zeros"):
            for L in (1, 6, TT + 1, 2 * TT + 1):
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


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_filtered_conv_post_against_float64(models, draw):
    mo, ledger = models("all", draw), vl.Ledger(draw)
    n = 0
    for L in (1, 5, 6, 255, 256, 257, 600):
        for length in sorted({L, max(1, L - 3), 10 ** 9}):
            for kind in (("n6",) if L not in (6, 257) else ("n6", "row_first", "row_last", "zeros")):
                n += 1
                B, div = 2 + n % 2, (1.0, 0.95)[n % 2]
                x = vl.make_input(kind, B, 8, L, vl.POST_TILE_ROWS, seed_of(draw, "post", L, length, kind))
                rows = min(L, length)
                out = torch.full((B, rows), float("nan"), device=DEV)
                info = mo.layer(KIND_POST, to_dev(x), out, length=length, div=div)
                assert info[:2] == [rows, 1]
                with torch.no_grad():
                    r64 = aao.conv_post(mo.sd, x, length, torch.float64)[:, 0].numpy() / np.float64(np.float32(div))
                    r32 = (aao.conv_post(mo.sd, x, length, torch.float32)[:, 0].numpy() / np.float32(div)).astype(np.float64)
                ledger.add("conv_post/filtered", vl.compare(out.cpu().numpy(), r64, r32,
                                                            f"filtered conv_post B={B} L={L} length={length} div={div} input={kind}",
                                                            tile_rows=vl.POST_TILE_ROWS))
    ledger.close()


# ----------------------------------------------------------------------------------------------- 6. the reference's run
def stage_tap(mo, mel_tm, i):
    B, T = mel_tm.shape[0], mel_tm.shape[1]
    ws, nws = mo.eng.workspace(B, T)
    n = ctypes.c_int64()
    mo.abi.check(mo.lib.bvc_test_vocoder_tap(mo.eng.handle, mo.abi.ptr(mel_tm), B, T, 2 + 2 * i, None, ctypes.byref(n), ws, nws, mo.eng.stream()))
    out = torch.full((B, n.value), float("nan"), device=DEV)
    mo.abi.check(mo.lib.bvc_test_vocoder_tap(mo.eng.handle, mo.abi.ptr(mel_tm), B, T, 2 + 2 * i, mo.abi.ptr(out), ctypes.byref(n), ws, nws,
                                             mo.eng.stream()))
    torch.cuda.synchronize()
    return out


def check_fixture(mo, tag):
    g = load_golden(f"g10_bigvgan_aa_{tag}")
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


@pytest.mark.parametrize("tag", sorted(aao.CONFIGS))
def test_reference_fixture_through_forward_and_decode(models, tag):
    """BigVGAN.forward against the reference's waveform (rms <= 1e-4) and stage taps (<= 2e-5), the bars test_gpu_parity.py has for
    g5; `mixed` runs filtered stages in front of the persistent C = 16 kernel and behind it.  The fixture starts at the mel, so the
    facade's decode is held against forward on the mel its own coder decodes, with the waveform bar (rms <= 1e-4)."""
    mo = models(tag)
    check_fixture(mo, tag)
    rng = np.random.default_rng(3)
    codes = torch.from_numpy(rng.integers(0, 2, size=(2, 12, 64)).astype(np.float32)).to(DEV)
    wav = mo.model.decode(codes, 3000)
    mel, _ = mo.model.bvrnn.decode(codes, torch.zeros(1, 2, H_DIM, device=DEV))
    from bvcodec.model import SCALING
    ref = mo.model.vocoder(mel, 3000, _scale_div=float(SCALING), _time_major=True)[:, 0]
    assert wav.shape == (2, 3000) and bool(torch.isfinite(wav).all())
    rms = float((wav - ref).pow(2).mean().sqrt())
    print(f"FIXTURE {tag}: decode against forward on its own mel, rms {rms:.3e}, equal bits {torch.equal(wav, ref)}")
    assert rms <= 1e-4


# ----------------------------------------------------------------------------------------------- 7. invariance
def test_item_of_a_batch_equals_the_item_alone(models):
    """64 + 3 frames: workgroups serve several tiles and items from stage 0 on."""
    mo = models("all")
    rng = np.random.default_rng(4)
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((5, 80, 67))).astype(np.float32)).to(DEV)
    full = mo.model.vocoder(mel, 10 ** 9)
    assert full.shape == (5, 1, 256 * 67 + 294) and bool(torch.isfinite(full).all())
    assert torch.equal(mo.model.vocoder(mel, 10 ** 9), full)
    for b in (0, 3, 4):
        assert torch.equal(mo.model.vocoder(mel[b:b + 1].contiguous(), 10 ** 9), full[b:b + 1]), b


# ----------------------------------------------------------------------------------------------- 8. refusals
def test_everything_causal_is_refused_and_offline_decode_goes_on(models):
    from bvcodec.streaming import StreamingCodec, StreamingDecoder, VocoderStream
    mo = models("mixed")
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingCodec(mo.model, 2, 3000)
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingCodec(mo.model, 2, 3000, direction="recv")
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingDecoder(mo.model, 2)
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingDecoder(mo.model, 2, incremental=False)
    with pytest.raises(ValueError, match="anti-aliased"):
        VocoderStream(mo.eng, 2, 4)
    codes = torch.full((2, 12, 64), 0.5, device=DEV)
    with pytest.raises(ValueError, match="anti-aliased"):
        mo.model.decode(codes, 3000, frames=[12, 7])
    with pytest.raises(ValueError, match="anti-aliased"):
        mo.model.decode(codes, [3000, 2000])
    with pytest.raises(ValueError, match="anti-aliased"):
        mo.model.decode_many([codes[0], codes[1, :7]], 3000)
    assert [tuple(w.shape) for w in mo.model.decode_many([codes[0], codes[1]], 3000, max_batch=1)] == [(3000,), (3000,)]
    # the library itself: BVC_EINVAL (-1) from the entry points under those classes, and from the windowed test entry
    h = ctypes.c_void_p()
    assert mo.lib.bvc_vocoder_stream_create(mo.eng.handle, 2, 4, ctypes.byref(h)) == -1 and b"anti-aliased" in mo.lib.bvc_last_error()
    assert mo.lib.bvc_stream_codec_create(mo.eng.handle, 2, 441, 35.0, 0.95, 0.95, ctypes.byref(h)) == -1
    x = torch.zeros(2, 40, 64, device=DEV)
    rc, _ = mo.layer_rc(KIND_AMP, x, torch.empty_like(x), 0, 0, 0, window=1)
    assert rc == -1 and b"anti-aliased" in mo.lib.bvc_last_error()
    check_fixture(mo, "mixed")                                            # a following offline call is untouched
