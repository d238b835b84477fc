"""Anti-aliased activations on the GPU: every filtered AMP pair and the filtered conv_post one launch at a time against the
float64 oracle (oracle/bigvgan.py) with the project's bar, vocoder_layers.compare: e_hip = max|hip - oracle64| <= 8 x
max(e32, 2^-24 max|oracle64|); the two reference fixtures through BigVGAN.forward and the facade's decode; batch invariance; and
the refusals of everything that counts on a causal generator.  Measured ratios: profiles/antialias_parity.md.
Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_generator as gg
import vocoder_layers as vl
from gpu_generator import DEV, H_DIM, KIND_AMP, amp_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """models(tag, draw): the product model of one of vl.AA_CONFIGS and one generator draw."""
    directory = str(tmp_path_factory.mktemp("antialias"))
    get, close = gg.cached(lambda tag, draw: gg.Model(directory, draw, tag, switches=vl.AA_CONFIGS[tag], h_dim=H_DIM))
    yield lambda tag, draw="seed1235": get(tag, draw)
    close()


def check_fixture(mo, tag):
    gg.check_fixture(mo, f"g10_bigvgan_aa_{tag}", tag, ("stage0", "stage1", "stage2", "stage3"), rms_bar=1e-4)


# ----------------------------------------------------------------------------------------------- 5. layer parity
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
        TT = vl.amp_tile_rows(C, ks, d, 10 ** 6, False, form="filtered")[0]
        assert TT == vl.AA_TILE_HEIGHT[C] - (ks - 1) - 10
        epi = (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(q + stage) % 3]
        for L in vl.aa_lengths(TT, ks, d):
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
    gg.every_channel_count_meets_every_epilogue(models("all").conf)


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_filtered_conv_post_against_float64(models, draw):
    mo, ledger = models("all", draw), vl.Ledger(draw)
    gg.conv_post_sweep(mo, ledger, "filtered", (1, 5, 6, 255, 256, 257, 600), (6, 257), ("n6", "row_first", "row_last", "zeros"))
    ledger.close()


# ----------------------------------------------------------------------------------------------- 6. the reference's run
@pytest.mark.parametrize("tag", sorted(vl.AA_CONFIGS))
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
    rc, _ = mo.layer_rc(KIND_AMP, x, torch.empty_like(x), 0, 0, 0, window=(0, 0))
    assert rc == -1 and b"anti-aliased" in mo.lib.bvc_last_error()
    check_fixture(mo, "mixed")                                            # a following offline call is untouched
