"""The incremental generator behind a look-ahead window on the GPU: every symmetric AMP pair in a look-ahead window, one launch at a
time against the float64 oracle with the project's bar (vocoder_layers.compare, MARGIN = 8) and with the tiles of
lookahead_oracle.sym_window_tile_rows asserted; the stream (bvc_vocoder_stream_create_lookahead, push, flush) against the offline call
bit for bit for several cuts; the causal model through the new create against the plain stream; a 256-wide generator with symmetric
narrow stages; StreamingDecoder(lookahead=True) against decode; what stays refused.  Measured ratios:
profiles/lookahead_stream_parity.md.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_generator as gg
import lookahead_oracle as lo
import vocoder_layers as vl
from gpu_generator import DEV, H_DIM, nan_like, seed_of, to_dev

pytestmark = pytest.mark.gpu

CAUSAL = "causal"
WIDE = "wide256"                             # upsample_initial_channel 256: stage 0 (128 channels) causal, the narrower ones symmetric
PAIR_DRAWS = ("seed1235", "wide")
T_, F_ = True, False


def make_model(directory, tag, draw):
    if tag == WIDE:
        return gg.Model(directory, draw, tag, width=256, switches=dict(layers_sym=[F_, T_, T_, T_], pre_sym=True, post_sym=True), h_dim=H_DIM)
    return gg.Model(directory, draw, tag, switches=None if tag == CAUSAL else vl.SYM_CONFIGS[tag], h_dim=H_DIM)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    directory = str(tmp_path_factory.mktemp("lookahead"))
    get, close = gg.cached(lambda tag, draw: make_model(directory, tag, draw))
    yield lambda tag, draw="seed1235": get(tag, draw)
    close()


def mel_draw(B, T, seed):
    """(B, T, num_mels) time-major on the device."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32)).to(DEV)


def offline(mo, mel_tm, div=1.0):
    return mo.model.vocoder(mel_tm, 10 ** 9, _scale_div=div, _time_major=True)[:, 0]


def stream_pieces(vs, mel_tm, cuts, div=1.0):
    """The pushes of ``cuts`` frames and the flush; every count is held against bvc_vocoder_stream_samples (asked before the call)
    and against the issue's arithmetic."""
    conf, pieces, t = vs.eng.conf, [], 0
    for k in cuts:
        want = vs.samples(k) if k <= vs.kmax else None             # (a longer push goes through in pieces)
        pieces.append(vs.push(mel_tm[:, t:t + k].contiguous(), div))
        assert pieces[-1].shape == (vs.B, lo.push_samples(conf, t, t + k)), (cuts, t, k, pieces[-1].shape)
        assert want is None or want == pieces[-1].shape[1]
        t += k
    want = vs.samples(-1)
    pieces.append(vs.flush(div))
    assert pieces[-1].shape == (vs.B, want)
    return pieces


# ----------------------------------------------------------------------------------------------- 1. one pair in a look-ahead window
def window_case(mo, ledger, pair, B, new_rows, regime, origin, epi, n):
    """One launch of bvc_test_amp_pair_window against the float64 oracle.  regime 'mid': row_end = L_in - reach and the oracle's
    signal CONTINUES with real rows behind L_in (the launch cannot see them and must not need them); 'flush': row_end = L_in, the
    signal ends there.  origin 'inside': t_origin > 0, the history rows are real data; 'before': the window starts before the signal
    (t_origin < 0), its first rows are zeros and the S2 rows before time 0 are zero - time 0 is the first new row or the row before."""
    i, j, m, C, ks, d, pre = pair
    h = vl.reach(ks, d)
    rb = h + 4 + n % 3                                              # history: the reach-back and a little more
    re = rb + new_rows
    L_in = re + (h if regime == "mid" else 0)
    behind = h + 5 if regime == "mid" else 0                        # real rows of the signal behind the window
    TT, family = lo.sym_window_tile_rows(C, ks, new_rows)
    what = f"look-ahead pair stage {i} block {j} iteration {m} (C={C} ks={ks} d={d}) epi={epi} B={B} rows [{rb}, {re}) of {L_in} {regime} {origin}"
    seed = seed_of(mo.draw, i, j, m, B, new_rows, regime, origin, epi)
    if origin == "inside":
        t0 = 37
        x_ref = vl.make_input("n6", B, C, t0 + L_in + behind, TT, seed)
        buf, lo_ref = x_ref[:, :, t0:t0 + L_in], t0 + rb
    else:
        z = rb - n % 2                                              # buffer row of global time 0
        t0 = -z
        x_ref = vl.make_input("n6", B, C, L_in - z + behind, TT, seed)
        buf, lo_ref = torch.cat([torch.zeros(B, C, z), x_ref[:, :, :L_in - z]], 2), rb - z
    acc = acc_ref = None
    if epi >= vl.CE_RES_ACC:
        acc = vl.make_input("n1", B, C, L_in, TT, seed + 1)
        acc_ref = torch.zeros_like(x_ref)
        acc_ref[:, :, lo_ref:lo_ref + new_rows] = acc[:, :, rb:re]
    with torch.no_grad():
        r64 = vl.cl(vl.oracle_pair(mo.sd, pair, x_ref, torch.float64, epi, acc_ref, sym=True))[:, lo_ref:lo_ref + new_rows]
        r32 = vl.cl(vl.oracle_pair(mo.sd, pair, x_ref, torch.float32, epi, acc_ref, sym=True))[:, lo_ref:lo_ref + new_rows]
    out, x_dev, acc_dev = nan_like(B, L_in, C), to_dev(buf), None if acc is None else to_dev(acc)
    info = (ctypes.c_int64 * 5)()
    mo.abi.check(mo.lib.bvc_test_amp_pair_window(mo.eng.handle, i, j, m, mo.abi.ptr(x_dev), B, L_in, mo.abi.ptr(out), epi,
                                                 mo.abi.ptr(acc_dev), rb, re, t0, info, mo.eng.stream()))
    tiles = B * -(-new_rows // TT)
    assert list(info) == [L_in, C, tiles, (tiles + 7) // 8 * 8, TT], (what, list(info), "assumed tiles / rows per tile", tiles, TT)
    got = out.cpu().numpy()
    assert np.isnan(got[:, :rb]).all() and np.isnan(got[:, re:]).all(), what + ": rows outside [row_begin, row_end) written"
    ledger.add(family, vl.compare(got[:, rb:re], r64, r32, what, tile_rows=TT))


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_symmetric_pairs_in_look_ahead_windows_against_float64(models, stage):
    """The nine (ks, d) pairs of the stage (C = 64 / 32 / 16 / 8): 1, 8, the short tile's height, one more row, 129 and 400 new rows; both
    regimes; both origins; the epilogue rotating so that every (C, epilogue) occurs (the running sum in a buffer of its own: the
    output is NaN before the launch and rows outside [row_begin, row_end) are NaN after it); draws and B in {2, 3} rotating."""
    conf = models("all").conf
    gg.every_channel_count_meets_every_epilogue(conf)
    ledgers = {draw: vl.Ledger(draw) for draw in PAIR_DRAWS}
    n = 0
    for q, pair in enumerate(p for p in vl.pairs(conf) if p[0] == stage):
        C, ks = pair[3], pair[4]
        epi = (vl.CE_RES, vl.CE_RES_ACC, vl.CE_RES_ACC_DIV)[(q + stage) % 3]
        for new_rows in lo.sym_window_new_rows(C, ks):
            for regime in ("mid", "flush"):
                for origin in ("inside", "before"):
                    n += 1
                    draw = PAIR_DRAWS[n % 2]
                    window_case(models("all", draw), ledgers[draw], pair, 2 + (n // 2) % 2, new_rows, regime, origin, epi, n)
    for ledger in ledgers.values():
        ledger.close()


# ----------------------------------------------------------------------------------------------- 2. the stream is the offline call
CUTS_40 = ((8, [1] * 40), (8, [2, 1, 4, 8, 8, 8, 8, 1]), (8, [8] * 5), (2, [3] * 13 + [1]))


@pytest.mark.parametrize("tag", ["all", "mixed"])
def test_stream_equals_the_offline_call_bit_for_bit(models, tag):
    """B = 3, T = 40: pushes and flush concatenated are bvc_bigvgan over the whole mel, for every cut (the last one through pushes the
    class splits); the counts are bvc_vocoder_stream_samples' and sum to generator_length(T); the early pushes of "all" are empty."""
    from bvcodec import config
    from bvcodec.streaming import VocoderStream
    mo = models(tag)
    B, T = 3, 40
    mel = mel_draw(B, T, 21)
    ref = offline(mo, mel)
    assert ref.shape == (B, config.generator_length(mo.conf, T))
    for kmax, cuts in CUTS_40:
        vs = VocoderStream(mo.eng, B, kmax, lookahead=True)
        assert vs.lookahead == config.generator_lookahead(mo.conf) == mo.lib.bvc_vocoder_lookahead(mo.eng.handle)
        pieces = stream_pieces(vs, mel, cuts)
        if tag == "all" and cuts[0] == 1:
            assert all(p.shape == (B, 0) for p in pieces[:12]) and pieces[12].shape[1] == 13 * 256 - 3258
        got = torch.cat(pieces, 1)
        assert got.shape == ref.shape and torch.equal(got, ref), (tag, kmax, cuts, float((got - ref).abs().max()))


def test_short_utterance_reset_and_rows(models):
    """T = 5 on "all": everything comes from the flush.  reset, then another mel: equal again.  Row b of the batch is a stream of that
    row alone.  The output gain divides as in the offline call."""
    from bvcodec.streaming import VocoderStream
    mo = models("all")
    vs = VocoderStream(mo.eng, 3, 4, lookahead=True)
    mel = mel_draw(3, 5, 22)
    pieces = stream_pieces(vs, mel, [2, 3])
    assert [p.shape[1] for p in pieces] == [0, 0, 5 * 256]
    assert torch.equal(pieces[-1], offline(mo, mel))
    vs.reset()
    mel2 = mel_draw(3, 17, 23)
    assert torch.equal(torch.cat(stream_pieces(vs, mel2, [4, 4, 4, 4, 1], 0.95), 1), offline(mo, mel2, 0.95))
    vs.reset()
    whole = torch.cat(stream_pieces(vs, mel2, [3, 4, 4, 4, 2]), 1)
    one = VocoderStream(mo.eng, 1, 4, lookahead=True)
    for b in (0, 2):
        assert torch.equal(torch.cat(stream_pieces(one, mel2[b:b + 1].contiguous(), [4, 4, 4, 4, 1]), 1), whole[b:b + 1]), b
        one.reset()
    empty = VocoderStream(mo.eng, 2, 4, lookahead=True)
    assert empty.samples(-1) == 0 and empty.flush().shape == (2, 0)


# ----------------------------------------------------------------------------------------------- 3. the causal model
def test_causal_model_through_the_look_ahead_create(models):
    """Every push is the plain stream's bits, the look-ahead is 0, the flush is the offline tail behind 256 T."""
    from bvcodec.streaming import VocoderStream
    mo = models(CAUSAL)
    B, T = 2, 13
    mel = mel_draw(B, T, 24)
    plain, ahead = VocoderStream(mo.eng, B, 4), VocoderStream(mo.eng, B, 4, lookahead=True)
    assert ahead.lookahead == 0 and mo.lib.bvc_vocoder_lookahead(mo.eng.handle) == 0
    t = 0
    for k in (1, 4, 2, 3, 3):
        a, b = plain.push(mel[:, t:t + k].contiguous()), ahead.push(mel[:, t:t + k].contiguous())
        assert a.shape == (B, 256 * k) and torch.equal(a, b), (t, k)
        t += k
    tail = ahead.flush()
    assert tail.shape == (B, 294) and torch.equal(tail, offline(mo, mel)[:, 256 * T:])


# ----------------------------------------------------------------------------------------------- 4. width 256
def test_wide_generator_with_symmetric_narrow_stages(models):
    from bvcodec import config
    from bvcodec.streaming import VocoderStream
    mo = models(WIDE)
    B, T = 2, 16
    mel = mel_draw(B, T, 25)
    ref = offline(mo, mel)
    assert ref.shape == (B, config.generator_length(mo.conf, T))
    for kmax, cuts in ((2, [1, 2, 1, 2, 2, 2, 2, 2, 2]), (8, [8, 5, 3])):
        vs = VocoderStream(mo.eng, B, kmax, lookahead=True)
        assert vs.lookahead == mo.lib.bvc_vocoder_lookahead(mo.eng.handle) > 0
        assert torch.equal(torch.cat(stream_pieces(vs, mel, cuts), 1), ref), cuts


# ----------------------------------------------------------------------------------------------- 5. StreamingDecoder
@pytest.mark.parametrize("tag", ["all", "mixed"])
def test_streaming_decoder_with_look_ahead_equals_decode(models, tag):
    """cat(pushes + [finish(n)]) is decode(codes, n): n = 3000 on 12 frames (the pushes of "mixed" have returned 2752 samples by
    then, finish cuts the rest), 10**9 on 20 frames, and n = 200, below both look-aheads, on one frame.  What the pushes have returned
    stays returned, so a cut needs 256 T - look-ahead <= n."""
    from bvcodec import config
    from bvcodec.streaming import StreamingDecoder
    mo = models(tag)
    rng = np.random.default_rng(6)
    D = config.generator_lookahead(mo.conf)
    for T, n, cuts in ((12, 3000, [5, 1, 4, 2]), (20, 10 ** 9, [5, 1, 4, 7, 3]), (1, 200, [1])):
        assert n < D or max(0, 256 * T - D) <= n
        codes = torch.from_numpy(rng.integers(0, 2, size=(2, T, 64)).astype(np.float32)).to(DEV)
        dec = StreamingDecoder(mo.model, 2, lookahead=True, max_frames_per_push=4)
        assert dec.lookahead == D
        pushes, t = [], 0
        for k in cuts:
            pushes.append(dec.push(codes[:, t:t + k]))
            t += k
        assert sum(p.shape[1] for p in pushes) == max(0, 256 * T - D) <= n
        got = torch.cat(pushes + [dec.finish(n)], 1)
        ref = mo.model.decode(codes, n)
        assert got.shape == ref.shape and torch.equal(got, ref), (tag, T, n, float((got - ref).abs().max()))


# ----------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(models):
    from bvcodec.streaming import StreamingDecoder, VocoderStream
    aa = models("with_aa")
    with pytest.raises(ValueError, match="anti-aliased"):
        VocoderStream(aa.eng, 2, 4, lookahead=True)
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingDecoder(aa.model, 2, lookahead=True)
    h = ctypes.c_void_p()
    assert aa.lib.bvc_vocoder_stream_create_lookahead(aa.eng.handle, 2, 4, ctypes.byref(h)) == -1 and b"anti-aliased" in aa.lib.bvc_last_error()
    assert aa.lib.bvc_vocoder_lookahead(aa.eng.handle) < 0
    x = torch.zeros(2, 40, 64, device=DEV)
    rc = aa.lib.bvc_test_amp_pair_window(aa.eng.handle, 0, 0, 0, aa.abi.ptr(x), 2, 40, aa.abi.ptr(torch.empty_like(x)), 1, None, 10, 20, 0, None,
                                         aa.eng.stream())
    assert rc == -1 and b"anti-aliased" in aa.lib.bvc_last_error()
    mo = models("mixed")
    with pytest.raises(ValueError, match="incremental"):
        StreamingDecoder(mo.model, 2, incremental=False, lookahead=True)
    vs = VocoderStream(mo.eng, 2, 2, lookahead=True)
    mel = mel_draw(2, 3, 26)
    wav = torch.empty(2, 4096, device=DEV)
    assert mo.lib.bvc_vocoder_stream_push(vs.handle, mo.abi.ptr(mel), 3, 1.0, mo.abi.ptr(wav), mo.eng.stream()) == -1       # k > kmax
    assert b"outside 1..2" in mo.lib.bvc_last_error()
    vs.push(mel[:, :2].contiguous())
    vs.flush()
    assert mo.lib.bvc_vocoder_stream_push(vs.handle, mo.abi.ptr(mel), 1, 1.0, mo.abi.ptr(wav), mo.eng.stream()) == -1       # push after flush
    assert b"flushed" in mo.lib.bvc_last_error()
    assert mo.lib.bvc_vocoder_stream_flush(vs.handle, 1.0, mo.abi.ptr(wav), mo.eng.stream()) == -1
    with pytest.raises(ValueError, match="flushed"):
        vs.push(mel[:, :1].contiguous())
    vs.reset()
    assert vs.push(mel[:, :2].contiguous()).shape == (2, lo.push_samples(mo.conf, 0, 2))
    plain = VocoderStream(models(CAUSAL).eng, 2, 2)
    with pytest.raises(ValueError, match="lookahead"):
        plain.flush()
    assert mo.lib.bvc_vocoder_stream_flush(plain.handle, 1.0, mo.abi.ptr(wav), mo.eng.stream()) == -1


# ----------------------------------------------------------------------------------------------- 7. one table on both sides
def test_library_and_config_agree_on_the_look_ahead(models):
    from bvcodec import config
    for tag, want in (("all", 3258), ("mixed", 320), ("with_aa", -1), (CAUSAL, 0)):
        mo = models(tag)
        assert mo.lib.bvc_vocoder_lookahead(mo.eng.handle) == config.generator_lookahead(mo.conf) == want, tag
