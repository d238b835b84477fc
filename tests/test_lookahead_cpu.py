"""The look-ahead window of the incremental generator without a GPU: the look-ahead of a symmetric generator measured on the float64
oracle against config.generator_lookahead / config.stream_lags, a float64 emulation of the stream (lookahead_oracle.StreamEmulation:
every tensor only up to its frontier per push, then the flush) against the offline oracle for several cuts, and the surface - the
lookahead= keywords, the refusals that stay, the ABI table."""
import inspect
import os
import re
import types

import pytest
import torch

import lookahead_oracle as lo
import vocoder_layers as vl
from bvcodec import _abi, config, synth
from oracle import bigvgan as obig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("all", "mixed")


def draw(conf_var, tag, T, B=1, seed=11):
    conf = conf_var if tag == "causal" else vl.with_switches(conf_var, vl.SYM_CONFIGS[tag])
    sd = synth.generator_state_dict(conf, 1235)
    g = torch.Generator().manual_seed(seed)
    mel = (-4.0 + 1.6 * torch.randn(B, conf["num_mels"], T, generator=g, dtype=torch.float64))
    return conf, sd, mel


# ----------------------------------------------------------------------------------------------- 1. the look-ahead, measured
def test_hand_worked_figures(conf_var):
    """The recursion on the shipped geometry (rates 8, 8, 2, 2; ks 3, 7, 11; dilations 1, 3, 5), by hand: all symmetric
    3 -> 28 -> 88 -> 708 -> 768 -> 1537 -> 1597 -> 3195 -> 3255 -> 3258; the mixed one 0 -> 0 -> 0 -> 4 -> 64 -> 128 -> 128 -> 257 ->
    317 -> 320."""
    la = config.stream_lags(vl.with_switches(conf_var, vl.SYM_CONFIGS["all"]))
    assert [la[k] for k in ("conv_pre", "up0", "stage0", "up1", "stage1", "up2", "stage2", "up3", "stage3", "wav")] == \
        [3, 28, 88, 708, 768, 1537, 1597, 3195, 3255, 3258]
    assert la["P"][0] == [28 + 2, 28 + 6, 28 + 10] and la["Q"][0] == [28 + 2 + 4, 28 + 6 + 12, 28 + 10 + 20]
    lm = config.stream_lags(vl.with_switches(conf_var, vl.SYM_CONFIGS["mixed"]))
    assert [lm[k] for k in ("conv_pre", "up0", "stage0", "up1", "stage1", "up2", "stage2", "up3", "stage3", "wav")] == \
        [0, 0, 0, 4, 64, 128, 128, 257, 317, 320]
    assert config.generator_lookahead(vl.with_switches(conf_var, vl.SYM_CONFIGS["all"])) == 3258
    assert config.generator_lookahead(vl.with_switches(conf_var, vl.SYM_CONFIGS["mixed"])) == 320


@pytest.mark.parametrize("tag", TAGS + ("causal",))
def test_lookahead_measured_on_the_oracle(conf_var, tag):
    """Perturbing mel frame t0 of T = 24: the first sample that changes is 256 t0 - generator_lookahead, and the first row of every
    tap rate * t0 - its lag; a causal generator's is 0."""
    T, t0 = 24, 16
    conf, sd, mel = draw(conf_var, tag, T)
    lags, rates = config.stream_lags(conf), lo.rates(conf)
    D = config.generator_lookahead(conf)
    assert D == lags["wav"] and (D == 0) == (tag == "causal")
    taps, taps_p = {}, {}
    wav = obig.forward(sd, conf["vocoder_config"], mel, 10 ** 9, torch.float64, taps=taps)
    melp = mel.clone()
    # The earliest sample is reached through the outermost tap of every conv on the way alone, some forty small weights in a row: a
    # perturbation of order 1 arrives there below float64's resolution of the sample (measured: the first `!=` then comes 5 to 21
    # samples late).  SnakeBeta passes x through linearly, so a huge one arrives whole, and everything stays finite.
    melp[:, :, t0] += 1e20 * torch.randn(conf["num_mels"], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    wav_p = obig.forward(sd, conf["vocoder_config"], melp, 10 ** 9, torch.float64, taps=taps_p)

    def first_change(a, b):
        return int((a != b).any(dim=1)[0].nonzero()[0])
    assert 256 * t0 - D > 0 and bool(torch.isfinite(wav_p).all())
    assert first_change(wav, wav_p) == 256 * t0 - D
    for name in taps:
        assert first_change(taps[name], taps_p[name]) == rates[name] * t0 - lags[name], name


def test_a_filtered_generator_cannot_stream(conf_var):
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS["with_aa"])
    assert config.generator_lookahead(conf) == -1
    with pytest.raises(ValueError, match="anti-aliased"):
        config.stream_lags(conf)


# ----------------------------------------------------------------------------------------------- 2. the stream, emulated in float64
@pytest.mark.parametrize("tag", TAGS)
def test_emulated_stream_equals_the_offline_oracle(conf_var, tag):
    """T = 24 cut three ways, and T = 5 - shorter than the look-ahead of "all", so everything comes from the flush: the pieces,
    concatenated, are oracle.bigvgan.forward exactly; every push returns the issue's count; every tensor ends at its true length."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for T, cuts in [(24, c) for c in lo.CUTS_24] + [(5, [2, 3])]:
            conf, sd, mel = draw(conf_var, tag, T, B=2 if cuts == [24] else 1)
            taps = {}
            ref = obig.forward(sd, conf["vocoder_config"], mel, 10 ** 9, torch.float64, taps=taps)
            assert ref.shape[2] == config.generator_length(conf, T)
            pieces, em = lo.run_cuts(sd, conf, mel, cuts)
            n = 0
            for k, piece in zip(cuts, pieces):
                assert piece.shape[2] == lo.push_samples(conf, n, n + k), (T, cuts, n, k)
                n += k
            if T == 5 and tag == "all":
                assert all(p.shape[2] == 0 for p in pieces[:-1])
            assert torch.equal(torch.cat(pieces, 2), ref), (T, cuts)
            for name in taps:
                assert torch.equal(em.done[name], taps[name]), (T, cuts, name)
    finally:
        torch.set_num_threads(threads)


def test_emulated_causal_stream_flushes_the_tail(conf_var):
    conf, sd, mel = draw(conf_var, "causal", 6)
    pieces, _ = lo.run_cuts(sd, conf, mel, [1, 2, 3])
    assert [p.shape[2] for p in pieces] == [256, 512, 768, 294]
    assert torch.equal(torch.cat(pieces, 2), obig.forward(sd, conf["vocoder_config"], mel, 10 ** 9, torch.float64))


# ----------------------------------------------------------------------------------------------- 3. the surface
def test_lookahead_keywords_exist_and_the_defaults_still_refuse(conf_var):
    from bvcodec.streaming import StreamingCodec, StreamingDecoder, VocoderStream
    assert inspect.signature(VocoderStream.__init__).parameters["lookahead"].default is False
    assert inspect.signature(StreamingDecoder.__init__).parameters["lookahead"].default is False
    assert "lookahead" not in inspect.signature(StreamingCodec.__init__).parameters     # sessions: not part of this
    for tag, word in (("all", "symmetric"), ("mixed", "symmetric"), ("with_aa", "anti-aliased")):
        holder = types.SimpleNamespace(conf=vl.with_switches(conf_var, vl.SYM_CONFIGS[tag]))
        with pytest.raises(ValueError, match=word):
            VocoderStream(holder, 2, 4)
        with pytest.raises(ValueError, match=word):
            StreamingDecoder(holder, 2)
        with pytest.raises(ValueError, match=word):
            StreamingDecoder(holder, 2, incremental=False)
    aa = types.SimpleNamespace(conf=vl.with_switches(conf_var, vl.SYM_CONFIGS["with_aa"]))
    with pytest.raises(ValueError, match="anti-aliased"):
        VocoderStream(aa, 2, 4, lookahead=True)
    with pytest.raises(ValueError, match="anti-aliased"):
        StreamingDecoder(aa, 2, lookahead=True)
    sym = types.SimpleNamespace(conf=vl.with_switches(conf_var, vl.SYM_CONFIGS["all"]))
    with pytest.raises(ValueError, match="incremental"):
        StreamingDecoder(sym, 2, incremental=False, lookahead=True)


def test_abi_table_equals_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvcodec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bvc_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_abi.SIGNATURES), declared ^ set(_abi.SIGNATURES)
    new = ("bvc_vocoder_lookahead", "bvc_vocoder_stream_create_lookahead", "bvc_vocoder_stream_samples", "bvc_vocoder_stream_flush",
           "bvc_test_amp_pair_window")
    assert all(n in declared for n in new)
    lib = _abi.load()
    assert all(hasattr(lib, n) for n in new) and lib.bvc_abi_version() == 3
    assert lib.bvc_vocoder_lookahead(None) == -1 and lib.bvc_vocoder_stream_samples(None, 1) == 0
