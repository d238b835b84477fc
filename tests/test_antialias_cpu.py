"""Anti-aliased activations without a GPU: the oracle (oracle/bigvgan.py) against the reference's own run
(tests/golden/g10_bigvgan_aa_*.npz, written by tests/golden/make_golden_antialias.py), the checkpoint key layouts, the reach of
one filtered AMP pair - the halo the GPU kernel's tiles are cut with - and its conditioning in float32."""
import os

import numpy as np
import pytest
import torch

import vocoder_layers as vl
from conftest import load_golden
from bvcodec import synth, weights
from oracle import bigvgan as obig

TAPS = ("conv_pre", "stage0", "stage1", "stage2", "stage3")


@pytest.fixture(scope="module")
def conf_all(conf_var):
    return vl.with_switches(conf_var, vl.AA_CONFIGS["all"])


# ----------------------------------------------------------------------------------------------- 1. the oracle is the reference
@pytest.mark.parametrize("tag", sorted(vl.AA_CONFIGS))
def test_oracle_equals_reference_fixture_bit_for_bit(conf_var, tag):
    """Waveform and every tap, float32, with the weight fold of the reference's forward pre-hook (torch._weight_norm: the oracle's own
    fold_weight_norm gives weights one bit away, see oracle/bigvgan.py) and the fixture script's thread count, which decides
    how the CPU convolutions split their sums."""
    g = load_golden(f"g10_bigvgan_aa_{tag}")
    sw = vl.AA_CONFIGS[tag]
    assert list(g["layers_antialias"]) == sw["layers_antialias"] and bool(g["antialias_post"]) == sw["antialias_post"]
    conf = vl.with_switches(conf_var, sw)
    sd = synth.generator_state_dict(conf, seed=int(g["seed"]))
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        taps = {}
        wav = obig.forward(sd, conf["vocoder_config"], torch.from_numpy(g["mel"]), 10 ** 9, taps=taps, fold=obig.REFERENCE_FOLD)
    finally:
        torch.set_num_threads(threads)
    T = g["mel"].shape[2]
    assert wav.shape == g["wav"].shape == (2, 1, 256 * T + 294)
    assert np.array_equal(wav.numpy(), g["wav"]), float(np.abs(wav.numpy() - g["wav"]).max())
    for k in TAPS:
        assert np.array_equal(taps[k].numpy(), g[k]), (k, float(np.abs(taps[k].numpy() - g[k]).max()))
    assert float(np.sqrt((g["wav"] ** 2).mean())) > 0.05                  # a non-trivial signal
    # the oracle's own fold (the float64 truth's): the bar test_oracle_golden.py has for g5
    wav2 = obig.forward(sd, conf["vocoder_config"], torch.from_numpy(g["mel"]), 10 ** 9)
    assert np.abs(wav2.numpy() - g["wav"]).max() < 2e-6


def test_plain_stages_equal_the_plain_oracle(conf_var):
    """The by-keys dispatch leaves a checkpoint of plain stages on the plain path: the shipped configuration's waveform and taps
    against the reference's (g5), by the criterion of test_oracle_golden.py::test_bigvgan_stage_taps."""
    g = load_golden("g5_bigvgan_taps")
    sd = synth.generator_state_dict(conf_var, seed=int(g["seed"]))
    assert not any(".act." in k or "filter" in k for k in sd)
    taps = {}
    w = obig.forward(sd, conf_var["vocoder_config"], torch.from_numpy(g["mel"]), 10 ** 9, taps=taps)
    assert np.abs(w.numpy() - g["wav"]).max() < 2e-6
    for i in range(4):
        assert taps[f"up{i}"].shape[2] == g[f"up{i}"].shape[2]
        assert np.abs(taps[f"up{i}"].numpy() - g[f"up{i}"]).max() < 1e-4
        mean3 = (g[f"res{i}_0"] + g[f"res{i}_1"] + g[f"res{i}_2"]) / 3
        assert np.abs(taps[f"stage{i}"].numpy() - mean3).max() < 1e-4
    assert np.abs(taps["conv_pre"].numpy() - g["conv_pre"]).max() < 1e-5


# ----------------------------------------------------------------------------------------------- 2. key layouts
def test_config_accepts_the_switches_and_checks_the_list(tmp_path, conf_var):
    from bvcodec import config
    for tag, sw in vl.AA_CONFIGS.items():
        c = vl.write_config(str(tmp_path / f"{tag}.toml"), switches=sw)
        assert config.antialias_flags(c) == (sw["layers_antialias"], sw["antialias_post"]) and config.is_antialiased(c)
    assert config.antialias_flags(conf_var) == ([False] * 4, False) and not config.is_antialiased(conf_var)
    bad = vl.with_switches(conf_var, dict(layers_antialias=[True, False, True], antialias_post=False))
    with pytest.raises(ValueError, match="layers_antialias"):
        config.check_supported(bad)
    sym = vl.with_switches(conf_var, vl.AA_CONFIGS["all"])
    sym["vocoder_config"]["layers_sym"] = [True, False, False, False]
    with pytest.raises(ValueError, match="causal"):
        config.check_supported(sym)
    snake = vl.with_switches(conf_var, vl.AA_CONFIGS["all"])
    snake["vocoder_config"]["activation"] = "snake"
    with pytest.raises(ValueError, match="snakebeta"):
        config.check_supported(snake)


@pytest.mark.parametrize("tag", sorted(vl.AA_CONFIGS))
def test_checkpoint_keys_follow_the_config_both_ways(conf_var, tag):
    layers, post = vl.AA_CONFIGS[tag]["layers_antialias"], vl.AA_CONFIGS[tag]["antialias_post"]
    conf = vl.with_switches(conf_var, vl.AA_CONFIGS[tag])
    vr = synth.bvrnn_state_dict(conf_var, 3)
    g_aa, g_plain = synth.generator_state_dict(conf, 4), synth.generator_state_dict(conf_var, 4)
    ht = weights.host_tensors(conf, vr, g_aa)                              # loads under its own config
    assert ht["layers_antialias"].tolist() == [float(f) for f in layers] and ht["antialias_post"].tolist() == [float(post)]
    nk = len(conf["vocoder_config"]["resblock_kernel_sizes"])
    for n in range(4 * nk):
        name = f"resblocks.{n}.activations.5"
        if layers[n // nk]:
            assert ht[name + ".upsample.filter"].shape == (1, 1, 12) and ht[name + ".downsample.lowpass.filter"].shape == (1, 1, 12)
            assert name + ".act.alpha" in ht and name + ".alpha" not in ht
        else:
            assert name + ".alpha" in ht and name + ".act.alpha" not in ht and name + ".upsample.filter" not in ht
    assert ("activation_post.act.beta" in ht) == post and ("activation_post.beta" in ht) == (not post)
    assert "layers_antialias" not in weights.host_tensors(conf_var, vr, g_plain)
    with pytest.raises(RuntimeError, match=r"Missing key\(s\): \['resblocks.*Unexpected key\(s\): \['resblocks"):
        weights.host_tensors(conf_var, vr, g_aa)                           # refused under a shipped config
    with pytest.raises(RuntimeError, match=r"Missing key\(s\): \['resblocks.*Unexpected key\(s\): \['resblocks"):
        weights.host_tensors(conf, vr, g_plain)                            # a shipped-layout checkpoint under the filtered config
    # the reference's filter: 12 taps of a Kaiser-windowed sinc, unit sum, symmetric
    f = g_aa["resblocks.0.activations.0.upsample.filter"].flatten()
    assert abs(float(f.sum()) - 1.0) < 1e-6 and torch.equal(f, f.flip(0)) and abs(float(f[5]) - 0.4432) < 1e-4


def test_synthetic_draws_of_the_shipped_configs_are_unchanged(conf_var):
    """The same order of random numbers as before: g5's weights, regenerated, still give g5's waveform (the bar of
    test_oracle_golden.py), and a filtered layout holds the same alpha / beta / conv draws under its own names."""
    g = load_golden("g5_bigvgan")
    sd = synth.generator_state_dict(conf_var, seed=int(g["seed"]))
    w = obig.forward(sd, conf_var["vocoder_config"], torch.from_numpy(g["mel"]), 8192)
    assert np.abs(w.numpy() - g["wav_8192"]).max() < 2e-6
    assert not any(".act." in k or "filter" in k for k in sd)
    sd_aa = synth.generator_state_dict(vl.with_switches(conf_var, vl.AA_CONFIGS["mixed"]), seed=int(g["seed"]))
    for k, v in sd.items():
        k2 = k if k in sd_aa else k.replace(".alpha", ".act.alpha").replace(".beta", ".act.beta")
        assert torch.equal(sd_aa[k2], v), k


# ----------------------------------------------------------------------------------------------- 3. reach
@pytest.mark.parametrize("ks,d", [(3, 1), (11, 5)])
def test_reach_of_one_filtered_pair(conf_all, ks, d):
    """Perturbing x[s] changes out[t] exactly for s in [t - (ks-1)(d+1) - 10, t + 10]: the halo of the GPU tiles."""
    pair = next(p for p in vl.pairs(conf_all) if p[3] == 8 and p[4] == ks and p[5] == d)
    i, j, m, C, _, _, pre = pair
    sd = synth.generator_state_dict(conf_all, 1235)
    L, t = 200, 120
    x = vl.make_input("n1", 1, C, L, L, 5).double()
    base = obig.amp_pair(sd, pre, m, x, ks, d, dtype=torch.float64)
    lo, hi = t - vl.halo(ks, d), t + 2 * obig.REACH
    assert lo == t - (ks - 1) * (d + 1) - 10 and hi == t + 10
    for s in range(lo - 12, hi + 13):
        xp = x.clone()
        xp[:, :, s] += 0.5
        changed = bool((obig.amp_pair(sd, pre, m, xp, ks, d, dtype=torch.float64)[:, :, t] != base[:, :, t]).any())
        assert changed == (lo <= s <= hi), (s, lo, hi, changed)


def test_reach_of_one_activation(conf_all):
    sd = {k: v.double() for k, v in synth.generator_state_dict(conf_all, 1235).items()}
    x = vl.make_input("n1", 1, 8, 60, 60, 6).double()
    base = obig.activation(sd, "activation_post", x, torch.float64)
    assert base.shape == x.shape
    for s in range(30 - 9, 30 + 10):
        xp = x.clone()
        xp[:, :, s] += 0.5
        changed = bool((obig.activation(sd, "activation_post", xp, torch.float64)[:, :, 30] != base[:, :, 30]).any())
        assert changed == (abs(s - 30) <= obig.REACH), s


# ----------------------------------------------------------------------------------------------- 4. conditioning
@pytest.mark.parametrize("draw", vl.DRAWS)
def test_filtered_pair_is_well_conditioned_in_float32(conf_all, draw):
    """max|oracle32 - oracle64| <= 5e-6 max|oracle64|, the bound the plain pairs have: the GPU test's bar
    8 x max(e32, 2^-24 max|oracle64|) means something on every draw."""
    sd = vl.generator_draw(conf_all, draw)
    pair = next(p for p in vl.pairs(conf_all) if p[3] == 64 and p[4] == 11 and p[5] == 5)
    i, j, m, C, ks, d, pre = pair
    for kind in ("n1", "n6"):
        x = vl.make_input(kind, 2, C, 300, 300, 11)
        r64 = obig.amp_pair(sd, pre, m, x, ks, d, dtype=torch.float64)
        r32 = obig.amp_pair(sd, pre, m, x, ks, d, dtype=torch.float32)
        e32, scale = float((r32.double() - r64).abs().max()), float(r64.abs().max())
        print(f"CONDITIONING draw={draw} input={kind} e32/scale={e32 / scale:.3e}")
        assert e32 <= 5e-6 * scale, (draw, kind, e32, scale)
