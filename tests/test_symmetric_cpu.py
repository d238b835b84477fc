"""Symmetric layers without a GPU: the oracle (oracle/bigvgan.py) against the reference's own run
(tests/golden/g11_bigvgan_sym_*.npz, written by tests/golden/make_golden_symmetric.py), the reach of one symmetric AMP pair - the
halo the GPU kernel's tiles are cut with -, and what config and weights make of the three switches."""
import numpy as np
import pytest
import torch

import vocoder_layers as vl
from conftest import load_golden
from bvcodec import config, synth, weights
from oracle import bigvgan as obig

TAPS = ("conv_pre", "stage0", "stage1", "stage2", "stage3")
SWITCHES = ("layers_sym", "pre_sym", "post_sym", "layers_antialias", "antialias_post")


# ----------------------------------------------------------------------------------------------- 1. the oracle is the reference
@pytest.mark.parametrize("tag", sorted(vl.SYM_CONFIGS))
def test_oracle_equals_reference_fixture_bit_for_bit(conf_var, tag):
    """Waveform and every tap, float32, with the weight fold of the reference's forward pre-hook and the fixture script's thread
    count (see test_antialias_cpu.py)."""
    g = load_golden(f"g11_bigvgan_sym_{tag}")
    sw = vl.SYM_CONFIGS[tag]
    for k in SWITCHES:
        assert g[k].tolist() == sw[k], k
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS[tag])
    sd = synth.generator_state_dict(conf, seed=int(g["seed"]))
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        taps = {}
        wav = obig.forward(sd, conf["vocoder_config"], torch.from_numpy(g["mel"]), 10 ** 9, taps=taps, fold=obig.REFERENCE_FOLD)
    finally:
        torch.set_num_threads(threads)
    assert wav.shape == g["wav"].shape
    assert np.array_equal(wav.numpy(), g["wav"]), float(np.abs(wav.numpy() - g["wav"]).max())
    for k in TAPS:
        assert taps[k].shape == g[k].shape, k
        assert np.array_equal(taps[k].numpy(), g[k]), (k, float(np.abs(taps[k].numpy() - g[k]).max()))
    assert float(np.sqrt((g["wav"] ** 2).mean())) > 0.05                  # a non-trivial signal


def test_every_switch_off_equals_the_plain_oracle(conf_var):
    """The five switches present and false (the shipped TOML) against a table without them (what a configuration from before the
    switches holds): the same bits, waveform and every tap."""
    v = conf_var["vocoder_config"]
    assert all(k in v and not any(np.atleast_1d(v[k])) for k in SWITCHES)
    bare = {k: f for k, f in v.items() if k not in SWITCHES}
    sd = synth.generator_state_dict(conf_var, 1235)
    mel = torch.from_numpy(load_golden("g11_bigvgan_sym_all")["mel"])
    taps, taps0 = {}, {}
    wav = obig.forward(sd, v, mel, 10 ** 9, taps=taps)
    assert torch.equal(wav, obig.forward(sd, bare, mel, 10 ** 9, taps=taps0))
    assert sorted(taps) == sorted(taps0) and all(torch.equal(taps[k], taps0[k]) for k in taps)


# ----------------------------------------------------------------------------------------------- 2. reach
@pytest.mark.parametrize("ks,d", [(ks, d) for ks in vl.KSIZES for d in vl.DILATIONS])
def test_reach_of_one_symmetric_pair(conf_var, ks, d):
    """Perturbing x[s] changes outputs up to (ks-1)(d+1)/2 rows away on each side, exactly the rows the two convs' taps reach,
    and no others."""
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS["all"])
    i, j, m, C, _, _, pre = next(p for p in vl.pairs(conf) if p[3] == 8 and p[4] == ks and p[5] == d)
    sd = synth.generator_state_dict(conf, 1235)
    h = vl.reach(ks, d)
    assert h == (ks - 1) * (d + 1) // 2 and 2 * h == (ks - 1) * (d + 1)
    L, s = 4 * h + 40, 2 * h + 17
    x = vl.make_input("n1", 1, C, L, L, 5).double()
    base = obig.amp_pair(sd, pre, m, x, ks, d, dtype=torch.float64, sym=True)
    assert base.shape == x.shape
    xp = x.clone()
    xp[:, :, s] += 0.5
    changed = (obig.amp_pair(sd, pre, m, xp, ks, d, dtype=torch.float64, sym=True) != base).any(dim=1)[0]
    # conv1's taps sit d rows apart and conv2's one row: the rows s + a d + b, |a|, |b| <= (ks-1)/2 (all of [s - h, s + h] where
    # d <= ks, and always both ends)
    p2 = (ks - 1) // 2
    rows = sorted({s + a * d + b for a in range(-p2, p2 + 1) for b in range(-p2, p2 + 1)})
    assert rows[0] == s - h and rows[-1] == s + h and (d > ks or rows == list(range(s - h, s + h + 1)))
    assert changed.nonzero().flatten().tolist() == rows, (ks, d, h)
    # and the causal form of the same pair reaches back only
    base_c = obig.amp_pair(sd, pre, m, x, ks, d, dtype=torch.float64, sym=False)
    changed_c = (obig.amp_pair(sd, pre, m, xp, ks, d, dtype=torch.float64, sym=False) != base_c).any(dim=1)[0]
    assert changed_c.nonzero().flatten().tolist() == [r + h for r in rows]


def test_symmetric_upsampler_is_a_view_of_the_causal_one(conf_var):
    """ConvTranspose1d(padding = (k - u) / 2), k = 2u: rows [u/2, u/2 + L u) of the unpadded result - what the GPU path computes."""
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS["all"])
    sd = synth.generator_state_dict(conf, 1235)
    v = conf["vocoder_config"]
    for i, u in enumerate(v["upsample_rates"]):
        x = vl.make_input("n1", 2, v["upsample_initial_channel"] >> i, 9, 9, 40 + i)
        full = obig.upsample(sd, v, i, x, torch.float64, sym=False)     # (float32: the CPU sums the two taps in another order)
        assert full.shape[2] == 10 * u
        assert torch.equal(obig.upsample(sd, v, i, x, torch.float64, sym=True), full[:, :, u // 2:u // 2 + 9 * u])


# ----------------------------------------------------------------------------------------------- 3. configuration and weights
def test_config_accepts_the_three_configurations(tmp_path, conf_var):
    for tag, sw in vl.SYM_CONFIGS.items():
        c = vl.write_config(str(tmp_path / f"{tag}.toml"), switches=sw)
        assert config.symmetric_flags(c) == (sw["layers_sym"], sw["pre_sym"], sw["post_sym"])
        assert config.antialias_flags(c) == (sw["layers_antialias"], sw["antialias_post"])
        assert not config.is_causal(c)
        assert "symmetric" in config.not_causal_message(c) or config.is_antialiased(c)
    assert "symmetric" in config.not_causal_message(vl.with_switches(conf_var, vl.SYM_CONFIGS["mixed"]))
    assert "anti-aliased" in config.not_causal_message(vl.with_switches(conf_var, vl.SYM_CONFIGS["with_aa"]))
    assert config.symmetric_flags(conf_var) == ([False] * 4, False, False) and config.is_causal(conf_var)
    only_aa = vl.with_switches(conf_var, dict(layers_antialias=[True, False, False, False]))
    assert not config.is_causal(only_aa) and config.symmetric_flags(only_aa) == ([False] * 4, False, False)


@pytest.mark.parametrize("tag", sorted(vl.SYM_CONFIGS))
def test_generator_length_equals_the_fixture(conf_var, tag):
    g = load_golden(f"g11_bigvgan_sym_{tag}")
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS[tag])
    T = g["mel"].shape[2]
    lens = config.generator_length(conf, T, stages=True)
    assert lens == [g[f"stage{i}"].shape[2] for i in range(4)] == vl.sym_lengths(conf["vocoder_config"], T)
    assert config.generator_length(conf, T) == g["wav"].shape[2] == lens[-1]
    expect = {"all": [96, 768, 1536, 3072], "mixed": [104, 832, 1666, 3332]}.get(tag)
    assert expect is None or lens == expect
    assert config.generator_length(conf_var, T) == 256 * T + 294


def test_config_refuses_what_is_not_built(conf_var):
    with pytest.raises(ValueError, match="layers_sym"):
        config.check_supported(vl.with_switches(conf_var, dict(layers_sym=[True, False, True])))
    even = vl.with_switches(conf_var, dict(layers_sym=[False, True, False, False]))
    even["vocoder_config"]["resblock_kernel_sizes"] = [3, 8, 11]
    with pytest.raises(ValueError, match="odd"):
        config.check_supported(even)
    even["vocoder_config"]["layers_sym"] = [False] * 4                   # a causal generator may have even kernels
    config.check_supported(even)
    both = vl.with_switches(conf_var, dict(layers_sym=[False, False, True, False], layers_antialias=[False, False, True, True]))
    with pytest.raises(ValueError, match="causal"):
        config.check_supported(both)
    post = vl.with_switches(conf_var, dict(post_sym=True, antialias_post=True))
    with pytest.raises(ValueError, match="causal"):
        config.check_supported(post)
    # what stays refused
    snake = vl.with_switches(conf_var, vl.SYM_CONFIGS["all"])
    snake["vocoder_config"]["activation"] = "snake"
    with pytest.raises(ValueError, match="snakebeta"):
        config.check_supported(snake)


@pytest.mark.parametrize("tag", sorted(vl.SYM_CONFIGS))
def test_host_tensors_carry_the_flags(conf_var, tag):
    sw = vl.SYM_CONFIGS[tag]
    conf = vl.with_switches(conf_var, vl.SYM_CONFIGS[tag])
    vr, gen = synth.bvrnn_state_dict(conf_var, 3), synth.generator_state_dict(conf, 4)
    ht = weights.host_tensors(conf, vr, gen)
    assert ht["layers_sym"].tolist() == [float(f) for f in sw["layers_sym"]]
    assert ht["pre_sym"].tolist() == [float(sw["pre_sym"])] and ht["post_sym"].tolist() == [float(sw["post_sym"])]
    assert ("layers_antialias" in ht) == (any(sw["layers_antialias"]) or sw["antialias_post"])
    # the switches add no keys: the same draws under the same names as the causal layout of the same filters
    plain = synth.generator_state_dict(vl.with_switches(conf_var, dict(layers_antialias=sw["layers_antialias"],
                                                                          antialias_post=sw["antialias_post"])), 4)
    assert list(plain) == list(gen) and all(torch.equal(plain[k], gen[k]) for k in gen)


def test_a_causal_configuration_carries_no_flag_tensor(conf_var):
    ht = weights.host_tensors(conf_var, synth.bvrnn_state_dict(conf_var, 3), synth.generator_state_dict(conf_var, 4))
    assert not {"layers_sym", "pre_sym", "post_sym"} & set(ht)
