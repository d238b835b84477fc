"""Wide generators (``upsample_initial_channel`` 256 and 512) without a GPU: the test oracle against the reference's own run
(tests/golden/g12_bigvgan_wide_*.npz, written by tests/golden/make_golden_wide.py), what config, the C ABI's admission check and
weights make of the width, and the arithmetic of the tile shapes restated in tests/vocoder_layers.py."""
import ctypes

import numpy as np
import pytest
import torch

import vocoder_layers as vl
from conftest import load_golden
from bvcodec import config, synth, weights
from oracle import bigvgan as obig

TAPS = ("conv_pre", "stage0", "stage1", "stage2", "stage3")


# ----------------------------------------------------------------------------------------------- 1. the oracle is the reference
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_oracle_equals_reference_fixture_bit_for_bit(conf_var, width):
    """Waveform and every stored tap, float32, with the weight fold of the reference's forward pre-hook and the fixture script's
    thread count (see test_antialias_cpu.py)."""
    g = load_golden(f"g12_bigvgan_wide_{width}")
    assert int(g["width"]) == width and g["conv_pre"].shape[1] == width
    conf = vl.with_switches(conf_var, width=width)
    sd = synth.generator_state_dict(conf, seed=int(g["seed"]))
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        taps = {}
        wav = obig.forward(sd, conf["vocoder_config"], torch.from_numpy(g["mel"]), 10 ** 9, taps=taps, fold=obig.REFERENCE_FOLD)
    finally:
        torch.set_num_threads(threads)
    assert wav.shape == g["wav"].shape
    assert torch.equal(wav, torch.from_numpy(g["wav"])), float(np.abs(wav.numpy() - g["wav"]).max())
    for k in TAPS:
        assert taps[k].shape == g[k].shape, k
        assert torch.equal(taps[k], torch.from_numpy(g[k])), (k, float(np.abs(taps[k].numpy() - g[k]).max()))
    rms, peak = float(np.sqrt((g["wav"] ** 2).mean())), float(np.abs(g["wav"]).max())
    assert (round(rms, 4), round(peak, 4)) == {256: (0.0733, 0.2951), 512: (0.0891, 0.2469)}[width]
    assert [g[f"stage{i}"].shape[1:] for i in range(4)] == [(width >> (i + 1), L) for i, L in enumerate((56, 456, 914, 1830))]


# ----------------------------------------------------------------------------------------------- 2. configuration
def test_config_accepts_the_wide_generators(tmp_path, conf_var, conf_fix):
    for width in vl.WIDTHS:
        c = vl.write_config(str(tmp_path / f"wide{width}.toml"), width=width)
        assert c["vocoder_config"]["upsample_initial_channel"] == width and c["h_dim"] == conf_var["h_dim"]
        assert config.is_causal(c) and vl.stage_channels(c) == [width >> (i + 1) for i in range(4)]
        assert vl.write_config(str(tmp_path / f"wide{width}_64.toml"), width=width, h_dim=64)["h_dim"] == 64
    for path in (config.DEFAULT_CONFIG, config.DEFAULT_CONFIG_64BIT):
        assert config.load_config(path)["vocoder_config"]["upsample_initial_channel"] == 128
    for c0 in (16, 32, 64, 128):                                           # what the library took before, with the stages that end at 8
        narrow = vl.with_switches(conf_var, width=c0)
        n = {16: 1, 32: 2, 64: 3, 128: 4}[c0]
        for key in ("upsample_rates", "upsample_kernel_sizes"):
            narrow["vocoder_config"][key] = conf_var["vocoder_config"][key][4 - n:]
        for key in ("layers_sym", "layers_antialias"):
            narrow["vocoder_config"].pop(key, None)
        config.check_supported(narrow)


def test_config_refuses_other_widths(conf_var):
    for c0 in (1024, 96):
        with pytest.raises(ValueError, match="upsample_initial_channel"):
            config.check_supported(vl.with_switches(conf_var, width=c0))
    three = vl.with_switches(conf_var, width=512)                                   # three stages: 64 channels in front of conv_post
    for key in ("upsample_rates", "upsample_kernel_sizes", "layers_sym", "layers_antialias"):
        if key in three["vocoder_config"]:
            three["vocoder_config"][key] = three["vocoder_config"][key][:3]
    with pytest.raises(ValueError, match="upsample_initial_channel"):
        config.check_supported(three)


@pytest.mark.parametrize("key", ["layers_sym", "layers_antialias"])
def test_config_refuses_the_switches_on_wide_stages_only(conf_var, key):
    """Stages of 128 and 256 channels have the causal, unfiltered kernels only; the narrow stages of a wide generator take both."""
    for width, wide in ((256, [0]), (512, [0, 1])):
        for i in range(4):
            c = vl.with_switches(vl.with_switches(conf_var, width=width), {key: [k == i for k in range(4)]})
            if i in wide:
                with pytest.raises(ValueError, match=key):
                    config.check_supported(c)
            else:
                config.check_supported(c)
    config.check_supported(vl.with_switches(conf_var, {key: [True] * 4}))          # the shipped width: every stage


# ----------------------------------------------------------------------------------------------- 3. admission in the library
def _create(width, n_up=4):
    """bvc_model_create with the struct of test_abi_cpu.py::test_model_create_fails_loudly_without_gpu and another width."""
    from bvcodec import _abi
    lib = _abi.load()
    cfg = _abi.BvcConfig()
    cfg.num_mels, cfg.h_dim, cfg.z_dim, cfg.var_bit = 80, 1024, 64, 1
    cfg.n_fft, cfg.hop, cfg.pad_left, cfg.sample_rate = 1024, 256, 256, 22050
    cfg.upsample_initial_channel, cfg.n_up, cfg.n_resk = width, n_up, 3
    for i, (u, k) in enumerate(((8, 16), (8, 16), (2, 4), (2, 4))[:n_up]):
        cfg.up_rates[i], cfg.up_kernels[i] = u, k
    t = (_abi.BvcTensor * 1)()
    dummy = np.zeros(4, dtype=np.float32)
    t[0].name, t[0].h_data, t[0].numel = b"mean_mel", dummy.ctypes.data, 4
    h = ctypes.c_void_p()
    rc = lib.bvc_model_create(ctypes.byref(cfg), t, 1, ctypes.byref(h))
    return rc, lib.bvc_last_error()


def test_model_create_admits_the_wide_generators():
    """The configuration check runs before the device check: an admitted width gets as far as "no HIP device" (or, on a GPU, as far
    as the missing tensors), a refused one is BVC_EINVAL on either machine."""
    passed = (-4,) if torch.cuda.is_available() else (-5,)                 # BVC_EMISSING / BVC_ENODEVICE
    for width in (512, 256, 128):
        rc, msg = _create(width)
        assert rc in passed and b"upsample_initial_channel" not in msg, (width, rc, msg)
    rc, msg = _create(1024)
    assert rc == -1 and b"upsample_initial_channel" in msg, (rc, msg)      # BVC_EINVAL
    rc, msg = _create(512, n_up=3)
    assert rc == -1 and b"final channel count" in msg, (rc, msg)
    rc, msg = _create(16, n_up=2)
    assert rc == -1 and b"too many upsampling stages" in msg, (rc, msg)


# ----------------------------------------------------------------------------------------------- 4. weights, lengths
@pytest.mark.parametrize("width", vl.WIDTHS)
def test_host_tensors_carry_the_wide_tensors(conf_var, width):
    conf = vl.with_switches(conf_var, width=width)
    ht = weights.host_tensors(conf, synth.bvrnn_state_dict(conf_var, 3), synth.generator_state_dict(conf, 4))
    v = conf["vocoder_config"]
    assert tuple(ht["conv_pre.weight"].shape) == (width, 80, 7) and ht["conv_pre.bias"].numel() == width
    for i, (u, C) in enumerate(zip(v["upsample_rates"], vl.stage_channels(conf))):
        assert tuple(ht[f"ups.{i}.1.weight"].shape) == (2 * C, C, 2 * u)
        for j, ks in enumerate(v["resblock_kernel_sizes"]):
            pre = f"resblocks.{i * 3 + j}"
            for m in range(3):
                assert tuple(ht[f"{pre}.convs1.{m}.weight"].shape) == tuple(ht[f"{pre}.convs2.{m}.weight"].shape) == (C, C, ks)
            for a in range(6):
                assert ht[f"{pre}.activations.{a}.alpha"].numel() == ht[f"{pre}.activations.{a}.beta"].numel() == C
    last = width >> 4
    assert tuple(ht["conv_post.weight"].shape) == (1, last, 7) and ht["activation_post.alpha"].numel() == last
    assert not {"layers_sym", "layers_antialias"} & set(ht)
    for T in (1, 6, 430):
        assert config.generator_length(conf, T) == config.generator_length(conf_var, T) == 256 * T + 294
    assert config.generator_length(conf, 6, stages=True) == [56, 456, 914, 1830]


# ----------------------------------------------------------------------------------------------- 5. the geometry restatement
def test_tile_geometry_fits_the_lds():
    """Every compiled shape of the wide channel counts, every (ks, d): LDS within 160 KiB, the S2 tile and the output staging
    inside the S1 rows, and at least one valid output row."""
    for C in vl.WIDE_CHANNELS:
        assert vl.AMP_HEIGHTS[C][0] == vl.AMP_HEIGHT[C]
        for h in vl.AMP_HEIGHTS[C] + (vl.AMP_SHORT,):
            assert h % 16 == 0
            for ks in vl.KSIZES:
                for d in vl.DILATIONS:
                    assert 0 < vl.amp_lds_bytes(C, ks, d, h) <= vl.LDS_LIMIT, (C, h, ks, d)
                    assert h - (ks - 1) > 0
                    assert vl.amp_tile_rows(C, ks, d, 10 ** 6, False, height=h) == (h - (ks - 1), f"amp{C}/{h}")
    assert vl.amp_lds_bytes(256, 11, 5, 64) == 114 * 258 * 4 and vl.amp_lds_bytes(128, 11, 5, 64) == 114 * 130 * 4
    for ks in vl.KSIZES:
        short = vl.AMP_SHORT - (ks - 1)
        for C in vl.WIDE_CHANNELS:
            assert vl.amp_tile_rows(C, ks, 1, short, True) == (short, f"amp{C}/window32")
            assert vl.amp_tile_rows(C, ks, 1, short + 1, True) == (vl.AMP_HEIGHT[C] - (ks - 1), f"amp{C}/{vl.AMP_HEIGHT[C]}/window")
            assert vl.amp_tile_rows(C, ks, 1, short, False)[0] == vl.AMP_HEIGHT[C] - (ks - 1)
        assert vl.wide_window_new_rows(ks)[:2] == [1, 8] and short in vl.wide_window_new_rows(ks) and short + 1 in vl.wide_window_new_rows(ks)
    narrow = {64: (122, "amp64/128"), 32: (250, "amp32/256"), 16: (250, "amp16/persistent"), 8: (246, "amp8/full<2,2>")}
    for C in (64, 32, 16, 8):                                              # the narrow stages keep their geometry beside the wide ones
        assert vl.amp_tile_rows(C, 7, 3, 1000, False) == narrow[C]
    # upsamplers out of 512 and 256 channels (2 taps), conv_pre (7 taps, 80 channels whatever the width), conv_post
    assert vl.conv_tile_rows(512) == 64 and vl.conv_tile_rows(256) == 128 and vl.conv_tile_rows(128) == 128
    assert vl.conv_lds_bytes(512, 2, 1, vl.conv_tile_rows(512)) == 65 * 514 * 4 <= vl.LDS_LIMIT
    assert vl.conv_lds_bytes(256, 2, 1, vl.conv_tile_rows(256)) == 129 * 258 * 4 <= vl.LDS_LIMIT
    assert vl.conv_lds_bytes(512, 2, 1, 128) > vl.LDS_LIMIT                # why the 512-channel upsampler has 64-row tiles
    for cin in (512, 256):
        assert vl.conv_lds_bytes(cin, 2, 1, 16) <= 64 * 1024               # streaming hops: the column-split form, 16 rows
    for C in (16, 32):
        assert vl.post_lds_bytes(C, 7) <= 34 * 1024 and vl.post_lds_bytes(C, 7, antialias=True) <= vl.LDS_LIMIT
    # the host's row guard: 2 M rows at C = 256, 4 M at C = 128
    assert vl.max_rows(256) == 2097151 - 512 and vl.max_rows(128) == 4194303 - 512
    assert (vl.max_rows(256) + vl.ROW_GUARD) * 256 * 4 < 2 ** 31 and (vl.max_rows(128) + vl.ROW_GUARD) * 128 * 4 < 2 ** 31
