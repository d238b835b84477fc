"""What the per-layer parity tests of the generator (test_gpu_vocoder_layers.py) stand on, checked without a GPU: the single-layer
oracle functions compose to ``forward`` bit for bit, one AMP pair is well conditioned in float32 on every weight draw the GPU tests
use (so that a bar of a few times the float32 oracle's own error means something), the tile geometry the GPU tests assume, and the
comparison function rejects a single wrong element and a row taken from its neighbour."""
import numpy as np
import pytest
import torch

import vocoder_layers as vl
from oracle import bigvgan as obig


@pytest.fixture(scope="module")
def vcfg(conf_var):
    return conf_var["vocoder_config"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_single_layer_oracle_composes_to_forward_bit_for_bit(conf_var, vcfg, dtype):
    sd = vl.generator_draw(conf_var, "seed1235")
    rng = np.random.default_rng(3)
    mel = torch.from_numpy((-4 + 1.6 * rng.standard_normal((2, 80, 9))).astype(np.float32))
    taps = {}
    for length in (1500, 10 ** 9):
        ref = obig.forward(sd, vcfg, mel, length, dtype=dtype, taps=taps)
        with torch.no_grad():
            x = obig.conv_pre(sd, mel, dtype)
            assert torch.equal(x, taps["conv_pre"])
            nk = len(vcfg["resblock_kernel_sizes"])
            for i in range(len(vcfg["upsample_rates"])):
                n_in = x.shape[2]
                x = obig.upsample(sd, vcfg, i, x, dtype)
                assert torch.equal(x, taps[f"up{i}"]) and x.shape[2] == (n_in + 1) * vcfg["upsample_rates"][i]
                xs = None
                for j, ks in enumerate(vcfg["resblock_kernel_sizes"]):
                    r = x
                    for m, d in enumerate(vcfg["resblock_dilation_sizes"][j]):
                        r = obig.amp_pair(sd, f"resblocks.{i * nk + j}", m, r, ks, d, dtype=dtype)
                    xs = r if xs is None else xs + r
                x = xs / nk
                assert torch.equal(x, taps[f"stage{i}"])
            wav = obig.conv_post(sd, x, length, dtype)
        assert wav.dtype == dtype and wav.shape == ref.shape and torch.equal(wav, ref)


def test_upsampler_output_length(conf_var, vcfg):
    sd = vl.generator_draw(conf_var, "seed8")
    x = torch.zeros(1, 128, 5)
    for i, u in enumerate(vcfg["upsample_rates"]):
        x = obig.upsample(sd, vcfg, i, x)
        assert x.shape[1] == vl.CHANNELS[i]
    assert x.shape[2] == (((5 + 1) * 8 + 1) * 8 + 1) * 2 * 2 + 2


@pytest.mark.parametrize("draw", vl.DRAWS)
def test_one_amp_pair_is_well_conditioned_in_float32(conf_var, draw):
    """The precondition of the bar: e32 / max|oracle64| <= 5e-6 for every pair of every draw on both noise inputs (B = 2, L = 1,500).
    Measured: at most 1.6e-7 on the synthetic draws (alpha, beta ~ N(0, 0.3)) and 1.6e-6 on the wide one (N(0, 1))."""
    sd = vl.generator_draw(conf_var, draw)
    worst = 0.0
    with torch.no_grad():
        for pair in vl.pairs(conf_var):
            C = pair[3]
            for kind in ("n1", "n6"):
                x = vl.make_input(kind, 2, C, 1500, 0, seed=17 + C)
                r64 = vl.oracle_pair(sd, pair, x, torch.float64)
                r32 = vl.oracle_pair(sd, pair, x, torch.float32)
                assert r32.dtype == torch.float32 and r64.dtype == torch.float64
                rel = float((r32.double() - r64).abs().max() / r64.abs().max())
                worst = max(worst, rel)
                assert rel <= 5e-6, (draw, pair, kind, rel)
    print(f"draw {draw}: worst e32 / max|oracle64| over 36 pairs x 2 inputs = {worst:.2e}")


def test_wide_draw_is_wide_and_keeps_the_convs(conf_var):
    base, wide = vl.generator_draw(conf_var, "seed1235"), vl.generator_draw(conf_var, "wide")
    assert list(base) == list(wide)
    al = torch.cat([wide[k] for k in wide if k.endswith(".alpha")])
    assert 0.9 < float(al.std()) < 1.1 and float(al.max()) > 2.5          # exp(alpha) beyond 12
    for k in base:
        assert (k.endswith(".alpha") or k.endswith(".beta")) != torch.equal(base[k], wide[k]), k


def test_tile_geometry_table():
    """The restatement of the launchers' tile shapes (every GPU case also checks it against what the launch reports)."""
    assert vl.amp8_tile_rows(3, 1, 2) == 254 and vl.amp8_tile_rows(11, 3, 2) == 242 and vl.amp8_tile_rows(7, 5, 2) == 244
    assert vl.amp8_tile_rows(11, 5, 1) == 110
    assert vl.amp_tile_rows(64, 7, 3, 1000, False, height=96) == (90, "amp64/96")
    assert vl.amp_tile_rows(64, 7, 3, 26, True)[0] == 26 and vl.amp_tile_rows(64, 7, 3, 27, True)[0] == 58
    assert vl.amp_tile_rows(64, 7, 3, 116, True)[0] == 58 and vl.amp_tile_rows(64, 7, 3, 117, True)[0] == 122
    assert vl.amp_tile_rows(32, 11, 5, 162, True)[0] == 54 and vl.amp_tile_rows(32, 11, 5, 163, True)[0] == 246
    assert vl.amp_tile_rows(16, 3, 1, 500, False)[0] == 254 and vl.amp_tile_rows(16, 3, 1, 500, False, c16=False)[0] == 126
    assert vl.amp_tile_rows(16, 3, 1, 500, True)[0] == 126
    assert vl.amp_tile_rows(8, 3, 5, 128, True)[0] == 118 and vl.amp_tile_rows(8, 3, 5, 129, True)[0] == 248
    assert vl.amp_tile_rows(8, 3, 5, 129, True, c8=False)[0] == 254
    for ks in vl.KSIZES:
        for d in vl.DILATIONS:
            ls = vl.lengths(128 - (ks - 1), ks, d)
            assert ls[0] == 1 and ls[-1] == 3 * (128 - (ks - 1)) + 17 and all(a < b for a, b in zip(ls, ls[1:]))


# ---------------------------------------------------------------------------------------------- the comparison has teeth
def _pair_case(conf_var):
    sd = vl.generator_draw(conf_var, "seed1235")
    pair = next(p for p in vl.pairs(conf_var) if p[3] == 64 and p[4] == 7 and p[5] == 3)
    TT = 128 - 6
    x = vl.make_input("n1", 3, 64, 2 * TT + 1, TT, seed=5)
    with torch.no_grad():
        return TT, vl.cl(vl.oracle_pair(sd, pair, x, torch.float64)), vl.cl(vl.oracle_pair(sd, pair, x, torch.float32))


def test_comparison_accepts_the_float32_oracle_and_names_one_moved_element(conf_var):
    TT, r64, r32 = _pair_case(conf_var)
    v = vl.compare(r32, r64, r32, "case", tile_rows=TT)
    assert v.ok and v.ratio == 1.0
    bad = r32.copy()
    bad[1, TT, 37] += 1e-4 * np.abs(r64).max()                       # first row of the second tile, one channel
    v = vl.compare(bad, r64, r32, "case", tile_rows=TT)
    assert not v.ok and v.worst == (1, TT, 37) and v.row_in_tile == 0
    assert "item 1, row %d, channel 37" % TT in v.message and "row % TT = 0" in v.message
    lost = r32.copy()
    lost[2, 5, 3] = np.nan                                           # an element nobody wrote
    v = vl.compare(lost, r64, r32, "case", tile_rows=TT)
    assert not v.ok and v.worst == (2, 5, 3)


def test_comparison_rejects_a_row_taken_from_its_neighbour(conf_var):
    TT, r64, r32 = _pair_case(conf_var)
    bad = r32.copy()
    bad[0, TT - 1] = r32[0, TT - 2]                                  # the last row of the first tile repeats the row before
    v = vl.compare(bad, r64, r32, "case", tile_rows=TT)
    assert not v.ok and v.worst[:2] == (0, TT - 1) and v.row_in_tile == TT - 1 and f"row {TT - 1}," in v.message
    ledger = vl.Ledger("seed1235")
    ledger.add("amp64/128", v)
    with pytest.raises(AssertionError, match="1 of 1 cases failed"):
        ledger.close()


def test_comparison_floor_for_an_exact_float32_oracle():
    ref = np.ones((2, 4, 8))
    got = ref.copy()
    got[0, 0, 0] += 4 * vl.U                                         # four units in the last place of the largest value: inside 8 u
    assert vl.compare(got, ref, ref, "x").ok
    got[0, 0, 0] = 1 + 16 * vl.U
    assert not vl.compare(got, ref, ref, "x").ok
