"""Concealment of lost frames from the prior net, without a GPU: the operator's definition (tests/conceal_oracle.py, composed from
the CPU oracle's pieces) against golden vectors stepped with the reference's own modules (tests/golden/make_golden_conceal.py), the
facade's argument checks, and the new symbols."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from bvcodec import synth
from oracle import bvrnn as obv

import conceal_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)

FIXTURES = [("h64_var", 64, True), ("h1024_fix", 1024, False)]
NEW_SYMBOLS = ("bvc_bvrnn_decode_conceal", "bvc_decode_conceal", "bvc_stream_codec_set_conceal")


def t(a):
    return torch.from_numpy(np.asarray(a))


def _conf(conf_var, h_dim, var_bit):
    c = dict(conf_var); c["h_dim"] = h_dim; c["var_bit"] = var_bit
    return c


@pytest.mark.parametrize("tag,h_dim,var_bit", FIXTURES)
def test_fixture_loss_pattern(tag, h_dim, var_bit):
    """What the fixtures are for: an isolated loss, a burst of >= 5 frames, a lost frame 0, one row without loss; NaN at the lost
    positions of the stored codes."""
    g = load_golden(f"g9_conceal_{tag}")
    p = g["present"].astype(bool)
    assert p.shape == (2, 40) and g["codes"].shape == (2, 40, 64)
    assert not p[0, 0] and p[1].all()
    lost = (~p[0]).astype(int)
    runs = [len(r) for r in "".join(map(str, lost)).split("0") if r]
    assert 1 in runs and max(runs) >= 5
    assert np.isnan(g["codes"][~p]).all() and not np.isnan(g["codes"][p]).any()
    assert not np.isnan(g["codes_out"]).any() and set(np.unique(g["codes_out"])) <= {0.0, 0.5, 1.0}


@pytest.mark.parametrize("tag,h_dim,var_bit", FIXTURES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_conceal_oracle_matches_reference_modules(tag, h_dim, var_bit, dtype, conf_var):
    """The bars tests/test_oracle_golden.py holds for g3_* / g8_*: codes equal, probabilities < 1e-6 (mel 2e-5, state 2e-6)."""
    g = load_golden(f"g9_conceal_{tag}")
    sd = synth.bvrnn_state_dict(_conf(conf_var, h_dim, var_bit), seed=int(g["seed"]))
    r = co.decode_conceal(sd, t(g["codes"]), t(g["present"]), t(g["bits"]), torch.zeros(2, h_dim), var_bit=var_bit, dtype=dtype)
    assert np.array_equal(r["codes_out"].float().numpy(), g["codes_out"])
    assert np.abs(r["prior"].double().numpy() - g["prior"]).max() < 1e-6
    assert np.abs(r["mel"].double().numpy() - g["mel"]).max() < 2e-5
    assert np.abs(r["h_last"].double().numpy() - g["h_last"]).max() < 2e-6
    present = g["present"].astype(bool)
    assert np.array_equal(g["codes_out"][present], g["codes"][present])              # received codes pass through
    # the generated bits lie away from a tie (the seed search of the generator), so the equality above is meaningful
    act = np.arange(64)[None, None, :] < (g["bits"][:, :, None] if var_bit else 64)
    gen = act & ~present[:, :, None]
    assert gen.sum() > 300 and np.abs(g["prior"] - 0.5)[gen].min() > 1e-5
    if var_bit:
        assert (g["codes_out"][~present][~act[~present]] == 0.5).all()


@pytest.mark.parametrize("tag,h_dim,var_bit", FIXTURES)
def test_row_without_loss_is_plain_decode(tag, h_dim, var_bit, conf_var):
    """With every frame present the operator IS BVRNN.decode: the oracle's decode of the filled codes gives the same bits, and the row
    that lost nothing got its codes back."""
    g = load_golden(f"g9_conceal_{tag}")
    sd = synth.bvrnn_state_dict(_conf(conf_var, h_dim, var_bit), seed=int(g["seed"]))
    h0 = torch.zeros(2, h_dim)
    r = co.decode_conceal(sd, t(g["codes"]), t(g["present"]), t(g["bits"]), h0, var_bit=var_bit)
    assert torch.equal(r["codes_out"][1], t(g["codes"][1]))
    d = obv.decode(sd, r["codes_out"], h0)
    assert torch.equal(d["mel"][1], r["mel"][1]) and torch.equal(d["h_last"][1], r["h_last"][1])
    assert torch.equal(d["mel"], r["mel"])                                            # (and so does the row with losses)
    assert torch.equal(co.prior_at_states(sd, r["codes_out"], h0), r["prior"])


def test_concealed_frames_differ_from_frames_of_no_bits(conf_var):
    """A sanity line on the fixtures' kind of data, not a test of the feature (it calls no new entry point and passes without it).
    Keeps the GPU tests meaningful: on the lost frames the concealed mel and the no-bits mel differ by far more than the GPU mel
    bar (2e-4), so a path that silently decodes 0.5 cannot pass.  Synthetic weights, h 1024, 8 x 120 frames, 5 % loss plus a burst."""
    sd = synth.bvrnn_state_dict(conf_var, seed=1234)
    B, T, nb = 8, 120, 35
    rng = np.random.default_rng(5)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
    bits = torch.full((B, T), float(nb))
    h0 = torch.zeros(B, 1024)
    codes = obv.encode(sd, y, bits, h0, var_bit=True)["codes"]
    present = co.loss_pattern(B, T, 0.05, seed=3)
    a = co.decode_conceal(sd, codes, present, bits, h0, var_bit=True)
    b = co.decode_conceal(sd, codes, present, bits, h0, var_bit=True, mode="none")
    per_frame = (a["mel"] - b["mel"]).abs().amax(-1)[~present]
    med, mx = float(per_frame.median()), float(per_frame.max())
    print(f"lost frames {int((~present).sum())}: |mel(prior) - mel(no bits)| median {med:.2e} max {mx:.2e}")
    assert med >= 10 * 2e-4, (med, mx)
    assert torch.equal(b["codes_out"][~present], torch.full_like(b["codes_out"][~present], 0.5))


def test_new_symbols_in_header_exports_and_signatures():
    from bvcodec import _abi
    hdr = open(os.path.join(ROOT, "include", "bvcodec.h")).read()
    declared = set(re.findall(r"\b(bvc_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.SIGNATURES and hasattr(lib, name), name
    assert len(_abi.SIGNATURES["bvc_bvrnn_decode_conceal"][1]) == 14
    assert len(_abi.SIGNATURES["bvc_decode_conceal"][1]) == 13
    assert lib.bvc_abi_version() == 3
    assert "no concealment from the model's prior" not in hdr


def test_facade_argument_checks_need_no_device(tmp_path, conf_var, conf_fix):
    from bvcodec import BVRNNCodecModel, config, synth as sy
    from bvcodec.streaming import StreamingCodec
    p1, p2 = sy.write_checkpoints(conf_var, str(tmp_path), seed=7)
    m = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2)
    codes = torch.full((2, 6, 64), 0.5)
    lost = torch.zeros(2, 6, dtype=torch.bool)
    with pytest.raises(ValueError, match="mixed-length"):
        m.decode(codes, 1536, frames=[6, 4], lost=lost, bitrate=3000)
    with pytest.raises(ValueError, match="mixed-length"):
        m.decode(codes, [1536, 1000], lost=lost, bitrate=3000)
    with pytest.raises(ValueError, match="bitrate"):
        m.decode(codes, 1536, lost=lost)
    with pytest.raises(ValueError, match="lost"):
        m.decode(codes, 1536, lost=lost[:, :5], bitrate=3000)
    with pytest.raises(ValueError, match="bits"):
        m.bvrnn.decode(codes, torch.zeros(1, 2, 1024), present=~lost)
    for direction in ("send", "duplex"):
        with pytest.raises(ValueError, match="receive session"):
            StreamingCodec(m, 2, 3000, direction=direction, conceal="prior")
    with pytest.raises(ValueError, match="conceal must be"):
        StreamingCodec(m, 2, 3000, direction="recv", conceal="zeros")
