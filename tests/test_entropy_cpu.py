"""The entropy-coded wire format without a GPU: the numpy coder of entropy_oracle.py against its own specification (round trips, the
overhead bound, the carry path, a stride that is too small), what the constructed checkpoints of the GPU tests reach on the float32
oracle, and the surface (header, exports, signatures, the facade's argument checks)."""
import os
import re

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import conceal_oracle as co
import entropy_oracle as eo
from oracle import bvrnn as obv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 5, 35
SYMBOLS = ("bvc_entropy_stride", "bvc_entropy_workspace_bytes", "bvc_entropy_encode", "bvc_entropy_decode", "bvc_bvrnn_entropy_pack",
           "bvc_bvrnn_entropy_unpack", "bvc_decode_entropy")


@pytest.mark.parametrize("segment", [1, 8, None])
@pytest.mark.parametrize("z_dim", [16, 64, 128])
@pytest.mark.parametrize("kind", eo.PROB_CLASSES)
def test_round_trip_and_overhead(kind, z_dim, segment):
    """35 frames in segments of 8 leave a ragged last segment of 3; the bit counts 0, 1, 34.5, z_dim and 1000 walk over rows and frames,
    so segments of one frame are empty where the count is 0.  Extreme probabilities get 2 % wrong bits: 16 bits each."""
    p = eo.prob_case(kind, B, T, z_dim, seed=3)
    codes = eo.draw_codes(p, 3, wrong=0.02 if kind == "extreme" else 0.0)
    bits = eo.bits_case(B, T, z_dim)
    o = eo.pack(codes, p, bits, segment)
    assert np.array_equal(eo.unpack(o["data"], o["sizes"], p, bits, segment), eo.masked(codes, bits))
    assert (o["sizes"] >= 0).all() and (o["sizes"] <= o["data"].shape[2]).all()
    assert (o["sizes"][o["n"] == 0] == 0).all()                                     # a segment without a coded bit has no bytes
    slack = 8.0 * o["sizes"] - o["ideal"] - eo.TRUNC * o["n"]
    print(f"{kind} z {z_dim} segment {segment}: {int(o['n'].sum())} bits in {int(o['sizes'].sum())} bytes, ideal {o['ideal'].sum() / 8:.1f} bytes, "
          f"largest 8 size - ideal - {eo.TRUNC} n = {slack.max():.2f} bits, empty segments {int((o['n'] == 0).sum())}, carry {bool(o['carried'].any())}")
    assert eo.overhead_ok(o["sizes"], o["ideal"], o["n"]).all()
    for s in range(o["sizes"].shape[1]):                                              # bytes from size to stride are zero
        for b in range(B):
            assert not o["data"][b, s, o["sizes"][b, s]:].any()


def test_empty_call_and_single_symbols():
    p = eo.prob_case("flat", 2, 4, 16, seed=1)
    codes = eo.draw_codes(p, 1)
    none = np.zeros((2, 4), dtype=np.float32)
    o = eo.pack(codes, p, none, 2)
    assert not o["sizes"].any() and not o["data"].any()
    assert np.array_equal(eo.unpack(o["data"], o["sizes"], p, none, 2), np.full((2, 4, 16), 0.5, dtype=np.float32))
    for q, b in ((1, 0), (1, 1), (65535, 0), (65535, 1), (32768, 0), (32768, 1)):
        stored, _ = eo.encode_segment([b], [q])
        assert eo.decode_segment(stored, [q]) == [b] and len(stored) <= 4


def test_the_carry_path_is_exercised():
    """2240 symbols, default_rng(8), uniform p, bits drawn from q: a carry runs into pending 0xFF bytes.  The seed was chosen on the CPU."""
    codes, p, bits = eo.carry_case()
    o = eo.pack(codes, p, bits)
    assert bool(o["carried"].all())
    assert np.array_equal(eo.unpack(o["data"], o["sizes"], p, bits), codes)
    assert eo.overhead_ok(o["sizes"], o["ideal"], o["n"]).all()


def test_a_stride_that_is_too_small():
    p = eo.prob_case("flat", 3, 16, 64, seed=2)
    codes = eo.draw_codes(p, 2)
    bits = np.full((3, 16), 64.0, dtype=np.float32)
    full = eo.pack(codes, p, bits, 8)
    small = int(full["sizes"].max()) - 1
    cut = eo.pack(codes, p, bits, 8, stride=small)
    assert ((cut["sizes"] == -1) == (full["sizes"] > small)).all() and (cut["sizes"] == -1).any()
    assert np.array_equal(cut["data"], full["data"][:, :, :small])
    assert eo.safe_stride(64, 8) == 2 * 8 * 64 + 0 + 8 and eo.safe_stride(64, 430) == 2 * 430 * 64 + 26 + 8


def test_quantisation():
    p = np.array([0.0, 1.0, 1e-6, 1 - 1e-6, 0.5, 1.5 / 65536, 2.5 / 65536, np.nan, 7.62939453125e-06], dtype=np.float32)
    assert eo.quantise(p).tolist() == [1, 65535, 1, 65535, 32768, 2, 2, 1, 1]       # round-half-even; the clamp; 0.5 / 65536 rounds to 0, clamped


# ---------------------------------------------------------------------------------------------- the constructed checkpoints
def matched(sd):
    """pin_logits with the prior's table equal to the encoder's: the prior predicts every bit."""
    sd = bd.pin_logits(sd)
    sd["prior.4.bias"] = sd["enc.4.bias"].clone()
    return sd


def oracle_stream(sd, h_dim, Bm=5, Tm=24):
    """The float32 oracle's codes of the pinned inputs and the prior along the decoder's own states."""
    y, _ = bd.inputs(Bm, Tm)
    bits = bd.pinned_bits(Bm, Tm)
    h0 = torch.zeros(Bm, h_dim)
    codes = obv.encode(sd, y, bits, h0)["codes"]
    prior = co.decode_with_prior(sd, codes, h0)["prior"]
    return codes.numpy(), prior.numpy(), bits.numpy()


def test_constructed_checkpoints():
    """matched: the ideal code length is less than half of the one stored bit per coded bit that pack spends.  Mismatched (the stock
    pin_logits, whose prior table is another permutation): the stream is LONGER than pack's, and still within the safe stride."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    base = bd.state_dict(64, "default")
    for name, sd in (("matched", matched(base)), ("mismatched", bd.pin_logits(base))):
        codes, prior, bits = oracle_stream(sd, 64)
        o = eo.pack(codes, prior, bits, 8)
        n = int(o["n"].sum())
        ideal, stored = float(o["ideal"].sum()) / n, 8.0 * float(o["sizes"].sum()) / n
        print(f"{name}: {n} coded bits, ideal {ideal:.4f} bit per bit, stored {stored:.4f} bit per bit (pack: 1), largest segment "
              f"{int(o['sizes'].max())} of {o['data'].shape[2]} bytes")
        assert np.array_equal(eo.unpack(o["data"], o["sizes"], prior, bits, 8), codes)
        assert eo.overhead_ok(o["sizes"], o["ideal"], o["n"]).all()
        if name == "matched":
            assert ideal < 0.5
        else:
            assert ideal > 1.0 and stored > 1.0
            assert (o["sizes"] >= 0).all() and int(o["sizes"].max()) <= eo.safe_stride(64, 8)


# ---------------------------------------------------------------------------------------------- the surface
def test_symbols_in_header_exports_and_signatures():
    from bvcodec import _abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvcodec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bvc_[a-z_0-9]+)\s*\(", hdr))
    lib = _abi.load()
    for name in SYMBOLS:
        assert name in declared and name in _abi.SIGNATURES and hasattr(lib, name), name
    assert lib.bvc_entropy_stride(64, 8) == eo.safe_stride(64, 8) and lib.bvc_entropy_stride(128, 35) == eo.safe_stride(128, 35)
    assert lib.bvc_entropy_stride(64, 0) == -1 and lib.bvc_entropy_stride(0, 4) == -1
    assert lib.bvc_entropy_workspace_bytes(None, 4, 10) == 0
    assert lib.bvc_abi_version() == 3


@pytest.fixture(scope="module")
def cpu_models(tmp_path_factory, conf_var, conf_fix):
    from bvcodec import BVRNNCodecModel, config, synth
    out = {}
    for var, conf, cfg in ((True, conf_var, config.DEFAULT_CONFIG), (False, conf_fix, config.DEFAULT_CONFIG_64BIT)):
        p1, p2 = synth.write_checkpoints(conf, str(tmp_path_factory.mktemp("ck")), seed=7)
        out[var] = BVRNNCodecModel(cfg, p1, p2)
    return out


def test_facade_argument_checks_need_no_device(cpu_models):
    m = cpu_models[True]
    codes = torch.full((2, 6, 64), 0.5)
    data, sizes = torch.zeros(2, 2, 9, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32)
    h = torch.zeros(1, 2, 1024)
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(ValueError, match="segment"):
            m.pack_entropy(codes, bitrate=3000, segment=bad)
        with pytest.raises(ValueError, match="segment"):
            m.unpack_entropy(data, sizes, 6, bitrate=3000, segment=bad)
        with pytest.raises(ValueError, match="segment"):
            m.decode_entropy(data, sizes, 6, 1000, bitrate=3000, segment=bad)
        with pytest.raises(ValueError, match="segment"):
            m.bvrnn.entropy_pack(codes, torch.zeros(2, 6), h, segment=bad)
    with pytest.raises(ValueError, match="bitrate"):
        m.pack_entropy(codes)                                                       # a variable-rate model needs the rate
    with pytest.raises(ValueError, match="bitrate"):
        m.unpack_entropy(data, sizes, 6, segment=3)
    with pytest.raises(ValueError, match="bitrate"):
        m.decode_entropy(data, sizes, 6, 1000, segment=3)
    with pytest.raises(ValueError, match="not both"):
        m.pack_entropy(codes, bitrate=3000, bits=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="bits must be"):
        m.pack_entropy(codes, bits=torch.zeros(2, 5))
    with pytest.raises(ValueError, match="mixed"):
        m.pack_entropy(codes, bitrate=[3000, 1500])
    with pytest.raises(ValueError, match="mixed"):
        m.decode_entropy(data, sizes, 6, [1000, 900], bitrate=3000, segment=3)
    with pytest.raises(ValueError, match="codes must be"):
        m.pack_entropy(torch.zeros(2, 6, 32), bitrate=3000)
    with pytest.raises(ValueError, match="uint8"):
        m.unpack_entropy(data.float(), sizes, 6, bitrate=3000, segment=3)
    with pytest.raises(ValueError, match="uint8"):
        m.unpack_entropy(data[0], sizes, 6, bitrate=3000, segment=3)
    with pytest.raises(ValueError, match="sizes"):
        m.unpack_entropy(data, sizes[:, :1], 6, bitrate=3000, segment=3)
    with pytest.raises(ValueError, match="sizes"):
        m.unpack_entropy(data, sizes.float(), 6, bitrate=3000, segment=3)
    with pytest.raises(ValueError, match="segments given"):
        m.unpack_entropy(data, sizes, 6, bitrate=3000, segment=2)                    # 6 frames in segments of 2 make 3
    with pytest.raises(ValueError, match="segments given"):
        m.decode_entropy(data, sizes, 6, 1000, bitrate=3000)                         # the whole call is one segment
    with pytest.raises(ValueError, match="frames"):
        m.unpack_entropy(data, sizes, 0, bitrate=3000)
    with pytest.raises(ValueError, match="bits"):
        m.bvrnn.entropy_unpack(data, sizes, 6, None, h, segment=3)
    f = cpu_models[False]
    if not torch.cuda.is_available():                                                # a fixed-rate model needs no rate: the call gets as far as the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f.pack_entropy(codes)
