"""The rate cap of closed-loop encoding and the sessions that choose their own rates, without a GPU: the capped oracle against the
uncapped one, the capped cases' own conditions, the bucket's arithmetic and its window guarantee, the new symbols of the C ABI, the
argument errors of ``encode_vbr(rate_cap=)`` and ``StreamingCodec(vbr=)`` (raised before anything is created), and the wire of a
session tick as numpy states it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vbr_cap_oracle as vc
import vbr_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h_dim, draw, B, T, ladder, rate [bits per frame], burst [bits])
CASES = ((128, "wide", 5, 20, (8, 16, 32, 64), 20, 96), (1024, "default", 3, 6, (17, 35, 64), 30, 70))
NEW_SYMBOLS = ("bvc_bvrnn_encode_vbr_capped", "bvc_encode_vbr_capped", "bvc_test_vbr_select_capped", "bvc_stream_codec_create_vbr",
               "bvc_stream_codec_set_target", "bvc_stream_codec_sizes", "bvc_stream_codec_bits")


def test_cap_off_is_the_uncapped_oracle():
    c = vo.make_case(*CASES[0][:5])
    for dtype in (torch.float32, torch.float64):
        ref = vo.encode_vbr(c.sd, c.y, c.ladder, c.tau, c.h0, dtype)
        got = vc.encode_vbr_capped(c.sd, c.y, c.ladder, c.tau, c.h0, dtype=dtype)
        for k, v in ref.items():
            assert torch.equal(got[k], v), k
        assert got["tok_next"] is None and torch.equal(got["k_target"], ref["choice"])
    # a bucket that never empties changes nothing either
    big = vc.encode_vbr_capped(c.sd, c.y, c.ladder, c.tau, c.h0, rate_q8=64 * 256, burst_q8=64 * 256)
    ref = vo.encode_vbr(c.sd, c.y, c.ladder, c.tau, c.h0)
    assert torch.equal(big["codes"], ref["codes"]) and torch.equal(big["all_h"], ref["all_h"])
    assert big["tok_next"].tolist() == ((64 - ref["bits"][:, -1]) * 256).long().tolist()      # refilled to the brim before every frame


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"h{c[0]}-{c[1]}")
def test_capped_cases_meet_their_conditions(case):
    """The cap binds on at least two frames and does not on at least two, step 1's min clamps at least once, every D the rule looks at
    lies a margin from its target and the two precisions make the same choices; then the guarantee on every window of every row."""
    c = vc.make_case(*case)
    n_bind, n_free, n_clamp = vc.check_case(c)
    o = c.o64
    assert case[4][0] * 256 <= c.rate_q8                              # the premise of the guarantee
    slack = vc.check_windows(o["bits"], c.rate_q8, c.burst_q8)
    print(f"cap binds on {n_bind} frames, not on {n_free}, clamps {n_clamp} times; tightest window slack {slack / 256:g} bits; "
          f"rungs {[int((o['choice'] == k).sum()) for k in range(len(c.ladder))]}")
    # a cut anywhere changes nothing once tok travels with h
    T = c.y.shape[1]
    cut = T // 2
    a = vc.encode_vbr_capped(c.sd, c.y[:, :cut], c.ladder, c.tau[:, :cut], c.h0, c.rate_q8, c.burst_q8, dtype=torch.float64)
    z = vc.encode_vbr_capped(c.sd, c.y[:, cut:], c.ladder, c.tau[:, cut:], a["h_last"], c.rate_q8, c.burst_q8, tok0=a["tok_next"],
                             dtype=torch.float64)
    assert torch.equal(torch.cat([a["choice"], z["choice"]], 1), o["choice"]) and torch.equal(z["tok_next"], o["tok_next"])
    assert torch.equal(torch.cat([a["codes"], z["codes"]], 1), o["codes"])


def test_bucket_arithmetic():
    lad = (8, 16, 32, 64)
    # full bucket of 96 bits, 20 per frame: the top rung, then what is left
    k, tok, i = vc.bucket_step(96 * 256, 3, lad, 20 * 256, 96 * 256)
    assert (k, tok, i["a"], i["clamped"], i["floored"]) == (3, 32 * 256, 3, True, False)
    k, tok, i = vc.bucket_step(tok, 3, lad, 20 * 256, 96 * 256)
    assert (k, tok, i["a"], i["clamped"]) == (2, 20 * 256, 2, False)          # 52 bits: rung 2, the cap binds
    k, tok, i = vc.bucket_step(tok, 0, lad, 20 * 256, 96 * 256)
    assert (k, tok, i["a"]) == (0, 32 * 256, 2)                               # the target asks for less than the bucket holds
    # exactly enough counts as enough; one q8 less does not
    assert vc.bucket_step(16 * 256 - 5, 3, lad, 5, 96 * 256)[0] == 1
    assert vc.bucket_step(16 * 256 - 6, 3, lad, 5, 96 * 256)[0] == 0
    # a rate below rung 0: nothing is affordable, rung 0 goes out all the same and the bucket stops at zero (step 4's max)
    tiny = (8, 16)
    k, tok, i = vc.bucket_step(8 * 256, 1, tiny, 2 * 256, 8 * 256)
    assert (k, tok, i["floored"]) == (0, 0, False)
    k, tok, i = vc.bucket_step(tok, 1, tiny, 2 * 256, 8 * 256)
    assert (k, tok, i["a"], i["floored"]) == (0, 0, 0, True)


def test_tiny_case_runs_the_floor_of_step_4():
    c = vo.make_case(128, "wide", 2, 6, (8, 16))
    o = vc.encode_vbr_capped(c.sd, c.y, c.ladder, torch.full((2, 6), -float("inf")), c.h0, rate_q8=2 * 256, burst_q8=8 * 256)
    assert int(o["floored"].sum()) >= 2 and bool((o["choice"] == 0).all()) and o["tok_next"].tolist() == [0, 0]
    with pytest.raises(AssertionError):                               # and without its premise the guarantee does not hold
        vc.check_windows(o["bits"], 2 * 256, 8 * 256)


def test_window_guarantee_on_a_rate_target():
    """A target of -inf spends whatever the bucket allows: random ladders, rates and bursts, integers only."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        K = int(rng.integers(1, 9))
        lad = sorted(rng.choice(np.arange(0, 65), size=K, replace=False).tolist())
        rate = int(rng.integers(lad[0] * 256, 70 * 256))
        burst = int(rng.integers(lad[0] * 256, 200 * 256))
        tok, bits = burst, []
        for t in range(40):
            k, tok, _ = vc.bucket_step(tok, int(rng.integers(0, K)) if t % 3 else K - 1, lad, rate, burst)
            bits.append(lad[k])
        vc.check_windows(np.array([bits]), rate, burst)


_CTYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", "bvcodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"([a-z_0-9]+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/bvcodec.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_declared_exported_and_bound_alike(name):
    from bvcodec import _abi
    lib = _abi.load()
    assert hasattr(lib, name) and lib.bvc_abi_version() == 3
    ret, args = _declared(name)
    res, argtypes = _abi.SIGNATURES[name]
    assert res is _CTYPES[ret]
    assert len(args) == len(argtypes), (args, argtypes)
    for a, ct in zip(args, argtypes):
        if "*" in a:
            assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, a, ct)
            if issubclass(ct, ctypes._Pointer) and "**" not in a:
                assert ct._type_ is _CTYPES[a.replace("const ", "").split()[0]], (name, a, ct)
        else:
            assert ct is _CTYPES[a.split()[0]], (name, a, ct)


def test_uncapped_entries_keep_their_signatures():
    from bvcodec import _abi
    assert len(_abi.SIGNATURES["bvc_bvrnn_encode_vbr"][1]) == 18 and len(_abi.SIGNATURES["bvc_encode_vbr"][1]) == 13
    assert _abi.SIGNATURES["bvc_bvrnn_encode_vbr_capped"][1][:18] == _abi.SIGNATURES["bvc_bvrnn_encode_vbr"][1]
    assert _abi.SIGNATURES["bvc_encode_vbr_capped"][1][:13] == _abi.SIGNATURES["bvc_encode_vbr"][1]


def _facade(tmp_path, conf, cfg_path):
    from bvcodec import BVRNNCodecModel, synth
    p1, p2 = synth.write_checkpoints(conf, str(tmp_path), seed=7)
    return BVRNNCodecModel(cfg_path, p1, p2).eval()


def test_cap_units():
    from bvcodec import config
    from bvcodec.model import cap_q8
    conf = config.load_config(config.DEFAULT_CONFIG)
    assert cap_q8(conf, [17, 35, 64], None, None) is None
    rate, burst = cap_q8(conf, [17, 35, 64], 2600, None)
    assert rate == round(2600 * conf["hopsize"] / conf["fs"] * 256) and burst == 4 * 64 * 256
    assert cap_q8(conf, [8, 16], 0, 8) == (0, 8 * 256)


def test_encode_vbr_cap_argument_errors(tmp_path, conf_var):
    from bvcodec import config
    m = _facade(tmp_path, conf_var, config.DEFAULT_CONFIG)
    x = torch.zeros(2, 256 * 10)
    with pytest.raises(ValueError, match="burst without rate_cap"):
        m.encode_vbr(x, 0.5, burst=96)
    with pytest.raises(ValueError, match="not negative"):
        m.encode_vbr(x, 0.5, rate_cap=-1)
    with pytest.raises(ValueError, match="not negative"):
        m.encode_vbr(x, 0.5, rate_cap=2000, burst=-3)
    with pytest.raises(ValueError, match="not negative"):
        m.encode_vbr(x, 0.5, rate_cap=float("nan"))
    with pytest.raises(ValueError, match="never holds rung 0"):
        m.encode_vbr(x, 0.5, rate_cap=2000, burst=16)                 # rung 0 of (1500, 3000, 6000) is 17 bits
    with pytest.raises(ValueError, match=r"2\^31"):
        m.encode_vbr(x, 0.5, rate_cap=1e9)
    y, h = torch.zeros(2, 10, 80), torch.zeros(1, 2, conf_var["h_dim"])
    with pytest.raises(ValueError, match="both rate_q8 and burst_q8"):
        m.bvrnn.encode_vbr(y, (16, 32), 0.5, h, rate_q8=100)
    with pytest.raises(ValueError, match="tok without"):
        m.bvrnn.encode_vbr(y, (16, 32), 0.5, h, tok=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="integers"):
        m.bvrnn.encode_vbr(y, (16, 32), 0.5, h, rate_q8=1.5, burst_q8=8000)
    with pytest.raises(ValueError, match="never holds rung 0"):
        m.bvrnn.encode_vbr(y, (16, 32), 0.5, h, rate_q8=0, burst_q8=16 * 256 - 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.encode_vbr(x, 0.5, rate_cap=2600, burst=96)


def test_streaming_codec_vbr_argument_errors(tmp_path, conf_var, conf_fix):
    """All ValueError before anything is created: none needs a GPU."""
    from bvcodec import config
    from bvcodec.streaming import StreamingCodec
    m = _facade(tmp_path, conf_var, config.DEFAULT_CONFIG)
    ok = dict(bitrates=(1500, 3000, 6000), target=0.35)
    for direction in ("send", "duplex"):
        with pytest.raises(ValueError, match="takes dict"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=True)
        with pytest.raises(ValueError, match="unknown keys.*ladder"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=dict(ok, ladder=(1, 2)))
        with pytest.raises(ValueError, match="ascend strictly"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=dict(ok, bitrates=(3000, 1500)))
        with pytest.raises(ValueError, match="1 to 8 rungs"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=dict(ok, bitrates=tuple(range(500, 5000, 500))))
        with pytest.raises(ValueError, match="burst without rate_cap"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=dict(ok, burst=96))
        with pytest.raises(ValueError, match="never holds rung 0"):
            StreamingCodec(m, 2, 3000, direction=direction, vbr=dict(ok, rate_cap=2600, burst=10))
    with pytest.raises(ValueError, match="vbr=True"):
        StreamingCodec(m, 2, 3000, direction="recv", vbr=ok)
    with pytest.raises(ValueError, match="no repair window"):
        StreamingCodec(m, 2, 3000, direction="recv", vbr=True, repair=8)
    fix = _facade(tmp_path, conf_fix, config.DEFAULT_CONFIG_64BIT)
    for direction, v in (("send", ok), ("recv", True)):
        with pytest.raises(ValueError, match="fixed-rate"):
            StreamingCodec(fix, 2, 3000, direction=direction, vbr=v)
    got = StreamingCodec._check_vbr(m, "send", 0, dict(ok, rate_cap=2600, burst=96))
    assert got == dict(ladder=[17, 35, 64], target=0.35, rate_q8=round(2600 * 256 / 22050 * 256), burst_q8=96 * 256)
    assert StreamingCodec._check_vbr(m, "duplex", 0, ok)["burst_q8"] == -1
    assert StreamingCodec._check_vbr(m, "recv", 0, True)["ladder"] == [] and StreamingCodec._check_vbr(m, "send", 0, None) is None


def test_tick_wire_stated_in_numpy():
    """Frame j of row b at (b * kmax + j) * stride, stride = 1 + ceil(Z / 8); sizes = 1 + ceil(n / 8) at b * kmax + j."""
    rng = np.random.default_rng(5)
    B, k, kmax, Z = 3, 2, 3, 64
    bits = np.array([[17, 64], [35, 0], [8, 9]], dtype=np.float32)
    raw = rng.integers(0, 2, size=(B, k, Z)).astype(np.float32)
    codes = np.where(np.arange(Z)[None, None, :] < bits[:, :, None], raw, np.float32(0.5))
    buf, sizes = vc.tick_wire(codes, bits, kmax)
    stride = 9
    assert buf.shape == (B * kmax * stride,) and sizes.shape == (B, kmax)
    assert sizes.tolist() == [[4, 9, 0], [6, 1, 0], [2, 3, 0]]
    for b in range(B):
        for j in range(k):
            fr = buf[(b * kmax + j) * stride:(b * kmax + j + 1) * stride]
            assert fr[0] == bits[b, j] and not fr[sizes[b, j]:].any()
            back, nb = vo.unpack_vbr(fr[None, None], Z)
            assert np.array_equal(back[0, 0], codes[b, j]) and nb[0, 0] == bits[b, j]
        assert not buf[(b * kmax + k) * stride:(b + 1) * kmax * stride].any()          # frames the tick did not emit
    assert buf[(0 * kmax + 0) * stride + 3] == int(codes[0, 0, 16])                      # 17 bits: one bit in the third byte of bits
