"""Closed-loop variable-rate encoding without a GPU: the oracle against oracle.bvrnn.encode, the test cases' own margins, the new
symbols of the C ABI, the per-frame wire format as numpy states it, and the facade's argument errors (raised before the library is
called)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vbr_oracle as vo
from oracle import bvrnn as obv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((128, "wide", 5, 20, (8, 16, 32, 64)), (1024, "default", 3, 6, (17, 35, 64)))
NEW_SYMBOLS = ("bvc_vbr_workspace_bytes", "bvc_bvrnn_encode_vbr", "bvc_encode_vbr", "bvc_pack_codes_vbr", "bvc_unpack_codes_vbr",
               "bvc_test_vbr_select")


@pytest.mark.parametrize("n", [16, 64])
def test_oracle_with_one_rung_is_the_plain_encoder(n):
    c = vo.make_case(*CASES[0])
    B, T = c.y.shape[:2]
    got = vo.encode_vbr(c.sd, c.y, (n,), torch.full((B, T), float("nan")), c.h0)
    ref = obv.encode(c.sd, c.y, torch.full((B, T), float(n)), c.h0)
    assert torch.equal(got["codes"], ref["codes"]) and torch.equal(got["all_h"], ref["all_h"])
    assert bool((got["bits"] == n).all()) and bool((got["choice"] == 0).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"h{c[0]}-{c[1]}")
def test_cases_keep_their_margins(case):
    """Every D the rule looks at lies 1e-4 from its target, every rung and the fallback occur at least twice, no probability that
    reaches a candidate lies within 5e-6 of 0.5, and the float32 oracle makes the float64 oracle's choices on the same targets."""
    c = vo.make_case(*case)
    counts = vo.check_case(c)
    e = float((c.o64["dist"] - c.o32["dist"].double()).abs().max())
    print(f"chosen rungs {counts}, fallback frames {int(c.fallback.sum())}, max |D32 - D64| {e:.2e}")
    assert e < vo.MARGIN / 20                                   # the margin is far above float32 noise
    assert c.tau.dtype == torch.float32 and tuple(c.tau.shape) == tuple(c.y.shape[:2])


def test_choice_rule_at_the_edges():
    D = torch.tensor([[3.0, 2.0, 1.0]] * 6)
    nan, inf = float("nan"), float("inf")
    tau = torch.tensor([2.0, 0.5, nan, inf, -inf, 1.0])       # D_k == tau counts; nothing meets 0.5; NaN and -inf: the last rung; +inf: rung 0
    assert vo.choose(D, tau).tolist() == [1, 2, 2, 0, 2, 2]
    assert vo.choose(torch.tensor([[nan, 1.0]]), torch.tensor([2.0])).tolist() == [1]


_CTYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", "bvcodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"([a-z_0-9]+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/bvcodec.h"
    args = [" ".join(a.split()) for a in m.group(2).split(",")]
    return m.group(1), args


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
            is_ptr = ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer)
            assert is_ptr, (name, a, ct)
            if issubclass(ct, ctypes._Pointer):
                assert ct._type_ is _CTYPES[a.replace("const ", "").split()[0]], (name, a, ct)
        else:
            assert ct is _CTYPES[a.split()[0]], (name, a, ct)


def test_workspace_query_refuses_without_a_model():
    from bvcodec import _abi
    lib = _abi.load()
    assert lib.bvc_vbr_workspace_bytes(None, 4, 10, 3) == 0


def test_wire_format_stated_in_numpy():
    rng = np.random.default_rng(3)
    B, T, Z = 3, 7, 64
    bits = rng.integers(0, Z + 1, size=(B, T)).astype(np.float32)
    bits[0, 0], bits[0, 1], bits[0, 2], bits[0, 3] = 0, Z, 8, 9
    raw = rng.integers(0, 2, size=(B, T, Z)).astype(np.float32)
    codes = np.where(np.arange(Z)[None, None, :] < bits[:, :, None], raw, np.float32(0.5))
    packed, sizes = vo.pack_vbr(codes, bits)
    assert packed.shape == (B, T, 9) and packed.dtype == np.uint8
    assert np.array_equal(packed[:, :, 0], bits.astype(np.uint8))
    assert np.array_equal(sizes, 1 + np.ceil(bits / 8).astype(np.int32))
    assert sizes[0, 0] == 1 and sizes[0, 1] == 9 and sizes[0, 2] == 2 and sizes[0, 3] == 3
    for b in range(B):
        for t in range(T):
            assert not packed[b, t, sizes[b, t]:].any()                      # the rest of the stride is zero
            n = int(bits[b, t])
            if n % 8:
                assert packed[b, t, sizes[b, t] - 1] >> (n % 8) == 0         # and so are the bits of the last byte behind n
    assert packed[0, 3, 1] == sum(int(codes[0, 3, i]) << i for i in range(8))   # bit i at byte i / 8, LSB first
    back, nb = vo.unpack_vbr(packed, Z)
    assert np.array_equal(back, codes) and np.array_equal(nb, bits)
    # a header above z_dim reads as z_dim
    wild = packed.copy()
    wild[1, 1, 0] = 255
    back, nb = vo.unpack_vbr(wild, Z)
    assert nb[1, 1] == Z and set(np.unique(back[1, 1])) <= {0.0, 1.0}
    assert vo.stride_of(16) == 3 and vo.stride_of(17) == 4


def _facade(tmp_path, conf, cfg_path):
    from bvcodec import BVRNNCodecModel, synth
    p1, p2 = synth.write_checkpoints(conf, str(tmp_path), seed=7)
    return BVRNNCodecModel(cfg_path, p1, p2).eval()


def test_facade_argument_errors(tmp_path, conf_var):
    """All of them ValueError, raised before the library is called: none needs a GPU."""
    from bvcodec import config
    m = _facade(tmp_path, conf_var, config.DEFAULT_CONFIG)
    x = torch.zeros(2, 256 * 10)
    with pytest.raises(ValueError, match=r"ascend strictly.*35, 64, 64"):
        m.encode_vbr(x, 0.5, bitrates=(3000, 6000, 12000))            # 70 and 139 bits both saturate at z_dim = 64
    with pytest.raises(ValueError, match=r"ascend strictly"):
        m.encode_vbr(x, 0.5, bitrates=(3000, 1500))
    with pytest.raises(ValueError, match="1 to 8 rungs"):
        m.encode_vbr(x, 0.5, bitrates=tuple(range(500, 5000, 500)))
    with pytest.raises(ValueError, match="1 to 8 rungs"):
        m.encode_vbr(x, 0.5, bitrates=())
    for bad in (torch.zeros(3), torch.zeros(2, 11), torch.zeros(2, 10, 1)):
        with pytest.raises(ValueError, match="target must be"):
            m.encode_vbr(x, bad)
    with pytest.raises(ValueError, match="lengths"):
        m.encode_vbr(x, 0.5, lengths=[2560, 2000])
    y, h = torch.zeros(2, 10, 80), torch.zeros(1, 2, conf_var["h_dim"])
    with pytest.raises(ValueError, match="ascend strictly"):
        m.bvrnn.encode_vbr(y, (16, 16), 0.5, h)
    with pytest.raises(ValueError, match=r"\[0, 64\]"):
        m.bvrnn.encode_vbr(y, (16, 65), 0.5, h)
    with pytest.raises(ValueError, match="integer"):
        m.bvrnn.encode_vbr(y, (16.5, 32), 0.5, h)
    with pytest.raises(ValueError, match="target must be"):
        m.bvrnn.encode_vbr(y, (16, 32), torch.zeros(10), h)
    with pytest.raises(ValueError, match="pack_vbr"):
        m.pack_vbr(torch.zeros(2, 10, 64), torch.zeros(2, 9))
    with pytest.raises(ValueError, match="unpack_vbr"):
        m.unpack_vbr(torch.zeros(2, 10, 8, dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):    # well-formed arguments get as far as the device
            m.encode_vbr(x, 0.5)


def test_facade_refuses_a_fixed_rate_model(tmp_path, conf_fix):
    from bvcodec import config
    m = _facade(tmp_path, conf_fix, config.DEFAULT_CONFIG_64BIT)
    with pytest.raises(ValueError, match="fixed-rate"):
        m.encode_vbr(torch.zeros(2, 2560), 0.5)
    with pytest.raises(ValueError, match="fixed-rate"):
        m.bvrnn.encode_vbr(torch.zeros(2, 10, 80), (16, 32), 0.5, torch.zeros(1, 2, conf_fix["h_dim"]))
