"""Mixed-rate sessions, the host side: the constructor's refusals (no device), the client hops of a 20 ms tick, the scalar refusals as
they were, the four new symbols of the ABI and ``bvc_resampler_create_multi``'s refusals before any device, and the per-slot finish
plans."""
import ctypes
import os
import re

import pytest

from resample_cases import FS, GEOMETRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES7 = (8000, 16000, 24000, 32000, 44100, 48000, 22050)             # the six usual rates and the model's own
NEW_SYMBOLS = ("bvc_resampler_create_multi", "bvc_resampler_set_taps_rate", "bvc_resampler_open_rate", "bvc_resampler_push_multi")


@pytest.fixture(scope="module")
def model(tmp_path_factory, conf_var):
    from bvcodec import BVRNNCodecModel, config, synth
    p1, p2 = synth.write_checkpoints(conf_var, str(tmp_path_factory.mktemp("mixed")), seed=7)
    return BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2)


def check(model, hop, client_rate, direction="duplex", fmt="f32"):
    from bvcodec.streaming import StreamingCodec
    return StreamingCodec._check_args(model, hop, direction, "none", 0, client_rate, fmt, None)


def test_mixed_refusals_need_no_device(model):
    """Every refusal is a ValueError that matches client_rate and names the offending rate, from _check_args and from the constructor."""
    from bvcodec.streaming import StreamingCodec
    with pytest.raises(ValueError, match=r"client_rate 48000.*478\.912"):                 # 220 internal samples: no whole hop at 48 kHz
        check(model, 220, (44100, 48000, 8000))
    with pytest.raises(ValueError, match=r"client_rate 16000.*0\.725624"):
        check(model, 1, (22050, 16000))
    with pytest.raises(ValueError, match="client_rate.*9"):
        check(model, 441, (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000))
    with pytest.raises(ValueError, match="client_rate.*0"):
        check(model, 441, ())
    with pytest.raises(ValueError, match="client_rate.*16000.*twice"):
        check(model, 441, (8000, 16000, 16000))
    with pytest.raises(ValueError, match=r"client_rate.*16000\.5"):
        check(model, 441, (16000.5,))
    for bad in (0, -8000):
        with pytest.raises(ValueError, match=f"client_rate.*{bad}"):
            check(model, 441, [16000, bad])
    with pytest.raises(ValueError, match="sample_format"):
        check(model, 441, (16000, 48000), fmt="s24")
    with pytest.raises(ValueError, match="conceal"):                                       # the other refusals still come
        StreamingCodec._check_args(model, 441, "send", "prior", 0, (16000,), "f32", None)
    with pytest.raises(ValueError, match=r"client_rate 48000"):                            # ... and the constructor raises them first
        StreamingCodec(model, 2, 3000, hop=220, client_rate=(44100, 48000))
    # a receive session has no hop to check; a list is a tuple afterwards
    assert check(model, 220, [8000, 48000], direction="recv") == (None, (8000, 48000), 0)


def test_twenty_millisecond_hops_pass(model):
    vbr, rates, hop_in = check(model, 441, RATES7, fmt="s16")
    assert vbr is None and rates == RATES7 and hop_in == 441
    assert [441 * r // FS for r in rates] == [160, 320, 480, 640, 882, 960, 441]
    assert all(441 * r % FS == 0 for r in rates)
    assert check(model, 882, (48000,)) == (None, (48000,), 882)                            # one listed rate is a mixed session too


def test_scalar_refusals_are_what_they_were(model):
    with pytest.raises(ValueError, match=r"480.*220\.5|220\.5.*480"):
        check(model, 480, 48000)
    for bad_rate in (0, -16000, 16000.5):
        with pytest.raises(ValueError, match="client_rate must be a positive number of Hz"):
            check(model, 320, bad_rate)
    with pytest.raises(ValueError, match="sample_format: a session without client_rate speaks float32"):
        check(model, 441, None, fmt="s16")
    assert check(model, 320, 16000) == (None, 16000, 441)
    assert check(model, 441, FS) == (None, None, 441) and check(model, 441, None) == (None, None, 441)
    assert check(model, 441, FS, fmt="s16") == (None, FS, 441)


def test_abi_has_the_multi_rate_resampler():
    from bvcodec import _abi
    hdr = open(os.path.join(ROOT, "include", "bvcodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(bvc_[a-z_0-9]+)\s*\(", hdr))
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.SIGNATURES and hasattr(lib, name), name
    assert lib.bvc_abi_version() == 3
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)
    r = ctypes.c_void_p()

    def create(rates, n=None, fixed=FS, direction=0, max_in=441, fmt_in=0, fmt_out=0):
        n = len(rates) if n is None else n
        return lib.bvc_resampler_create_multi(2, n, i32s(*rates), fixed, direction, i32s(*([max_in] * max(1, len(rates)))), fmt_in, fmt_out,
                                              ctypes.byref(r))

    nine = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
    refused = dict(no_rates=create((8000,), n=0), nine=create(nine), zero=create((16000, 0)), negative=create((-8000,)),
                   twice=create((8000, 16000, 8000)), fixed=create((8000,), fixed=0), fmt_in=create((8000,), fmt_in=2),
                   fmt_out=create((8000,), fmt_out=2), fmt_bits=create((8000,), fmt_out=32), direction=create((8000,), direction=2),
                   lds=create((8000, 48000), max_in=16384 - GEOMETRY[(48000, FS)][3] + 1))
    assert all(rc == -1 for rc in refused.values()) and not r.value, refused             # BVC_EINVAL before any device
    assert b"48000" in lib.bvc_last_error()                                               # (the LDS bound names the rate)


class _FakeSession:
    """What _MixedClientRate.finish uses of its session."""

    def slot_state(self, slot):
        return "running"


class _FakeResampler:
    def __init__(self):
        self.ended = []

    def end(self, slot, n_valid):
        self.ended.append((slot, n_valid))


@pytest.mark.parametrize("n_last", [0, 1, 123, "hop - 1", "hop"])
def test_slot_finish_plans(conf_var, n_last):
    """A mixed-rate adapter with a slot at each of the seven rates, three pushes in: finish(slot, n_last) counts the slot's own client
    samples - it ends the row's resampler with them and keeps (internal n_last, spills) of client_finish_plan at the slot's rate, what a
    single-rate session at that rate keeps.  Both cases occur: a tail that fits its push and one that spills."""
    from bvcodec.client_rate import _MixedClientRate
    from bvcodec.streaming import client_finish_plan
    a = object.__new__(_MixedClientRate)
    a.sc, a.conf, a.rates, a.B, a.rs_in = _FakeSession(), conf_var, RATES7, len(RATES7), _FakeResampler()
    a.hops = [441 * r // FS for r in RATES7]
    a.rate_of = list(range(len(RATES7)))
    a.n_push, a.open_push, a.ending, a.carry = 5, [2] * a.B, {}, {}
    spills = set()
    for slot, rate in enumerate(RATES7):
        hop = a.slot_hop(slot)
        assert a.slot_rate(slot) == rate and hop == 441 * rate // FS
        n = {"hop - 1": hop - 1, "hop": hop}.get(n_last, n_last)
        len_s, push, n22 = client_finish_plan(3 * hop + n, hop, rate, FS)
        a.finish(slot, n)
        assert a.rs_in.ended[-1] == (slot, n) and a.ending[slot] == (n22, push > 3), (rate, n)
        spills.add(push > 3)
        with pytest.raises(ValueError):                               # (a slot finishes once)
            a.finish(slot, n)
        with pytest.raises(ValueError):
            a.finish(slot + a.B, 0)
    if n_last in ("hop - 1", "hop"):
        assert True in spills                                         # the lag behind a (nearly) whole last hop spills at every rate
    if n_last in (1, 123):
        assert False in spills
    a.ending.clear()
    with pytest.raises(ValueError, match="outside 0..160"):           # the bound is the slot's own hop: 161 samples at 8 kHz
        a.finish(0, 161)
    a.finish(5, 161)
