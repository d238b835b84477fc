"""The facade's argument checks, the devices its outputs land on and its per-stream scratch, on the h_dim 64 models with a batch of 2.

The texts of the refusals are spelled out here, not taken from the package.  No other GPU test asserts one of these cases with the same
call: ``test_gpu_ragged.test_ragged_validation_errors`` has the reflect padding error of a mixed-length batch at other lengths, the
closed-loop refusals are otherwise checked without a device (``test_vbr_cpu``, ``test_vbr_stream_cpu``)."""
import pytest
import torch

from gpu_common import DEV, make_model

pytestmark = pytest.mark.gpu
LENGTHS = (0, 256, 257, 512, 513, 767, 768, 1023, 1024, 1025, 4099)


def _var():
    return make_model(True, 64)[0]


def _wave(L, seed=3):
    from bvcodec import synth
    return synth.synthetic_speech(2, L, seed=seed, kind="speech")


def test_python_frame_count_is_the_librarys():
    """``config.num_frames`` against ``bvc_num_frames`` at every length: the same count wherever there is one.  Where the reflect
    padding does not fit (L <= 512) the library answers BVC_EINVAL (-1, "< 0" in include/bvcodec.h) and the Python statement 0, as the
    arithmetic it replaces in ``encode_vbr`` did; every caller asks ``<= 0``.  Both values are held exactly."""
    from bvcodec.config import num_frames
    for model in (_var(), make_model(False, 64)[0]):
        eng = model.engine()
        python, library = [num_frames(model.conf, L) for L in LENGTHS], [eng.num_frames(L) for L in LENGTHS]
        assert python == [0, 0, 0, 0, 2, 2, 3, 3, 4, 4, 16]
        assert library == [n if n else -1 for n in python]


WAVE_CALLS = {
    "mel_spectrogram": lambda m, x: m.mel_spectrogram(x),
    "encode": lambda m, x: m.encode(x, 3000),
    "encode_lengths": lambda m, x: m.encode(x, 3000, lengths=[x.shape[-1]] * 2),
    "encode_vbr": lambda m, x: m.encode_vbr(x, 0.35)[0],
    "forward_fused": lambda m, x: m.forward_fused(x, 3000, return_codes=True)[0],
}


@pytest.mark.parametrize("call", sorted(WAVE_CALLS))
def test_shortest_waveform(call):
    """513 samples make 2 frames; at 512 the right reflect padding is as long as the signal."""
    model, fn = _var(), WAVE_CALLS[call]
    assert fn(model, _wave(513).to(DEV)).shape[:2] == (2, 2)
    with pytest.raises(RuntimeError, match="Padding size should be less.*length 512 "):
        fn(model, _wave(512).to(DEV))
    with pytest.raises(RuntimeError, match=r"expected a \(batch, length\) waveform"):
        fn(model, _wave(513)[0].to(DEV))


def test_short_utterance_of_a_mixed_length_batch_is_named():
    with pytest.raises(RuntimeError, match="Padding size should be less.*length 512 "):
        _var().encode(_wave(513).to(DEV), 3000, lengths=[513, 512])


def test_mixed_length_encode_looks_at_the_bitrate_last():
    """With ``lengths`` a bitrate per row is looked at behind the waveform, the lengths and the reflect padding: an input with one
    of those faults and a bitrate of the wrong entry count raises the former."""
    model, x = _var(), _wave(768).to(DEV)
    with pytest.raises(RuntimeError, match="lengths has 3 entries for a batch of 2"):
        model.encode(x, [3000] * 3, lengths=[1, 2, 3])
    with pytest.raises(RuntimeError, match=r"expected a \(batch, length\) waveform"):
        model.encode(x[0], [3000, 3000], lengths=[768, 768])
    with pytest.raises(RuntimeError, match="lengths must not exceed the row length 768"):
        model.encode(x, [3000] * 3, lengths=[768, 769])
    with pytest.raises(RuntimeError, match="Padding size should be less.*length 512 "):
        model.encode(x, [3000] * 3, lengths=[768, 512])
    with pytest.raises(RuntimeError, match="bitrate has 3 entries for a batch of 2"):
        model.encode(x, [3000] * 3, lengths=[768, 600])
    with pytest.raises(RuntimeError, match="bitrate has 3 entries for a batch of 2"):
        model.encode(x, [3000] * 3)


@pytest.mark.parametrize("how", ["plain", "lost", "frames"])
def test_codes_of_the_wrong_width(how):
    model = _var()
    codes = torch.full((2, 3, model.conf["z_dim"] - 1), 0.5, device=DEV)
    kw = {"plain": {}, "lost": dict(lost=torch.zeros(2, 3, dtype=torch.bool), bitrate=3000), "frames": dict(frames=[3, 2])}[how]
    with pytest.raises(RuntimeError, match=f"codes must have {model.conf['z_dim']} values per frame, got {model.conf['z_dim'] - 1}"):
        model.decode(codes, 768, **kw)


def _codes(m):
    return torch.full((2, 3, m.conf["z_dim"]), 0.5, device=DEV)


def _h(m):
    return torch.zeros(1, 2, m.conf["h_dim"], device=DEV)


def _mel(m):
    return torch.zeros(2, 3, m.conf["num_mels"], device=DEV)


REFUSALS = {   # name: (variable-rate model?, call, the message)
    "return_codes without lost": (True, lambda m: m.decode(_codes(m), 768, return_codes=True),
                                  r"decode: return_codes belongs to concealment \(pass lost\)"),
    "bits without present": (True, lambda m: m.bvrnn.decode(_codes(m), _h(m), bits=torch.full((2, 3), 35.0)),
                             r"decode: bits / return_codes belong to concealment \(pass present\)"),
    "encode_vbr lengths": (True, lambda m: m.encode_vbr(_wave(768).to(DEV), 0.35, lengths=[768, 600]),
                           r"encode_vbr: mixed-length batches \(lengths=\) are not supported"),
    "tok without a cap": (True, lambda m: m.bvrnn.encode_vbr(_mel(m), (16, 32), 0.35, _h(m), tok=torch.zeros(2, dtype=torch.int32)),
                          "encode_vbr: tok without rate_q8 and burst_q8"),
    "rate_q8 without burst_q8": (True, lambda m: m.bvrnn.encode_vbr(_mel(m), (16, 32), 0.35, _h(m), rate_q8=100),
                                 "encode_vbr: a rate cap takes both rate_q8 and burst_q8"),
    "fixed-rate model": (False, lambda m: m.encode_vbr(_wave(768).to(DEV), 0.35),
                         r"encode_vbr: a fixed-rate model \(var_bit = false\) has no bit mask to choose"),
    "ladder descends": (True, lambda m: m.encode_vbr(_wave(768).to(DEV), 0.35, bitrates=(3000, 1500)),
                        r"encode_vbr: the rungs must lie in \[0, 64\] and ascend strictly, got \[35, 17\]"),
    "target of another batch": (True, lambda m: m.encode_vbr(_wave(768).to(DEV), torch.zeros(3)),
                                r"encode_vbr: target must be a scalar, \(2,\) or \(2, 3\), got \(3,\)"),
    "pack_vbr bits shape": (True, lambda m: m.pack_vbr(_codes(m), torch.zeros(2, 4, device=DEV)),
                            r"pack_vbr: codes \(B, T, z_dim\) with bits \(B, T\)"),
    "unpack_vbr float": (True, lambda m: m.unpack_vbr(torch.zeros(2, 3, 9, device=DEV)),
                         r"unpack_vbr: uint8 \(B, T, 9\) expected"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    var_bit, call, message = REFUSALS[name]
    with pytest.raises(ValueError, match=message):
        call(make_model(var_bit, 64)[0])


def _on(device, tensors):
    return [t.to(device) for t in tensors]


CPU_CALLS = {    # name: (inputs on the CPU, call)
    "encode": lambda m: ([_wave(768)], lambda x: m.encode(x, 3000)),
    "decode": lambda m: ([m.encode(_wave(768), 3000)], lambda c: m.decode(c, 768)),
    "bvrnn.encode return_prob": lambda m: ([m.mel_spectrogram(_wave(768)), torch.full((2, 3), 35.0), torch.zeros(1, 2, 64)],
                                           lambda y, b, h: m.bvrnn.encode(y, b, h, return_prob=True)),
    "bvrnn.decode present return_codes": lambda m: (
        [m.encode(_wave(768), 3000), torch.zeros(1, 2, 64), torch.tensor([[1, 0, 1], [1, 1, 0]]), torch.full((2, 3), 35.0)],
        lambda z, h, p, b: m.bvrnn.decode(z, h, present=p, bits=b, return_codes=True)),
    "encode_vbr": lambda m: ([_wave(768)], lambda x: m.encode_vbr(x, 0.35)),
}
OUTPUTS = {"encode": 1, "decode": 1, "bvrnn.encode return_prob": 3, "bvrnn.decode present return_codes": 4, "encode_vbr": 2}


@pytest.mark.parametrize("name", sorted(CPU_CALLS))
def test_cpu_tensors_in_cpu_tensors_out(name):
    """Every output lands on the caller's device, and is what the same call gives for the GPU copy of the input."""
    inputs, call = CPU_CALLS[name](_var())
    on_cpu, on_gpu = call(*inputs), call(*_on(DEV, inputs))
    on_cpu, on_gpu = (on_cpu, on_gpu) if isinstance(on_cpu, tuple) else ((on_cpu,), (on_gpu,))
    assert len(on_cpu) == len(on_gpu) == OUTPUTS[name]
    for c, g in zip(on_cpu, on_gpu):
        assert c.device.type == "cpu" and g.device == torch.device(DEV)
        assert torch.equal(c, g.cpu())


def test_two_streams_take_their_own_scratch():
    """Stream A at 3 frames, stream B at 6 (its buffer is another, and larger), A again: each call equals the default stream's."""
    model = _var()
    short, long_ = _wave(768).to(DEV), _wave(1536, seed=4).to(DEV)
    ref_short, ref_long = model.encode(short, 3000), model.encode(long_, 3000)
    a, b = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    a.wait_stream(torch.cuda.current_stream(DEV))
    b.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(a):
        first = model.encode(short, 3000)
    with torch.cuda.stream(b):
        second = model.encode(long_, 3000)
    with torch.cuda.stream(a):
        third = model.encode(short, 3000)
    torch.cuda.synchronize()
    assert torch.equal(first, ref_short) and torch.equal(second, ref_long) and torch.equal(third, ref_short)
