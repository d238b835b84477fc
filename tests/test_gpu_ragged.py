"""Mixed-length batches (bvc_encode_ragged / bvc_decode_ragged and the facade's ``lengths`` keywords): row b of a batch of
utterances with their own lengths and bitrates equals, bit for bit, the equal-length call on that utterance alone.
Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HOP = 256
L_ROW = HOP * 40 + 13
# the shortest legal length (T_b = 2), lengths on and off the hop grid, one equal to the row
LENGTHS = [513, 600, 767, 768, 1000, 1500, 2048, 2049, 2500, 3000, 3333, 4096, 4100, 5000, 5555, 6000, 6500,
           7000, 7777, 8192, 8500, 9000, 10000, L_ROW]


def _model(var_bit=True):
    from gpu_common import make_model
    return make_model(var_bit, 1024)[0]


def _batch(lengths, L, seed, kind="speech"):
    from bvcodec import synth
    x = synth.synthetic_speech(len(lengths), L, seed=seed, kind=kind)
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
    return x.to(DEV)


def _frames(n):
    return n // HOP


def _check_rows_encode(model, x, lengths, bitrates, codes):
    assert codes.shape == (x.shape[0], _frames(x.shape[1]), model.conf["z_dim"])
    for b, n in enumerate(lengths):
        one = model.encode(x[b:b + 1, :n].contiguous(), bitrates[b])
        T_b = _frames(n)
        assert one.shape[1] == T_b
        assert torch.equal(codes[b:b + 1, :T_b], one), (b, n, bitrates[b])
        assert bool((codes[b, T_b:] == 0.5).all()), (b, n)


@pytest.mark.parametrize("var_bit", [True, False], ids=["var_bit", "64bit"])
@pytest.mark.parametrize("schedule", ["persistent", "layers"])
def test_ragged_encode_equals_single_calls(var_bit, schedule):
    model = _model(var_bit)
    x = _batch(LENGTHS, L_ROW, seed=11)
    try:
        model.set_recurrence(schedule)
        codes = model.encode(x, 3000, lengths=LENGTHS)
        _check_rows_encode(model, x, LENGTHS, [3000] * len(LENGTHS), codes)
    finally:
        model.set_recurrence("auto")


def test_ragged_encode_per_row_bitrate():
    model = _model(True)
    rates = [700, 1500, 3000, 6000, 12000]
    lengths = LENGTHS[:15]
    br = [rates[b % len(rates)] for b in range(len(lengths))]
    x = _batch(lengths, max(lengths), seed=12)
    codes = model.encode(x, br, lengths=lengths)
    _check_rows_encode(model, x, lengths, br, codes)
    # a per-row bitrate without lengths: every row is the whole row
    full = model.encode(x, torch.tensor(br))
    for b in range(len(lengths)):
        assert torch.equal(full[b:b + 1], model.encode(x[b:b + 1], br[b]))


def test_ragged_decode_and_forward_equal_single_calls():
    model = _model(True)
    x = _batch(LENGTHS, L_ROW, seed=13)
    codes = model.encode(x, 3000, lengths=LENGTHS)
    wav = model.decode(codes, LENGTHS)
    fwd = model.forward(x, 3000, lengths=LENGTHS)
    assert wav.shape == (len(LENGTHS), max(LENGTHS)) and torch.isfinite(wav).all()
    assert torch.equal(wav, fwd)
    for b, n in enumerate(LENGTHS):
        T_b = _frames(n)
        one = model.decode(codes[b:b + 1, :T_b].contiguous(), n)
        assert one.shape[1] == n
        assert torch.equal(wav[b:b + 1, :n], one), (b, n)
        assert bool((wav[b, n:] == 0).all()), (b, n)
        assert torch.equal(fwd[b:b + 1, :n], model.forward(x[b:b + 1, :n].contiguous(), 3000)), (b, n)
    # explicit frame counts and lengths that cut into / run past a row's generator output
    fr = [_frames(n) for n in LENGTHS]
    want = [n - 100 if b % 2 else 10 ** 6 for b, n in enumerate(LENGTHS)]
    w2 = model.decode(codes, want, frames=fr)
    for b in range(len(LENGTHS)):
        one = model.decode(codes[b:b + 1, :fr[b]].contiguous(), want[b])
        n_b = one.shape[1]
        assert torch.equal(w2[b:b + 1, :n_b], one) and bool((w2[b, n_b:] == 0).all()), b


@pytest.mark.parametrize("poison", [float("nan"), 1e30, -1e30])
def test_ragged_padding_is_never_read(poison):
    model = _model(True)
    x = _batch(LENGTHS, L_ROW, seed=14)
    codes = model.encode(x, 3000, lengths=LENGTHS)
    xp = x.clone()
    cp = codes.clone()
    for b, n in enumerate(LENGTHS):
        xp[b, n:] = poison
        cp[b, _frames(n):] = poison
    assert torch.equal(model.encode(xp, 3000, lengths=LENGTHS), codes)
    assert torch.equal(model.decode(cp, LENGTHS), model.decode(codes, LENGTHS))


@pytest.mark.parametrize("var_bit", [True, False], ids=["var_bit", "64bit"])
def test_ragged_equal_lengths_match_the_equal_length_entry_points(var_bit):
    model = _model(var_bit)
    B, L = 6, HOP * 30 + 77
    x = _batch([L] * B, L, seed=15, kind="noise")
    codes = model.encode(x, 3000)
    assert torch.equal(model.encode(x, 3000, lengths=[L] * B), codes)
    assert torch.equal(model.encode(x, [3000] * B), codes)
    assert torch.equal(model.decode(codes, [L] * B), model.decode(codes, L))
    T = codes.shape[1]
    assert torch.equal(model.decode(codes, [10 ** 9] * B), model.decode(codes, 10 ** 9))
    assert torch.equal(model.decode(codes, L, frames=[T] * B), model.decode(codes, L))


def test_ragged_large_batch():
    """B = 256: the interleaved-chain recurrence kernel."""
    model = _model(True)
    rng = np.random.default_rng(16)
    lengths = rng.integers(513, HOP * 12, size=256).tolist()
    lengths[7] = 513
    L = max(lengths)
    x = _batch(lengths, L, seed=16, kind="noise")
    codes = model.encode(x, 3000, lengths=lengths)
    wav = model.decode(codes, lengths)
    rows = sorted({0, 7, 100, 255} | set(rng.choice(256, 8, replace=False).tolist()))
    for b in rows:
        n = lengths[b]
        one = model.encode(x[b:b + 1, :n].contiguous(), 3000)
        assert torch.equal(codes[b:b + 1, :one.shape[1]], one), b
        assert torch.equal(wav[b:b + 1, :n], model.decode(one, n)), b
        assert bool((wav[b, n:] == 0).all()), b


def test_encode_many_decode_many():
    from bvcodec import synth
    model = _model(True)
    rng = np.random.default_rng(17)
    lens = rng.integers(513, HOP * 16, size=70).tolist()
    waves = [synth.synthetic_speech(1, n, seed=100 + i, kind="speech")[0] for i, n in enumerate(lens)]
    rates = [(700, 3000, 12000)[i % 3] for i in range(70)]
    codes = model.encode_many(waves, rates, max_batch=32)
    assert len(codes) == 70
    for i, w in enumerate(waves):
        assert codes[i].device == w.device
        assert torch.equal(codes[i], model.encode(w[None].to(DEV), rates[i])[0].cpu()), i
    wavs = model.decode_many(codes, lens, max_batch=32)
    for i, c in enumerate(codes):
        assert torch.equal(wavs[i], model.decode(c[None].to(DEV), lens[i])[0].cpu()), i
    one_rate = model.encode_many([w.to(DEV) for w in waves[:5]], 3000, max_batch=2)
    for i in range(5):
        assert torch.equal(one_rate[i], model.encode(waves[i][None].to(DEV), 3000)[0]), i


def test_ragged_against_the_oracle():
    """Per utterance against the CPU oracle, with smoke()'s rules: code bits equal except at ties, waveform RMS < 1e-4."""
    from gpu_common import make_model
    from oracle import codec as ocodec
    model, conf, vr, ge = make_model(True, 1024)
    oc = ocodec.OracleCodec(conf, vr, ge)
    lengths = [HOP * 3 + 1 + 512, HOP * 12 + 7, HOP * 18 + 100]
    x = _batch(lengths, max(lengths), seed=18)
    codes = model.encode(x, 3000, lengths=lengths)
    wav = model.decode(codes, lengths)
    for b, n in enumerate(lengths):
        xb = x[b:b + 1, :n].cpu()
        T_b = _frames(n)
        r = oc.encode(xb, 3000, full=True)
        got = codes[b:b + 1, :T_b].cpu()
        mism = got != r["codes"]
        margin = (r["prob"] - 0.5).abs()
        assert not bool((mism & (margin > 1e-5)).any()), b
        ref = oc.decode(got, n)
        rms = float((wav[b:b + 1, :n].cpu() - ref).pow(2).mean().sqrt())
        assert rms < 1e-4, (b, rms)


def test_ragged_decode_graph_capture():
    """bvc_decode_ragged captured into a torch.cuda.graph and replayed equals the eager call of the same schedule."""
    from bvcodec import _abi
    from bvcodec.model import SCALING
    model = _model(True)
    lengths = [700, 3000, 5000, 2049]
    x = _batch(lengths, max(lengths), seed=19)
    codes = model.encode(x, 3000, lengths=lengths)
    B, T, _ = codes.shape
    eng = model.engine(codes)
    frames = torch.tensor([_frames(n) for n in lengths], dtype=torch.int64, device=DEV)
    lens = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    n_max = max(lengths)
    try:
        model.set_recurrence("layers")
        ref = model.decode(codes, lengths)
    finally:
        model.set_recurrence("auto")
    wav = torch.empty(B, n_max, device=DEV)

    def call():
        ws, nws = eng.workspace(B, T)
        _abi.check(eng.lib.bvc_decode_ragged(eng.handle, _abi.ptr(codes), ctypes.c_void_p(frames.data_ptr()), B, T,
                                             ctypes.c_void_p(lens.data_ptr()), n_max, float(SCALING), _abi.ptr(wav), ws, nws,
                                             eng.stream()))

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        call()                                                 # warm call: the workspace of this stream exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        call()
    wav.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(wav, ref)
    model.check_status()


def test_ragged_validation_errors():
    model = _model(True)
    x = _batch([2000, 3000], 3000, seed=20)
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        model.encode(x, 3000, lengths=[512, 3000])
    with pytest.raises(RuntimeError, match="must not exceed"):
        model.encode(x, 3000, lengths=[2000, 3001])
    with pytest.raises(RuntimeError, match="entries for a batch"):
        model.encode(x, 3000, lengths=[2000])
    codes = model.encode(x, 3000, lengths=[2000, 3000])
    with pytest.raises(RuntimeError, match="frames must lie"):
        model.decode(codes, [2000, 3000], frames=[7, codes.shape[1] + 1])
    # a row without frames decodes to silence
    w = model.decode(codes, [2000, 3000], frames=[0, codes.shape[1]])
    assert bool((w[0] == 0).all()) and w.shape[1] == 3000
