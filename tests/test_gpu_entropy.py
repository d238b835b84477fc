"""The entropy-coded wire format on the MI355X: the coder alone against the numpy coder (bytes and sizes equal), through the model
(round trip, the bytes of the numpy coder fed with the GPU's own prior, the receive program's mel and state equal to the concealing
call's, decode_entropy equal to decode), one function whatever the batch, the chunking, the sender's schedule and the replay, and
the refusals.  Needs the MI355X."""
import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import entropy_oracle as eo
from gpu_common import DEV, make_model

pytestmark = pytest.mark.gpu
B, T = 5, 35


def lib():
    from bvcodec import _abi
    return _abi.load()


def check(rc):
    from bvcodec import _abi
    _abi.check(rc)


def gpu_encode(codes, prob, bits, segment, stride=None, canary=0):
    """bvc_entropy_encode on numpy inputs -> (data (B, nseg, stride), sizes, the canary bytes behind the buffer)."""
    from bvcodec._abi import ptr
    Bc, Tc, Z = codes.shape
    S, segs = eo.segments(Tc, segment)
    stride = eo.safe_stride(Z, S) if stride is None else stride
    n = Bc * len(segs) * stride
    buf = torch.full((n + canary,), 0xC3, dtype=torch.uint8, device=DEV)
    sizes = torch.full((Bc, len(segs)), -7, dtype=torch.int32, device=DEV)
    c, p, b = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (codes, prob, bits))
    check(lib().bvc_entropy_encode(ptr(c), ptr(p), ptr(b), 0.0, Bc, Tc, Z, S, ptr(buf, torch.uint8), stride, ptr(sizes, torch.int32), None))
    torch.cuda.synchronize()
    return buf[:n].reshape(Bc, len(segs), stride).cpu().numpy(), sizes.cpu().numpy(), buf[n:].cpu().numpy()


def gpu_decode(data, sizes, prob, bits, segment):
    from bvcodec._abi import ptr
    Bc, Tc, Z = prob.shape
    S, _ = eo.segments(Tc, segment)
    d, s = torch.from_numpy(np.ascontiguousarray(data)).to(DEV), torch.from_numpy(np.ascontiguousarray(sizes)).to(DEV)
    p, b = torch.from_numpy(prob).to(DEV), torch.from_numpy(bits).to(DEV)
    out = torch.full((Bc, Tc, Z), float("nan"), device=DEV)
    check(lib().bvc_entropy_decode(ptr(d, torch.uint8), data.shape[2], ptr(s, torch.int32), ptr(p), ptr(b), 0.0, Bc, Tc, Z, S, ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: the coder alone
@pytest.mark.parametrize("z_dim", [16, 64, 128])
def test_coder_alone_equals_the_numpy_coder(z_dim):
    for kind in eo.PROB_CLASSES:
        p = eo.prob_case(kind, B, T, z_dim, seed=3)
        codes = eo.draw_codes(p, 3, wrong=0.02 if kind == "extreme" else 0.0)
        bits = eo.bits_case(B, T, z_dim)
        for segment in (1, 8, 35):
            ref = eo.pack(codes, p, bits, segment)
            data, sizes, _ = gpu_encode(codes, p, bits, segment)
            assert np.array_equal(sizes, ref["sizes"]), (kind, segment)
            assert np.array_equal(data, ref["data"]), (kind, segment)                 # the bytes, and zeros from size to stride
            assert np.array_equal(gpu_decode(data, sizes, p, bits, segment), eo.masked(codes, bits)), (kind, segment)
            dirty = data.copy()
            for b in range(B):
                for s in range(sizes.shape[1]):
                    dirty[b, s, sizes[b, s]:] = 0xA5                                  # nothing at or behind `size` is read
            assert np.array_equal(gpu_decode(dirty, sizes, p, bits, segment), eo.masked(codes, bits)), (kind, segment)


def test_carry_case():
    codes, p, bits = eo.carry_case()
    ref = eo.pack(codes, p, bits)
    assert bool(ref["carried"].all())
    data, sizes, _ = gpu_encode(codes, p, bits, None)
    assert np.array_equal(sizes, ref["sizes"]) and np.array_equal(data, ref["data"])
    assert np.array_equal(gpu_decode(data, sizes, p, bits, None), codes)


def test_a_stride_that_is_too_small_and_the_canary():
    p = eo.prob_case("flat", 3, 16, 64, seed=2)
    codes = eo.draw_codes(p, 2)
    bits = np.full((3, 16), 64.0, dtype=np.float32)
    full = eo.pack(codes, p, bits, 8)
    small = int(full["sizes"].max()) - 1
    ref = eo.pack(codes, p, bits, 8, stride=small)
    data, sizes, canary = gpu_encode(codes, p, bits, 8, stride=small, canary=256)
    assert np.array_equal(sizes, ref["sizes"]) and (sizes == -1).any() and (sizes >= 0).any()
    assert (canary == 0xC3).all()
    fits = sizes >= 0
    assert np.array_equal(data[fits], ref["data"][fits])
    # the decoder takes a size outside [0, stride] as no bytes: it reads nothing, whatever it then decodes
    bad = sizes.copy()
    bad[0, 0], bad[1, 1] = -1, small + 1000
    out = gpu_decode(data, bad, p, bits, 8)
    zero = bad.copy()
    zero[0, 0], zero[1, 1] = 0, 0
    assert np.array_equal(out, eo.unpack(data, zero, p, bits, 8))


# ------------------------------------------------------------------------------------------------ 2: through the model
def matched_model(h_dim):
    """pin_logits with prior.4.bias = enc.4.bias (test_entropy_cpu.matched): made by editing the pinned model's checkpoint."""
    import os
    import tempfile
    from bvcodec import BVRNNCodecModel, config, synth
    key = ("matched", h_dim)
    if key not in _MODELS:
        conf = bd.conf_of(h_dim)
        d = tempfile.mkdtemp(prefix="bvc_entropy_")
        cfg = os.path.join(d, "cfg.toml")
        with open(config.DEFAULT_CONFIG) as f:
            txt = f.read()
        with open(cfg, "w") as f:
            f.write(txt.replace("h_dim = 1024", f"h_dim = {h_dim}"))
        p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
        vr = bd.pin_logits(synth.bvrnn_state_dict(conf, 1234))
        vr["prior.4.bias"] = vr["enc.4.bias"].clone()
        torch.save({"vrnn": vr}, p1)
        _MODELS[key] = BVRNNCodecModel(cfg, p1, p2).to(DEV)
    return _MODELS[key]


_MODELS = {}
MODELS = {"default": lambda h, var: make_model(var, h)[0],
          "saturated": lambda h, var: make_model(var, h, gains=bd.GAINS["saturated"])[0],
          "pinned": lambda h, var: make_model(var, h, pinned="logits")[0],
          "matched": lambda h, var: matched_model(h)}


def through_the_model(model, Bm, Tm, var_bit, segment, seed):
    """Codes of the model's own encoder on noise-like mel, packed and unpacked; returns what the assertions need."""
    H = model.conf["h_dim"]
    y, _ = bd.inputs(Bm, Tm, seed=seed)
    bits = bd.pinned_bits(Bm, Tm).to(DEV) if var_bit else None
    h0 = torch.zeros(1, Bm, H, device=DEV)
    codes, _ = model.bvrnn.encode(y.to(DEV), bits if var_bit else torch.full((Bm, Tm), 64.0, device=DEV), h0)
    present = torch.ones(Bm, Tm, device=DEV)
    mel_c, hT_c, _, prior_c = model.bvrnn.decode(codes, h0, present=present, bits=bits, return_codes=True)
    data, sizes, hT_s, prior_s = model.bvrnn.entropy_pack(codes, bits, h0, segment=segment, return_prior=True)
    got, mel_r, hT_r, prior_r = model.bvrnn.entropy_unpack(data, sizes, Tm, bits, h0, segment=segment, return_prior=True)
    torch.cuda.synchronize()
    return dict(codes=codes, bits=bits, data=data, sizes=sizes, got=got, mel_c=mel_c, hT_c=hT_c, prior_c=prior_c, hT_s=hT_s, prior_s=prior_s,
                mel_r=mel_r, hT_r=hT_r, prior_r=prior_r)


@pytest.mark.parametrize("h_dim,Bm,Tm", [(128, 5, 24), (64, 5, 24), (1024, 20, 12)])
@pytest.mark.parametrize("which,var_bit", [("default", True), ("default", False), ("saturated", True), ("saturated", False), ("pinned", True),
                                           ("matched", True)])
def test_through_the_model(h_dim, Bm, Tm, which, var_bit):
    model = MODELS[which](h_dim, var_bit)
    r = through_the_model(model, Bm, Tm, var_bit, 8, seed=5)
    assert torch.equal(r["got"], r["codes"])                                           # the 0.5 positions included
    assert torch.equal(r["prior_s"], r["prior_c"]) and torch.equal(r["prior_r"], r["prior_c"])
    assert torch.equal(r["mel_r"], r["mel_c"]) and torch.equal(r["hT_r"], r["hT_c"]) and torch.equal(r["hT_s"], r["hT_c"])
    np_bits = r["bits"].cpu().numpy() if var_bit else np.full((Bm, Tm), 64.0, dtype=np.float32)
    ref = eo.pack(r["codes"].cpu().numpy(), r["prior_c"].cpu().numpy(), np_bits, 8)
    assert np.array_equal(r["sizes"].cpu().numpy(), ref["sizes"])
    assert np.array_equal(r["data"].cpu().numpy(), ref["data"])                        # integers behind p: no tie rule
    n = int(ref["n"].sum())
    print(f"{which} h {h_dim} var_bit {var_bit}: {n} coded bits, ideal {ref['ideal'].sum() / max(n, 1):.4f}, stored "
          f"{8.0 * ref['sizes'].sum() / max(n, 1):.4f} bit per bit")
    if which == "matched":
        assert eo.overhead_ok(ref["sizes"], ref["ideal"], ref["n"]).all()
        assert ref["ideal"].sum() < 0.5 * n
    model.check_status()


@pytest.mark.parametrize("which,var_bit", [("default", True), ("default", False), ("matched", True)])
def test_facade_round_trip_and_decode_entropy(which, var_bit):
    from bvcodec import synth
    model = MODELS[which](128, var_bit)
    x = synth.synthetic_speech(5, 256 * 24, seed=3, kind="noise").to(DEV)
    codes = model.encode(x, 3000)
    Tm = codes.shape[1]
    for segment in (None, 8):
        data, sizes = model.pack_entropy(codes, bitrate=3000, segment=segment)
        assert data.shape[2] == int(sizes.max()) and data.dtype == torch.uint8 and sizes.dtype == torch.int32
        assert torch.equal(model.unpack_entropy(data, sizes, Tm, bitrate=3000, segment=segment), codes)
        d2, s2 = model.encode_entropy(x, 3000, segment=segment)
        assert torch.equal(d2, data) and torch.equal(s2, sizes)
        wav, back = model.decode_entropy(data, sizes, Tm, x.shape[1], bitrate=3000, segment=segment, return_codes=True)
        ref = model.decode(codes, x.shape[1], lost=torch.zeros(5, Tm, dtype=torch.bool, device=DEV), bitrate=3000)
        assert torch.equal(back, codes) and torch.equal(wav, ref)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 3: one function
def test_rows_chunks_schedules_and_replay():
    model = MODELS["default"](128, True)
    Bm, Tm, H = 5, 24, 128
    y, _ = bd.inputs(Bm, Tm, seed=9)
    bits = bd.pinned_bits(Bm, Tm).to(DEV)
    h0 = torch.from_numpy((0.2 * np.random.default_rng(4).standard_normal((1, Bm, H))).astype(np.float32)).to(DEV)
    codes, _ = model.bvrnn.encode(y.to(DEV), bits, h0)
    data, sizes, hT = model.bvrnn.entropy_pack(codes, bits, h0, segment=8)
    # the sender on every schedule
    for schedule in ("persistent", "layers", "auto"):
        try:
            model.set_recurrence(schedule)
            d, s, h = model.bvrnn.entropy_pack(codes, bits, h0, segment=8)
        finally:
            model.set_recurrence("auto")
        assert torch.equal(d, data) and torch.equal(s, sizes) and torch.equal(h, hT), schedule
    # a warm replayed call equals the first one, and the eager launches (BVC_NO_GRAPH) equal both
    first = model.bvrnn.entropy_unpack(data, sizes, Tm, bits, h0, segment=8)
    again = model.bvrnn.entropy_unpack(data, sizes, Tm, bits, h0, segment=8)
    eager = make_model(True, 128, env={"BVC_NO_GRAPH": "1"})[0].bvrnn.entropy_unpack(data, sizes, Tm, bits, h0, segment=8)
    for a, b, c in zip(first, again, eager):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(first[0], codes) and torch.equal(first[2], hT)
    # a row alone equals the row inside the batch
    for b in (0, 3):
        d1, s1, h1 = model.bvrnn.entropy_pack(codes[b:b + 1], bits[b:b + 1], h0[:, b:b + 1], segment=8)
        assert torch.equal(d1[0], data[b]) and torch.equal(s1[0], sizes[b]) and torch.equal(h1[0, 0], hT[0, b])
        c1, m1, g1 = model.bvrnn.entropy_unpack(data[b:b + 1], sizes[b:b + 1], Tm, bits[b:b + 1], h0[:, b:b + 1], segment=8)
        assert torch.equal(c1[0], first[0][b]) and torch.equal(m1[0], first[1][b]) and torch.equal(g1[0, 0], first[2][0, b])
    # [0, 16) + [16, 24) with the state carried equals the one call
    da, sa, ha = model.bvrnn.entropy_pack(codes[:, :16], bits[:, :16], h0, segment=8)
    db, sb, hb = model.bvrnn.entropy_pack(codes[:, 16:], bits[:, 16:], ha, segment=8)
    assert torch.equal(torch.cat([sa, sb], 1), sizes) and torch.equal(hb, hT)
    assert torch.equal(torch.cat([da, db], 1), data)
    ca, ma, ga = model.bvrnn.entropy_unpack(da, sa, 16, bits[:, :16], h0, segment=8)
    cb, mb, gb = model.bvrnn.entropy_unpack(db, sb, 8, bits[:, 16:], ga, segment=8)
    assert torch.equal(torch.cat([ca, cb], 1), codes) and torch.equal(torch.cat([ma, mb], 1), first[1]) and torch.equal(gb, hT)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 4: refusals
def test_refusals():
    from bvcodec import _abi
    from bvcodec._abi import ptr
    model = MODELS["default"](128, True)
    eng = model.engine()
    L = lib()
    codes = torch.full((2, 6, 64), 0.5, device=DEV)
    bits = torch.zeros(2, 6, device=DEV)
    data = torch.zeros(2, 1, 800, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(2, 1, dtype=torch.int32, device=DEV)
    mel = torch.zeros(2, 6, 80, device=DEV)
    ws, nws = eng.workspace(2, 6, "entropy")

    def pack(segment, stride=800, handle=eng.handle, d_bits=bits):
        return L.bvc_bvrnn_entropy_pack(handle, ptr(codes), ptr(d_bits), None, 2, 6, segment, ptr(data, torch.uint8), stride, ptr(sizes, torch.int32),
                                        None, None, ws, nws, None)

    def unpack(segment, stride=800):
        return L.bvc_bvrnn_entropy_unpack(eng.handle, ptr(data, torch.uint8), stride, ptr(sizes, torch.int32), ptr(bits), None, 2, 6, segment, None,
                                          ptr(mel), None, None, ws, nws, None)

    assert pack(0) == -1 and b"segment" in L.bvc_last_error()
    assert unpack(0) == -1 and unpack(-3) == -1
    assert pack(6, stride=-1) == -1 and b"stride" in L.bvc_last_error()
    assert pack(6, d_bits=None) == -1                                                  # a variable-rate model needs the bits
    assert L.bvc_bvrnn_entropy_unpack(eng.handle, ptr(data, torch.uint8), 800, None, ptr(bits), None, 2, 6, 6, None, ptr(mel), None, None, ws, nws,
                                      None) == -1
    assert L.bvc_decode_entropy(eng.handle, ptr(data, torch.uint8), 800, ptr(sizes, torch.int32), 35.0, 2, 6, 0, 1000, 1.0, ptr(mel), None, ws, nws,
                                None) == -1
    assert pack(6, handle=None) == -1
    assert pack(6) == 0 and unpack(6) == 0                                             # and the same arguments go through
    torch.cuda.synchronize()
    # sizes in pinned host memory are checked before anything is launched
    host = torch.tensor([[3], [801]], dtype=torch.int32).pin_memory()
    assert L.bvc_bvrnn_entropy_unpack(eng.handle, ptr(data, torch.uint8), 800, ptr(host, torch.int32), ptr(bits), None, 2, 6, 6, None, ptr(mel),
                                      None, None, ws, nws, None) == -1 and b"sizes[1]" in L.bvc_last_error()
    # z_dim > 3 h_dim: the concealing program's own limit
    small = make_model(True, 16, z_dim=64)[0]
    with pytest.raises(_abi.BvcError, match="z_dim > 3 h_dim"):
        small.bvrnn.entropy_pack(codes, bits, torch.zeros(1, 2, 16, device=DEV))
    with pytest.raises(_abi.BvcError, match="z_dim > 3 h_dim"):
        small.bvrnn.entropy_unpack(data, sizes, 6, bits, torch.zeros(1, 2, 16, device=DEV))


def test_missing_prior():
    """BVC_EMISSING on a model created without the prior.* tensors."""
    from bvcodec import _abi
    from bvcodec.engine import _Engine
    model = MODELS["default"](128, True)
    tensors = {k: v for k, v in model._tensors.items() if not k.startswith("prior.")}
    eng = _Engine(model.conf, tensors, torch.device(DEV))
    from bvcodec._abi import ptr
    codes = torch.full((2, 6, 64), 0.5, device=DEV)
    bits = torch.zeros(2, 6, device=DEV)
    data = torch.zeros(2, 1, 800, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(2, 1, dtype=torch.int32, device=DEV)
    mel = torch.zeros(2, 6, 80, device=DEV)
    ws, nws = eng.workspace(2, 6, "entropy")
    L = lib()
    assert L.bvc_bvrnn_entropy_pack(eng.handle, ptr(codes), ptr(bits), None, 2, 6, 6, ptr(data, torch.uint8), 800, ptr(sizes, torch.int32), None, None,
                                    ws, nws, None) == -4
    assert L.bvc_bvrnn_entropy_unpack(eng.handle, ptr(data, torch.uint8), 800, ptr(sizes, torch.int32), ptr(bits), None, 2, 6, 6, None, ptr(mel), None,
                                      None, ws, nws, None) == -4
    assert L.bvc_decode_entropy(eng.handle, ptr(data, torch.uint8), 800, ptr(sizes, torch.int32), 35.0, 2, 6, 6, 1000, 1.0, ptr(mel), None, ws, nws,
                                None) == -4 and b"prior" in L.bvc_last_error()
