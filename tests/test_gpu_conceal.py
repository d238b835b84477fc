"""Lost frames concealed from the model's prior net (bvc_bvrnn_decode_conceal, bvc_decode_conceal, bvc_stream_codec_set_conceal):
against golden vectors stepped with the reference's modules, against the CPU oracle at the benchmarked size, across schedules,
chunkings and batches, and in receive sessions.  Needs the MI355X."""
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden

import conceal_oracle as co
from gpu_common import on_schedule
from gpu_sessions import DEV, RATES, send_packets, set_schedule

pytestmark = pytest.mark.gpu


def t(a):
    return torch.from_numpy(np.asarray(a))


def mk(var_bit=True, h_dim=1024):
    from gpu_common import make_model
    return make_model(var_bit, h_dim)


def random_codes(B, T, nbits, seed):
    rng = np.random.default_rng(seed)
    codes = torch.from_numpy(rng.integers(0, 2, size=(B, T, 64)).astype(np.float32))
    codes[:, :, nbits:] = 0.5
    return codes


def conceal(model, codes, present, bits, h0=None):
    """(mel, hT (B,H), codes_out, prior) through the facade (bvc_bvrnn_decode_conceal)."""
    B = codes.shape[0]
    h = torch.zeros(1, B, model.conf["h_dim"], device=DEV) if h0 is None else h0.reshape(1, B, -1).to(DEV)
    mel, hT, out, prior = model.bvrnn.decode(codes.to(DEV), h, present=present.to(DEV), bits=None if bits is None else bits.to(DEV),
                                             return_codes=True)
    return mel, hT[0], out, prior


# ------------------------------------------------------------------------------------------------ 1: goldens
@pytest.mark.parametrize("tag,h_dim,var_bit", [("h64_var", 64, True), ("h1024_fix", 1024, False)])
@pytest.mark.parametrize("schedule", ["persistent", "layers"])
def test_goldens(tag, h_dim, var_bit, schedule):
    """codes_out equals the fixture's (a differing generated bit only where the fixture's |p - 0.5| < 1e-5: with the searched seeds none
    is expected); prior within 2e-6; mel / h_T at test_gpu_parity.py's bars for the g3_* decode goldens (5e-5 / 5e-6)."""
    g = load_golden(f"g9_conceal_{tag}")
    model = mk(var_bit, h_dim)[0]
    mel, hT, out, prior = on_schedule(model, schedule, lambda: conceal(model, t(g["codes"]), t(g["present"]), t(g["bits"]) if var_bit else None))
    diff = out.cpu().numpy() != g["codes_out"]
    print(f"{tag} {schedule}: differing code values {int(diff.sum())}, max |prior err| {np.abs(prior.cpu().numpy() - g['prior']).max():.2e}, "
          f"max |mel err| {np.abs(mel.cpu().numpy() - g['mel']).max():.2e}, max |h_T err| {np.abs(hT.cpu().numpy() - g['h_last']).max():.2e}")
    assert (np.abs(g["prior"] - 0.5)[diff] < 1e-5).all()
    assert not diff.any()
    assert np.abs(prior.cpu().numpy() - g["prior"]).max() < 2e-6
    assert np.abs(mel.cpu().numpy() - g["mel"]).max() < 5e-5
    assert np.abs(hT.cpu().numpy() - g["h_last"]).max() < 5e-6
    model.check_status()


# ------------------------------------------------------------------------------------------------ 2: benchmark size
@pytest.mark.parametrize("var_bit", [True, False])
def test_benchmark_size_against_the_oracle(var_bit):
    """h 1024, 64 x 5 s, var_bit at 3 kbit/s and config_64bit; 5 % random loss, a 10-frame burst per row, one row all lost, one row
    none.  The oracle is restarted from the GPU's own filled codes (the states follow from them)."""
    from bvcodec import synth
    model, conf, vr, _ = mk(var_bit, 1024)
    torch.set_num_threads(16)
    B, L = 64, int(22050 * 5.0)
    x = synth.synthetic_speech(B, L, seed=11, kind="noise")
    codes = model.encode(x.to(DEV), 3000)
    T = codes.shape[1]
    nb = int(model.active_bits(3000))
    present = co.loss_pattern(B, T, 0.05, seed=21, burst=10, all_lost_row=5, clean_row=9)
    assert not present[5].any() and present[9].all()
    bits = torch.full((B, T), float(nb)) if var_bit else None
    dirty = codes.clone()
    dirty[~present.to(DEV)] = float("nan")
    mel, hT, out, prior = conceal(model, dirty, present, bits)
    torch.cuda.synchronize()
    out_c = out.cpu()
    assert torch.equal(out_c[present], codes.cpu()[present])                       # received positions pass through
    assert bool(torch.isfinite(out_c).all()) and bool(torch.isfinite(mel).all())
    ref = co.decode_with_prior(vr, out_c, torch.zeros(B, 1024))
    e_mel = float((mel.cpu() - ref["mel"]).abs().max()); e_h = float((hT.cpu() - ref["h_last"]).abs().max())
    e_p = float((prior.cpu() - ref["prior"]).abs().max())
    gen = (~present)[:, :, None] & (torch.arange(64)[None, None, :] < nb)
    want = torch.round(ref["prior"])
    differ = (out_c != want) & gen
    near = ((ref["prior"] - 0.5).abs() < 1e-5) & gen
    print(f"\nvar_bit={var_bit}: {int((~present).sum())} lost frames of {B * T}, {int(gen.sum())} generated bits, {int(near.sum())} within 1e-5 of a tie "
          f"(left out), {int(differ.sum())} differ from round(oracle prior); max |mel err| {e_mel:.2e}, |h_T err| {e_h:.2e}, |prior err| {e_p:.2e}")
    assert e_mel < 2e-4 and e_h < 2e-5
    assert e_p < 5e-6
    assert not bool((differ & ~near).any())
    assert int(near.sum()) < 0.01 * int(gen.sum())
    if var_bit:
        assert bool((out_c[~present][:, nb:] == 0.5).all())
    assert bool((out_c[gen] != 0.5).all())                                         # generated, not frames of no bits
    model.check_status()


# ------------------------------------------------------------------------------------------------ 3: one function, every schedule
@pytest.mark.parametrize("h_dim,B", [(1024, 3), (1024, 40), (1024, 64), (1024, 80), (1024, 256), (128, 5), (512, 5)])
def test_every_schedule_gives_the_same_bits(h_dim, B):
    model = mk(True, h_dim)[0]
    T, nb = 24, 35
    codes = random_codes(B, T, nb, seed=B + h_dim).to(DEV)
    present = co.loss_pattern(B, T, 0.1, seed=B, burst=6).to(DEV)
    bits = torch.full((B, T), float(nb), device=DEV)
    rng = np.random.default_rng(B)
    h0 = torch.from_numpy((0.2 * rng.standard_normal((B, h_dim))).astype(np.float32)).to(DEV)

    def fn():
        mel, hT, out, prior = conceal(model, codes, present, bits, h0)
        wav, filled = model.decode(codes, 256 * T, lost=~present, bitrate=3000, return_codes=True)
        return mel, hT, out, prior, wav, filled

    eng = model.engine()
    print(f"h_dim {h_dim} B {B}: flow_resident {eng.get_option('flow_resident')} flow_supported {eng.get_option('flow_supported')}")
    ref = on_schedule(model, "persistent", fn)
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[4]).all())
    gen = (~present)[:, :, None] & (torch.arange(64, device=DEV)[None, None, :] < nb)
    assert bool((ref[2][gen] != 0.5).all()) and torch.equal(ref[2][present], codes[present])
    for schedule in ("layers", "graph"):
        got = on_schedule(model, schedule, fn)
        for name, a, b in zip(("mel", "h_T", "codes_out", "prior", "wav", "filled"), ref, got):
            assert torch.equal(a, b), (schedule, name, float((a - b).abs().max()))
    model.check_status()


# ------------------------------------------------------------------------------------------------ 4: chunking and batching
@pytest.mark.parametrize("schedule", ["persistent", "layers"])
def test_chunking_and_batching(schedule):
    model = mk(True, 1024)[0]
    B, T, k, nb = 40, 30, 11, 35
    codes = random_codes(B, T, nb, seed=4).to(DEV)
    present = co.loss_pattern(B, T, 0.1, seed=5, burst=7).to(DEV)
    present[:, k - 2:k + 2] = False                                                # a burst across the cut
    bits = torch.full((B, T), float(nb), device=DEV)
    bits[:, 20:] = 17.0

    def run():
        whole = conceal(model, codes, present, bits)
        a = conceal(model, codes[:, :k].contiguous(), present[:, :k].contiguous(), bits[:, :k].contiguous())
        b = conceal(model, codes[:, k:].contiguous(), present[:, k:].contiguous(), bits[:, k:].contiguous(), a[1])
        row = conceal(model, codes[17:18].contiguous(), present[17:18].contiguous(), bits[17:18].contiguous())
        return whole + a + b + row

    r = on_schedule(model, schedule, run)
    whole, a, b, row = r[0:4], r[4:8], r[8:12], r[12:16]
    for i in (0, 2, 3):                                                            # mel, codes_out, prior
        assert torch.equal(whole[i], torch.cat([a[i], b[i]], 1)), i
        assert torch.equal(whole[i][17:18], row[i]), i
    assert torch.equal(whole[1], b[1]) and torch.equal(whole[1][17:18], row[1])
    model.check_status()


# ------------------------------------------------------------------------------------------------ 5: lost positions are never read
def test_lost_positions_of_the_codes_reach_nothing():
    model = mk(True, 1024)[0]
    B, T, nb = 40, 20, 35
    codes = random_codes(B, T, nb, seed=8).to(DEV)
    present = co.loss_pattern(B, T, 0.15, seed=9, burst=5).to(DEV)
    bits = torch.full((B, T), float(nb), device=DEV)
    lost = ~present
    outs = []
    for fill in ("nan", "inf", "bytes"):
        c = codes.clone()
        if fill == "nan":
            c[lost] = float("nan")
        elif fill == "inf":
            c[lost] = float("-inf")
        else:
            junk = torch.randint(0, 2 ** 31 - 1, c.shape, dtype=torch.int32, device=DEV).view(torch.float32)
            c[lost] = junk[lost]
        for schedule in ("persistent", "layers"):
            outs.append(on_schedule(model, schedule, lambda: conceal(model, c, present, bits) +
                                    tuple(model.decode(c, 256 * T, lost=lost, bitrate=3000, return_codes=True))))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    model.check_status()


# ------------------------------------------------------------------------------------------------ 6: no loss
@pytest.mark.parametrize("B", [64, 130])
def test_no_loss_agrees_with_plain_decode_to_rounding(B):
    """present all ones against bvc_bvrnn_decode / bvc_decode: the encode-ordered sums against the decode-ordered ones, the kind of
    difference bvc_forward has against encode + decode: mel / h_T within 2e-5 / 5e-6, waveform within 1e-5 RMS."""
    model = mk(True, 1024)[0]
    T, nb = 40, 35
    codes = random_codes(B, T, nb, seed=7 * B).to(DEV)
    present = torch.ones(B, T, dtype=torch.bool, device=DEV)
    bits = torch.full((B, T), float(nb), device=DEV)
    rng = np.random.default_rng(B)
    h0 = torch.from_numpy((0.2 * rng.standard_normal((B, 1024))).astype(np.float32)).to(DEV)
    mel, hT, out, _ = conceal(model, codes, present, bits, h0)
    mel0, hT0 = model.bvrnn.decode(codes, h0.unsqueeze(0))
    wav = model.decode(codes, 256 * T, lost=~present, bitrate=3000)
    wav0 = model.decode(codes, 256 * T)
    torch.cuda.synchronize()
    e_mel, e_h = float((mel - mel0).abs().max()), float((hT - hT0[0]).abs().max())
    rms = float((wav - wav0).pow(2).mean().sqrt())
    print(f"B {B}: no loss against the plain decode: max |mel| {e_mel:.2e}, |h_T| {e_h:.2e}, waveform rms {rms:.2e}")
    assert torch.equal(out, codes)
    assert e_mel < 2e-5 and e_h < 5e-6
    assert rms < 1e-5
    model.check_status()


# ------------------------------------------------------------------------------------------------ 7: sessions
def offline_stream(model, packets, present, rates):
    """bvc_decode_conceal of ONE stream's own packets: packets (F, 8), present (F,), rates (F,) the bitrate in force per frame.
    Returns (wav (256 F,), filled codes (F, 64))."""
    F = packets.shape[0]
    segs, i = [], 0
    while i < F:                                                # unpack with the bit count in force
        j = i
        while j < F and rates[j] == rates[i]:
            j += 1
        used = (model.active_bits(rates[i]) + 7) // 8
        segs.append(model.unpack(packets[None, i:j, :used].contiguous(), rates[i]))
        i = j
    codes = torch.cat(segs, 1)
    codes[0][~present] = float("nan")
    if len(set(rates)) == 1:
        wav, filled = model.decode(codes, 256 * F, lost=~present[None], bitrate=rates[0], return_codes=True)
        return wav[0], filled[0]
    # re-rated mid-stream: the same composition with the bits per frame as a tensor (bvc_bvrnn_decode_conceal, then the vocoder)
    from bvcodec.model import SCALING
    bits = torch.tensor([[model.bits_per_frame(r) for r in rates]], device=DEV)
    mel, _, filled, _ = conceal(model, codes, present[None], bits)
    wav = model.vocoder(mel, 256 * F, _scale_div=SCALING, _time_major=True)
    return wav[0, 0], filled[0]


@pytest.mark.parametrize("B,schedule", [(3, "flow"), (40, "flow"), (256, "flow"), (3, "graph"), (40, "graph")])
def test_receive_sessions_conceal_like_the_offline_call(B, schedule, monkeypatch):
    """Receive sessions with conceal="prior" fed from a send session's packets, 5 % of the frames dropped plus a burst per row, the
    dropped frames' bytes random; row 1 opened late, row 0 re-rated mid-stream, row 2 closed and re-opened.  Every stream's samples and
    filled codes equal bvc_decode_conceal of that stream's own packets alone, on the persistent tick and on the launch-per-layer tick
    (eager while the streams are cold, replayed from the concealing graph table from frame 33 on)."""
    from bvcodec.streaming import StreamingCodec
    model = mk(True, 1024)[0]
    set_schedule(monkeypatch, schedule)
    ks, packets = send_packets(model, B, 50)
    F = packets.shape[1]
    present = co.loss_pattern(B, F, 0.05, seed=30 + B, burst=6).to(DEV)
    present[0, 0] = False
    lossy = packets.clone()
    junk = torch.randint(0, 256, lossy.shape, dtype=torch.int32, device=DEV).to(torch.uint8)
    lossy[~present] = junk[~present]
    T_LATE, T_RATE, T_CLOSE, T_REOPEN = 6, 14, 17, 19

    def run(pk, conceal_arg):
        sc = StreamingCodec(model, B, 3000, open_all=False, direction="recv", **conceal_arg)
        rate = {b: RATES[b % 4] for b in range(B)}
        streams, live = [], {}

        def start(b, f):
            live[b] = dict(row=b, f0=f, wav=[], codes=[], rates=[])
            streams.append(live[b])

        for b in range(B):
            if b != 1:
                sc.open(b, rate[b]); start(b, 0)
        f = 0
        for i, k in enumerate(ks):
            if i == T_LATE:
                sc.open(1, rate[1]); start(1, f)
            if i == T_RATE:
                rate[0] = 1500; sc.set_bitrate(0, 1500)
            if i == T_CLOSE and B > 2:
                sc.close(2); del live[2]
            if i == T_REOPEN and B > 2:
                rate[2] = 3000; sc.open(2, 3000); start(2, f)
            w = sc.push_packets(pk[:, f:f + k], present[:, f:f + k])
            c = sc.filled_codes(k)
            for b, s in live.items():
                s["wav"].append(w[b].clone()); s["codes"].append(c[b].clone()); s["rates"] += [rate[b]] * k
            f += k
        torch.cuda.synchronize()
        return streams

    streams = run(lossy, dict(conceal="prior"))
    assert len(streams) == B + (1 if B > 2 else 0)
    worst = 0.0
    for s in streams:
        n = len(s["rates"])
        wav, filled = offline_stream(model, lossy[s["row"], s["f0"]:s["f0"] + n], present[s["row"], s["f0"]:s["f0"] + n], s["rates"])
        got_w, got_c = torch.cat(s["wav"]), torch.cat(s["codes"])
        worst = max(worst, float((got_w - wav).abs().max()))
        assert torch.equal(got_c, filled), (s["row"], s["f0"])
        assert torch.equal(got_w, wav), (s["row"], s["f0"], float((got_w - wav).abs().max()))
    print(f"B {B} {schedule}: {len(streams)} streams, {int((~present).sum())} lost frames; max |session - offline| {worst:.2e}")
    if B == 3:
        # what the dropped frames' bytes hold reaches nothing
        other = packets.clone()
        other[~present] = 0xFF
        for s, o in zip(streams, run(other, dict(conceal="prior"))):
            assert torch.equal(torch.cat(s["wav"]), torch.cat(o["wav"])) and torch.equal(torch.cat(s["codes"]), torch.cat(o["codes"]))
    model.check_status()


@pytest.mark.parametrize("schedule", ["flow", "graph"])
def test_set_conceal_switches_from_the_next_tick(schedule, monkeypatch):
    """A session that never calls set_conceal decodes what the header documents for it: the offline decode of the unpacked codes with
    0.5 at the lost frames (samples within 2e-6, the bar tests/test_gpu_stream_direction.py holds for a receive session against the
    offline call; codes equal); a session created with "prior" and set back before its first tick equals it.  A session that switches
    prior -> none -> prior between ticks (on the launch-per-layer schedule: between its two graph tables, all three switches in warm
    ticks) equals the first up to the first switch, and its codes follow, segment by segment with the carried state, from
    bvc_bvrnn_decode (frames of no bits) and bvc_bvrnn_decode_conceal."""
    from bvcodec.streaming import StreamingCodec
    model = mk(True, 1024)[0]
    set_schedule(monkeypatch, schedule)
    B = 3
    ks, packets = send_packets(model, B, 60)
    F = packets.shape[1]
    present = co.loss_pattern(B, F, 0.1, seed=3, burst=5).to(DEV)
    SWITCH = {26: "prior", 34: "none", 42: "prior"}
    cuts = [0] + [sum(ks[:i]) for i in sorted(SWITCH)] + [F]
    assert cuts[1] >= 33                                                           # the streams are warm at every switch
    modes = ["none", "prior", "none", "prior"]

    def run(mode):
        sc = StreamingCodec(model, B, 3000, open_all=False, direction="recv", **(dict(conceal="prior") if mode == "back" else {}))
        if mode == "back":
            sc.set_conceal("none")
        for b in range(B):
            sc.open(b, 3000)
        f, wav, codes = 0, [], []
        for i, k in enumerate(ks):
            if mode == "switch" and i in SWITCH:
                sc.set_conceal(SWITCH[i])
            wav.append(sc.push_packets(packets[:, f:f + k], present[:, f:f + k]).clone())
            codes.append(sc.filled_codes(k).clone())
            f += k
        torch.cuda.synchronize()
        return torch.cat(wav, 1), torch.cat(codes, 1)

    w0, c0 = run("never")
    holed = model.unpack(packets[:, :, :(model.active_bits(3000) + 7) // 8].contiguous(), 3000)
    holed[~present] = 0.5
    assert torch.equal(c0, holed)
    err = float((w0 - model.decode(holed, 256 * F)).abs().max())
    print(f"{schedule}: a session that never conceals against the offline decode of the holed codes: max |err| {err:.2e}")
    assert err <= 2e-6
    w1, c1 = run("back")
    assert torch.equal(w0, w1) and torch.equal(c0, c1)
    w2, c2 = run("switch")
    assert torch.equal(w2[:, :256 * cuts[1]], w0[:, :256 * cuts[1]])
    assert not torch.equal(w2[:, 256 * cuts[1]:], w0[:, 256 * cuts[1]:])
    bits = torch.full((B, F), 35.0, device=DEV)
    h = torch.zeros(B, 1024, device=DEV)
    for a, e, mode in zip(cuts[:-1], cuts[1:], modes):
        pr = present[:, a:e].contiguous()
        assert not bool(pr.all())                                                  # every segment has lost frames
        if mode == "none":
            assert torch.equal(c2[:, a:e], holed[:, a:e])                          # frames of no bits
            _, hT = model.bvrnn.decode(holed[:, a:e].contiguous(), h.unsqueeze(0))
            h = hT[0]
        else:
            _, h, filled, _ = conceal(model, holed[:, a:e].contiguous(), pr, bits[:, a:e].contiguous(), h)
            assert torch.equal(filled, c2[:, a:e]), (a, e)
            assert bool((filled[~pr][:, :35] != 0.5).all())                        # generated
    model.check_status()


# ------------------------------------------------------------------------------------------------ 8: errors
def test_errors():
    from bvcodec import BVRNNCodecModel, _abi, config, synth
    from bvcodec.streaming import StreamingCodec
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_test_noprior_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=99)
    bare = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    for k in [k for k in bare._tensors if k.startswith("prior.")]:
        del bare._tensors[k]                                    # created without the prior.* tensors
    T = 8
    codes = random_codes(3, T, 35, seed=1).to(DEV)
    present = torch.ones(3, T, dtype=torch.bool, device=DEV)
    present[:, 3] = False
    bits = torch.full((3, T), 35.0, device=DEV)
    with pytest.raises(_abi.BvcError, match="error -4"):
        conceal(bare, codes, present, bits)
    with pytest.raises(_abi.BvcError, match="error -4"):
        bare.decode(codes, 256 * T, lost=~present, bitrate=3000)
    with pytest.raises(_abi.BvcError, match="error -4"):
        StreamingCodec(bare, 3, 3000, direction="recv", conceal="prior")
    pk = torch.randint(0, 256, (3, T, 8), dtype=torch.int32, device=DEV).to(torch.uint8)
    sc, fresh = StreamingCodec(bare, 3, 3000, direction="recv"), StreamingCodec(bare, 3, 3000, direction="recv")
    w = [sc.push_packets(pk[:, :4], present[:, :4]).clone()]
    with pytest.raises(_abi.BvcError, match="error -4"):
        sc.set_conceal("prior")                                 # refused, the session untouched
    w.append(sc.push_packets(pk[:, 4:], present[:, 4:]).clone())
    v = [fresh.push_packets(pk[:, :4], present[:, :4]).clone(), fresh.push_packets(pk[:, 4:], present[:, 4:]).clone()]
    assert torch.equal(torch.cat(w, 1), torch.cat(v, 1))
    assert bool(torch.isfinite(bare.decode(codes, 256 * T)).all())            # (the bare model still decodes)
    bare.check_status()
    model = mk(True, 1024)[0]
    for direction in ("duplex", "send"):
        other = StreamingCodec(model, 3, 3000, direction=direction)
        with pytest.raises(ValueError, match="not a receive session"):
            other.set_conceal("prior")                           # BVC_EINVAL
        with pytest.raises(ValueError, match="not a receive session"):
            other.set_conceal("none")
    recv = StreamingCodec(model, 3, 3000, direction="recv")
    assert recv.eng.lib.bvc_stream_codec_set_conceal(recv.handle, 2) == -1
    recv.set_conceal("prior"); recv.set_conceal("none")
    model.check_status()
