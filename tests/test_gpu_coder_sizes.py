"""The mel coder against float64 at the model sizes the config checks accept beside the shipped ones (profiles/coder_sizes.md):
every class of bvrnn_draws.SIZE_CLASSES - h_dim below, between and beyond the sizes the persistent kernel is laid out for, z_dim
from one k-block to more than the persistent kernel and the repair window take - on the default and the wide draw, through encode,
decode, the sampled forward and the concealing decoder on every schedule the size can take; the pinned checkpoints at four of the
sizes; and the wire format (pack / unpack and a send session feeding a receive session) where a frame is not 8 bytes.  A size that
an entry point refuses is held to the refusal's text.  The bar is the suite's: e_hip <= MARGIN x max(e32,
2^-24 max|oracle64|) per tensor, rounded outputs under the tie rule with its caps.  Needs the MI355X: run with ``-m gpu``."""
import re

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import test_gpu_bvrnn_draws as gd
from gpu_common import DEV, make_model, on_schedule

pytestmark = pytest.mark.gpu

SIZES = [(h, z) for _, h, z, _ in bd.SIZE_CLASSES]


def ledger_of(h_dim, z_dim):
    return "sizes: " + bd.class_of(h_dim, z_dim)


def schedules_of(model, h_dim, z_dim):
    """Where the persistent kernel exists both schedules run; where it does not the option says so, and asking for it changes nothing."""
    eng = model.engine()
    if bd.flow_supported(h_dim, z_dim):
        gd.persistent_ready(model)
        return ("persistent", "layers")
    assert eng.get_option("flow_supported") == 0
    return ("layers", "persistent")


def refused(text):
    return pytest.raises(RuntimeError, match=re.escape(text))


# ---------------------------------------------------------------------------------------------- 1: the draws, free-running
@pytest.mark.parametrize("h_dim,z_dim,B,T", bd.SIZE_CASES)
@pytest.mark.parametrize("draw", bd.SIZE_DRAWS)
def test_sizes_against_float64(draw, h_dim, z_dim, B, T):
    ref = bd.reference(draw, h_dim, B, T, z_dim)
    model = make_model(True, h_dim, seed=bd.seed_of(h_dim, draw, z_dim), gains=bd.GAINS[draw], z_dim=z_dim)[0]
    fwd, fallback, conceal = bd.forward_runs(h_dim, z_dim), bd.forward_fallback_runs(h_dim, z_dim), bd.conceal_runs(h_dim, z_dim)
    o64, o32, c32 = ref["o64"], ref["o32"], ref["cuts32"]
    y, bits, noise = ref["y"].to(DEV), ref["bits"].to(DEV), ref["noise"].to(DEV)
    codes_in, present = ref["codes"].to(DEV), ref["present"].to(DEV)
    h0 = torch.zeros(1, B, h_dim, device=DEV)
    case = gd.Case(ledger_of(h_dim, z_dim), f"{draw} h {h_dim} z {z_dim} B {B} T {T}")
    cut_at = 5 if T == 12 else 1                                    # chunked decode: 5 + 7 frames (1 + 3 of the four-frame case)

    # what this size does not run is refused, with its message, before anything is launched
    if not fwd:
        with refused(bd.FORWARD_REFUSAL):
            model.bvrnn(y, 0.3, False, bits, r=ref["r"], noise=noise, return_all=True)
    elif not fallback:
        with refused(bd.FORWARD_NEEDS_Z):
            model.bvrnn(y, 0.3, False, bits, r=ref["r"], noise=noise)
    if not conceal:
        with refused(bd.CONCEAL_REFUSAL):
            model.bvrnn.decode(codes_in, h0, present=present, bits=bits, return_codes=True)

    names = ["codes", "all_h", "prob", "ehT", "mel", "dhT", "mel_chunks", "dhT_chunks"]
    names += ["dec", "z", "fprob", "fprior", "kld", "kld_mean"] if fwd else []
    names += ["dec_fb", "kld_fb"] if fallback else []
    names += ["cmel", "chT", "filled", "cprior"] if conceal else []

    def fn():
        codes, all_h, prob = model.bvrnn.encode(y, bits, h0, return_prob=True)
        _, ehT = model.bvrnn.encode_stateful(y, bits, h0)
        mel, dhT = model.bvrnn.decode(codes_in, h0)
        m1, h1 = model.bvrnn.decode(codes_in[:, :cut_at].contiguous(), h0)
        m2, h2 = model.bvrnn.decode(codes_in[:, cut_at:].contiguous(), h1)
        out = [codes, all_h, prob, ehT[0], mel, dhT[0], torch.cat([m1, m2], 1), h2[0]]
        if fwd:
            dec, _, ex = model.bvrnn(y, 0.3, False, bits, r=ref["r"], noise=noise, return_all=True)
            out += [dec, ex["z"], ex["prob"], ex["prior"], ex["kld_frames"], torch.mean(ex["kld_frames"]).reshape(1)]
        if fallback:                                                 # the sample, prob and prior in the workspace's own buffers
            dec2, kld2 = model.bvrnn(y, 0.3, False, bits, r=ref["r"], noise=noise)
            out += [dec2, kld2.reshape(1)]
        if conceal:
            cmel, chT, filled, cprior = model.bvrnn.decode(codes_in, h0, present=present, bits=bits, return_codes=True)
            out += [cmel, chT[0], filled, cprior]
        return tuple(out)

    first = None
    for schedule in schedules_of(model, h_dim, z_dim):
        o = dict(zip(names, (t.cpu() for t in on_schedule(model, schedule, fn))))
        for k, v in o.items():
            assert bool(torch.isfinite(v).all()), (schedule, k)
        # chunked == whole, on every schedule
        assert torch.equal(o["mel_chunks"], o["mel"]) and torch.equal(o["dhT_chunks"], o["dhT"]), schedule
        if fallback:
            assert torch.equal(o["dec_fb"], o["dec"]) and torch.equal(o["kld_fb"], o["kld_mean"]), schedule
        if first is not None:                                        # every schedule gives the same bits
            for k in names:
                assert torch.equal(first[k], o[k]), (schedule, k, float((first[k] - o[k]).abs().max()))
            continue
        first = o
        cuts = bd.cuts_of(ref, o["codes"], o["z"] if fwd else o64["forward"]["z"], o["filled"] if conceal else o64["conceal"]["codes_out"],
                          "hip", z_dim=z_dim)
        for name, c in cuts.items():
            if (name == "forward" and not fwd) or (name == "conceal" and not conceal):
                continue
            print(" ", c, flush=True)
            c.check()
        whole = lambda cut: int(cut.first.min()) == T                # no row cut: values behind the last frame are compared too
        # encode
        ce, ce32 = cuts["encode"], c32["encode"]
        e64 = o64["encode"]
        for fam, key in (("prob", "prob"), ("all_h", "all_h")):
            r64 = bd.n64(e64[key])
            case.cmp(fam, ce.mask(o[key], r64, True), r64, ce32.mask(o32["encode"][key], r64, True), schedule + " encode")
        if whole(ce) and whole(ce32):
            case.cmp("h_T", o["ehT"], e64["h_last"], o32["encode"]["h_last"], schedule + " encode")
        # decode of the float64 oracle's codes: nothing is rounded, nothing is cut
        case.cmp("mel", o["mel"], o64["decode"]["mel"], o32["decode"]["mel"], schedule + " decode")
        case.cmp("h_T", o["dhT"], o64["decode"]["h_last"], o32["decode"]["h_last"], schedule + " decode")
        if fwd:                                                      # forward, sampled
            cf, cf32, f64 = cuts["forward"], c32["forward"], o64["forward"]
            for fam, got, key, incl in (("prob", "fprob", "prob", True), ("prior", "fprior", "prior", True), ("z", "z", "z", False), ("dec", "dec", "dec", False)):
                r64 = bd.n64(f64[key])
                case.cmp(fam, cf.mask(o[got], r64, incl), r64, cf32.mask(o32["forward"][key], r64, incl), schedule + " forward")
            n = min(T, min(cf.frames_all_rows(), cf32.frames_all_rows()) + 1)     # (the frame of a first difference: its KLD precedes the rounding)
            case.cmp("kld_frames", o["kld"][:n], f64["kld_frames"][:n], o32["forward"]["kld_frames"][:n], schedule + " forward")
        if conceal:                                                  # the concealing decoder
            cc, cc32, k64 = cuts["conceal"], c32["conceal"], o64["conceal"]
            for fam, got, key, incl in (("prior", "cprior", "prior", True), ("mel", "cmel", "mel", False)):
                r64 = bd.n64(k64[key])
                case.cmp(fam, cc.mask(o[got], r64, incl), r64, cc32.mask(o32["conceal"][key], r64, incl), schedule + " conceal")
            if whole(cc) and whole(cc32):
                case.cmp("h_T", o["chT"], k64["h_last"], o32["conceal"]["h_last"], schedule + " conceal")
    model.check_status()
    case.close()


# ---------------------------------------------------------------------------------------------- 2: the pinned checkpoints
def legs_of(h_dim, z_dim):
    return gd.LEGS if bd.flow_supported(h_dim, z_dim) else (("layers", 1), ("graph", 1))


PINNED_LEGS = [(h, z, leg) for h, z in bd.PINNED_SIZES for leg in legs_of(h, z)]
leg_id = lambda v: f"{v[0]}-fold{v[1]}" if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("h_dim,z_dim,leg", PINNED_LEGS, ids=leg_id)
@pytest.mark.parametrize("B", [5, 20])
def test_pinned_logits_at_sizes(h_dim, z_dim, leg, B):
    """The code epilogue's mask at bit counts up to z_dim and the KLD sum over z_dim terms against closed forms."""
    gd.pinned_logits_case(h_dim, z_dim, True, B, leg, ledger_name=ledger_of(h_dim, z_dim),
                          forward=bd.forward_runs(h_dim, z_dim), conceal=bd.conceal_runs(h_dim, z_dim))


@pytest.mark.parametrize("h_dim,z_dim,leg", PINNED_LEGS, ids=leg_id)
@pytest.mark.parametrize("B", [5, 20])
def test_pinned_gates_at_sizes(h_dim, z_dim, leg, B):
    """The GRU epilogue over an h_dim that is no power of two against its closed form."""
    gd.pinned_gates_case(h_dim, z_dim, B, leg, ledger_name=ledger_of(h_dim, z_dim))


# ---------------------------------------------------------------------------------------------- 3: the wire format
def wire_rates(model, z_dim):
    """A bitrate whose bit count ends inside a byte and one that saturates at z_dim."""
    part, full = (1000 if z_dim <= 32 else 3000), int(z_dim * 22050 / 256 * 1.1)
    n = model.active_bits(part)
    assert n % 8 and n < z_dim and model.active_bits(full) == z_dim and model.bits_per_frame(full) > z_dim
    return part, full


def packbits(codes, nbits):
    return np.packbits((codes[..., :nbits].cpu().numpy() > 0.75).astype(np.uint8), axis=-1, bitorder="little")


@pytest.mark.parametrize("h_dim,z_dim", bd.WIRE_SIZES)
def test_pack_unpack_at_sizes(h_dim, z_dim):
    model = make_model(True, h_dim, z_dim=z_dim)[0]
    rng = np.random.default_rng(z_dim)
    B, T = 5, 7
    for rate in wire_rates(model, z_dim):
        n = model.active_bits(rate)
        codes = torch.from_numpy(rng.integers(0, 2, size=(B, T, z_dim)).astype(np.float32))
        codes[:, :, n:] = 0.5
        codes = codes.to(DEV)
        packed = model.pack(codes, rate)
        assert packed.dtype == torch.uint8 and packed.shape == (B, T, (n + 7) // 8)
        assert np.array_equal(packed.cpu().numpy(), packbits(codes, n))
        assert torch.equal(model.unpack(packed, rate), codes)
    model.check_status()


@pytest.mark.parametrize("h_dim,z_dim", bd.WIRE_SIZES + ((64, 144),))
def test_send_session_feeds_receive_session_at_sizes(h_dim, z_dim):
    """Three ticks of a send session, B = 5 rows at two rates: the packets are numpy's little-order packing of the offline encode's
    codes, zeros behind each row's bits, and a receive session fed with them gives the offline decode's samples.  z_dim 144: a frame
    of 18 bytes is more than a late packet carries, so the repair window is refused and the session runs without it."""
    from bvcodec import synth
    import gpu_sessions as gs
    model = make_model(True, h_dim, z_dim=z_dim)[0]
    B, hop, ticks = 5, 441, 3
    bpf = (z_dim + 7) // 8
    part, full = wire_rates(model, z_dim)
    rates = [part if b % 2 == 0 else full for b in range(B)]
    x = synth.synthetic_speech(B, hop * ticks, seed=z_dim, kind="speech").to(DEV)
    s = gs.drive_sender(model, "send", x, hop, rates)
    ks, packets, codes = s.ks, s.first, s.second
    F = sum(ks)
    assert F == (hop * ticks - 768) // 256 + 1 == 3 and packets.dtype == torch.uint8 and tuple(packets.shape) == (B, F, bpf)
    packets, codes = packets.clone(), codes.clone()
    for b in range(B):
        n = model.active_bits(rates[b])
        off = model.encode(x[b:b + 1], rates[b])[:, :F]
        assert bool((off[:, :, :n] != 0.5).all()) and bool((off[:, :, n:] == 0.5).all())
        assert torch.equal(codes[b:b + 1], off), b
        got, used = packets[b].cpu().numpy(), (n + 7) // 8
        assert np.array_equal(got[:, :used], packbits(off[0], n)), b
        assert not got[:, used:].any(), b
    r = gs.drive_receiver(model, packets, [k for k in ks if k], rates, on_tick=gs.every_row_runs)
    wav, sc = r.wav, r.sc
    assert sc.bytes_per_frame == bpf
    if bpf > 16:
        with pytest.raises(ValueError, match=f"bvc_stream_codec_set_repair: frames of {bpf} bytes"):
            sc.set_repair(4)
        assert sc.repair == 0
    L = hop * ticks
    for b in range(B):
        off = model.decode(codes[b:b + 1].contiguous(), L)[:, :256 * F]
        assert torch.equal(wav[b:b + 1], off), (b, float((wav[b:b + 1] - off).abs().max()))
    model.check_status()


# ---------------------------------------------------------------------------------------------- the ledger
def test_sizes_parity_ledger():
    """Prints the PARITY lines of everything this module compared so far (profiles/coder_sizes.md); fails if any comparison did."""
    bad = []
    print(flush=True)
    for name in sorted(n for n in gd.LEDGERS if n.startswith("sizes: ")):
        try:
            gd.LEDGERS[name].close()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
