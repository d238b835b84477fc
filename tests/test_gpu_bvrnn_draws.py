"""The mel coder against float64 outside the regime of the synthetic default draw (every |logit| < 0.5, every probability in
[0.45, 0.55], the KLD clamp never active): pinned checkpoints whose logits / GRU gates ARE a bias table (closed-form float64
references through the public entry points, on every schedule), the scaled draws `wide` and `saturated` next to `default` against the
float64 oracle (free-running with the tie rule, and teacher-forced one frame per call), one layer deep into the ELU tail, and a
streaming session on the saturated model.  Every float tensor, maximum norm: e_hip = max|hip - oracle64| <= MARGIN x max(e32,
2^-24 max|oracle64|), e32 the float32 oracle's own distance on the same case (vocoder_layers.compare; measured
ratios in profiles/bvrnn_draws_parity.md).  Needs the MI355X: run with ``-m gpu``."""
import numpy as np
import pytest
import torch

import bvrnn_draws as bd
from gpu_common import DEV, make_model, on_schedule
from oracle import bvrnn as obv

pytestmark = pytest.mark.gpu

LEDGERS = {}                                            # per draw (and "pinned"): the largest ratio per family, printed by the last test


def ledger(name):
    if name not in LEDGERS:
        LEDGERS[name] = bd.Ledger(name)
    return LEDGERS[name]


class Case:
    """Collects the verdicts of one test: all of them go to the draw's ledger, the failures are raised together at the end."""

    def __init__(self, draw, what):
        self.ledger, self.what, self.failures = ledger(draw), what, []

    def cmp(self, family, got, ref64, ref32, label):
        as3 = lambda a: np.asarray(a, dtype=np.float64).reshape((1,) * (3 - np.ndim(a)) + tuple(np.shape(a)))
        v = bd.compare(as3(got), as3(ref64), as3(ref32), f"{self.what} {label} {family}")
        print(f"  {family}: ratio {v.ratio:.3f} e_hip {v.e_hip:.3e} e32 {v.e32:.3e} scale {v.scale:.3e} [{self.what} {label}]", flush=True)
        self.ledger.add(family, v)
        if not v.ok:
            self.failures.append(v.message)

    def close(self):
        assert not self.failures, f"{len(self.failures)} comparisons failed:\n" + "\n".join(self.failures[:12])


def persistent_ready(model):
    eng = model.engine()
    assert eng.get_option("flow_supported") == 1 and eng.get_option("flow_resident") == 1


# the legs of the pinned checkpoints: (schedule, encode_fold = decode_fold)
LEGS = (("persistent", 1), ("persistent", 0), ("layers", 1), ("graph", 1))


def on_leg(model, leg, fn):
    schedule, fold = leg
    eng = model.engine()
    if schedule == "persistent":
        persistent_ready(model)
    try:
        eng.set_option("encode_fold", fold)
        eng.set_option("decode_fold", fold)
        return on_schedule(model, schedule, fn)
    finally:
        eng.set_option("encode_fold", 1)
        eng.set_option("decode_fold", 1)


# ---------------------------------------------------------------------------------------------- 1: pinned logits
@pytest.mark.parametrize("leg", LEGS, ids=lambda l: f"{l[0]}-fold{l[1]}")
@pytest.mark.parametrize("B", [5, 20])
@pytest.mark.parametrize("var_bit", [True, False], ids=["var", "fix"])
@pytest.mark.parametrize("h_dim", [128, 1024])
def test_pinned_logits(h_dim, var_bit, B, leg):
    """enc.4.weight = prior.4.weight = 0: the logits are the bias tables whatever the mel and the states are."""
    pinned_logits_case(h_dim, bd.Z, var_bit, B, leg)


def pinned_logits_case(h_dim, z_dim, var_bit, B, leg, ledger_name="pinned", forward=True, conceal=True):
    """The body of test_pinned_logits at a model size.  forward / conceal False: that entry point refuses this size (z_dim > h_dim,
    z_dim > 3 h_dim; tests/test_gpu_coder_sizes.py pins the refusals) and is left out."""
    Z = z_dim
    model = make_model(var_bit, h_dim, pinned="logits", z_dim=Z)[0]
    T = 3
    y, _ = bd.inputs(B, T, seed=B, z_dim=Z)
    bits = bd.pinned_bits(B, T, Z) if var_bit else None
    noise = bd.pinned_noise(B, T, z_dim=Z)
    r = torch.tensor([0.1, 0.9, 0.2])                              # h2, h, h2 with p_use_gen 0.3
    c64 = bd.pinned_logits_reference(B, T, bits, noise, torch.float64, Z)
    c32 = bd.pinned_logits_reference(B, T, bits, noise, torch.float32, Z)
    present = torch.tensor([[(b + t) % 3 != 0 for t in range(T)] for b in range(B)])
    rng = np.random.default_rng(B)
    recv = torch.from_numpy(rng.integers(0, 2, size=(B, T, Z)).astype(np.float32))
    h0 = torch.from_numpy((0.3 * rng.standard_normal((1, B, h_dim))).astype(np.float32)).to(DEV)
    yd, bd_, nd, rd, pd = y.to(DEV), None if bits is None else bits.to(DEV), noise.to(DEV), recv.to(DEV), present.to(DEV)

    names = ["codes", "prob"] + (["gz", "gprob", "gprior", "gkld", "sz", "sprob", "sprior", "skld"] if forward else []) + (["filled", "prior"] if conceal else [])

    def fn():
        codes, _, prob = model.bvrnn.encode(yd, bd_, h0, return_prob=True)
        out = [codes, prob]
        if forward:
            _, _, g = model.bvrnn(yd, 0.3, True, bd_, r=r, return_all=True)
            _, _, s = model.bvrnn(yd, 0.3, False, bd_, r=r, noise=nd, return_all=True)
            out += [g["z"], g["prob"], g["prior"], g["kld_frames"], s["z"], s["prob"], s["prior"], s["kld_frames"]]
        if conceal:
            _, _, filled, prior = model.bvrnn.decode(rd, h0, present=pd, bits=bd_, return_codes=True)
            out += [filled, prior]
        return tuple(out)

    o = dict(zip(names, (t.cpu() for t in on_leg(model, leg, fn))))
    codes, prob = o["codes"], o["prob"]
    case = Case(ledger_name, f"pinned logits h {h_dim}{'' if Z == bd.Z else f' z {Z}'} {'var' if var_bit else 'fix'} B {B}")
    label = f"{leg[0]} fold {leg[1]}"
    be, bq = bd.logit_tables(Z)
    full = lambda v: v[None, None, :].expand(B, T, Z)
    probs = (prob,) + ((o["gprob"], o["sprob"]) if forward else ())
    priors = ((o["gprior"], o["sprior"]) if forward else ()) + ((o["prior"],) if conceal else ())
    for fam, tensors, table, key in (("prob", probs, be, "prob"), ("prior", priors, bq, "prior")):
        order = torch.argsort(table, stable=True)
        for tns in tensors:
            assert bool(torch.isfinite(tns).all()) and bool((tns >= 0).all()) and bool((tns <= 1).all()), fam
            assert bool((tns[:, :, order].diff(dim=2) >= 0).all()), f"{fam} is not monotone in the logit"
            assert bool((tns[:, :, table == 0] == 0.5).all()), f"{fam} at logit 0 is not 0.5f"
            case.cmp(fam, tns, full(c64[key]), full(c32[key]), label)
    # codes: the sign of the logit, 0 at logit 0 (half to even), 0.5 where the frame carries no bit
    assert torch.equal(codes.double(), c64["codes"]), int((codes.double() != c64["codes"]).sum())
    if forward:
        gz, sz, gkld, skld = o["gz"], o["sz"], o["gkld"], o["skld"]
        case.cmp("z", gz, c64["z_greedy"], c32["z_greedy"], label + " greedy")
        case.cmp("z", sz, c64["z_sampled"], c32["z_sampled"], label + " sampled")
        assert bool(((c64["arg"] - 0.5).abs() >= 1e-3).all())
        assert torch.equal(torch.round(gz).double()[c64["mask"]], torch.round(c64["z_greedy"])[c64["mask"]])
        assert torch.equal(torch.round(sz).double()[c64["mask"]], torch.round(c64["z_sampled"])[c64["mask"]])
        assert bool((gz[~c64["mask"]] == 0.5).all()) and bool((sz[~c64["mask"]] == 0.5).all())
        case.cmp("kld_frames", gkld, c64["kld_frames"], c32["kld_frames"], label + " greedy")
        case.cmp("kld_frames", skld, c64["kld_frames"], c32["kld_frames"], label + " sampled")
    if conceal:
        want = torch.where(present[:, :, None], recv.double(), c64["generated"])
        assert torch.equal(o["filled"].double(), want), int((o["filled"].double() != want).sum())
    model.check_status()
    case.close()


# ---------------------------------------------------------------------------------------------- 2: pinned gates
@pytest.mark.parametrize("leg", LEGS, ids=lambda l: f"{l[0]}-fold{l[1]}")
@pytest.mark.parametrize("B", [5, 20])
@pytest.mark.parametrize("h_dim", [128, 1024])
def test_pinned_gates(h_dim, B, leg):
    """rnn.weight_ih_l0 = rnn.weight_hh_l0 = 0: r, z and both halves of n are bias tables over {-30 ... 30}, the state follows from h0."""
    pinned_gates_case(h_dim, bd.Z, B, leg)


def pinned_gates_case(h_dim, z_dim, B, leg, ledger_name="pinned"):
    """The body of test_pinned_gates at a model size."""
    model = make_model(True, h_dim, pinned="gates", z_dim=z_dim)[0]
    T = 3
    y, bits = bd.inputs(B, T, seed=B, z_dim=z_dim)
    h0 = bd.pinned_h0(B, h_dim)
    rng = np.random.default_rng(B)
    z = torch.from_numpy(rng.integers(0, 2, size=(B, T, z_dim)).astype(np.float32)).to(DEV)
    yd, bd_, hd = y.to(DEV), bits.to(DEV), h0[None].to(DEV)

    def fn():
        _, e1 = model.bvrnn.encode_stateful(yd[:, :1].contiguous(), bd_[:, :1].contiguous(), hd)
        _, d1 = model.bvrnn.decode(z[:, :1].contiguous(), hd)
        _, all_h = model.bvrnn.encode(yd, bd_, hd)
        _, e3 = model.bvrnn.encode_stateful(yd, bd_, hd)
        _, d3 = model.bvrnn.decode(z, hd)
        return e1[0], d1[0], all_h, e3[0], d3[0]

    e1, d1, all_h, e3, d3 = (o.cpu() for o in on_leg(model, leg, fn))
    h64, h32 = bd.pinned_gates_reference(h0, T, torch.float64), bd.pinned_gates_reference(h0, T, torch.float32)
    case = Case(ledger_name, f"pinned gates h {h_dim}{'' if z_dim == bd.Z else f' z {z_dim}'} B {B}")
    label = f"{leg[0]} fold {leg[1]}"
    assert torch.equal(all_h[:, 0], h0)
    case.cmp("h_T", e1, h64[0], h32[0], label + " encode T 1")
    case.cmp("h_T", d1, h64[0], h32[0], label + " decode T 1")
    case.cmp("all_h", all_h[:, 1:], torch.stack(h64[:2], 1), torch.stack(h32[:2], 1), label + " encode T 3")
    case.cmp("h_T", e3, h64[2], h32[2], label + " encode T 3")
    case.cmp("h_T", d3, h64[2], h32[2], label + " decode T 3")
    for got in (e1, d1, e3, d3):
        assert bool((got.abs() <= 1).all())                          # a convex mix of h and tanh
    model.check_status()
    case.close()


# ---------------------------------------------------------------------------------------------- 3: the draws, free-running
def free_running_schedules(h_dim, B):
    return ("persistent", "layers", "graph") if (h_dim, B) == (1024, 20) else ("persistent", "layers")


@pytest.mark.parametrize("h_dim,B,T", bd.SHAPES)
@pytest.mark.parametrize("draw", bd.DRAWS)
def test_free_running_against_float64(draw, h_dim, B, T):
    ref = bd.reference(draw, h_dim, B, T)
    model = make_model(True, h_dim, seed=bd.seed_of(h_dim, draw), gains=bd.GAINS[draw])[0]
    persistent_ready(model)
    o64, o32, c32 = ref["o64"], ref["o32"], ref["cuts32"]
    y, bits, noise = ref["y"].to(DEV), ref["bits"].to(DEV), ref["noise"].to(DEV)
    codes_in, present = ref["codes"].to(DEV), ref["present"].to(DEV)
    h0 = torch.zeros(1, B, h_dim, device=DEV)
    case = Case(draw, f"{draw} h {h_dim} B {B} T {T}")

    def fn():
        codes, all_h, prob = model.bvrnn.encode(y, bits, h0, return_prob=True)
        _, ehT = model.bvrnn.encode_stateful(y, bits, h0)
        mel, dhT = model.bvrnn.decode(codes_in, h0)
        dec, _, ex = model.bvrnn(y, 0.3, False, bits, r=ref["r"], noise=noise, return_all=True)
        cmel, chT, filled, cprior = model.bvrnn.decode(codes_in, h0, present=present, bits=bits, return_codes=True)
        return (codes, all_h, prob, ehT[0], mel, dhT[0], dec, ex["z"], ex["prob"], ex["prior"], ex["kld_frames"], cmel, chT[0], filled, cprior)

    first = None
    for schedule in free_running_schedules(h_dim, B):
        out = [o.cpu() for o in on_schedule(model, schedule, fn)]
        if first is None:
            first = out
        else:                                                        # every schedule gives the same bits
            for i, (a, b) in enumerate(zip(first, out)):
                assert torch.equal(a, b), (schedule, i, float((a - b).abs().max()))
            continue
        codes, all_h, prob, ehT, mel, dhT, dec, z, fprob, fprior, kld, cmel, chT, filled, cprior = out
        cuts = bd.cuts_of(ref, codes, z, filled, "hip")
        for c in cuts.values():
            print(" ", c, flush=True)
            c.check()
        whole = lambda cut: int(cut.first.min()) == T                # no row cut: values behind the last frame are compared too
        # encode
        ce, ce32 = cuts["encode"], c32["encode"]
        e64 = o64["encode"]
        for fam, got, key in (("prob", prob, "prob"), ("all_h", all_h, "all_h")):
            r64 = bd.n64(e64[key])
            case.cmp(fam, ce.mask(got, r64, True), r64, ce32.mask(o32["encode"][key], r64, True), schedule + " encode")
        if whole(ce) and whole(ce32):
            case.cmp("h_T", ehT, e64["h_last"], o32["encode"]["h_last"], schedule + " encode")
        # decode of the float64 oracle's codes: nothing is rounded, nothing is cut
        case.cmp("mel", mel, o64["decode"]["mel"], o32["decode"]["mel"], schedule + " decode")
        case.cmp("h_T", dhT, o64["decode"]["h_last"], o32["decode"]["h_last"], schedule + " decode")
        # forward, sampled
        cf, cf32, f64 = cuts["forward"], c32["forward"], o64["forward"]
        for fam, got, key, incl in (("prob", fprob, "prob", True), ("prior", fprior, "prior", True), ("z", z, "z", False), ("dec", dec, "dec", False)):
            r64 = bd.n64(f64[key])
            case.cmp(fam, cf.mask(got, r64, incl), r64, cf32.mask(o32["forward"][key], r64, incl), schedule + " forward")
        n = min(T, min(cf.frames_all_rows(), cf32.frames_all_rows()) + 1)     # (the frame of a first difference: its KLD precedes the rounding)
        case.cmp("kld_frames", kld[:n], f64["kld_frames"][:n], o32["forward"]["kld_frames"][:n], schedule + " forward")
        # the concealing decoder
        cc, cc32, k64 = cuts["conceal"], c32["conceal"], o64["conceal"]
        for fam, got, key, incl in (("prior", cprior, "prior", True), ("mel", cmel, "mel", False)):
            r64 = bd.n64(k64[key])
            case.cmp(fam, cc.mask(got, r64, incl), r64, cc32.mask(o32["conceal"][key], r64, incl), schedule + " conceal")
        if whole(cc) and whole(cc32):
            case.cmp("h_T", chT, k64["h_last"], o32["conceal"]["h_last"], schedule + " conceal")
    model.check_status()
    case.close()


# ---------------------------------------------------------------------------------------------- 4: teacher-forced, one frame per call
@pytest.mark.parametrize("draw", bd.DRAWS)
def test_teacher_forced_one_frame_per_call(draw):
    """encode and decode restarted at the float64 oracle's state before frame t (rounded to float32: all three implementations start
    from that same state): an error belongs to one step."""
    h_dim, B, T = bd.SHAPES[0]
    ref = bd.reference(draw, h_dim, B, T)
    model = make_model(True, h_dim, seed=bd.seed_of(h_dim, draw), gains=bd.GAINS[draw])[0]
    sd, e64 = ref["sd"], ref["o64"]["encode"]
    case = Case(draw, f"{draw} teacher-forced h {h_dim} B {B}")
    for t in bd.TEACHER_FRAMES:
        h = e64["all_h"][:, t].float()
        y1, b1, z1 = ref["y"][:, t:t + 1], ref["bits"][:, t:t + 1], ref["codes"][:, t:t + 1]
        r64, r32 = obv.encode(sd, y1, b1, h, dtype=torch.float64), obv.encode(sd, y1, b1, h)
        d64, d32 = obv.decode(sd, z1, h, dtype=torch.float64), obv.decode(sd, z1, h)
        hd = h[None].to(DEV)
        codes, _, prob = model.bvrnn.encode(y1.to(DEV), b1.to(DEV), hd, return_prob=True)
        c2, ehT = model.bvrnn.encode_stateful(y1.to(DEV), b1.to(DEV), hd)
        mel, dhT = model.bvrnn.decode(z1.to(DEV), hd)
        assert torch.equal(codes, c2)
        cut = bd.Cut(f"hip {draw} frame {t} codes", codes.cpu(), r64["codes"], r64["prob"], bd.bit_mask(b1).numpy())
        cut32 = bd.Cut(f"float32 oracle {draw} frame {t} codes", r32["codes"], r64["codes"], r64["prob"], bd.bit_mask(b1).numpy())
        print(" ", cut, flush=True)
        cut.check()
        label = f"frame {t}"
        case.cmp("prob", prob.cpu(), r64["prob"], r32["prob"], label + " encode")
        if cut.rows_cut == 0 and cut32.rows_cut == 0:
            case.cmp("h_T", ehT[0].cpu(), r64["h_last"], r32["h_last"], label + " encode")
        case.cmp("mel", mel.cpu(), d64["mel"], d32["mel"], label + " decode")
        case.cmp("h_T", dhT[0].cpu(), d64["h_last"], d32["h_last"], label + " decode")
    model.check_status()
    case.close()


# ---------------------------------------------------------------------------------------------- 5: one layer, deep into the ELU tail
@pytest.mark.parametrize("M,N,K", bd.ELU_SHAPES)
def test_elu_tail_one_layer(M, N, K):
    from bvcodec import _abi
    lib = _abi.load()
    x, w, b, pre, ref64, ref32 = bd.elu_case(M, N, K)
    assert float(pre.min()) < -25 and float(pre.max()) > 15
    xd, wd, bd_ = x.to(DEV), w.to(DEV), b.to(DEV)
    st = _abi.current_stream(torch.device(DEV))
    y1 = torch.full((M, N), float("nan"), device=DEV)
    y2 = torch.full((M, N), float("nan"), device=DEV)
    _abi.check(lib.bvc_test_linear(_abi.ptr(xd), _abi.ptr(wd), _abi.ptr(bd_), M, N, K, 1, _abi.ptr(y1), st))
    _abi.check(lib.bvc_test_linear_batched(_abi.ptr(xd), _abi.ptr(wd), _abi.ptr(bd_), M, N, K, 1, _abi.ptr(y2), st))
    torch.cuda.synchronize()
    case = Case("layer", f"elu(linear) M {M} N {N} K {K}")
    case.cmp("elu", y1.cpu(), ref64, ref32, "recurrent-layer kernel")
    assert torch.equal(y1, y2), float((y1 - y2).abs().max())
    assert bool((y1 >= -1).all())
    case.close()


# ---------------------------------------------------------------------------------------------- 6: a streaming session, saturated
def test_streaming_session_on_the_saturated_model_equals_offline():
    """A duplex session of 441-sample hops on the saturated draw: the codes and the samples of every tick are the offline call's."""
    from bvcodec import synth
    from bvcodec.streaming import StreamingCodec
    model = make_model(True, 1024, gains=bd.GAINS["saturated"])[0]
    B, hop, ticks = 3, 441, 12
    L = hop * ticks
    x = synth.synthetic_speech(B, L, seed=23, kind="speech").to(DEV)
    sc = StreamingCodec(model, B, 3000, hop=hop)
    codes, wavs = [], []
    for i in range(ticks):
        c, w = sc.push(x[:, i * hop:(i + 1) * hop])
        codes.append(c.clone())
        wavs.append(w.clone())
    torch.cuda.synchronize()
    codes, wav = torch.cat(codes, 1), torch.cat(wavs, 1)
    F = codes.shape[1]
    assert F == (L - 768) // 256 + 1 and wav.shape[1] == 256 * F
    off = model.encode(x, 3000)
    nb = model.active_bits(3000)
    assert bool((off[:, :, :nb] != 0.5).all()) and 0.2 < float(off[:, :, :nb].mean()) < 0.8       # (not a constant code)
    assert torch.equal(codes, off[:, :F])
    wav_off = model.decode(off, L)[:, :256 * F]
    print(f"saturated session: {F} frames, max |session - offline| samples {float((wav - wav_off).abs().max()):.3e}", flush=True)
    assert torch.equal(wav, wav_off)
    model.check_status()


# ---------------------------------------------------------------------------------------------- the ledger
def test_parity_ledger():
    """Prints the PARITY lines of everything this module compared so far (profiles/bvrnn_draws_parity.md); fails if any comparison did."""
    bad = []
    for name in ("pinned", "layer") + bd.DRAWS:
        if name in LEDGERS:
            try:
                LEDGERS[name].close()
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, "\n".join(bad)
