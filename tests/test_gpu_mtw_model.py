"""The documented switches of the recurrent-layer kernels through the model: BVC_MTW=2|4 (2 or 4 row tiles of 16 per workgroup:
SK_LIN2 / SK_LIN4 / SK_GRU_IL2 of csrc/k_gemm.hip and the multi-frame twins) and BVC_LATENCY=1 (SK_LIN_LATENCY) give the bits of the
default model - DESIGN.md section 5 and INTEGRATION.md promise it - on every entry point that runs the layer kernels: encode, decode,
the training-time forward, the concealing decoder, the entropy-coded wire, the closed-loop rates and a streaming session.  BVC_MTW is
read at bvc_model_create, so the three models live in this process; BVC_LATENCY is read once per process and gets a child process.
The kernels alone, against float64: tests/test_gpu_skinny_tiles.py.  Needs the MI355X: run with ``-m gpu``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import conceal_oracle as co
import skinny_kernels as sk
from gpu_common import DEV, make_model, on_schedule
from oracle import bvrnn as obv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHED = ("2", "4")
BATCHES = (5, 17, 40, 49, 65)            # 1, 2, 3, 4, 5 row tiles: the clamp of mtw, last groups with 1 and 3 tiles missing, a last tile of one row
FRAMES = (1, 3, 4, 5, 12)                # <= 4: the all-frame layers on the multi-frame twins (1: the one-frame kernel); 5: the batched prologue


def models(h_dim, var_bit=True, **kw):
    """(the default model, {"2": the BVC_MTW=2 one, "4": ...}) of one checkpoint."""
    return make_model(var_bit, h_dim, **kw)[0], {v: make_model(var_bit, h_dim, env={"BVC_MTW": v}, **kw)[0] for v in SWITCHED}


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and bool(torch.isfinite(b).all()), (what, i)
        assert torch.equal(a, b), (what, i, float((a - b).abs().max()))


def coder_calls(model, B, T, var_bit, h_dim, seed):
    """encode (codes, all_h, prob) and decode (mel, hT) of seeded inputs from a non-zero state."""
    y, bits = bd.inputs(B, T, seed=seed)
    yd, bd_ = y.to(DEV), bits.to(DEV) if var_bit else None
    h0 = torch.from_numpy((0.3 * np.random.default_rng(seed).standard_normal((1, B, h_dim))).astype(np.float32)).to(DEV)

    def fn():
        codes, all_h, prob = model.bvrnn.encode(yd, bd_, h0, return_prob=True)
        mel, hT = model.bvrnn.decode(codes, h0)
        return codes, all_h, prob, mel, hT
    return fn


# ---------------------------------------------------------------------------------------------- 1: encode and decode, the sweep
@pytest.mark.parametrize("var_bit", [True, False], ids=["var", "fix"])
@pytest.mark.parametrize("B", BATCHES)
def test_encode_decode_on_the_layer_schedule(B, var_bit):
    base, switched = models(128, var_bit)
    for T in FRAMES:
        want = on_schedule(base, "layers", coder_calls(base, B, T, var_bit, 128, 100 * B + T))
        assert 0.1 < float((want[0] == 1).float().mean()) < 0.9                     # (not a constant code)
        for v, m in switched.items():
            same(on_schedule(m, "layers", coder_calls(m, B, T, var_bit, 128, 100 * B + T)), want, f"BVC_MTW={v} B {B} T {T}")


@pytest.mark.parametrize("T", [3, 12])
def test_encode_decode_on_the_persistent_schedule(T):
    """The recurrence itself is the persistent kernel's; the all-frame prologues and the decoder's epilogue take the row tiles per workgroup."""
    B = 49
    base, switched = models(128)
    for m in (base,) + tuple(switched.values()):
        eng = m.engine()
        assert eng.get_option("flow_supported") == 1 and eng.get_option("flow_resident") == 1
    want = on_schedule(base, "persistent", coder_calls(base, B, T, True, 128, 7 + T))
    same(want, on_schedule(base, "layers", coder_calls(base, B, T, True, 128, 7 + T)), "schedules of the default model")
    for v, m in switched.items():
        same(on_schedule(m, "persistent", coder_calls(m, B, T, True, 128, 7 + T)), want, f"BVC_MTW={v} persistent T {T}")


@pytest.mark.parametrize("which", ["saturated", "pinned"])
def test_encode_decode_at_the_shipped_size(which):
    """h_dim 1024 (64 k-blocks per layer, 128 in the concatenated ones), 40 rows = 3 row tiles, on checkpoints that leave the default
    draw's narrow regime: saturating gains, and logits pinned to the bias table."""
    kw = dict(gains=bd.GAINS["saturated"]) if which == "saturated" else dict(pinned="logits")
    base, switched = models(1024, **kw)
    for T in (3, 5):
        want = on_schedule(base, "layers", coder_calls(base, 40, T, True, 1024, 40 + T))
        for v, m in switched.items():
            same(on_schedule(m, "layers", coder_calls(m, 40, T, True, 1024, 40 + T)), want, f"BVC_MTW={v} {which} T {T}")


# ---------------------------------------------------------------------------------------------- 2: the other entry points
@pytest.mark.parametrize("B", [17, 65])
def test_forward_conceal_and_entropy(B):
    T, Z, H = 6, bd.Z, 128
    base, switched = models(H)
    y, bits = bd.inputs(B, T, seed=B)
    r, noise = obv.draw_randomness(T, B, Z, False, generator=torch.Generator().manual_seed(77))
    present = co.loss_pattern(B, T, 0.2, seed=B + T, burst=2)
    assert bool((~present).any()) and bool(present.any())
    recv = torch.from_numpy(np.random.default_rng(B).integers(0, 2, size=(B, T, Z)).astype(np.float32))
    yd, bd_, nd, pd, rd = y.to(DEV), bits.to(DEV), noise.to(DEV), present.to(DEV), recv.to(DEV)
    h0 = torch.zeros(1, B, H, device=DEV)

    def calls(m):
        def fn():
            gdec, _, g = m.bvrnn(yd, 0.3, True, bd_, r=r, return_all=True)
            sdec, _, s = m.bvrnn(yd, 0.3, False, bd_, r=r, noise=nd, return_all=True)
            cmel, chT, filled, prior = m.bvrnn.decode(rd, h0, present=pd, bits=bd_, return_codes=True)
            return (gdec, g["z"], g["prob"], g["prior"], g["kld_frames"], sdec, s["z"], s["prob"], s["prior"], s["kld_frames"], cmel, chT, filled, prior)
        return fn

    want = on_schedule(base, "layers", calls(base))
    lost = (~present)[:, :, None] & bd.bit_mask(bits)
    assert bool((want[12].cpu()[lost] != 0.5).all()) and bool((want[12].cpu()[present] == recv[present]).all())     # generated where lost, received elsewhere
    for v, m in switched.items():
        same(on_schedule(m, "layers", calls(m)), want, f"BVC_MTW={v} forward / conceal B {B}")
    if B != 17:
        return
    codes = on_schedule(base, "layers", lambda: base.bvrnn.encode(yd, bd_, h0))[0]

    def wire(m):
        def fn():
            data, sizes, hT_s = m.bvrnn.entropy_pack(codes, bd_, h0, segment=4)
            got, mel, hT = m.bvrnn.entropy_unpack(data, sizes, T, bd_, h0, segment=4)
            return data, sizes, hT_s, got, mel, hT
        return fn

    want = on_schedule(base, "layers", wire(base))
    assert torch.equal(want[3], codes)
    for v, m in switched.items():
        got = on_schedule(m, "layers", wire(m))
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (v, i)


def test_closed_loop_rates():
    """bvc_bvrnn_encode_vbr: the K = 4 rungs of B = 5 rows are 20 candidate rows - two row tiles - next to the one tile of the rows."""
    import vbr_oracle as vo
    from test_gpu_vbr import CASES
    c = vo.make_case(*CASES[0])
    h_dim, draw = CASES[0][:2]
    base, switched = models(h_dim, seed=bd.seed_of(h_dim, draw), gains=bd.GAINS[draw])
    y, tau, h0 = c.y.to(DEV), c.tau.to(DEV), c.h0[None].to(DEV)
    assert len(c.ladder) * y.shape[0] == 20

    def run(m):
        codes, bits, all_h, extra = m.bvrnn.encode_vbr(y, c.ladder, tau, h0, return_all=True)
        torch.cuda.synchronize()
        return codes, bits, all_h, extra["prob"], extra["dist"], extra["dec"], extra["h_next"]

    want = run(base)
    assert torch.equal(want[1].cpu().double(), c.o64["bits"])                       # (the case's own answer: test_gpu_vbr.py)
    for v, m in switched.items():
        same(run(m), want, f"BVC_MTW={v} encode_vbr")


def test_streaming_session_of_40_slots(monkeypatch):
    """A send session and a receive session of 40 slots (3 row tiles) on launch-per-layer ticks: the packets and the waveform of the
    default model's sessions."""
    import gpu_sessions as gs
    from bvcodec import synth
    monkeypatch.setenv("BVC_STREAM_FLOW", "0")
    B, hop, ticks = 40, 441, 8
    base, switched = models(128)
    x = synth.synthetic_speech(B, hop * ticks, seed=B, kind="speech").to(DEV)
    rates = [gs.RATES[b % 4] for b in range(B)]

    def session(m):
        s = gs.drive_sender(m, "send", x, hop, rates)
        F = s.first.shape[1]
        r = gs.drive_receiver(m, s.first, gs.chunked(F, 2), rates)
        return s.first, s.second, r.wav, r.codes

    want = session(base)
    assert want[0].shape[1] >= 6 and bool(torch.isfinite(want[2]).all()) and float(want[2].abs().max()) > 1e-3
    for v, m in switched.items():
        got = session(m)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (v, i)


# ---------------------------------------------------------------------------------------------- 3: the kernels did run
def test_launch_counts_name_the_variants():
    """Eager models (BVC_NO_GRAPH=1: every launch is a host-side launch, none hides in a replayed graph) at 49 rows = 4 row tiles: a
    call of 3 frames launches the wide kernels and their multi-frame twins and none of the one-tile kernels, and gives the default
    model's bits."""
    from bvcodec import _abi
    lib = _abi.load()
    B, T = 49, 3
    base = make_model(True, 128)[0]
    want = on_schedule(base, "layers", coder_calls(base, B, T, True, 128, 3))
    K = sk.SK_COUNT
    for v, lin in (("2", sk.SK_LIN2), ("4", sk.SK_LIN4)):
        m = make_model(True, 128, env={"BVC_MTW": v, "BVC_NO_GRAPH": "1"})[0]
        before = sk.counts(lib)
        got = on_schedule(m, "layers", coder_calls(m, B, T, True, 128, 3))
        d = sk.counts(lib) - before
        print(f"BVC_MTW={v}:", {("frames " if f else "") + sk.NAMES[k]: int(d[f, k]) for f in (0, 1) for k in range(K) if d[f, k]}, flush=True)
        same(got, want, f"BVC_MTW={v} eager")
        assert d[0, lin] >= 2 * T and d[1, lin] >= 4 and d[0, sk.SK_GRU_IL2] >= 2 * T, d      # a GRU launch per frame of encode and of decode
        others = [k for k in range(K) if k not in (lin, sk.SK_GRU_IL2)]
        assert not d[:, others].any() and not d[1, sk.SK_GRU_IL2], d
    # a clamped launch is counted as what it is: 5 rows are one tile, whatever the model asks for
    m = make_model(True, 128, env={"BVC_MTW": "4", "BVC_NO_GRAPH": "1"})[0]
    before = sk.counts(lib)
    on_schedule(m, "layers", coder_calls(m, 5, T, True, 128, 3))
    d = sk.counts(lib) - before
    assert d[0, sk.SK_LIN] > 0 and d[1, sk.SK_LIN] > 0 and d[0, sk.SK_GRU_IL] >= 2 * T and not d[:, [sk.SK_LIN2, sk.SK_LIN4, sk.SK_GRU_IL2]].any(), d


# ---------------------------------------------------------------------------------------------- 4: BVC_LATENCY=1
def test_latency_switch_in_a_child_process(tmp_path):
    import skinny_latency_job as job
    from bvcodec import _abi
    assert os.environ.get("BVC_LATENCY") is None
    env = dict(os.environ, BVC_LATENCY="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "skinny_latency_job.py"), str(tmp_path)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]          # (nothing below runs after a child that failed)
    lines = dict((ln.split()[0], [int(n) for n in ln.split()[1:]]) for ln in r.stdout.splitlines() if ln.startswith("SK_LIN"))
    print(lines, flush=True)
    assert lines["SK_LIN_LATENCY"][0] > 0 and lines["SK_LIN_LATENCY"][1] > 0 and lines["SK_LIN"] == [0, 0], lines
    ours, delta = job.run()
    assert delta[0, sk.SK_LIN] > 0 and not delta[:, sk.SK_LIN_LATENCY].any() and not sk.counts(_abi.load())[:, sk.SK_LIN_LATENCY].any()
    names = sorted(f[:-4] for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert names == sorted(ours) and len(names) == 2 * len(job.LINEAR_SHAPES) + 5 * len(job.MODEL_SHAPES)
    for name in names:
        theirs = np.load(os.path.join(tmp_path, name + ".npy"))
        assert theirs.shape == ours[name].shape and np.isfinite(theirs).all(), name
        assert np.array_equal(theirs, ours[name]), (name, float(np.abs(theirs - ours[name]).max()))
