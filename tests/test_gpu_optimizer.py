"""The optimiser on the device (csrc/optimizer.hip, csrc/k_optimizer.hip, bvcodec/optim.py): bvc_bvrnn_params_get / _set and
bvc_optimizer_step on live models.

The invariant everything hangs on: after any sequence of params_set and step calls the model is BIT FOR BIT the model bvc_model_create
builds from the exported parameters, on every entry point of the mel coder and on every schedule - a replayed step graph and a
captured call included.  It is checked against models built the ordinary way (gpu_common.make_model, or a checkpoint written from the
exported values), so a derived form that is not rewritten - the fragment-packed or gate-interleaved copies, the float64 fold
px0_dec3, the transposed copies of the backward pass - shows as differing bits.  The arithmetic of the step is held to the float64
oracle (tests/optimizer_oracle.py) at the project's bar, max|hip - g64| <= 8 x max(e32, 2^-24 max|g64|), e32 the float32 oracle's
error.  Measured ratios and the loss curve: profiles/optimizer_parity.md.  Needs the MI355X: run with ``-m gpu``.

The models this file changes are its own copies (``own_model``): the suite's shared ones (make_model's cache) are only read."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

import backward_oracle as bo
import bvrnn_draws as bd
import optimizer_oracle as oo
from gpu_common import DEV, make_model, on_schedule

pytestmark = pytest.mark.gpu

LEDGER = bd.Ledger("optimizer")
SCHEDULES = ("persistent", "layers")
B_, T_ = 3, 5


def own_model(h_dim, tag):
    """A model of this file's own with the default draw's values (seed 1234, so mean_mel / std_mel are the shared models'), cached
    under a key nobody else uses: the environment entry is read by nobody, it only makes the key."""
    model, _, sd, _ = make_model(h_dim=h_dim, env={"BVC_TEST_OWN_COPY": f"optimizer-{tag}"})
    return model, sd


def built_model(h_dim, draw):
    model, _, sd, _ = make_model(h_dim=h_dim, gains=bd.GAINS[draw])
    return model, sd


def rebuild(h_dim, params):
    """Today's way: a new model from a checkpoint that holds the exported parameters (bvc_model_create packs and folds on the host)."""
    from bvcodec import BVRNNCodecModel, config, synth
    conf = bd.conf_of(h_dim)
    d = tempfile.mkdtemp(prefix="bvc_test_opt_")
    txt = open(config.DEFAULT_CONFIG).read()
    assert txt.count("h_dim = 1024") == 1
    cfg_path = os.path.join(d, "cfg.toml")
    with open(cfg_path, "w") as f:
        f.write(txt.replace("h_dim = 1024", f"h_dim = {h_dim}"))
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    sd = dict(synth.bvrnn_state_dict(conf, 1234))
    sd.update({k: v.detach().cpu().clone() for k, v in params.items()})
    torch.save({"vrnn": sd}, p1)
    return BVRNNCodecModel(cfg_path, p1, p2).to(DEV)


def trainable(sd):
    return {k: sd[k] for k in bo.trainable(sd)}


def flat_of(model, named):
    layout, total = model.bvrnn.grad_layout()
    flat = torch.empty(total)
    for name, off, numel in layout:
        flat[off:off + numel] = named[name].reshape(-1)
    return flat


def folded_hop(model):
    from bvcodec import _abi
    eng, H = model.bvrnn.engine(), model.bvrnn.h_dim
    w, b = torch.empty(H, H, device=DEV), torch.empty(H, device=DEV)
    eng.call("bvc_test_folded_hop", eng.handle, _abi.ptr(w), _abi.ptr(b))
    torch.cuda.synchronize()
    return w.cpu(), b.cpu()


# ================================================================================================ 1. round trip
@pytest.mark.parametrize("h_dim", (64, 128, 192, 1024))
def test_params_round_trip(h_dim):
    """params_get is the state dict the model was built from, exactly; after params_set of the wide draw it is that draw, exactly.
    192: no persistent kernel; 1024: the grids' cut across 23.5 M elements, every tensor seam crossed."""
    model, sd = own_model(h_dim, "roundtrip")
    eng = model.bvrnn.engine()
    layout, total = model.bvrnn.grad_layout()
    assert all(off % 16 == 0 and numel % 16 == 0 for _, off, numel in layout)
    canary = torch.full((total + 64,), 777.0, device=DEV)
    eng.call("bvc_bvrnn_params_get", eng.handle, ctypes.c_void_p(canary.data_ptr()))
    torch.cuda.synchronize()
    assert bool((canary[total:] == 777.0).all()), "params_get wrote behind the buffer"
    assert torch.equal(canary[:total].cpu(), flat_of(model, trainable(sd)))
    wide = trainable(bd.state_dict(h_dim, "wide"))
    eng.params_set(flat_of(model, wide).to(DEV))
    got = eng.params_get(total).cpu()
    assert torch.equal(got, flat_of(model, wide))
    model.bvrnn._tensors.stale = eng
    live = model.bvrnn.grad_parameters()                                   # the Python-side copies follow
    assert set(live) == set(wide) and all(torch.equal(live[k], wide[k]) for k in wide)
    model.bvrnn.load_parameters({"enc.2.bias": sd["enc.2.bias"]})          # a subset
    live = model.bvrnn.grad_parameters()
    assert torch.equal(live["enc.2.bias"], sd["enc.2.bias"]) and torch.equal(live["enc.2.weight"], wide["enc.2.weight"])


# ================================================================================================ 2. in place equals rebuilt
def coder_calls(model, y, bits, codes, lost, r, noise):
    """name -> fn() -> tensors, the mel coder's entry points on the inputs of the case"""
    h0 = torch.zeros(1, y.shape[0], model.bvrnn.h_dim, device=DEV)
    length = 256 * y.shape[1]

    def forward():
        dec, kld, ex = model.bvrnn.forward(y, 0.5, False, bits, r=r, noise=noise, return_all=True)
        return [dec, kld, ex["z"], ex["prob"], ex["prior"], ex["kld_frames"]]
    return {"encode": lambda: list(model.bvrnn.encode(y, bits, h0)),
            "decode": lambda: list(model.bvrnn.decode(codes, h0)),
            "forward": forward,
            "decode_lost": lambda: list(model.decode(codes, length, lost=lost, bitrate=3000, return_codes=True))}


def run_backward(model, y, bits, r, noise, gdec):
    g = model.bvrnn.backward(y, 0.5, False, bits, gdec, 0.7, r=r, noise=noise, grad_input=True)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("order", ("backward_before", "backward_late"))
@pytest.mark.parametrize("h_dim", (64, 128, 192, 1024))
def test_in_place_equals_rebuilt(h_dim, order):
    """Model A (default draw) gets the wide draw's values in place; model B is built from the wide draw.  Every output of encode,
    decode, forward(return_all), decode(lost=) and every gradient of backward is torch.equal, on the persistent and the
    launch-per-layer schedule; A has run every call BEFORE the update, so the layer schedule replays its captured step graphs on the
    new weights, and a whole encode call captured before the update is replayed after it.  backward_before: A's transposed copies
    exist and are rewritten; backward_late: A's first backward comes after the update and builds them then.  The folded hop is
    compared directly as well: it decides every bit of a persistent decode."""
    A, sd_a = own_model(h_dim, order)
    Bm, sd_b = built_model(h_dim, "wide")
    assert all(torch.equal(sd_a[k], sd_b[k]) for k in ("mean_mel", "std_mel"))
    if bd.flow_supported(h_dim, 64):
        assert A.engine().get_option("flow_supported") == 1
    y, bits = (t.to(DEV) for t in bd.inputs(B_, T_))
    rng = np.random.default_rng(h_dim)
    r = torch.from_numpy(rng.random(T_).astype(np.float32))
    noise = torch.from_numpy(rng.random((B_, T_, 64)).astype(np.float32))
    gdec = torch.from_numpy(rng.standard_normal((B_, T_, 80)).astype(np.float32)).to(DEV)
    lost = torch.zeros(B_, T_, dtype=torch.bool)
    lost[0, 1], lost[2, 3:] = True, True
    codes = Bm.bvrnn.encode(y, bits, torch.zeros(1, B_, h_dim, device=DEV))[0].clone()
    calls_a, calls_b = coder_calls(A, y, bits, codes, lost, r, noise), coder_calls(Bm, y, bits, codes, lost, r, noise)

    before = {(s, n): on_schedule(A, s, fn) for s in SCHEDULES for n, fn in calls_a.items()}
    if order == "backward_before":
        run_backward(A, y, bits, r, noise, gdec)
    # a whole call captured before the update
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        calls_a["encode"]()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        captured = calls_a["encode"]()
    torch.cuda.synchronize()

    A.bvrnn.load_parameters(trainable(sd_b))
    torch.cuda.synchronize()

    wa, ba = folded_hop(A)
    wb, bb = folded_hop(Bm)
    assert torch.equal(ba, bb), f"folded bias: {int((ba != bb).sum())} of {ba.numel()} differ, max {float((ba - bb).abs().max()):.3e}"
    assert torch.equal(wa, wb), f"folded weight: {int((wa != wb).sum())} of {wa.numel()} differ, max {float((wa - wb).abs().max()):.3e}"
    changed = 0
    for s in SCHEDULES:
        for n in calls_a:
            got, want = on_schedule(A, s, calls_a[n]), on_schedule(Bm, s, calls_b[n])
            for i, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), f"{n} output {i} on {s}: {int((g != w).sum())} of {g.numel()} elements differ"
            changed += any(not torch.equal(g, b) for g, b in zip(got, before[(s, n)]))
    assert changed == len(SCHEDULES) * len(calls_a), "the update left some call's outputs as they were"
    for o in captured:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(captured, on_schedule(Bm, "graph", calls_b["encode"])):
        assert torch.equal(g, w), "a call captured before the update, replayed after it"
    ga, gb = run_backward(A, y, bits, r, noise, gdec), run_backward(Bm, y, bits, r, noise, gdec)
    assert set(ga) == set(gb)
    for k in gb:
        assert torch.equal(ga[k], gb[k]), f"backward {k}: {int((ga[k] != gb[k]).sum())} of {gb[k].numel()} elements differ"
    A.check_status()


# ================================================================================================ 3. Adam arithmetic
def held(got, o64, o32, what, family):
    bad = []
    for k in o64:
        v = bd.compare(got[k].detach().cpu().double().reshape(1, -1).numpy(), o64[k].reshape(1, -1), o32[k].astype(np.float64).reshape(1, -1),
                       f"{what} {k}")
        LEDGER.add(family, v)
        if not v.ok:
            bad.append(v.message)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("weight_decay,max_grad_norm", ((0.0, 0.0), (0.1, 1.0)))
@pytest.mark.parametrize("h_dim", (64, 128))
def test_adam_arithmetic_against_float64_oracle(h_dim, weight_decay, max_grad_norm):
    """Synthetic gradients straight into step (magnitudes over fourteen decades, a tensor of zeros, a tensor with one element), lr 0.05
    so that an update is a visible share of the weights; after 1, 2 and 5 steps every tensor of the parameters and of both moments
    against the float64 oracle at the project's bar.  The returned norm to 1e-6; a second optimiser fed the same sequence gives the
    same bits; without decay the all-zero tensor's parameters do not move."""
    models = [own_model(h_dim, t)[0] for t in ("adam", "adam2")]
    _, sd = own_model(h_dim, "adam")
    start = trainable(sd)
    hyper = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    opts = []
    for m in models:
        m.bvrnn.load_parameters(start)
        opts.append(m.bvrnn.optimizer(**hyper))
    o64, o32 = oo.AdamWOracle(start, np.float64), oo.AdamWOracle(start, np.float32)
    shapes = {k: tuple(v.shape) for k, v in start.items()}
    what = f"h{h_dim} wd={weight_decay} clip={max_grad_norm}"
    for step in range(1, 6):
        g = oo.synthetic_grads(shapes, 100 + step)
        n64 = o64.step(g, **hyper)
        o32.step(g, **hyper)
        norm = opts[0].step(dict(g, y=torch.zeros(1)))                     # as backward(grad_input=True) returns them: "y" is not a parameter
        norm2 = opts[1].step(flat_of(models[1], g).to(DEV))                # the flat form of the same gradients
        assert norm.device.type == "cuda" and norm.dim() == 0 and torch.equal(norm, norm2)
        assert abs(float(norm) - n64) <= 1e-6 * n64, (float(norm), n64)
        if step in (1, 2, 5):
            p, st = models[0].bvrnn.grad_parameters(), opts[0].state_dict()
            assert st["step"] == step
            held(p, o64.p, o32.p, f"{what} step {step} param", "param")
            held({k: s["exp_avg"] for k, s in st["state"].items()}, o64.m, o32.m, f"{what} step {step} exp_avg", "exp_avg")
            held({k: s["exp_avg_sq"] for k, s in st["state"].items()}, o64.v, o32.v, f"{what} step {step} exp_avg_sq", "exp_avg_sq")
            if weight_decay == 0:
                assert torch.equal(p[oo.ZERO_TENSOR], start[oo.ZERO_TENSOR])
            moved = max(float((p[k] - start[k]).abs().max()) for k in p)
            assert moved >= 0.04, moved
    p2, st2 = models[1].bvrnn.grad_parameters(), opts[1].state_dict()
    assert all(torch.equal(p[k], p2[k]) for k in p)
    assert all(torch.equal(st["state"][k][m], st2["state"][k][m]) for k in p for m in ("exp_avg", "exp_avg_sq"))


def test_step_refusals():
    from bvcodec import _abi
    model, sd = own_model(64, "adam")
    opt = model.bvrnn.optimizer()
    eng = opt._engine()
    flat = torch.zeros(model.bvrnn.grad_layout()[1], device=DEV)
    before = eng.params_get(flat.numel()).clone()
    for bad in ((-1.0, 0.9, 0.999, 1e-8, 0.0, 0.0), (1e-3, 1.0, 0.999, 1e-8, 0.0, 0.0), (1e-3, 0.9, -0.5, 1e-8, 0.0, 0.0),
                (1e-3, 0.9, 0.999, 0.0, 0.0, 0.0), (float("nan"), 0.9, 0.999, 1e-8, 0.0, 0.0)):
        cfg = _abi.BvcAdamWConfig(*bad)
        assert eng.lib.bvc_optimizer_step(opt._handle, ctypes.byref(cfg), _abi.ptr(flat), None, eng.stream()) == -1, bad
    cfg = _abi.BvcAdamWConfig(1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    assert eng.lib.bvc_optimizer_step(opt._handle, None, _abi.ptr(flat), None, eng.stream()) == -1
    assert eng.lib.bvc_optimizer_step(opt._handle, ctypes.byref(cfg), None, None, eng.stream()) == -1
    assert eng.lib.bvc_optimizer_step(opt._handle, ctypes.byref(cfg), ctypes.c_void_p(flat.data_ptr() + 4), None, eng.stream()) == -1
    assert opt.state_dict()["step"] == 0 and torch.equal(eng.params_get(flat.numel()), before)


# ================================================================================================ 4. state
def test_state_round_trip_and_params_set_between_steps():
    h_dim = 64
    U, sd = own_model(h_dim, "state-u")
    V, _ = own_model(h_dim, "state-v")
    start, wide = trainable(sd), trainable(bd.state_dict(h_dim, "wide"))
    shapes = {k: tuple(v.shape) for k, v in start.items()}
    g = [oo.synthetic_grads(shapes, 200 + i) for i in range(3)]
    hyper = dict(lr=0.01, weight_decay=0.1, max_grad_norm=5.0)
    U.bvrnn.load_parameters(start)
    ou = U.bvrnn.optimizer(**hyper)
    for gi in g:
        ou.step(gi)
    V.bvrnn.load_parameters(start)
    ov = V.bvrnn.optimizer(**hyper)
    ov.step(g[0])
    after_one = ov.state_dict()
    ov.step(g[1])
    state = ov.state_dict()
    assert state["step"] == 2 and set(state["state"]) == set(start)
    assert all(state["state"][k]["exp_avg"].shape == start[k].shape and state["state"][k]["exp_avg"].device.type == "cpu" for k in start)
    W = rebuild(h_dim, V.bvrnn.grad_parameters())
    ow = W.bvrnn.optimizer(**hyper)
    ow.load_state_dict(state)
    ow.step(g[2])
    pu, pw = U.bvrnn.grad_parameters(), W.bvrnn.grad_parameters()
    assert all(torch.equal(pu[k], pw[k]) for k in pu), "interrupted and uninterrupted runs differ"
    su, sw = ou.state_dict(), ow.state_dict()
    assert su["step"] == sw["step"] == 3
    assert all(torch.equal(su["state"][k][m], sw["state"][k][m]) for k in pu for m in ("exp_avg", "exp_avg_sq"))
    # params_set between two steps: the second step starts from the values that were set
    V.bvrnn.load_parameters(start)
    ov.load_state_dict(after_one)
    V.bvrnn.load_parameters(wide)
    ov.step(g[1])
    X = rebuild(h_dim, wide)
    ox = X.bvrnn.optimizer(**hyper)
    ox.load_state_dict(after_one)
    ox.step(g[1])
    pv, px = V.bvrnn.grad_parameters(), X.bvrnn.grad_parameters()
    assert all(torch.equal(pv[k], px[k]) for k in pv)
    assert not torch.equal(pv["dec.0.weight"], pu["dec.0.weight"])


# ================================================================================================ 5. the loop
def test_training_loop_equals_a_new_model_every_iteration():
    """Three iterations of forward, backward(flat=True), step on a live model, against today's way: every iteration a NEW model from
    the exported parameters, its backward, and the same float32 step through an optimiser of that model whose state is carried over.
    Gradients and loss are equal bit for bit at every iteration."""
    h_dim, B, T = 64, 2, 4
    A, sd = own_model(h_dim, "loop")
    A.bvrnn.load_parameters(trainable(sd))
    y, bits = (t.to(DEV) for t in bd.inputs(B, T, seed=9))
    rng = np.random.default_rng(3)
    r = torch.from_numpy(rng.random(T).astype(np.float32))
    noise = torch.from_numpy(rng.random((B, T, 64)).astype(np.float32))
    hyper = dict(lr=0.01, weight_decay=0.01, max_grad_norm=10.0)

    def iteration(model, opt):
        dec, kld = model.bvrnn.forward(y, 0.5, False, bits, r=r, noise=noise)
        loss = 0.5 * (dec - y).pow(2).sum() + 0.1 * kld
        flat = model.bvrnn.backward(y, 0.5, False, bits, dec - y, 0.1, r=r, noise=noise, flat=True)
        opt.step(flat)
        return loss.clone(), flat.clone()

    oa = A.bvrnn.optimizer(**hyper)
    params, state, losses = trainable(sd), None, []
    for it in range(3):
        la, ga = iteration(A, oa)
        M = rebuild(h_dim, params)
        om = M.bvrnn.optimizer(**hyper)
        if state is not None:
            om.load_state_dict(state)
        lm, gm = iteration(M, om)
        assert torch.equal(ga, gm), f"iteration {it}: {int((ga != gm).sum())} gradient elements differ"
        assert torch.equal(la, lm), (it, float(la), float(lm))
        params, state = M.bvrnn.grad_parameters(), om.state_dict()
        live = A.bvrnn.grad_parameters()
        assert all(torch.equal(live[k], params[k]) for k in params)
        losses.append(float(la))
    assert len(set(losses)) == 3, losses


# ================================================================================================ 6. forward_train round
def test_forward_train_round():
    h_dim, B, T = 64, 2, 4
    A, sd = own_model(h_dim, "autograd")
    A.bvrnn.load_parameters(trainable(sd))
    y, bits = bd.inputs(B, T, seed=10)
    r = torch.tensor([0.9, 0.1, 0.7, 0.2])
    params = {k: v.requires_grad_(True) for k, v in A.bvrnn.grad_parameters().items()}
    opt = A.bvrnn.optimizer(lr=0.01)
    dec, kld = A.bvrnn.forward_train(y, 0.5, True, bits, params, r=r)
    ((dec - y).pow(2).mean() + 0.1 * kld).backward()
    assert all(p.grad is not None for p in params.values())
    first = dec.detach().clone()
    norm = opt.step({n: p.grad for n, p in params.items()}, params=params)
    want = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in params.values()))
    assert abs(float(norm) - float(want)) <= 1e-6 * float(want)
    live = A.bvrnn.grad_parameters()
    assert all(p.requires_grad and p.is_leaf and torch.equal(p.detach(), live[n]) for n, p in params.items())
    assert not torch.equal(live["dec.6.bias"], sd["dec.6.bias"])
    dec2, kld2 = A.bvrnn.forward_train(y, 0.5, True, bits, params, r=r)
    fdec, fkld = A.bvrnn.forward(y, 0.5, True, bits, r=r)
    assert torch.equal(dec2.detach(), fdec) and torch.equal(kld2.detach(), fkld) and not torch.equal(fdec, first)


# ================================================================================================ 7. it learns
def test_it_learns():
    """The fixed batch, learning rate and loss of optimizer_oracle (set on the CPU at float64, where the loss falls by a factor of
    6.96 and LEARN_FALL = 5 is asserted): the library's loop falls by at least half of that in log terms."""
    A, sd = own_model(oo.LEARN_H, "learn")
    A.bvrnn.load_parameters(trainable(sd))
    y, bits, r = oo.learn_batch()
    y, bits = y.to(DEV), bits.to(DEV)
    opt = A.bvrnn.optimizer(lr=oo.LEARN_LR, weight_decay=0.0)
    curve = []
    for it in range(oo.LEARN_STEPS + 1):
        dec, kld = A.bvrnn.forward(y, 0.0, True, bits, r=r)
        loss, gdec, gkld = oo.learn_loss_and_grads(dec, kld, y)
        curve.append(loss)
        if it < oo.LEARN_STEPS:
            opt.step(A.bvrnn.backward(y, 0.0, True, bits, gdec, gkld, r=r, flat=True))
    print("LEARN curve:", " ".join(f"{v:.4g}" for v in curve), f"fall {curve[0] / curve[-1]:.3f}", flush=True)
    assert all(np.isfinite(curve))
    assert curve[0] / curve[-1] >= np.sqrt(oo.LEARN_FALL), (curve[0], curve[-1])
    A.check_status()


def test_optimizer_parity_ledger():
    """Prints the PARITY lines of the arithmetic comparisons (profiles/optimizer_parity.md)."""
    LEDGER.close()
