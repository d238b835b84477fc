"""Helpers shared by the GPU parity tests."""
import os
import tempfile

import numpy as np
import torch

from bvcodec import BVRNNCodecModel, config, synth

_CACHE = {}
DEV = "cuda:0"


def make_model(var_bit=True, h_dim=1024, seed=1234, env=None, mel_stats=None, gains=None, pinned=None, z_dim=None, frontend=None):
    """Product model on cuda:0 with seeded synthetic checkpoints (+ the matching oracle state dicts).
    env: extra environment variables that are read when the engine is created (BVC_NO_GRAPH, ...).
    gains: synth.bvrnn_state_dict's (g_hidden, g_out, g_gru).  pinned: a name of bvrnn_draws.PINNED - that edit of the coder's
    state dict (one layer's weight zeroed, its bias from a table) is what the model and the returned state dict hold.
    z_dim: None = the config's own (64).  frontend: a dict with some of fs, fmin, fmax, mel_pad_left - the front end's keys set to
    these values."""
    gains = None if gains is None else tuple(float(g) for g in gains)
    frontend = {k: v for k, v in (frontend or {}).items() if v is not None}
    assert set(frontend) <= {"fs", "fmin", "fmax", "mel_pad_left"}, frontend
    key = (var_bit, h_dim, seed, tuple(sorted((env or {}).items())), mel_stats, gains, pinned, z_dim, tuple(sorted(frontend.items())))
    if key in _CACHE:
        return _CACHE[key]
    base = config.DEFAULT_CONFIG if var_bit else config.DEFAULT_CONFIG_64BIT
    conf = config.load_config(base)
    d = tempfile.mkdtemp(prefix="bvc_test_")
    cfg_path = base
    z_dim = conf["z_dim"] if z_dim is None else z_dim
    if h_dim != conf["h_dim"] or z_dim != conf["z_dim"] or any(conf[k] != v for k, v in frontend.items()):
        cfg_path = os.path.join(d, "cfg.toml")
        with open(base) as f:
            txt = f.read()
        assert txt.count("h_dim = 1024") == 1 and txt.count("z_dim = 64") == 1
        txt = txt.replace("h_dim = 1024", f"h_dim = {h_dim}").replace("z_dim = 64", f"z_dim = {z_dim}")
        conf["h_dim"], conf["z_dim"] = h_dim, z_dim
        for k, v in frontend.items():
            assert txt.count(f"\n{k} = {conf[k]}\n") == 1, k
            txt = txt.replace(f"\n{k} = {conf[k]}\n", f"\n{k} = {v}\n")
            conf[k] = v
        with open(cfg_path, "w") as f:
            f.write(txt)
    p1, p2 = synth.write_checkpoints(conf, d, seed=seed, mel_stats=mel_stats, gains=gains)
    vr = synth.bvrnn_state_dict(conf, seed, mel_stats, gains)
    if pinned is not None:
        import bvrnn_draws
        vr = bvrnn_draws.PINNED[pinned](vr)
        torch.save({"vrnn": vr}, p1)
    model = BVRNNCodecModel(cfg_path, p1, p2).to("cuda:0")
    if env:                      # the library reads its switches in bvc_model_create: create the engine now
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            model.engine()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    ge = synth.generator_state_dict(conf, seed + 1)
    _CACHE[key] = (model, conf, vr, ge)
    return _CACHE[key]


def report(name, got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    s = (f"{name}: shape {got.shape} max|err| {err.max():.3e} rms err {np.sqrt((err ** 2).mean()):.3e} "
         f"ref rms {np.sqrt((ref ** 2).mean()):.3e} nan {int(np.isnan(got).sum())}")
    print(s, flush=True)
    return err


def on_schedule(model, schedule, fn):
    """fn() on the persistent kernel, on the launch-per-layer kernels, or captured into a graph and replayed."""
    if schedule in ("persistent", "layers"):
        try:
            model.set_recurrence(schedule)
            out = fn()
            torch.cuda.synchronize()
        finally:
            model.set_recurrence("auto")
        return [o.clone() for o in out]
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        fn()                                                   # warm call: this stream's workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        out = fn()
    for o in out:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    return [o.clone() for o in out]
