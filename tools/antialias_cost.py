#!/usr/bin/env python3
"""What anti-aliased activations cost on the chip, at 64 x 5 s (profiles/antialias_cost.md):

* per stage, the filtered AMP-pair launch against the plain launch of the same shape - bvc_test_vocoder_layer, one launch per
  call, timed by the library's in-situ family timer (bvc_probe_begin kind 3: an event pair around the launch on its own stream),
  mean over the stage's nine (ks, d) pairs; the filtered conv_post against the plain one (kind 6);
* whole-call decode(codes, 110250) of the shipped configuration and of the two filtered ones (host clock around a synchronised call).

    python tools/antialias_cost.py [--batch 64] [--frames 430] [--reps 5]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402
import torch                # noqa: E402

import vocoder_layers as vl                                     # noqa: E402
from bvcodec import BVRNNCodecModel, _abi, synth                # noqa: E402

DEV = "cuda:0"
PK_CONV, PK_POST = 3, 6


def make(directory, tag, switches):
    cfg = os.path.join(directory, f"{tag}.toml")
    conf = vl.write_config(cfg, switches=switches)
    p1, p2 = os.path.join(directory, "bvrnn"), os.path.join(directory, f"bigvgan_{tag}")
    if not os.path.exists(p1):
        torch.save({"vrnn": synth.bvrnn_state_dict(conf, 1234)}, p1)
    torch.save({"generator": synth.generator_state_dict(conf, 1235)}, p2)
    model = BVRNNCodecModel(cfg, p1, p2).to(DEV)
    return model, model.engine(torch.empty(0, device=DEV)), conf


def probe(lib, kind, fn, reps):
    fn()                                                        # warm: code object, attributes
    torch.cuda.synchronize()
    _abi.check(lib.bvc_probe_begin(kind, 1, reps))
    for _ in range(reps):
        fn()
    mean, mn, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
    _abi.check(lib.bvc_probe_end(ctypes.byref(mean), ctypes.byref(mn), ctypes.byref(n)))
    assert n.value == reps, n.value
    return mean.value, mn.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _abi.load()
    d = tempfile.mkdtemp(prefix="bvc_aa_cost_")
    models = {"plain": make(d, "plain", None)}
    for tag, sw in vl.AA_CONFIGS.items():
        models[tag] = make(d, tag, sw)
    B, T = a.batch, a.frames
    rng = np.random.default_rng(0)
    info = (ctypes.c_int64 * 5)()

    print(f"per launch, B = {B}, {T} frames; us = mean (min) of {a.reps} launches per pair, nine pairs per stage")
    L = T
    for stage in range(4):
        L = (L + 1) * (8, 8, 2, 2)[stage]
        C = 64 >> stage
        x = torch.from_numpy(rng.standard_normal((B, L, C)).astype(np.float32)).to(DEV)
        out = torch.empty_like(x)
        row = {}
        for tag in ("plain", "all"):
            eng = models[tag][1]
            tot, tiles = [], None
            for block in range(3):
                for it in range(3):
                    def fn():
                        _abi.check(lib.bvc_test_vocoder_layer(eng.handle, 2, stage, block, it, _abi.ptr(x), B, L, _abi.ptr(out), 1, None, 0, 0, 0,
                                                              0, 1.0, info, eng.stream()))
                    tot.append(probe(lib, PK_CONV, fn, a.reps))
                    tiles = (info[2], info[3], info[4])
            row[tag] = (float(np.mean([t[0] for t in tot])), float(np.mean([t[1] for t in tot])), [round(t[0], 1) for t in tot], tiles)
        p, f = row["plain"], row["all"]
        print(f"stage {stage} C={C} L={L}: plain {p[0]:.1f} ({p[1]:.1f}) us, filtered {f[0]:.1f} ({f[1]:.1f}) us, ratio {f[0] / p[0]:.2f}")
        print(f"   plain per pair {p[2]} last cut {p[3]}")
        print(f"   filtered per pair {f[2]} last cut {f[3]}", flush=True)
        del x, out
    x = torch.from_numpy(rng.standard_normal((B, L, 8)).astype(np.float32)).to(DEV)
    out = torch.empty(B, L, device=DEV)
    for tag in ("plain", "all"):
        eng = models[tag][1]

        def fn():
            _abi.check(lib.bvc_test_vocoder_layer(eng.handle, 3, 0, 0, 0, _abi.ptr(x), B, L, _abi.ptr(out), 1, None, 0, 0, 0, L, 1.0, info, eng.stream()))
        m, mn = probe(lib, PK_POST, fn, a.reps)
        print(f"conv_post L={L} {tag}: {m:.1f} ({mn:.1f}) us", flush=True)
    del x, out

    codes = torch.from_numpy(rng.integers(0, 2, size=(B, T, 64)).astype(np.float32)).to(DEV)
    n = T * 256 + 170
    for tag, (model, eng, conf) in models.items():
        model.decode(codes, n)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps + 2):
            t0 = time.perf_counter()
            model.decode(codes, n)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        model.check_status()
        print(f"decode {B} x {n} samples, {tag}: {np.mean(ts):.2f} ms mean, {min(ts):.2f} min, {max(ts):.2f} max of {len(ts)}", flush=True)


if __name__ == "__main__":
    main()
