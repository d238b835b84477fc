#!/usr/bin/env python3
"""What symmetric layers cost on the chip, at 64 x 430 frames (profiles/symmetric_cost.md): ``model.vocoder`` of the shipped causal
configuration and of the all-symmetric one, warmed, profiler off, timed with device events around each call; medians of the
repetitions, the two configurations alternating.  Per stage, the stage's nine AMP-pair launches (bvc_test_vocoder_layer, one launch
per call, device events around the nine) of both models on the same rows.

    python tools/symmetric_cost.py [--batch 64] [--frames 430] [--reps 21]
"""
import argparse
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402
import torch                # noqa: E402

import vocoder_layers as vl                                     # noqa: E402
from bvcodec import BVRNNCodecModel, _abi, config, synth        # noqa: E402

DEV = "cuda:0"


def make(directory, tag):
    cfg = os.path.join(directory, f"{tag}.toml")
    if tag == "causal":
        with open(cfg, "w") as f:
            f.write(open(config.DEFAULT_CONFIG).read())
        conf = config.load_config(cfg)
    else:
        conf = vl.write_config(cfg, switches=vl.SYM_CONFIGS[tag])
    p1, p2 = os.path.join(directory, "bvrnn"), os.path.join(directory, f"bigvgan_{tag}")
    if not os.path.exists(p1):
        torch.save({"vrnn": synth.bvrnn_state_dict(conf, 1234)}, p1)
    torch.save({"generator": synth.generator_state_dict(conf, 1235)}, p2)
    model = BVRNNCodecModel(cfg, p1, p2).to(DEV)
    return model, model.engine(torch.empty(0, device=DEV)), conf


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _abi.load()
    d = tempfile.mkdtemp(prefix="bvc_sym_cost_")
    models = {tag: make(d, tag) for tag in ("causal", "all")}
    B, T = a.batch, a.frames
    rng = np.random.default_rng(0)
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32)).to(DEV)

    ts = {tag: [] for tag in models}
    for tag, (model, _, _) in models.items():
        for _ in range(3):
            model.vocoder(mel, 10 ** 9)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for tag, (model, _, _) in models.items():
            ts[tag].append(timed(lambda: model.vocoder(mel, 10 ** 9)))
    for tag, (model, eng, conf) in models.items():
        model.check_status()
        v = np.asarray(ts[tag])
        print(f"vocoder {B} x {T} frames -> {eng.vocoder_length(T)} samples, {tag}: median {np.median(v):.2f} ms, min {v.min():.2f}, max {v.max():.2f} "
              f"of {len(v)}", flush=True)

    info = (ctypes.c_int64 * 5)()
    for stage in range(4):
        C = 64 >> stage
        L = config.generator_length(models["all"][2], T, stages=True)[stage]         # the same rows for both models
        x = torch.from_numpy(rng.standard_normal((B, L, C)).astype(np.float32)).to(DEV)
        out = torch.empty_like(x)
        row = {}
        for tag, (model, eng, conf) in models.items():
            def nine():
                for block in range(3):
                    for it in range(3):
                        _abi.check(lib.bvc_test_vocoder_layer(eng.handle, 2, stage, block, it, _abi.ptr(x), B, L, _abi.ptr(out), 1, None, 0, 0, 0,
                                                              0, 1.0, info, eng.stream()))
            nine()
            row[tag] = (float(np.median([timed(nine) for _ in range(a.reps)])), (info[2], info[3], info[4]))
        c, s = row["causal"], row["all"]
        print(f"stage {stage} C={C} L={L}: nine pairs (each launch synchronised) causal {c[0]:.3f} ms last cut {c[1]}, symmetric {s[0]:.3f} ms last cut {s[1]}, "
              f"ratio {s[0] / c[0]:.2f}", flush=True)
        del x, out


if __name__ == "__main__":
    main()
