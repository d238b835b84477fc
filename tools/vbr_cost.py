#!/usr/bin/env python3
"""What closed-loop rate selection costs on the chip, at 64 x 5 s (profiles/vbr_cost.md): ``BVRNN.encode_vbr`` with K = 1, 2, 4 and 8
rungs against ``BVRNN.encode`` on the launch-per-layer schedule with ``encode_fold = 0`` - the same layer list, K = 1 gives its bits -
and against the default ``BVRNN.encode`` (the persistent kernel, folded hop), all on the same mel, state and build.  A call is timed
with a HIP event pair around it: 3 warm-ups, median of 5.  A second pass with the in-kernel stamps of the replayed step
(bvc_kprobe_enable) says where a frame's time goes, layer group by layer group: the span from the first workgroup's start to the last
one's end, mean over the frames.  Stamping slows the kernels down, so that pass is timed on its own and its groups are to be read
against its own time per frame, not against the first pass's.

    python tools/vbr_cost.py [--batch 64] [--frames 430] [--out profiles/vbr_cost.md]
"""
import argparse
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from bvcodec import BVRNNCodecModel, _abi, config, synth       # noqa: E402

DEV = "cuda:0"
LADDERS = {1: (64,), 2: (35, 64), 4: (8, 17, 35, 64), 8: (8, 16, 24, 32, 40, 48, 56, 64)}
GROUPS = (("enc.0-4", 0, 3), ("phi_z.0-4", 3, 6), ("dec.0-6", 6, 10), ("phi_x.0-4", 10, 13), ("GRU", 13, 14))     # kernels of the unfolded step


def timed(fn, warm=3, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def stamps(lib, fn):
    """Mean span in us of every layer group over the frames of one call, from the in-kernel stamps, and that call's own ms."""
    _abi.check(lib.bvc_kprobe_enable(1))
    try:
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out = []
        for _, lo, hi in GROUPS:
            mean, mn, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
            _abi.check(lib.bvc_kprobe_read(lo, hi, ctypes.byref(mean), ctypes.byref(mn), ctypes.byref(n)))
            out.append(mean.value * (hi - lo))          # the group's kernels, one after the other
    finally:
        _abi.check(lib.bvc_kprobe_enable(0))
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbr_cost.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_vbr_cost_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    eng = model.engine()
    lib = eng.lib
    B, T, H = a.batch, a.frames, conf["h_dim"]
    rng = np.random.default_rng(0)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32)).to(DEV)
    h0 = torch.zeros(1, B, H, device=DEV)
    bits = torch.full((B, T), 35.0, device=DEV)

    rows = []
    rows.append(("encode, default schedule", timed(lambda: model.bvrnn.encode(y, bits, h0)), None, None))
    model.set_recurrence("layers")
    eng.set_option("encode_fold", 0)
    try:
        plain = lambda: model.bvrnn.encode(y, bits, h0)
        rows.append(("encode, layers, encode_fold = 0", timed(plain), stamps(lib, plain), None))
        # a target in the middle of what the rungs reach on this input, so that the ladder is in use
        _, _, _, ex = model.bvrnn.encode_vbr(y, LADDERS[8], float("nan"), h0, return_all=True)
        tau = float(ex["dist"].median())
        for K, ladder in LADDERS.items():
            fn = lambda: model.bvrnn.encode_vbr(y, ladder, tau, h0)
            mean_bits = float(fn()[1].mean())
            rows.append((f"encode_vbr, K = {K} {ladder}", timed(fn), stamps(lib, fn), mean_bits))
    finally:
        eng.set_option("encode_fold", 1)
        model.set_recurrence("auto")
    model.check_status()

    base = rows[1][1][0]
    lines = [f"# Closed-loop rate selection: cost at {B} x {T} frames ({T * 256 / 22050:.1f} s of audio per row)", "",
             "`tools/vbr_cost.py`: the mel coder alone (`BVRNN.encode` / `BVRNN.encode_vbr`), HIP events around a call, 3 warm-ups, median "
             "of 5 (min - max); per-frame spans of the layer groups from the in-kernel stamps of the replayed step.", "",
             "| call | ms per call | against layers, fold 0 | us per frame | mean bits | stamped pass: us per frame | " + " | ".join(g[0] for g in GROUPS) + " | rest |",
             "|---|---|---|---|---|---|" + "---|" * (len(GROUPS) + 1)]
    for name, (med, lo, hi), st, mb in rows:
        per = med * 1e3 / T
        cells = ["-"] * (len(GROUPS) + 2) if st is None else [f"{st[1] * 1e3 / T:.1f}"] + [f"{v:.1f}" for v in st[0]] + [f"{st[1] * 1e3 / T - sum(st[0]):.1f}"]
        lines.append(f"| {name} | {med:.2f} ({lo:.2f} - {hi:.2f}) | {med / base:.2f} x | {per:.1f} | {'-' if mb is None else f'{mb:.1f}'} | " + " | ".join(cells) + " |")
    lines += ["", "The layer groups and `rest` are us per frame of the stamped pass.  `rest` is what the stamped kernels do not cover: the gaps between the kernels of a replayed frame, the step-advance kernel, "
              "for encode_vbr the candidate and select kernels, and the all-frame phi_x prologue's share of a frame.", ""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
