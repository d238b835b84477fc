#!/usr/bin/env python3
"""What the entropy-coded wire format costs on the chip, at 64 x 430 frames, h 1024, 3 kbit/s (profiles/entropy_cost.md).  One leg per
invocation, so that every GPU step has its own time limit and a chain of them stops at the first that fails:

    timeout -k 10 120 python tools/entropy_bench.py --leg conceal && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg conceal_layers && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg unpack && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg pack && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg decode_conceal && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg decode_conceal_layers && \\
    timeout -k 10 120 python tools/entropy_bench.py --leg decode_entropy

The comparison that matters is `unpack` (bvc_bvrnn_entropy_unpack, always launch-per-layer) against `conceal_layers`
(bvc_bvrnn_decode_conceal with recurrence = 1, every frame present): the difference is the decode node.  Its own time per frame comes
from a kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats -d /tmp/entropy_trace -- python tools/entropy_bench.py --leg unpack --reps 1 --warm 1

A call is timed with a HIP event pair around it: 3 warm-ups, median of 5.  Each leg prints one JSON line; --out appends it to a file.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from bvcodec import BVRNNCodecModel, config, synth       # noqa: E402

DEV = "cuda:0"
LEGS = ("conceal", "conceal_layers", "unpack", "pack", "decode_conceal", "decode_conceal_layers", "decode_entropy")


def timed(fn, warm, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS, required=True)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--segment", type=int, default=None)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_entropy_bench_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    B, T, H = a.batch, a.frames, conf["h_dim"]
    nb = float(model.active_bits(3000))
    rng = np.random.default_rng(0)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32)).to(DEV)
    h0 = torch.zeros(1, B, H, device=DEV)
    bits = torch.full((B, T), nb, device=DEV)
    codes, _ = model.bvrnn.encode(y, bits, h0)
    present = torch.ones(B, T, device=DEV)
    lost = torch.zeros(B, T, dtype=torch.bool, device=DEV)
    data, sizes = model.pack_entropy(codes, bitrate=3000, segment=a.segment)
    n = 256 * T
    layers = a.leg.endswith("_layers")
    fn = {"conceal": lambda: model.bvrnn.decode(codes, h0, present=present, bits=bits),
          "unpack": lambda: model.bvrnn.entropy_unpack(data, sizes, T, bits, h0, segment=a.segment),
          "pack": lambda: model.bvrnn.entropy_pack(codes, bits, h0, segment=a.segment),
          "decode_conceal": lambda: model.decode(codes, n, lost=lost, bitrate=3000),
          "decode_entropy": lambda: model.decode_entropy(data, sizes, T, n, bitrate=3000, segment=a.segment)}[a.leg.replace("_layers", "")]
    model.set_recurrence("layers" if layers else "auto")
    try:
        med, lo, hi = timed(fn, a.warm, a.reps)
    finally:
        model.set_recurrence("auto")
    model.check_status()
    stored = float(sizes.sum()) * 8.0
    res = dict(leg=a.leg, batch=B, frames=T, segment=a.segment, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
               us_per_frame=round(med * 1e3 / T, 2), stored_bits_per_coded_bit=round(stored / (B * T * nb), 4), stride=int(data.shape[2]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
