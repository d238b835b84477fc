#!/usr/bin/env python3
"""Offline cost of concealment: bvc_decode against bvc_decode_conceal, 64 x 5 s at 3 kbit/s on one MI355X (profiles/conceal_cost.md).
Prints one JSON line: ms per call (median of --reps calls after --warmup) for the plain decode and for the concealing decode at
0 % and 5 % loss, and for the two recurrences alone (bvc_bvrnn_decode / bvc_bvrnn_decode_conceal)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, torch
from gpu_common import make_model
from bvcodec import synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


B, L = arg("--batch", 64), int(22050 * 5.0)
reps, warmup = arg("--reps", 20), arg("--warmup", 3)
model = make_model()[0]
dev = "cuda:0"
x = synth.synthetic_speech(B, L, seed=11, kind="noise").to(dev)
codes = model.encode(x, 3000)
T = codes.shape[1]
g = torch.Generator().manual_seed(11)
lost0 = torch.zeros(B, T, dtype=torch.bool, device=dev)
lost5 = (torch.rand(B, T, generator=g) < 0.05).to(dev)
bits = torch.full((B, T), model.bits_per_frame(3000), device=dev)
h0 = torch.zeros(1, B, model.conf["h_dim"], device=dev)
res = {"config": f"{B} x 5 s @ 3 kbit/s ({T} frames), ms per call (median of {reps})",
       "decode": timed(lambda: model.decode(codes, L), reps, warmup),
       "decode_conceal_loss0": timed(lambda: model.decode(codes, L, lost=lost0, bitrate=3000), reps, warmup),
       "decode_conceal_loss5": timed(lambda: model.decode(codes, L, lost=lost5, bitrate=3000), reps, warmup),
       "bvrnn_decode": timed(lambda: model.bvrnn.decode(codes, h0), reps, warmup),
       "bvrnn_decode_conceal_loss5": timed(lambda: model.bvrnn.decode(codes, h0, present=~lost5, bits=bits), reps, warmup)}
res["per_frame_us"] = {"bvrnn_decode": round(res["bvrnn_decode"] * 1e3 / T, 2),
                       "bvrnn_decode_conceal": round(res["bvrnn_decode_conceal_loss5"] * 1e3 / T, 2)}
model.check_status()
print(json.dumps(res))
