"""Throughput on a corpus of utterances of different lengths (mixed-length batches) against two baselines at the same audio.

    python tools/ragged_bench.py [--items 256] [--min-s 1] [--max-s 10] [--bitrate 3000] [--max-batch 64] [--legs many,loop,equal]

  many   encode_many + decode_many: sorted by length, mixed-length calls of at most --max-batch rows
  loop   one encode / decode call per utterance (B = 1)
  equal  equal-length batches of --max-batch rows at the corpus' mean length, the same total audio

One JSON line per leg: audio seconds coded (encode + decode) per wall second.  Each leg can run as its own process
(--legs many, ...), so a job script can give every GPU step a time limit of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bvcodec import synth  # noqa: E402
from gpu_common import make_model  # noqa: E402


def timed(fn, reps):
    fn()                                           # warm: workspaces, graphs of the launch-per-layer schedule
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--bitrate", type=float, default=3000)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-items", type=int, default=0, help="utterances the per-utterance loop times (0: all)")
    ap.add_argument("--legs", default="many,loop,equal")
    args = ap.parse_args()
    fs = 22050
    dev = torch.device("cuda:0")
    model = make_model(True, 1024)[0]
    rng = np.random.default_rng(0)
    lens = rng.integers(int(args.min_s * fs), int(args.max_s * fs) + 1, size=args.items).tolist()
    waves = [synth.synthetic_speech(1, n, seed=i, kind="speech")[0].to(dev) for i, n in enumerate(lens)]
    audio = sum(lens) / fs
    base = {"items": args.items, "seconds": [args.min_s, args.max_s], "bitrate": args.bitrate, "max_batch": args.max_batch}

    def report(leg, secs, wall, **kw):
        print(json.dumps(dict(base, leg=leg, audio_s=round(secs, 2), wall_s=round(wall, 4),
                              audio_s_per_s=round(secs / wall, 1), **kw)), flush=True)

    for leg in args.legs.split(","):
        if leg == "many":
            def run():
                codes = model.encode_many(waves, args.bitrate, max_batch=args.max_batch)
                model.decode_many(codes, lens, max_batch=args.max_batch)
            report(leg, audio, timed(run, args.reps))
        elif leg == "loop":
            k = args.loop_items or args.items

            def run():
                for w in waves[:k]:
                    model.decode(model.encode(w[None], args.bitrate), w.shape[0])
            report(leg, sum(lens[:k]) / fs, timed(run, 1), timed_items=k)
        elif leg == "equal":
            n = int(round(np.mean(lens)))
            nb = max(1, int(round(args.items / args.max_batch)))
            x = synth.synthetic_speech(args.max_batch, n, seed=1, kind="speech").to(dev)

            def run():
                for _ in range(nb):
                    model.decode(model.encode(x, args.bitrate), n)
            report(leg, nb * args.max_batch * n / fs, timed(run, args.reps), batches=nb, length=n)
        else:
            raise SystemExit(f"unknown leg {leg}")
    model.check_status()


if __name__ == "__main__":
    main()
