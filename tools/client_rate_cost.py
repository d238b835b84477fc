#!/usr/bin/env python3
"""What rate conversion at the session boundary costs per tick (profiles/client_rate_cost.md): 256 streams, 20 ms hops; duplex, send
and receive sessions, each plain (twice: the spread of a variant against itself), at 16 kHz and at 48 kHz.  All sessions live in one
process and take turns, a block of ticks each; every variant gets its warm ticks first and then the timed ones, each timed with a
pair of device events around the push and synchronised like a real-time loop's.

    python tools/client_rate_cost.py [--streams 256] [--warm 200] [--ticks 2000] [--block 100] [--out FILE.md]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from bvcodec import BVRNNCodecModel, config, synth        # noqa: E402
from bvcodec.streaming import StreamingCodec              # noqa: E402

DEV = "cuda:0"
FS = 22050


class Variant:
    def __init__(self, model, B, direction, rate, tag, ks):
        self.name = f"{direction} {tag}"
        self.direction, self.rate = direction, rate
        hop = 441 if rate is None else rate // 50
        self.sc = StreamingCodec(model, B, 3000, hop=hop, direction=direction, client_rate=rate)
        g = torch.Generator().manual_seed(3)
        if direction == "recv":
            self.inputs = [torch.randint(0, 256, (B, k, self.sc.bytes_per_frame), generator=g, dtype=torch.uint8).to(DEV) for k in ks]
        else:
            self.inputs = [(0.1 * torch.randn(B, hop, generator=g)).to(DEV) for _ in range(16)]
        self.at, self.ms = 0, []

    def tick(self, timed):
        x = self.inputs[self.at % len(self.inputs)]
        self.at += 1
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if self.direction == "recv":
            self.sc.push_packets(x)
        else:
            self.sc.push(x)
        b.record()
        b.synchronize()
        if timed:
            self.ms.append(a.elapsed_time(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_client_rate_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    # the frame counts of a plain send session's ticks: what a receive session is given
    probe = StreamingCodec(model, 2, 3000, hop=441, direction="send")
    ks = [probe.push(torch.zeros(2, 441, device=DEV))[0].shape[1] for _ in range(64)][8:]
    del probe
    variants = [Variant(model, a.streams, direction, rate, tag, ks)
                for direction in ("duplex", "send", "recv")
                for rate, tag in ((None, "plain"), (None, "plain again"), (16000, "16 kHz"), (48000, "48 kHz"))]
    for v in variants:
        for _ in range(a.warm):
            v.tick(False)
    done = 0
    while done < a.ticks:
        n = min(a.block, a.ticks - done)
        for v in variants:
            for _ in range(n):
                v.tick(True)
        done += n
    torch.cuda.synchronize()
    model.check_status()
    lines = [f"{a.streams} streams, 20 ms hops, {a.warm} warm and {a.ticks} timed ticks per variant in blocks of {a.block}, device events per push.", "",
             "| session | p50 ms | p99 ms | mean ms | p50 - plain p50, us |", "|---|---|---|---|---|"]
    stats = {v.name: (np.percentile(v.ms, 50), np.percentile(v.ms, 99), float(np.mean(v.ms))) for v in variants}
    for v in variants:
        p50, p99, mean = stats[v.name]
        base = stats[f"{v.direction} plain"][0]
        lines.append(f"| {v.name} | {p50:.3f} | {p99:.3f} | {mean:.3f} | {1e3 * (p50 - base):+.0f} |")
    lines.append("")
    for direction in ("duplex", "send", "recv"):
        x, y = stats[f"{direction} plain"], stats[f"{direction} plain again"]
        lines.append(f"Spread of the plain {direction} session against itself: p50 {1e3 * abs(x[0] - y[0]):.0f} us, p99 {1e3 * abs(x[1] - y[1]):.0f} us.")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
