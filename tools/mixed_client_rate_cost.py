#!/usr/bin/env python3
"""What a client rate per slot costs per tick (profiles/mixed_client_rate_cost.md): 256 streams, 20 ms hops, 3 kbit/s; for send, receive
and duplex sessions each: a single-rate 48 kHz session and its twin (the spread of a variant against itself), the mixed-rate session
with its slots dealt 8 / 16 / 48 kHz in rotation, and what a user does without it - three single-rate sessions of 86 / 85 / 85 streams
ticked one after the other, timed as one tick.  All sessions live in one process and take turns, a block of ticks each; every variant
gets its warm ticks first and then the timed ones, each timed with a pair of device events around the push(es) and synchronised like a
real-time loop's.

    python tools/mixed_client_rate_cost.py [--streams 256] [--warm 200] [--ticks 2000] [--block 100] [--out FILE.md]
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
RATES = (8000, 16000, 48000)


class Variant:
    """One line of the table: the sessions that make up one tick, pushed one after the other between one pair of events."""

    def __init__(self, model, direction, tag, sessions, ks):
        self.name, self.direction, self.ms, self.at = f"{direction} {tag}", direction, [], 0
        self.sessions = []                                    # (session, its inputs in rotation)
        g = torch.Generator().manual_seed(3)
        for B, rate in sessions:                              # rate: one client rate, or the tuple of a mixed-rate session
            mixed = isinstance(rate, tuple)
            sc = StreamingCodec(model, B, 3000, hop=441 if mixed else rate // 50, direction=direction, client_rate=rate, open_all=not mixed)
            if mixed:
                for b in range(B):
                    sc.open(b, 3000, client_rate=rate[b % len(rate)])
            if direction == "recv":
                inputs = [torch.randint(0, 256, (B, k, sc.bytes_per_frame), generator=g, dtype=torch.uint8).to(DEV) for k in ks]
            else:
                inputs = [(0.1 * torch.randn(B, sc.hop, generator=g)).to(DEV) for _ in range(16)]
            self.sessions.append((sc, inputs))

    def tick(self, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for sc, inputs in self.sessions:
            x = inputs[self.at % len(inputs)]
            if self.direction == "recv":
                sc.push_packets(x)
            else:
                sc.push(x)
        b.record()
        b.synchronize()
        self.at += 1
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
    d = tempfile.mkdtemp(prefix="bvc_mixed_rate_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    # the frame counts of a plain send session's ticks: what a receive session is given
    probe = StreamingCodec(model, 2, 3000, hop=441, direction="send")
    ks = [probe.push(torch.zeros(2, 441, device=DEV))[0].shape[1] for _ in range(64)][8:]
    del probe
    B = a.streams
    split = [(B // 3 + (1 if i < B % 3 else 0), rate) for i, rate in enumerate(RATES)]      # 256: 86 / 85 / 85
    variants = [Variant(model, direction, tag, sessions, ks)
                for direction in ("send", "recv", "duplex")
                for tag, sessions in (("48 kHz", [(B, 48000)]), ("48 kHz again", [(B, 48000)]), ("mixed 8/16/48 kHz", [(B, RATES)]),
                                      ("three sessions " + "/".join(str(n) for n, _ in split), split))]
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
    lines = [f"{B} streams, 20 ms hops, 3 kbit/s, {a.warm} warm and {a.ticks} timed ticks per variant in blocks of {a.block}, device events per tick.",
             "", "| session | p50 ms | p99 ms | mean ms | p50 - 48 kHz p50, us |", "|---|---|---|---|---|"]
    stats = {v.name: (np.percentile(v.ms, 50), np.percentile(v.ms, 99), float(np.mean(v.ms))) for v in variants}
    for v in variants:
        p50, p99, mean = stats[v.name]
        lines.append(f"| {v.name} | {p50:.3f} | {p99:.3f} | {mean:.3f} | {1e3 * (p50 - stats[f'{v.direction} 48 kHz'][0]):+.0f} |")
    lines.append("")
    for direction in ("send", "recv", "duplex"):
        x, y = stats[f"{direction} 48 kHz"], stats[f"{direction} 48 kHz again"]
        lines.append(f"Spread of the 48 kHz {direction} session against its twin: p50 {1e3 * abs(x[0] - y[0]):.0f} us, "
                     f"p99 {1e3 * abs(x[1] - y[1]):.0f} us, mean {1e3 * abs(x[2] - y[2]):.0f} us.")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
