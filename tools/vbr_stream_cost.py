#!/usr/bin/env python3
"""What a send tick costs when the session chooses its own rates (profiles/vbr_stream_cost.md): 256 streams at a hop of 441 samples,
warm, p50 and p99 of a tick for ``StreamingCodec(direction="send", vbr=...)`` with K = 1, 2 and 4 rungs, K = 4 under a rate cap, and
the plain send session on its default schedule and with ``BVC_STREAM_FLOW=0`` - the launch-per-layer tick a vbr tick is built from.
All in one run, one session after the other on the same input.  A tick is timed with a HIP event pair around ``push`` on the caller's
stream (the session's stream waits for it and it for the session's), 80 warm-up ticks, then 400 timed ones.

    python tools/vbr_stream_cost.py [--streams 256] [--out profiles/vbr_stream_cost.md]
    python tools/vbr_stream_cost.py --plain-only [--root TREE]      # the two plain rows alone, as JSON (runs on a tree without vbr=)
    rocprofv3 --kernel-trace --stats -d DIR -o vbr -- python tools/vbr_stream_cost.py --trace-only      # K = 4 uncapped, 200 ticks
    python tools/vbr_stream_cost.py --shares DIR/.../vbr_kernel_stats.csv                                # kernel-time shares of that run
"""
import argparse
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HOP = 441
LADDERS = {1: (6000,), 2: (3000, 6000), 4: (689, 1500, 3000, 6000)}        # 64 / 35, 64 / 8, 17, 35, 64 bits per frame
GROUPS = (("candidates", ("vbr_candidates_kernel",)), ("select", ("vbr_select_kernel",)), ("pack", ("sc_pack_rows_vbr_kernel",)),
          ("bucket in / out, call", ("vbr_tok_kernel", "vbr_set_call_kernel")))


def make_model():
    from bvcodec import BVRNNCodecModel, config, synth
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_vbr_stream_cost_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
    return BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)


def ticks_of(model, B, x, warm, timed, env=None, **kw):
    """ms of every timed tick of one send session (those that emit frames), and its mean bits per frame (None without vbr)."""
    import numpy as np
    import torch
    from bvcodec.streaming import StreamingCodec
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        sc = StreamingCodec(model, B, 3000, hop=HOP, direction="send", **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    ms, bits = [], []
    n = x.shape[1] // HOP
    for t in range(warm + timed):
        row = x[:, (t % n) * HOP:(t % n + 1) * HOP]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        p, _ = sc.push(row)
        b.record()
        torch.cuda.synchronize()
        if t >= warm and p.shape[1]:
            ms.append(a.elapsed_time(b))
            if kw.get("vbr"):
                bits.append(float(sc.last_bits.mean()))
    model.check_status()
    return np.array(ms), (float(np.mean(bits)) if bits else None)


def shares(path):
    """Kernel-time shares from a rocprofv3 --kernel-trace --stats file (columns Name, TotalDurationNs or Percentage)."""
    rows = list(csv.DictReader(open(path)))
    dur = lambda r: float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0)
    total = sum(dur(r) for r in rows)
    out = []
    for name, keys in GROUPS:
        t = sum(dur(r) for r in rows if any(k in r["Name"] for k in keys))
        out.append((name, t, 100.0 * t / total))
    return total, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--warm", type=int, default=80)
    ap.add_argument("--timed", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbr_stream_cost.md"))
    ap.add_argument("--root", default=ROOT, help="the tree whose bvcodec package is measured")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--shares")
    a = ap.parse_args()
    if a.shares:
        total, out = shares(a.shares)
        print(f"kernel time {total / 1e6:.2f} ms")
        for name, t, pct in out:
            print(f"| {name} | {t / 1e6:.3f} ms | {pct:.2f} % |")
        return
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from bvcodec import synth
    assert torch.cuda.is_available(), "needs the MI355X"
    model = make_model()
    B = a.streams
    x = synth.synthetic_speech(B, HOP * 100, seed=7, kind="speech").to(DEV)
    if a.trace_only:
        ticks_of(model, B, x, 40, 160, vbr=dict(bitrates=LADDERS[4], target=0.35))
        return
    pct = lambda v: (float(np.percentile(v, 50)), float(np.percentile(v, 99)))
    rows = [("plain send, default schedule", ticks_of(model, B, x, a.warm, a.timed)),
            ("plain send, BVC_STREAM_FLOW=0", ticks_of(model, B, x, a.warm, a.timed, env={"BVC_STREAM_FLOW": "0"}))]
    if a.plain_only:
        print(json.dumps({name: dict(p50_ms=pct(v)[0], p99_ms=pct(v)[1], ticks=int(v.size)) for name, (v, _) in rows}))
        return
    # a target in the middle of what the rungs reach on this input, so that the ladder is in use
    mel = model.mel_spectrogram(x[:8])
    ex = model.bvrnn.encode_vbr(mel, [8, 17, 35, 64], float("nan"), torch.zeros(1, 8, model.conf["h_dim"], device=DEV), return_all=True)[3]
    tau = float(ex["dist"].median())
    for K, ladder in LADDERS.items():
        rows.append((f"vbr send, K = {K} {ladder} bit/s", ticks_of(model, B, x, a.warm, a.timed, vbr=dict(bitrates=ladder, target=tau))))
    rows.append(("vbr send, K = 4, rate_cap 2600 bit/s, burst 96 bits", ticks_of(model, B, x, a.warm, a.timed,
                 vbr=dict(bitrates=LADDERS[4], target=tau, rate_cap=2600, burst=96))))
    base = pct(rows[1][1][0])[0]
    lines = [f"# Sessions that choose their own rates: cost of a send tick at {B} streams, hop {HOP}", "",
             f"`tools/vbr_stream_cost.py`: HIP events around `push`, {a.warm} warm-up ticks, {a.timed} timed; ms per tick "
             "(a tick of 441 samples emits one or two frames; only ticks that emit frames are counted).", "",
             "| session | p50 ms | p99 ms | against BVC_STREAM_FLOW=0 | mean bits per frame |", "|---|---|---|---|---|"]
    for name, (v, mb) in rows:
        p50, p99 = pct(v)
        lines.append(f"| {name} | {p50:.3f} | {p99:.3f} | {p50 / base:.2f} x | {'-' if mb is None else f'{mb:.1f}'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
