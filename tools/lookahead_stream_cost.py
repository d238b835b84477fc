#!/usr/bin/env python3
"""What a hop of the incremental generator costs behind a look-ahead window, on the chip (profiles/lookahead_stream_cost.md).

Per batch (64, 256 streams) and hop (k = 1, 2 frames), ms per push, device events around every push, median / min / max of the
repetitions behind a warm-up that carries every stream past its look-ahead; the variants of one (batch, hop) alternate push by push:

* ``lookahead <tag>``: ``VocoderStream(lookahead=True)`` of the all-symmetric and the mixed configuration, with the short window tiles
  (amp_symmetric_window, k_vocoder_amp.hip) and, BVC_SYM_WINDOW_TILES=offline, with the offline tile shapes: the sweep;
* ``plain causal``: the shipped causal model's plain ``VocoderStream`` - the yardstick.  ``--plain-only --tree DIR`` runs this line
  alone on the package of another checkout (the parent commit, built), in the same session on the same card;
* ``offline window <tag>``: what a user has without the look-ahead window - ``model.vocoder`` over a context of
  ceil(D / 256) + 26 + k frames per hop.

``--alone`` times every variant once more in a run of its own: alternating, each push finds the caches filled by the six others (the
plain stream alone is 0.05 ms faster per push than between the others).

    python tools/lookahead_stream_cost.py [--batches 64 256] [--hops 1 2] [--reps 60] [--alone] [--plain-only] [--tree DIR]
"""
import argparse
import math
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
ap.add_argument("--hops", type=int, nargs="+", default=[1, 2])
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warm", type=int, default=24)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--alone", action="store_true", help="also time every variant in a run of its own, not alternating")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.tree)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402
import torch                # noqa: E402

import vocoder_layers as vl                                     # noqa: E402
from bvcodec import BVRNNCodecModel, config, synth              # noqa: E402
from bvcodec.streaming import VocoderStream                     # noqa: E402

DEV = "cuda:0"
CONTEXT = 26                                                    # frames of context the stateless scheme keeps (stream_plans.CONTEXT_FRAMES)


def make(directory, tag):
    cfg = os.path.join(directory, f"{tag}.toml")
    conf = vl.write_config(cfg, switches=None if tag == "causal" else vl.SYM_CONFIGS[tag], h_dim=64)     # the coder is not timed
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


def report(what, B, k, ts):
    v = np.asarray(ts)
    print(f"COST B={B} k={k} {what}: median {np.median(v):.3f} ms per push, min {v.min():.3f}, max {v.max():.3f} of {len(v)}", flush=True)


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    d = tempfile.mkdtemp(prefix="bvc_lookahead_cost_")
    tags = ("causal",) if ARGS.plain_only else ("causal", "all", "mixed")
    models = {tag: make(d, tag) for tag in tags}
    rng = np.random.default_rng(0)
    for B in ARGS.batches:
        for k in ARGS.hops:
            mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, k, 80))).astype(np.float32)).to(DEV)
            runs = {"plain causal": (VocoderStream(models["causal"][1], B, k), None)}
            if not ARGS.plain_only:
                for tag in ("all", "mixed"):
                    for tiles in ("short", "offline"):
                        runs[f"lookahead {tag} tiles={tiles}"] = (VocoderStream(models[tag][1], B, k, lookahead=True), tiles)
            calls = {}
            for what, (vs, tiles) in runs.items():
                def push(vs=vs, tiles=tiles):
                    if tiles == "offline":
                        os.environ["BVC_SYM_WINDOW_TILES"] = "offline"
                    try:
                        vs.push(mel)
                    finally:
                        os.environ.pop("BVC_SYM_WINDOW_TILES", None)
                calls[what] = push
            if not ARGS.plain_only:
                for tag in ("all", "mixed"):
                    model, _, conf = models[tag]
                    frames = math.ceil(config.generator_lookahead(conf) / 256) + CONTEXT + k
                    ctx = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, frames, 80))).astype(np.float32)).to(DEV)
                    calls[f"offline window {tag} ({frames} frames)"] = lambda model=model, ctx=ctx: model.vocoder(ctx, 10 ** 9, _time_major=True)
            for _ in range(max(ARGS.warm, 16)):                  # every stream past its look-ahead (13 frames at the most), every shape warm
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            ts = {what: [] for what in calls}
            for _ in range(ARGS.reps):
                for what, fn in calls.items():
                    ts[what].append(timed(fn))
            for what in calls:
                report(what, B, k, ts[what])
            if ARGS.alone:                                        # each variant in a run of its own: its weights and histories stay in the caches
                for what, fn in calls.items():
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    report(what + " [alone]", B, k, [timed(fn) for _ in range(ARGS.reps)])
            del runs, calls
            torch.cuda.empty_cache()
    for model, _, _ in models.values():
        model.check_status()


if __name__ == "__main__":
    main()
