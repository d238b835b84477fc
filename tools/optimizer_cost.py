#!/usr/bin/env python3
"""What an optimiser step on a live model costs on the chip at the reference's training shape - batch_size 32, 4.0 s = 344 frames,
h_dim 1024 (profiles/optimizer_cost.md) - next to the ``bvc_bvrnn_backward`` call it follows and to the path it replaces, all from one
run and one build: ``bvc_optimizer_step`` (norm, AdamW, rewrite of every derived form of the weights) and ``bvc_bvrnn_backward``, each
timed with a HIP event pair around the library call, 3 warm-ups, median of 7, the two alternating; and the replaced path - the
parameters copied to the host, then ``bvc_model_create`` with the same tensors - with host timers around a synchronised call, median
of 3.  The split of the step into norm, Adam and re-layout comes from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o steps -- python tools/optimizer_cost.py --steps-only 10
    python tools/optimizer_cost.py [--batch 32] [--frames 344] [--trace TRACE_DIR --trace-steps 10] [--out profiles/optimizer_cost.md]
"""
import argparse
import csv
import glob
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from bvcodec import BVRNNCodecModel, config, synth       # noqa: E402
from bvcodec.engine import _Engine                       # noqa: E402

DEV = "cuda:0"
FAMILIES = (("norm", ("norm_partial_kernel", "norm_final_kernel")), ("Adam", ("adam_kernel",)),
            ("re-layout", ("copy_segments_kernel", "repack_rows_kernel", "pack_gru_il_kernel", "fold_px0_dec3_kernel", "transpose_kernel")))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def trace_split(trace_dir, steps):
    """{family: (ms per step, launches per step)} of the LAST ``steps`` steps of a traced run (a step starts with the first stage of
    the norm; what the run launches before them - the transposed copies' first build, the step that allocates - is left out), or None."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    starts = [i for i, r in enumerate(rows) if "norm_partial_kernel" in r[2]]
    if len(starts) < steps:
        return None
    out = {name: [0.0, 0.0] for name, _ in FAMILIES}
    out["other kernels"] = [0.0, 0.0]
    for t0, t1, name in rows[starts[-steps]:]:
        fam = next((f for f, keys in FAMILIES if any(k in name for k in keys)), "other kernels")
        out[fam][0] += (t1 - t0) / 1e6 / steps
        out[fam][1] += 1.0 / steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=344)
    ap.add_argument("--steps-only", type=int, default=0, help="run this many steps after the model's first backward and leave (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="directory of that traced run")
    ap.add_argument("--trace-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.frames
    conf = config.load_config(config.DEFAULT_CONFIG)
    H, Z, X = conf["h_dim"], conf["z_dim"], conf["num_mels"]
    p1, p2 = synth.write_checkpoints(conf, tempfile.mkdtemp(prefix="bvc_cost_"), seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    g = torch.Generator().manual_seed(3)
    bvrnn = model.bvrnn
    _, total = bvrnn.grad_layout()
    opt = bvrnn.optimizer(lr=1e-4, weight_decay=0.01, max_grad_norm=1000.0)        # the reference's clip_grad_norm_(.., 1000): the norm always runs
    if a.steps_only:
        # the transposed copies exist (a model that trains has run backward), so the traced steps rewrite them too
        eng = bvrnn.engine()
        eng.call("bvc_bvrnn_backward_prepare", eng.handle)
        flat = 1e-3 * torch.randn(total, generator=g).to(DEV)
        opt.step(flat)                                                             # the first step allocates the master copy
        torch.cuda.synchronize()
        for _ in range(a.steps_only):
            opt.step(flat)
        torch.cuda.synchronize()
        return
    y = (-4.0 + 1.6 * torch.randn(B, T, X, generator=g)).to(DEV)
    bits = torch.randint(0, Z + 1, (B, T), generator=g).float().to(DEV)
    r, noise = torch.rand(T, generator=g), torch.rand(B, T, Z, generator=g).to(DEV)
    gdec = torch.randn(B, T, X, generator=g).to(DEV)
    grads = {}
    bwd = lambda: grads.__setitem__("flat", bvrnn.backward(y, 0.5, False, bits, gdec, 0.1, r=r, noise=noise, flat=True))
    step = lambda: opt.step(grads["flat"])
    for _ in range(3):
        bwd(); step()
    torch.cuda.synchronize()
    tb, ts = [], []
    for _ in range(7):
        tb.append(event_ms(bwd)); ts.append(event_ms(step))
    b_ms, s_ms = float(np.median(tb)), float(np.median(ts))
    # the path a step replaces: the 36 tensors to the host, then a new model from them
    eng = bvrnn.engine()
    layout, _ = bvrnn.grad_layout()
    told = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flat = eng.params_get(total).cpu()
        t1 = time.perf_counter()
        tensors = dict(model._tensors)
        tensors.update({n: flat[off:off + numel].view(tensors[n].shape).clone() for n, off, numel in layout})
        fresh = _Engine(conf, tensors, eng.device)
        torch.cuda.synchronize()
        told.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        del fresh
    copy_ms, create_ms = (float(np.median([t[i] for t in told])) for i in (0, 1))
    lines = [
        "# Optimiser step on a live model: cost at the training shape", "",
        f"`python tools/optimizer_cost.py --batch {B} --frames {T}` on one MI355X; h_dim {H}, {total} parameters ({4 * total / 1e6:.1f} MB), AdamW with "
        "weight decay and the 2-norm clip, the transposed copies of the backward pass rewritten with every step.  One run, one build.", "",
        "| what | median ms | min | max |", "|---|---|---|---|",
        f"| `bvc_bvrnn_backward` ({B} x {T} frames) | {b_ms:.2f} | {min(tb):.2f} | {max(tb):.2f} |",
        f"| `bvc_optimizer_step` (norm, AdamW, every derived form rewritten) | {s_ms:.3f} | {min(ts):.3f} | {max(ts):.3f} |",
        f"| replaced path: parameters to the host | {copy_ms:.1f} | {min(t[0] for t in told):.1f} | {max(t[0] for t in told):.1f} |",
        f"| replaced path: `bvc_model_create` with the same tensors | {create_ms:.1f} | {min(t[1] for t in told):.1f} | {max(t[1] for t in told):.1f} |", "",
        f"The step is {s_ms / b_ms:.4f} of the backward call measured alongside it; the path it replaces, {copy_ms + create_ms:.0f} ms, is "
        f"{(copy_ms + create_ms) / b_ms:.2f} of it ({(copy_ms + create_ms) / s_ms:.0f} steps).  Events around the library call (backward, step); "
        "host timers around synchronised calls (replaced path, which also rebuilds the generator and runs the residency census).", ""]
    split = trace_split(a.trace, a.trace_steps) if a.trace else None
    if split:
        tot = sum(v[0] for v in split.values())
        lines += [f"Kernel time of a step by family, from a kernel trace of {a.trace_steps} steps taken in a run of its own (`--steps-only`):", "",
                  "| family | ms per step | launches per step | share |", "|---|---|---|---|"]
        lines += [f"| {fam} | {ms:.3f} | {n:.1f} | {ms / tot:.2f} |" for fam, (ms, n) in split.items()]
        lines += ["", f"Sum of kernel time: {tot:.3f} ms per step.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
