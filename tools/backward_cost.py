#!/usr/bin/env python3
"""What the backward pass of ``BVRNN.forward`` costs on the chip at the reference's training shape - batch_size 32, 4.0 s = 344 frames,
h_dim 1024 (profiles/backward_cost.md): ``bvc_bvrnn_backward`` (which runs its own forward) against ``bvc_bvrnn_forward`` on the same
inputs and build, each timed with a HIP event pair around the library call: 3 warm-ups, median of 7, the two alternating.  The
weight-gradient GEMMs are timed on their own through ``bvc_test_weight_grad`` at the call's shapes (it allocates and synchronises, so
its figure is an upper bound, taken with host timers around a call whose workspace is warm).  Launch counts are those of the program
(csrc/backward.hip), per frame and per call.

    python tools/backward_cost.py [--batch 32] [--frames 344] [--out profiles/backward_cost.md]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from bvcodec import BVRNNCodecModel, _abi, config, synth       # noqa: E402

DEV = "cuda:0"
PEAK_TFLOPS = 157.3          # fp32 MFMA peak of the MI355X, the figure the README uses


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=344)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.frames
    conf = config.load_config(config.DEFAULT_CONFIG)
    H, Z, X = conf["h_dim"], conf["z_dim"], conf["num_mels"]
    p1, p2 = synth.write_checkpoints(conf, tempfile.mkdtemp(prefix="bvc_cost_"), seed=1234)
    model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    g = torch.Generator().manual_seed(3)
    y = (-4.0 + 1.6 * torch.randn(B, T, X, generator=g)).to(DEV)
    bits = torch.randint(0, Z + 1, (B, T), generator=g).float().to(DEV)
    r, noise = torch.rand(T, generator=g), torch.rand(B, T, Z, generator=g).to(DEV)
    gdec = torch.randn(B, T, X, generator=g).to(DEV)
    fwd = lambda: model.bvrnn.forward(y, 0.5, False, bits, r=r, noise=noise)
    bwd = lambda: model.bvrnn.backward(y, 0.5, False, bits, gdec, 0.1, r=r, noise=noise, grad_input=True)
    for _ in range(3):
        fwd(); bwd()
    torch.cuda.synchronize()
    tf, tb = [], []
    for _ in range(7):
        tf.append(event_ms(fwd)); tb.append(event_ms(bwd))
    f_ms, b_ms = float(np.median(tf)), float(np.median(tb))
    # the weight-gradient GEMMs of one call: (rows, N, K, how many)
    TB = B * T
    shapes = [(2 * TB, H, X, 1), (2 * TB, H, H, 2), (TB, H, Z, 1), (TB, H, H, 2 + 2 + 1 + 1 + 1 + 2 + 2), (TB, Z, H, 2), (TB, X, H, 1),
              (2 * TB, 3 * H, H, 3)]
    lib = _abi.load()
    wg_ms, flop = 0.0, 0.0
    for M, N, K, n in shapes:
        dy, x, out = torch.randn(M, N, device=DEV), torch.randn(M, K, device=DEV), torch.empty(N, K, device=DEV)
        call = lambda: _abi.check(lib.bvc_test_weight_grad(_abi.ptr(dy), _abi.ptr(x), M, N, K, _abi.ptr(out), None, _abi.current_stream(torch.device(DEV))))
        call(); call()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        wg_ms += n * float(np.median(ts))
        flop += n * 2.0 * M * N * K
    # per frame, both chains running (csrc/backward.hip): 2 x 6 for the GRU cells (two gate products, the cell, three dX), 6 for the frame's
    # own phi_x, 1 mel, 8 dec, 6 phi_z, 1 sampler + KLD, 6 enc, 6 prior
    per_frame = 2 * 6 + 6 + 1 + 8 + 6 + 1 + 6 + 6
    lines = [
        "# Backward pass of `BVRNN.forward`: cost at the training shape", "",
        f"`python tools/backward_cost.py --batch {B} --frames {T}` on one MI355X; h_dim {H}, p_use_gen 0.5, sampled, the input gradient asked for.", "",
        "| call | median ms | min | max |", "|---|---|---|---|",
        f"| `bvc_bvrnn_forward` | {f_ms:.2f} | {min(tf):.2f} | {max(tf):.2f} |",
        f"| `bvc_bvrnn_backward` (runs its own forward) | {b_ms:.2f} | {min(tb):.2f} | {max(tb):.2f} |", "",
        f"Backward / forward: {b_ms / f_ms:.2f}.  The weight-gradient GEMMs of one call, timed alone (upper bound, host timers): {wg_ms:.2f} ms = "
        f"{wg_ms / b_ms:.2f} of the call, {flop / 1e9:.1f} GFLOP, {flop / wg_ms / 1e9:.1f} TFLOP/s = {flop / wg_ms / 1e9 / PEAK_TFLOPS:.2f} of the fp32 MFMA peak "
        f"({PEAK_TFLOPS} TFLOP/s).", "",
        f"Launches: the taped forward's own (as `bvc_bvrnn_forward`), then about {per_frame} per frame of the reverse recurrence (one per layer, per "
        "activation and per GRU piece, both chains running) plus one copy, and 5 + 41 + 40 kernels over all frames (phi_x's transposed layers, "
        "the weight gradients with their reductions, the bias sums).  No threshold: the number to beat is the one above.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
