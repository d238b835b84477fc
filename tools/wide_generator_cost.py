#!/usr/bin/env python3
"""What a wide generator costs on the chip, at 64 x 430 frames (profiles/wide_generator_cost.md): ``model.vocoder`` at
``upsample_initial_channel`` 128 (shipped), 256 and 512 - 3 warm-ups, median of 10 calls, device events around each call - and the
time of every layer group from the cumulative time of bvc_test_vocoder_tap up to each tap, differenced (tools/voc_stage_times.py's
method, with device events).  Beside each time the algorithmic FLOPs counted as bench.py's roofline counts the generator's
convolutions, the TFLOP/s they make and their share of the fp32-MFMA figure bench.py uses.  ``--sweep`` repeats the wide stages with
the other compiled tile heights (BVC_AMP256_TR / BVC_AMP128_TR are read per launch).

    python tools/wide_generator_cost.py [--batch 64] [--frames 430] [--widths 128,256,512] [--sweep]
"""
import argparse
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np          # noqa: E402
import torch                # noqa: E402

import vocoder_layers as vl                                     # noqa: E402
from bvcodec import BVRNNCodecModel, _abi, synth                # noqa: E402

DEV = "cuda:0"
PEAK_FP32_MFMA_TFLOPS = 157.3          # bench.py
SWEEP = {256: ("BVC_AMP256_TR", vl.AMP_HEIGHTS[256]), 128: ("BVC_AMP128_TR", vl.AMP_HEIGHTS[128])}


def make(directory, width):
    cfg = os.path.join(directory, f"wide{width}.toml")
    conf = vl.write_config(cfg, width=width, h_dim=64)
    p1, p2 = os.path.join(directory, "bvrnn"), os.path.join(directory, f"bigvgan_{width}")
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


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return float(np.median([timed(fn) for _ in range(reps)]))


def group_flops(conf, frames):
    """2 x MACs of conv_pre, then (upsampler, nine AMP pairs) per stage, then conv_post, for `frames` frames in all (bench.py's
    flops_per_step counts the same products)."""
    v = conf["vocoder_config"]
    ch, rate = v["upsample_initial_channel"], 1
    out = [("conv_pre", conf["num_mels"] * ch * 7)]
    for i, (u, k) in enumerate(zip(v["upsample_rates"], v["upsample_kernel_sizes"])):
        rate *= u
        out.append((f"up{i} {ch}->{ch // 2}", rate * ch * (ch // 2) * (k // u)))
        ch //= 2
        out.append((f"amp{i} C={ch}", rate * ch * ch * sum(v["resblock_kernel_sizes"]) * 6))
    out.append((f"conv_post C={ch}", rate * ch * 7))
    return [(name, 2.0 * frames * macs) for name, macs in out]


def tap_times(eng, lib, mel_tm, B, T, reps, taps=range(9)):
    ws, nws = eng.workspace(B, T)
    n = ctypes.c_int64()
    cum = {}
    for which in taps:
        def run():
            _abi.check(lib.bvc_test_vocoder_tap(eng.handle, _abi.ptr(mel_tm), B, T, which, None, ctypes.byref(n), ws, nws, eng.stream()))
        cum[which] = median_ms(run, 1, reps)
    return cum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--widths", default="128,256,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _abi.load()
    d = tempfile.mkdtemp(prefix="bvc_wide_cost_")
    B, T = a.batch, a.frames
    rng = np.random.default_rng(0)
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32)).to(DEV)
    mel_tm = mel.permute(0, 2, 1).contiguous()
    for width in (int(w) for w in a.widths.split(",")):
        model, eng, conf = make(d, width)
        ms = median_ms(lambda: model.vocoder(mel, 10 ** 9), 3, a.reps)
        groups = group_flops(conf, B * T)
        total = sum(f for _, f in groups)
        print(f"width {width}: vocoder {B} x {T} frames -> {eng.vocoder_length(T)} samples: median of {a.reps} {ms:.2f} ms, {total / 1e12:.3f} TFLOP, "
              f"{total / ms / 1e9:.1f} TFLOP/s = {total / ms / 1e9 / PEAK_FP32_MFMA_TFLOPS:.3f} of {PEAK_FP32_MFMA_TFLOPS}", flush=True)
        cum = tap_times(eng, lib, mel_tm, B, T, max(3, a.reps // 2))
        prev = 0.0
        for which, (name, fl) in enumerate(groups[:-1]):
            dt = cum[which] - prev
            prev = cum[which]
            print(f"  width {width} {name}: {dt:.3f} ms, {fl / 1e9:.1f} GFLOP, {fl / dt / 1e9:.1f} TFLOP/s = {fl / dt / 1e9 / PEAK_FP32_MFMA_TFLOPS:.3f}", flush=True)
        print(f"  width {width} {groups[-1][0]} (whole call - last tap): {ms - cum[8]:.3f} ms", flush=True)
        if a.sweep:
            for stage, C in enumerate(vl.stage_channels(conf)):
                if C not in SWEEP:
                    continue
                key, heights = SWEEP[C]
                fl = dict(groups)[f"amp{stage} C={C}"]
                for h in heights:
                    os.environ[key] = str(h)
                    try:
                        cs = tap_times(eng, lib, mel_tm, B, T, max(3, a.reps // 2), (1 + 2 * stage, 2 + 2 * stage))
                    finally:
                        del os.environ[key]
                    dt = cs[2 + 2 * stage] - cs[1 + 2 * stage]
                    print(f"  sweep width {width} stage {stage} C={C} {key}={h}: {dt:.3f} ms, {fl / dt / 1e9:.1f} TFLOP/s = "
                          f"{fl / dt / 1e9 / PEAK_FP32_MFMA_TFLOPS:.3f}", flush=True)
        model.check_status()
        del model, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
