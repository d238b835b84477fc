#!/usr/bin/env python3
"""Generate tests/golden/g12_bigvgan_wide_{256,512}.npz: the REFERENCE's own ``BigVGAN`` (third_party/BigVGAN/models.py) with
``upsample_initial_channel`` 256 and 512 - the width of the generator configuration the reference ships beside its code,
third_party/BigVGAN/bigvgan_base_22khz_80band.json, is 512 - on seeded synthetic weights (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py [--ref /root/reference]

The reference's variable-rate TOML otherwise unchanged (causal layers, rates [8, 8, 2, 2]).  The inputs come from ONE
``np.random.default_rng(79)`` stream, mel = -4 + 1.6 N(0, 1), in this order: width 256 with B = 2, T = 6, then width 512 with B = 1,
T = 6.  Stored are the input, the untrimmed waveform, conv_pre and the four stage outputs (what the next upsampler, or
``activation_post``, receives), the seed and the width; the upsampler results are not (they would take a file beyond a MiB).  The
weights are regenerated from the seed by the tests (``load_state_dict`` is strict, so the layout is the reference's).

Expected output (a regenerated file is recognised by it):
    width 256: stage lengths [56, 456, 914, 1830], wav rms 0.0733 max 0.2951
    width 512: stage lengths [56, 456, 914, 1830], wav rms 0.0891 max 0.2469
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bvcodec import config as bconfig, synth          # noqa: E402
import vocoder_layers as vl                            # noqa: E402

SEED = 1235
CASES = ((256, 2, 6), (512, 1, 6))                     # (width, B, T), in the order the inputs are drawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    # the reference's utils.py imports meldataset.py, which imports librosa (absent from the image, make_golden.py): an empty
    # stand-in, nothing of it is called on this path
    import types
    librosa, util, filters = types.ModuleType("librosa"), types.ModuleType("librosa.util"), types.ModuleType("librosa.filters")
    util.normalize, filters.mel = None, None
    librosa.util, librosa.filters = util, filters
    sys.modules.update({"librosa": librosa, "librosa.util": util, "librosa.filters": filters})
    from third_party.BigVGAN.env import AttrDict                        # reference
    from third_party.BigVGAN.models import BigVGAN                      # reference

    conf = bconfig.load_config(os.path.join(a.ref, "configs", "config_varBitRate.toml"))
    rng = np.random.default_rng(79)
    for width, B, T in CASES:
        mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, 80, T))).astype(np.float32))
        c = vl.with_switches(conf, width=width)
        bconfig.check_supported(c)
        sd = synth.generator_state_dict(c, seed=SEED)
        voc = BigVGAN(AttrDict(c["vocoder_config"]))
        voc.load_state_dict(sd)                                           # strict: the key layout is the reference's
        voc.eval()
        taps = {}
        hooks = [voc.conv_pre.register_forward_hook(lambda m, i, o: taps.__setitem__("conv_pre", o.detach().clone()))]
        for i in range(1, 4):                                             # stage i - 1 is what upsampler i receives
            hooks.append(voc.ups[i][0].register_forward_pre_hook(
                lambda m, inp, i=i: taps.__setitem__(f"stage{i - 1}", inp[0].detach().clone())))
        hooks.append(voc.activation_post.register_forward_pre_hook(
            lambda m, inp: taps.__setitem__("stage3", inp[0].detach().clone())))
        with torch.no_grad():
            wav = voc(mel, 10 ** 9)
        for h in hooks:
            h.remove()
        lens = bconfig.generator_length(c, T, stages=True)
        assert [taps[f"stage{i}"].shape[2] for i in range(4)] == lens and wav.shape == (B, 1, lens[-1]) and len(taps) == 5
        assert [taps[f"stage{i}"].shape[1] for i in range(4)] == vl.stage_channels(c) and taps["conv_pre"].shape == (B, width, T)
        print(f"width {width}: stage lengths {lens}, wav rms {float(wav.pow(2).mean().sqrt()):.4f} max {float(wav.abs().max()):.4f}")
        path = os.path.join(HERE, f"g12_bigvgan_wide_{width}.npz")
        np.savez_compressed(path, mel=mel.numpy(), wav=wav.numpy(), seed=np.int64(SEED), width=np.int64(width),
                            **{k: v.numpy() for k, v in taps.items()})
        print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
