#!/usr/bin/env python3
"""Generate tests/golden/g11_bigvgan_sym_*.npz: the REFERENCE's own ``BigVGAN`` with symmetric layers (``layers_sym`` /
``pre_sym`` / ``post_sym``, third_party/BigVGAN/models.py:35-44,151-155,209-213,230-233) on seeded synthetic weights (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_symmetric.py [--ref /root/reference]

Three configurations of the shipped TOML (tests/vocoder_layers.py SYM_CONFIGS): ``all`` (every switch on), ``mixed``
(``layers_sym = [false, true, false, true]``, ``post_sym``) and ``with_aa`` (symmetric stages 0 and 2 and conv_pre, filtered
stages 1 and 3 and activation_post).  B = 2, T = 12 frames; stored are the input, the untrimmed waveform, conv_pre and the four
stage outputs (what the next upsampler, or ``activation_post``, receives), and the switches.  The weights are regenerated from the
seed by the tests (the switches add no keys; ``load_state_dict`` is strict, so the layout is the reference's).
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
    mel = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((2, 80, 12))).astype(np.float32))
    for tag, sw in vl.SYM_CONFIGS.items():
        c = vl.with_switches(conf, sw)
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
        lens = vl.sym_lengths(c["vocoder_config"], 12)
        assert [taps[f"stage{i}"].shape[2] for i in range(4)] == lens and wav.shape == (2, 1, lens[-1]) and len(taps) == 5
        print(f"{tag}: stage lengths {lens}, wav rms {float(wav.pow(2).mean().sqrt()):.4f} max {float(wav.abs().max()):.4f}")
        path = os.path.join(HERE, f"g11_bigvgan_sym_{tag}.npz")
        np.savez_compressed(path, mel=mel.numpy(), wav=wav.numpy(), seed=np.int64(SEED),
                            **{k: np.asarray(v) for k, v in sw.items()}, **{k: v.numpy() for k, v in taps.items()})
        print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
