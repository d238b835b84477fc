#!/usr/bin/env python3
"""Generate tests/golden/g9_conceal_*.npz: a decoder that fills lost frames from the model's prior net, stepped frame by
frame with the REFERENCE's own modules (build container only).  Only torch is needed by that module.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conceal.py [--ref /root/reference]

The reference has no such operator (its BVRNN.decode, bvrnn.py:211-229, knows no lost frame), but it has every piece, and only whole
calls of it are made here: the codes come from its ``BVRNN.encode``; per frame, ``net.prior(h)`` (bvrnn.py:68-73) gives the
probabilities, the script rounds them, puts 0.5 behind the frame's bit count on a variable-rate model and takes them where the frame
is marked lost, and ONE call of ``BVRNN.decode`` on that single frame, from the carried state, gives the frame's mel and the next
state.  At the end ``BVRNN.decode`` of all filled codes in one call must give the same bits.  The weights are seeded synthetic ones
(bvcodec/synth.py) and are regenerated from the seed by the tests.

The input seed is searched as make_golden.py does, so that every GENERATED active bit keeps |p - 0.5| above nb_thr.
Loss pattern (row 0): frame 0 lost, an isolated loss, a burst of 6 frames, a second burst at the end; row 1 loses nothing.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from bvcodec import config as bconfig, synth          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    from bvrnn import BVRNN                                              # reference

    conf = bconfig.load_config(os.path.join(a.ref, "configs", "config_varBitRate.toml"))
    B, T, Z = 2, 40, 64
    present = torch.ones(B, T, dtype=torch.bool)
    present[0, 0] = False                                   # a lost frame 0: generated from prior(h0)
    present[0, 7] = False                                   # an isolated loss
    present[0, 15:21] = False                               # a burst
    present[0, 36:40] = False                               # the sequence ends inside a burst
    for h_dim, var_bit in ((64, True), (1024, False)):
        c = dict(conf); c["h_dim"] = h_dim; c["var_bit"] = var_bit
        tag = f"h{h_dim}_{'var' if var_bit else 'fix'}"
        sd = synth.bvrnn_state_dict(c, seed=1234)
        net = BVRNN(80, h_dim, Z, [np.zeros(80), np.ones(80)], c["log_sigma_init"], variableBit=var_bit)
        net.load_state_dict(sd)
        net.eval()
        nb_thr = 2e-5 if var_bit else 1e-5                  # make_golden.py's margins
        idx = torch.arange(Z)[None, :]
        for in_seed in range(77, 677):
            rng = np.random.default_rng(in_seed)
            y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
            bits = torch.full((B, T), 35.0)
            bits[0, 16], bits[0, 17], bits[0, 18] = 17.0, 64.0, 0.0          # re-rated inside the burst (a var_bit model reads them)
            bits[1] = torch.from_numpy(rng.integers(0, 65, size=T).astype(np.float32))
            with torch.no_grad():
                codes, _ = net.encode(y, bits, torch.zeros(1, B, h_dim))
                h = torch.zeros(1, B, h_dim)
                mel, zs, ps = [], [], []
                worst = 1.0
                for t in range(T):
                    p = net.prior(h[-1])                                       # bvrnn.py:68-73 (sigmoid included)
                    g = torch.round(p)
                    act = idx < (bits[:, t, None] if var_bit else torch.full((B, 1), float(Z)))
                    g = torch.where(act, g, torch.full_like(g, 0.5))           # no bits behind the frame's bit count
                    lost = ~present[:, t]
                    z_t = torch.where(lost[:, None], g, codes[:, t])
                    sel = act & lost[:, None]
                    if bool(sel.any()):
                        worst = min(worst, float((p - 0.5).abs()[sel].min()))
                    mel_t, h = net.decode(z_t[:, None], h)                     # the reference's decoder on this one frame
                    mel.append(mel_t[:, 0]); zs.append(z_t); ps.append(p)
            if worst > nb_thr:
                break
        st = lambda l: torch.stack(l).permute(1, 0, 2).contiguous()
        codes_out, prior, mel = st(zs), st(ps), st(mel)
        n_gen = int(((idx[None] < (bits[:, :, None] if var_bit else 64.0)) & ~present[:, :, None]).sum())
        print(f"{tag}: input seed {in_seed}, {int((~present).sum())} lost frames, {n_gen} generated bits, "
              f"min |p-0.5| over them = {worst:.3e}")
        # frame by frame or in one call: BVRNN.decode of the filled codes gives the same bits, and the row without loss got the
        # encoder's codes back untouched
        with torch.no_grad():
            mel_ref, h_ref = net.decode(codes_out, torch.zeros(1, B, h_dim))
        assert torch.equal(mel_ref, mel) and torch.equal(h_ref, h) and torch.equal(codes_out[1], codes[1])
        # whatever the lost positions of the stored codes hold must not matter: store NaN there
        stored = codes.clone()
        stored[~present] = float("nan")
        out = dict(codes=stored, present=present.to(torch.uint8), bits=bits, codes_out=codes_out, prior=prior, mel=mel,
                   h_last=h[0], seed=np.int64(1234))
        path = os.path.join(HERE, f"g9_conceal_{tag}.npz")
        np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
                                     for k, v in out.items()})
        print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
