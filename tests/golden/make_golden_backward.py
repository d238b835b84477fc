#!/usr/bin/env python3
"""Generate tests/golden/g13_bvrnn_backward_*.npz by running the REFERENCE's own ``BVRNN`` (bvrnn.py:86-160) under torch.autograd on
the CPU, at float32.  Only torch is needed by that module.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_backward.py [--ref /root/reference]

The loss is ``(all_dec_mean * gdec).sum() + gkld * kld`` with a seeded gdec, so the stored gradients are the vector-Jacobian product
at (gdec, gkld).  The random numbers the reference consumed are re-drawn after re-seeding (oracle.bvrnn.draw_randomness) and stored,
as tests/golden/make_golden_forward.py does.  A case's seed is searched until, in the float64 oracle (tests/backward_oracle.py),
every rounded argument of an active bit is at least 2e-5 from 0.5 and every e, 1 - e, prior, 1 - prior under the mask at least 1e-5
from the 1e-3 clip of the KLD - so that float32 and float64 take the same branch everywhere.  The script asserts that the oracle at
float32 gives the reference's gradients (measured: bit for bit).

h_dim 64 (B = 3, T = 12, the four modes of make_golden_forward.py, one row of random bit counts that includes 0 and 64): every gradient
in full, two modes a file so that no file exceeds 1 MiB.  h_dim 1024 (B = 2, T = 6, modes 0 and 2): biases in full; of each weight
matrix 4096 seeded entries and the float64 Frobenius norm of the whole.  Weights are regenerated from the seed by the tests.
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

import backward_oracle as bo                          # noqa: E402
from bvcodec import config as bconfig, synth          # noqa: E402
from oracle import bvrnn as obv                       # noqa: E402

MODES = ((0.0, True), (1.0, False), (0.5, False), (0.5, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    from bvrnn import BVRNN                                              # reference

    conf = bconfig.load_config(os.path.join(a.ref, "configs", "config_varBitRate.toml"))
    for h_dim, B, T, modes, files in ((64, 3, 12, (0, 1, 2, 3), {0: "", 1: "", 2: "_2", 3: "_2"}), (1024, 2, 6, (0, 2), {0: "", 2: ""})):
        c = dict(conf); c["h_dim"] = h_dim; c["var_bit"] = True
        sd = synth.bvrnn_state_dict(c, seed=1234)
        net = BVRNN(80, h_dim, 64, [np.zeros(80), np.ones(80)], c["log_sigma_init"], variableBit=True)
        net.load_state_dict(sd)
        net.train()
        net.device = torch.device("cpu")
        outs = {}
        for mode in modes:
            p_use_gen, greedy = MODES[mode]
            for rs in range(5000 + 1000 * mode, 5000 + 1000 * mode + 600):
                rng = np.random.default_rng(rs)
                y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
                bits = torch.full((B, T), 35.0)
                bits[1] = torch.from_numpy(rng.integers(0, 65, size=T).astype(np.float32))
                bits[1, 0], bits[1, 1] = 0.0, 64.0
                gdec = torch.from_numpy(rng.standard_normal((B, T, 80)).astype(np.float32))
                gkld = 0.5 + float(rng.random())
                torch.manual_seed(rs)
                r, noise = obv.draw_randomness(T, B, 64, greedy)
                g64, f64 = bo.grads(sd, y, bits, p_use_gen, greedy, r, noise, gdec, gkld, torch.float64)
                rm, cm = bo.margins(f64, bits, 64)
                if rm >= bo.ROUND_MARGIN and cm >= bo.CLIP_MARGIN:
                    break
            else:
                raise SystemExit(f"h{h_dim} mode {mode}: no seed with the margins")
            net.zero_grad()
            yl = y.clone().requires_grad_(True)
            torch.manual_seed(rs)
            dec, kld = net(yl, p_use_gen, greedy, bits)
            ((dec * gdec).sum() + gkld * kld).backward()
            ref = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters() if k not in bo.NOT_TRAINED}
            ref["y"] = yl.grad.detach().clone()
            g32, f32 = bo.grads(sd, y, bits, p_use_gen, greedy, r, noise, gdec, gkld, torch.float32)
            assert set(ref) == set(g32), set(ref) ^ set(g32)
            worst = max(float((g32[k] - ref[k]).abs().max()) for k in ref)
            assert torch.equal(f32["dec"], dec.detach()) and all(torch.equal(g32[k], ref[k]) for k in ref), (h_dim, mode, worst)
            print(f"h{h_dim} mode {mode} (p_use_gen={p_use_gen}, greedy={greedy}): seed {rs}, rounding margin {rm:.2e}, clip margin {cm:.2e}, "
                  f"kld {float(kld.detach()):.6f}, use_gen {int((r < p_use_gen).sum())}/{T}, max|oracle32 - reference| {worst:.1e}")
            k = f"m{mode}_"
            o = outs.setdefault(files[mode], {"seed": np.int64(1234)})
            o.update({k + "y": y, k + "bits": bits, k + "p_use_gen": np.float64(p_use_gen), k + "greedy": np.bool_(greedy), k + "r": r,
                      k + "gdec": gdec, k + "gkld": np.float64(gkld), k + "dec": dec.detach(), k + "kld": kld.detach(),
                      k + "torch_seed": np.int64(rs)})
            if noise is not None:
                o[k + "noise"] = noise
            for name, g in ref.items():
                if h_dim == 64 or g.dim() < 2 or name == "y":
                    o[k + "g_" + name] = g
                else:
                    o[k + "e_" + name] = g.reshape(-1)[torch.from_numpy(bo.entries(g.numel()))]
                    o[k + "n_" + name] = np.float64(g.double().norm())
        for suffix, o in outs.items():
            path = os.path.join(HERE, f"g13_bvrnn_backward_h{h_dim}_var{suffix}.npz")
            np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in o.items()})
            print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.0f} KiB)")
            assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
