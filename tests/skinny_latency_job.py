"""The workload test_gpu_mtw_model.py runs twice - in a child process under BVC_LATENCY=1 (the switch is read once per process, at the
first launch of the recurrent-layer kernel) and in the test process without it - and compares array by array:

    python tests/skinny_latency_job.py OUT_DIR      writes OUT_DIR/<name>.npy and prints "SK_LIN_LATENCY <one-frame> <multi-frame>"
"""
import os
import sys

import numpy as np
import torch

# (M, N, K) of tests/test_gpu_skinny_tiles.py: empty waves, the remainder loop alone, trips of the unrolled loop (U = 4 here) with and
# without a remainder, a last tile of one row, column tiles that are no multiple of 8
LINEAR_SHAPES = ((1, 16, 16), (17, 16, 16), (65, 80, 80), (33, 144, 1152), (65, 144, 1024), (49, 80, 2048), (130, 1024, 2048))
MODEL_SHAPES = ((5, 3), (5, 6), (40, 3), (40, 6))        # (B, T): T <= 4 runs the all-frame layers on the multi-frame twin
H_DIM = 128


def run():
    """{name: numpy array} of the workload in this process, and the launch counts (2, SK_COUNT) it added."""
    import bvrnn_draws as bd
    import skinny_kernels as sk
    from bvcodec import _abi
    from gpu_common import DEV, make_model, on_schedule
    lib = _abi.load()
    before = sk.counts(lib)
    st = _abi.current_stream(torch.device(DEV))
    out = {}
    for M, N, K in LINEAR_SHAPES:
        for act in (0, 1):
            g = torch.Generator().manual_seed(M + N + K + act)
            x = torch.randn(M, K, generator=g).to(DEV)
            w = (torch.randn(N, K, generator=g) / np.sqrt(K)).to(DEV)
            b = torch.randn(N, generator=g).to(DEV)
            y = torch.full((M, N), float("nan"), device=DEV)
            _abi.check(lib.bvc_test_linear(_abi.ptr(x), _abi.ptr(w), _abi.ptr(b), M, N, K, act, _abi.ptr(y), st))
            torch.cuda.synchronize()
            out[f"linear_{M}_{N}_{K}_{act}"] = y.cpu().numpy()
    model = make_model(True, H_DIM)[0]
    for B, T in MODEL_SHAPES:
        y, bits = bd.inputs(B, T, seed=B + T)
        yd, bd_ = y.to(DEV), bits.to(DEV)
        h0 = torch.zeros(1, B, H_DIM, device=DEV)

        def fn():
            codes, all_h, prob = model.bvrnn.encode(yd, bd_, h0, return_prob=True)
            mel, hT = model.bvrnn.decode(codes, h0)
            return codes, all_h, prob, mel, hT

        for name, t in zip(("codes", "all_h", "prob", "mel", "hT"), on_schedule(model, "layers", fn)):
            out[f"model_{B}_{T}_{name}"] = t.cpu().numpy()
    model.check_status()
    return out, sk.counts(lib) - before


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import skinny_kernels
    arrays, delta = run()
    for name, a in arrays.items():
        np.save(os.path.join(sys.argv[1], name + ".npy"), a)
    print("SK_LIN_LATENCY", int(delta[0, skinny_kernels.SK_LIN_LATENCY]), int(delta[1, skinny_kernels.SK_LIN_LATENCY]), flush=True)
    print("SK_LIN", int(delta[0, skinny_kernels.SK_LIN]), int(delta[1, skinny_kernels.SK_LIN]), flush=True)
