"""Shared by test_skinny_pick_cpu.py, test_gpu_skinny_tiles.py and test_gpu_mtw_model.py: the instantiations of the recurrent-layer
kernel as the comments of csrc/k_gemm.hip list them, the rule by which a launch takes one, and the read-back of the launch counts."""
import ctypes

import numpy as np

SK_GRU, SK_GRU_IL, SK_GRU_IL2, SK_GRU_PART, SK_LIN, SK_LIN_LATENCY, SK_LIN2, SK_LIN4, SK_COUNT = range(9)
NAMES = ("SK_GRU", "SK_GRU_IL", "SK_GRU_IL2", "SK_GRU_PART", "SK_LIN", "SK_LIN_LATENCY", "SK_LIN2", "SK_LIN4")
# (gates, accumulator groups, waves, row tiles per workgroup, has a multi-frame twin) of each kernel: the table SKINNY_KERNELS
SHAPE = {SK_GRU: (3, 2, 8, 1, False), SK_GRU_IL: (3, 2, 8, 1, False), SK_GRU_IL2: (3, 2, 8, 2, False), SK_GRU_PART: (3, 1, 8, 1, False),
         SK_LIN: (1, 1, 8, 1, True), SK_LIN_LATENCY: (1, 1, 8, 1, True), SK_LIN2: (1, 1, 8, 2, True), SK_LIN4: (1, 1, 8, 4, True)}
EPI_LINEAR, EPI_ELU, EPI_CODE, EPI_MEL, EPI_GRU, EPI_GRU_PART, EPI_SIGMOID = range(7)
LDS_KIB_PER_CU = 160
BVC_EINVAL = -1


def lds_kib(kernel):
    """NW * NG * NGRP * MTW partial tiles of 1 KiB."""
    ng, ngrp, nw, mtw, _ = SHAPE[kernel]
    return nw * ng * ngrp * mtw


def rule(M, epi, gate_il, mtw, latency):
    """(kernel, row tiles per workgroup it runs) of a launch of M rows, from the comments of launch_gemm_skinny."""
    tiles = (M + 15) // 16
    mtw = (4 if tiles >= 4 else 2 if tiles >= 2 else 1) if mtw > tiles else mtw         # more than there are tiles: 4, 2 or 1 by the tile count
    mtw = mtw if mtw in (2, 4) else 1                                                  # anything but 2 or 4 is 1
    k = ((SK_GRU_IL2 if mtw >= 2 else SK_GRU_IL) if gate_il else SK_GRU) if epi == EPI_GRU else SK_GRU_PART if epi == EPI_GRU_PART else \
        {4: SK_LIN4, 2: SK_LIN2, 1: SK_LIN_LATENCY if latency else SK_LIN}[mtw]         # the latency kernel: a linear launch at mtw 1 only
    return k, SHAPE[k][3]


def linear_kernel(M, mtw, latency=False):
    """The kernel a linear / ELU launch of M rows at `mtw` must take."""
    return rule(M, EPI_LINEAR, 0, mtw, latency)[0]


def pick(lib, M, epi, gate_il, mtw, latency):
    out = (ctypes.c_int32 * 2)()
    rc = lib.bvc_test_skinny_pick(M, epi, gate_il, mtw, latency, out)
    return rc, (out[0], out[1])


def counts(lib):
    """int64 (2, SK_COUNT): [0] the one-frame launches per kernel so far, [1] the multi-frame ones."""
    out = (ctypes.c_int64 * (2 * (SK_COUNT)))()
    assert lib.bvc_test_skinny_counts(out) == 0
    return np.array(list(out), dtype=np.int64).reshape(2, SK_COUNT)
