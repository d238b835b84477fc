// Device helpers shared by the dense GEMM kernels (k_gemm.hip, k_gemm_batched.hip, k_rows.hip) and the persistent recurrence
// (k_flow.hip).  The head of k_gemm.hip promises the same bits whichever kernel computes a layer: the product and the activations
// it speaks of are the ones below, written once.
#pragma once
#include "bvc_internal.h"

namespace bvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float elu1(float v) { return v > 0.0f ? v : expf(v) - 1.0f; }
__device__ __forceinline__ float sigmoid1(float v) { return 1.0f / (1.0f + expf(-v)); }

// offset (in floats) of element (m, n) of a fragment-packed [.][ld] matrix
__device__ __forceinline__ long long packed_off(int m, int n, long long ld) {
    return ((((long long)(m >> 4) * (ld >> 4) + (n >> 4)) * 64 + ((n & 15) >> 2) * 16 + (m & 15)) << 2) + (n & 3);
}

}  // namespace bvc
