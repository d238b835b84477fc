// Kernels of the optimiser step and of the in-place rewrite of a live model's weights (optimizer.hip): the copy of many tensors in one
// launch (the gather of bvc_bvrnn_params_get, the scatter of the natural forms), the GRU's gate-interleaved packing and the float64
// fold of dec.6 -> norm -> phi_x.0 as weight_pack.h computes them on the host, the two-stage 2-norm of the flat gradient buffer and
// the AdamW update of the whole flat buffer.  Every store is an ordinary vector store; no atomics: the order of every sum is a
// function of the sizes alone.  Every tensor of the flat layout starts at a multiple of 16 floats and has a
// multiple of 16 of them (all dimensions are multiples of 16), so the flat kernels move 16-byte granules and have no tail.
#include "k_gemm.h"

namespace bvc {

namespace {

int blocks_for4(long long n4, int cap = 4096) {
    const long long b = (n4 + 255) / 256;
    return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// segment blockIdx.y: n floats (a multiple of 4) from src to dst, both 16-byte aligned
__global__ __launch_bounds__(256) void copy_segments_kernel(CopySegments segs) {
    const CopySegment sg = segs.s[blockIdx.y];
    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(sg.src);
    float4 *__restrict__ dst = reinterpret_cast<float4 *>(sg.dst);
    const long long n4 = sg.n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i];
}

// pack_gru_interleaved (weight_pack.h): W [3H][K] -> [H/16][K/16][gate][lane][4]; one thread per granule of four k
__global__ __launch_bounds__(256) void pack_gru_il_kernel(const float *__restrict__ W, int H, int K, float *__restrict__ out) {
    const long long n4 = (long long)3 * H * K / 4;
    const int k4s = K / 4, nb = K / 16;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % k4s) * 4;
        const long long row = i / k4s;                     // q * H + n
        const int q = (int)(row / H), n = (int)(row % H);
        const float4 v = *reinterpret_cast<const float4 *>(W + row * K + k);
        const long long o = ((((long long)(n >> 4) * nb + (k >> 4)) * 3 + q) * 64 + ((k & 15) >> 2) * 16 + (n & 15)) << 2;
        *reinterpret_cast<float4 *>(out + o) = v;
    }
}

// fold_px0_dec3 (weight_pack.h), bit for bit: row n of W = phi_x.0.W diag(1 / std) dec.6.W and b[n], in float64 with the host's
// operations - g_j = (double)wp0[n][j] / (double)std[j], the sums over j ascending, every product and every sum rounded on its own (the
// host code is baseline x86-64, which has no fused multiply-add; the device compiler contracts unless told otherwise), one rounding to
// float at the end.  One workgroup per row n; W goes straight to its fragment-packed place.
__global__ __launch_bounds__(256) void fold_px0_dec3_kernel(const float *__restrict__ wp0, const float *__restrict__ bp0,
                                                            const float *__restrict__ wd6, const float *__restrict__ bd6,
                                                            const float *__restrict__ mean, const float *__restrict__ stdv, int H, int X,
                                                            float *__restrict__ wp_out, float *__restrict__ b_out) {
#pragma clang fp contract(off)
    __shared__ double g[128];                              // X <= 128 (check_config)
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < X; j += blockDim.x) g[j] = (double)wp0[(long long)n * X + j] / (double)stdv[j];
    __syncthreads();
    // (plain operators under the pragma: the header's __dmul_rn / __dadd_rn are inline x * y and x + y of ANOTHER scope, and contract)
    for (int k = threadIdx.x; k < H; k += blockDim.x) {
        double acc = 0.0;
        for (int j = 0; j < X; ++j) {
            const double prod = g[j] * (double)wd6[(long long)j * H + k];
            acc = acc + prod;
        }
        wp_out[packed_off(n, k, H)] = (float)acc;
    }
    if (threadIdx.x == 0) {
        double b = (double)bp0[n];
        for (int j = 0; j < X; ++j) {
            const double prod = g[j] * ((double)bd6[j] - (double)mean[j]);
            b = b + prod;
        }
        b_out[n] = (float)b;
    }
}

// fixed-order sum of a workgroup's 256 doubles
__device__ __forceinline__ double block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// stage 1 of the norm: partial[c] = sum of g^2 over chunk c of NORM_CHUNK floats, float64; thread t takes the granules t, t + 256, ...
__global__ __launch_bounds__(256) void norm_partial_kernel(const float *__restrict__ g, long long n4, double *__restrict__ partial) {
    __shared__ double red[256];
    const float4 *__restrict__ g4 = reinterpret_cast<const float4 *>(g);
    const long long c0 = (long long)blockIdx.x * (NORM_CHUNK / 4);
    const long long c1 = c0 + NORM_CHUNK / 4 < n4 ? c0 + NORM_CHUNK / 4 : n4;
    double acc = 0.0;
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
        const float4 v = g4[i];
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// stage 2 (one workgroup): norm = sqrt(sum of the partials), thread t taking t, t + 256, ...; scal[0] = the factor every gradient is
// scaled by, min(1, max_norm / (norm + 1e-6)) (1 without clipping), scal[1] = the norm
__global__ __launch_bounds__(256) void norm_final_kernel(const double *__restrict__ partial, int chunks, float max_norm, float *__restrict__ scal,
                                                         float *__restrict__ norm_out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < chunks; i += 256) acc += partial[i];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        double c = 1.0;
        if (max_norm > 0.0f) { c = (double)max_norm / (norm + 1e-6); c = c < 1.0 ? c : 1.0; }
        scal[0] = (float)c;
        scal[1] = (float)norm;
        if (norm_out) *norm_out = (float)norm;
    }
}

__device__ __forceinline__ void adam_one(float &p, float &m, float &v, float g, const AdamScalars &a) {
#pragma clang fp contract(off)
    p = p * a.decay;
    m = a.b1 * m + a.one_b1 * g;
    v = a.b2 * v + (a.one_b2 * g) * g;
    p = p - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

// AdamW over the whole flat buffer: every tensor in one launch.  g is read, scaled by the device-resident factor, and left alone.
__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ g,
                                                   const float *__restrict__ scal, long long n4, AdamScalars a) {
#pragma clang fp contract(off)
    const float c = scal[0];
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam_one(pp.x, mm.x, vv.x, gg.x * c, a);
        adam_one(pp.y, mm.y, vv.y, gg.y * c, a);
        adam_one(pp.z, mm.z, vv.z, gg.z * c, a);
        adam_one(pp.w, mm.w, vv.w, gg.w * c, a);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
}

}  // namespace

int launch_copy_segments(const CopySegments &segs, hipStream_t s) {
    if (segs.n <= 0) return BVC_OK;
    long long nmax = 0;
    for (int i = 0; i < segs.n; ++i) nmax = segs.s[i].n > nmax ? segs.s[i].n : nmax;
    if (nmax <= 0) return BVC_OK;
    hipLaunchKernelGGL(copy_segments_kernel, dim3(blocks_for4(nmax / 4, 1024), segs.n), dim3(256), 0, s, segs);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_pack_gru_interleaved(const float *W, int H, int K, float *out, hipStream_t s) {
    hipLaunchKernelGGL(pack_gru_il_kernel, dim3(blocks_for4((long long)3 * H * K / 4)), dim3(256), 0, s, W, H, K, out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_fold_px0_dec3(const float *wp0, const float *bp0, const float *wd6, const float *bd6, const float *mean, const float *stdv, int H,
                         int X, float *wp_out, float *b_out, hipStream_t s) {
    if (X > 128) { set_error("the fold kernel takes num_mels <= 128 (got %d)", X); return BVC_EINVAL; }
    hipLaunchKernelGGL(fold_px0_dec3_kernel, dim3(H), dim3(256), 0, s, wp0, bp0, wd6, bd6, mean, stdv, H, X, wp_out, b_out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int norm_chunks(long long total) { return (int)((total + NORM_CHUNK - 1) / NORM_CHUNK); }

int launch_grad_norm(const float *g, long long total, float max_norm, double *partial, float *scal, float *norm_out, hipStream_t s) {
    const int chunks = norm_chunks(total);
    hipLaunchKernelGGL(norm_partial_kernel, dim3(chunks), dim3(256), 0, s, g, total / 4, partial);
    BVC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(256), 0, s, partial, chunks, max_norm, scal, norm_out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_adam(float *p, float *m, float *v, const float *g, const float *scal, long long total, const AdamScalars &a, hipStream_t s) {
    hipLaunchKernelGGL(adam_kernel, dim3(blocks_for4(total / 4)), dim3(256), 0, s, p, m, v, g, scal, total / 4, a);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
