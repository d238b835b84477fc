// Closed-loop rate selection (bvc_bvrnn_encode_vbr) for gfx950: the two kernels that sit between the recurrent-layer GEMMs of a frame,
// and the wire format that carries a per-frame bit count.
//
//  vbr_candidates_kernel - from the frame's unmasked code z = round(p) (EPI_CODE with var_bit off) the K masked copies
//                          z^k = z on positions < n_k, 0.5 behind them, as candidate rows k * B + b of a fragment-packed matrix
//                          (the operand layout of phi_z.0), and h_t K times over (the h half of dec.0 on the same rows).
//  vbr_select_kernel     - one wave per utterance: D_k = mean_j |d^k_j - y_j| of every rung in float32, the first rung with
//                          D_k <= tau (else the last), then the frame's results - D, bits, codes, decoded mel - and the chosen rung's
//                          rows of phi_z and of the normalised mel, gathered into B-row operands of phi_x.0 and the GRU.
//
// The order of D's summation is fixed and depends on the row alone: lane l adds the bands l, l + 64, ... in ascending order, the 64
// partial sums meet in a butterfly (partners 32, 16, 8, 4, 2, 1 lanes apart), the sum is divided by num_mels.  Rows are independent:
// neither kernel reads a fragment row at or beyond its row count, and neither writes one.
#include "k_gemm.h"

namespace bvc {

namespace {

struct VbrFrame { int t; long long T; bool ok; };

__device__ __forceinline__ VbrFrame vbr_frame(const VbrStep &a, int tstep) {
    if (!a.desc) return {0, 1, true};
    const int t = a.desc->t + tstep;
    const long long T = a.desc->T;
    return {t, T, t >= 0 && t < T};
}

// z under a mask of n leading bits (k_gemm.hip, EPI_CODE: a NaN stays a NaN under the mask too)
__device__ __forceinline__ float vbr_mask(float z, int j, int n) { return j < n ? z : (z != z ? z : 0.5f); }

// one thread per (candidate row, granule of four columns) of [zc | hrep]
__global__ __launch_bounds__(256) void vbr_candidates_kernel(VbrStep a, int tstep) {
    const VbrFrame f = vbr_frame(a, tstep);
    if (!f.ok) return;
    const int gz = a.Z >> 2, gh = a.H >> 2, per_row = gz + gh;
    const long long total = (long long)a.K * a.B * per_row;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / per_row), g = (int)(i - (long long)row * per_row);
    const int k = row / a.B, b = row - k * a.B;
    if (g < gz) {
        const int j = g << 2;
        const int n = a.call->ladder[k];
        const f32x4 z = *reinterpret_cast<const f32x4 *>(a.zraw + packed_off(b, j, a.Z));
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = vbr_mask(z[e], j + e, n);
        *reinterpret_cast<f32x4 *>(a.zc + packed_off(row, j, a.Z)) = o;
    } else {
        const int j = (g - gz) << 2;
        const float *h = a.hbuf + ((f.t & 1) ? a.MH : 0);
        *reinterpret_cast<f32x4 *>(a.hrep + packed_off(row, j, a.H)) = *reinterpret_cast<const f32x4 *>(h + packed_off(b, j, a.H));
    }
}

// one wave per utterance
__global__ __launch_bounds__(64) void vbr_select_kernel(VbrStep a, int tstep) {
    const VbrFrame f = vbr_frame(a, tstep);
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!f.ok || b >= a.B) return;
    const VbrCall &c = *a.call;
    const long long bt = (long long)b * f.T + f.t;
    const float *y = c.y + bt * a.X;
    const float tau = c.tau[bt];
    int choice = a.K - 1;
    bool found = false;
    for (int k = 0; k < a.K; ++k) {
        const float *d = a.melk + (long long)(k * a.B + b) * a.X;
        float sum = 0.0f;
        for (int j = lane; j < a.X; j += 64) sum += fabsf(d[j] - y[j]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float D = sum / (float)a.X;
        if (c.dist && lane == 0) c.dist[bt * a.K + k] = D;
        if (!found && D <= tau) { choice = k; found = true; }       // (a NaN on either side compares false)
    }
    if (c.capped) {
        // the row's token bucket, in q8 integers (every lane computes the same numbers, lane 0 keeps them): never more than it holds
        long long tok = (long long)c.tok[b] + c.rate_q8;
        if (tok > c.burst_q8) tok = c.burst_q8;
        int afford = 0;
        for (int k = 1; k < a.K; ++k) if ((long long)c.ladder[k] * 256 <= tok) afford = k;
        if (afford < choice) choice = afford;
        tok -= (long long)c.ladder[choice] * 256;
        if (lane == 0) c.tok[b] = tok > 0 ? (int)tok : 0;
    }
    const int n = c.ladder[choice];
    const int row = choice * a.B + b;
    if (lane == 0) {
        if (c.bits) c.bits[bt] = (float)n;
        if (c.choice) c.choice[bt] = choice;
    }
    if (c.codes && a.zraw)
        for (int j = lane; j < a.Z; j += 64) c.codes[bt * a.Z + j] = vbr_mask(a.zraw[packed_off(b, j, a.Z)], j, n);
    if (c.dec)
        for (int j = lane; j < a.X; j += 64) c.dec[bt * a.X + j] = a.melk[(long long)row * a.X + j];
    if (a.pzk && a.pzsel)
        for (int j = lane << 2; j < a.H; j += 256)
            *reinterpret_cast<f32x4 *>(a.pzsel + packed_off(b, j, a.H)) = *reinterpret_cast<const f32x4 *>(a.pzk + packed_off(row, j, a.H));
    if (a.dnk && a.dnsel)
        for (int j = lane << 2; j < a.X; j += 256)
            *reinterpret_cast<f32x4 *>(a.dnsel + packed_off(b, j, a.X)) = *reinterpret_cast<const f32x4 *>(a.dnk + packed_off(row, j, a.X));
}

__global__ void vbr_set_call_kernel(VbrCall *d, VbrCall v) {
    if (threadIdx.x == 0) *d = v;
}

__device__ __forceinline__ int vbr_nbits(float v, int z) { return v >= (float)z ? z : (v > 0.0f ? (int)v : 0); }

// one thread per byte of a frame's stride
__global__ void pack_codes_vbr_kernel(const float *__restrict__ codes, const float *__restrict__ bits, long long frames, int z, int stride,
                                      unsigned char *__restrict__ out, int *__restrict__ sizes) {
    const long long total = frames * stride;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long f = i / stride;
        const int j = (int)(i - f * stride);
        const int n = vbr_nbits(bits[f], z);
        unsigned v = 0;
        if (j == 0) {
            v = (unsigned)n;
            if (sizes) sizes[f] = 1 + ((n + 7) >> 3);
        } else {
            for (int q = 0; q < 8; ++q) {
                const int bit = (j - 1) * 8 + q;
                if (bit < n && codes[f * z + bit] > 0.75f) v |= 1u << q;
            }
        }
        out[i] = (unsigned char)v;
    }
}

// one thread per code position; a header above z reads as z, so no read leaves the frame's stride
__global__ void unpack_codes_vbr_kernel(const unsigned char *__restrict__ in, long long frames, int z, int stride, float *__restrict__ codes,
                                        float *__restrict__ bits) {
    const long long total = frames * z;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long f = i / z;
        const int bit = (int)(i - f * z);
        const unsigned char *fr = in + f * stride;
        const int h = fr[0];
        const int n = h > z ? z : h;
        codes[i] = bit < n ? (float)((fr[1 + (bit >> 3)] >> (bit & 7)) & 1u) : 0.5f;
        if (bits && bit == 0) bits[f] = (float)n;
    }
}

// the rows' buckets into or out of the call's workspace: dst[b] = src ? src[b] : fill
__global__ void vbr_tok_kernel(int *__restrict__ dst, const int *__restrict__ src, int fill, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) dst[b] = src ? src[b] : fill;
}

// ---- the same wire inside a streaming tick (bvc_stream_codec_create_vbr): codes (B, k, z) and bits (B, k) of the tick, frame j of row b
// at (b * kstride + j) * stride of the packet buffer; sizes and the bit counts as floats at b * kstride + j.  One thread per byte.
__global__ void sc_pack_rows_vbr_kernel(const float *__restrict__ codes, const float *__restrict__ bits, int B, int k, int z, int stride, int kstride,
                                        unsigned char *__restrict__ out, int *__restrict__ sizes, float *__restrict__ bits_out) {
    const long long total = (long long)B * k * stride;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long f = i / stride;
        const int y = (int)(i - f * stride);
        const int b = (int)(f / k), j = (int)(f - (long long)b * k);
        const long long pf = (long long)b * kstride + j;
        const int n = vbr_nbits(bits[f], z);
        unsigned v = 0;
        if (y == 0) {
            v = (unsigned)n;
            if (sizes) sizes[pf] = 1 + ((n + 7) >> 3);
            if (bits_out) bits_out[pf] = (float)n;
        } else {
            for (int q = 0; q < 8; ++q) {
                const int bit = (y - 1) * 8 + q;
                if (bit < n && codes[f * z + bit] > 0.75f) v |= 1u << q;
            }
        }
        if (out) out[pf * stride + y] = (unsigned char)v;
    }
}

// one thread per code position.  A frame that did not arrive (present == 0) has no header: it is a frame of no bits, and so is every
// frame of an idle row (row_off[b] < 0).  A header above z reads as z, so no read leaves the frame's stride.
__global__ void sc_unpack_rows_vbr_kernel(const unsigned char *__restrict__ in, const unsigned char *__restrict__ present,
                                          const int *__restrict__ row_off, int B, int k, int z, int stride, int kstride,
                                          float *__restrict__ codes, float *__restrict__ bits_out) {
    const long long total = (long long)B * k * z;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long f = i / z;
        const int bit = (int)(i - f * z);
        const int b = (int)(f / k), j = (int)(f - (long long)b * k);
        const long long pf = (long long)b * kstride + j;
        const unsigned char *fr = in + pf * stride;
        int n = 0;
        if (row_off[b] >= 0 && present[pf] != 0) { const int h = fr[0]; n = h > z ? z : h; }
        codes[i] = bit < n ? (float)((fr[1 + (bit >> 3)] >> (bit & 7)) & 1u) : 0.5f;
        if (bits_out && bit == 0) bits_out[pf] = (float)n;
    }
}

int vbr_step_ok(const VbrStep &a) {
    if (a.B <= 0 || a.K < 1 || a.K > VBR_MAX_RUNGS || a.X <= 0 || (a.Z & 15) || (a.H & 15) || (a.dnk && (a.X & 15))) {
        set_error("vbr: B=%d K=%d Z=%d H=%d X=%d: 1..%d rungs, packed rows in multiples of 16", a.B, a.K, a.Z, a.H, a.X, VBR_MAX_RUNGS);
        return BVC_EINVAL;
    }
    return BVC_OK;
}

}  // namespace

int launch_vbr_set_call(VbrCall *d, const VbrCall &v, hipStream_t s) {
    hipLaunchKernelGGL(vbr_set_call_kernel, dim3(1), dim3(64), 0, s, d, v);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_vbr_tok(int *dst, const int *src, int fill, int B, hipStream_t s) {
    if (B <= 0 || !dst || dst == src) return BVC_OK;
    hipLaunchKernelGGL(vbr_tok_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, dst, src, fill, B);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_pack_rows_vbr(const float *codes, const float *bits, int B, int k, int z, int kstride, unsigned char *out, int *sizes,
                         float *bits_out, hipStream_t s) {
    const int stride = 1 + (z + 7) / 8;
    const long long total = (long long)B * k * stride;
    if (total <= 0) return BVC_OK;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(sc_pack_rows_vbr_kernel, dim3(grid), dim3(256), 0, s, codes, bits, B, k, z, stride, kstride, out, sizes, bits_out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_unpack_rows_vbr(const unsigned char *in, const unsigned char *present, const int *row_off, int B, int k, int z, int kstride,
                           float *codes, float *bits_out, hipStream_t s) {
    const int stride = 1 + (z + 7) / 8;
    const long long total = (long long)B * k * z;
    if (total <= 0) return BVC_OK;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(sc_unpack_rows_vbr_kernel, dim3(grid), dim3(256), 0, s, in, present, row_off, B, k, z, stride, kstride, codes, bits_out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_vbr_candidates(const VbrStep &a, int tstep, hipStream_t s) {
    if (int rc = vbr_step_ok(a)) return rc;
    const long long total = (long long)a.K * a.B * ((a.Z + a.H) >> 2);
    hipLaunchKernelGGL(vbr_candidates_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, tstep);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_vbr_select(const VbrStep &a, int tstep, hipStream_t s) {
    if (int rc = vbr_step_ok(a)) return rc;
    hipLaunchKernelGGL(vbr_select_kernel, dim3(a.B), dim3(64), 0, s, a, tstep);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_pack_codes_vbr(const float *codes, const float *bits, long long frames, int z, unsigned char *out, int *sizes, hipStream_t s) {
    const int stride = 1 + (z + 7) / 8;
    const long long total = frames * stride;
    if (total <= 0) return BVC_OK;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(pack_codes_vbr_kernel, dim3(grid), dim3(256), 0, s, codes, bits, frames, z, stride, out, sizes);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_unpack_codes_vbr(const unsigned char *in, long long frames, int z, float *codes, float *bits, hipStream_t s) {
    const int stride = 1 + (z + 7) / 8;
    const long long total = frames * z;
    if (total <= 0) return BVC_OK;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(unpack_codes_vbr_kernel, dim3(grid), dim3(256), 0, s, in, frames, z, stride, codes, bits);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
