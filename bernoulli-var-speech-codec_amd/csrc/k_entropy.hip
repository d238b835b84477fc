// The entropy-coded wire format for gfx950: a binary range coder with carry propagation that codes every bit of a frame under the
// probability the prior net gives it (bvc_internal.h states the format).  Bytes and integers only behind the quantisation of p.
//
//  entropy_encode_kernel       - one lane per (row, segment), serial over the segment's frames and positions; nothing of it depends on
//                                the recurrence, so all segments run in one launch behind the pass that produced the probabilities.
//  entropy_decode_kernel       - the same walk backwards, on a given probability tensor (bvc_entropy_decode).
//  entropy_decode_step_kernel  - ONE frame of all rows, a node of the receive program's step (OP_ENTROPY_DECODE): one wave per row.  The
//                                wave fetches the frame's probabilities and the row's byte window - a frame consumes at most
//                                2 * z_dim + 4 bytes - into LDS with independent loads, lane 0 runs the serial loop out of LDS, and the
//                                wave stores z_t.  The coder's state of a row (code, range, bytes consumed) lives in the call's workspace.
//
// All three share the coder below.  Reads are bounded by the segment's size (a byte at or beyond it is 0), writes by its stride.
#include "bvc_internal.h"

namespace bvc {

namespace {

constexpr unsigned EC_TOP = 1u << 24;

// P(bit = 1) in 16 bits; the product is exact in float32, rintf is round-half-even, a NaN quantises to 1
__device__ __forceinline__ unsigned ec_quant(float p) { return (unsigned)fminf(fmaxf(rintf(p * 65536.0f), 1.0f), 65535.0f); }

// positions of a frame that carry a bit: those with bits > n, n = 0 .. Z - 1
__device__ __forceinline__ int ec_nbits(float bits, int Z) { return bits >= (float)Z ? Z : (bits > 0.0f ? (int)ceilf(bits) : 0); }

// sizes[] as the decoder takes it: an entry outside [0, stride] reads as no bytes
__device__ __forceinline__ long long ec_size(int size, long long stride) { return (size < 0 || size > stride) ? 0 : size; }

struct EcEnc {
    unsigned long long low;
    unsigned range, cache;
    long long cache_size, emitted, size;      // emitted: bytes so far, the unstored first one included; size: behind the last non-zero stored byte
    unsigned char *out;
    long long stride;
    bool over;

    __device__ __forceinline__ void init(unsigned char *o, long long st) {
        low = 0; range = 0xFFFFFFFFu; cache = 0; cache_size = 1; emitted = 0; size = 0; out = o; stride = st; over = false;
    }
    __device__ __forceinline__ void emit(unsigned v) {
        v &= 0xFFu;
        const long long i = emitted++ - 1;    // (the first byte is always 0 and is not stored)
        if (i < 0 || !v) return;              // zeros are what the cleared buffer holds
        if (i < stride) out[i] = (unsigned char)v; else over = true;
        size = i + 1;
    }
    __device__ __forceinline__ void shift_low() {
        if ((unsigned)low < 0xFF000000u || (low >> 32) != 0) {
            const unsigned carry = (unsigned)(low >> 32);
            emit(cache + carry);
            for (; cache_size > 1; --cache_size) emit(0xFFu + carry);
            cache = (unsigned)(low >> 24) & 0xFFu;
            cache_size = 0;
        }
        cache_size += 1;
        low = (low & 0x00FFFFFFull) << 8;
    }
    __device__ __forceinline__ void bit(int b, unsigned q) {
        const unsigned bound = (range >> 16) * (65536u - q);
        if (!b) range = bound;
        else { low += bound; range -= bound; }
        while (range < EC_TOP) { shift_low(); range <<= 8; }
    }
    __device__ __forceinline__ int finish() {
        for (int i = 0; i < 5; ++i) shift_low();
        return over ? -1 : (int)size;
    }
};

// src(i): byte i of the segment, 0 at or beyond its size
struct EcDec {
    unsigned code, range;
    long long pos;

    template <typename Src>
    __device__ __forceinline__ void init(Src src) {
        range = 0xFFFFFFFFu; code = 0;
        for (int i = 0; i < 4; ++i) code = (code << 8) | src((long long)i);
        pos = 4;
    }
    template <typename Src>
    __device__ __forceinline__ int bit(unsigned q, Src src) {
        const unsigned bound = (range >> 16) * (65536u - q);
        int b = 0;
        if (code < bound) range = bound;
        else { code -= bound; range -= bound; b = 1; }
        while (range < EC_TOP) { code = (code << 8) | src(pos++); range <<= 8; }
        return b;
    }
};

struct EcShape { int B, Z; long long T, S; int nseg; };

// one lane per (row, segment)
__global__ __launch_bounds__(64) void entropy_encode_kernel(const float *__restrict__ codes, const float *__restrict__ prob,
                                                            const float *__restrict__ bits, float bpf, EcShape g,
                                                            unsigned char *__restrict__ data, long long stride, int *__restrict__ sizes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)g.B * g.nseg) return;
    const int b = (int)(i / g.nseg), sg = (int)(i - (long long)b * g.nseg);
    const long long t0 = (long long)sg * g.S, t1 = t0 + g.S < g.T ? t0 + g.S : g.T;
    EcEnc e;
    e.init(data + i * stride, stride);
    for (long long t = t0; t < t1; ++t) {
        const long long bt = (long long)b * g.T + t;
        const int n = ec_nbits(bits ? bits[bt] : bpf, g.Z);
        const float *c = codes + bt * g.Z, *p = prob + bt * g.Z;
        for (int j = 0; j < n; j += 4) {              // (Z is a multiple of 4: the loads of four positions go out together)
            float cv[4], pv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { cv[k] = c[j + k]; pv[k] = p[j + k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) if (j + k < n) e.bit(cv[k] > 0.5f, ec_quant(pv[k]));
        }
    }
    sizes[i] = e.finish();
}

__global__ __launch_bounds__(64) void entropy_decode_kernel(const unsigned char *__restrict__ data, long long stride, const int *__restrict__ sizes,
                                                            const float *__restrict__ prob, const float *__restrict__ bits, float bpf,
                                                            EcShape g, float *__restrict__ codes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)g.B * g.nseg) return;
    const int b = (int)(i / g.nseg), sg = (int)(i - (long long)b * g.nseg);
    const long long t0 = (long long)sg * g.S, t1 = t0 + g.S < g.T ? t0 + g.S : g.T;
    const unsigned char *seg = data + i * stride;
    const long long size = ec_size(sizes[i], stride);
    auto src = [&](long long k) -> unsigned { return k < size ? seg[k] : 0u; };
    EcDec d;
    d.init(src);
    for (long long t = t0; t < t1; ++t) {
        const long long bt = (long long)b * g.T + t;
        const int n = ec_nbits(bits ? bits[bt] : bpf, g.Z);
        const float *p = prob + bt * g.Z;
        float *c = codes + bt * g.Z;
        for (int j = 0; j < g.Z; j += 4) {
            float pv[4], cv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = j + k < n ? p[j + k] : 0.5f;
#pragma unroll
            for (int k = 0; k < 4; ++k) cv[k] = j + k < n ? (float)d.bit(ec_quant(pv[k]), src) : 0.5f;
#pragma unroll
            for (int k = 0; k < 4; ++k) c[j + k] = cv[k];
        }
    }
}

// One wave per row.  Dynamic LDS: q [Z] unsigned, z [Z] float, the byte window [2 Z + 8]
__global__ __launch_bounds__(64) void entropy_decode_step_kernel(EntropyStep a, int tstep) {
    extern __shared__ unsigned ec_lds[];
    const int t = a.desc->t + tstep;
    const long long T = a.desc->T;
    const int b = blockIdx.x, lane = threadIdx.x, Z = a.Z;
    if (t < 0 || t >= T || b >= a.B) return;
    const float *prob = a.desc->p[DS_PROB], *bits = a.desc->p[DS_BITS];
    float *codes = a.desc->p[DS_CODES];
    if (!prob || !bits || !codes) return;
    unsigned *q = ec_lds;
    float *z = reinterpret_cast<float *>(ec_lds + Z);
    unsigned char *win = reinterpret_cast<unsigned char *>(ec_lds + 2 * Z);
    const EntropyCall c = *a.call;
    const long long bt = (long long)b * T + t;
    const int sg = t / c.segment;
    const long long seg_i = (long long)b * c.nseg + sg;
    // everything the frame needs, requested before anything is used: the state, the size, the bit count, the probabilities
    const uint4 st = *reinterpret_cast<const uint4 *>(a.state + 4 * b);
    const bool fresh = t - sg * c.segment == 0 || st.y < EC_TOP;      // (a normalised range is never below 2^24: the loops below end)
    const int size_raw = c.sizes[seg_i];
    const float nb = bits[bt];
    for (int j = lane; j < Z; j += 64) q[j] = ec_quant(prob[bt * Z + j]);
    const int n = ec_nbits(nb, Z);
    const long long size = ec_size(size_raw, c.stride);
    const unsigned char *seg = c.data + seg_i * c.stride;
    const long long pos0 = fresh ? 0 : (long long)st.z;
    const int wlen = 2 * n + (fresh ? 4 : 0);
    for (int k = lane; k < wlen; k += 64) win[k] = pos0 + k < size ? seg[pos0 + k] : (unsigned char)0;
    __syncthreads();
    if (lane == 0) {
        auto src = [&](long long k) -> unsigned { return win[k]; };      // k counts from pos0: never beyond wlen
        EcDec d;
        if (fresh) d.init(src);
        else { d.code = st.x; d.range = st.y; d.pos = 0; }
        for (int j = 0; j < n; ++j) z[j] = (float)d.bit(q[j], src);
        *reinterpret_cast<uint4 *>(a.state + 4 * b) = make_uint4(d.code, d.range, (unsigned)(pos0 + d.pos), 0u);
    }
    __syncthreads();
    for (int j = lane; j < Z; j += 64) codes[bt * Z + j] = j < n ? z[j] : 0.5f;
}

__global__ void entropy_set_call_kernel(EntropyCall *d, EntropyCall v) {
    if (threadIdx.x == 0) *d = v;
}

__global__ void entropy_bits_kernel(const float *__restrict__ bits, float dflt, long long n, float *__restrict__ sel) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = bits ? bits[i] : dflt;
        sel[i] = v > 0.0f ? v : 0.0f;
    }
}

int ec_shape(int B, long long T, int Z, long long S, long long stride, EcShape *g) {
    if (B <= 0 || T <= 0 || Z <= 0 || (Z & 3) || S < 1 || stride < 0 || stride > 0x7FFFFFFFll) {
        set_error("entropy coder: B=%d T=%lld z_dim=%d segment=%lld stride=%lld: positive sizes, z_dim a multiple of 4, segment >= 1, 0 <= stride < 2^31",
                  B, T, Z, S, stride);
        return BVC_EINVAL;
    }
    if (S > T) S = T;
    *g = EcShape{B, Z, T, S, (int)((T + S - 1) / S)};
    return BVC_OK;
}

}  // namespace

int launch_entropy_set_call(EntropyCall *d, const EntropyCall &v, hipStream_t s) {
    hipLaunchKernelGGL(entropy_set_call_kernel, dim3(1), dim3(64), 0, s, d, v);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_entropy_bits(const float *bits, float dflt, long long n, float *sel, hipStream_t s) {
    if (n <= 0) return BVC_OK;
    const int grid = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
    hipLaunchKernelGGL(entropy_bits_kernel, dim3(grid), dim3(256), 0, s, bits, dflt, n, sel);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_entropy_decode_step(const EntropyStep &a, int tstep, hipStream_t s) {
    if (a.B <= 0 || a.Z <= 0 || !a.desc || !a.call || !a.state) { set_error("entropy decode step: bad arguments"); return BVC_EINVAL; }
    const size_t lds = (size_t)a.Z * 8 + (size_t)2 * a.Z + 8;
    hipLaunchKernelGGL(entropy_decode_step_kernel, dim3(a.B), dim3(64), lds, s, a, tstep);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_entropy_encode(const float *codes, const float *prob, const float *bits, float bits_per_frame, int B, long long T, int Z,
                          long long segment, unsigned char *data, long long stride, int *sizes, hipStream_t s) {
    EcShape g;
    if (int rc = ec_shape(B, T, Z, segment, stride, &g)) return rc;
    const long long lanes = (long long)B * g.nseg;
    if (stride > 0) BVC_HIP_TRY(hipMemsetAsync(data, 0, (size_t)lanes * (size_t)stride, s));
    hipLaunchKernelGGL(entropy_encode_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, codes, prob, bits, bits_per_frame, g, data, stride, sizes);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_entropy_decode(const unsigned char *data, long long stride, const int *sizes, const float *prob, const float *bits,
                          float bits_per_frame, int B, long long T, int Z, long long segment, float *codes, hipStream_t s) {
    EcShape g;
    if (int rc = ec_shape(B, T, Z, segment, stride, &g)) return rc;
    const long long lanes = (long long)B * g.nseg;
    hipLaunchKernelGGL(entropy_decode_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, data, stride, sizes, prob, bits, bits_per_frame, g, codes);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
