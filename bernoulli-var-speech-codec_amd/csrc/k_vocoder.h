// Device helpers shared by the vocoder kernels (k_vocoder.hip: conv_mfma, conv_post; k_vocoder_amp.hip: the AMP pairs): SnakeBeta,
// rows through a buffer descriptor, the 16-byte LDS park, the anti-aliased activation on rows parked in LDS, tile number -> rows, and
// the walk of a persistent AMP kernel's workgroup over its tiles.
#pragma once
#include <type_traits>

#include "bvc_internal.h"

namespace bvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// xs / num_kernels (models.py:225), a true IEEE division like the reference's - in ONE of a stage's nine launches.  The test is uniform,
// but hipcc turns `if (epi == DIV) o = o / d` into the division (a dozen vector instructions per element) on EVERY launch plus a select;
// the empty asm statement cannot be speculated, so the division stays behind a scalar branch (a fifth of these kernels' vector
// instructions were this).
__device__ __forceinline__ void divide_if(bool div, f32x4 &v, float d) {
    if (div) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / d;
    }
}

// tile index -> (batch item, tile of the item): the quotient by a run-time divisor through a host-made reciprocal (one scalar multiply-high)
// instead of hipcc's float-reciprocal emulation of the 32-bit division - some forty vector instructions, per tile and wave in the persistent
// kernels.  Exact while bid * tiles_per_batch < 2^32 (launch_* check it).
__device__ __forceinline__ unsigned div_tpb(unsigned bid, unsigned tpb_magic) { return __umulhi(bid, tpb_magic); }
static inline unsigned tpb_magic_of(unsigned d) { return d <= 1u ? 0xFFFFFFFFu : (unsigned)(0x100000000ull / d) + 1u; }      // (d == 1: q = bid handled by the callers)

// Rows of a channels-last (L, C) signal through a BUFFER descriptor of exactly L * C floats: a row before the start or behind the end of the
// signal is out of the descriptor's range and reads as zeros by itself (also a negative row: its byte offset wraps to a huge unsigned one) -
// no clamping, no compare, no select per item (a third of the vector instructions the tile loads of these kernels issued beside SnakeBeta).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(const float *base, long long L, int C) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (int)(L * C * 4), 0x00020000);
}
__device__ __forceinline__ f32x4 rows_load4(__amdgpu_buffer_rsrc_t rs, int row, int C, int c0) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (row * C + c0) * 4, 0, 0));
}

// sin(x)^2 with |error| < 2.5e-7 (checked against float64 up to |x| = 8060: tests/test_gpu_numerics.py; the reduction
// constants keep their accuracy while k = x*2/pi stays below ~2^17): three-constant Cody-Waite reduction by pi/2 with fma to
// r in [-pi/4, pi/4], then ONE even minimax polynomial sin(r)^2 = u*P(u), u = r^2 (|P error| < 5e-10).  The square removes
// the quadrant sign: sin(x)^2 = sin(r)^2 in even quadrants and 1 - sin(r)^2 in odd ones, i.e. 1/2 -+ (1/2 - sin(r)^2) - so
// h = u*P(u) - 1/2 is computed by the last fma and its sign is flipped for odd quadrants by a multiply with +-1 whose sign bit is
// the quadrant's parity.  k comes from the round-to-nearest of adding 1.5 * 2^23 (no rint, no conversion: the parity is the sum's
// lowest mantissa bit).  14 VALU operations per element, 12 of them packable two elements at a time (round 2: 16 + two
// conversions, two masks and two selects per pair); max |error| 9.7e-8 against 1.1e-7 before (numpy emulation over +-8060).
// ocml's sinf is equally accurate but carries a Payne-Hanek path and costs ~4x the instructions, and the generator evaluates
// 476 of these per output sample on SIMDs whose issue slots it shares with the MFMAs.
__device__ __forceinline__ float sin_squared(float x) {
    const float t = fmaf(x, 0.636619772367581343f, 12582912.0f);
    const float k = t - 12582912.0f;
    float r = fmaf(-k, 1.57079625129699707031e+00f, x);
    r = fmaf(-k, 7.54978941586159635335e-08f, r);
    r = fmaf(-k, 5.39030252995776476554e-15f, r);
    const float u = r * r;
    const float p = fmaf(fmaf(fmaf(fmaf(1.345194032182917e-4f, u, -3.1710113398730755e-3f), u, 4.444364085793495e-2f), u,
                              -3.33333283662796e-1f), u, 1.0f);
    const float h = fmaf(p, u, -0.5f);
    const float sg = __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, t) << 31) | 0x3F800000u);      // -1 in odd quadrants
    return fmaf(h, sg, 0.5f);
}

// SnakeBeta (activations.py:107-120): x + 1/(exp(beta)+1e-9) * sin(x*exp(alpha))^2
__device__ __forceinline__ float snakebeta(float x, float a, float ib) {
    return __fadd_rn(x, __fmul_rn(ib, sin_squared(__fmul_rn(x, a))));
}

// Two elements per lane: the same operations as sin_squared / snakebeta on both halves (bit-identical results),
// written on 2-vectors so that the multiplies and fused multiply-adds become packed-fp32 instructions
// (v_pk_mul_f32 / v_pk_fma_f32: two fp32 lanes per instruction at full rate) - SnakeBeta is ~40 % of the
// generator's vector instructions and shares the SIMD's issue slots with the MFMAs.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(float v) { return (f32x2){v, v}; }
__device__ __forceinline__ f32x2 sin_squared2(f32x2 x) {
    const f32x2 t = __builtin_elementwise_fma(x, splat2(0.636619772367581343f), splat2(12582912.0f));
    const f32x2 nk = splat2(12582912.0f) - t;             // -k
    f32x2 r = __builtin_elementwise_fma(nk, splat2(1.57079625129699707031e+00f), x);
    r = __builtin_elementwise_fma(nk, splat2(7.54978941586159635335e-08f), r);
    r = __builtin_elementwise_fma(nk, splat2(5.39030252995776476554e-15f), r);
    const f32x2 u = r * r;
    f32x2 p = __builtin_elementwise_fma(splat2(1.345194032182917e-4f), u, splat2(-3.1710113398730755e-3f));
    p = __builtin_elementwise_fma(p, u, splat2(4.444364085793495e-2f));
    p = __builtin_elementwise_fma(p, u, splat2(-3.33333283662796e-1f));
    p = __builtin_elementwise_fma(p, u, splat2(1.0f));
    const f32x2 h = __builtin_elementwise_fma(p, u, splat2(-0.5f));
    // +-1 with the quadrant's parity (the sum's lowest mantissa bit) as sign: one v_lshl_or_b32 per element.  Written as asm: from the
    // C expression (bits(t[i]) << 31) | 0x3F800000 on the two elements hipcc 7.2 built ONE such instruction, on element 0, and fed
    // its result to both halves of the packed fma below (op_sel_hi:[1,0,0]) - tests/test_gpu_numerics.py caught it on pairs that
    // straddle a quadrant; the 2-vector integer form is right but takes two instructions per element.
    // (the s_nop: hipcc pads a packed-fp32 result by one state before its next reader and knows nothing about the asm's reads)
    float s0, s1;
    asm("s_nop 0\n\tv_lshl_or_b32 %0, %2, 31, 1.0\n\tv_lshl_or_b32 %1, %3, 31, 1.0" : "=&v"(s0), "=v"(s1) : "v"(t[0]), "v"(t[1]));
    return __builtin_elementwise_fma(h, (f32x2){s0, s1}, splat2(0.5f));
}
__device__ __forceinline__ f32x2 snakebeta2(f32x2 x, f32x2 a, f32x2 ib) {
#pragma clang fp contract(off)
    const f32x2 q = ib * sin_squared2(x * a);
    return x + q;
}

// 16 bytes to / from channels c0 .. c0 + 3 of a row of an LDS tile whose row stride is S floats.  S = C + 2 keeps a row 8-byte aligned
// only, so the granule moves as two 8-byte halves.
template <int S>
__device__ __forceinline__ void park16(float *tile, int row, int c0, f32x4 v) {
    float2 *dst = reinterpret_cast<float2 *>(tile + row * S + c0);
    dst[0] = make_float2(v[0], v[1]);
    dst[1] = make_float2(v[2], v[3]);
}
template <int S>
__device__ __forceinline__ f32x4 parked16(const float *tile, int row, int c0) {
    const float2 lo = *reinterpret_cast<const float2 *>(tile + row * S + c0);
    const float2 hi = *reinterpret_cast<const float2 *>(tile + row * S + c0 + 2);
    return (f32x4){lo.x, lo.y, hi.x, hi.y};
}

// (SnakeBeta of an f32x4, the AMP epilogue value, the rows-before-the-signal clamp, the edge / inner tile pair and the persistent kernels'
// row request stay written out in each kernel: as functions of this header each of them changed the code of some kernel -
// profiles/vocoder_fold.md.)

// Arguments of the AMP-pair kernels (k_vocoder_amp.hip)
struct AmpArgs {
    const float *x; float *out; const float *acc;
    long long L;
    const float *w1, *b1, *a1, *ib1;
    const float *w2, *b2, *a2, *ib2;
    float divisor;
    int epi, ks, dil, tiles_per_batch;
    unsigned tpb_magic;           // tpb_magic_of(tiles_per_batch)
    unsigned ntile;               // workgroups that have a tile (grid is padded to a multiple of 8)
    long long bs;                 // floats between batch items of x / out / acc
    long long row_begin;          // first output row (streaming: rows before it are history)
    long long t_origin;           // global time of buffer row 0 (streaming); 0 offline
    const int *row_age;           // streaming sessions whose rows start at different times: frames since row b's own start (capped where
    int age_rate;                 // no row of a window lies before it any more); row b's t_origin is t_origin + age_rate * row_age[b]
    int row_end;                  // symmetric pair (amp_pair_kernel<..., SYM = true>, whose rows fit 31 bits): one past the last output row - L
                                  // offline; in a look-ahead window L ends the readable input and row_end <= L the rows written.  0 for every
                                  // other kernel: none reads it (it fills the struct's padding: their arguments lie where they lay)
    const float *fu1, *fd1, *fu2, *fd2;   // anti-aliased pair (amp_pair_kernel<..., AA = true>): the 12-tap up / down filters of S1 and S2
};
__device__ __forceinline__ long long amp_t_origin(const AmpArgs &a, int b) {
    return a.row_age ? a.t_origin + (long long)a.age_rate * a.row_age[b] : a.t_origin;
}

// tile number -> batch item b and first output row t0 of the tile; TT = valid output rows per tile
__device__ __forceinline__ void tile_origin(const AmpArgs &a, unsigned bid, int TT, int &b, long long &t0) {
    b = a.tiles_per_batch == 1 ? (int)bid : (int)div_tpb(bid, a.tpb_magic);
    t0 = a.row_begin + (long long)(bid - (unsigned)b * (unsigned)a.tiles_per_batch) * TT;
}

// The walk of a persistent kernel's workgroup over its tiles.  Workgroups are dealt round-robin to the 8 XCDs; neighbouring tiles
// share their halo rows, so each XCD takes a contiguous run of `per` tiles (the halo then hits in that XCD's L2) and its workgroups
// stride through the run.
struct TileWalk {
    unsigned per, nli, xcd, li, run_end;
    __device__ __forceinline__ explicit TileWalk(unsigned ntile) {
        per = (ntile + 7u) >> 3; nli = gridDim.x >> 3;
        xcd = blockIdx.x & 7u;
        li = blockIdx.x >> 3;
        run_end = (xcd + 1u) * per < ntile ? (xcd + 1u) * per : ntile;
    }
    __device__ __forceinline__ unsigned tile() const { return xcd * per + li; }
    __device__ __forceinline__ bool has_tile() const { return tile() < run_end; }       // (uniform)
    __device__ __forceinline__ bool next() { li += nli; return has_tile(); }
};

// ------------------------------------------------------------------------------------------------
// Anti-aliased activation, Activation1d (alias_free_torch/act.py:8-28) around SnakeBeta S, on rows parked in LDS:
//     up[2t]   = 2 sum_k f[2k+1] x[c(t+2-k)],  up[2t+1] = 2 sum_k f[2k] x[c(t+3-k)]     k = 0..5, c = clamp to the signal [0, L-1]
//     a[n]     = S(up[n])                                                                 n in [0, 2L)
//     y[t]     = sum_j g[j] a[clamp(2t-5+j, 0, 2L-1)]                                     j = 0..11
// (resample.py:10-33: replicate pad 5, conv_transpose1d stride 2, times 2, crop 15; filter.py:86-95: replicate pad (5, 6), conv1d
// stride 2).  Two clamps: a position outside [0, 2L) takes a[0] / a[2L-1], not an up value of clamped x.  y[t] reads x[t-5 .. t+5].
// src holds the raw rows [src_first, src_first + nsrc) of the signal (global row numbers; stride S floats, C channels), dst takes
// y of the rows [dst_first, dst_first + ndst); rows before time 0 are written as zeros (the convs' causal padding follows the
// activation).  The caller guarantees that src covers dst's rows -5 .. +5 as far as they lie inside the signal; rows of dst
// behind the signal's end get finite values nobody reads.
// A thread owns two channels and a run of consecutive rows and slides a window of six (a[2t], a[2t+1]) pairs along it, so every
// S(up[n]) is evaluated once per run (plus six pairs of warm-up per run); the packed-fp32 forms carry both channels.
template <int C>
__device__ __forceinline__ void aa_rows(const float *src, int src_first, int nsrc, long long L, float *dst, int dst_first, int ndst,
                                        int S, const float *act_a, const float *act_ib, const float *fu, const float *fd) {
    constexpr int C2 = C / 2, NRUN = 256 / C2;
    const int tid = threadIdx.x;
    const int run = tid / C2, c = (tid - run * C2) * 2;
    const int R = (ndst + NRUN - 1) / NRUN;
    const int j0 = run * R, j1 = j0 + R < ndst ? j0 + R : ndst;
    if (j0 >= j1) return;
    const int last = L - 1 > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)(L - 1);
    const int glo = src_first > 0 ? src_first : 0;                                   // rows of the signal that src holds
    const int ghi = src_first + nsrc - 1 < last ? src_first + nsrc - 1 : last;
    const f32x2 aa = *reinterpret_cast<const f32x2 *>(act_a + c), bb = *reinterpret_cast<const f32x2 *>(act_ib + c);
    float f[12], g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { f[k] = fu[k]; g[k] = fd[k]; }                      // (uniform: scalar registers)
    // the pair (a[2t], a[2t+1]) as the down filter sees it: t outside the signal takes the end value on both places
    auto pair = [&](int t, f32x2 &ev, f32x2 &od) {
        const int tc = t < 0 ? 0 : (t > last ? last : t);
        f32x2 xr[7];                                                                   // x[c(tc-3)] .. x[c(tc+3)]
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            int q = tc - 3 + k;
            q = q < glo ? glo : (q > ghi ? ghi : q);
            xr[k] = *reinterpret_cast<const f32x2 *>(src + (q - src_first) * S + c);
        }
        f32x2 ue = splat2(f[1]) * xr[5], uo = splat2(f[0]) * xr[6];
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            ue = __builtin_elementwise_fma(splat2(f[2 * k + 1]), xr[5 - k], ue);
            uo = __builtin_elementwise_fma(splat2(f[2 * k]), xr[6 - k], uo);
        }
        ev = snakebeta2(ue * splat2(2.0f), aa, bb);
        od = snakebeta2(uo * splat2(2.0f), aa, bb);
        if (t < 0) od = ev;
        if (t > last) ev = od;
    };
    // window for output row t: pairs t-3 .. t+2 (pe / po[0..5]); pair t+3 arrives with the row
    f32x2 pe[6], po[6];
    const int tfirst = dst_first + j0;
#pragma unroll
    for (int k = 0; k < 6; ++k) pair(tfirst - 3 + k, pe[k], po[k]);
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
        const int t = dst_first + j;
        f32x2 ne, no;
        pair(t + 3, ne, no);
        f32x2 y = splat2(g[0]) * po[0];                                               // a[2t-5] = a[2(t-3)+1]
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            y = __builtin_elementwise_fma(splat2(g[2 * k - 1]), pe[k], y);
            y = __builtin_elementwise_fma(splat2(g[2 * k]), po[k], y);
        }
        y = __builtin_elementwise_fma(splat2(g[11]), ne, y);                          // a[2t+6] = a[2(t+3)]
        if (t < 0) y = splat2(0.0f);
        *reinterpret_cast<float2 *>(dst + j * S + c) = make_float2(y[0], y[1]);
#pragma unroll
        for (int k = 0; k < 5; ++k) { pe[k] = pe[k + 1]; po[k] = po[k + 1]; }
        pe[5] = ne; po[5] = no;
    }
}

// occupancy of every persistent AMP kernel instance, once, outside any stream capture (conv_kernels_init; k_vocoder_amp.hip)
int amp_kernels_init();

}  // namespace bvc
