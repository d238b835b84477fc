// Batched GEMMs of the BVRNN for gfx950: a layer over ALL frames of a call (phi_x at bvrnn.py:178, phi_z, the pre-computed halves),
// M = B*T rows.  Same products and the same order of summation per output as the recurrent-step kernels (head of k_gemm.hip).
//
//  gemm_batched_kernel      - 128x128 workgroup tile, 64x64 per wave (4x4 MFMA tiles), operands loaded as k-contiguous float4
//                             fragments: the register-only form (the K = 64 / 80 first layers, odd shapes).
//  gemm_batched_cols_kernel - the K = 1024 layers, through LDS: four waves along the columns, tile height picked per launch by
//                             gemm_batched_cut so that the grid fills whole rounds of the workgroup slots.
//  gemm_batched_lds_kernel  - through LDS, 2 x 2 waves: the quarter / half tiles of the two-launch cut, and the `legacy` cut.
//
// Host side, below the kernels: the switches (gemm_switches), the cost model of the row cut (gemm_batched_cut, a pure function),
// ONE table of the LDS kernels' instantiations, and launch_gemm_batched = validation, then cut, then launch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "k_gemm.h"

namespace bvc {

// Where element (row, col) of a batched GEMM goes (GemmOut):
//   GO_NATURAL           y[row][col]
//   GO_FRAME_MAJOR_ROWS  rows come utterance-major (row = b*T + t) and leave frame-major (row' = t*mt16 + b):
//                        the following layers then see whole 16-utterance groups of ONE frame per row tile
//   GO_PACKED_FRAMES     rows are frame-major (row = t*mt16 + b); frame t is written as the fragment-packed
//                        [mt16][N] matrix the recurrent kernels read: a 16x16 MFMA tile is one 1 KiB block
//   GO_PACKED_FROM_UTT   utterance-major rows straight to packed frames (16-byte granules; small jobs only)
__device__ __forceinline__ long long out_index(int row, int col, int N, long long ldy, long long T, int mt16, int mode) {
    if (mode == GO_NATURAL) return (long long)row * ldy + col;
    if (mode == GO_FRAME_MAJOR_ROWS) {
        const long long bb = row / T, tt = row - bb * T;
        return (tt * mt16 + bb) * ldy + col;
    }
    if (mode == GO_PACKED_FRAMES) {
        const int tt = row / mt16, bb = row - tt * mt16;
        return (long long)tt * mt16 * N + packed_off(bb, col, N);
    }
    const long long bb = row / T, tt = row - bb * T;
    return tt * (long long)mt16 * N + packed_off((int)bb, col, N);
}
// The same layout with the row part computed once per output row (gemm_batched_cols_kernel):
//     out_at(out_row(row), col) == out_index(row, col)   for every mode.
// Both forms are written out, and a change of the layout is made in both: out_index divides by the 64-bit T, out_row by its 32-bit
// value, so out_index defined as out_at(out_row(..)) is other device code in the 14 kernels that call it (profiles/gemm_fold.md).
struct OutRow { long long base; int bb; };
__device__ __forceinline__ OutRow out_row(int row, int N, long long ldy, long long T, int mt16, int mode) {
    if (mode == GO_NATURAL) return {(long long)row * ldy, 0};
    if (mode == GO_PACKED_FRAMES) {
        const int tt = row / mt16;
        return {(long long)tt * mt16 * N, row - tt * mt16};
    }
    const int Ti = (int)T;                               // (T divides M: it fits an int, and the division stays a 32-bit one)
    const int bb = row / Ti;
    const long long tt = row - bb * Ti;
    if (mode == GO_FRAME_MAJOR_ROWS) return {(tt * mt16 + bb) * ldy, 0};
    return {tt * (long long)mt16 * N, bb};
}
__device__ __forceinline__ long long out_at(const OutRow &o, int col, int N, int mode) {
    return mode <= GO_FRAME_MAJOR_ROWS ? o.base + col : o.base + packed_off(o.bb, col, N);
}

// The epilogue's value: bias, then the activation (ACT 1: ELU).  The 16-byte form serves the two LDS kernels; the register-only
// kernel's ROWVEC epilogue keeps the same lines written out (as a call, hipcc orders gemm_batched_kernel<1, true> differently).
template <int ACT>
__device__ __forceinline__ f32x4 bias_act4(f32x4 acc, f32x4 b4) {
    f32x4 v = acc + b4;
    if (ACT == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = elu1(v[e]);
    }
    return v;
}
template <int ACT>
__device__ __forceinline__ float bias_act1(float acc, float b) {
    float v = acc + b;
    if (ACT == 1) v = elu1(v);
    return v;
}

// ------------------------------------------------------------------------------------------------
// Batched GEMM: y[M,N] = act(x[M,K] @ w[N,K]^T + bias).  128x128 per workgroup, 64x64 per wave.
// ROWVEC (GO_NATURAL output, N and ldy multiples of 4): the MFMA operands are swapped (tile of y^T = w x^T), so that a lane's four
// results are four CONSECUTIVE COLUMNS of one output row and leave as one 16-byte store (the K = 64 / 80 first layers are bound by
// their 113 MB of output: 64 four-byte stores per lane otherwise).  Same products, same order of summation per output.
template <int ACT, bool ROWVEC = false>
__global__ __launch_bounds__(256, 2) void gemm_batched_kernel(const float *__restrict__ x, long long ldx,
                                                           const float *__restrict__ w, long long ldw,
                                                           const float *__restrict__ bias, int M, int N,
                                                           int K, float *__restrict__ y, long long ldy,
                                                           long long frames_T, int mt16, int out_mode) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.y * 128 + (wave >> 1) * 64;
    const int n0 = blockIdx.x * 128 + (wave & 1) * 64;
    if (m0 >= M || n0 >= N) return;                                  // wave-uniform

    f32x4 acc[4][4], tot[4][4];                          // the running chunk | the sum of the finished chunks (head of this file)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    const float *xp[4];
    const float *wp[4];
    bool xok[4], wok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + i * 16 + r;
        xok[i] = row < M;
        xp[i] = x + (long long)(xok[i] ? row : (M - 1)) * ldx + g * 4;
        const int col = n0 + i * 16 + r;
        wok[i] = col < N;
        wp[i] = w + (long long)(wok[i] ? col : (N - 1)) * ldw + g * 4;
    }
    // The fragments of k-block kb+1 are requested before block kb is multiplied (unconditionally: past the end the last block
    // is read again), so that only the first request's latency is exposed - these are the K = 64 / 80 first layers, five blocks.
    const int nblk = K >> 4;
    int chunk = 0, cend = nblk >> 3;                       // chunk c = blocks [nblk*c/8, nblk*(c+1)/8)
    while (cend == 0) { ++chunk; cend = (nblk * (chunk + 1)) >> 3; }
    bool first_chunk = true;
    f32x4 xv[4], wv[4], xn[4], wn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xv[i] = *reinterpret_cast<const f32x4 *>(xp[i]);
        wv[i] = *reinterpret_cast<const f32x4 *>(wp[i]);
    }
    // one k-block; START: the block opens a chunk - its first MFMA per tile starts from zero (no accumulator to clear)
    auto block = [&](auto start_c) {
        constexpr bool START = decltype(start_c)::value;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 c = (START && e == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[i][j];
                    acc[i][j] = ROWVEC ? mfma16(wv[j][e], xv[i][e], c) : mfma16(xv[i][e], wv[j][e], c);
                }
    };
    bool cstart = true;
#pragma unroll 1
    for (int kb = 0; kb < nblk; ++kb) {
        const long long nxt = (long long)(kb + 1 < nblk ? kb + 1 : nblk - 1) * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xn[i] = *reinterpret_cast<const f32x4 *>(xp[i] + nxt);
            wn[i] = *reinterpret_cast<const f32x4 *>(wp[i] + nxt);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (cstart) block(std::true_type());
        else        block(std::false_type());
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) { xv[i] = xn[i]; wv[i] = wn[i]; }
        cstart = kb + 1 == cend;
        if (cstart) {                                      // (uniform) block kb ends chunk `chunk`: add it to the sum
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) tot[i][j] = first_chunk ? acc[i][j] : tot[i][j] + acc[i][j];
            first_chunk = false;
            do { ++chunk; cend = (nblk * (chunk + 1)) >> 3; } while (chunk < 7 && cend == kb + 1);     // (empty chunks: K < 128)
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j];
    if (ROWVEC) {                                          // acc[i][j][e] = y[m0 + 16 i + r][n0 + 16 j + 4 g + e]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + i * 16 + r;
            if (row >= M) continue;
            float *yr = y + (long long)row * ldy + n0 + g * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + j * 16 + g * 4;
                if (col >= N) continue;
                const f32x4 b4 = bias ? *reinterpret_cast<const f32x4 *>(bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
                f32x4 v = acc[i][j] + b4;
                if (ACT == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = elu1(v[e]);
                }
                *reinterpret_cast<f32x4 *>(yr + j * 16) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + j * 16 + r;
        if (col >= N) continue;
        const float b = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + i * 16 + g * 4 + e;
                if (row < M) {
                    const float v = bias_act1<ACT>(acc[i][j][e], b);
                    y[out_index(row, col, N, ldy, frames_T, mt16, out_mode)] = v;
                }
            }
    }
}

// LDS-tiled variant for the large layers (K a multiple of 32, N a multiple of 128): 128x128 tile, 32-deep
// stages, two LDS buffers.  The next stage travels global -> registers while the current one feeds the
// MFMAs, and is parked in the other LDS buffer afterwards (one barrier per stage).  Rows are padded to
// 36 floats so that the 16-byte fragment reads of 8 consecutive lanes cover all banks.  The k order seen
// by each accumulator is the one of gemm_batched_kernel (16-blocks in order, k = 4*g + e inside), so both
// produce the same bits: eight chunks of K/8, each a chain from zero, added in order (head of this file).
// BM: rows per workgroup tile, 128 or 64 (the half-height form finishes the last, partly filled round of a launch: see
// launch_gemm_batched); m_off: first row of this launch's tiles.
template <int ACT, int BM, bool ROWVEC = false>
__global__ __launch_bounds__(256, 2) void gemm_batched_lds_kernel(const float *__restrict__ x, long long ldx,
                                                                  const float *__restrict__ w, long long ldw,
                                                                  const float *__restrict__ bias, int M, int N,
                                                                  int K, float *__restrict__ y, long long ldy,
                                                                  long long frames_T, int mt16, int out_mode, int m_off) {
    constexpr int BK = 32, LDT = BK + 4;                 // floats per LDS row
    static_assert(BM == 128 || BM == 64 || BM == 32, "tile heights");
    constexpr int MI = BM / 32;                          // 16-row MFMA tiles per wave (waves: 2 along M x 2 along N)
    constexpr int PA = BM / 32;                          // staging passes of 32 rows for the A operand
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][A BMxLDT | B 128xLDT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int mblk = m_off + blockIdx.y * BM, nblk = blockIdx.x * 128;
    const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * 64;

    // global staging: thread -> (row = tid/8 + 32*p, 16-byte piece tid%8) of the BM x 32 / 128 x 32 stage of the operands
    const int srow = tid >> 3, spc = (tid & 7) * 4;
    const float *xg[PA], *wg[4];
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int row = mblk + srow + 32 * p;
        xg[p] = x + (long long)(row < M ? row : M - 1) * ldx + spc;      // rows past M: re-read the last one, never stored
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) wg[p] = w + (long long)(nblk + srow + 32 * p) * ldw + spc;
    f32x4 acc[MI][4], tot[MI][4];                        // the running chunk | the sum of the finished chunks (head of this file)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    constexpr int STAGE = (BM + 128) * LDT;              // floats per LDS buffer
    f32x4 ga[PA], gb[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int p = 0; p < PA; ++p) ga[p] = *reinterpret_cast<const f32x4 *>(xg[p] + (long long)kt * BK);
#pragma unroll
        for (int p = 0; p < 4; ++p) gb[p] = *reinterpret_cast<const f32x4 *>(wg[p] + (long long)kt * BK);
    };
    auto park = [&](int buf) {
        float *A = smem + buf * STAGE, *B = A + BM * LDT;
#pragma unroll
        for (int p = 0; p < PA; ++p) *reinterpret_cast<f32x4 *>(A + (srow + 32 * p) * LDT + spc) = ga[p];
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4 *>(B + (srow + 32 * p) * LDT + spc) = gb[p];
    };
    const int nk = K / BK;
    const int cst = nk >> 3;                             // stages per chunk (K is a multiple of 256: launch_gemm_batched)
    gload(0);
    park(0);
    __syncthreads();
    // one 32-deep stage; FIRST: the stage opens a chunk - its first MFMA per tile starts from zero (no accumulator to clear)
    auto stage = [&](int kt, auto first_c) {
        constexpr bool FIRST = decltype(first_c)::value;
        const float *A = smem + (kt & 1) * STAGE + (wm + r) * LDT + g * 4;
        const float *B = smem + (kt & 1) * STAGE + BM * LDT + (wn + r) * LDT + g * 4;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 av[MI], bv[4];
#pragma unroll
            for (int i = 0; i < MI; ++i) av[i] = *reinterpret_cast<const f32x4 *>(A + i * 16 * LDT + h * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const f32x4 *>(B + i * 16 * LDT + h * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 c = (FIRST && h == 0 && e == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[i][j];
                        acc[i][j] = ROWVEC ? mfma16(bv[j][e], av[i][e], c) : mfma16(av[i][e], bv[j][e], c);
                    }
        }
    };
    int in_chunk = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) gload(kt + 1);
        if (in_chunk == 0) stage(kt, std::true_type());
        else               stage(kt, std::false_type());
        if (++in_chunk == cst) {                         // (uniform) the chunk is complete: add it to the sum
            in_chunk = 0;
            if (kt < cst) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) tot[i][j] = acc[i][j];
            } else {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) tot[i][j] += acc[i][j];
            }
        }
        if (more) park((kt + 1) & 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j];

    const int m0 = mblk + wm, n0 = nblk + wn;
    if (ROWVEC) {           // operands swapped (tile of y^T): acc[i][j][e] = y[m0 + 16 i + r][n0 + 16 j + 4 g + e], one 16-byte granule in every
#pragma unroll              // output layout (see gemm_batched_kernel)
        for (int i = 0; i < MI; ++i) {
            const int row = m0 + i * 16 + r;
            if (row >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + j * 16 + g * 4;
                const f32x4 b4 = bias ? *reinterpret_cast<const f32x4 *>(bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
                const f32x4 v = bias_act4<ACT>(acc[i][j], b4);
                *reinterpret_cast<f32x4 *>(y + out_index(row, col, N, ldy, frames_T, mt16, out_mode)) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + j * 16 + r;
        const float b = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + i * 16 + g * 4 + e;
                if (row < M) {
                    const float v = bias_act1<ACT>(acc[i][j][e], b);
                    y[out_index(row, col, N, ldy, frames_T, mt16, out_mode)] = v;
                }
            }
    }
}

// The same tile with the four waves side by side along the COLUMNS (each BM x 32: BM / 16 row tiles x 2 column tiles), so that
// BM is any multiple of 16 - 144 rows put the layers of the benchmark shapes on whole rounds of the 512 workgroup slots
// (launch_gemm_batched) - and with the LDS reads run as a pipeline: a 32-deep stage is 2 * BM / 16 steps of eight MFMAs (one A
// fragment against the two B fragments of its half), the A fragment of step s + D and the B fragments of the next half are
// requested before step s is multiplied (a few steps ahead: D below), and the stage's barrier stands D steps before its end - every read of the
// current buffer has been issued by then - so that the first fragments of the next stage travel under the last MFMAs of this
// one.  The barrier is a bare s_barrier behind lgkmcnt(0): the global loads of stage kt + 2 stay in flight across it.
// Same products in the same order per accumulator as gemm_batched_lds_kernel: the same bits.
template <int ACT, int BM, bool ROWVEC = false>
__global__ __launch_bounds__(256, 2) void gemm_batched_cols_kernel(const float *__restrict__ x, long long ldx,
                                                                   const float *__restrict__ w, long long ldw,
                                                                   const float *__restrict__ bias, int M, int N,
                                                                   int K, float *__restrict__ y, long long ldy,
                                                                   long long frames_T, int mt16, int out_mode, int m_off) {
    constexpr int BK = 32, LDT = BK + 4;                 // floats per LDS row
    static_assert(BM % 16 == 0 && BM >= 48 && BM <= 144, "tile heights: 2 x 2 x (BM + 128) x 36 floats of LDS per CU");
    constexpr int MI = BM / 16;                          // 16-row MFMA tiles per wave
    constexpr int PA = (BM + 31) / 32;                   // staging passes of 32 rows for the A operand (the last one may be half used)
    constexpr int NS = 2 * MI;                           // steps per stage
    constexpr int RING = NS % 4 == 0 ? 4 : NS % 6 == 0 ? 6 : NS % 5 == 0 ? 5 : 7;      // A fragments in flight: step s lives in slot
    constexpr int D = RING - 1;                          // s % RING in every stage, so RING divides the steps of a stage
    static_assert(NS % RING == 0 && MI >= D && NS - D >= MI, "fragment ring");
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][A BMxLDT | B 128xLDT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int mblk = m_off + blockIdx.y * BM, nblk = blockIdx.x * 128;
    const int wn = wave * 32;

    // global staging through buffer loads: 32-bit lane offsets, the stage (and the weights' pass) go into the scalar offset - half
    // the address registers of nine 64-bit pointers
    const int srow = tid >> 3, spc = (tid & 7) * 4;
    const int xrows = M - mblk < PA * 32 ? M - mblk : PA * 32;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x + (long long)mblk * ldx), 0, (int)(xrows * ldx * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w + (long long)nblk * ldw), 0, (int)(128 * ldw * 4), 0x00020000);
    int xvo[PA];                                         // rows past M re-read the last one (never stored)
#pragma unroll
    for (int p = 0; p < PA; ++p) xvo[p] = ((srow + 32 * p < xrows ? srow + 32 * p : xrows - 1) * (int)ldx + spc) * 4;
    const int wvo = (srow * (int)ldw + spc) * 4;
    f32x4 acc[MI][2], tot[MI][2];                        // the running chunk | the sum of the finished chunks (head of this file)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    constexpr int STAGE = (BM + 128) * LDT;              // floats per LDS buffer
    const int nk = K / BK;
    const int cst = nk >> 3;                             // stages per chunk (K is a multiple of 256: launch_gemm_batched)
    f32x4 ga[PA], gb[4];
    auto gload = [&](int kt) {                           // unconditional: past the end the last stage is read again
        const int ko = (kt < nk ? kt : nk - 1) * BK;
#pragma unroll
        for (int p = 0; p < PA; ++p) ga[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xvo[p], ko * 4, 0));
#pragma unroll
        for (int p = 0; p < 4; ++p) gb[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wvo, (32 * p * (int)ldw + ko) * 4, 0));
    };
    auto park = [&](float *A) {
        float *B = A + BM * LDT;
#pragma unroll
        for (int p = 0; p < PA; ++p)
            if (32 * (p + 1) <= BM || srow + 32 * p < BM) *reinterpret_cast<f32x4 *>(A + (srow + 32 * p) * LDT + spc) = ga[p];
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4 *>(B + (srow + 32 * p) * LDT + spc) = gb[p];
    };
    auto lds_barrier = [&]() {                           // LDS visibility only: no vmcnt(0)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    const int fo = r * LDT + g * 4;                      // this lane's fragment piece inside a 16-row tile
    auto lda = [&](const float *buf, int s) {            // A fragment of step s: row tile s % MI, half s / MI
        return *reinterpret_cast<const f32x4 *>(buf + fo + (s % MI) * 16 * LDT + (s / MI) * 16);
    };
    auto ldb = [&](const float *buf, int h, int j) {
        return *reinterpret_cast<const f32x4 *>(buf + fo + (BM + wn + j * 16) * LDT + h * 16);
    };
    f32x4 ring[RING], bq[2][2];
    gload(0);
    park(smem);
    gload(1);
    lds_barrier();
#pragma unroll
    for (int s = 0; s < D; ++s) ring[s] = lda(smem, s);
#pragma unroll
    for (int j = 0; j < 2; ++j) bq[0][j] = ldb(smem, 0, j);

    // one 32-deep stage
    auto stage = [&](int kt) {
        const float *cur = smem + (kt & 1) * STAGE;
        float *nxt = smem + ((kt + 1) & 1) * STAGE;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int h = s / MI, i = s % MI;
            if (s == NS - D) {                           // every read of `cur` has been issued: stage kt + 1 may land in `nxt`
                park(nxt);
                __builtin_amdgcn_sched_barrier(0);       // (the staging registers are free again only behind the writes)
                gload(kt + 2);
                lds_barrier();
#pragma unroll
                for (int j = 0; j < 2; ++j) bq[0][j] = ldb(nxt, 0, j);
            }
            if (s == MI - D) {
#pragma unroll
                for (int j = 0; j < 2; ++j) bq[1][j] = ldb(cur, 1, j);
            }
            ring[(s + D) % RING] = s + D < NS ? lda(cur, s + D) : lda(nxt, s + D - NS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = ROWVEC ? mfma16(bq[h][j][e], ring[s % RING][e], acc[i][j]) : mfma16(ring[s % RING][e], bq[h][j][e], acc[i][j]);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // A chunk's chain starts from a cleared accumulator and the sum of the chunks from zero: a chain that starts from +0 never
    // ends in -0, so 0 + chunk 0 has the bits of the copy the other kernels make.
    int in_chunk = 0;
    for (int kt = 0; kt < nk; ++kt) {
        stage(kt);
        if (++in_chunk == cst) {                         // (uniform) the chunk is complete: add it to the sum
            in_chunk = 0;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        }
    }

    const int n0 = nblk + wn;
    if (ROWVEC) {           // operands swapped (tile of y^T): tot[i][j][e] = y[mblk + 16 i + r][n0 + 16 j + 4 g + e], one 16-byte granule in every
        f32x4 b4[2];        // output layout (see gemm_batched_kernel)
#pragma unroll
        for (int j = 0; j < 2; ++j) b4[j] = bias ? *reinterpret_cast<const f32x4 *>(bias + n0 + j * 16 + g * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int row = mblk + i * 16 + r;
            if (row >= M) continue;
            const OutRow o = out_row(row, N, ldy, frames_T, mt16, out_mode);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 v = bias_act4<ACT>(tot[i][j], b4[j]);
                *reinterpret_cast<f32x4 *>(y + out_at(o, n0 + j * 16 + g * 4, N, out_mode)) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = mblk + i * 16 + g * 4 + e;
            if (row >= M) continue;
            const OutRow o = out_row(row, N, ldy, frames_T, mt16, out_mode);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + j * 16 + r;
                const float v = bias_act1<ACT>(tot[i][j][e], (bias ? bias[col] : 0.0f));
                y[out_at(o, col, N, out_mode)] = v;
            }
        }
}

// ---- the switches of the batched GEMM (host only), all read here and nowhere else:
//   once per process    BVC_NO_LDS_GEMM      the register-only kernel for every shape (A/B switch for the profiles)
//                       BVC_NO_GEMM_TAIL     no half- / quarter-height tiles for the last round (a single launch of 128-row tiles)
//                       BVC_NO_GEMM_QUARTER  half-height tail tiles only
//                       BVC_TILE_TRACE       one line per distinct launch shape on stderr (profiles/tile_rounds.md)
//   at every call       BVC_TILE_CUT=legacy  the cuts of before the plan (128-row tiles of gemm_batched_lds_kernel plus a tail
//                                            launch; one AMP tile shape per channel count) for A/B runs
//                       BVC_GEMM_BM          one compiled tile height forced
//   (the last two: tests flip them inside one process and compare the results)
GemmSwitches gemm_switches() {
    static const bool no_lds = getenv("BVC_NO_LDS_GEMM") != nullptr, no_tail = getenv("BVC_NO_GEMM_TAIL") != nullptr,
                      no_quarter = getenv("BVC_NO_GEMM_QUARTER") != nullptr, trace = getenv("BVC_TILE_TRACE") != nullptr;
    const char *cut = getenv("BVC_TILE_CUT");
    return {no_lds, no_tail, no_quarter, trace, cut != nullptr && cut[0] == 'l', getenv("BVC_GEMM_BM")};
}

bool tile_cut_legacy() { return gemm_switches().legacy; }

void tile_trace(const char *what, long long rows, long long cols, int height, int tail_height, long long tiles, int slots, long long rounds) {
    if (!gemm_switches().trace) return;
    static long long seen[64][4];
    static int nseen = 0;
    const long long key[4] = {(long long)what[0] * 256 + what[1], rows, cols, height * 1000 + tail_height};
    for (int i = 0; i < nseen; ++i)
        if (seen[i][0] == key[0] && seen[i][1] == key[1] && seen[i][2] == key[2] && seen[i][3] == key[3]) return;
    if (nseen < 64) { for (int q = 0; q < 4; ++q) seen[nseen][q] = key[q]; ++nseen; }
    fprintf(stderr, "tile_trace %s rows=%lld cols=%lld height=%d tail_height=%d tiles=%lld slots=%d rounds=%lld (%.2f needed)\n", what, rows, cols,
            height, tail_height, tiles, slots, rounds, (double)tiles / slots);
}

// ---- how launch_gemm_batched cuts the rows (host only, a pure function of its arguments; tile_plan in bvc_internal.h)
GemmCut g_last_gemm_cut = {0, 0, 0, 0, 0, 0};
// fixed: rows' worth of time a tile costs whatever its height (prologue fill, epilogue), fitted from the 144- and 112-row tiles
// (3 rounds in 465.0 us against 4 rounds in 483.5 us: 1.4 rows; profiles/tile_rounds.md).  The tail launch of the two-launch cut runs at a lower rate than the main one (the same 128-column
// weight stage for a quarter / half of the products): a quarter tile costs 0.46, a half tile 0.55 of a full one (measured).
static constexpr int GEMM_FIXED_ROWS = 1;
static constexpr int GEMM_SLOTS = 512;                    // two workgroups per CU
GemmCut gemm_batched_cut(int M, int N, int force_height, bool legacy, bool no_tail, bool no_q) {
    GemmCut c = {0, 0, 0, 0, 0, 0};
    if (M <= 0 || N < 128) return c;
    const int ncol = N / 128, rows_blk = (M + 127) / 128;
    // the two-launch cut: 128-row tiles for the full rounds, the rows of a partly filled last round as quarter / half tiles
    const int per_round = GEMM_SLOTS / ncol > 0 ? GEMM_SLOTS / ncol : 1;     // row blocks per full round
    int full_blk = rows_blk;
    if (!no_tail && rows_blk > per_round && rows_blk % per_round != 0 && (rows_blk % per_round) * 2 <= per_round)   // the half tiles fit ONE round
        full_blk = (rows_blk / per_round) * per_round;
    GemmCut two = {128, full_blk, 0, 0, 0, 0};
    two.tiles = (long long)ncol * full_blk;
    two.rounds = (two.tiles + GEMM_SLOTS - 1) / GEMM_SLOTS;
    two.cost100 = two.rounds * 100 * (128 + GEMM_FIXED_ROWS);
    if (full_blk < rows_blk) {
        const int m_off = full_blk * 128;
        const long long q_tiles = (long long)ncol * ((M - m_off + 31) / 32), h_tiles = (long long)ncol * ((M - m_off + 63) / 64);
        const bool quarter = !no_q && q_tiles <= 768;     // three quarter-height workgroups fit a CU
        two.tail_height = quarter ? 32 : 64;
        const long long t_tiles = quarter ? q_tiles : h_tiles, t_slots = quarter ? 768 : GEMM_SLOTS;
        const long long t_rounds = (t_tiles + t_slots - 1) / t_slots;
        two.tiles += t_tiles; two.rounds += t_rounds;
        two.cost100 += t_rounds * (quarter ? 46 : 55) * (128 + GEMM_FIXED_ROWS);
    }
    if (legacy && force_height == 0) return two;
    static const int heights[3] = {144, 128, 112}, slots[3] = {GEMM_SLOTS, GEMM_SLOTS, GEMM_SLOTS};
    TilePlan p;
    if (force_height) {
        int one = 0;
        for (int h : heights) if (h == force_height) one = h;
        if (!one) return c;
        p = tile_plan(M, ncol, &one, slots, 1, GEMM_FIXED_ROWS);
    } else {
        p = tile_plan(M, ncol, heights, slots, 3, GEMM_FIXED_ROWS);
    }
    if (!force_height && two.tail_height != 0 && two.cost100 < p.cost * 100) return two;
    c.height = p.height; c.full_blocks = (M + p.height - 1) / p.height; c.tail_height = 0;
    c.tiles = p.tiles; c.rounds = p.rounds; c.cost100 = p.cost * 100;
    return c;
}

// ---- the launch: validation, then cut, then launch
struct BatchedArgs {
    const float *x; long long ldx; const float *w; long long ldw; const float *bias;
    int M, N, K, act; float *y; long long ldy; hipStream_t s; int out_mode; long long frames_T; int mt16;
};

// The instantiations of the two LDS kernels, keyed by (family, ACT, BM, ROWVEC): the only place the host names one.  The two
// families share a signature, so batched_kernels_init and launch_lds_tiles work on the looked-up pointer.
typedef void (*BatchedLdsFn)(const float *, long long, const float *, long long, const float *, int, int, int, float *, long long, long long,
                             int, int, int);
enum GemmFamily { GF_LDS = 0, GF_COLS = 1 };
struct BatchedKernel {
    int family, act, bm; bool rowvec;
    BatchedLdsFn fn;
    size_t lds() const { return (size_t)2 * (bm + 128) * 36 * sizeof(float); }         // two buffers of A BM x 36 | B 128 x 36
};
#define BVC_BATCHED(FAMILY, KERNEL, BM) {FAMILY, 0, BM, false, KERNEL<0, BM, false>}, {FAMILY, 1, BM, false, KERNEL<1, BM, false>}, \
                                        {FAMILY, 0, BM, true, KERNEL<0, BM, true>},   {FAMILY, 1, BM, true, KERNEL<1, BM, true>}
static const BatchedKernel BATCHED_KERNELS[] = {
    BVC_BATCHED(GF_LDS, gemm_batched_lds_kernel, 128),  BVC_BATCHED(GF_LDS, gemm_batched_lds_kernel, 64),
    BVC_BATCHED(GF_LDS, gemm_batched_lds_kernel, 32),
    BVC_BATCHED(GF_COLS, gemm_batched_cols_kernel, 144), BVC_BATCHED(GF_COLS, gemm_batched_cols_kernel, 128),
    BVC_BATCHED(GF_COLS, gemm_batched_cols_kernel, 112),
};
static const BatchedKernel *batched_kernel(int family, int act, int bm, bool rowvec) {
    for (const BatchedKernel &k : BATCHED_KERNELS)
        if (k.family == family && k.act == act && k.bm == bm && k.rowvec == rowvec) return &k;
    return nullptr;
}

// Every tile of the table needs more dynamic LDS than a kernel gets unasked (BM = 32 apart): allowed once per process, from whichever
// thread launches first (launch_gemm_batched holds the result in a function-local static).
static int batched_kernels_init() {
    for (const BatchedKernel &k : BATCHED_KERNELS)
        BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds()));
    return BVC_OK;
}

static int batched_validate(const BatchedArgs &a) {
    if (a.K % 16 || a.ldx % 4 || a.ldw % 4) {
        set_error("gemm_batched: K=%d ldx=%lld ldw=%lld must be multiples of 16/4/4", a.K, a.ldx, a.ldw);
        return BVC_EINVAL;
    }
    if (a.out_mode == GO_NATURAL) return BVC_OK;
    const bool utt_rows = a.out_mode == GO_FRAME_MAJOR_ROWS || a.out_mode == GO_PACKED_FROM_UTT;
    if (a.mt16 <= 0 || a.mt16 % 16 || a.N % 16 || (utt_rows && (a.frames_T <= 0 || a.M % a.frames_T || a.M / a.frames_T > a.mt16)) ||
        (a.out_mode == GO_PACKED_FRAMES && a.M % a.mt16)) {
        set_error("gemm_batched: inconsistent frame layout (M=%d T=%lld mt16=%d N=%d mode=%d)", a.M, a.frames_T, a.mt16, a.N, a.out_mode);
        return BVC_EINVAL;
    }
    return BVC_OK;
}

// 16-byte epilogue stores (operands swapped, see gemm_batched_kernel) whenever the output granules are aligned.  The LDS kernels
// store a granule in every output layout; the register-only kernel's ROWVEC form writes natural rows only (natural_only).
static bool stores_16_bytes(const BatchedArgs &a, bool natural_only) {
    const auto aligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return (!natural_only || a.out_mode == GO_NATURAL) && a.N % 4 == 0 && a.ldy % 4 == 0 && aligned(a.y) && (!a.bias || aligned(a.bias));
}

// the register-only kernel: four instantiations, [ACT][ROWVEC]
static int launch_batched_regs(const BatchedArgs &a) {
    typedef void (*Fn)(const float *, long long, const float *, long long, const float *, int, int, int, float *, long long, long long, int, int);
    static const Fn kernels[2][2] = {{gemm_batched_kernel<0, false>, gemm_batched_kernel<0, true>},
                                     {gemm_batched_kernel<1, false>, gemm_batched_kernel<1, true>}};
    const dim3 grid((a.N + 127) / 128, (a.M + 127) / 128);
    hipLaunchKernelGGL(kernels[a.act == 1][stores_16_bytes(a, true)], grid, dim3(256), 0, a.s, a.x, a.ldx, a.w, a.ldw, a.bias, a.M, a.N, a.K,
                       a.y, a.ldy, a.frames_T, a.mt16, a.out_mode);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// How the rows are cut (gemm_batched_cut above), recorded for the tests and the trace
static int batched_cut(const BatchedArgs &a, const GemmSwitches &sw, GemmCut *cut) {
    const int force = sw.gemm_bm ? atoi(sw.gemm_bm) : 0;
    *cut = gemm_batched_cut(a.M, a.N, force, sw.legacy, sw.no_tail, sw.no_quarter);
    if (sw.gemm_bm && cut->height != force) { set_error("gemm_batched: BVC_GEMM_BM=%s is not a compiled tile height", sw.gemm_bm); return BVC_EINVAL; }
    g_last_gemm_cut = *cut;
    tile_trace("gemm_batched", a.M, a.N, cut->height, cut->tail_height, cut->tiles, 512, cut->rounds);
    return BVC_OK;
}

// `blocks` row blocks of bm rows from row m_off on, on the kernel of `family`
static int launch_lds_tiles(const BatchedArgs &a, int family, int bm, int blocks, int m_off) {
    const BatchedKernel *k = batched_kernel(family, a.act == 1, bm, stores_16_bytes(a, false));
    if (!k) { set_error("gemm_batched: no kernel for tiles of %d rows", bm); return BVC_EINVAL; }
    const dim3 grid(a.N / 128, blocks);
    hipLaunchKernelGGL(k->fn, grid, dim3(256), k->lds(), a.s, a.x, a.ldx, a.w, a.ldw, a.bias, a.M, a.N, a.K, a.y, a.ldy, a.frames_T, a.mt16,
                       a.out_mode, m_off);
    return BVC_OK;
}

// One launch of the column-layout kernel at the height that fills whole rounds, or 128-row tiles plus a second launch of quarter /
// half tiles for the last round.  The `legacy` cut keeps its 128-row tiles on gemm_batched_lds_kernel; its tail is whatever rows
// its cut.full_blocks blocks of 128 leave (with a forced height as well: cut.tail_height is 0 then, and half tiles run).
static int launch_batched_cut(const BatchedArgs &a, const GemmCut &cut, bool legacy) {
    int rc = BVC_OK;
    if (!legacy)                   rc = launch_lds_tiles(a, GF_COLS, cut.height, cut.full_blocks, 0);
    else if (cut.full_blocks > 0)  rc = launch_lds_tiles(a, GF_LDS, 128, cut.full_blocks, 0);
    if (rc) return rc;
    const int m_off = cut.full_blocks * 128;
    if (legacy ? m_off < a.M : cut.tail_height != 0) {
        const int bm = cut.tail_height == 32 ? 32 : 64;
        if ((rc = launch_lds_tiles(a, GF_LDS, bm, (a.M - m_off + bm - 1) / bm, m_off))) return rc;
    }
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_gemm_batched(const float *x, long long ldx, const float *w, long long ldw, const float *bias,
                        int M, int N, int K, int act, float *y, long long ldy, hipStream_t s, int out_mode,
                        long long frames_T, int mt16) {
    if (M <= 0) return BVC_OK;
    const BatchedArgs a = {x, ldx, w, ldw, bias, M, N, K, act, y, ldy, s, out_mode, frames_T, mt16};
    if (int rc = batched_validate(a)) return rc;
    ProbeScope probe(PK_BATCHED, s);
    const GemmSwitches sw = gemm_switches();
    if (sw.no_lds || K % 256 != 0 || N % 128 != 0) return launch_batched_regs(a);      // (LDS: eight chunks of whole 32-deep stages)
    static const int init_rc = batched_kernels_init();
    if (init_rc) { set_error("gemm_batched: the LDS limits of the batched kernels could not be raised"); return init_rc; }
    GemmCut cut;
    if (int rc = batched_cut(a, sw, &cut)) return rc;
    return launch_batched_cut(a, cut, sw.legacy);
}

}  // namespace bvc
