// The AMPBlock1 iterations of the generator (models.py:103-121), one fused kernel per iteration: the generic amp_pair_kernel (every channel
// count, with its anti-aliased, symmetric and wide forms), the persistent kernels of the C = 8 and C = 16 stages, and launch_amp_pair,
// which picks among them.  The conv kernel they share their conventions with is in k_vocoder.hip, the device helpers in k_vocoder.h.
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "k_vocoder.h"

namespace bvc {

#ifdef BVC_PHASE_PROBE
__device__ unsigned long long g_phase[16];
#define PHASE(i) do { if (threadIdx.x == 0) { unsigned long long now_ = __builtin_readcyclecounter(); atomicAdd(&g_phase[i], now_ - last_); last_ = now_; } } while (0)
#else
#define PHASE(i)
#endif

// ------------------------------------------------------------------------------------------------
// One AMPBlock1 iteration in one kernel (models.py:106-119):
//     x' = x + conv2( S2( conv1_dil( S1(x) ) ) )            S = SnakeBeta, both convs causal
// Phase 1 parks S1(x) for the output rows plus both halos in LDS; phase 2 runs conv1 on the MFMA for
// TR rows starting (ks-1) rows before the tile, applies bias + S2 and parks the result in a second LDS
// tile (rows before t=0 are zero: the reference pads AFTER the activation); phase 3 runs conv2 on that
// tile and fuses bias, residual, the sum over the three parallel AMP blocks and the final /3.
// The intermediate never touches HBM: 2 tensor passes per iteration instead of 5.
// CS: how many of the four waves lie along the COLUMN tiles (1, 2 or 4); the other 4 / CS lie along the rows.  A wave computes MT row
// tiles x NT / CS column tiles, a workgroup (4 / CS) * MT * 16 rows.  CS = 1 re-reads every weight fragment in all four waves
// (from L2: the weight set of a conv does not fit L1) and feeds MT MFMAs with it; with the waves along the columns a fragment is
// read once per workgroup and feeds CS * MT MFMAs at the same rows per workgroup - the C = 64 stage (180 KB of weights per conv
// at ks = 11) 2.63 -> 2.36 ms per step with CS = 4, MT = 8.  Streaming hops (a hop's one or two new frames are a handful of
// rows: row-split tiles would mostly compute rows nobody reads) use CS = 4 with MT = 2.
// AA: both activations of the pair are anti-aliased (aa_rows).  conv1 then runs on 10 more rows - TT = TR - (ks-1) - 10 - and
// its raw result goes through a second LDS region U behind the first: phase 0 parks the raw x rows [t0-(ks-1)(d+1)-10, t0+TT+10)
// in U, A1 of them becomes the S1 tile, conv1 + bias goes back to U (rows [t0-(ks-1)-5, .. + TR)), A2 of those - clamped to the
// signal's rows 0 and L-1 - becomes the S2 tile of the rows [t0-(ks-1), t0+TT); conv2 and the epilogues are the plain kernel's.
// The S2 tile always re-uses the S1 tile's LDS (ALIAS is ignored).  Offline only: a filtered stage is not causal.
// SYM: both convs pad symmetrically (AMPBlock1(symmetric=True), models.py:35-44,106-119; ks odd): conv1 (ks-1) d / 2 rows on each side,
// conv2 (ks-1) / 2, so out[t] reads x[t - h .. t + h], h = (ks-1)(d+1)/2.  The same tile with its windows shifted: the S1 span starts
// (ks-1) d / 2 rows before conv1's first row instead of (ks-1) d, conv1's rows start (ks-1) / 2 before the tile instead of ks - 1, and the
// S2 rows behind the signal's end are zeros like the ones before its start (the reference pads AFTER the activation on both sides; the
// S1 rows there read as zeros through the descriptor, whatever lies behind the signal in memory).  LDS, TR, TT, the MFMA loops, the
// order of summation and the epilogues are the causal kernel's.  Not with AA.  In a streaming window (row_begin, t_origin as in the
// causal form) the pair looks ahead, so the rows it writes end before the rows it may read: a.L ends the readable input - rows from
// there on read as zeros and the S2 tile is zero behind it - and a.row_end <= a.L bounds the stores and the tile count.  Mid-stream
// row_end = L - h, so no stored row consumes those zeros; at the end of the signal row_end = L, the offline meaning of a.L.
template <int C, int MT, int OCC, bool ALIAS, int CS = 1, bool AA = false, bool SYM = false>
__global__ __launch_bounds__(256, OCC) void amp_pair_kernel(AmpArgs a) {
    static_assert(!(SYM && AA), "a filtered stage is a causal stage");
#ifdef BVC_PHASE_PROBE
    unsigned long long last_ = __builtin_readcyclecounter();
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int S = C + 2;
    constexpr int NT = (C + 15) / 16;
    constexpr int C4 = C / 4;
    constexpr int TR = (4 / CS) * MT * 16;                // rows computed by each conv phase
    constexpr int NTL = NT / CS;                          // column tiles of one wave
    static_assert((CS == 1 || CS == 2 || CS == 4) && NT % CS == 0, "the waves along the columns must divide the column tiles");
    constexpr int CGU = C4 < 16 / NTL ? C4 : 16 / NTL;    // k-steps per weight chunk: 16 fragments per lane and register set (offline C = 64,
                                                          // CS = 1: 4 / 8 / 16 k-steps measured, 2.63 / 2.60 / 2.65 ms for the stage)
    constexpr bool W4 = C >= 32 && CGU % 4 == 0;          // streamed weights in 16-byte granules (a.w1 / a.w2 = ConvLayer::wp4)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int ks = a.ks, dil = a.dil;
    constexpr int AAH = AA ? 5 : 0;                        // rows an anti-aliased activation reads beyond its own, each side
    const int TT = TR - (ks - 1) - 2 * AAH;                // valid output rows of this workgroup
    // Workgroups are dealt round-robin to the 8 XCDs; neighbouring tiles share their halo rows, so each
    // XCD takes a contiguous run of tiles (the halo then hits in that XCD's L2).
    const unsigned nwg = gridDim.x, per = (nwg + 7u) >> 3;
    unsigned bid = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (bid >= a.ntile) return;                           // grid is padded to a multiple of 8
    int b; long long t0;
    tile_origin(a, bid, TT, b, t0);
    const int halo1 = (ks - 1) * dil;
    const int rows1 = TR + halo1;                          // S1(x) rows [t0-(ks-1)-halo1, t0-(ks-1)+TR)
    float *t1 = lds;
    float *t2 = (ALIAS || AA) ? lds : lds + rows1 * S;     // S2(u) rows [t0-(ks-1), t0-(ks-1)+TR) (+ ks-1 spare): takes over
                                                           // the S1(x) tile once conv1 has consumed it (halves the LDS)
    const float *xb = a.x + (long long)b * a.bs;
    const long long tbase = t0 - (SYM ? (ks - 1) / 2 : ks - 1) - AAH;      // global row of local row 0 of phase 2 (conv1's output rows)
    const int rowsA = rows1 > TR + ks - 1 ? rows1 : TR + ks - 1;
    float *traw = lds + rowsA * S;                         // AA: region U, rows1 + 10 rows (raw x, then conv1's raw result)
    (void)traw;

    // ---- phase 1: activated input span.  All global loads of the span are issued before the first
    // SnakeBeta is evaluated (one exposed memory round trip per workgroup instead of one per row group).
    if constexpr (AA) {
        constexpr int NLD = ((TR + 10 * 5 + 2 * AAH) * C4 + 255) / 256;
        f32x4 v[NLD];
        const int total = (rows1 + 2 * AAH) * C4;
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(xb, a.L, C);       // rows outside the signal read as zeros; aa_rows never reads them
        const int xfirst = (int)(tbase - halo1) - AAH;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            const int row = idx / C4, c4 = idx - row * C4;
            v[i] = rows_load4(rs, xfirst + row, C, c4 * 4);
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            if (idx < total) {
                const int row = idx / C4, c4 = idx - row * C4;
                park16<S>(traw, row, c4 * 4, v[i]);
            }
        }
        __syncthreads();
        aa_rows<C>(traw, xfirst, rows1 + 2 * AAH, a.L, t1, xfirst + AAH, rows1, S, a.a1, a.ib1, a.fu1, a.fd1);
    } else {
        constexpr int NLD = ((TR + 10 * 5) * C4 + 255) / 256;       // ks <= 11, dil <= 5
        // The loads are UNCONDITIONAL (rows outside the signal read a clamped row and are zeroed afterwards): a load under a branch
        // made hipcc wait `vmcnt(0)` behind every other one - five exposed round trips per tile at C = 32 instead of one.
        f32x4 v[NLD];
        const int total = rows1 * C4;
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(xb, a.L, C);       // rows outside the signal read as zeros (rows_load4)
        const int tfirst = (int)(tbase - (SYM ? halo1 / 2 : halo1));
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            const int row = idx / C4, c4 = idx - row * C4;
            v[i] = rows_load4(rs, tfirst + row, C, c4 * 4);
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            if (idx < total) {
                const int row = idx / C4, c4 = idx - row * C4;
                const f32x4 aa = *reinterpret_cast<const f32x4 *>(a.a1 + c4 * 4);
                const f32x4 bb = *reinterpret_cast<const f32x4 *>(a.ib1 + c4 * 4);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; e += 2) {                                        // S(0) = 0 keeps the zero padding
                    const f32x2 o2 = snakebeta2((f32x2){v[i][e], v[i][e + 1]}, (f32x2){aa[e], aa[e + 1]}, (f32x2){bb[e], bb[e + 1]});
                    o[e] = o2[0]; o[e + 1] = o2[1];
                }
                park16<S>(t1, row, c4 * 4, o);
            }
        }
    }
    __syncthreads();
    PHASE(0);

    const int mbase = (wave / CS) * MT * 16;
    const int nt0 = (wave % CS) * NTL;                    // first column tile of this wave
    f32x4 acc[MT][NTL];
    auto mma = [&](const float *tile, int d, const float *wp) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int n = 0; n < NTL; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // weight fragments of chunk q+1 are fetched while chunk q feeds the MFMAs
        const float *wl = wp + lane;
        constexpr int CPT = C4 / CGU;                       // chunks per tap
        const int nch = ks * CPT;
        // W4 (C >= 32): the weights come packed [tap][cin/16][ntile][64][4] (ConvLayer::wp4): four k-steps' fragments per 16-byte load
        constexpr int G4 = W4 ? CGU / 4 : CGU;                 // load granules per column tile and chunk
        typedef typename std::conditional<W4, f32x4, float>::type BW;
        BW bcur[G4][NTL], bnxt[G4][NTL];
        auto loadb = [&](BW (&dstb)[G4][NTL], int q) {
            if constexpr (W4) {
                const f32x4 *wq = reinterpret_cast<const f32x4 *>(wp) + (long long)q * G4 * NT * 64 + lane;
#pragma unroll
                for (int u = 0; u < G4; ++u)
#pragma unroll
                    for (int n = 0; n < NTL; ++n) dstb[u][n] = wq[(u * NT + nt0 + n) * 64];
            } else {
                const float *wq = wl + (long long)q * CGU * NT * 64;      // packed [tap][cin/4][ntile][64] is chunk-linear
#pragma unroll
                for (int u = 0; u < CGU; ++u)
#pragma unroll
                    for (int n = 0; n < NTL; ++n) dstb[u][n] = wq[(u * NT + nt0 + n) * 64];
            }
        };
        auto bfrag = [&](const BW (&bw)[G4][NTL], int u, int n) -> float {
            if constexpr (W4) return bw[u >> 2][n][u & 3];
            else return bw[u][n];
        };
        // two register sets take turns (no copies): chunk q+1 is in flight while chunk q feeds the MFMAs
        auto compute = [&](const BW (&bw)[G4][NTL], int q) {
            const int j = q / CPT, cg0 = (q - j * CPT) * CGU;
            const float *arow = tile + (mbase + r + j * d) * S + g;
#pragma unroll
            for (int u = 0; u < CGU; ++u) {
                float av[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) av[i] = arow[i * 16 * S + (cg0 + u) * 4];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int n = 0; n < NTL; ++n)
                        acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bfrag(bw, u, n), acc[i][n], 0, 0, 0);
            }
        };
        // The prefetch is UNCONDITIONAL (past the end it re-reads the last chunk): a load under a branch makes
        // the compiler wait with vmcnt(0) before the next MFMA, i.e. for the prefetch it has just issued, or
        // sink the load next to its use.  The register copy at the end of a chunk is where the wait belongs.
        loadb(bcur, 0);
        if constexpr (C == 32) {
            // the two register sets take turns (no copies: 16 v_mov per tap otherwise); an odd last chunk is multiplied behind the loop.
            // (C = 64 with the waves along the columns spills in this form: every other channel count copies, below.)
            int q = 0;
#pragma unroll 1
            for (; q + 1 < nch; q += 2) {
                loadb(bnxt, q + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(bcur, q);
                __builtin_amdgcn_sched_barrier(0);
                loadb(bcur, q + 2 < nch ? q + 2 : nch - 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(bnxt, q + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (q < nch) compute(bcur, q);
        } else {
#pragma unroll 1
            for (int q = 0; q < nch; ++q) {
                loadb(bnxt, q + 1 < nch ? q + 1 : nch - 1);
                __builtin_amdgcn_sched_barrier(0);             // keep the prefetch ahead of this chunk's MFMAs
                compute(bcur, q);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < G4; ++u)
#pragma unroll
                    for (int n = 0; n < NTL; ++n) bcur[u][n] = bnxt[u][n];
            }
        }
    };

    // Narrow stages (C <= 16): a conv's whole weight set is <= 44 fragments per lane, so it is fetched once
    // into registers and the tap loop is fully unrolled (no per-chunk wait on a weight load; the LDS reads
    // of later taps are scheduled under the MFMAs of earlier ones).  Same accumulation order as mma().
    auto mma_small = [&](const float *tile, int d, const float *wp, auto ks_c) {
        constexpr int KS = decltype(ks_c)::value;
        static_assert(NT == 1 || KS == 0, "mma_small is for one 16-column tile");
        float wreg[KS][C4];
        const float *wl = wp + lane;
#pragma unroll
        for (int j = 0; j < KS; ++j)
#pragma unroll
            for (int c = 0; c < C4; ++c) wreg[j][c] = wl[(j * C4 + c) * NT * 64];
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const float *arow = tile + (mbase + r + j * d) * S + g;
#pragma unroll
            for (int c = 0; c < C4; ++c) {
                float av[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) av[i] = arow[i * 16 * S + c * 4];
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], wreg[j][c], acc[i][0], 0, 0, 0);
            }
        }
    };
    auto conv = [&](const float *tile, int d, const float *wp) {
        if constexpr (C <= 16) {
            if (ks == 11) { mma_small(tile, d, wp, std::integral_constant<int, 11>()); return; }
            if (ks == 7) { mma_small(tile, d, wp, std::integral_constant<int, 7>()); return; }
            if (ks == 3) { mma_small(tile, d, wp, std::integral_constant<int, 3>()); return; }
        }
        mma(tile, d, wp);
    };

    // ---- phase 2: u = conv1(S1(x)) ; t2 = S2(u + b1), zero before the start of the signal
    conv(t1, dil, a.w1);
    PHASE(1);
    if (ALIAS || AA) __syncthreads();                      // every wave is done with S1(x): its LDS becomes t2
    // local rows before `zrow` lie before the start of the signal: zero there (the reference pads AFTER the activation)
    const long long zr64 = -(tbase + amp_t_origin(a, b));
    const int zrow = zr64 <= 0 ? 0 : (zr64 > TR ? TR : (int)zr64);
    // SYM: local rows from `zend` on lie behind the end of the signal: zero there too
    const long long ze64 = a.L - tbase;
    const int zend = !SYM ? TR : (ze64 <= 0 ? 0 : (ze64 > TR ? TR : (int)ze64));
    if constexpr (AA) {
        // conv1 + bias, raw, to U (the raw x rows there were consumed before conv1 began); then A2 of U's rows, clamped to the
        // signal, is the S2 tile of the TR - 10 rows from t0 - (ks-1) on; behind them zeros up to row TR + ks - 1 (read by discarded outputs)
#pragma unroll
        for (int n = 0; n < NTL; ++n) {
            const int col = (nt0 + n) * 16 + r;
            if (col < C) {
                const float bias = a.b1[col];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) traw[(mbase + i * 16 + g * 4 + e) * S + col] = acc[i][n][e] + bias;
            }
        }
        for (int idx = tid; idx < (ks - 1 + 2 * AAH) * S; idx += 256) t2[(TR - 2 * AAH) * S + idx] = 0.0f;
        __syncthreads();
        aa_rows<C>(traw, (int)tbase, TR, a.L, t2, (int)tbase + AAH, TR - 2 * AAH, S, a.a2, a.ib2, a.fu2, a.fd2);
    } else {
    for (int idx = tid; idx < (ks - 1) * S; idx += 256) t2[TR * S + idx] = 0.0f;    // spare rows read by discarded outputs
    if constexpr (C == 8) {
        // Only 8 of the tile's 16 columns exist: lanes r >= 8 hold padding.  They take over rows g*4+2, g*4+3 of
        // column r-8 from their neighbour 8 lanes down (DPP row_shr:8), so that every lane evaluates ONE SnakeBeta
        // pair per row tile instead of half the lanes evaluating two.
        const int col = r & 7, e0 = (r >> 3) * 2;
        const float bias = a.b1[col], aa = a.a2[col], bb = a.ib2[col];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const float a0 = acc[i][0][0], a1 = acc[i][0][1], a2 = acc[i][0][2], a3 = acc[i][0][3];
            const float hi0 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a2), 0x118, 0xf, 0xf, false));   // row_shr:8
            const float hi1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a3), 0x118, 0xf, 0xf, false));
            const float v0 = r < 8 ? a0 : hi0, v1 = r < 8 ? a1 : hi1;
            const int row = mbase + i * 16 + g * 4 + e0;
            const f32x2 s2 = snakebeta2((f32x2){v0 + bias, v1 + bias}, splat2(aa), splat2(bb));
            t2[row * S + col] = (row >= zrow && (!SYM || row < zend)) ? s2[0] : 0.0f;
            t2[(row + 1) * S + col] = (row + 1 >= zrow && (!SYM || row + 1 < zend)) ? s2[1] : 0.0f;
        }
    } else {
        // (all tiles but the first of a signal lie wholly inside it: no row to zero - two selects per pair less; the test is uniform)
        auto s2_tile = [&](auto edge_c) {
            constexpr bool EDGE = decltype(edge_c)::value;
#pragma unroll
            for (int n = 0; n < NTL; ++n) {
                const int col = (nt0 + n) * 16 + r;
                if (col < C) {
                    const float bias = a.b1[col], aa = a.a2[col], bb = a.ib2[col];
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int e = 0; e < 4; e += 2) {
                            const int row = mbase + i * 16 + g * 4 + e;
                            const f32x2 u2 = (f32x2){acc[i][n][e] + bias, acc[i][n][e + 1] + bias};
                            const f32x2 s2 = snakebeta2(u2, splat2(aa), splat2(bb));
                            t2[row * S + col] = (!EDGE || (row >= zrow && (!SYM || row < zend))) ? s2[0] : 0.0f;
                            t2[(row + 1) * S + col] = (!EDGE || (row + 1 >= zrow && (!SYM || row + 1 < zend))) ? s2[1] : 0.0f;
                        }
                }
            }
        };
        if (zrow > 0 || (SYM && zend < TR)) s2_tile(std::true_type());
        else                                s2_tile(std::false_type());
    }
    }
    (void)zrow; (void)zend;
    __syncthreads();
    PHASE(2);

    // ---- phase 3: x' = conv2(t2) + b2 + x   (+ running sum over the AMP blocks, / num_kernels)
    // The residual (and running-sum) operands are fetched BEFORE the MFMA loop so that their latency is
    // covered by it instead of being exposed in the epilogue.
    // The rows of a workgroup are consecutive and C is the whole row, so its output (and the residual /
    // running-sum operands) is ONE contiguous span of global memory: it is moved as float4 per lane, with
    // the conv2 result transposed from the MFMA layout through LDS (the S1(x) tile is dead by now).
    const long long ob = (long long)b * a.bs + t0 * C;
    constexpr int NLD3 = (TR * C4 + 255) / 256;
    long long rows_left = a.L - t0;
    if constexpr (SYM) rows_left = a.row_end - t0;
    const int nvalid4 = (int)(rows_left < TT ? rows_left : TT) * C4;
    f32x4 resq[NLD3], accq[NLD3];
    const bool with_acc = a.epi >= CE_RES_ACC;             // (uniform)
#pragma unroll
    for (int i = 0; i < NLD3; ++i) {                       // unconditional, clamped: items past the tile's valid rows are never stored
        const int idx = tid + i * 256;
        const int idc = idx < nvalid4 ? idx : 0;
        resq[i] = reinterpret_cast<const f32x4 *>(a.x + ob)[idc];
        accq[i] = with_acc ? reinterpret_cast<const f32x4 *>(a.acc + ob)[idc] : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    PHASE(3);
    conv(t2, 1, a.w2);
    PHASE(4);
    if (ALIAS || AA) __syncthreads();                      // t2 is dead: the same LDS now stages the output tile
#pragma unroll
    for (int n = 0; n < NTL; ++n) {
        const int col = (nt0 + n) * 16 + r;
        if (col >= C) continue;
        const float bias = a.b2[col];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) t1[(mbase + i * 16 + g * 4 + e) * S + col] = acc[i][n][e] + bias;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NLD3; ++i) {
        const int idx = tid + i * 256;
        if (idx >= nvalid4) continue;
        const int row = idx / C4, c4 = idx - row * C4;
        f32x4 v = parked16<S>(t1, row, c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float o = v[e] + resq[i][e];                             // x = xt + x      (models.py:119)
            if (a.epi >= CE_RES_ACC) o = accq[i][e] + o;             // xs += resblock  (models.py:224)
            v[e] = o;
        }
        divide_if(a.epi == CE_RES_ACC_DIV, v, a.divisor);            // xs / num_kernels (models.py:225)
        reinterpret_cast<f32x4 *>(a.out + ob)[idx] = v;
    }
    PHASE(5);
}

// ------------------------------------------------------------------------------------------------
// The C = 8 stage (the last and longest signal: 256 rows per frame) on FULL MFMA tiles.  With eight channels a 16-column
// tile of the kernel above is half padding.  Here the 16 columns are (p, co): output rows t and t + d (d = the conv's
// dilation) side by side, p = 0 / 1.  Row t + p*d reads x[t + p*d - m*d] = x[t - (m - p)*d], so both rows read the same
// ks + 1 input rows t - l*d, l = -1 .. ks-1, and the B matrix holds W_j in the p = 0 columns and W_(j-1) in the p = 1
// columns of k-step j (zero where that runs off the kernel): (ks + 1) / (2 ks) of the MFMAs of the padded form, and every
// lane of the SnakeBeta epilogue has work.  A column still accumulates its taps in the order j = 0 .. ks-1, input
// channels ascending (the added zero products come first or last), so results equal the generic kernel's bit for bit.
// Rows are paired inside blocks of 2d rows: pair m <-> rows R(m) + p*d, R(m) = (m / d) * 2d + m % d.  The LDS tiles are
// stored de-interleaved to match: row rho = 2d*blk + half*d + i sits at position half * H + blk*d + i, which puts the A
// operand of pair m, k-step k' = 2a + b at position m + a*d + b*H: lane stride = one row (S = 10 floats: conflict-free
// ds_read_b32), one compile-time offset per k-step.
// which of the stage-specific kernels a model starts with (bvc_model_set_option "vocoder_full_tiles" / "vocoder_c16_kernel": validation switches)
unsigned amp_kernels_default() {
    return (getenv("BVC_NO_AMP8") == nullptr ? AMPK_C8 : 0u) | (getenv("BVC_NO_AMP16") == nullptr ? AMPK_C16 : 0u);
}

template <int D>
__device__ __forceinline__ int pair_row(int m) { return (m / D) * (2 * D) + m % D; }
template <int D>
__device__ __forceinline__ int row_pos(int rho, int H) {
    const int blk = rho / (2 * D), w = rho - blk * (2 * D);
    return w >= D ? H + blk * D + (w - D) : blk * D + w;
}
template <int KS, int D, int MT2>
struct Amp8Geom {
    static constexpr int NP = 4 * MT2 * 16;                     // row pairs per conv phase and workgroup
    static constexpr int NPE = (NP / D) * D;                    // pairs in whole blocks (conv1)
    static constexpr int TR1 = 2 * NPE;                         // rows conv1 produces: [tbase, tbase + TR1)
    static constexpr int TR = 2 * NP;                           // rows conv2 sweeps
    static constexpr int TT = TR1 - (KS - 1);                   // valid output rows per workgroup
    static constexpr int HALO1 = (KS - 1) * D;
    static constexpr int ROWS1 = TR1 + HALO1;                   // S1(x) rows [tbase - HALO1, tbase + TR1)
    static constexpr int H1 = NP + ((KS + 1) / 2) * D;          // half size of the S1(x) tile (positions)
    static constexpr int H2 = NP + (KS + 1) / 2;                // half size of the S2(u) tile
    static constexpr int S = 10;
    static constexpr int LDS_ROWS = 2 * H1 > TR ? 2 * H1 : TR;  // (2 * H2 <= 2 * H1)
    static constexpr size_t LDS_BYTES = (size_t)LDS_ROWS * S * sizeof(float);
};

// The kernel is persistent: a workgroup keeps both convs' weights, biases and SnakeBeta parameters in registers and walks
// over tiles; the input rows of its NEXT tile are requested as soon as the registers that held the current ones are free
// (after S1), so that their latency lies under the current tile's two convs instead of in front of every tile.
template <int KS, int D, int MT2, int OCC>
__global__ __launch_bounds__(256, OCC) void amp_pair8_kernel(AmpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = Amp8Geom<KS, D, MT2>;
    constexpr int C = 8, S = G::S, NP = G::NP, NPE = G::NPE, TR = G::TR, TT = G::TT, H1 = G::H1, H2 = G::H2;
    constexpr int NLD = (G::ROWS1 * 2 + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    TileWalk walk(a.ntile);
    if (!walk.has_tile()) return;

    float w1reg[KS + 1][2], w2reg[KS + 1][2];
#pragma unroll
    for (int k = 0; k <= KS; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            w1reg[k][q] = a.w1[(k * 2 + q) * 64 + lane];
            w2reg[k][q] = a.w2[(k * 2 + q) * 64 + lane];
        }
    const f32x4 aa1 = *reinterpret_cast<const f32x4 *>(a.a1 + (tid & 1) * 4);      // phase 1: item idx has channels (idx & 1) * 4 ..; idx & 1 == tid & 1
    const f32x4 bb1 = *reinterpret_cast<const f32x4 *>(a.ib1 + (tid & 1) * 4);
    // The MFMA operands are swapped (weights as A, activations as B): acc[i][e] = out[pair mbase + 16 i + r][column 4 g + e], column =
    // p * 8 + co - a lane's four results are four consecutive channels of ONE row, so the epilogues work on 16-byte granules
    const int p = g >> 1, co0 = (g & 1) * 4;
    const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(a.b1 + co0), aa2 = *reinterpret_cast<const f32x4 *>(a.a2 + co0);
    const f32x4 bb2 = *reinterpret_cast<const f32x4 *>(a.ib2 + co0), bias2 = *reinterpret_cast<const f32x4 *>(a.b2 + co0);

    auto load_rows = [&](unsigned bid, f32x4 (&v)[NLD]) {       // x rows [t0 - (KS-1) - HALO1, .. + ROWS1) of tile bid
        int b; long long t0;
        tile_origin(a, bid, TT, b, t0);
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(a.x + (long long)b * a.bs, a.L, C);
        const int tfirst = (int)(t0 - (KS - 1) - G::HALO1);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {                        // (items past the tile's rows: loaded like the others, never parked)
            const int idx = tid + i * 256;
            v[i] = rows_load4(rs, tfirst + (idx >> 1), C, (idx & 1) * 4);
        }
    };

    const int mbase = wave * MT2 * 16;
    f32x4 acc[MT2];
    // one conv on row pairs: KS + 1 k-steps of two MFMAs (input channels 0-3, 4-7); all offsets are compile-time
    auto conv = [&](auto dd, int H, const float (&wreg)[KS + 1][2]) {
        constexpr int DD = decltype(dd)::value;
        const float *arow = lds + (mbase + r) * S + g;
#pragma unroll
        for (int i = 0; i < MT2; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k <= KS; ++k) {
            const int pos = (k >> 1) * DD + (k & 1) * H;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float av[MT2];
#pragma unroll
                for (int i = 0; i < MT2; ++i) av[i] = arow[(pos + i * 16) * S + q * 4];
#pragma unroll
                for (int i = 0; i < MT2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[k][q], av[i], acc[i], 0, 0, 0);      // tile of out^T: see the epilogues
            }
        }
    };

    f32x4 v[NLD];
    load_rows(walk.tile(), v);
    for (;;) {
        const unsigned bid = walk.tile();
        int b; long long t0;
        tile_origin(a, bid, TT, b, t0);
        const long long tbase = t0 - (KS - 1);             // global row of conv1's local output row 0

        // ---- phase 1: S1(x) rows [tbase - HALO1, tbase + TR1) into LDS, de-interleaved by D
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            if (idx < G::ROWS1 * 2) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; e += 2) {                                        // S(0) = 0 keeps the zero padding
                    const f32x2 o2 = snakebeta2((f32x2){v[i][e], v[i][e + 1]}, (f32x2){aa1[e], aa1[e + 1]}, (f32x2){bb1[e], bb1[e + 1]});
                    o[e] = o2[0]; o[e + 1] = o2[1];
                }
                park16<S>(lds, row_pos<D>(idx >> 1, H1), (idx & 1) * 4, o);
            }
        }
        const bool more = walk.next();                     // (uniform)
        if (more) load_rows(walk.tile(), v);             // the next tile's rows travel under this tile's convs
        __syncthreads();

        // ---- phase 2: u = conv1(S1(x)); the tile of S2(u + b1) (de-interleaved by 1) takes over the LDS
        conv(std::integral_constant<int, D>(), H1, w1reg);
        __syncthreads();                                   // every wave is done with S1(x)
        {
            const long long zr64 = -(tbase + amp_t_origin(a, b));  // local rows before zrow lie before the start of the signal: zero
            const int zrow = zr64 <= 0 ? 0 : (zr64 > TR ? TR : (int)zr64);      // (the reference pads AFTER the activation)
            auto s2_tile = [&](auto edge_c) {                  // (only a signal's first tile has rows to zero: the test is uniform)
                constexpr bool EDGE = decltype(edge_c)::value;
#pragma unroll
                for (int i = 0; i < MT2; ++i) {
                    const int m = mbase + i * 16 + r;      // this lane's pair; its row of column block p
                    const int row = pair_row<D>(m) + p * D;
                    const f32x4 u4 = acc[i] + bias1;
                    const f32x2 s01 = snakebeta2((f32x2){u4[0], u4[1]}, (f32x2){aa2[0], aa2[1]}, (f32x2){bb2[0], bb2[1]});
                    const f32x2 s23 = snakebeta2((f32x2){u4[2], u4[3]}, (f32x2){aa2[2], aa2[3]}, (f32x2){bb2[2], bb2[3]});
                    const bool keep = !EDGE || row >= zrow;
                    if (NPE == NP || m < NPE) {
                        float2 *dst = reinterpret_cast<float2 *>(lds + row_pos<1>(row, H2) * S + co0);
                        dst[0] = keep ? make_float2(s01[0], s01[1]) : make_float2(0.f, 0.f);
                        dst[1] = keep ? make_float2(s23[0], s23[1]) : make_float2(0.f, 0.f);
                    }
                }
            };
            if (zrow > 0) s2_tile(std::true_type());
            else          s2_tile(std::false_type());
            // rows conv1 did not produce ([TR1, TR + KS]): read only by discarded outputs, but keep them defined
            for (int idx = tid; idx < (TR + KS + 1 - G::TR1) * C; idx += 256) {
                const int row = G::TR1 + idx / C;
                if (row_pos<1>(row, H2) < 2 * H2) lds[row_pos<1>(row, H2) * S + (idx % C)] = 0.0f;
            }
        }
        __syncthreads();

        // ---- phase 3: x' = conv2(t2) + b2 + x (+ running sum, / num_kernels); operands requested before the MFMAs
        const long long ob = (long long)b * a.bs + t0 * C;
        constexpr int NLD3 = (TT * 2 + 255) / 256;
        const long long rows_left = a.L - t0;
        const int nvalid4 = (int)(rows_left < TT ? rows_left : TT) * 2;
        f32x4 resq[NLD3], accq[NLD3];
#pragma unroll
        for (int i = 0; i < NLD3; ++i) {
            const int idx = tid + i * 256;
            const bool ok = idx < nvalid4;
            resq[i] = ok ? reinterpret_cast<const f32x4 *>(a.x + ob)[idx] : (f32x4){0.f, 0.f, 0.f, 0.f};
            accq[i] = (ok && a.epi >= CE_RES_ACC) ? reinterpret_cast<const f32x4 *>(a.acc + ob)[idx] : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        conv(std::integral_constant<int, 1>(), H2, w2reg);
        __syncthreads();                                   // t2 is dead: the LDS now stages the output tile, row-major
#pragma unroll
        for (int i = 0; i < MT2; ++i) {
            const f32x4 o4 = acc[i] + bias2;
            park16<S>(lds, 2 * (mbase + i * 16 + r) + p, co0, o4);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NLD3; ++i) {
            const int idx = tid + i * 256;
            if (idx >= nvalid4) continue;
            f32x4 o4 = parked16<S>(lds, idx >> 1, (idx & 1) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float o = o4[e] + resq[i][e];                            // x = xt + x      (models.py:119)
                if (a.epi >= CE_RES_ACC) o = accq[i][e] + o;             // xs += resblock  (models.py:224)
                o4[e] = o;
            }
            divide_if(a.epi == CE_RES_ACC_DIV, o4, a.divisor);           // xs / num_kernels (models.py:225)
            reinterpret_cast<f32x4 *>(a.out + ob)[idx] = o4;
        }
        if (!more) break;
        __syncthreads();                                   // the staging rows are read: the next tile's S1(x) may overwrite them
    }
}

// ------------------------------------------------------------------------------------------------
// The C = 16 stage on a kernel of its own, in the manner of amp_pair8_kernel: persistent (a workgroup keeps both convs' weights,
// the biases and the SnakeBeta parameters in registers and walks over tiles; the input rows of its NEXT tile travel under the
// current tile's convs), taps and dilation at compile time, and the MFMA operands swapped (weights as A, activations as B), so
// that a lane's four results are four consecutive channels of ONE row: the S2 tile is written as one 16-byte LDS store per row
// tile and the output (with its residual / running-sum operands) moves as 16 bytes per lane straight from the accumulators -
// a wave's 16 rows x 64 bytes are one contiguous KiB - with no transposition through LDS.  Row stride 20 floats: the B-operand
// reads of a wave (16 rows x 4 channels) fall into 64 different banks, and rows stay 16-byte aligned.  Two barriers per tile (the
// S1 and S2 tiles do not share LDS).  Same taps, same k order per output as amp_pair_kernel<16, ...>: the same bits
// (tests/test_gpu_parity.py::test_vocoder_c16_kernel_equals_generic).
template <int KS, int D, int MT>
struct Amp16Geom {
    static constexpr int S = 20;
    static constexpr int TR = 4 * MT * 16;                      // rows per conv phase and workgroup
    static constexpr int TT = TR - (KS - 1);                    // valid output rows
    static constexpr int HALO1 = (KS - 1) * D;
    static constexpr int ROWS1 = TR + HALO1;                    // S1(x) rows [tbase - HALO1, tbase + TR)
    static constexpr int ROWS2 = TR + KS - 1;                   // S2(u) rows [tbase, tbase + TR) + spare rows read by discarded outputs
    static constexpr size_t LDS_BYTES = (size_t)(ROWS1 + ROWS2) * S * sizeof(float);
};

template <int KS, int D, int MT, int OCC>
__global__ __launch_bounds__(256, OCC) void amp_pair16_kernel(AmpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = Amp16Geom<KS, D, MT>;
    constexpr int C = 16, C4 = 4, S = G::S, TR = G::TR, TT = G::TT;
    constexpr int NLD = (G::ROWS1 * C4 + 255) / 256;
    float *t1 = lds, *t2 = lds + G::ROWS1 * S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    TileWalk walk(a.ntile);
    if (!walk.has_tile()) return;

    float w1reg[KS][C4], w2reg[KS][C4];
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
        for (int c = 0; c < C4; ++c) {
            w1reg[j][c] = a.w1[(j * C4 + c) * 64 + lane];
            w2reg[j][c] = a.w2[(j * C4 + c) * 64 + lane];
        }
    const f32x4 aa1 = *reinterpret_cast<const f32x4 *>(a.a1 + (tid & 3) * 4);       // phase 1: item idx has channels (idx & 3) * 4 ..; idx & 3 == tid & 3
    const f32x4 bb1 = *reinterpret_cast<const f32x4 *>(a.ib1 + (tid & 3) * 4);
    const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(a.b1 + g * 4), aa2 = *reinterpret_cast<const f32x4 *>(a.a2 + g * 4);
    const f32x4 bb2 = *reinterpret_cast<const f32x4 *>(a.ib2 + g * 4), bias2 = *reinterpret_cast<const f32x4 *>(a.b2 + g * 4);
    for (int idx = tid; idx < (KS - 1) * S; idx += 256) t2[TR * S + idx] = 0.0f;     // spare rows: never written again

    auto load_rows = [&](unsigned bid, f32x4 (&v)[NLD]) {       // x rows [t0 - (KS-1) - HALO1, .. + ROWS1) of tile bid
        int b; long long t0;
        tile_origin(a, bid, TT, b, t0);
        const __amdgpu_buffer_rsrc_t rs = rows_rsrc(a.x + (long long)b * a.bs, a.L, C);
        const int tfirst = (int)(t0 - (KS - 1) - G::HALO1);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {                        // (items past the tile's rows: loaded like the others, never parked)
            const int idx = tid + i * 256;
            v[i] = rows_load4(rs, tfirst + (idx >> 2), C, (idx & 3) * 4);
        }
    };

    const int mbase = wave * MT * 16;
    f32x4 acc[MT];
    // acc[i][e] = out[row mbase + 16 i + r][channel 4 g + e]; tap j of output row m reads tile row m + j * DD
    auto conv = [&](auto dd, const float *tile, const float (&wreg)[KS][C4]) {
        constexpr int DD = decltype(dd)::value;
        const float *brow = tile + (mbase + r) * S + g;
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KS; ++j)
#pragma unroll
            for (int c = 0; c < C4; ++c) {
                float bv[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) bv[i] = brow[(j * DD + i * 16) * S + c * 4];
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[j][c], bv[i], acc[i], 0, 0, 0);
            }
    };

    f32x4 v[NLD];
    load_rows(walk.tile(), v);
    for (;;) {
        const unsigned bid = walk.tile();
        int b; long long t0;
        tile_origin(a, bid, TT, b, t0);
        const long long tbase = t0 - (KS - 1);             // global row of conv1's local output row 0

        // ---- phase 1: S1(x) rows [tbase - HALO1, tbase + TR) into LDS
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int idx = tid + i * 256;
            if (idx < G::ROWS1 * C4) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; e += 2) {                                        // S(0) = 0 keeps the zero padding
                    const f32x2 o2 = snakebeta2((f32x2){v[i][e], v[i][e + 1]}, (f32x2){aa1[e], aa1[e + 1]}, (f32x2){bb1[e], bb1[e + 1]});
                    o[e] = o2[0]; o[e + 1] = o2[1];
                }
                *reinterpret_cast<f32x4 *>(t1 + (idx >> 2) * S + (idx & 3) * 4) = o;
            }
        }
        const bool more = walk.next();                     // (uniform)
        if (more) load_rows(walk.tile(), v);             // the next tile's rows travel under this tile's convs
        __syncthreads();

        // ---- phase 2: u = conv1(S1(x)); S2(u + b1) into its own tile, zero before the start of the signal
        conv(std::integral_constant<int, D>(), t1, w1reg);
        {
            const long long zr64 = -(tbase + amp_t_origin(a, b));  // local rows before zrow lie before the start of the signal
            const int zrow = zr64 <= 0 ? 0 : (zr64 > TR ? TR : (int)zr64);      // (the reference pads AFTER the activation)
            auto s2_tile = [&](auto edge_c) {                  // (only a signal's first tile has rows to zero: the test is uniform)
                constexpr bool EDGE = decltype(edge_c)::value;
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const int row = mbase + i * 16 + r;
                    const f32x4 u4 = acc[i] + bias1;
                    const f32x2 s01 = snakebeta2((f32x2){u4[0], u4[1]}, (f32x2){aa2[0], aa2[1]}, (f32x2){bb2[0], bb2[1]});
                    const f32x2 s23 = snakebeta2((f32x2){u4[2], u4[3]}, (f32x2){aa2[2], aa2[3]}, (f32x2){bb2[2], bb2[3]});
                    const bool keep = !EDGE || row >= zrow;
                    *reinterpret_cast<f32x4 *>(t2 + row * S + g * 4) = keep ? (f32x4){s01[0], s01[1], s23[0], s23[1]} : (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            };
            if (zrow > 0) s2_tile(std::true_type());
            else          s2_tile(std::false_type());
        }
        __syncthreads();

        // ---- phase 3: x' = conv2(t2) + b2 + x (+ running sum, / num_kernels): operands requested before the MFMAs, 16 bytes per
        // lane, straight from / to the accumulator layout (output row m of this lane: global row t0 + m)
        const long long ob = (long long)b * a.bs + t0 * C;
        const long long rows_left = a.L - t0;
        const int nvalid = (int)(rows_left < TT ? rows_left : TT);
        f32x4 resq[MT], accq[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = mbase + i * 16 + r;
            const bool ok = row < nvalid;
            resq[i] = ok ? *reinterpret_cast<const f32x4 *>(a.x + ob + row * C + g * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
            accq[i] = (ok && a.epi >= CE_RES_ACC) ? *reinterpret_cast<const f32x4 *>(a.acc + ob + row * C + g * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        conv(std::integral_constant<int, 1>(), t2, w2reg);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = mbase + i * 16 + r;
            if (row >= nvalid) continue;
            f32x4 o4 = acc[i] + bias2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float o = o4[e] + resq[i][e];                            // x = xt + x      (models.py:119)
                if (a.epi >= CE_RES_ACC) o = accq[i][e] + o;             // xs += resblock  (models.py:224)
                o4[e] = o;
            }
            divide_if(a.epi == CE_RES_ACC_DIV, o4, a.divisor);           // xs / num_kernels (models.py:225)
            *reinterpret_cast<f32x4 *>(a.out + ob + row * C + g * 4) = o4;
        }
        if (!more) break;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side: one launch path for the three kernel families.
AmpLaunch g_last_amp_launch = {0, 0, 0};
typedef void (*AmpKernel)(AmpArgs);

// workgroups of one persistent kernel instance the device holds at once (first call: conv_kernels_init, outside any stream capture)
template <AmpKernel KERN, size_t LDS_BYTES>
static int amp_slots(const char *name) {
    static int slots = 0;
    if (!slots) {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(KERN), 256, LDS_BYTES) != hipSuccess) {
            set_error("%s: occupancy query failed", name);
            return -1;
        }
        slots = (per_cu > 0 ? per_cu : 1) * cus;
    }
    return slots;
}

// One launch of `kern` on tiles of TT valid output rows each.  prepare(slots) makes the kernel family's own checks (they come behind the
// common ones when errors are reported): a persistent kernel sets `slots` to the workgroups the device holds - the grid is then at most
// that many, each walking over tiles - and the generic kernel leaves it 0: one workgroup per tile.  Either grid is a multiple of 8, so
// that the XCD-contiguous renumbering covers every tile exactly once.
template <class Prepare>
static int launch_amp_tiles(AmpKernel kern, AmpArgs a, int B, int TT, size_t lds, hipStream_t s, Prepare prepare) {
    a.tiles_per_batch = (int)(((a.row_end ? a.row_end : a.L) - a.row_begin + TT - 1) / TT);
    if (a.tiles_per_batch <= 0) return BVC_OK;
    a.tpb_magic = tpb_magic_of((unsigned)a.tiles_per_batch);
    if ((unsigned long long)a.tiles_per_batch * a.tiles_per_batch * (unsigned long long)B >= 0x100000000ull) { set_error("vocoder: tile count beyond the reciprocal's range"); return BVC_EINVAL; }
    int slots = 0;
    if (const int rc = prepare(slots)) return rc;
    ProbeScope probe(PK_CONV, s);
    const unsigned ntile = (unsigned)(a.tiles_per_batch * (long long)B);
    a.ntile = ntile;
    const unsigned grid = (slots == 0 || ntile < (unsigned)slots) ? ((ntile + 7u) & ~7u) : ((unsigned)slots & ~7u);
    g_last_amp_launch = {(long long)ntile, (long long)grid, TT};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// The run-time (ks, dilation) of a pair as a compile-time pair: f(Int<KS>(), Int<D>()) for the nine shapes of the generator's AMP
// blocks, -1 for any other (the generic kernel takes it).
template <int V> using Int = std::integral_constant<int, V>;
template <class F>
static int amp_shape(int ks, int dil, F &&f) {
    auto with_dil = [&](auto ks_c) -> int {
        switch (dil) {
            case 1:  return f(ks_c, Int<1>());
            case 3:  return f(ks_c, Int<3>());
            case 5:  return f(ks_c, Int<5>());
            default: return -1;
        }
    };
    switch (ks) {
        case 3:  return with_dil(Int<3>());
        case 7:  return with_dil(Int<7>());
        case 11: return with_dil(Int<11>());
        default: return -1;
    }
}
template <class F>
static bool amp_shapes_all(F &&f) {                          // f > 0 for every one of the nine
    for (int ks : {3, 7, 11})
        for (int dil : {1, 3, 5})
            if (amp_shape(ks, dil, f) <= 0) return false;
    return true;
}

template <int KS, int D, int MT2, int OCC>
static int amp8_slots() { return amp_slots<amp_pair8_kernel<KS, D, MT2, OCC>, Amp8Geom<KS, D, MT2>::LDS_BYTES>("amp_pair8"); }
template <int MT2, int OCC>
static bool amp8_slots_all() {
    return amp_shapes_all([](auto ks_c, auto d_c) { return amp8_slots<decltype(ks_c)::value, decltype(d_c)::value, MT2, OCC>(); });
}
template <int MT2, int OCC>
static int launch_amp8(AmpArgs a, int B, hipStream_t s) {
    return amp_shape(a.ks, a.dil, [&](auto ks_c, auto d_c) {
        constexpr int KS = decltype(ks_c)::value, D = decltype(d_c)::value;
        using G = Amp8Geom<KS, D, MT2>;
        return launch_amp_tiles(amp_pair8_kernel<KS, D, MT2, OCC>, a, B, G::TT, G::LDS_BYTES, s, [](int &slots) -> int {
            slots = amp8_slots<KS, D, MT2, OCC>();
            return slots > 0 ? BVC_OK : BVC_EHIP;
        });
    });
}

// The C = 16 kernel's instance for KS taps when MT row tiles per wave are asked for.  OCC: the register budget the taps leave (both convs'
// weights live in registers: 8 KS floats per lane); KS = 11, 88 weight registers: four row tiles at most.
template <int KS, int MT> struct Amp16Occ { static constexpr int V = MT >= 4 ? 2 : (KS == 3 ? 4 : KS == 7 ? 3 : 2); };
template <int KS, int D, int MT>
struct Amp16Inst {
    static constexpr int MTK = KS == 11 ? (MT > 4 ? 4 : MT) : MT;
    using G = Amp16Geom<KS, D, MTK>;
    static constexpr AmpKernel kern = amp_pair16_kernel<KS, D, MTK, Amp16Occ<KS, MT>::V>;
    static int slots() { return amp_slots<kern, G::LDS_BYTES>("amp_pair16"); }
};
template <int MT>
static bool amp16_slots_all() {
    return amp_shapes_all([](auto ks_c, auto d_c) { return Amp16Inst<decltype(ks_c)::value, decltype(d_c)::value, MT>::slots(); });
}
template <int MT>
static int launch_amp16(AmpArgs a, int B, hipStream_t s) {
    return amp_shape(a.ks, a.dil, [&](auto ks_c, auto d_c) {
        using I = Amp16Inst<decltype(ks_c)::value, decltype(d_c)::value, MT>;
        return launch_amp_tiles(I::kern, a, B, I::G::TT, I::G::LDS_BYTES, s, [](int &slots) -> int {
            slots = I::slots();
            return slots > 0 ? BVC_OK : BVC_EHIP;
        });
    });
}

int amp_kernels_init() {
    return amp8_slots_all<1, 4>() && amp8_slots_all<2, 2>() && amp16_slots_all<4>() ? BVC_OK : BVC_EHIP;
}

template <int C, int MT, int OCC, bool ALIAS, int CS = 1, bool AA = false, bool SYM = false>
static int launch_amp_t(AmpArgs a, int B, hipStream_t s) {
    constexpr int TR = (4 / CS) * MT * 16;
    constexpr AmpKernel kern = amp_pair_kernel<C, MT, OCC, ALIAS, CS, AA, SYM>;
    const int TT = TR - (a.ks - 1) - (AA ? 10 : 0);
    const int rows1 = TR + (a.ks - 1) * a.dil;
    const size_t lds = AA ? (size_t)((rows1 > TR + a.ks - 1 ? rows1 : TR + a.ks - 1) + rows1 + 10) * (C + 2) * sizeof(float)
                          : (size_t)(rows1 + (ALIAS ? 0 : TR + (a.ks - 1))) * (C + 2) * sizeof(float);
    return launch_amp_tiles(kern, a, B, TT, lds, s, [&](int &) -> int {
        if (AA && a.L + TR > 0x7FFFFFFFll) { set_error("amp_pair: %lld rows are beyond the anti-aliased kernel's row index", a.L); return BVC_EINVAL; }
        if (lds > 160 * 1024 || TT <= 0) { set_error("amp_pair tile needs %zu B of LDS", lds); return BVC_EINVAL; }
        static bool attr = false;
        if (!attr) { BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
        return BVC_OK;
    });
}

// ---- how the offline AMP pair of the C = 64 stage is cut into tiles (host only; tile_plan in bvc_internal.h).
// A tile of TR rows yields TR - (ks - 1) output rows of one batch item; 512 slots (two workgroups per CU).  fixed: the rows'
// worth of time a tile costs whatever its height, fitted from two measured heights on nearly whole rounds (ks = 7: 96 rows, 5 rounds,
// 224.3 us against 80 rows, 6 rounds, 223.6 us: 1.5 rows; profiles/tile_rounds.md).
TilePlan g_last_amp_cut = {0, 0, 0, 0};
static constexpr int AMP64_FIXED_ROWS = 1;
TilePlan amp_pair_cut(long long L, int B, int ks, int force_height, bool legacy) {
    static const int heights[4] = {128, 112, 96, 80}, slots[4] = {512, 512, 512, 512};
    if (!force_height && !legacy) return tile_plan(L, B, heights, slots, 4, AMP64_FIXED_ROWS, ks - 1);
    int one = force_height ? 0 : heights[0];               // the shape of before the plan: the tallest
    for (int h : heights) if (h == force_height) one = h;
    if (!one) return {0, 0, 0, 0};
    return tile_plan(L, B, &one, slots, 1, AMP64_FIXED_ROWS, ks - 1);
}

// ---- which launch a pair takes.  Tile shapes are from measured sweeps (tools/voc_stage_times.py): MT = 16-row tiles per wave, OCC =
// workgroups per CU the register budget is set for, ALIAS = the S2 tile re-uses the LDS of the S1 tile (one more barrier, half the
// LDS), CS = waves along the columns.
typedef int (*AmpLauncher)(AmpArgs, int, hipStream_t);
static int launch_by(AmpLauncher launch, const AmpArgs &a, int C, int B, hipStream_t s) {
    if (!launch) { set_error("amp_pair: unsupported channel count %d", C); return BVC_EINVAL; }
    return launch(a, B, s);
}

// anti-aliased pair: the generic kernel with the filters around both activations, one tile shape per stage - the tallest whose
// two LDS regions leave the stage's workgroups per CU (C = 64: 96 rows, 78 KiB at ks = 11; C = 32 / 16: 128 rows; C = 8: 256)
static AmpLauncher amp_antialiased(int C) {
    switch (C) {
        case 64: return launch_amp_t<64, 6, 2, true, 4, true>;
        case 32: return launch_amp_t<32, 2, 3, true, 1, true>;
        case 16: return launch_amp_t<16, 2, 4, true, 1, true>;
        case 8:  return launch_amp_t<8, 4, 4, true, 1, true>;
        default: return nullptr;
    }
}

// symmetric pair: the generic kernel's SYM form at every channel count, with the tile shape the causal generic kernel has there
// (C = 64: the tallest, 128 rows)
static AmpLauncher amp_symmetric(int C) {
    switch (C) {
        case 64: return launch_amp_t<64, 8, 2, true, 4, false, true>;
        case 32: return launch_amp_t<32, 4, 3, true, 1, false, true>;
        case 16: return launch_amp_t<16, 2, 4, false, 1, false, true>;
        case 8:  return launch_amp_t<8, 4, 4, true, 1, false, true>;
        default: return nullptr;
    }
}

// symmetric pair in a look-ahead window (the incremental generator, generator.hip): a hop brings 8 - 512 new rows per stage, of which the
// offline shapes above (128 - 256 rows per workgroup) would mostly compute rows nobody reads - the causal short windows' situation
// (amp_short_window below), and the same cuts: C = 64 one 32-row tile with the waves along the columns for the one or two frames of
// stage 0, else 64-row tiles; C = 32 and 16 up to three 64-row tiles; C = 8 up to three 128-row tiles.  BVC_SYM_WINDOW_TILES=offline
// (read per call: tools/lookahead_stream_cost.py runs both in one process) keeps the offline shapes; profiles/lookahead_stream_cost.md
static AmpLauncher amp_symmetric_window(int C, int ks, long long new_rows) {
    const char *force = getenv("BVC_SYM_WINDOW_TILES");
    if (force && !strcmp(force, "offline")) return nullptr;
    if (C == 64 && new_rows <= 32 - (ks - 1)) return launch_amp_t<64, 2, 2, true, 4, false, true>;
    if (C == 64 && new_rows <= 2 * (64 - (ks - 1))) return launch_amp_t<64, 1, 2, true, 1, false, true>;
    if (C == 32 && new_rows <= 3 * (64 - (ks - 1))) return launch_amp_t<32, 1, 3, true, 1, false, true>;
    if (C == 16 && new_rows <= 3 * (64 - (ks - 1))) return launch_amp_t<16, 1, 4, false, 1, false, true>;
    if (C == 8 && new_rows <= 3 * (128 - (ks - 1))) return launch_amp_t<8, 2, 4, true, 1, false, true>;
    return nullptr;
}

// wide stages (generators of 256 / 512 initial channels): the generic pair with the waves along the columns (a conv's weights
// are 0.7 - 2.9 MB: a fragment is read once per workgroup) and the S2 tile in the S1 tile's LDS.  C = 256: 64 rows, 114 x 258
// floats = 117.6 KB at ks = 11, d = 5, one workgroup per CU: 32.9 ms for the stage at 64 x 430 frames; 96 rows (150.7 KB), the
// other compiled height, 39.0.  C = 128: 64 rows, 114 x 130 floats = 59 KB, two per CU: 7.69 ms as stage 0 of a 256-wide
// generator, 60.70 as stage 1 of a 512-wide one; 128 rows (92.6 KB, one per CU) 8.35 / 60.73.  BVC_AMP256_TR / BVC_AMP128_TR
// pick the other height (read per call: tests and tools/wide_generator_cost.py run both in one process;
// profiles/wide_generator_cost.md).  A streaming window of at most one 32-row tile takes that tile, like C = 64.
static int launch_amp_wide(const AmpArgs &a, int C, bool win, bool short_win, int B, hipStream_t s) {
    if (short_win) return C == 256 ? launch_amp_t<256, 2, 1, true, 4>(a, B, s) : launch_amp_t<128, 2, 2, true, 4>(a, B, s);
    const char *name = C == 256 ? "BVC_AMP256_TR" : "BVC_AMP128_TR";
    const char *force = win ? nullptr : getenv(name);
    const int tr = force ? atoi(force) : 64;
    if (C == 256) {
        if (tr == 64) return launch_amp_t<256, 4, 1, true, 4>(a, B, s);
        if (tr == 96) return launch_amp_t<256, 6, 1, true, 4>(a, B, s);
    } else {
        if (tr == 64) return launch_amp_t<128, 4, 2, true, 4>(a, B, s);
        if (tr == 128) return launch_amp_t<128, 8, 1, true, 4>(a, B, s);
    }
    set_error("amp_pair: %s=%s is not a compiled tile height", name, force);
    return BVC_EINVAL;
}

// streaming hops compute a few new rows behind a 64-row history: the 128 / 256-row tiles of the offline sweep would spend
// most of their MFMAs on rows nobody reads, so short windows take the smallest tile (4 waves x 16 rows); nullptr: not a short window
static AmpLauncher amp_short_window(int C, int ks, long long new_rows) {
    if (C == 64 && new_rows <= 32 - (ks - 1)) return launch_amp_t<64, 2, 2, true, 4>;      // 32 rows, waves split the columns
    if (C == 64 && new_rows <= 2 * (64 - (ks - 1))) return launch_amp_t<64, 1, 2, true>;
    if (C == 32 && new_rows <= 3 * (64 - (ks - 1))) return launch_amp_t<32, 1, 3, true>;   // (3 tiles of 64 rows against one of 256 for a two-frame hop: 1.53 -> 1.47 ms per tick at 256 streams)
    return nullptr;
}

// C = 64 behind the short windows: the waves along the columns, 2.33 ms per step for the stage with eight row tiles per wave (two column
// groups x two row groups: 2.60; the waves along the rows: 2.63, profiles/r03_vocoder_variants.txt); offline, the plan picks the tile
// height per launch (whole rounds of the 512 slots: amp_pair_cut)
static int launch_amp64(const AmpArgs &a, bool win, long long new_rows, int B, hipStream_t s) {
    int tr = 128;
    if (!win) {
        const char *force = getenv("BVC_AMP64_TR");       // read per call: tests force every compiled height in one process
        const TilePlan cut = amp_pair_cut(new_rows, B, a.ks, force ? atoi(force) : 0, tile_cut_legacy());
        if (cut.height == 0) { set_error("amp_pair: BVC_AMP64_TR=%s is not a compiled tile height", force ? force : ""); return BVC_EINVAL; }
        g_last_amp_cut = cut;
        tile_trace("amp_pair64", new_rows, (long long)B * 100 + a.ks, cut.height, 0, cut.tiles, 512, cut.rounds);
        tr = cut.height;
    }
    switch (tr) {
        case 80:  return launch_amp_t<64, 5, 2, true, 4>(a, B, s);
        case 96:  return launch_amp_t<64, 6, 2, true, 4>(a, B, s);
        case 112: return launch_amp_t<64, 7, 2, true, 4>(a, B, s);
        default:  return launch_amp_t<64, 8, 2, true, 4>(a, B, s);
    }
}

// C = 8: the full-tile form where the layers carry its weight packing and the model allows it.  Tile shapes from a measured sweep (16-pair
// tiles per wave x register budget): <2, 2> 2.07 ms per step for the stage, <2, 4> 2.17 (spills at ks = 11), <4, 4> 2.19, <1, 4> 2.4;
// the generic padded kernel 2.68 (3.14 before its own sweep).  Short streaming windows take the smallest tile (4 waves x 16 pairs = 128 rows).
static int launch_amp_c8(AmpArgs a, const ConvLayer &c1, const ConvLayer &c2, bool win, long long new_rows, unsigned kernels, int B, hipStream_t s) {
    if (c1.wp2 && c2.wp2 && (kernels & AMPK_C8)) {
        AmpArgs a8 = a;
        a8.w1 = c1.wp2; a8.w2 = c2.wp2;
        const int rc8 = (win && new_rows <= 128) ? launch_amp8<1, 4>(a8, B, s) : launch_amp8<2, 2>(a8, B, s);
        if (rc8 != -1) return rc8;
    }
    return launch_amp_t<8, 4, 4, true>(a, B, s);
}

// C = 16: the offline sweep on the persistent kernel, four row tiles per wave (256 rows per workgroup): 2.82 (generic kernel) -> 2.62 ms
// per step for the stage; two tiles 2.82, six (KS <= 7) 2.60.  The generic kernel: MT 4 / ALIAS no gain.
static int launch_amp_c16(const AmpArgs &a, bool win, unsigned kernels, int B, hipStream_t s) {
    if ((kernels & AMPK_C16) && !win) {
        const int rc16 = launch_amp16<4>(a, B, s);
        if (rc16 != -1) return rc16;
    }
    return launch_amp_t<16, 2, 4, false>(a, B, s);
}

int launch_amp_pair(const ConvLayer &c1, const ConvLayer &c2, const float *x, long long L, float *out, int B, int epi,
                    const float *acc, float divisor, hipStream_t s, const ConvWindow *win, unsigned kernels, bool sym, long long bs) {
    if (B <= 0 || L <= 0) return BVC_OK;
    const int C = c1.cin;
    if (c1.cin != c1.cout || c2.cin != c1.cin || c2.ks != c1.ks || c2.dil != 1 || !c1.act_a || !c2.act_a) {
        set_error("amp_pair: unsupported layer pair");
        return BVC_EINVAL;
    }
    AmpArgs a;
    a.x = x; a.out = out; a.acc = acc; a.L = L;
    a.w1 = c1.wp; a.b1 = c1.bias; a.a1 = c1.act_a; a.ib1 = c1.act_ib;
    a.w2 = c2.wp; a.b2 = c2.bias; a.a2 = c2.act_a; a.ib2 = c2.act_ib;
    if (C >= 32) {                                         // amp_pair_kernel<32 / 64, ...> streams its weights in 16-byte granules
        if (!c1.wp4 || !c2.wp4) { set_error("amp_pair: layer pair without the 16-byte weight packing"); return BVC_EINVAL; }
        a.w1 = c1.wp4; a.w2 = c2.wp4;
    }
    a.divisor = divisor; a.epi = epi; a.ks = c1.ks; a.dil = c1.dil; a.tiles_per_batch = 0;
    a.bs = win ? win->in_bs : (bs ? bs : L * C);
    a.row_begin = win ? win->row_begin : 0;
    a.t_origin = win ? win->t_origin : 0;
    a.row_age = win ? win->row_age : nullptr;
    a.age_rate = win ? win->age_rate : 0;
    a.fu1 = c1.aa_up; a.fd1 = c1.aa_down; a.fu2 = c2.aa_up; a.fd2 = c2.aa_down;
    a.row_end = 0;
    // wide stages (C = 128 / 256) exist as causal, unfiltered pairs only; their rows go through 32-bit byte offsets (rows_load4)
    const bool wide = C >= 128;
    if (wide) {
        if (C != 128 && C != 256) { set_error("amp_pair: unsupported channel count %d", C); return BVC_EINVAL; }
        if (c1.aa_up || c2.aa_up || c1.aa_down || c2.aa_down) { set_error("amp_pair: anti-aliased activations are not implemented on a stage of %d channels (64 at most)", C); return BVC_EINVAL; }
        if (sym) { set_error("amp_pair: symmetric layers are not implemented on a stage of %d channels (64 at most)", C); return BVC_EINVAL; }
        if (L + 512 > 0x7FFFFFFFll / C / 4) { set_error("amp_pair: %lld rows of %d channels are beyond the kernel's row index", L, C); return BVC_EINVAL; }
    }
    if (c1.aa_up || c2.aa_up) {
        if (!c1.aa_up || !c1.aa_down || !c2.aa_up || !c2.aa_down) { set_error("amp_pair: a pair is filtered on both activations or on none"); return BVC_EINVAL; }
        if (win) { set_error("amp_pair: an anti-aliased pair looks ahead and has no streaming window"); return BVC_EINVAL; }
        return launch_by(amp_antialiased(C), a, C, B, s);
    }
    if (sym) {
        if (win && !win->lookahead) { set_error("amp_pair: a symmetric pair looks ahead and has no streaming window (but a look-ahead window)"); return BVC_EINVAL; }
        if (c1.ks % 2 == 0) { set_error("amp_pair: a symmetric pair needs an odd kernel size (got %d)", c1.ks); return BVC_EINVAL; }
        if (L + 512 > 0x7FFFFFFFll / C / 4) { set_error("amp_pair: %lld rows are beyond the symmetric kernel's row index", L); return BVC_EINVAL; }
        a.row_end = (int)L;
        if (win) {
            if (win->row_age || a.row_begin < 0 || win->row_end < a.row_begin || win->row_end > L) {
                set_error("amp_pair: look-ahead window rows [%lld, %lld) of %lld readable rows", a.row_begin, win->row_end, L); return BVC_EINVAL;
            }
            if (win->row_end == a.row_begin) return BVC_OK;
            a.row_end = (int)win->row_end;
            if (const AmpLauncher launch = amp_symmetric_window(C, c1.ks, a.row_end - a.row_begin)) return launch(a, B, s);
        }
        return launch_by(amp_symmetric(C), a, C, B, s);
    }
    if (bs) { set_error("amp_pair: a batch stride of its own belongs to a symmetric stage's view"); return BVC_EINVAL; }
    const long long new_rows = L - a.row_begin;
    if (wide) return launch_amp_wide(a, C, win != nullptr, win && new_rows <= 32 - (c1.ks - 1), B, s);
    if (win)
        if (const AmpLauncher launch = amp_short_window(C, c1.ks, new_rows)) return launch(a, B, s);
    switch (C) {
        case 64: return launch_amp64(a, win != nullptr, new_rows, B, s);
        case 32: return launch_amp_t<32, 4, 3, true>(a, B, s);     // (waves along the columns, CS = 2 with 4 or 8 row tiles: 4.64 / 4.41 against 4.48;
                                                                   // three row tiles per wave, 192 rows: slower at every ks, profiles/tile_rounds.md)
        case 16: return launch_amp_c16(a, win != nullptr, kernels, B, s);
        case 8:  return launch_amp_c8(a, c1, c2, win != nullptr, new_rows, kernels, B, s);
        default: set_error("amp_pair: unsupported channel count %d", C); return BVC_EINVAL;
    }
}

#ifdef BVC_PHASE_PROBE
int phase_probe_read(unsigned long long *out, int reset) {
    BVC_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 16));
    if (reset) { unsigned long long z[16] = {0}; BVC_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z))); }
    return BVC_OK;
}
#endif
}  // namespace bvc
