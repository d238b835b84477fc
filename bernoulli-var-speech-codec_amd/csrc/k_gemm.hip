// BVRNN GEMM kernels for gfx950 (fp32-in / fp32-accumulate MFMA, exact fp32 products).
//
//  gemm_skinny_kernel  - one recurrent-step layer: y[M,N] = epi( [x1|x2|x3] @ W^T + b ), M = batch
//                        (<= a few hundred rows).  One workgroup per 16x16 output tile, the K
//                        dimension is split over the 8 waves of the workgroup (each wave streams
//                        its slice of the activation rows and weight rows straight from L2/MALL
//                        into MFMA operand registers - there is no reuse inside a workgroup, so no
//                        LDS staging), partial tiles are summed in fixed order through LDS, and the
//                        layer's epilogue (bias, ELU, sigmoid/round/bit-mask, mel normalisation,
//                        GRU cell) is applied by the first 256 threads.  Workgroups that share
//                        weight rows (the batch tiles of one feature tile) are placed on the same
//                        XCD so each weight row crosses the fabric once per step.
//  step_advance / set_desc - the two one-thread kernels that keep the call descriptor of a replayed step graph.
//  The batched GEMMs over all frames are in k_gemm_batched.hip, the row-wise utilities in k_rows.hip, the device helpers all of
//  them (and k_flow.hip) share in k_gemm.h.
//
// ONE order of summation per output, whichever kernel computes a layer (the persistent recurrence kernel of k_flow.hip, the
// launch-per-layer kernel below, the batched kernels): the K/16 k-blocks of a segment are cut into NCHUNK = 8 chunks - chunk c =
// blocks [nb*c/8, nb*(c+1)/8) -, a chunk is a chain of MFMAs over its blocks in k order starting from zero, the chunks are added
// in ascending order (the first one is copied), then the bias, then an optional pre-computed addend, then the activation.  In the
// recurrent kernels a chunk is a wave's share of the split K; the batched kernels run the chunks one after the other in the same
// accumulators.  A layer over a concatenated input [x1 | x2] cuts EACH segment into its 8 chunks and chains chunk c of x2 behind
// chunk c of x1 in the same accumulator.  So a code bit does not depend on the schedule that computed it.
//
// Reference semantics: nn.Linear / nn.ELU / nn.Sigmoid / torch.round / nn.GRU as used at
// bvrnn.py:44-83,163-229.
#include <atomic>
#include <cstdlib>

#include "k_gemm.h"

namespace bvc {

struct Resolved { float *p; long long ld; bool ok; int packed; };

// Effective address of a DynPtr for frame t.  Packed frame tensors hold one fragment-packed
// [mt16][dim] matrix per frame (mt16 = rows rounded up to 16).
// Scalar loads of call-descriptor fields.  hipcc emits VECTOR loads for these (the descriptor is not
// provably invariant), and then waits vmcnt(0) for them - which also waits for every weight load issued
// just before.  s_load + lgkmcnt keeps the descriptor off the vector-memory counter.  (The scalar cache
// is invalidated by the acquire at every kernel dispatch, like for kernel arguments.)
__device__ __forceinline__ int sload_i32(const void *p) {
    int v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
__device__ __forceinline__ long long sload_i64(const void *p) {
    long long v;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}

// The frame counter is read from the descriptor only by pointers that need it (kind 1/2): layers whose
// operands are all workspace-static never wait for that line.
// MF: the launch covers several frames (grid.y = frame): static pointers advance by their frame stride (other launches never read blockIdx.y)
template <bool MF = false>
__device__ __forceinline__ Resolved resolve(const DynPtr &d, const CallDesc *c, int mt16, int tstep) {
    const int kind = d.meta & 15, packed = (d.meta >> 4) & 1;
    if (kind == 0) return {MF ? d.base + (long long)blockIdx.y * d.poff : d.base, (long long)d.ld, d.base != nullptr, packed};
    const int toff = ((d.meta >> 16) & 255) - 8;
    const int t = sload_i32(&c->t) + tstep;
    if (kind == 2) return {d.base + (((t + toff) & 1) ? d.poff : 0), (long long)d.ld, true, packed};
    const long long T = sload_i64(&c->T);
    float *b = reinterpret_cast<float *>(sload_i64(&c->p[(d.meta >> 8) & 255]));
    const long long tt = (long long)t + toff;
    const bool ok = (b != nullptr) && tt >= 0 && tt < T;
    if (packed) return {ok ? b + tt * (long long)mt16 * d.dim : nullptr, (long long)d.dim, ok, 1};
    return {ok ? b + tt * d.dim : nullptr, T * d.dim, ok, 0};
}

__device__ __forceinline__ void store_out(const Resolved &y, int m, int n, float v) {
    if (y.packed) y.p[packed_off(m, n, y.ld)] = v;
    else y.p[(long long)m * y.ld + n] = v;
}

// Accumulate k-blocks [lo, hi) of one segment into acc[MTW][NG].  wl: this lane's pointer into the packed
// weights of (n-tile, gate 0, k-block 0).  The weight loads of the first chunk are issued BEFORE the
// activation pointer is resolved: weight addresses come from kernel arguments only, while a frame- or
// parity-indexed activation pointer needs the frame counter from the call descriptor (a dependent
// load of a line another kernel has just written), whose latency is thus hidden behind the weights.
// MTW row tiles share every weight fragment in registers (weights cross the L2->CU path once per MTW*16 rows).
template <int NG, int U, int MTW, bool MF = false>
__device__ __forceinline__ void run_segment(const float *wl, long long gate_stride, long long kbs, const DynPtr &xd,
                                            const CallDesc *dsc, int mt16, int tstep, const int (&mtile)[MTW],
                                            const int (&xrow)[MTW], int lane, int g, int lo, int hi,
                                            f32x4 (&acc)[MTW][NG]) {
    const float *xl[MTW];
    int xstep = 0;
    bool have_x = false;
    auto resolve_x = [&]() {
        const Resolved x = resolve<MF>(xd, dsc, mt16, tstep);
#pragma unroll
        for (int j = 0; j < MTW; ++j) {
            if (x.packed) { xl[j] = x.p + (long long)mtile[j] * (x.ld >> 4) * 256 + lane * 4; xstep = 256; }
            else          { xl[j] = x.p + (long long)xrow[j] * x.ld + g * 4;                  xstep = 16; }
        }
        have_x = true;
    };
    int kb = lo;
    for (; kb + U <= hi; kb += U) {
        f32x4 xv[U][MTW];
        f32x4 wv[U][NG];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < NG; ++q)
                wv[u][q] = *reinterpret_cast<const f32x4 *>(wl + (long long)q * gate_stride + (long long)(kb + u) * kbs);
        if (!have_x) resolve_x();
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < MTW; ++j) xv[u][j] = *reinterpret_cast<const f32x4 *>(xl[j] + (long long)(kb + u) * xstep);
        __builtin_amdgcn_sched_barrier(0);      // keep all U blocks' loads in flight ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < MTW; ++j)
#pragma unroll
                    for (int q = 0; q < NG; ++q) acc[j][q] = mfma16(xv[u][j][e], wv[u][q][e], acc[j][q]);
        }
    }
    for (; kb < hi; ++kb) {
        f32x4 wv[NG];
#pragma unroll
        for (int q = 0; q < NG; ++q)
            wv[q] = *reinterpret_cast<const f32x4 *>(wl + (long long)q * gate_stride + (long long)kb * kbs);
        if (!have_x) resolve_x();
#pragma unroll
        for (int j = 0; j < MTW; ++j) {
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(xl[j] + (long long)kb * xstep);
#pragma unroll
            for (int q = 0; q < NG; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][q] = mfma16(xv[e], wv[q][e], acc[j][q]);
        }
    }
}

template <int NG, int NGRP, int NW, int U, int MTW, bool GIL = false, bool MF = false>
__global__ __launch_bounds__(NW * 64) void gemm_skinny_kernel(GemmParams p, int epi) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [NW][NGRP*NG][MTW][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const CallDesc *dsc = p.desc;
    unsigned long long t_start = 0;
    if (p.probe) t_start = wall_clock64();                           // probe builds of the graph only

    const int n_tiles = p.N >> 4;
    const int m_tiles = (p.M + 15) >> 4;
    const int m_groups = (m_tiles + MTW - 1) / MTW;                  // MTW row tiles per workgroup
    const int mt16 = m_tiles << 4;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int ntile = (slot / m_groups) * 8 + xcd;
    const int mgroup = slot % m_groups;
    if (ntile >= n_tiles) return;                                    // uniform per workgroup
    const int n0 = ntile << 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;

    // epilogue constants are fetched up front so their latency overlaps the operand stream
    constexpr int NACC = NG * NGRP;
    float bias[NACC];
    if (tid < 256) {
        const int n = n0 + (tid & 15);
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            bias[q] = p.bias0 ? p.bias0[(long long)q * p.gate_rows + n] : 0.0f;
            if (NGRP > 1) bias[NG + q] = p.bias1[(long long)q * p.gate_rows + n];
        }
    }

    int mtile[MTW], xrow[MTW];
#pragma unroll
    for (int j = 0; j < MTW; ++j) {
        const int mt = mgroup * MTW + j;
        mtile[j] = mt < m_tiles ? mt : m_tiles - 1;                  // a missing tile re-reads the last one; never stored
        const int row = (mtile[j] << 4) + r;
        xrow[j] = row < p.M ? row : p.M - 1;                         // natural layout: clamp (row never stored)
    }

    f32x4 acc0[MTW][NG], acc1[MTW][NG];
#pragma unroll
    for (int j = 0; j < MTW; ++j)
#pragma unroll
        for (int q = 0; q < NG; ++q) { acc0[j][q] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[j][q] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    // every segment is cut over the waves on its own (wave w = chunk w of the summation order, see the head of this file): the
    // accumulator of a wave chains its chunk of the first segment, then its chunk of the second, ...
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s > 0 && s >= p.nseg) break;
        const int sb = p.seg[s].K >> 4;
        const int lo = (int)(((long long)sb * wave) / NW);
        const int hi = (int)(((long long)sb * (wave + 1)) / NW);
        if (lo < hi) {
            // floats between k-blocks / between gates: [n/16][k/16][lane][4] per gate, or gate-interleaved [n/16][k/16][gate][lane][4]
            constexpr long long kbs = GIL ? NG * 256 : 256;
            const long long gate_stride = GIL ? 256 : (long long)(p.gate_rows >> 4) * p.seg[s].wnb * 256;
            const float *wl = p.seg[s].w + (long long)ntile * p.seg[s].wnb * kbs + lane * 4;
            if constexpr (NGRP == 1) {
                run_segment<NG, U, MTW, MF>(wl, gate_stride, kbs, p.seg[s].x, dsc, mt16, p.tstep, mtile, xrow, lane, g, lo, hi, acc0);
            } else {
                if (p.seg[s].grp == 0)
                    run_segment<NG, U, MTW, MF>(wl, gate_stride, kbs, p.seg[s].x, dsc, mt16, p.tstep, mtile, xrow, lane, g, lo, hi, acc0);
                else
                    run_segment<NG, U, MTW, MF>(wl, gate_stride, kbs, p.seg[s].x, dsc, mt16, p.tstep, mtile, xrow, lane, g, lo, hi, acc1);
            }
        }
    }

    // ---- cross-wave reduction through LDS, fixed order (deterministic)
#pragma unroll
    for (int j = 0; j < MTW; ++j)
#pragma unroll
        for (int q = 0; q < NG; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = ((g * 4 + e) << 4) + r;              // D[row=g*4+e][col=r]
                red[((wave * NACC + q) * MTW + j) * 256 + idx] = acc0[j][q][e];
                if (NGRP > 1) red[((wave * NACC + NG + q) * MTW + j) * 256 + idx] = acc1[j][q][e];
            }
    __syncthreads();
    if (tid >= 256) return;
    const int i = tid >> 4, jj = tid & 15;
    const int n = n0 + jj;
#pragma unroll 1
    for (int j = 0; j < MTW; ++j) {
        const int mt = mgroup * MTW + j;
        const int m = (mt << 4) + i;
        if (mt >= m_tiles || m >= p.M) continue;
        float v[NACC];
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            float sum = red[(a * MTW + j) * 256 + tid];
#pragma unroll
            for (int w = 1; w < NW; ++w) sum += red[((w * NACC + a) * MTW + j) * 256 + tid];
            v[a] = sum + bias[a];
        }
        const Resolved y = resolve<MF>(p.y, dsc, mt16, p.tstep);
        if (epi == EPI_LINEAR || epi == EPI_ELU) {
            float o = v[0];
            if (p.aux.base || (p.aux.meta & 15)) {                            // pre-computed half of a split dot product
                const Resolved ad = resolve<MF>(p.aux, dsc, mt16, p.tstep);
                o += ad.p[(long long)m * ad.ld + n];
            }
            if (epi == EPI_ELU) o = elu1(o);
            store_out(y, m, n, o);
            if (p.y2.meta & 15) {                                             // a second copy (the folded hop keeps ELU(dec.4) of every frame)
                const Resolved y2 = resolve<MF>(p.y2, dsc, mt16, p.tstep);
                if (y2.ok) store_out(y2, m, n, o);
            }
        } else if (epi == EPI_SIGMOID) {
            store_out(y, m, n, sigmoid1(v[0]));
        } else if (epi == EPI_CODE) {
            const float pr = sigmoid1(v[0]);
            float z;
            if (p.sample == CS_ENCODE || p.sample == CS_SELECT) {
                z = rintf(pr);                                       // round half to even (torch.round)
            } else {                                                 // BVRNN.forward: straight-through forward value
                float arg = pr;
                if (p.sample == CS_SAMPLE) {
                    const Resolved un = resolve<MF>(p.y2, dsc, mt16, p.tstep);
                    arg = __fadd_rn(__fsub_rn(un.p[(long long)m * un.ld + n], 0.5f), pr);     // (u - 0.5) + p
                }
                z = __fadd_rn(__fsub_rn(rintf(arg), pr), pr);        // round(.) - p + p
            }
            if (p.sample == CS_SELECT) {                             // the concealing decoder: a SELECT between the received code and the generated bit
                const Resolved bt = resolve<MF>(p.aux, dsc, mt16, p.tstep);
                const float sel = bt.p[(long long)m * bt.ld];        // < 0: the frame arrived; else the bits a generated frame gets
                z = (sel > (float)n) ? z : (z != z ? z : 0.5f);
                if (sel < 0.0f) {                                    // (a lost frame's received codes are never read)
                    const Resolved ci = resolve<MF>(p.y2, dsc, mt16, p.tstep);
                    z = ci.p[(long long)m * ci.ld + n];
                }
            } else if (p.var_bit) {
                const Resolved bt = resolve<MF>(p.aux, dsc, mt16, p.tstep);
                const float bits = bt.p[(long long)m * bt.ld];
                z = (bits > (float)n) ? z : (z != z ? z : 0.5f);     // z*m + 0.5*(1-m): a NaN stays a NaN under the mask too (NaN * 0)
            }
            store_out(y, m, n, z);
            const Resolved y3 = resolve<MF>(p.y3, dsc, mt16, p.tstep);
            if (y3.ok) store_out(y3, m, n, pr);
        } else if (epi == EPI_MEL) {
            const float d = v[0];
            if (y.ok) store_out(y, m, n, d);
            const Resolved y2 = resolve<MF>(p.y2, dsc, mt16, p.tstep);
            store_out(y2, m, n, (d - p.mean[n]) / p.stdv[n]);
        } else if (epi == EPI_GRU_PART) {
          if constexpr (NG == 3 && NGRP == 1) {
            // gi = W_ih [phi_x_gen ; phi_z] + b_ih with the phi_z half (+ b_ih) taken from the side branch,
            // gh = W_hh h + b_hh entirely from the side branch.  NGRP == 1: v[0..2] hold the phi_x_gen half.
            const long long H = p.gate_rows;
            const float *pi = p.part_i + (long long)m * p.ldpart + n;
            const float *ph = p.part_h + (long long)m * p.ldpart + n;
            const float gi_r = v[0] + pi[0], gi_z = v[1] + pi[H], gi_n = v[2] + pi[2 * H];      // bias0 is null here
            const float rg = sigmoid1(ph[0] + gi_r);
            const float zg = sigmoid1(ph[H] + gi_z);
            const float ng = tanhf(gi_n + rg * ph[2 * H]);
            const Resolved hprev = resolve<MF>(p.aux, dsc, mt16, p.tstep);
            const float hp = hprev.packed ? hprev.p[packed_off(m, n, hprev.ld)] : hprev.p[(long long)m * hprev.ld + n];
            const float hn = (hp - ng) * zg + ng;
            store_out(y, m, n, hn);
            const Resolved y2 = resolve<MF>(p.y2, dsc, mt16, p.tstep);
            if (y2.ok) store_out(y2, m, n, hn);
          }
        } else if (epi == EPI_GRU) {
          if constexpr (NG == 3 && NGRP == 2) {
            float gi_r = v[0], gi_z = v[1], gi_n = v[2];
            const float gh_r = v[3], gh_z = v[4], gh_n = v[5];
            if (p.y3.meta & 15) {                                            // W_ih[:, H:] phi_z + b_ih, batched over all frames
                const Resolved pg = resolve<MF>(p.y3, dsc, mt16, p.tstep);
                const float *q = pg.p + (long long)m * pg.ld + n;
                gi_r += q[0]; gi_z += q[p.gate_rows]; gi_n += q[2 * p.gate_rows];
            }
            const float rg = sigmoid1(gh_r + gi_r);
            const float zg = sigmoid1(gh_z + gi_z);
            const float ng = tanhf(gi_n + rg * gh_n);
            const Resolved hprev = resolve<MF>(p.aux, dsc, mt16, p.tstep);
            const float hp = hprev.packed ? hprev.p[packed_off(m, n, hprev.ld)] : hprev.p[(long long)m * hprev.ld + n];
            const float hn = (hp - ng) * zg + ng;
            store_out(y, m, n, hn);
            const Resolved y2 = resolve<MF>(p.y2, dsc, mt16, p.tstep);
            if (y2.ok) store_out(y2, m, n, hn);
          }
        }
    }
    if (p.probe && tid == 0) {   // slots: [0, T*nodes) first-workgroup start, [T*nodes, 2*T*nodes) last end
        const int nps = sload_i32(&dsc->nodes_per_step);
        const long long slot_i = (long long)(sload_i32(&dsc->t) + p.tstep) * nps + p.node;
        atomicMin(&p.probe[slot_i], t_start);
        atomicMax(&p.probe[sload_i64(&dsc->T) * nps + slot_i], (unsigned long long)wall_clock64());
    }
}

// The instantiations launch_gemm_skinny can choose, listed once: this table is the only place the host names a skinny kernel.
// `frames` is the multi-frame (MF) twin; the GRU-shaped kernels have none (launch_gemm_skinny refuses frames > 1 for them).
// The order is SkinnyId's (bvc_internal.h).
typedef void (*SkinnyFn)(GemmParams, int);
struct SkinnyKernel {
    int ng, ngrp, nw, mtw;
    SkinnyFn one, frames;
    size_t lds() const { return (size_t)nw * ng * ngrp * mtw * 256 * sizeof(float); }      // NW * NG * NGRP * MTW KiB of partial tiles
};
#define BVC_SKINNY(NG, NGRP, NW, U, MTW, GIL, FRAMES) \
    {NG, NGRP, NW, MTW, gemm_skinny_kernel<NG, NGRP, NW, U, MTW, GIL, false>, FRAMES}
#define BVC_SKINNY_LIN(U, MTW) BVC_SKINNY(1, 1, 8, U, MTW, false, (gemm_skinny_kernel<1, 1, 8, U, MTW, false, true>))
static const SkinnyKernel SKINNY_KERNELS[SK_COUNT] = {
    BVC_SKINNY(3, 2, 8, 1, 1, false, nullptr),           // SK_GRU       natural weights
    BVC_SKINNY(3, 2, 8, 1, 1, true, nullptr),            // SK_GRU_IL    gate-interleaved weights
    BVC_SKINNY(3, 2, 8, 3, 2, true, nullptr),            // SK_GRU_IL2   ... two row tiles per workgroup (96 KiB)
    BVC_SKINNY(3, 1, 8, 4, 1, false, nullptr),           // SK_GRU_PART
    BVC_SKINNY_LIN(2, 1),                                // SK_LIN
    BVC_SKINNY_LIN(4, 1),                                // SK_LIN_LATENCY
    BVC_SKINNY_LIN(8, 2),                                // SK_LIN2
    BVC_SKINNY_LIN(4, 4),                                // SK_LIN4
};

static void launch_skinny(const SkinnyKernel &k, const GemmParams &p, int epi, hipStream_t s) {
    const int n_tiles = p.N / 16, m_tiles = (p.M + 15) / 16, m_groups = (m_tiles + k.mtw - 1) / k.mtw;
    const int grid = 8 * ((n_tiles + 7) / 8) * m_groups;
    if (p.frames > 1) hipLaunchKernelGGL(k.frames, dim3(grid, p.frames), dim3(k.nw * 64), k.lds(), s, p, epi);
    else              hipLaunchKernelGGL(k.one, dim3(grid), dim3(k.nw * 64), k.lds(), s, p, epi);
}

// Dynamic LDS beyond 64 KiB has to be allowed per kernel before its first launch.
int skinny_kernels_init() {
    for (const SkinnyKernel &k : SKINNY_KERNELS) {
        if (k.lds() <= 64 * 1024) continue;
        for (SkinnyFn f : {k.one, k.frames})
            if (f) BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds()));
    }
    return BVC_OK;
}

// mtw = row tiles (of 16) per workgroup: 1 maximises the number of workgroups (lowest latency of a single
// dependent chain), 2 / 4 share every weight fragment among more rows (less L2->CU traffic: higher
// throughput when several independent chains run concurrently).
// How many k-blocks a wave keeps in flight is a trade between one chain and several: chunks of 4 give the shortest
// single launch (4.0 us, 4,180 audio-s/s on one stream) but their load bursts crowd out the other streams' kernels.
// With FOUR chains in flight: chunks of 4 -> 6,750 audio-s/s, of 2 -> 6,830 (one stream 4,080), of 1 -> 6,850 (3,850);
// with three chains the spread was 6,100 / 6,100 / 6,270.  Default: chunks of 2 (1 at K = 2048, 12 waves);
// BVC_LATENCY=1 (`latency`) selects the single-chain optimum.
// EIGHT waves everywhere: a wave is one chunk of the summation order (head of this file), so the wave count is part of the result.
// (Round 1 ran the GRU launch and the K = 2048 layers on 12 / 16 waves for 2 % more throughput with three chains in flight.)
SkinnyPick skinny_pick(int M, int epi, int gate_il, int mtw, bool latency) {
    const int m_tiles = M / 16 + (M % 16 != 0);              // (no M + 15: the test entry passes any M on)
    if (mtw > m_tiles) mtw = m_tiles >= 4 ? 4 : (m_tiles >= 2 ? 2 : 1);
    if (mtw != 2 && mtw != 4) mtw = 1;
    SkinnyId id;
    if (epi == EPI_GRU) {
        // chunks of ONE k-block in flight: a workgroup that bursts 8 KiB of loads per wave only queues them (tools/gru_splitk_bench.hip)
        if (!gate_il)      id = SK_GRU;
        else if (mtw >= 2) id = SK_GRU_IL2;               // (mtw 4: two row tiles per workgroup here - four sets of partial tiles exceed the LDS)
        else               id = SK_GRU_IL;
    } else if (epi == EPI_GRU_PART) {
        id = SK_GRU_PART;
    } else {
        // mtw 1: chunks of 4 k-blocks (52 VGPRs) measured 2 % faster than chunks of 8 (88 VGPRs), alone and
        // with three chains in flight
        if (mtw == 4)      id = SK_LIN4;
        else if (mtw == 2) id = SK_LIN2;
        else               id = latency ? SK_LIN_LATENCY : SK_LIN;
    }
    return {id, SKINNY_KERNELS[id].mtw};
}

// what launch_gemm_skinny launched in this process (tests): see skinny_launch_counts in bvc_internal.h
static std::atomic<long long> g_skinny_launches[2 * SK_COUNT];

void skinny_launch_counts(long long *out) {
    for (int i = 0; i < 2 * SK_COUNT; ++i) out[i] = g_skinny_launches[i].load(std::memory_order_relaxed);
}

int launch_gemm_skinny(const GemmParams &p, int epi, hipStream_t s, int mtw) {
    if (p.M <= 0) return BVC_OK;
    if (p.N % 16) { set_error("gemm_skinny: N=%d not a multiple of 16", p.N); return BVC_EINVAL; }
    int nb = 0;
    for (int i = 0; i < p.nseg; ++i) {
        const DynPtr &x = p.seg[i].x;
        const long long xl = dp_kind(x) == 1 ? x.dim : x.ld;
        if (p.seg[i].K % 16 || xl % (dp_packed(x) ? 16 : 4) || p.seg[i].wnb <= 0) {
            set_error("gemm_skinny: segment %d K=%d row length %lld: K must be a multiple of 16, rows of 4 (16 packed)",
                      i, p.seg[i].K, xl);
            return BVC_EINVAL;
        }
        nb += p.seg[i].K / 16;
    }
    if (p.frames > 1) {                                      // frames in grid.y: static pointers only (the frame counter of a call descriptor is not advanced per block)
        bool ok = dp_kind(p.y) == 0 && (dp_kind(p.aux) == 0) && (p.y2.meta & 15) == 0 && (p.y3.meta & 15) == 0 && !p.probe;
        for (int i = 0; i < p.nseg; ++i) ok = ok && dp_kind(p.seg[i].x) == 0;
        if (!ok) { set_error("gemm_skinny: a multi-frame launch takes static pointers only"); return BVC_EINVAL; }
        if (epi == EPI_GRU || epi == EPI_GRU_PART) { set_error("gemm_skinny: a multi-frame launch has no GRU epilogue (frames=%d)", p.frames); return BVC_EINVAL; }
    }
    if (nb != p.nb_total) { set_error("gemm_skinny: nb_total %d does not match the segments (%d)", p.nb_total, nb); return BVC_EINVAL; }
    static const bool latency_mode = getenv("BVC_LATENCY") != nullptr && getenv("BVC_LATENCY")[0] == '1';
    ProbeScope probe((epi == EPI_GRU || epi == EPI_GRU_PART) ? PK_GRU : PK_LINEAR, s);
    if (p.gate_il && epi != EPI_GRU) { set_error("gemm_skinny: gate-interleaved weights are for the GRU launch only"); return BVC_EINVAL; }
    const SkinnyId id = skinny_pick(p.M, epi, p.gate_il, mtw, latency_mode).id;
    launch_skinny(SKINNY_KERNELS[id], p, epi, s);
    BVC_HIP_TRY(hipGetLastError());
    g_skinny_launches[(p.frames > 1 ? SK_COUNT : 0) + id].fetch_add(1, std::memory_order_relaxed);
    return BVC_OK;
}

__global__ void step_advance_kernel(CallDesc *d, int by) {
    if (threadIdx.x == 0) d->t = d->t + by;
}

int launch_step_advance(CallDesc *d, int by, hipStream_t s) {
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, s, d, by);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

__global__ void set_desc_kernel(CallDesc *d, CallDesc v) {
    if (threadIdx.x == 0) *d = v;
}

int launch_set_desc(CallDesc *d, const CallDesc &v, hipStream_t s) {
    hipLaunchKernelGGL(set_desc_kernel, dim3(1), dim3(64), 0, s, d, v);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
