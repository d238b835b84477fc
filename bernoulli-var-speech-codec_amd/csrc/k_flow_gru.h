// The persistent recurrence's GRU cell (device code, included by k_flow.hip behind k_flow_layers.h): the rounds of the gate
// weights' stream, the operand fetches, the cell's reduction and epilogue, and the layer for one chain (flow_gru) or for the
// chains of a workgroup, two at a time (flow_gru_chains).
#pragma once
#include "k_flow_layers.h"

namespace bvc {
namespace {

// One round of a GRU segment: HALF k-blocks x 3 gates of weights (gate-interleaved [n/16][k/16][gate][lane][4]).
template <int HALF>
__device__ __forceinline__ void gru_issue_w(GPtr ub, unsigned l16, int h0, f32x4 (&w3)[HALF][3]) {
#pragma unroll
    for (int u = 0; u < HALF; ++u)
#pragma unroll
        for (int q = 0; q < 3; ++q) w3[u][q] = wload(ub, l16, (h0 + u) * 3 + q);
}
template <int PER, int HALF>
__device__ __forceinline__ void gru_round(const f32x4 (&w3)[HALF][3], const u32x4 (&xr)[PER], int h0, f32x4 (&acc)[3]) {
#pragma unroll
    for (int u = 0; u < HALF; ++u) {
        const f32x4 xv = __builtin_bit_cast(f32x4, xr[h0 + u]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = mfma16(w3[u][q][e], xv[e], acc[q]);
    }
}

// operand blocks of an input this wave has already fetched and verified earlier in the frame (h at the first layer, phi_z
// at dec.0): complete, and not re-armed before the next frame, so neither a flag wait nor a check is needed
template <int PER>
__device__ __forceinline__ void gru_issue_known(const FlowWg &g, unsigned buf, int nb, u32x4 (&xr)[PER]) {
    const int kb0 = g.wave * PER;
    FlowSrc s;
    s.base = __builtin_amdgcn_readfirstlane(buf + (unsigned)(g.mtile * nb + kb0) * 1024u);
    s.vl = (unsigned)g.lane * 16u;
    flow_issue<PER>(g, s, xr);
}

// operand blocks of the input that is being produced right now: wait, fetch, verify
template <int PER>
__device__ __forceinline__ void gru_fetch_fresh(const FlowWg &g, unsigned buf, int nb, u32x4 (&xr)[PER], bool &give_up, unsigned code) {
    const int kb0 = g.wave * PER;
    unsigned spins = 0;
    const FlowSrc src = flow_wait<PER>(g, buf, nb, kb0, give_up, code, spins);
    bool again;
    do {
        flow_issue<PER>(g, src, xr);
        bool bad = false;
#pragma unroll
        for (int u = 0; u < PER; ++u) bad |= is_poison4(xr[u]);
        again = __any(bad) && !give_up;
        if (again) flow_spin(g, g.lane, spins, give_up, code);
    } while (again);
}

// The GRU cell's reduction and epilogue for ONE chain (c.g.mtile / c.row / c.rowok / c.fr say which): gi / gh are this wave's partial
// gate sums; prefetch: request the next frame's first weights (wn) in front of the first barrier.
template <bool ENCODE, int PERN, int NW>
__device__ __forceinline__ void gru_epilogue(const FlowCtx &c, int hopid, int hb, int n0, unsigned ytile, const f32x4 (&gi)[3], const f32x4 (&gh)[3],
                                             const FlowLin nxt, f32x4 (&wn)[PERN], bool prefetch) {
    const FlowWg &g = c.g;
    const auto &a = *c.a;
    const int lane = g.lane, wave = g.wave;
    const long long H = (long long)hb * 16;
    const unsigned hbuf = (unsigned)(FB_H * 2) * c.sb;
    if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 3);
    // The cell's epilogue is spread over the waves (one wave doing all of it - 48 partial tiles to sum, two sigmoids and a tanh for
    // each of its four outputs per lane - took 1.5 us with seven waves idle): wave k < 6 sums quantity k (gi_r, gi_z, gi_n, gh_r,
    // gh_z, gh_n) over the eight waves and adds its bias, wave j < 4 then evaluates the cell for output j of every lane, wave 0
    // gathers the four and publishes.  Same operations in the same order per output as the one-wave form.
    // Their operands are requested now: they arrive while the other waves reach the barrier.
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f}, p4 = {0.f, 0.f, 0.f, 0.f};
    float hp = 0.0f;
    if (wave < 3) {
        if (ENCODE) b4 = *reinterpret_cast<const f32x4 *>(a.b_ih + wave * H + n0);
        if (!ENCODE && c.rowok) p4 = *reinterpret_cast<const f32x4 *>(a.part_gru + c.fr * 3 * H + wave * H + n0);
    } else if (wave < 6) {
        b4 = *reinterpret_cast<const f32x4 *>(a.b_hh + (wave - 3) * H + n0);
    }
    // this workgroup's own block of h(t): written by itself a frame ago (or the initial state); wave j takes element j of each lane
    if (wave < 4) hp = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(g.rs, hbuf + c.par * c.sb + ytile + (unsigned)wave * 4u, 0, AUX_SC1));
    if (prefetch) {    // the first layer of the next frame (after the last frame a harmless extra request: no value is carried across)
        const GPtr ub = uniform_ptr(nxt.w, ((size_t)g.ntile * nxt.wnb + wave * PERN) * g.wmul);
#pragma unroll
        for (int u = 0; u < PERN; ++u) wn[u] = wload(ub, (unsigned)lane * 16u, u);
    }
    float *red_gru = c.red_gru;
    float *red2 = c.red_lin + (c.hopctr & 1u) * (NW * 256);            // [6][256] sums | [256] outputs: the layer partials' free slot
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        *reinterpret_cast<f32x4 *>(red_gru + ((wave * 6 + q) * 64 + lane) * 4) = gi[q];
        *reinterpret_cast<f32x4 *>(red_gru + ((wave * 6 + 3 + q) * 64 + lane) * 4) = gh[q];
    }
    __syncthreads();
    if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 4);
    if (wave < 6) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(red_gru + (wave * 64 + lane) * 4);
#pragma unroll
        for (int w = 1; w < NW; ++w) v += *reinterpret_cast<const f32x4 *>(red_gru + ((w * 6 + wave) * 64 + lane) * 4);
        v += b4;                                           // gi: (sum + b_ih) + the pre-computed phi_z part; gh: sum + b_hh
        if (wave < 3) v += p4;
        *reinterpret_cast<f32x4 *>(red2 + (wave * 64 + lane) * 4) = v;
    }
    __syncthreads();
    if (wave < 4) {
        float sgm[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) sgm[k] = red2[(k * 64 + lane) * 4 + wave];
        const float rg = sigmoid1(sgm[3] + sgm[0]);
        const float zg = sigmoid1(sgm[4] + sgm[1]);
        const float ng = tanhf(sgm[2] + rg * sgm[5]);
        red2[6 * 256 + lane * 4 + wave] = (hp - ng) * zg + ng;
    }
    __syncthreads();
    if (wave == 0) {
        const f32x4 hn = *reinterpret_cast<const f32x4 *>(red2 + 6 * 256 + lane * 4);
        if (a.all_h && c.rowok && c.t + 1 < a.T) *reinterpret_cast<f32x4 *>(a.all_h + (c.fr + 1) * H + n0) = hn;   // all_h[:, t+1], bvrnn.py:205
        // h(t)'s slot is NOT re-armed here: other workgroups may still be reading h(t) in their own GRU layer.  It is re-armed
        // by the second layer of frame t+1 (REARM_H), whose inputs prove that every workgroup has left frame t.
        __builtin_amdgcn_raw_buffer_store_b128(publishable(hn, c.rowok), g.rs, hbuf + (c.par ^ 1u) * c.sb + ytile, 0, AUX_SC1);
        flow_stamp(c, hopid, 1);
    }
    // red_gru is single-buffered, also when chains are interleaved (MULTI): its next writers are past this call's three barriers,
    // the partials' readers between the first and the second
}

// GRU cell (PyTorch gate order r, z, n; bvrnn.py:206,227): gh = W_hh h, gi = W_ih [phi_x_gen ; phi_z]; in decode the
// phi_z half of gi (+ b_ih) arrives pre-computed (a.part_gru).  Segments in the order their inputs become ready.
template <int PER, bool ENCODE, int PERN, bool FILL, int NW = 8>
__device__ __forceinline__ void flow_gru(FlowCtx &c, int hopid, int hb, const FlowLin nxt, f32x4 (&wn)[PERN]) {
    const FlowWg &g = c.g;
    const auto &a = *c.a;
    if (g.ntile >= hb) {
        if (c.pre_now) {
            wzero(wn);
        }
        return;
    }
    int lane = g.lane;
    const int wave = g.wave;
    // (opaque per layer: what is derived from the lane - tile offsets, feature indices, their float forms - is then recomputed here
    // instead of being hoisted out of the frame loop for all fourteen layers and SPILLED; a spill reload in an epilogue waits, in
    // order, for every prefetch the wave has in flight)
    asm volatile("" : "+v"(lane));
    const unsigned code = (unsigned)((c.t << 4) | (unsigned)hopid) | 0x80000000u;
    const int n0 = g.ntile * 16 + (lane >> 4) * 4;
    const unsigned ytile = (unsigned)((g.mtile * hb + g.ntile) * 1024 + lane * 16);
    const unsigned hbuf = (unsigned)(FB_H * 2) * c.sb;
    flow_stamp(c, hopid, 0);
    f32x4 gi[3], gh[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        gi[q] = FILL ? c.fgi[q] : (f32x4){0.f, 0.f, 0.f, 0.f};
        gh[q] = FILL ? c.fgh[q] : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // h(t) and (encode) phi_z(z_t) are complete and were verified by this very wave earlier in the frame: their blocks are
    // requested at once and multiplied while phi_x(d_t), the input produced last, is still on its way
    // The weights stream through two register sets: the request for round i+1 is issued before round i is multiplied.
    if (!(PER == 1 && wave >= hb)) {                       // (wave-uniform) a wave without a k-block of its own contributes zeros
        constexpr int HALF = FILL ? (PER >= BVC_GRU_ROUNDS_FILL ? PER / BVC_GRU_ROUNDS_FILL : 1) : (PER >= 4 ? PER / 4 : 1);       // k-blocks per round
        constexpr int RPS = PER / HALF;                    // rounds per segment
        constexpr int NSEG = FILL ? 1 : (ENCODE ? 3 : 2);  // FILL: the h and phi_z products were accumulated earlier in the frame
        constexpr int NR = NSEG * RPS;
        const int kb0 = wave * PER;
        const unsigned l16 = (unsigned)lane * 16u;
        const GPtr uh = uniform_ptr(a.w_hh, ((size_t)g.ntile * hb + kb0) * 3 * g.wmul);
        const GPtr uz = uniform_ptr(a.w_ihz, ((size_t)g.ntile * 2 * hb + kb0) * 3 * g.wmul);
        const GPtr ux = uniform_ptr(a.w_ihx, ((size_t)g.ntile * 2 * hb + kb0) * 3 * g.wmul);
        u32x4 xa[PER], xb[PER];
        // The weights stream through DEPTH register sets: the request for round i + DEPTH - 1 is issued before round i is multiplied.
        // The scheduling fences make that true: hipcc sinks a load to just in front of its first use when left alone (it schedules
        // for few live registers although this kernel may use all 256), and every round then waited a full cache round trip for
        // its own weights - the GRU hop measured 6 us against the 2.6 us its 192 MFMAs per SIMD take.
        constexpr int DEPTH = (FILL && BVC_GRU_DEPTH > 2) ? (BVC_GRU_DEPTH < NR ? BVC_GRU_DEPTH : NR) : 2;
        f32x4 wr[DEPTH][HALF][3];
        auto wsrc = [&](int i) { const int sn = i / RPS; return FILL ? ux : (sn == 0 ? uh : ((ENCODE && sn == 1) ? uz : ux)); };
#pragma unroll
        for (int i = 0; i < DEPTH - 1; ++i)
            if (i < NR) gru_issue_w<HALF>(wsrc(i), l16, (i % RPS) * HALF, wr[i]);
        if (!FILL) gru_issue_known<PER>(g, hbuf + c.par * c.sb, hb, xa);
        if (!FILL && ENCODE) gru_issue_known<PER>(g, (unsigned)(FB_Q3 * 2 + c.par) * c.sb, hb, xb);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int sg = i / RPS, h0 = (i % RPS) * HALF;
            if (i + DEPTH - 1 < NR) gru_issue_w<HALF>(wsrc(i + DEPTH - 1), l16, ((i + DEPTH - 1) % RPS) * HALF, wr[(i + DEPTH - 1) % DEPTH]);
            if (BVC_GRU_FENCE) __builtin_amdgcn_sched_barrier(0);
            if (i == (NSEG - 1) * RPS) {                   // the last segment's input, phi_x(d_t): wait, fetch, verify.  (What was requested in front
                gru_fetch_fresh<PER>(g, (unsigned)(FB_G3 * 2 + c.par) * c.sb, hb, xa, c.give_up, code);     // of the poll travels during the wait.)
                if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 2);        // (here: flags seen AND operands fetched)
            }
            if (FILL)                   gru_round<PER, HALF>(wr[i % DEPTH], xa, h0, gi);
            else if (sg == 0)           gru_round<PER, HALF>(wr[i % DEPTH], xa, h0, gh);
            else if (ENCODE && sg == 1) gru_round<PER, HALF>(wr[i % DEPTH], xb, h0, gi);
            else                        gru_round<PER, HALF>(wr[i % DEPTH], xa, h0, gi);
            if (BVC_GRU_FENCE) __builtin_amdgcn_sched_barrier(0);
        }
    }
    gru_epilogue<ENCODE, PERN, NW>(c, hopid, hb, n0, ytile, gi, gh, nxt, wn, c.pre_now && !(BVC_FLOW_PARKL && FILL && PER == 8));
}

// MULTI: the GRU cell for the chains of this workgroup, two chains at a time: a round's weights (two k-blocks x three gates, streamed
// through two register sets as in flow_gru) are multiplied with BOTH chains' operand blocks, so the 576 KiB (encode; decode 384) of
// gate weights per workgroup cross the compute unit's memory path once per pair instead of once per chain - they were a third of
// everything a workgroup requested per frame.  Per chain and wave the same products in the same order as flow_gru (segments h,
// phi_z, phi_x; k ascending), hence the same bits; the cells' epilogues run one after the other (gru_epilogue).
template <int PER, bool ENCODE, int PERN, int NW>
__device__ __forceinline__ void flow_gru_chains(FlowCtx &c, int hopid, int hb, const FlowLin nxt, f32x4 (&wn)[PERN], int mt0, int nch, long long T) {
    static_assert(PER == 8, "interleaved chains are built for h_dim 1024");
    FlowWg &g = c.g;
    const auto &a = *c.a;
    if (g.ntile >= hb) {
        wzero(wn);
        return;
    }
    int lane = g.lane;
    const int wave = g.wave;
    asm volatile("" : "+v"(lane));                         // (see flow_layer)
    const unsigned code = (unsigned)((c.t << 4) | (unsigned)hopid) | 0x80000000u;
    const int n0 = g.ntile * 16 + (lane >> 4) * 4;
    const unsigned hbuf = (unsigned)(FB_H * 2) * c.sb;
    constexpr int HALF = 2, RPS = PER / HALF, NSEG = ENCODE ? 3 : 2, NR = NSEG * RPS;
    const int kb0 = wave * PER;
    const unsigned l16 = (unsigned)lane * 16u;
    flow_stamp(c, hopid, 0);
    for (int p0 = 0; p0 < nch; p0 += 2) {
        const bool two = p0 + 1 < nch;                     // (uniform) an odd last chain goes alone: its partner's products are skipped
        FlowWg gA = g, gB = g;
        gA.mtile = mt0 + p0;
        gB.mtile = mt0 + p0 + (two ? 1 : 0);
        f32x4 giA[3], ghA[3], giB[3], ghB[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) giA[q] = ghA[q] = giB[q] = ghB[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const GPtr uh = uniform_ptr(a.w_hh, ((size_t)g.ntile * hb + kb0) * 3 * g.wmul);
        const GPtr uz = uniform_ptr(a.w_ihz, ((size_t)g.ntile * 2 * hb + kb0) * 3 * g.wmul);
        const GPtr ux = uniform_ptr(a.w_ihx, ((size_t)g.ntile * 2 * hb + kb0) * 3 * g.wmul);
        u32x4 xA[PER], xB[PER];
        f32x4 wr[2][HALF][3];
        gru_issue_w<HALF>(uh, l16, 0, wr[0]);
        gru_issue_known<PER>(gA, hbuf + c.par * c.sb, hb, xA);      // h(t) of both chains: complete since the frame began
        gru_issue_known<PER>(gB, hbuf + c.par * c.sb, hb, xB);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int sg = i / RPS, h0 = (i % RPS) * HALF;
            if (i + 1 < NR) {
                const int sn = (i + 1) / RPS, hn0 = ((i + 1) % RPS) * HALF;
                gru_issue_w<HALF>(sn == 0 ? uh : ((ENCODE && sn == 1) ? uz : ux), l16, hn0, wr[(i + 1) & 1]);
            }
            // a chain's operand blocks of the NEXT segment are requested as soon as its last round of this one is multiplied: they
            // travel under the partner's round (phi_x(d_t), produced last, is waited for, fetched and verified; h and phi_z are known)
            const bool seg_end = (i % RPS == RPS - 1) && i + 1 < NR;
            const bool next_fresh = (i + 1) / RPS == NSEG - 1;
            if (sg == 0) gru_round<PER, HALF>(wr[i & 1], xA, h0, ghA);
            else         gru_round<PER, HALF>(wr[i & 1], xA, h0, giA);
            if (seg_end) {
                if (next_fresh) gru_fetch_fresh<PER>(gA, (unsigned)(FB_G3 * 2 + c.par) * c.sb, hb, xA, c.give_up, code);
                else            gru_issue_known<PER>(gA, (unsigned)(FB_Q3 * 2 + c.par) * c.sb, hb, xA);
            }
            if (two) {
                if (sg == 0) gru_round<PER, HALF>(wr[i & 1], xB, h0, ghB);
                else         gru_round<PER, HALF>(wr[i & 1], xB, h0, giB);
            }
            if (seg_end) {
                if (next_fresh) { if (two) gru_fetch_fresh<PER>(gB, (unsigned)(FB_G3 * 2 + c.par) * c.sb, hb, xB, c.give_up, code); }
                else            gru_issue_known<PER>(gB, (unsigned)(FB_Q3 * 2 + c.par) * c.sb, hb, xB);
            }
        }
        // the two cells' epilogues, one after the other (one set of partial tiles in LDS)
        for (int k = 0; k < (two ? 2 : 1); ++k) {
            FlowCtx ce = c;
            flow_set_chain(ce, mt0 + p0 + k, lane, a.B, T, c.t);
            ce.probe = c.probe && p0 == 0 && k == 0;
            const unsigned ytile = (unsigned)((ce.g.mtile * hb + g.ntile) * 1024 + lane * 16);
            const bool lastc = p0 + k == nch - 1;
            if (k == 0) gru_epilogue<ENCODE, PERN, NW>(ce, hopid, hb, n0, ytile, giA, ghA, nxt, wn, lastc);
            else        gru_epilogue<ENCODE, PERN, NW>(ce, hopid, hb, n0, ytile, giB, ghB, nxt, wn, lastc);
        }
    }
}

}  // namespace
}  // namespace bvc
