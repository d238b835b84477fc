// The persistent recurrence's layer bodies (device code, included by k_flow.hip behind the compile-time tunables and
// k_flow_handoff.h): a segment's products, the filler quanta, the per-workgroup state of the frame loop, the stamps, the
// publishing epilogue, and a layer for one chain (flow_layer) or for all chains of a workgroup (flow_layer_chains).
#pragma once
#include "k_flow_handoff.h"

namespace bvc {
namespace {

// What a layer wants done between a segment's operand requests and its products: the next layer's weights requested
// (BVC_FLOW_EARLYW), diagnostic stamps taken.
typedef u32x4 __attribute__((address_space(3))) *LdsX;      // this wave's stash of operand blocks in LDS: [k-block][lane]
struct SegHook {
    const float *nw; int nwnb; bool pre;           // next layer's packed weights, k-blocks per row; request them here?
    unsigned long long *st_flags, *st_done;       // BVC_FLOW_DIAG: where to stamp "flags seen" / "products done" (or null)
    LdsX stash;                                    // keep the verified operand blocks of this segment there (or null)
};
__device__ __forceinline__ SegHook no_hook() { return SegHook{nullptr, 0, false, nullptr, nullptr, (LdsX)0}; }

// acc += W[ntile rows][segment] . X[segment]   for this wave's share of the segment's k-blocks
// (FEARLY: unused.  It and the constant of that name in flow_layer are what is left of a dropped experiment, the quantum's weights
// requested in here: without them hipcc orders a few instructions of the two narrowest concealing kernels differently,
// bvrnn_flow_kernel<1, true, false, 8, false, -1, true> and <1, true, true, 8, false, -1, true> - profiles/flow_fold.md.)
template <int PER, int PERN, bool FEARLY = false>
__device__ __forceinline__ void lin_segment(const FlowWg &g, const float *w, int wnb, int nb, unsigned buf, bool w_ready,
                                            f32x4 (&wv)[PER], f32x4 &acc, bool &give_up, unsigned code, int kb_off,
                                            const SegHook &hk, f32x4 (&wn)[PERN]) {
    const int kb0 = kb_off + g.wave * PER;
    if (PER == 1 && kb0 >= nb) return;                     // wave-uniform: fewer k-blocks than waves
    if (!w_ready) {
        const GPtr ub = uniform_ptr(w, ((size_t)g.ntile * wnb + kb0) * g.wmul);
#pragma unroll
        for (int u = 0; u < PER; ++u) wv[u] = wload(ub, (unsigned)g.lane * 16u, u);
    }
    unsigned spins = 0;
    const FlowSrc src = flow_wait<PER>(g, buf, nb, kb0, give_up, code, spins);
    if (BVC_FLOW_DIAG && hk.st_flags) *hk.st_flags = __builtin_amdgcn_s_memrealtime();
    const f32x4 acc_in = acc;
    u32x4 xr[PER];
    flow_issue<PER>(g, src, xr);
    // behind the operand requests (nothing this layer waits for queues behind them; a wave's loads return in order):
    if (hk.pre) {                                          // the next layer's weights
        const GPtr ub = uniform_ptr(hk.nw, ((size_t)g.ntile * hk.nwnb + g.wave * PERN) * g.wmul);
#pragma unroll
        for (int u = 0; u < PERN; ++u) wn[u] = wload(ub, (unsigned)g.lane * 16u, u);
    }
    for (;;) {
        // The blocks are multiplied as they arrive (the loads return in order); whether one of them still held the
        // sentinel is only known at the end: then the products are thrown away and everything is fetched again.
        f32x4 a2 = acc_in;
        bool bad = false;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const f32x4 xv = __builtin_bit_cast(f32x4, xr[u]);
#pragma unroll
            for (int e = 0; e < 4; ++e) a2 = mfma16(wv[u][e], xv[e], a2);
            __builtin_amdgcn_sched_barrier(0);                             // block u's products before block u + 1 is waited for
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) bad |= is_poison4(xr[u]);
        if (!(__any(bad) && !give_up)) {
            acc = a2;
            if (hk.stash) {
#pragma unroll
                for (int u = 0; u < PER; ++u) hk.stash[(kb_off / 8 * PER + u) * 64 + g.lane] = xr[u];
            }
            break;
        }
        flow_spin(g, g.lane, spins, give_up, code);
        flow_issue<PER>(g, src, xr);
    }
    if (BVC_FLOW_DIAG && hk.st_done) *hk.st_done = __builtin_amdgcn_s_memrealtime();
}
template <int PER>
__device__ __forceinline__ void lin_segment(const FlowWg &g, const float *w, int wnb, int nb, unsigned buf, bool w_ready,
                                            f32x4 (&wv)[PER], f32x4 &acc, bool &give_up, unsigned code, int kb_off = 0) {
    f32x4 none[1];
    lin_segment<PER, 1>(g, w, wnb, nb, buf, w_ready, wv, acc, give_up, code, kb_off, no_hook(), none);
}

// One filler quantum: acc += W[ntile rows][this wave's k-blocks] . X for an input that is complete and was verified by this very
// wave earlier in the frame (no wait, no check).  GATE >= 0: gate-interleaved GRU weights, that gate only; GATE == -1: plain
// packed weights; GATE == -2: no filler.  The operands are REQUESTED before a layer's reduction barrier and MULTIPLIED behind its
// epilogue, i.e. while the inputs of the next layer are still being produced.
struct FlowFill { const float *w; int wnb; int nb; unsigned buf; };
template <int PER, int GATE>
__device__ __forceinline__ bool fill_active(const FlowWg &g, const FlowFill &f) {
    return GATE != -2 && g.ntile < f.nb && !(PER == 1 && g.wave >= f.nb);       // (these products have h_dim outputs and inputs)
}
template <int PER, int GATE>
__device__ __forceinline__ void fill_issue(const FlowWg &g, const FlowFill &f, f32x4 (&wv)[PER], u32x4 (&xr)[PER]) {
    // (xr: unused, like FlowFill::buf - the quantum's operands come out of the stash.  Both are still here because hipcc compiles kernels to
    // different instructions without them (profiles/flow_fold.md): without xr the encode and the concealing filler kernels of h_dim 512 and
    // 1024, bvrnn_flow_kernel<4 | 8, true, true, 8, false, -1, false | true>; without buf the plain ones of h_dim <= 128,
    // bvrnn_flow_kernel<1, true, false, 8, false, -1, false | true>, which then spill 26 SGPRs instead of 27 / 29.)
    if (!fill_active<PER, GATE>(g, f)) {                   // (defined on every path: no stale value stays live across the frame loop)
#pragma unroll
        for (int u = 0; u < PER; ++u) { wv[u] = (f32x4){0.f, 0.f, 0.f, 0.f}; xr[u] = (u32x4){0u, 0u, 0u, 0u}; }
        return;
    }
    const int kb0 = g.wave * PER;
    const unsigned l16 = (unsigned)g.lane * 16u;
    const GPtr ub = uniform_ptr(f.w, (GATE >= 0 ? ((size_t)g.ntile * f.wnb + kb0) * 3 + GATE : (size_t)g.ntile * f.wnb + kb0) * g.wmul);
#pragma unroll
    for (int u = 0; u < PER; ++u) wv[u] = wload(ub, l16, GATE >= 0 ? u * 3 : u);
}
template <int PER, int GATE>
__device__ __forceinline__ void fill_multiply(const FlowWg &g, const FlowFill &f, const f32x4 (&wv)[PER], f32x4 &acc, LdsX stash) {
    if (!fill_active<PER, GATE>(g, f)) return;
    u32x4 xs[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) xs[u] = stash[u * 64 + g.lane];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const f32x4 xv = __builtin_bit_cast(f32x4, xs[u]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma16(wv[u][e], xv[e], acc);
    }
}

// per-workgroup state of the frame loop
// The kernel arguments are read through a constant-address-space pointer that is made opaque once per frame: their
// fields then come in by scalar loads where they are used, instead of ~100 SGPRs being filled (and spilled) up front.
typedef const FlowArgs __attribute__((address_space(4))) *FlowArgsC;

struct FlowCtx {
    FlowWg g;
    FlowArgsC a;
    float *red_lin, *red_gru;
    float *red_chain;        // MULTI: [2][4][NW][256] partial tiles of a group of chains (flow_layer_chains)
    unsigned sb;             // bytes per flow buffer slot: kept in a register (every layer needs it before its first request; a scalar
                             // load there is a cache round trip on the critical path)
    LdsX stash;              // this wave's operand blocks of the quanta's input (fetched and verified for the layer that consumes them first)
    LdsX lpark;              // BVC_FLOW_PARKL: this wave's eight blocks of the first layer's weights
    volatile unsigned __attribute__((address_space(3))) *pubflag;      // BVC_FLOW_PARTNER_WAIT: hop count of wave 0's last publishing store
    unsigned par;            // frame parity
    long long t, fr;         // frame; (utterance, frame) index of this lane's row
    int row;
    bool rowok, give_up;
    bool pre_now;            // MULTI: the next layer's weights are requested by the LAST chain of a layer only (true otherwise)
    bool probe;              // this lane records layer entry / exit times (bench instrumentation)
    unsigned hopctr;
    // FILL: this wave's partial sums of the products whose inputs exist long before their layer - W_hh h, W_ih[:, H:] phi_z, the
    // h half of dec.0 - computed one quantum at a time in the waits behind other layers
    f32x4 fgh[3], fgi[3], fd0;
};

// the context of one chain (utterance group mtile) of a workgroup that interleaves several: its rows, this frame's (utterance, frame) index
__device__ __forceinline__ void flow_set_chain(FlowCtx &c, int mtile, int lane, int B, long long T, long long t) {
    c.g.mtile = mtile;
    c.row = mtile * 16 + (lane & 15);
    c.rowok = c.row < B;
    c.fr = (long long)c.row * T + t;
}

__device__ __forceinline__ unsigned long long *flow_stamp_slot(const FlowCtx &c, int hopid, int which) {
    if (!c.probe) return nullptr;
    const auto &a = *c.a;
    return a.probe + ((long long)which * a.T + c.t) * a.probe_nodes + (hopid - a.probe_first);
}
// which: 0 layer entered, 1 output published (wave 0); BVC_FLOW_DIAG: 2 flags of the (last) segment seen, 3 its products done,
// 4 barrier passed, 5 layer left (behind the filler quantum)
__device__ __forceinline__ void flow_stamp(const FlowCtx &c, int hopid, int which) {
    unsigned long long *p = flow_stamp_slot(c, hopid, which);
    if (p) *p = __builtin_amdgcn_s_memrealtime();
}

// Wave 0 of a workgroup, after the barrier: sum the waves' partial tiles (fixed order), apply the layer's epilogue and publish the
// 1 KiB block; re-arm (poison) this workgroup's block of the other frame parity.
template <int EPI, bool ADD, bool REARM_H, int NW>
__device__ __forceinline__ void flow_publish(const FlowCtx &c, int hopid, const float *r, int n0, unsigned ytile, int ntiles, int out,
                                             const f32x4 bias4, const f32x4 add4, const f32x4 mean4, const f32x4 std4, float bitsv,
                                             const f32x4 recv4 = (f32x4){0.f, 0.f, 0.f, 0.f}) {
    const FlowWg &g = c.g;
    const auto &a = *c.a;
    const int lane = g.lane;
    __builtin_amdgcn_s_setprio(3);                     // the publishing wave goes first: its SIMD partner may be multiplying a filler
    f32x4 v = *reinterpret_cast<const f32x4 *>(r + lane * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *reinterpret_cast<const f32x4 *>(r + (w * 64 + lane) * 4);
    v += bias4;
    f32x4 o, pr = {0.f, 0.f, 0.f, 0.f};
    if (EPI == FE_ELU || EPI == FE_ELU_KEEP) {
        if (ADD) v += add4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = elu1(v[j]);
    } else if (EPI == FE_CODE) {                       // bvrnn.py:189-194
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pr[j] = sigmoid1(v[j]);
            float z = rintf(pr[j]);                    // round half to even (torch.round)
            if (a.var_bit) z = (bitsv > (float)(n0 + j)) ? z : (z != z ? z : 0.5f);    // z*m + 0.5*(1-m): NaN * 0 is NaN (bvrnn.py:193-194)
            o[j] = z;
        }
    } else if (EPI == FE_CODE_SEL) {                   // the concealing decoder: bitsv is the selector (< 0: the frame arrived), recv4 the received codes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pr[j] = sigmoid1(v[j]);                    // the prior's probability (bvrnn.py:68-73)
            float z = rintf(pr[j]);
            z = (bitsv > (float)(n0 + j)) ? z : (z != z ? z : 0.5f);
            o[j] = bitsv < 0.0f ? recv4[j] : z;        // a select: what a lost frame's codes hold reaches nothing
        }
    } else {                                           // FE_MEL, bvrnn.py:202-204
        if (a.mel && c.rowok) *reinterpret_cast<f32x4 *>(a.mel + c.fr * (ntiles * 16) + n0) = v;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean4[j]) / std4[j];
    }
    unsigned pv = FLOW_POISON;
    asm volatile("" : "+v"(pv));                       // re-materialised here (hoisted out of the frame loop it gets spilled)
    const u32x4 poison4 = {pv, pv, pv, pv};
    const unsigned ob = (unsigned)(out * 2) * c.sb;
    __builtin_amdgcn_raw_buffer_store_b128(publishable(o, c.rowok), g.rs, ob + c.par * c.sb + ytile, 0, AUX_SC1);
    __builtin_amdgcn_raw_buffer_store_b128(poison4, g.rs, ob + (c.par ^ 1u) * c.sb + ytile, 0, AUX_SC1);
    // The slot that will receive h(t+1) still holds h(t-1).  This layer's input was produced by workgroups that had all
    // consumed h(t), i.e. had all finished frame t-1: nobody reads h(t-1) any more (same tile shape as this layer's).
    if (REARM_H) __builtin_amdgcn_raw_buffer_store_b128(poison4, g.rs, (unsigned)(FB_H * 2 + (c.par ^ 1u)) * c.sb + ytile, 0, AUX_SC1);
    if (EPI == FE_ELU_KEEP && c.rowok && a.keep) *reinterpret_cast<f32x4 *>(a.keep + c.fr * (ntiles * 16) + n0) = o;     // (behind the hand-off stores; encode keeps u only for the fused forward)
    if ((EPI == FE_CODE || EPI == FE_CODE_SEL) && c.rowok) {      // the call's outputs: behind the hand-off stores as well (-0.06 ms per step)
        *reinterpret_cast<f32x4 *>(a.codes + c.fr * (ntiles * 16) + n0) = o;
        if (a.prob) *reinterpret_cast<f32x4 *>(a.prob + c.fr * (ntiles * 16) + n0) = pr;
    }
    __builtin_amdgcn_s_setprio(0);
    flow_stamp(c, hopid, 1);
}

// One layer: y = epi( sum_s W_s . x_s + bias [+ addend] ).  PER k-blocks per wave and segment (compile time), one or
// two segments (the one whose input is produced last comes last), PRE_IN: wv already holds segment 0's weights,
// PRE_OUT: request `nxt`'s weights (PERN blocks per wave) into wn (inside the last segment, or before the reduction).
// FGATE != -2: a filler quantum rides on this layer - its weights are requested in front of the reduction barrier and multiplied
// behind the barrier, in the shadow of the epilogue and the hand-off.
template <int PER, int EPI, bool TWO, bool ADD, bool PRE_IN, bool PRE_OUT, int PERN, bool REARM_H = false, int FGATE = -2, int NW = 8>
__device__ __forceinline__ void flow_layer(FlowCtx &c, int hopid, const FlowLin l0, int src0, const FlowLin l1, int src1,
                                           int nb, int ntiles, int out, f32x4 (&wv)[PER], const FlowLin nxt, f32x4 (&wn)[PERN],
                                           const f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, const FlowFill fill = FlowFill{nullptr, 0, 0, 0u},
                                           f32x4 *facc = nullptr) {
    const FlowWg &g = c.g;
    const auto &a = *c.a;
    f32x4 fw[PERN];
    u32x4 fx[PERN];
    if (g.ntile >= ntiles) {                               // uniform per workgroup (layers narrower than h_dim)
        if (PRE_OUT && c.pre_now) {
            wzero(wn);
        }
        if (FGATE != -2) {                                 // nothing else to do in this layer: the whole quantum right away
            fill_issue<PERN, FGATE>(g, fill, fw, fx);
            fill_multiply<PERN, FGATE>(g, fill, fw, *facc, c.stash);
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
    const unsigned ytile = (unsigned)((g.mtile * ntiles + g.ntile) * 1024 + lane * 16);
    flow_stamp(c, hopid, 0);
    // ---- epilogue operands of wave 0, requested up front
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, add4 = {0.f, 0.f, 0.f, 0.f}, mean4 = {0.f, 0.f, 0.f, 0.f}, std4 = {1.f, 1.f, 1.f, 1.f};
    float bitsv = 0.0f;
    f32x4 recv4 = {0.f, 0.f, 0.f, 0.f};
    if (wave == 0) {
        if (l0.bias) bias4 = *reinterpret_cast<const f32x4 *>(l0.bias + n0);
        if (ADD && c.rowok) add4 = *reinterpret_cast<const f32x4 *>(a.part0 + c.fr * (ntiles * 16) + n0);
        if (EPI == FE_CODE && a.var_bit && c.rowok) bitsv = a.bits[c.fr];
        if (EPI == FE_CODE_SEL && c.rowok) {               // the selector and the received granule (used only where the frame arrived)
            bitsv = a.bits[c.fr];
            recv4 = *reinterpret_cast<const f32x4 *>(a.codes_in + c.fr * (ntiles * 16) + n0);
        }
        if (EPI == FE_MEL) {
            mean4 = *reinterpret_cast<const f32x4 *>(a.mean + n0);
            std4 = *reinterpret_cast<const f32x4 *>(a.stdv + n0);
        }
    }
    f32x4 acc = acc0;
    // EARLY: the next layer's weights are requested inside the (last) segment, right behind its operand requests
    constexpr bool EARLY = BVC_FLOW_EARLYW && PRE_OUT && PER > 1;
    constexpr bool FEARLY = false;
    SegHook hk = no_hook();
    if (BVC_FLOW_DIAG) { hk.st_flags = flow_stamp_slot(c, hopid, 2); hk.st_done = flow_stamp_slot(c, hopid, 3); }
    // the layer behind which the first quantum of a product is requested is the one that fetches that product's input
    if (FGATE == 0) hk.stash = c.stash;
    if (PER == 1) {                                        // a narrow input (<= 8 k-blocks): one block per wave and pass
        for (int off = 0; off < nb; off += NW)
            lin_segment<PER, PERN>(g, l0.w, l0.wnb, nb, (unsigned)(src0 * 2 + c.par) * c.sb, false, wv, acc, c.give_up, code, off, hk, wn);
        if (TWO)                                           // (h_dim <= 128 without filler quanta: dec.0 of encode has both halves here)
            for (int off = 0; off < nb; off += NW)
                lin_segment<PER, PERN>(g, l1.w, l1.wnb, nb, (unsigned)(src1 * 2 + c.par) * c.sb, false, wv, acc, c.give_up, code, off, hk, wn);
    } else {
        SegHook hl = hk;
        if (EARLY) { hl.nw = nxt.w; hl.nwnb = nxt.wnb; hl.pre = c.pre_now; }
        if (TWO) {
            lin_segment<PER>(g, l0.w, l0.wnb, nb, (unsigned)(src0 * 2 + c.par) * c.sb, PRE_IN, wv, acc, c.give_up, code);
            lin_segment<PER, PERN, FEARLY>(g, l1.w, l1.wnb, nb, (unsigned)(src1 * 2 + c.par) * c.sb, false, wv, acc, c.give_up, code, 0, hl, wn);
        } else {
            lin_segment<PER, PERN, FEARLY>(g, l0.w, l0.wnb, nb, (unsigned)(src0 * 2 + c.par) * c.sb, PRE_IN, wv, acc, c.give_up, code, 0, hl, wn);
        }
    }
    if (PRE_OUT && !EARLY && c.pre_now) {         // the next layer's weights travel during the reduction and the wait
        const GPtr ub = uniform_ptr(nxt.w, ((size_t)g.ntile * nxt.wnb + wave * PERN) * g.wmul);
#pragma unroll
        for (int u = 0; u < PERN; ++u) wn[u] = wload(ub, (unsigned)lane * 16u, u);
    }
    // The quantum's operands are requested in front of the barrier and multiplied behind it.  (Round 2 measured the other orders with
    // the quantum's input re-fetched from memory: the publishing wave requesting its own behind its store, or every wave behind the
    // store: 56.8 / 59.1 against 56.4 ms per step - the quantum's own fetch is then exposed behind the layer.)
    if (FGATE != -2) fill_issue<PERN, FGATE>(g, fill, fw, fx);
    float *r = c.red_lin + (c.hopctr & 1u) * (NW * 256);
    ++c.hopctr;
    *reinterpret_cast<f32x4 *>(r + (wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 4);
    if (wave == 0) {
        if constexpr (EPI == FE_CODE_SEL) flow_publish<EPI, ADD, REARM_H, NW>(c, hopid, r, n0, ytile, ntiles, out, bias4, add4, mean4, std4, bitsv, recv4);
        else flow_publish<EPI, ADD, REARM_H, NW>(c, hopid, r, n0, ytile, ntiles, out, bias4, add4, mean4, std4, bitsv);
        if (BVC_FLOW_PARTNER_WAIT && NW == 8 && FGATE != -2) *c.pubflag = c.hopctr;
    } else if (BVC_FLOW_PARTNER_WAIT && NW == 8 && wave == 4 && FGATE != -2) {
        // waves 0 and 4 share a SIMD: this wave's MFMAs would take issue slots from the epilogue everybody is waiting for
        // (stamps: barrier -> published 0.87 us with the partner multiplying, 0.46 with it waiting, 0.42 in layers without a quantum)
        for (int i = 0; i < 4096 && *c.pubflag != c.hopctr; ++i) __builtin_amdgcn_s_sleep(2);
    }
    if (FGATE != -2) fill_multiply<PERN, FGATE>(g, fill, fw, *facc, c.stash);
    if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 5);
}

// MULTI: one single-segment layer for ALL chains of this workgroup.  The chains' products are software-pipelined (while chain ci is
// multiplied, the operand blocks of chain ci+1 are on their way - fetched without a flag poll: their producers published them while
// this workgroup was busy with other chains - and verified like every fetch; a block that still holds the sentinel sends the wave
// through the ordinary wait-and-fetch path) and reduced in GROUPS of up to four chains: four accumulators per wave, ONE reduction
// barrier per group, then wave k of the group's four publishing waves (0-3 for even groups, 4-7 for odd ones) runs chain k's
// epilogue while everybody else goes on.  (One barrier and one single-wave epilogue per CHAIN - round 2 - made wave 0 the pole of
// every chain: its own products, then the epilogue, with seven waves waiting at the next chain's barrier.)  The partial tiles of a
// group lie in LDS slot (group & 1): the next writers of a slot are two groups away, and a group's partials are only written
// after ALL its products, whose operands - the previous layer's outputs of those chains from every workgroup, this one included -
// exist only once the publishing waves have read what they publish.  Same arithmetic, same order per output as flow_layer.
// TWO: y = epi(W0 x0 + W1 x1 + bias) - the group's chains are first multiplied with segment 0 (its weights are fetched here, into
// registers of their own), then with segment 1 (wv), into the same accumulators: per output the order of flow_layer's two segments.
template <int PER, int EPI, bool ADD, bool PRE_IN, bool PRE_OUT, int PERN, bool REARM_H, int NW, bool TWO = false>
__device__ __forceinline__ void flow_layer_chains(FlowCtx &c, int hopid, const FlowLin l0, int src0, int nb, int ntiles, int out,
                                                  f32x4 (&wv)[PER], const FlowLin nxt, f32x4 (&wn)[PERN], int mt0, int nch, long long T,
                                                  const FlowLin lfirst = FlowLin{nullptr, nullptr, 0, 0}, int srcfirst = 0) {
    static_assert(PER > 1, "narrow inputs take the per-chain path");
    static_assert(NW == 8, "two sets of four publishing waves");
    constexpr int GM = 4;                                  // at most four chains per reduction group ...
    const int G = nch >= 3 ? BVC_CHAIN_G : 1;              // ... and one with two chains per workgroup (measured: 128 x 5 s 6,390 audio-s/s with
                                                           // one chain per barrier against 6,250 with both behind one; 256 x 5 s 6,790 / 6,960)
    FlowWg &g = c.g;
    const auto &a = *c.a;
    if (g.ntile >= ntiles) {
        if (PRE_OUT) {
            wzero(wn);
        }
        return;
    }
    int lane = g.lane;
    const int wave = g.wave;
    asm volatile("" : "+v"(lane));                         // (see flow_layer)
    const unsigned code = (unsigned)((c.t << 4) | (unsigned)hopid) | 0x80000000u;
    const int n0 = g.ntile * 16 + (lane >> 4) * 4;
    const int kb0 = wave * PER;
    const unsigned bufb = (unsigned)(src0 * 2 + c.par) * c.sb;
    if (!PRE_IN) {
        const GPtr ub = uniform_ptr(l0.w, ((size_t)g.ntile * l0.wnb + kb0) * g.wmul);
#pragma unroll
        for (int u = 0; u < PER; ++u) wv[u] = wload(ub, (unsigned)lane * 16u, u);
    }
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, mean4 = {0.f, 0.f, 0.f, 0.f}, std4 = {1.f, 1.f, 1.f, 1.f};
    if (l0.bias) bias4 = *reinterpret_cast<const f32x4 *>(l0.bias + n0);         // (every wave may publish a chain)
    if (EPI == FE_MEL) {
        mean4 = *reinterpret_cast<const f32x4 *>(a.mean + n0);
        std4 = *reinterpret_cast<const f32x4 *>(a.stdv + n0);
    }
    unsigned spins = 0;
    flow_stamp(c, hopid, 0);
    f32x4 wfirst[TWO ? PER : 1];
    if (TWO) {
        const GPtr ub = uniform_ptr(lfirst.w, ((size_t)g.ntile * lfirst.wnb + kb0) * g.wmul);
#pragma unroll
        for (int u = 0; u < PER; ++u) wfirst[u] = wload(ub, (unsigned)lane * 16u, u);
    }
    u32x4 xc[PER], xn[PER];
    for (int g0 = 0, grp = 0; g0 < nch; g0 += G, ++grp) {
        const int gn = nch - g0 < G ? nch - g0 : G;
        f32x4 accs[GM];
#pragma unroll
        for (int k = 0; k < GM; ++k) accs[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int pass = TWO ? 0 : 1; pass < 2; ++pass) {
        const unsigned bufp = (TWO && pass == 0) ? (unsigned)(srcfirst * 2 + c.par) * c.sb : bufb;
        const f32x4 (&wp)[TWO ? PER : 1] = wfirst;         // (pass 0 only)
        // the first chain of this pass (of this group): wait for its producers, request its blocks
        if (TWO || g0 == 0) {
            g.mtile = mt0 + g0;
            const FlowSrc s0 = flow_wait<PER>(g, bufp, nb, kb0, c.give_up, code, spins);
            flow_issue<PER>(g, s0, xc);
        }
#pragma unroll
        for (int k = 0; k < GM; ++k) {
            if (k < gn) {                                  // (uniform)
                const int ci = g0 + k;
                g.mtile = mt0 + ci;
                if (TWO ? k + 1 < gn : ci + 1 < nch) {     // the next chain's blocks: requested before this chain's are waited for
                    FlowSrc sn;                            // (TWO: within the group's pass; else on across the groups)
                    sn.base = __builtin_amdgcn_readfirstlane(bufp + (unsigned)((g.mtile + 1) * nb + kb0) * 1024u);
                    sn.vl = (unsigned)lane * 16u;
                    flow_issue<PER>(g, sn, xn);
                } else {
#pragma unroll
                    for (int u = 0; u < PER; ++u) xn[u] = (u32x4){0u, 0u, 0u, 0u};
                }
                bool bad = false;
#pragma unroll
                for (int u = 0; u < PER; ++u) bad |= is_poison4(xc[u]);
                while (__any(bad) && !c.give_up) {         // (rare) not published yet, or a flag ahead of its block: wait, fetch again
                    const FlowSrc sr = flow_wait<PER>(g, bufp, nb, kb0, c.give_up, code, spins);
                    flow_issue<PER>(g, sr, xc);
                    bad = false;
#pragma unroll
                    for (int u = 0; u < PER; ++u) bad |= is_poison4(xc[u]);
                    flow_spin(g, lane, spins, c.give_up, code);
                }
                if (BVC_FLOW_DIAG && k == 0 && g0 == 0 && pass == 1) flow_stamp(c, hopid, 2);     // first chain's operands here
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const f32x4 xv = __builtin_bit_cast(f32x4, xc[u]);
                    const f32x4 wu = (TWO && pass == 0) ? wp[TWO ? u : 0] : wv[u];
#pragma unroll
                    for (int e = 0; e < 4; ++e) accs[k] = mfma16(wu[e], xv[e], accs[k]);
                }
#pragma unroll
                for (int u = 0; u < PER; ++u) xc[u] = xn[u];
            }
        }
      }
        if (BVC_FLOW_DIAG && g0 == 0) flow_stamp(c, hopid, 3);
        if (PRE_OUT && g0 + G >= nch) {                    // the next layer's weights travel during the last group's reduction
            const GPtr ub = uniform_ptr(nxt.w, ((size_t)g.ntile * nxt.wnb + wave * PERN) * g.wmul);
#pragma unroll
            for (int u = 0; u < PERN; ++u) wn[u] = wload(ub, (unsigned)lane * 16u, u);
        }
        // this wave's chain to publish (if any) and its epilogue operands, requested in front of the barrier
        const int pk = wave - (grp & 1) * GM;              // publishing waves of this group: (grp & 1) * 4 + k
        const bool pub = pk >= 0 && pk < gn;
        FlowCtx ce = c;
        flow_set_chain(ce, mt0 + g0 + (pub ? pk : 0), lane, a.B, T, c.t);
        ce.probe = c.probe && pk == 0 && g0 == 0;
        f32x4 add4 = {0.f, 0.f, 0.f, 0.f};
        float bitsv = 0.0f;
        f32x4 recv4 = {0.f, 0.f, 0.f, 0.f};
        if (pub) {
            if (ADD && ce.rowok) add4 = *reinterpret_cast<const f32x4 *>(a.part0 + ce.fr * (ntiles * 16) + n0);
            if (EPI == FE_CODE && a.var_bit && ce.rowok) bitsv = a.bits[ce.fr];
            if (EPI == FE_CODE_SEL && ce.rowok) {
                bitsv = a.bits[ce.fr];
                recv4 = *reinterpret_cast<const f32x4 *>(a.codes_in + ce.fr * (ntiles * 16) + n0);
            }
        }
        float *rg = c.red_chain + (grp & 1) * (GM * NW * 256);
#pragma unroll
        for (int k = 0; k < GM; ++k)
            if (k < gn) *reinterpret_cast<f32x4 *>(rg + ((k * NW + wave) * 64 + lane) * 4) = accs[k];
        __syncthreads();
        if (BVC_FLOW_DIAG && g0 == 0) flow_stamp(c, hopid, 4);
        if (pub) {
            const unsigned ytile = (unsigned)((ce.g.mtile * ntiles + g.ntile) * 1024 + lane * 16);
            if constexpr (EPI == FE_CODE_SEL) flow_publish<EPI, ADD, REARM_H, NW>(ce, hopid, rg + pk * (NW * 256), n0, ytile, ntiles, out, bias4, add4, mean4, std4, bitsv, recv4);
            else flow_publish<EPI, ADD, REARM_H, NW>(ce, hopid, rg + pk * (NW * 256), n0, ytile, ntiles, out, bias4, add4, mean4, std4, bitsv);
        }
    }
    if (BVC_FLOW_DIAG) flow_stamp(c, hopid, 5);
}

}  // namespace
}  // namespace bvc
