// Persistent BVRNN recurrence for gfx950: ALL frames of BVRNN.encode / BVRNN.decode (bvrnn.py:186-206,
// 222-227) in ONE kernel launch.  This file: the compile-time tunables with what was measured and dropped, the kernel (the layer
// program), the table of its instantiations and the launch.  The device code it is made of: k_flow_handoff.h (the "poisoned
// buffer" hand-off between workgroups, the weight loads), k_flow_layers.h (a layer's products, filler quanta, epilogue and
// publication), k_flow_gru.h (the GRU cell).  The support kernels (census, fill, prepare, arguments) are k_flow_support.hip.
//
// One workgroup (8 waves) owns one 16x16 output tile (16 utterances x 16 features) of EVERY layer of the
// step, for all frames; the 64 feature tiles of an utterance group form a chain of all-to-all hand-offs
// (a layer needs the whole output of the previous one), the utterance groups are independent chains.
// K is split over the 8 waves, partial tiles are summed in fixed order through LDS, wave 0 applies the
// layer's epilogue (bias, ELU, sigmoid/round/bit-mask, mel normalisation, GRU cell).  The MFMA computes
// Y^T = W X^T (A = weight fragment, B = activation fragment) so that a lane's four results are four
// consecutive features of one utterance: exactly the 16-byte granule of the next layer's operand block.
// The next layer's first weight blocks are requested before the wait, so they travel meanwhile.  The layer sequence
// is a compile-time program (bvrnn_flow_kernel<PERH, ENCODE>), its operands come from a device-resident FlowArgs.
//
// What sits in a compute unit for the whole launch (filler form, h_dim 1024): the weights of two wide layers (decode: three) in registers -
// the kernel needs 165 of the 256 VGPRs a wave may have - and the first layer's in the 64 KiB of LDS the kernel had left; the vector
// instructions on a hop's critical path are few on purpose (fp32 MFMAs and vector instructions share the ALUs, also within one wave:
// profiles/r04_mfma_valu_overlap.txt), and scheduling fences keep loads and checks where the source puts them (hipcc sinks loads to their
// first use and hoists checks in front of the products when left alone: profiles/r04_flow_variants.txt).

// Compile-time tunables (tools/flow_variants.py builds and times variants; the values here are what ships):
#ifndef BVC_FLOW_DIAG
#define BVC_FLOW_DIAG 0            // 1: the probing lane also stamps flags-seen / products-done / barrier-passed (include/bvcodec.h; flow_variants.py run --diag)
#endif
#ifndef BVC_FLOW_WAVES_PER_SIMD
#define BVC_FLOW_WAVES_PER_SIMD 2  // launch bound of the 8-wave kernels, i.e. their register budget (build.py: BVC_FLOW_WAVES)
#endif
#ifndef BVC_FLOW_POLL_SLEEP
#define BVC_FLOW_POLL_SLEEP 1      // s_sleep units (64 clocks) between two polls of a wave (0 / 4 / 12 measured: +-0.1 ms, the waits end within one or two polls)
#endif
#ifndef BVC_FLOW_PARTNER_WAIT
#define BVC_FLOW_PARTNER_WAIT 1    // the wave that shares wave 0's SIMD (wave 4) starts its quantum's products only once wave 0 has issued the
#endif                             // publishing store (its MFMAs take issue slots from the epilogue everybody waits for)
#ifndef BVC_FLOW_PARKV
#define BVC_FLOW_PARKV 2           // (filler form; 0 off, 1 two layers) the weights of dec.2 and dec.4, in decode also phi_x.4 - this wave's 8 blocks each - stay
#endif                             // in registers for the whole launch (165 of 256 VGPRs): 128 KiB (decode 192) per compute unit and frame less to pull from
                                   // the L2, whose fill path into the compute units is what the kernel is bound by
#ifndef BVC_FLOW_PARKL
#define BVC_FLOW_PARKL 1           // (filler form) the FIRST layer's weights (enc.0 / dec.0, the half that multiplies h) stay in LDS for the whole launch - the
#endif                             // 64 KiB that the kernel's 128 KiB left of a compute unit's 160 - instead of being requested by every frame's GRU
                                   // layer, at the most crowded point of the frame
#ifndef BVC_GRU_ROUNDS_FILL
#define BVC_GRU_ROUNDS_FILL 4      // rounds in which the GRU layer's remaining weights (phi_x third) pass through the registers
#endif
#ifndef BVC_GRU_DEPTH
#define BVC_GRU_DEPTH 3            // register sets that stream runs through (2: the request for round i + 1 in front of round i's products; up to all four rounds)
#endif
#ifndef BVC_GRU_FENCE
#define BVC_GRU_FENCE 1            // scheduling fences around the rounds of the GRU layer's weight stream (see flow_gru)
#endif
#ifndef BVC_CHAIN_G
#define BVC_CHAIN_G 4              // chains per reduction group of flow_layer_chains (three and more chains per workgroup)
#endif
#ifndef BVC_FLOW_EARLYW
#define BVC_FLOW_EARLYW 0          // 1: the next layer's weights are requested right behind this layer's operand requests instead of in front of the
#endif                             // reduction barrier.  A measured loser (54.3 against 52.8 ms per step, profiles/r03_flow_variants.txt: v5 / v5_noew) that
                                   // is still here because hipcc orders a few instructions of the two narrowest concealing kernels differently without its dead
                                   // arm (bvrnn_flow_kernel<1, true, false | true, 8, false, -1, true>: profiles/flow_fold.md)
// What the request order is about: a compute unit takes vector-memory requests in order, 64 B per clock (1 KiB per wave-instruction = 16
// clocks), and a wave that issues a request into a full queue stalls.  Everything requested in front of the reduction barrier
// therefore holds the barrier - and the publishing store behind it - back: 24 KiB per wave there (next weights, quantum weights,
// quantum operands) cost every filler layer more than a microsecond (stamps: products -> barrier 1.2-1.8 us, 0.2-0.5 without).
//
// Measured and dropped - no longer compiled; last built at 2defbdd (DESIGN.md section 4 names the switch each form was built under there).
// ms are per step (64 x 5 s); r03 / r04 = profiles/r03_flow_variants.txt / profiles/r04_flow_variants.txt.
//   next layer's weights requested behind the reduction barrier instead of in front of it: 53.1 against 52.8 (r03: v6_latew)
//   a quantum's weights requested inside the layer's segment too: 56.5 against 54.3 (r03: v5_fe)
//   a quantum's operand blocks re-fetched from memory instead of kept in this wave's LDS stash: the stash took 20 % off the
//       L2 -> CU traffic, 54.2 against 55.1 (r03: stash0e / earlyw)
//   GRU layer's phi_x weights half requested a layer early, a quarter parked in LDS, a quarter streamed (h_dim 1024, filler form,
//       in place of BVC_FLOW_PARKL - one use of the parking region): 52.76 either way (r03: v6), +0.4 against the fenced stream (r04: gfast) - with its
//       h and phi_z parts taken out by the quanta the layer is bound by the 192 MFMAs its two waves per SIMD issue, not by the weight stream
//   operand blocks requested without polling their flags first, requested again while one holds the sentinel: 47.9-48.0
//       against 45.9 (r04: spec); the same for the first chain of flow_layer_chains: groups of four chains lose 2 % (r04: g4s)
//   sentinel checks wherever hipcc schedules them - in front of the first product, block 0 requested second to last - instead of fenced
//       behind the last product: 48.6 against 48.2 (r04: maxchk / inord)
//   sentinel check as four compares and three ors per 16 bytes instead of an unsigned maximum: 49.9 against 48.5 (r04: base / maxchk)
//   phi_x.2 + phi_x.4 as the register-resident layers instead of dec.2 + dec.4: 46.9 against 46.55 (r04: s0v2 / s1v2)
//   two or three flag polls in flight per wave (retired earlier): 57.9 / 59.2 against 55.7 - the polls themselves load the hand-off path (r03: poll2 / poll3)
//   quanta requested behind the publishing store and multiplied a layer later, with and without a pre-issued poll of the next layer's flags:
//       shorter layer spans, 43.8 against 45.2 us per encode frame, but wave 0 leaves each layer later: 55.0-55.9 against 54.1 (r03: pipe*)
//   the ELU epilogue split over four waves (wave j reduces and activates output j of every lane, wave 0 gathers through LDS and publishes):
//       barrier -> published stays at 0.45 us, 53.8 against 52.8 (r03: v7_split) - unlike the GRU cell's, which did shrink from 1.5 to 0.8 us
//       that way, the linear layers' epilogue is not bound by its instruction count
//   resident rounds of the GRU stream, other request orders, fences in the chain kernels: r04

#include "k_flow_gru.h"         // (and through it k_flow_layers.h, k_flow_handoff.h, k_gemm.h): they read the tunables above

namespace bvc {
namespace {

template <bool C, typename A, typename B>
__device__ __forceinline__ decltype(auto) pick(A &a, B &b) {
    if constexpr (C) return (a);
    else return (b);
}

template <typename P>
__device__ __forceinline__ FlowLin L(const P &l) {        // member-wise copy out of the constant address space
    FlowLin r;
    r.w = l.w; r.bias = l.bias; r.wnb = l.wnb; r.pad_ = 0;
    return r;
}

}  // namespace

// PERH: k-blocks per wave of an h_dim-sized operand (h_dim = 128 * PERH, or h_dim <= 128 for PERH = 1: then a wave owns at
// most one k-block); the z_dim- and num_mels-sized operands (<= 128) always have one k-block per wave.
// A layer of ONE segment of the static program (all but encode's unfilled dec.0): flow_layer with the layer and no second segment, the
// next weights PERH blocks per wave.  (A macro, i.e. the call written out: the same layers through a function template over
// flow_layer compile to other instructions in three kernels, profiles/flow_fold.md.)
#define FLOW_LAYER1(PER, EPI, ADD, PRE_IN, PRE_OUT, REARM_H, FGATE, hop, l, src, ...) \
    flow_layer<PER, EPI, false, ADD, PRE_IN, PRE_OUT, PERH, REARM_H, FGATE, NW>(c, hop, l, src, l, 0, __VA_ARGS__)
// MULTI: one layer of the static program, chain by chain.  (Also a macro: as a function template over a callable it changes the
// decode chain kernel without the fold and the four encode-side chain kernels: a VGPR or an SGPR spill more.)
#define FLOW_EACH_CHAIN(...)                                                                                         \
    for (int ci_ = 0; ci_ < nch; ++ci_) {                                                                               \
        flow_set_chain(c, mt0 + ci_, c.g.lane, a.B, T, t);                                                              \
        c.pre_now = ci_ == nch - 1;                                                                                     \
        __VA_ARGS__;                                                                                                    \
    }

// MULTI: a workgroup owns its feature tile for MG utterance groups ("chains": utterances never interact) and works through a
// layer chain by chain with the same weight registers; by the time it returns to a chain for the next layer, that chain's
// inputs - produced by the other workgroups in the same order - have long arrived, so the hand-off latency of one chain lies
// under the products of the others.  Batches of more than 16 * (CUs / feature tiles) utterances (64 at h_dim 1024) run this way.
// FOLD: 1 / 0: the folded hop (FlowArgs::pxc) is / is not compiled in; -1: both, chosen at run time.  (The interleaved-chain
// kernels with both programs in them spill: they are instantiated once per program.)
// CONCEAL: the third program, the concealing decoder (bvc_bvrnn_decode_conceal): the ENCODE program with the prior net in the encoder's
// place - FlowArgs::enc0h / enc1 / enc2 then hold prior.{0,2,4}, the first layer has its own bias and no pre-computed half - and the code
// epilogue selecting between the received codes and the generated bits (FE_CODE_SEL).  Everything behind layer 3 is the encode program.
template <int PERH, bool ENCODE, bool FILL, int NW = 8, bool MULTI = false, int FOLD = -1, bool CONCEAL = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? BVC_FLOW_WAVES_PER_SIMD : 1) void bvrnn_flow_kernel(const FlowArgs *a0) {
    static_assert(!(MULTI && FILL), "the filler quanta are per chain: not built for interleaved chains");
    static_assert(!CONCEAL || ENCODE, "the concealing decoder is a variant of the encode program");
    constexpr int EPI3 = CONCEAL ? FE_CODE_SEL : FE_CODE;      // layer 3's epilogue
    extern __shared__ __attribute__((aligned(16))) float lds[];     // laid out by FlowLds (bvc_internal.h)
    typedef FlowLds<NW> Lds;
    const int tid = threadIdx.x;
    FlowCtx c;
    FlowArgsC ap = (FlowArgsC)(unsigned long long)a0;      // device-resident copy of the arguments (flow_set_args_kernel)
    c.a = ap;
    c.red_lin = lds + Lds::partials;
    c.red_gru = lds + Lds::gru;
    c.red_chain = lds + Lds::chain;                        // (MULTI only)
    c.stash = (LdsX)(lds + Lds::stash) + (tid >> 6) * (PERH * 64);
    c.lpark = (LdsX)(lds + Lds::park) + (tid >> 6) * (8 * 64);
    c.pubflag = (volatile unsigned __attribute__((address_space(3))) *)(lds + Lds::flag);
    if (FILL && tid == 0) c.pubflag[0] = 0xFFFFFFFFu;
    c.g.lane = tid & 63;
    c.g.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int MT = ap->MT;
    const int MG = MULTI ? ap->MG : 1;                     // chains per workgroup
    const int MTG = MULTI ? (MT + MG - 1) / MG : MT;       // workgroups per feature tile
    c.g.ntile = (slot / MTG) * 8 + xcd;                   // the utterance groups of a feature tile share an XCD (weights cross the fabric once)
    const int mt0 = (slot % MTG) * MG;
    const int nch = MULTI ? (MT - mt0 < MG ? MT - mt0 : MG) : 1;
    c.g.mtile = mt0;
    if (ap->dbg_withhold && bid == 0) return;              // tests: a workgroup that never publishes (its consumers time out)
    if (c.g.ntile >= ap->NTG) return;                      // grid is rounded up to a multiple of 8 feature tiles
    c.g.rs = __builtin_amdgcn_make_buffer_rsrc(ap->flow, 0, (int)(FB_COUNT * 2u * ap->slot_bytes), 0x00020000);
    c.sb = ap->slot_bytes;
    c.g.spin_limit = ap->spin_limit;
    c.g.wmul = ap->dbg_hot_w ? 0 : 1;
    c.g.status = ap->status;
    c.row = c.g.mtile * 16 + (c.g.lane & 15);
    c.rowok = c.row < ap->B;
    c.give_up = false;
    c.pre_now = true;
    c.probe = ap->probe != nullptr && bid == ap->probe_wg && tid == ap->probe_wave * 64;
    c.hopctr = 0;
    const int hb = ap->hb, zb = ap->zb, xb = ap->xb;
    const long long T = ap->T;
    const bool hfull = c.g.ntile < hb;                     // this workgroup owns a tile of the h_dim-wide layers
    f32x4 wa[PERH], wb[PERH], w1[1];
    // BVC_FLOW_PARKV: wide layers whose weights - this wave's eight blocks each - stay in registers for the whole launch.  Layers that
    // carry a filler quantum first (their waves request two weight sets in front of the reduction barrier otherwise): dec.2, dec.4; decode has
    // registers for a third: phi_x.4
    constexpr bool PK = BVC_FLOW_PARKV && FILL && !MULTI;
    constexpr bool PL = BVC_FLOW_PARKL && FILL && !MULTI && PERH == 8;
    constexpr bool P8 = PK, P9 = PK, P13 = PK && !ENCODE && BVC_FLOW_PARKV >= 2;
    f32x4 k8[P8 ? PERH : 1], k9[P9 ? PERH : 1], k13[P13 ? PERH : 1];
    {
        auto park = [&](auto &k, const FlowLin l) {
            const GPtr u = uniform_ptr(l.w, hfull ? (size_t)c.g.ntile * l.wnb + c.g.wave * PERH : 0);
#pragma unroll
            for (int i = 0; i < PERH; ++i) k[i] = wload(u, (unsigned)c.g.lane * 16u, i);
        };
        if constexpr (P8) park(k8, L(ap->dec1));
        if constexpr (P9) park(k9, L(ap->dec2));
        if constexpr (P13) park(k13, L(ap->px2));
    }
    {
        const FlowLin first = ENCODE ? L(ap->enc0h) : L(ap->dec0h);
        const GPtr ub = uniform_ptr(first.w, hfull ? (size_t)c.g.ntile * first.wnb + c.g.wave * PERH : 0);
#pragma unroll
        for (int u = 0; u < PERH; ++u) wa[u] = wload(ub, (unsigned)c.g.lane * 16u, u);
        if constexpr (PL) {
#pragma unroll
            for (int u = 0; u < PERH; ++u) c.lpark[u * 64 + c.g.lane] = __builtin_bit_cast(u32x4, wa[u]);      // (read back by this very wave only)
        }
    }
    for (long long t = 0; t < T; ++t) {
        if constexpr (PL) {                                // the first layer's weights come out of LDS (requested by nobody)
#pragma unroll
            for (int u = 0; u < PERH; ++u) wa[u] = __builtin_bit_cast(f32x4, c.lpark[u * 64 + c.g.lane]);
        }
        asm volatile("" : "+s"(ap));                       // see FlowArgsC
        c.a = ap;
        const auto &a = *ap;
        c.t = t;
        c.par = (unsigned)(t & 1);
        c.fr = (long long)c.row * T + t;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        if (FILL) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { c.fgh[q] = zero4; c.fgi[q] = zero4; }
            c.fd0 = zero4;
        }
        const unsigned hsrc = (unsigned)(FB_H * 2 + c.par) * c.sb, zsrc = (unsigned)(FB_Q3 * 2 + c.par) * c.sb;
        // FILL: behind a layer, while its successors' inputs are still being produced, a wave multiplies one "quantum" of a product
        // whose input has been complete since the start of the frame (h) or since phi_z (encode): the three gates of W_hh h, the
        // h half of dec.0, the three gates of W_ih[:, H:] phi_z.  The GRU layer then only has phi_x(d_t)'s third left.
        constexpr int G0 = FILL ? 0 : -2, G1 = FILL ? 1 : -2, G2 = FILL ? 2 : -2, GP = FILL ? -1 : -2;
        const FlowFill f_hh = {a.w_hh, hb, hb, hsrc}, f_d0 = {a.dec0h.w, a.dec0h.wnb, hb, hsrc}, f_iz = {a.w_ihz, 2 * hb, hb, zsrc};
        const bool folded = FOLD < 0 ? a.pxc.w != nullptr : FOLD == 1;      // (uniform) dec.6 -> norm -> phi_x.0 folded into one layer (FlowArgs::pxc)
        if constexpr (!MULTI) {
            // (wK: the weights of wide layer K - prefetched into wa / wb by the layer in front of it, or resident in registers: P8, P9, P13)
            auto &w8 = pick<P8>(k8, wb);  auto &w9 = pick<P9>(k9, wa);  auto &w13 = pick<P13>(k13, wb);
            if (ENCODE) {
                //          PER   epilogue add    pre_in pre_out rearm filler  hop  layer  input
                FLOW_LAYER1(PERH, FE_ELU, !CONCEAL, true, true, false, G0, 1, L(a.enc0h), FB_H, hb, hb, FB_E1, wa, L(a.enc1), wb, zero4, f_hh, &c.fgh[0]);
                FLOW_LAYER1(PERH, FE_ELU, false, true, false, true, G1, 2, L(a.enc1), FB_E1, hb, hb, FB_E2, wb, L(a.enc1), wa, zero4, f_hh, &c.fgh[1]);
                FLOW_LAYER1(PERH, EPI3, false, false, false, false, G2, 3, L(a.enc2), FB_E2, hb, zb, FB_ZC, wa, L(a.enc2), wb, zero4, f_hh, &c.fgh[2]);
                FLOW_LAYER1(1, FE_ELU, false, false, true, false, GP, 4, L(a.pz0), FB_ZC, zb, hb, FB_Q1, w1, L(a.pz1), wa, zero4, f_d0, &c.fd0);
                FLOW_LAYER1(PERH, FE_ELU, false, true, true, false, -2, 5, L(a.pz1), FB_Q1, hb, hb, FB_Q2, wa, L(a.pz2), wb);
                if (FILL) {
                    FlowLin d0 = L(a.dec0z);                   // dec.0: only the phi_z half is left; the bias travels with dec0h
                    d0.bias = a.dec0h.bias;
                    FLOW_LAYER1(PERH, FE_ELU, false, true, true, false, -2, 6, L(a.pz2), FB_Q2, hb, hb, FB_Q3, wb, d0, wa);
                    FLOW_LAYER1(PERH, FE_ELU, false, true, !P8, false, G0, 7, d0, FB_Q3, hb, hb, FB_D1, wa, L(a.dec1), wb, c.fd0, f_iz, &c.fgi[0]);
                } else {
                    FLOW_LAYER1(PERH, FE_ELU, false, true, true, false, -2, 6, L(a.pz2), FB_Q2, hb, hb, FB_Q3, wb, L(a.dec0h), wa);
                    flow_layer<PERH, FE_ELU, true, false, true, true, PERH, false, -2, NW>(c, 7, L(a.dec0h), FB_H, L(a.dec0z), FB_Q3, hb, hb, FB_D1, wa, L(a.dec1), wb);
                }
                FLOW_LAYER1(PERH, FE_ELU, false, true, !P9, false, G1, 8, L(a.dec1), FB_D1, hb, hb, FB_D2, w8, L(a.dec2), wa, zero4, f_iz, &c.fgi[1]);
                if (folded) {
                    FLOW_LAYER1(PERH, FE_ELU_KEEP, false, true, true, false, G2, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, w9, L(a.pxc), wb, zero4, f_iz, &c.fgi[2]);
                    FLOW_LAYER1(PERH, FE_ELU, false, true, true, false, -2, 11, L(a.pxc), FB_D3, hb, hb, FB_G1, wb, L(a.px1), wa);
                } else {
                    FLOW_LAYER1(PERH, FE_ELU, false, true, false, false, G2, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, w9, L(a.dec2), wb, zero4, f_iz, &c.fgi[2]);
                    FLOW_LAYER1(PERH, FE_MEL, false, false, false, false, -2, 10, L(a.dec3), FB_D3, hb, xb, FB_DN, wa, L(a.dec3), wb);
                }
            } else {
                FLOW_LAYER1(PERH, FE_ELU, true, true, !P8, false, G0, 7, L(a.dec0h), FB_H, hb, hb, FB_D1, wa, L(a.dec1), wb, zero4, f_hh, &c.fgh[0]);
                FLOW_LAYER1(PERH, FE_ELU, false, true, !P9, true, G1, 8, L(a.dec1), FB_D1, hb, hb, FB_D2, w8, L(a.dec2), wa, zero4, f_hh, &c.fgh[1]);
                if (folded) {                              // dec.4 (its output is kept for all frames) -> phi_x.0 o norm o dec.6 as one wide layer
                    FLOW_LAYER1(PERH, FE_ELU_KEEP, false, true, true, false, G2, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, w9, L(a.pxc), wb, zero4, f_hh, &c.fgh[2]);
                    FLOW_LAYER1(PERH, FE_ELU, false, true, true, false, -2, 11, L(a.pxc), FB_D3, hb, hb, FB_G1, wb, L(a.px1), wa);
                } else {
                    FLOW_LAYER1(PERH, FE_ELU, false, true, false, false, G2, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, w9, L(a.dec2), wb, zero4, f_hh, &c.fgh[2]);
                    FLOW_LAYER1(PERH, FE_MEL, false, false, false, false, -2, 10, L(a.dec3), FB_D3, hb, xb, FB_DN, wa, L(a.dec3), wb);
                }
            }
            if (!folded)
                FLOW_LAYER1(1, FE_ELU, false, false, true, false, -2, 11, L(a.px0), FB_DN, xb, hb, FB_G1, w1, L(a.px1), wa);
            FLOW_LAYER1(PERH, FE_ELU, false, true, !P13, false, -2, 12, L(a.px1), FB_G1, hb, hb, FB_G2, wa, L(a.px2), wb);
            FLOW_LAYER1(PERH, FE_ELU, false, true, false, false, -2, 13, L(a.px2), FB_G2, hb, hb, FB_G3, w13, L(a.px2), wa);
            flow_gru<PERH, ENCODE, PERH, FILL, NW>(c, 14, hb, ENCODE ? L(a.enc0h) : L(a.dec0h), wa);
        } else {
            // the same program on interleaved chains (no filler quanta): wide single-segment layers pipeline their chains
            // (flow_layer_chains), the two narrow-input layers, the two-segment dec.0 of encode and the GRU go chain by chain
            constexpr bool E = ENCODE;
            if (E) {
                flow_layer_chains<PERH, FE_ELU, !CONCEAL, true, true, PERH, false, NW>(c, 1, L(a.enc0h), FB_H, hb, hb, FB_E1, wa, L(a.enc1), wb, mt0, nch, T);
                flow_layer_chains<PERH, FE_ELU, false, true, false, PERH, true, NW>(c, 2, L(a.enc1), FB_E1, hb, hb, FB_E2, wb, L(a.enc1), wa, mt0, nch, T);
                flow_layer_chains<PERH, EPI3, false, false, false, PERH, false, NW>(c, 3, L(a.enc2), FB_E2, hb, zb, FB_ZC, wa, L(a.enc2), wb, mt0, nch, T);
                FLOW_EACH_CHAIN(FLOW_LAYER1(1, FE_ELU, false, false, true, false, -2, 4, L(a.pz0), FB_ZC, zb, hb, FB_Q1, w1, L(a.pz1), wa));
                flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW>(c, 5, L(a.pz1), FB_Q1, hb, hb, FB_Q2, wa, L(a.pz2), wb, mt0, nch, T);
                flow_layer_chains<PERH, FE_ELU, false, true, false, PERH, false, NW>(c, 6, L(a.pz2), FB_Q2, hb, hb, FB_Q3, wb, L(a.pz2), wa, mt0, nch, T);
                // two segments share the weight registers: the first segment's weights are fetched per chain
                {                                          // dec.0 = dec0h . h + dec0z . phi_z: both segments for a group's chains, then one reduction
                    const GPtr ub = uniform_ptr(a.dec0z.w, ((size_t)c.g.ntile * a.dec0z.wnb + c.g.wave * PERH) * c.g.wmul);
#pragma unroll
                    for (int u = 0; u < PERH; ++u) wa[u] = wload(ub, (unsigned)c.g.lane * 16u, u);
                    FlowLin d0 = L(a.dec0z);
                    d0.bias = a.dec0h.bias;
                    flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW, true>(c, 7, d0, FB_Q3, hb, hb, FB_D1, wa, L(a.dec1), wb, mt0, nch, T, L(a.dec0h), FB_H);
                }
                flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW>(c, 8, L(a.dec1), FB_D1, hb, hb, FB_D2, wb, L(a.dec2), wa, mt0, nch, T);
                if (folded) {
                    flow_layer_chains<PERH, FE_ELU_KEEP, false, true, true, PERH, false, NW>(c, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, wa, L(a.pxc), wb, mt0, nch, T);
                    flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW>(c, 11, L(a.pxc), FB_D3, hb, hb, FB_G1, wb, L(a.px1), wa, mt0, nch, T);
                } else {
                    flow_layer_chains<PERH, FE_ELU, false, true, false, PERH, false, NW>(c, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, wa, L(a.dec2), wb, mt0, nch, T);
                }
            } else {
                flow_layer_chains<PERH, FE_ELU, true, true, true, PERH, false, NW>(c, 7, L(a.dec0h), FB_H, hb, hb, FB_D1, wa, L(a.dec1), wb, mt0, nch, T);
                flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, true, NW>(c, 8, L(a.dec1), FB_D1, hb, hb, FB_D2, wb, L(a.dec2), wa, mt0, nch, T);
                if (folded) {
                    flow_layer_chains<PERH, FE_ELU_KEEP, false, true, true, PERH, false, NW>(c, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, wa, L(a.pxc), wb, mt0, nch, T);
                    flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW>(c, 11, L(a.pxc), FB_D3, hb, hb, FB_G1, wb, L(a.px1), wa, mt0, nch, T);
                } else {
                    flow_layer_chains<PERH, FE_ELU, false, true, false, PERH, false, NW>(c, 9, L(a.dec2), FB_D2, hb, hb, FB_D3, wa, L(a.dec2), wb, mt0, nch, T);
                }
            }
            if (!folded) {
                flow_layer_chains<PERH, FE_MEL, false, false, false, PERH, false, NW>(c, 10, L(a.dec3), FB_D3, hb, xb, FB_DN, wa, L(a.dec3), wb, mt0, nch, T);
                FLOW_EACH_CHAIN(FLOW_LAYER1(1, FE_ELU, false, false, true, false, -2, 11, L(a.px0), FB_DN, xb, hb, FB_G1, w1, L(a.px1), wa));
            }
            flow_layer_chains<PERH, FE_ELU, false, true, true, PERH, false, NW>(c, 12, L(a.px1), FB_G1, hb, hb, FB_G2, wa, L(a.px2), wb, mt0, nch, T);
            flow_layer_chains<PERH, FE_ELU, false, true, false, PERH, false, NW>(c, 13, L(a.px2), FB_G2, hb, hb, FB_G3, wb, L(a.px2), wa, mt0, nch, T);
            flow_gru_chains<PERH, ENCODE, PERH, NW>(c, 14, hb, ENCODE ? L(a.enc0h) : L(a.dec0h), wa, mt0, nch, T);
        }
    }
}

// The 30 instantiations of bvrnn_flow_kernel, keyed by (PERH, program, form): the only place the host names one.  The key says which
// instantiation it is (BVC_FLOW); an entry's LDS bytes are what FlowLds lays out for its form.  tools/flow_host_check.hip holds the
// list written out by hand: the filler and the plain form of a program give the same bits, so no parity test notices a wrong pick.
enum FlowProgram { FP_ENCODE = 0, FP_DECODE = 1, FP_CONCEAL = 2 };
typedef void (*FlowFn)(const FlowArgs *);
struct FlowKernel { int perh, program, form; FlowFn fn; size_t lds; };
#define BVC_FLOW(PERH, P, F) {PERH, P, F, bvrnn_flow_kernel<PERH, (P) != FP_DECODE, (F) == FF_FILL, 8, ((F) >= FF_CHAINS), \
                                                            ((F) >= FF_CHAINS ? (F) - FF_CHAINS : -1), (P) == FP_CONCEAL>, FlowLds<8>::bytes(F)}
#define BVC_FLOW_FORMS(PERH, F0, F1) BVC_FLOW(PERH, FP_ENCODE, F0), BVC_FLOW(PERH, FP_ENCODE, F1), BVC_FLOW(PERH, FP_DECODE, F0), \
                                     BVC_FLOW(PERH, FP_DECODE, F1), BVC_FLOW(PERH, FP_CONCEAL, F0), BVC_FLOW(PERH, FP_CONCEAL, F1)
static const FlowKernel FLOW_KERNELS[] = {
    BVC_FLOW_FORMS(1, FF_PLAIN, FF_FILL), BVC_FLOW_FORMS(2, FF_PLAIN, FF_FILL), BVC_FLOW_FORMS(4, FF_PLAIN, FF_FILL),
    BVC_FLOW_FORMS(8, FF_PLAIN, FF_FILL), BVC_FLOW_FORMS(8, FF_CHAINS, FF_CHAINS_FOLDED),      // interleaved chains are built for h_dim 1024
};
static const FlowKernel *flow_kernel(int perh, int program, int form) {
    for (const FlowKernel &k : FLOW_KERNELS)
        if (k.perh == perh && k.program == program && k.form == form) return &k;
    return nullptr;
}

// k-blocks per wave of an h_dim-sized segment, or 0 if this h_dim is not laid out for the persistent kernel (the PERH of FLOW_KERNELS)
int flow_perh(int h_dim) {
    if (h_dim % 16) return 0;
    if (h_dim == 128) return 1;
    if (h_dim == 256) return 2;
    if (h_dim == 512) return 4;
    if (h_dim == 1024) return 8;
    if (h_dim < 128) return 1;
    return 0;
}

// every entry (and the census kernel) needs more dynamic LDS than a kernel gets unasked
int flow_kernels_init() {
    for (const FlowKernel &k : FLOW_KERNELS)
        BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
    return flow_census_init();
}

// Which kernel a launch takes: validation, then the lookup.  Null: refused, the reason in set_error.
static const FlowKernel *flow_pick(const FlowArgs &a, int perh, bool encode, bool fill, bool conceal) {
    const bool chains = a.MG > 1;                          // interleaved chains: more utterance groups than workgroup slots per feature tile
    if (conceal && (!encode || !a.codes_in || !a.codes || !a.bits)) { set_error("launch_flow: the concealing program needs the encode layout, codes and a selector"); return nullptr; }
    if (chains && perh != 8) { set_error("launch_flow: interleaved chains are built for h_dim 1024 only"); return nullptr; }
    const FlowKernel *k = flow_kernel(perh, conceal ? FP_CONCEAL : (encode ? FP_ENCODE : FP_DECODE),
                                      chains ? (a.pxc.w ? FF_CHAINS_FOLDED : FF_CHAINS) : (fill ? FF_FILL : FF_PLAIN));
    if (!k) set_error("launch_flow: unsupported blocks per wave %d", perh);
    return k;
}

// d_args: device memory for a copy of `a` (read by the kernel through the scalar cache); it must stay untouched until the
// launch has finished.
// (A 4-wave form - bvrnn_flow_kernel<16, ., false, 4>: one wave per SIMD, 214 VGPRs, so that the vocoder of the same or of
// another call could share the CUs with the recurrence - was built and measured: correct, but 27 % slower per frame, and with
// four batches in flight 5,120 audio-s/s against 5,700.  NW stays a template parameter; only the 8-wave form is instantiated.)
int launch_flow(const FlowArgs &a, FlowArgs *d_args, int perh, bool encode, bool fill, hipStream_t s, bool args_resident, bool conceal) {
    const FlowKernel *k = flow_pick(a, perh, encode, fill, conceal);
    if (!k) return BVC_EINVAL;
    int rc;
    if (!args_resident && (rc = launch_flow_set_args(a, d_args, s))) return rc;
    const int grid = ((a.NTG + 7) / 8) * 8 * (a.MG > 1 ? (a.MT + a.MG - 1) / a.MG : a.MT);
    hipLaunchKernelGGL(k->fn, dim3(grid), dim3(512), k->lds, s, static_cast<const FlowArgs *>(d_args));
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
