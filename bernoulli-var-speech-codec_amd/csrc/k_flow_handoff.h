// The persistent recurrence's hand-off between workgroups and its weight loads (device code, included by k_flow.hip behind the
// compile-time tunables; the layer bodies are k_flow_layers.h, the GRU cell k_flow_gru.h).
//
// There is no grid barrier and no flag: the hand-off is "poisoned buffer" dataflow.
//   * every activation buffer exists twice (frame parity) and starts filled with a NaN sentinel;
//   * a producer stores its 1 KiB output block write-through (sc1) and re-arms its block of the other
//     parity with the sentinel (its readers finished a frame ago);
//   * a consumer wave watches the last dword of each producer block it needs (one sc1 load per poll),
//     then fetches the blocks with sc1 loads (they bypass the non-coherent L1) and verifies that no
//     dword is the sentinel before it multiplies.  A value equal to the sentinel is never published.
// Every wait is bounded: a wave that waits too long records it in the model's status word and stops
// waiting for good (results are then garbage, the kernel still ends) - bvc_model_status() reports it.
//
// Measured form of the hand-off: MI355X_MICROARCH.md (valid forms: sc1 stores, sc1 loads, data-tagged
// granules), tools/persist_bench.hip (3.3-3.8 us per 1024x1024 layer against 4.25 launch-per-layer).
#pragma once
#include "k_gemm.h"             // f32x4, mfma16, elu1, sigmoid1: one definition for every kernel that computes a layer

namespace bvc {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int AUX_SC1 = 16;

// the status word lives in host-mapped pinned memory (the host reads it without synchronising): a plain system-scope store
__device__ __forceinline__ void flow_report(unsigned *status, unsigned code) {
    __hip_atomic_store(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct FlowWg {
    __amdgpu_buffer_rsrc_t rs;       // the flow region
    int lane, wave, mtile, ntile;
    int wmul;                        // 1 (0 in the hot-weights timing experiment)
    unsigned spin_limit;
    unsigned *status;
};

// "Does a fetched block still hold the sentinel" as an unsigned maximum over the block's dwords (two v_max3_u32 and a compare per 16 bytes);
// nothing but the sentinel itself may then lie at or above it: publishable() maps every such bit pattern (negative NaNs with an all-ones
// payload top) to the canonical NaN.
__device__ __forceinline__ unsigned umax3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ bool is_poison4(const u32x4 v) {
    return umax3(umax3(v[0], v[1], v[2]), v[3], 0u) >= FLOW_POISON;
}

// one more round of a bounded wait: past the limit the wave gives up for good and says so in the status word
__device__ __forceinline__ void flow_spin(const FlowWg &g, int lane, unsigned &spins, bool &give_up, unsigned code) {
    if (++spins > g.spin_limit) {
        give_up = true;
        if (lane == 0) flow_report(g.status, code);
    }
}

// Operand blocks [kb0, kb0 + PER) of utterance group g.mtile from the flow buffer at byte offset `buf`
// (nbdim blocks per utterance group), waiting for their producers.
// (Tried and dropped: a self-tuned delay followed by fetching the blocks directly, without the flag poll - 0.4 us per
// layer faster in tools/persist_bench.hip, no faster in the real step, whose layers are bound by the operand stream.)
struct FlowSrc { unsigned base, vl; };     // scalar byte offset of this wave's first operand block, lane offset

// Waits until the producers of blocks [kb0, kb0 + PER) of utterance group g.mtile have published them (one dword per
// producer block and poll).  A flag can be visible before the rest of its block: the consumer still verifies what it fetches.
template <int PER>
__device__ __forceinline__ FlowSrc flow_wait(const FlowWg &g, unsigned buf, int nbdim, int kb0, bool &give_up, unsigned code,
                                             unsigned &spins) {
    FlowSrc s;
    // uniform part of every address in the scalar offset, lane part in one shared VGPR
    s.base = __builtin_amdgcn_readfirstlane(buf + (unsigned)(g.mtile * nbdim + kb0) * 1024u);
    s.vl = (unsigned)g.lane * 16u;
    const unsigned fl = (unsigned)(g.lane < PER ? g.lane : PER - 1) * 1024u + 63u * 16u + 12u;
    while (!give_up) {
        const unsigned t = __builtin_amdgcn_raw_buffer_load_b32(g.rs, fl, s.base, AUX_SC1);
        if (!__any(t == FLOW_POISON)) break;
        __builtin_amdgcn_s_sleep(BVC_FLOW_POLL_SLEEP);
        flow_spin(g, g.lane, spins, give_up, code);
    }
    return s;
}

// A segment's operand blocks are requested strictly in k order and multiplied in that order, each as soon as IT has arrived (a wave's loads
// return in order), with the sentinel checks behind the last product.  The scheduling fences make that true: hipcc otherwise schedules the
// checks - which need every block - in front of the first product and requests block 0 second to last, so that all eight blocks have to be
// there before the first MFMA issues.
template <int PER>
__device__ __forceinline__ void flow_issue(const FlowWg &g, const FlowSrc &s, u32x4 (&xr)[PER]) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        xr[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(g.rs, s.vl, s.base + (unsigned)u * 1024u, AUX_SC1));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Lane's view of a run of weight blocks: a wave-uniform byte pointer (kept in SGPRs, re-derived every frame so that the
// compiler does not hoist fourteen layers' worth of per-lane addresses out of the frame loop) plus lane * 16.
typedef const char __attribute__((address_space(1))) *GPtr;        // global (not flat) loads
__device__ __forceinline__ GPtr uniform_ptr(const float *w, size_t block) {
    unsigned long long p = reinterpret_cast<unsigned long long>(w) + (block << 10);
    asm volatile("" : "+s"(p));
    return (GPtr)p;
}
__device__ __forceinline__ f32x4 wload(GPtr ub, unsigned lane16, int blk) {
    // (Measured and not kept: the part of blk * 1024 beyond the instruction's 4095-byte immediate moved into an opaque SCALAR base - a
    // third fewer 64-bit vector adds in front of the reduction barrier, and 0.15 ms per step slower: profiles/r04_flow_variants.txt)
    return *reinterpret_cast<const f32x4 __attribute__((address_space(1))) *>(ub + lane16 + (unsigned)blk * 1024u);
}

// a weight set defined as zeros (where this workgroup has no tile of the layer: no value lives across the layer)
template <int N>
__device__ __forceinline__ void wzero(f32x4 (&wn)[N]) {
#pragma unroll
    for (int u = 0; u < N; ++u) wn[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ u32x4 publishable(f32x4 o, bool rowok) {
    u32x4 b = __builtin_bit_cast(u32x4, o);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (b[j] >= FLOW_POISON) b[j] = 0x7FC00000u;       // never publish the sentinel as data
        if (!rowok) b[j] = 0u;                             // padding rows of the last utterance group stay zero
    }
    return b;
}

}  // namespace
}  // namespace bvc
