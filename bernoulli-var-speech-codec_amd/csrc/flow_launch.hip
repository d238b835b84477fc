// The host side of the persistent recurrence (k_flow.hip): the hop tables, the launch with its tickets and fences, the RS_AUTO
// switch between the two schedules, and the environment switches of the schedule.
#include "recurrence.h"

using namespace bvc;

namespace {

inline FlowLin flin(const Linear &l, size_t kb_offset = 0, bool with_bias = true) {
    FlowLin f;
    f.w = l.wp + kb_offset * 256; f.bias = with_bias ? l.b : nullptr; f.wnb = l.in / 16; f.pad_ = 0;
    return f;
}

// The layers of one frame (encode: bvrnn.py:187-206, decode: bvrnn.py:222-227).  Halves of a concatenated input that do
// not depend on the frame's own chain - phi_x(y_t) in enc.0, phi_z(z_t) in dec.0 and in the GRU's input gates when the
// codes are known - are batched over all frames beforehand and enter as addends (part0 / part_gru).
void flow_layers(const bvc_model *m, bool encode, FlowArgs *a, bool conceal = false) {
    const int hb = m->cfg.h_dim / 16;
    a->enc0h = flin(m->enc[0], hb, false);            // enc.0[:, H:] h  (+ part0 = enc.0[:, :H] phi_x + b)
    a->enc1 = flin(m->enc[1]);
    a->enc2 = flin(m->enc[2]);
    if (conceal) {                                    // the concealing decoder: the prior net in the encoder's place, its first bias its own
        a->enc0h = flin(m->prior[0]);
        a->enc1 = flin(m->prior[1]);
        a->enc2 = flin(m->prior[2]);
    }
    a->pz0 = flin(m->phi_z[0]);
    a->pz1 = flin(m->phi_z[1]);
    a->pz2 = flin(m->phi_z[2]);
    a->dec0h = flin(m->dec[0], hb, encode);           // dec.0[:, H:] h; decode: + part0 = dec.0[:, :H] phi_z + b
    a->dec0z = flin(m->dec[0], 0, false);             // dec.0[:, :H] phi_z (encode)
    a->dec1 = flin(m->dec[1]);
    a->dec2 = flin(m->dec[2]);
    a->dec3 = flin(m->dec[3]);
    a->px0 = flin(m->phi_x[0]);
    a->px1 = flin(m->phi_x[1]);
    a->px2 = flin(m->phi_x[2]);
    if (((encode && !conceal) ? m->encode_fold : m->decode_fold) && m->px0_dec3.wp) a->pxc = flin(m->px0_dec3);      // (a concealing decoder is a decoder)
    a->w_hh = m->w_hh_il;
    a->w_ihx = m->w_ih_il;
    a->w_ihz = m->w_ih_il + (size_t)hb * 3 * 256;
    a->b_ih = m->b_ih; a->b_hh = m->b_hh;
    a->hb = hb; a->zb = m->cfg.z_dim / 16; a->xb = m->cfg.num_mels / 16;
}

constexpr int FLOW_MAX_CHAINS = 8;

// What the persistent launches of one device share (any model of this process); g_flow_mu guards it.
//   Tickets: the persistent kernel needs all its workgroups resident at once (they wait for each other), so launches from different
// streams are serialised through one event: at most one is in flight per process and device (BVC_FLOW_TICKETS=2: two).
//   RS_AUTO: the end of the last recurrence-bearing call on this device and the stream it ran on.  A call that starts while the
// previous one - issued on ANOTHER stream - is still running has company: batches are in flight on several streams, where the
// launch-per-layer chains of the streams interleave on the chip while persistent launches (each takes every compute unit) would run
// one after the other.  The switch is sticky for AUTO_HOLD calls so that all streams change together.
//   Fences (bvc_flow_fence): work a caller issued on some stream - an RCCL collective that holds compute units while it waits for
// its peers, say - that must have finished before the next persistent launch starts.  A small ring; a persistent launch
// waits for every pending entry (later launches wait for that launch through the ticket).
constexpr int FLOW_MAX_TICKETS = 2;
constexpr int AUTO_HOLD = 2;
constexpr int FLOW_FENCES = 8;
struct LastCall { hipEvent_t ev = nullptr; hipStream_t s = nullptr; bool any = false; int hold = 0; };
struct FlowFence { hipEvent_t ev = nullptr; bool pending = false; };
struct FlowDevice {
    hipEvent_t ticket[FLOW_MAX_TICKETS] = {};
    unsigned long long launches = 0;
    LastCall last;
    FlowFence fence[FLOW_FENCES];
    unsigned fences = 0;
};
FlowDevice g_flow_dev[16];

// the calling thread's device; null if it cannot be asked (the HIP error stays pending; with `report` it is the error text, as BVC_HIP_TRY writes it)
FlowDevice *flow_device(bool report = true) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        if (report) set_error("%s failed: %s (%s:%d)", "hipGetDevice(&dev)", hipGetErrorString(e), __FILE__, __LINE__);
        return nullptr;
    }
    return &g_flow_dev[dev & 15];
}

inline float *flow_buf(const Workspace &w, int id, int parity) { return w.flow + (size_t)(id * 2 + parity) * w.flow_slot; }

}  // namespace

namespace bvc {

std::mutex g_flow_mu;

// ---- the switches of the persistent recurrence (host only), all read here and nowhere else:
//   once per process    BVC_FLOW_HOTW        experiments: every weight request hits the same blocks (wrong results; FlowArgs::dbg_hot_w)
//                       BVC_FLOW_FILL=0      the plain kernels instead of the filler form
//                       BVC_FLOW_TICKETS=2   two persistent launches may be in flight per device instead of one
//                       BVC_FLOW_NO_CHAINS   batches beyond one chain per workgroup take the launch-per-layer schedule
//   at every call that stamps (probing)      BVC_PROBE_WG / BVC_PROBE_WAVE: which workgroup / wave records the stamps (default 0 / 0)
FlowSwitches flow_switches(bool probing) {
    static const bool hot_w = getenv("BVC_FLOW_HOTW") != nullptr, fill = !(getenv("BVC_FLOW_FILL") && getenv("BVC_FLOW_FILL")[0] == '0'),
                      no_chains = getenv("BVC_FLOW_NO_CHAINS") != nullptr;
    static const int tickets = (getenv("BVC_FLOW_TICKETS") && atoi(getenv("BVC_FLOW_TICKETS")) == 2) ? 2 : 1;
    FlowSwitches sw = {hot_w, fill, no_chains, tickets, 0, 0};
    if (probing) {
        sw.probe_wg = getenv("BVC_PROBE_WG") ? atoi(getenv("BVC_PROBE_WG")) : 0;
        sw.probe_wave = getenv("BVC_PROBE_WAVE") ? atoi(getenv("BVC_PROBE_WAVE")) & 7 : 0;
    }
    return sw;
}

// The persistent kernel needs every one of its workgroups resident (they wait for each other) and a workgroup takes a whole
// compute unit (8 waves x 256 VGPRs): utterance groups x feature tiles must not exceed the device's CU count (256 on MI355X:
// up to 64 utterances at h_dim 1024).  Anything else takes the launch-per-layer schedule.
// Larger batches interleave MG utterance groups ("chains") per workgroup (h_dim 1024 only; k_flow.hip, MULTI).
int flow_chains_static(const bvc_model *m, int B) {      // 0: not usable; else utterance groups per workgroup
    if (m->recurrence == RS_LAYERS || m->side_branch || !m->flow_resident || (g_stream_tick && !g_tick_flow) || m->flow_perh <= 0) return 0;
    const int ntg = flow_grid_tiles(m);
    const int mt = (B + 15) / 16;
    const int slots = m->cu_count / ntg;                   // workgroups per feature tile that fit on the device
    if (slots <= 0) return 0;
    const int mg = (mt + slots - 1) / slots;
    if (mg <= 1) return 1;
    if (flow_switches().no_chains || m->flow_perh != 8 || mg > FLOW_MAX_CHAINS) return 0;
    return mg;
}

// Which schedule does THIS call take?  0: launch per layer; else utterance groups per workgroup of the persistent kernel.
// Called once per recurrence-bearing call (run_encode / run_decode); mark_call_end() follows at its end.
int flow_chains(const bvc_model *m, int B, hipStream_t s) {
    if (m->census_due && (!g_stream_tick || g_tick_flow)) {               // a time-out was reported: is a full grid still co-resident?  (synchronises: error path only)
        if (capture_state(s) == CAP_NONE) {
            m->census_due = false;
            (void)flow_census(m);
        } else {
            (void)hipGetLastError();
        }
    }
    const int chains = flow_chains_static(m, B);
    if (!chains) return 0;
    const Capture cap = capture_state(s);
    if (cap == CAP_FAILED) { (void)hipGetLastError(); return 0; }
    // a caller's capture: the persistent launch cannot be captured (its one-at-a-time ticket is a host-side wait on an event
    // recorded outside the capture, and replays would skip it): captured calls take the launch-per-layer kernels
    if (cap == CAP_ACTIVE) return 0;
    if (m->recurrence != RS_AUTO) return chains;
    FlowDevice *fd = flow_device(false);
    if (!fd) { (void)hipGetLastError(); return chains; }
    std::lock_guard<std::mutex> lk(g_flow_mu);
    LastCall &lc = fd->last;
    const bool company = lc.any && lc.s != s && hipEventQuery(lc.ev) == hipErrorNotReady;
    (void)hipGetLastError();
    if (company) lc.hold = AUTO_HOLD;
    else if (lc.hold > 0) --lc.hold;
    return (company || lc.hold > 0) ? 0 : chains;
}

int mark_call_end(hipStream_t s) {
    if (capture_state(s) != CAP_NONE) { (void)hipGetLastError(); return BVC_OK; }
    FlowDevice *fd = flow_device();
    if (!fd) return BVC_EHIP;
    std::lock_guard<std::mutex> lk(g_flow_mu);
    LastCall &lc = fd->last;
    if (!lc.ev) BVC_HIP_TRY(hipEventCreateWithFlags(&lc.ev, hipEventDisableTiming));
    BVC_HIP_TRY(hipEventRecord(lc.ev, s));
    lc.s = s; lc.any = true;
    return BVC_OK;
}

// All T frames of BVRNN.encode (encode = true) or BVRNN.decode in one launch.  w.part_dec0 (and w.part_gru for decode)
// must hold the pre-computed halves; h0 may be null (zero state).
int run_flow(const bvc_model *m, const Workspace &w, bool encode, int chains, const float *d_h0, int B, int64_t T, const float *d_bits,
             float *d_codes, float *d_prob, float *d_all_h, float *d_mel, float *d_hT, hipStream_t s, const float *d_codes_in) {
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    const int mt16 = pad16(B);
    const bool conceal = d_codes_in != nullptr;        // the concealing decoder (encode = true: its program is encode's; d_bits = the selector)
    int rc;
    {
        const Capture cap = capture_state(s, true);
        if (cap == CAP_FAILED) return BVC_EHIP;
        if (cap == CAP_ACTIVE) { set_error("the persistent recurrence cannot be captured into a graph"); return BVC_EINVAL; }
    }
    float *h0p = flow_buf(w, FB_H, 0);
    FlowArgs a;
    memset(&a, 0, sizeof(a));
    flow_layers(m, encode, &a, conceal);
    a.codes_in = d_codes_in;
    a.flow = w.flow;
    a.slot_bytes = (unsigned)(w.flow_slot * sizeof(float));
    a.B = B; a.MT = mt16 / 16; a.T = T;
    a.MG = chains;
    a.NTG = (H > X ? (H > Z ? H : Z) : (X > Z ? X : Z)) / 16;
    a.part0 = w.part_dec0;
    a.part_gru = encode ? nullptr : w.part_gru;
    a.codes = d_codes; a.prob = d_prob; a.bits = d_bits; a.all_h = d_all_h; a.mel = d_mel;
    a.keep = (encode && !d_mel) ? nullptr : w.pxB;   // folded hop: ELU(dec.4) of all frames (pxB is idle once the batched phi_x / phi_z layers are through);
                                                     // encode keeps it only when the caller wants the decoder's output too (bvc_forward)
    a.mean = m->mean_mel; a.stdv = m->std_mel;
    a.var_bit = m->cfg.var_bit;
    a.status = m->d_status;
    const FlowSwitches sw = flow_switches(g_kprobe.enabled);
    a.dbg_hot_w = sw.hot_w ? 1 : 0;
    a.spin_limit = m->flow_spin_limit;
    a.dbg_withhold = m->flow_debug_withhold;
    if (g_kprobe.enabled) {                    // bench instrumentation: per-layer entry / exit stamps of workgroup 0
        const int nodes = encode ? 14 : 8;
        const size_t need = (size_t)FLOW_STAMPS * T * nodes;
        if (need > g_kprobe.capacity) { set_error("kprobe buffer too small for T=%lld", (long long)T); return BVC_EINVAL; }
        BVC_HIP_TRY(hipMemsetAsync(g_kprobe.dev, 0, need * sizeof(unsigned long long), s));
        g_kprobe.T = T; g_kprobe.nodes = nodes;
        a.probe = g_kprobe.dev; a.probe_nodes = nodes; a.probe_first = encode ? 1 : 7;
        a.probe_wg = sw.probe_wg;
        a.probe_wave = sw.probe_wave;
    }
    // the flow region filled with the sentinel, h(-1) in its first buffer (FB_H, parity 0, at the start of the region) and the device copy
    // of the arguments: one kernel (a misaligned initial state takes the three separate ones)
    const long long n_flow = (long long)FB_COUNT * 2 * (long long)w.flow_slot;
    const bool fused_prepare = !d_h0 || (reinterpret_cast<uintptr_t>(d_h0) & 15) == 0;
    if (fused_prepare) {
        if ((rc = launch_flow_prepare(a, w.flow_args, reinterpret_cast<unsigned *>(w.flow), n_flow, (long long)mt16 * H, d_h0, B, H, s))) return rc;
    } else {
        if ((rc = launch_fill_u32(reinterpret_cast<unsigned *>(w.flow), FLOW_POISON, n_flow, s))) return rc;
        if ((rc = launch_fill(h0p, 0.0f, (long long)mt16 * H, s))) return rc;
        if ((rc = launch_repack_rows(d_h0, h0p, H, B, H, 0, s))) return rc;
    }
    if (d_all_h && (rc = launch_repack_rows(h0p, d_all_h, (long long)T * H, B, H, 1, s))) return rc;     // all_h[:, 0] = h0
    {
        std::lock_guard<std::mutex> lk(g_flow_mu);
        FlowDevice *fd = flow_device();
        if (!fd) return BVC_EHIP;
        hipEvent_t &ev = fd->ticket[fd->launches % sw.tickets];        // the launch `tickets` launches ago must have finished
        if (!ev) BVC_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (fd->launches >= (unsigned long long)sw.tickets) BVC_HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        for (auto &f : fd->fence)
            if (f.pending) { BVC_HIP_TRY(hipStreamWaitEvent(s, f.ev, 0)); f.pending = false; }
        ProbeScope probe(PK_LINEAR, s);
        if ((rc = launch_flow(a, w.flow_args, m->flow_perh, encode, sw.fill && !m->flow_debug_nofill && a.MG == 1, s, fused_prepare, conceal))) return rc;
        BVC_HIP_TRY(hipEventRecord(ev, s));
        ++fd->launches;
    }
    if (d_hT && (rc = launch_repack_rows(flow_buf(w, FB_H, (int)(T & 1)), d_hT, H, B, H, 1, s))) return rc;
    // folded decode: the decoder's output dec.6(u_t) for all frames at once (bvrnn.py:224-225)
    if (a.pxc.w && d_mel && (rc = decode_epilogue(m, w.pxB, B, T, d_mel, s))) return rc;
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int bvc_flow_fence(void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const Capture cap = capture_state(s, true);
    if (cap == CAP_FAILED) return BVC_EHIP;
    if (cap == CAP_ACTIVE) { set_error("bvc_flow_fence: not while the stream is being captured"); return BVC_EINVAL; }
    FlowDevice *fd = flow_device();
    if (!fd) return BVC_EHIP;
    std::lock_guard<std::mutex> lk(g_flow_mu);
    FlowFence &f = fd->fence[fd->fences++ % FLOW_FENCES];
    if (!f.ev) BVC_HIP_TRY(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    // a slot that is still pending holds a fence nobody has waited for yet (more than FLOW_FENCES fences without a persistent launch in
    // between): order this stream behind it first, so that the new record implies the old one
    if (f.pending) BVC_HIP_TRY(hipStreamWaitEvent(s, f.ev, 0));
    BVC_HIP_TRY(hipEventRecord(f.ev, s));
    f.pending = true;
    return BVC_OK;
}

}  // extern "C"
