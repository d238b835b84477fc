// Host side of libbvcodec_hip.so, shared by its sources model_build.hip, model.hip, recurrence.hip, step_plan.hip, flow_launch.hip,
// backward.hip, optimizer.hip, generator.hip, stream_codec.hip and bvcodec_abi.hip (what only the three sources of the recurrence share is in recurrence.h; the
// arithmetic behind every uploaded weight is weight_pack.h, which model_build.hip alone includes): the model, the workspace layout, the GEMM parameter helpers, the drivers of the offline paths and the state that
// crosses a file boundary.  Host only.  What more than one source uses lives in namespace bvc, next to the launchers of
// bvc_internal.h; everything else is local to its file.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <list>
#include <mutex>

#include "bvc_internal.h"

namespace bvc {

struct Linear { const float *w = nullptr, *wp = nullptr, *b = nullptr; int in = 0, out = 0; };   // w natural, wp fragment-packed

struct AmpPair { ConvLayer c1, c2; };

// ---- incremental (history-buffer) vocoder for streaming --------------------------------------------
// Every activation tensor of the generator is kept as a (B, H + kmax*rate, C) buffer whose first H rows
// are the last H rows of the previous hop; a hop computes only the rows of the new frames and then
// rotates the last H rows to the front of the twin buffer (ping-pong: source and destination overlap
// when fewer than H rows are new).
struct StreamTensor { float *buf[2]; int C, H, rate; long long rows; };
struct RotEntry { float *buf[2]; long long bs; int C, H, rate, pad_; };

}  // namespace bvc

struct bvc_model {
    bvc_config cfg;
    std::vector<void *> allocs;
    // front-end
    bvc::FrontendTables fe;
    // BVRNN
    const float *mean_mel = nullptr, *std_mel = nullptr;
    bvc::Linear phi_x[3], phi_z[3], enc[3], dec[4];
    bvc::Linear prior[3];            // only used by bvc_bvrnn_forward; optional (has_prior)
    bool has_prior = false;
    const float *w_ih = nullptr, *w_hh = nullptr, *b_ih = nullptr, *b_hh = nullptr;     // w_*: fragment-packed
    const float *w_ih_il = nullptr, *w_hh_il = nullptr;   // gate-interleaved packing (pack_gru_interleaved): the GRU launches
    const float *w_ih_nat = nullptr;      // natural [3H][2H] copy: the phi_z half is applied to all frames at once in decode
    // vocoder
    bvc::ConvLayer conv_pre;
    std::vector<bvc::ConvLayer> ups;                       // n_up
    std::vector<std::vector<std::vector<bvc::AmpPair>>> amp;   // [stage][kernel][dilation]
    std::vector<int> stage_ch;                        // channels after each upsampler
    const float *post_a = nullptr, *post_ib = nullptr, *post_w = nullptr, *post_b = nullptr;
    const float *post_up = nullptr, *post_down = nullptr;   // antialias_post: activation_post's two filters
    int post_c = 0, post_ks = 7;
    bool antialiased = false;   // some stage, or activation_post, has anti-aliased activations: the generator is not causal
    std::vector<bool> stage_sym;        // layers_sym: upsampler i and the stage's AMP blocks pad symmetrically (models.py:35-44,151-155)
    bool pre_sym = false, post_sym = false;   // conv_pre / conv_post pad [3, 3] instead of [6, 0]
    bool symmetric = false;     // any of them
    bool noncausal = false;     // antialiased || symmetric: what streaming, the windowed test entry and mixed lengths refuse
    // captured recurrent steps (hipGraph), keyed by (kind, batch, workspace)
    // (launch-per-layer schedule only) most recently used first; `idle` is recorded behind the entry's last replay, so an
    // entry is only destroyed once the GPU is done with it
    struct StepGraph { int kind; int B; void *ws; void *probe; hipGraphExec_t exec1, execN; hipEvent_t idle; };
    mutable std::list<StepGraph> graphs;
    mutable std::mutex graph_mu;
    mutable hipStream_t cap_stream = nullptr, side_stream = nullptr;
    mutable std::vector<hipEvent_t> cap_events;
    bool side_branch = false;   // measured SLOWER on MI355X (cross-branch graph dependencies + no spare L2->CU bandwidth): opt-in
    bool use_graph = true;
    bool fused_amp = true;
    unsigned amp_kernels = bvc::AMPK_ALL;   // stage-specific generator kernels in use (options vocoder_full_tiles / vocoder_c16_kernel)
    bool precomp_pz = true;     // decode: the phi_z halves of dec.0 and of the GRU input product are batched over all frames
    int mtw = 1;                // 16-row tiles per workgroup in the recurrent kernels (BVC_MTW = 1 | 2 | 4)
    // persistent recurrence (k_flow.hip, its device code in k_flow_handoff.h / k_flow_layers.h / k_flow_gru.h): hop tables of encode / decode, resident in device memory
    // recurrence schedule: RS_PERSISTENT one launch per call (k_flow.hip), RS_LAYERS one launch per layer (hipGraph replay),
    // RS_AUTO (default) persistent while calls come one at a time, layers while calls of several streams overlap
    int recurrence = 2;         // BVC_RECURRENCE=persistent|layers|auto, bvc_model_set_option("recurrence")
    mutable std::atomic<bool> flow_resident{false}; // the residency census found a full persistent grid co-resident on this device
    mutable std::atomic<bool> census_due{false};    // a recurrence time-out was seen: the census runs again before the next persistent launch (another
                                        // tenant may have arrived after bvc_model_create: the model then moves to the layer schedule)
    mutable hipStream_t census_stream = nullptr;
    mutable unsigned *census_ctr = nullptr;
    int flow_perh = 0;          // k-blocks per wave of an h_dim-sized segment (0: h_dim not supported by the persistent kernel)
    // sticky status word of the persistent kernels, in host-mapped pinned memory: a kernel whose wait timed out stores its
    // code there; every compute entry point reads it WITHOUT synchronising (h_status) and reports BVC_ETIMEOUT once
    volatile unsigned *h_status = nullptr;
    unsigned *d_status = nullptr;       // device address of the same word
    int cu_count = 0;                   // compute units of the device: a persistent launch needs one per workgroup
    unsigned flow_spin_limit = 4000000u;   // polls before a wait gives up (> 1 s: only a workgroup that never became resident gets there)
    int flow_debug_withhold = 0;        // tests only: workgroup 0 of a persistent launch returns at once (its peers time out)
    int flow_debug_nofill = 0;          // tests only: no filler quanta (the plain layer program)
    // decode_fold / encode_fold (default 1): the persistent kernels run phi_x.0(norm(dec.6(u))) - three maps without a non-linearity
    // between them (bvrnn.py:80, :204 / :226) - as the one affine map px0_dec3 (folded in float64 at model creation): one wide layer
    // instead of two narrow hops per frame.  Decode computes dec.6 itself, the decoder's output, as one batched GEMM behind the
    // launch; encode does not need it (BVRNN.encode returns codes and states only).  In encode the folded layer feeds the next
    // state and with it the next codes: same function, another rounding (like another order of summation) - every golden and the
    // full-size parity runs give the same bits and the same largest probability deviation (1.2e-7) with and without it.
    bvc::Linear px0_dec3{};
    int decode_fold = 1;
    int encode_fold = 1;
    // The backward pass (backward.hip): the transposed weights, natural (.w) and fragment-packed (.wp) with in / out swapped, so that
    // dX = dY W is a forward layer of the kernels as they stand.  Made on the first bvc_bvrnn_backward (or bvc_bvrnn_backward_prepare),
    // under bwd_mu; a model that never calls them allocates nothing.  Order: phi_x.0/2/4, phi_z.0/2/4, enc.0/2/4, prior.0/2/4, dec.0/2/4/6,
    // rnn.weight_ih, rnn.weight_hh.
    mutable std::mutex bwd_mu;
    mutable bool bwd_ready = false;
    mutable bvc::Linear bwd_t[18];
    mutable std::vector<void *> bwd_allocs;
    // The optimiser (optimizer.hip): the flat float32 master copy of the 36 trainable tensors in grad_layout order.  Made on the first
    // bvc_bvrnn_params_set or bvc_optimizer_step, under bwd_mu, from the values the model holds; from then on bvc_bvrnn_params_set
    // writes it and every form derived from it (a step updates it in place and ends in that rewrite).  A model that never calls them
    // allocates nothing.
    mutable float *master = nullptr;

    ~bvc_model() {
        for (auto &g : graphs) { (void)hipGraphExecDestroy(g.exec1); (void)hipGraphExecDestroy(g.execN); if (g.idle) (void)hipEventDestroy(g.idle); }
        if (census_stream) (void)hipStreamDestroy(census_stream);
        if (census_ctr) (void)hipFree(census_ctr);
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        if (side_stream) (void)hipStreamDestroy(side_stream);
        for (auto e : cap_events) (void)hipEventDestroy(e);
        if (h_status) (void)hipHostFree(const_cast<unsigned *>(h_status));
        for (void *p : allocs) (void)hipFree(p);
        for (void *p : bwd_allocs) (void)hipFree(p);
        if (master) (void)hipFree(master);
    }
};

struct bvc_vocoder_stream {
    const bvc_model *m = nullptr;
    int B = 0, kmax = 0, parity = 0;
    // slide: ONE buffer per tensor with room for cap_frames frames; the window of a hop starts `cursor` frames into it and the history is
    // moved back to the front only when the room is used up (every cap_frames / kmax - 1 hops at least) instead of after every hop.  The
    // addresses of a hop then change from hop to hop: not for a hop that is replayed from a graph (bvc_stream_codec's eager ticks only).
    bool slide = false;
    int cursor = 0, cap_frames = 0;
    int64_t frames = 0;
    float *pool = nullptr;
    size_t pool_floats = 0;
    bvc::RotEntry *d_tab = nullptr;
    int n_ten = 0, max_hc4 = 0;
    // rows that start at different times (bvc_stream_codec's slots): frames since each row's own start, capped at STREAM_WARM_FRAMES,
    // in device memory owned by the session (nullptr: every row started with the state, `frames` decides)
    const int *d_age = nullptr;
    bvc::StreamTensor mel, y0;
    std::vector<bvc::StreamTensor> X, XS;                  // per stage
    std::vector<bvc::StreamTensor> P, Q;                   // per (stage, AMP block): each block's intermediates keep their own history
    // look-ahead window (bvc_vocoder_stream_create_lookahead; generator.hip): after n frames, rows [0, rate * n - lag) of a tensor are
    // final.  The tensors of a stage share the row numbering of its X - buffer row 0 is row rate * n - lag_x - H of the stage - and end at
    // their own frontiers: P and Q of a block lag_p / lag_q rows before X's, XS `spread` rows.
    bool lookahead = false, flushed = false;
    int64_t delay = 0;                                     // the waveform's lag, in samples
    int lag_y0 = 0, lag_post = 0;                          // conv_pre's and conv_post's own (3 where symmetric)
    std::vector<long long> lag_x, spread, tail;            // per stage; tail: rows of the stage beyond rate * T at the end of the signal
    std::vector<long long> lag_p, lag_q;                   // per (stage, AMP block), relative to X
    ~bvc_vocoder_stream() {
        if (pool) (void)hipFree(pool);
        if (d_tab) (void)hipFree(d_tab);
    }
};

namespace bvc {

// ---- state shared between the sources ---------------------------------------------------------------
extern thread_local bool g_capturing;     // no event probes while THIS thread captures a stream (captures are thread-local)
extern thread_local bool g_stream_tick;   // inside bvc_stream_codec_tick: a launch-per-layer recurrence is launched eagerly (the tick itself is the graph)
extern thread_local bool g_tick_flow;     // ... of a tick that is NOT a graph: its recurrences may take the persistent kernel
extern std::mutex g_flow_mu;              // persistent launches and the residency census, one at a time per process (flow_launch.hip)
// the two tick flags for a scope (a tick's body, a replay pass): no path out of it leaves them set
struct TickFlags {
    explicit TickFlags(bool flow) { g_stream_tick = true; g_tick_flow = flow; }
    ~TickFlags() { g_stream_tick = false; g_tick_flow = false; }
    TickFlags(const TickFlags &) = delete;
    TickFlags &operator=(const TickFlags &) = delete;
};

// in-kernel timestamp probes for the graph-replayed recurrent kernels (wall_clock64, 100 MHz)
struct KProbe {
    bool enabled = false;
    unsigned long long *dev = nullptr;
    size_t capacity = 0;                   // in u64
    long long T = 0; int nodes = 0;        // geometry of the last probed call
};
extern KProbe g_kprobe;

// ---- workspace layout ---------------------------------------------------------------------------
// n rounded up to a multiple of 16: the rows of a fragment-packed matrix of n utterances (whole 16-row tiles), the bytes of a ring slot
template <typename T>
inline T pad16(T rows) { return (rows + 15) / 16 * 16; }

struct Workspace {
    // encode
    float *yn, *pxA, *pxB, *pxC;
    float *step[16];            // per-step [B, max(H, ...)] scratch vectors
    float *hbuf;                // [2][B][H] GRU state ping-pong (parity of the frame counter)
    float *part_i, *part_h, *part_d;   // side-branch partial sums: W_ih[:,H:] phi_z + b_ih, W_hh h + b_hh, dec.0[:,H:] h
    CallDesc *desc;             // per-call dynamic state read by the captured step kernels
    float *mel, *bits;          // facade-level buffers
    float *part_dec0, *part_gru; // decode: dec.0[:, :H] phi_z + b (B,T,H) and W_ih[:, H:] phi_z + b_ih (B,T,3H), all frames
    float *flow;                // persistent recurrence: FB_COUNT x 2 fragment-packed [mt16][dmax] activation buffers
    size_t flow_slot;           // floats per flow buffer
    FlowArgs *flow_args;        // device copy of the persistent kernel's arguments
    // vocoder
    float *y0, *X, *P, *Q, *U, *XS;
    size_t total;
};

int64_t stage_len(const bvc_model *m, int64_t T, int stage);    // length after upsampler `stage`
void carve(const bvc_model *m, int B, int64_t T, char *base, Workspace *w);
int check_ws(const bvc_model *m, int B, int64_t T, void *d_ws, size_t ws_bytes, Workspace *w);
int sticky_status(const bvc_model *m);
int need_prior(const bvc_model *m, const char *fn);
extern const char *const NOT_CAUSAL;
const char *not_causal(const bvc_model *m);     // why a noncausal model is refused: NOT_CAUSAL for a filtered one, else the symmetric text
int build_flow(bvc_model *m);                   // at model creation: is the model laid out for the persistent kernel?  With the first census
int flow_census(const bvc_model *m);
// The environment switches of the model, read by model_switches() alone (model_build.hip, which names them and says when each is read).
// The first eight as the model keeps them (bvc_model_create); the last two are the residency census's
struct ModelSwitches { bool use_graph, side_branch, fused_amp, precomp, decode_fold, encode_fold; int mtw, recurrence; bool census_oversubscribe, quiet; };
ModelSwitches model_switches();

// ---- GEMM parameters ----------------------------------------------------------------------------
inline GemmSeg mkseg(DynPtr x, const float *w, int wnb, int K, int grp) { return GemmSeg{w, wnb, K, x, grp, 0}; }

// keeps nb_total consistent with the segments
inline void finish(GemmParams &p) { p.nb_total = 0; for (int i = 0; i < p.nseg; ++i) p.nb_total += p.seg[i].K / 16; }

// y = x W^T (+ bias) over K columns of a fragment-packed W with wnb k-blocks per row tile: a Linear, a slice of one, or of the GRU's matrices
inline GemmParams mat_params(DynPtr x, const float *wp, int wnb, int K, int M, int N, const float *bias, DynPtr y) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = 1;
    p.seg[0] = mkseg(x, wp, wnb, K, 0);
    p.M = M; p.N = N;
    p.bias0 = bias;
    p.y = y;
    finish(p);
    return p;
}
inline GemmParams lin_params(const Linear &l, DynPtr x, int M, DynPtr y) { return mat_params(x, l.wp, l.in / 16, l.in, M, l.out, l.b, y); }
// the part of a Linear over a concatenated input that starts kb0 k-blocks in: l.w[:, 16 kb0 : 16 kb0 + K] x, with or without l.b
inline GemmParams half_params(const Linear &l, int kb0, DynPtr x, int K, int M, DynPtr y, bool bias) {
    return mat_params(x, l.wp + (size_t)kb0 * 256, l.in / 16, K, M, l.out, bias ? l.b : nullptr, y);
}

// linear over the concatenation [x1 | x2] (torch.cat at bvrnn.py:189,202)
inline GemmParams lin2_params(const Linear &l, DynPtr x1, int K1, DynPtr x2, int K2, int M, DynPtr y) {
    GemmParams p = lin_params(l, x1, M, y);
    p.nseg = 2;
    p.seg[0] = mkseg(x1, l.wp, l.in / 16, K1, 0);
    p.seg[1] = mkseg(x2, l.wp + (size_t)(K1 / 16) * 256, l.in / 16, K2, 0);
    finish(p);
    return p;
}

// ---- schedules and drivers ----------------------------------------------------------------------
enum { RS_PERSISTENT = 0, RS_LAYERS = 1, RS_AUTO = 2 };
inline int flow_grid_tiles(const bvc_model *m) {          // feature tiles covered by a persistent grid (rounded up to 8: one per XCD)
    const int H = m->cfg.h_dim, X = m->cfg.num_mels, Z = m->cfg.z_dim;
    return ((H > X ? (H > Z ? H : Z) : (X > Z ? X : Z)) / 16 + 7) / 8 * 8;
}
// The environment switches of the persistent recurrence, read by flow_switches() alone (flow_launch.hip, which says when): BVC_FLOW_HOTW,
// BVC_FLOW_FILL, BVC_FLOW_TICKETS, BVC_FLOW_NO_CHAINS; with `probing` also BVC_PROBE_WG and BVC_PROBE_WAVE (0 / 0 otherwise)
struct FlowSwitches { bool hot_w, fill, no_chains; int tickets, probe_wg, probe_wave; };
FlowSwitches flow_switches(bool probing = false);
int flow_chains_static(const bvc_model *m, int B);      // 0: not usable; else utterance groups per workgroup

int run_encode(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_mel, const float *d_bits, const float *d_h0, int B,
               int64_t T, float *d_codes, float *d_all_h, float *d_hT, float *d_prob, hipStream_t s, float *d_melhat = nullptr);
int run_decode(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_codes, const float *d_h0, int B, int64_t T,
               float *d_mel, float *d_hT, hipStream_t s);
int run_decode_conceal(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_codes, const float *d_sel, const float *d_h0,
                       int B, int64_t T, float *d_mel, float *d_hT, float *d_codes_out, float *d_prior, hipStream_t s);
// ---- closed-loop rate selection (bvc_bvrnn_encode_vbr): its workspace is the frame buffers of the K * B candidate rows, whose size depends
// on (B, K) alone, FOLLOWED by the ordinary workspace of (B, T) - so every address a captured step holds is a function of (base, B, K)
struct VbrWorkspace {
    float *zraw, *zc, *hrep, *pz[3], *d[3], *melk, *dnk, *pzsel, *dnsel;
    VbrCall *call;
    int *tok;                   // (B) the buckets of a capped call, behind `call`
    size_t floats;              // the frame buffers in front of `call` (cleared at the start of a call: padded rows hold zeros)
    size_t total;               // bytes in front of the ordinary workspace
};
void carve_vbr(const bvc_model *m, int B, int K, char *base, VbrWorkspace *v);
int run_encode_vbr(const bvc_model *m, const Workspace &w, const VbrWorkspace &v, void *ws_base, const float *d_mel, const float *d_tau,
                   const int *h_ladder, int K, const float *d_h0, int B, int64_t T, float *d_codes, float *d_bits, float *d_all_h,
                   float *d_hT, float *d_prob, float *d_dist, float *d_dec, hipStream_t s, const VbrCap *cap = nullptr);
// ---- entropy-coded wire format (bvc_bvrnn_entropy_pack / _unpack): its workspace is what the decode node of a frame holds - the coder's
// state per row and the call's stream, whose size depends on B alone - FOLLOWED by the ordinary workspace of (B, T) and, behind that, the
// prior's probabilities of all frames (B,T,z_dim): every address a captured step holds is a function of (base, B)
struct EntropyWorkspace {
    unsigned *state;            // [B][4]
    EntropyCall *call;
    size_t total;               // bytes in front of the ordinary workspace
    size_t prob_bytes;          // bytes behind it
};
void carve_entropy(const bvc_model *m, int B, int64_t T, char *base, EntropyWorkspace *e);
// The receive program: bvc_bvrnn_decode_conceal's step with every frame's codes decoded from the stream inside the frame.  d_sel (B,T):
// the bit count of every frame, not below 0 (launch_entropy_bits).  Always the launch-per-layer schedule.
int run_entropy_unpack(const bvc_model *m, const Workspace &w, const EntropyWorkspace &e, void *ws_base, const EntropyCall &call,
                       const float *d_sel, const float *d_h0, int B, int64_t T, float *d_codes, float *d_mel, float *d_hT, float *d_prior,
                       hipStream_t s);
struct ForwardTapeSpec;         // (below, with the backward pass)
int run_forward(const bvc_model *m, const Workspace &w, const float *d_mel, const float *d_bits, const uint8_t *h_use_gen, bool update_h,
                bool update_h2, const float *d_noise, int B, int64_t T, float *d_dec, float *d_kld, float *d_z, float *d_prob,
                float *d_prior, hipStream_t s, const ForwardTapeSpec *tape = nullptr);
int forward_tape_phi_x(const bvc_model *m, const Workspace &w, int B, int64_t T, float *p1, float *p2, float *p3, hipStream_t s);
// Where run_forward keeps every frame for the backward pass: the FORWARD_TAPE_SLOTS scratch vectors of frame t at steps + (t * SLOTS + k) *
// slot (fragment-packed, in the order of Workspace::step: e1 e2 pz1 pz2 pz3 d1 d2 d3 dn g1 g2 g3 q1 q2), and the two GRU chains as T + 1
// fragment-packed [mt16][H] matrices each, zeroed by the caller: [t] the state frame t starts from.  With a tape, d_z / d_prob / d_prior
// are the caller's (the workspace buffers they fall back to hold phi_x's hidden layers, which the backward pass reads).
enum { FORWARD_TAPE_SLOTS = 14 };
struct ForwardTapeSpec { float *steps; size_t slot; float *state[2]; };
// ---- the backward pass of run_forward (backward.hip): its workspace is the ordinary one of (B, T) FOLLOWED by the tape and the gradients
size_t backward_extra_bytes(const bvc_model *m, int B, int64_t T);
int backward_prepare(const bvc_model *m, hipStream_t s);
struct BackwardCall {
    const float *d_mel, *d_bits; const uint8_t *h_use_gen; bool update_h, update_h2; const float *d_noise; int B; int64_t T;
    const float *d_gdec; float g_kld;
    float *d_grads, *d_gmel, *d_dec, *d_kld, *d_z, *d_prob, *d_prior;
};
int run_backward(const bvc_model *m, const Workspace &w, char *extra, const BackwardCall &c, hipStream_t s);
// the layout of d_grads: entry i is tensor `name` (state-dict key) of `numel` floats at float offset `offset`; returns the entry count
struct GradEntry { const char *name; long long offset, numel; };
int grad_layout(const bvc_config &c, GradEntry *out, long long *total);
enum { GRAD_ENTRIES = 36 };
int run_vocoder(const bvc_model *m, const Workspace &w, const float *d_mel, int B, int64_t T, int64_t length, float div, float *d_wav,
                int stop_after, const float **tap, int64_t *tap_len, int *tap_ch, hipStream_t s, const long long *lim = nullptr,
                int64_t *tap_bs = nullptr);     // tap_bs: floats between the tap's batch items (a symmetric stage works on a view)

int copy_rows(const float *src, long long src_bs, float *dst, long long dst_bs, long long n, int B, hipStream_t s);   // generator.hip

const int64_t STREAM_WARM_FRAMES = 32;   // rate * 32 - 64 >= 60 = the longest receptive field of an AMP pair, for every stage rate >= 8
const int STREAM_H = 64;     // history rows per stage: >= (ks-1)*dil + (ks-1) of every AMP pair (max 60) and a multiple of every rate
int vocoder_stream_create(const bvc_model *m, int32_t B, int32_t max_frames_per_push, bool slide, bvc_vocoder_stream **out, bool lookahead = false);

}  // namespace bvc
