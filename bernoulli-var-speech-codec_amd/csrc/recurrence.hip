// The drivers of the BVRNN recurrence - encode, the closed-loop rates, decode, the concealing decoder and the training-time forward
// pass - with the all-frame prologues in front of the recurrence and the epilogue behind it.  The launch-per-layer schedule they run is
// step_plan.hip, the persistent kernel's host side flow_launch.hip.
#include "recurrence.h"

using namespace bvc;

namespace {

constexpr int64_t SMALL_T_FRAMES = 4;          // up to this many frames per call the all-frame MLPs run frame by frame on the recurrent-layer kernel

}  // namespace

namespace bvc {

thread_local bool g_stream_tick = false;
thread_local bool g_tick_flow = false;

// dec.6 over the kept u = ELU(dec.4) of all frames (the folded hop): the decoder's output mel^ (bvrnn.py:224-225)
int decode_epilogue(const bvc_model *m, const float *keep, int B, int64_t T, float *d_mel, hipStream_t s) {
    const int H = m->cfg.h_dim, X = m->cfg.num_mels;
    const int BT = (int)((long long)B * T);
    if (T <= SMALL_T_FRAMES)
        return launch_gemm_skinny(lin_params(m->dec[3], dp_static(keep, H), BT, dp_static(d_mel, X)), EPI_LINEAR, s, m->mtw);
    return launch_gemm_batched(keep, H, m->dec[3].w, H, m->dec[3].b, BT, X, H, 0, d_mel, X, s);
}

}  // namespace bvc

namespace {

// one launch of the recurrent-layer kernel over all T frames of a call: the frame is the grid's second dimension
int launch_frames(const bvc_model *m, GemmParams p, int epi, int64_t T, hipStream_t s) {
    p.frames = (int)T;
    return launch_gemm_skinny(p, epi, s, m->mtw);
}

// Three-layer ELU MLP over ALL frames (phi_x at bvrnn.py:178, phi_z at bvrnn.py:223): in (B*T rows of K0, utterance-major).  The
// last layer's result goes to pxA, one fragment-packed [mt16][H] matrix per frame (MLP3_PACKED: the step kernels read it), or to pxC,
// natural (B,T,H) (MLP3_NATURAL: a batched projection follows).  Up to SMALL_T_FRAMES frames it is packed in pxA in both modes.
// (Re-ordering the rows frame-major in the first layer, so that the last one writes whole 1 KiB blocks - GO_FRAME_MAJOR_ROWS /
// GO_PACKED_FRAMES - measured 0.3 ms per step SLOWER: the first layer's row scatter costs more than the last layer's 16-byte granules.)
enum { MLP3_PACKED = 0, MLP3_NATURAL = 1 };
int mlp3_frames(const bvc_model *m, const Workspace &w, const Linear (&l)[3], const float *in, int K0, int B, int64_t T, int last,
                hipStream_t s) {
    const int H = m->cfg.h_dim;
    const int mt16 = pad16(B);
    const int BT = (int)((long long)B * T);
    int rc;
    if (T <= SMALL_T_FRAMES) {
        // a streaming hop (1-2 frames): B*T rows fill a handful of the batched kernel's 128x128 tiles (102 us per 1024^2
        // layer at 256 streams); the recurrent-layer kernel takes the rows of ONE frame (row stride T*K0) in 10 us and
        // writes the fragment-packed frame matrix directly.  Same bits either way (one order of summation: k_gemm.hip).
        const long long FS = (long long)mt16 * H;
        const DynPtr a = dp_static_frames(w.pxA, H, FS, 1), b = dp_static_frames(w.pxB, H, FS, 1), c = dp_static_frames(w.pxC, H, FS, 1);
        if ((rc = launch_frames(m, lin_params(l[0], dp_static_frames(in, T * K0, K0), B, c), EPI_ELU, T, s))) return rc;
        if ((rc = launch_frames(m, lin_params(l[1], c, B, b), EPI_ELU, T, s))) return rc;
        return launch_frames(m, lin_params(l[2], b, B, a), EPI_ELU, T, s);
    }
    const bool packed = last == MLP3_PACKED;
    if ((rc = launch_gemm_batched(in, K0, l[0].w, K0, l[0].b, BT, H, K0, 1, w.pxC, H, s))) return rc;
    if ((rc = launch_gemm_batched(w.pxC, H, l[1].w, H, l[1].b, BT, H, H, 1, w.pxB, H, s))) return rc;
    return launch_gemm_batched(w.pxB, H, l[2].w, H, l[2].b, BT, H, H, 1, packed ? w.pxA : w.pxC, H, s,
                               packed ? GO_PACKED_FROM_UTT : GO_NATURAL, packed ? T : 0, packed ? mt16 : 0);
}

// l[:, :H] x + b for all frames -> w.part_dec0, natural (B,T,H): x = what mlp3_frames(.., MLP3_NATURAL) left, l = enc.0 or dec.0
int first_half_frames(const bvc_model *m, const Workspace &w, const Linear &l, int B, int64_t T, hipStream_t s) {
    const int H = m->cfg.h_dim;
    if (T <= SMALL_T_FRAMES) {
        const DynPtr x = dp_static_frames(w.pxA, H, (long long)pad16(B) * H, 1);
        return launch_frames(m, half_params(l, 0, x, H, B, dp_static_frames(w.part_dec0, T * H, H), true), EPI_LINEAR, T, s);
    }
    return launch_gemm_batched(w.pxC, H, l.w, 2 * H, l.b, (int)((long long)B * T), H, H, 0, w.part_dec0, H, s);
}

// Everything of BVRNN.encode that does not depend on the recurrence, for all frames: phi_x(yn) (bvrnn.py:178) and the phi_x half of
// enc.0 with its bias (bvrnn.py:189) -> w.part_dec0.
int encode_prologue(const bvc_model *m, const Workspace &w, int B, int64_t T, hipStream_t s) {
    if (int rc = mlp3_frames(m, w, m->phi_x, w.yn, m->cfg.num_mels, B, T, MLP3_NATURAL, s)) return rc;
    return first_half_frames(m, w, m->enc[0], B, T, s);
}

// ... and of BVRNN.decode (the codes are known): phi_z(z) (bvrnn.py:223), the phi_z half of dec.0 with its bias (bvrnn.py:224) ->
// w.part_dec0, and the phi_z half of the GRU's input gates with b_ih (bvrnn.py:227) -> w.part_gru (B,T,3H).
int decode_prologue(const bvc_model *m, const Workspace &w, const float *d_codes, int B, int64_t T, hipStream_t s) {
    const int H = m->cfg.h_dim;
    int rc;
    if ((rc = mlp3_frames(m, w, m->phi_z, d_codes, m->cfg.z_dim, B, T, MLP3_NATURAL, s))) return rc;
    if ((rc = first_half_frames(m, w, m->dec[0], B, T, s))) return rc;
    if (T <= SMALL_T_FRAMES) {
        const DynPtr pz = dp_static_frames(w.pxA, H, (long long)pad16(B) * H, 1);
        return launch_frames(m, mat_params(pz, m->w_ih + (size_t)(H / 16) * 256, 2 * H / 16, H, B, 3 * H, m->b_ih, dp_static_frames(w.part_gru, T * 3 * H, 3 * H)),
                             EPI_LINEAR, T, s);
    }
    return launch_gemm_batched(w.pxC, H, m->w_ih_nat + H, 2 * H, m->b_ih, (int)((long long)B * T), 3 * H, H, 0, w.part_gru, 3 * H, s);
}

// The launch-per-layer schedule of one call, from the initial state to the final one: T frames of the step `plan` (graph-cache key
// `kind`) over the descriptor `d`, whose slots the caller has filled.  all_h[:, 0] = h0 where the call returns the states (DS_ALLH).
// mel_out (folded hop only): the step kept u = ELU(dec.4) of every frame in w.pxB; dec.6(u), the decoder's output, goes there for all
// frames at once.
int run_layers(const bvc_model *m, const Workspace &w, void *ws_base, CallDesc &d, const std::vector<StepNode> &plan, int kind,
               const float *d_h0, int B, int64_t T, float *d_hT, float *mel_out, hipStream_t s) {
    const int H = m->cfg.h_dim;
    const long long MH = (long long)pad16(B) * H;
    int rc;
    // the GRU state lives fragment-packed in hbuf[parity of the frame counter]; h0 (or zero) goes to parity 0
    if ((rc = d_h0 ? launch_repack_rows(d_h0, w.hbuf, H, B, H, 0, s) : launch_fill(w.hbuf, 0.0f, MH, s))) return rc;
    if (d.p[DS_ALLH] && (rc = launch_repack_rows(w.hbuf, d.p[DS_ALLH], (long long)T * H, B, H, 1, s))) return rc;
    d.T = T;
    if ((rc = begin_call(m, w, d, count_kernels(plan), g_kprobe.enabled, s))) return rc;
    if ((rc = run_recurrence(m, w, ws_base, B, T, kind, plan, s))) return rc;
    if (d_hT && (rc = launch_repack_rows(w.hbuf + (T & 1) * MH, d_hT, H, B, H, 1, s))) return rc;
    if (mel_out && (rc = decode_epilogue(m, w.pxB, B, T, mel_out, s))) return rc;
    return BVC_OK;
}

// A recurrence-bearing call: its body, then the end-of-call mark (also when the body failed); the first non-zero code is the call's.
template <typename Body>
int end_call(hipStream_t s, Body body) {
    const int rc = body();
    const int rc2 = mark_call_end(s);
    return rc ? rc : rc2;
}

// Where the decoder's output of a launch-per-layer call goes.  Unfolded: dec.6 writes every frame to `mel` (DS_MEL).  Folded hop: the
// step keeps u = ELU(dec.4) of every frame in w.pxB through `keep_slot` (idle once the batched layers are through) and dec.6 follows
// behind the recurrence: returns run_layers' mel_out.
float *route_decoder_output(CallDesc &d, const Workspace &w, int kind, int keep_slot, float *mel) {
    const bool fold = (kind & STEP_FOLD) != 0;
    if (fold) d.p[keep_slot] = w.pxB;
    else d.p[DS_MEL] = mel;
    return fold ? mel : nullptr;
}

}  // namespace

namespace bvc {

// d_melhat (optional): the decoder's output dec(phi_z(z_t), h_t) of every frame (B,T,num_mels) - what BVRNN.decode(codes) would compute over again
// from the same trajectory (bvrnn.py:202 vs :224-225; the fused forward, bvc_forward)
int run_encode(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_mel, const float *d_bits,
               const float *d_h0, int B, int64_t T, float *d_codes, float *d_all_h, float *d_hT, float *d_prob,
               hipStream_t s, float *d_melhat) {
    return end_call(s, [&]() -> int {
        int rc;
        if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
        // y = (y - mean) / std ; phi_x over all frames (bvrnn.py:173-178)
        if ((rc = launch_normalize_rows(d_mel, m->mean_mel, m->std_mel, (long long)B * T, m->cfg.num_mels, w.yn, s))) return rc;
        const int chains = flow_chains(m, B, s);
        if ((rc = encode_prologue(m, w, B, T, s))) return rc;
        if (chains) return run_flow(m, w, true, chains, d_h0, B, T, d_bits, d_codes, d_prob, d_all_h, d_melhat, d_hT, s);
        CallDesc d;
        memset(&d, 0, sizeof(d));
        d.p[DS_PARTD] = w.part_dec0; d.p[DS_CODES] = d_codes; d.p[DS_BITS] = const_cast<float *>(d_bits);
        d.p[DS_PROB] = d_prob; d.p[DS_ALLH] = d_all_h;
        const int kind = STEP_ENCODE | step_fold(m, true);
        float *mel_out = d_melhat ? route_decoder_output(d, w, kind, DS_KEEP_ENC, d_melhat) : nullptr;      // (no mel^ wanted: both slots stay null)
        return run_layers(m, w, ws_base, d, build_step(m, w, B, kind), kind, d_h0, B, T, d_hT, mel_out, s);
    });
}

void carve_vbr(const bvc_model *m, int B, int K, char *base, VbrWorkspace *v) {
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float *p = reinterpret_cast<float *>(base + off);
        off += (nfloats * sizeof(float) + 255) / 256 * 256;
        return p;
    };
    const size_t mb = (size_t)pad16(B), mk = (size_t)pad16(K * B);
    v->zraw = take(mb * Z);
    v->zc = take(mk * Z);
    v->hrep = take(mk * H);
    for (int i = 0; i < 3; ++i) v->pz[i] = take(mk * H);
    for (int i = 0; i < 3; ++i) v->d[i] = take(mk * H);
    v->melk = take(mk * X);
    v->dnk = take(mk * X);
    v->pzsel = take(mb * H);
    v->dnsel = take(mb * X);
    v->floats = off / sizeof(float);
    v->call = reinterpret_cast<VbrCall *>(take((sizeof(VbrCall) + 3) / 4));
    v->tok = reinterpret_cast<int *>(take((size_t)B));
    v->total = off;
}

// BVRNN.encode with the bits of every frame chosen inside the frame (build_vbr_step).  Always the launch-per-layer schedule, whatever
// `recurrence` says: the persistent kernel has no candidate rows.  h_ladder: K ascending bit counts, checked by the caller.  cap (null
// or capped == 0: none): the token bucket of the selection, the rows' buckets from cap->tok0 (null: full) and back to cap->tokT.
int run_encode_vbr(const bvc_model *m, const Workspace &w, const VbrWorkspace &v, void *ws_base, const float *d_mel, const float *d_tau,
                   const int *h_ladder, int K, const float *d_h0, int B, int64_t T, float *d_codes, float *d_bits, float *d_all_h,
                   float *d_hT, float *d_prob, float *d_dist, float *d_dec, hipStream_t s, const VbrCap *cap) {
    return end_call(s, [&]() -> int {
        int rc;
        const bool capped = cap && cap->capped;
        if ((rc = launch_normalize_rows(d_mel, m->mean_mel, m->std_mel, (long long)B * T, m->cfg.num_mels, w.yn, s))) return rc;
        if ((rc = encode_prologue(m, w, B, T, s))) return rc;
        if ((rc = launch_fill(v.zraw, 0.0f, (long long)v.floats, s))) return rc;      // rows of a fragment behind the last candidate read as zeros
        VbrCall c;
        memset(&c, 0, sizeof(c));
        c.y = d_mel; c.tau = d_tau; c.codes = d_codes; c.bits = d_bits; c.dist = d_dist; c.dec = d_dec;
        for (int k = 0; k < K; ++k) c.ladder[k] = h_ladder[k];
        if (capped) {
            c.capped = 1; c.rate_q8 = cap->rate_q8; c.burst_q8 = cap->burst_q8; c.tok = v.tok;
            if ((rc = launch_vbr_tok(v.tok, cap->tok0, cap->burst_q8, B, s))) return rc;
        }
        if ((rc = launch_vbr_set_call(v.call, c, s))) return rc;
        CallDesc d;
        memset(&d, 0, sizeof(d));
        d.p[DS_PARTD] = w.part_dec0; d.p[DS_PROB] = d_prob; d.p[DS_ALLH] = d_all_h;
        if ((rc = run_layers(m, w, ws_base, d, build_vbr_step(m, w, v, B, K), STEP_ENCODE_VBR | (K << STEP_RUNGS_SHIFT), d_h0, B, T, d_hT, nullptr, s)))
            return rc;
        return capped ? launch_vbr_tok(cap->tokT, v.tok, 0, B, s) : BVC_OK;
    });
}

int run_decode(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_codes, const float *d_h0, int B,
               int64_t T, float *d_mel, float *d_hT, hipStream_t s) {
    return end_call(s, [&]() -> int {
        int rc;
        CallDesc d;
        memset(&d, 0, sizeof(d));
        const int chains = flow_chains(m, B, s);
        const bool pre = chains > 0 || m->precomp_pz;     // (BVC_NO_PRECOMP=1: the round-1 step with both halves inside, another order of summation)
        if (pre) {
            // phi_z depends on the codes only: all frames at once, outside the recurrence (bvrnn.py:223), and so do the phi_z halves of
            // dec.0 (bvrnn.py:224) and of the GRU's input product (bvrnn.py:227)
            if ((rc = decode_prologue(m, w, d_codes, B, T, s))) return rc;
            d.p[DS_PARTD] = w.part_dec0; d.p[DS_PARTG] = w.part_gru;
            if (chains) return run_flow(m, w, false, chains, d_h0, B, T, nullptr, nullptr, nullptr, nullptr, d_mel, d_hT, s);
        } else {
            if ((rc = mlp3_frames(m, w, m->phi_z, d_codes, m->cfg.z_dim, B, T, MLP3_PACKED, s))) return rc;
            d.p[DS_PZ] = w.pxA;
        }
        const int kind = (pre ? STEP_DECODE_PRE : STEP_DECODE) | step_fold(m, false);
        d.p[DS_MEL] = d_mel;                              // (also when folded, where no kernel of the step reads it)
        float *mel_out = route_decoder_output(d, w, kind, DS_KEEP, d_mel);
        return run_layers(m, w, ws_base, d, build_step(m, w, B, kind), kind, d_h0, B, T, d_hT, mel_out, s);
    });
}

// ---- the concealing decoder (bvc_bvrnn_decode_conceal) -------------------------------------------------
// BVRNN.decode in which a frame that did not arrive is generated from the prior net (bvrnn.py:68-73) at the decoder's own state.  d_sel
// (B,T): the selector (launch_conceal_select).  The frame's codes are only known inside the frame, so nothing is batched beforehand: the
// program is encode's from the code epilogue on (dec.0 and the GRU's input gates sum their h half before their phi_z half), on every
// schedule - a call that conceals runs it on all its frames, lost or not, so its result does not depend on where the losses are cut.
int run_decode_conceal(const bvc_model *m, const Workspace &w, void *ws_base, const float *d_codes, const float *d_sel, const float *d_h0,
                       int B, int64_t T, float *d_mel, float *d_hT, float *d_codes_out, float *d_prior, hipStream_t s) {
    return end_call(s, [&]() -> int {
        if (m->cfg.z_dim > 3 * m->cfg.h_dim) { set_error("bvc_bvrnn_decode_conceal: z_dim > 3 h_dim is not supported"); return BVC_EINVAL; }
        float *codes = d_codes_out ? d_codes_out : w.part_gru;        // the filled codes feed phi_z: nobody's output goes to a tensor this program does not use
        const int chains = flow_chains(m, B, s);
        if (chains) return run_flow(m, w, true, chains, d_h0, B, T, d_sel, codes, d_prior, nullptr, d_mel, d_hT, s, d_codes);
        CallDesc d;
        memset(&d, 0, sizeof(d));
        d.p[DS_CODES] = codes; d.p[DS_BITS] = const_cast<float *>(d_sel); d.p[DS_PROB] = d_prior; d.p[DS_NOISE] = const_cast<float *>(d_codes);
        const int kind = STEP_CONCEAL | step_fold(m, false);
        float *mel_out = route_decoder_output(d, w, kind, DS_KEEP_ENC, d_mel);
        return run_layers(m, w, ws_base, d, build_step(m, w, B, kind), kind, d_h0, B, T, d_hT, mel_out, s);
    });
}

// ---- the entropy-coded wire's receive program (bvc_bvrnn_entropy_unpack) -------------------------------
void carve_entropy(const bvc_model *m, int B, int64_t T, char *base, EntropyWorkspace *e) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    e->state = reinterpret_cast<unsigned *>(base);
    e->call = reinterpret_cast<EntropyCall *>(base + up((size_t)B * 4 * sizeof(unsigned)));
    e->total = up((size_t)B * 4 * sizeof(unsigned)) + up(sizeof(EntropyCall));
    e->prob_bytes = up((size_t)B * (size_t)T * m->cfg.z_dim * sizeof(float));
}

// The concealing step with one node more (build_step, STEP_ENTROPY): prior.{0,2,4} and the code epilogue are the concealing call's own
// launches, so p_t is the number the sender coded under; the node decodes z_t from the stream and phi_z goes on from it.  The decoder
// needs p_t of every frame, so where the caller wants no d_prior it goes to the tail of the workspace.
int run_entropy_unpack(const bvc_model *m, const Workspace &w, const EntropyWorkspace &e, void *ws_base, const EntropyCall &call,
                       const float *d_sel, const float *d_h0, int B, int64_t T, float *d_codes, float *d_mel, float *d_hT, float *d_prior,
                       hipStream_t s) {
    return end_call(s, [&]() -> int {
        int rc;
        if ((rc = launch_entropy_set_call(e.call, call, s))) return rc;
        CallDesc d;
        memset(&d, 0, sizeof(d));
        d.p[DS_CODES] = d_codes ? d_codes : w.part_gru;
        d.p[DS_BITS] = const_cast<float *>(d_sel);
        d.p[DS_PROB] = d_prior ? d_prior : reinterpret_cast<float *>(static_cast<char *>(ws_base) + e.total + w.total);
        const int kind = STEP_ENTROPY | step_fold(m, false);
        float *mel_out = route_decoder_output(d, w, kind, DS_KEEP_ENC, d_mel);
        const EntropyStep es{w.desc, e.call, e.state, B, m->cfg.z_dim};
        return run_layers(m, w, ws_base, d, build_step(m, w, B, kind, &es), kind, d_h0, B, T, d_hT, mel_out, s);
    });
}

int run_forward(const bvc_model *m, const Workspace &w, const float *d_mel, const float *d_bits,
                const uint8_t *h_use_gen, bool update_h, bool update_h2, const float *d_noise, int B, int64_t T,
                float *d_dec, float *d_kld, float *d_z, float *d_prob, float *d_prior, hipStream_t s, const ForwardTapeSpec *tape) {
    const int H = m->cfg.h_dim, X = m->cfg.num_mels, Z = m->cfg.z_dim;
    const long long BT = (long long)B * T;
    int rc;
    if (!m->has_prior) { set_error("bvc_bvrnn_forward: the model was created without the prior.* tensors"); return BVC_EMISSING; }
    if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
    if (Z > H) { set_error("bvc_bvrnn_forward: z_dim > h_dim is not supported"); return BVC_EINVAL; }
    // y = (y - mean) / std ; phi_x over all frames (bvrnn.py:96-101)
    if ((rc = launch_normalize_rows(d_mel, m->mean_mel, m->std_mel, BT, X, w.yn, s))) return rc;
    if ((rc = mlp3_frames(m, w, m->phi_x, w.yn, X, B, T, MLP3_PACKED, s))) return rc;
    // h = h2 = 0 (bvrnn.py:103-104); both parities so that a state that is never updated stays zero
    const long long MH = (long long)pad16(B) * H;
    if ((rc = launch_fill(w.hbuf, 0.0f, 2 * MH, s))) return rc;
    if ((rc = launch_fill(w.part_i, 0.0f, 2 * MH, s))) return rc;
    // optional outputs fall back to workspace buffers that are idle during the recurrence (Z <= H, Z <= num_mels or not:
    // pxB / pxC hold B*T*H floats each, mel B*T*num_mels)
    float *prob = d_prob ? d_prob : w.pxB;
    float *prior = d_prior ? d_prior : w.pxC;
    float *z = d_z ? d_z : (Z <= X ? w.mel : w.pxB + BT * Z);
    if (!d_z && Z > X && 2 * Z > H) { set_error("bvc_bvrnn_forward: pass d_z for this z_dim"); return BVC_EINVAL; }
    CallDesc d;
    memset(&d, 0, sizeof(d));
    d.p[DS_PX] = w.pxA; d.p[DS_CODES] = z; d.p[DS_BITS] = const_cast<float *>(d_bits);
    d.p[DS_PROB] = prob; d.p[DS_PRIOR] = prior; d.p[DS_MEL] = d_dec; d.p[DS_NOISE] = const_cast<float *>(d_noise);
    d.T = T;
    const bool greedy = d_noise == nullptr;
    const std::vector<StepNode> plan0 = build_forward_step(m, w, B, 0, greedy, update_h, update_h2);
    const std::vector<StepNode> plan1 = build_forward_step(m, w, B, 1, greedy, update_h, update_h2);
    rc = begin_call(m, w, d, count_kernels(plan0), false, s);      // no probes: they index by a fixed kernel count per step
    if (!tape)
        for (int64_t t = 0; !rc && t < T; ++t) rc = launch_steps(m, h_use_gen[t] ? plan1 : plan0, w, 1, s, nullptr);
    // the backward pass's forward: the same launches, every frame into scratch vectors and state matrices of its own
    for (int64_t t = 0; tape && !rc && t < T; ++t) {
        Workspace wt = w;
        for (int k = 0; k < FORWARD_TAPE_SLOTS; ++k) wt.step[k] = tape->steps + ((size_t)t * FORWARD_TAPE_SLOTS + k) * tape->slot;
        const ForwardTape ft = {{tape->state[0] + t * MH, tape->state[1] + t * MH}, {tape->state[0] + (t + 1) * MH, tape->state[1] + (t + 1) * MH}};
        rc = launch_steps(m, build_forward_step(m, wt, B, h_use_gen[t], greedy, update_h, update_h2, &ft), wt, 1, s, nullptr);
    }
    if (rc) return rc;
    return launch_kld_frames(prob, prior, m->cfg.var_bit ? d_bits : nullptr, B, T, Z, d_kld, s);
}

// phi_x.0 / .2 / .4 of all frames, as run_forward's prologue left them (mlp3_frames, MLP3_PACKED), as natural matrices with frame-major
// rows t * B + b: p1, p2, p3 (T B, H)
int forward_tape_phi_x(const bvc_model *m, const Workspace &w, int B, int64_t T, float *p1, float *p2, float *p3, hipStream_t s) {
    const int H = m->cfg.h_dim;
    const long long FS = (long long)pad16(B) * H;
    int rc;
    if ((rc = launch_unpack_frames(w.pxA, FS, T, B, H, p3, s))) return rc;
    if (T <= SMALL_T_FRAMES) {
        if ((rc = launch_unpack_frames(w.pxC, FS, T, B, H, p1, s))) return rc;
        return launch_unpack_frames(w.pxB, FS, T, B, H, p2, s);
    }
    if ((rc = launch_reorder_rows(w.pxC, B, T, H, p1, 0, nullptr, s))) return rc;
    return launch_reorder_rows(w.pxB, B, T, H, p2, 0, nullptr, s);
}

}  // namespace bvc
