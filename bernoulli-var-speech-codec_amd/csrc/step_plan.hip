// The launch-per-layer schedule of the BVRNN recurrence: the operation sequence of one frame (one builder, three plans), its launch,
// the hipGraph cache with its replay, and the per-call descriptor.
#include "recurrence.h"

using namespace bvc;

namespace {

enum { EV_START = 0, EV_DEC0H = 1, EV_PZ = 2, EV_GATES = 3, EV_COUNT = 4 };

// What every plan is written over: the model, the workspace and the batch, the plan with its node counter, whether its kernels carry
// probes, the GRU state by frame parity and the named scratch vectors.  A layer group is stated once, as a member that takes its
// operands and its row count.  A group of more than one K-segment takes its segments in the order of the caller: the order of the
// segments is the order of summation, and the plans differ in it.  Internal activations are kept in MFMA fragment order (S: packed = 1)
// so every operand load is a coalesced 1 KiB read.
struct StepBuilder {
    const bvc_model *m;
    const Workspace &w;
    const int B;
    const bool probes;
    const int H, Z, X;
    const long long MH;
    std::vector<StepNode> plan;
    int node = 0;
    float *const e1, *const e2, *const pz1, *const pz2, *const pz3, *const d1, *const d2, *const d3, *const dn, *const g1, *const g2,
        *const g3, *const q1, *const q2;

    StepBuilder(const bvc_model *m_, const Workspace &w_, int B_, bool probes_)
        : m(m_), w(w_), B(B_), probes(probes_), H(m_->cfg.h_dim), Z(m_->cfg.z_dim), X(m_->cfg.num_mels), MH((long long)pad16(B_) * H),
          e1(w_.step[0]), e2(w_.step[1]), pz1(w_.step[2]), pz2(w_.step[3]), pz3(w_.step[4]), d1(w_.step[5]), d2(w_.step[6]), d3(w_.step[7]),
          dn(w_.step[8]), g1(w_.step[9]), g2(w_.step[10]), g3(w_.step[11]), q1(w_.step[12]), q2(w_.step[13]) {}

    static DynPtr S(float *p, int ld) { return dp_static(p, ld, 1); }
    // a GRU state ping-pongs in [2][mt16][H] by frame parity: this frame's and the next one's
    DynPtr h_cur(float *buf) const { return dp_parity(buf, H, MH, 0, 1); }
    DynPtr h_next(float *buf) const { return dp_parity(buf + MH, H, -MH, 0, 1); }

    void K(GemmParams p, int epi, int branch = BR_MAIN) {
        p.desc = w.desc; p.node = node++;
        p.probe = probes ? g_kprobe.dev : nullptr;
        finish(p);
        plan.push_back(StepNode{OP_KERNEL, branch, -1, p, epi});
    }
    // out = ELU(l(in)) over M rows
    void elu(const Linear &l, DynPtr in, int M, float *out) { K(lin_params(l, in, M, S(out, H)), EPI_ELU); }

    // the encoder's first two layers: enc.0([phi_x, h]) = (enc.0[:, :H] phi_x + b) [all frames beforehand: encode_prologue] + enc.0[:, H:] h,
    // as in the persistent kernel; enc.2
    void enc02(DynPtr h) {
        GemmParams p = half_params(m->enc[0], H / 16, h, H, B, S(e1, H), false);
        p.aux = dp_frame(DS_PARTD, H);
        K(p, EPI_ELU);
        elu(m->enc[1], S(e1, H), B, e2);
    }
    // phi_z.0-4 from `in` over M rows
    void phi_z(DynPtr in, int M, float *a, float *b, float *out) {
        elu(m->phi_z[0], in, M, a);
        elu(m->phi_z[1], S(a, H), M, b);
        elu(m->phi_z[2], S(b, H), M, out);
    }
    // dec.0 over the concatenation [phi_z, h] as two K-segments, summed in the order given
    GemmSeg dec0_z(DynPtr pz) const { return mkseg(pz, m->dec[0].wp, 2 * H / 16, H, 0); }
    GemmSeg dec0_h(DynPtr h) const { return mkseg(h, m->dec[0].wp + (size_t)(H / 16) * 256, 2 * H / 16, H, 0); }
    void dec0(GemmSeg s0, GemmSeg s1, int M, float *out) {
        GemmParams p = lin_params(m->dec[0], s0.x, M, S(out, H));
        p.nseg = 2;
        p.seg[0] = s0; p.seg[1] = s1;
        K(p, EPI_ELU);
    }
    // dec.2 / dec.4; keep (folded hop): u = ELU(dec.4) also goes to a tensor of all frames
    void dec24(float *in, int M, float *mid, float *out, DynPtr keep = dp_null()) {
        elu(m->dec[1], S(in, H), M, mid);
        GemmParams p = lin_params(m->dec[2], S(mid, H), M, S(out, H));
        p.y2 = keep;
        K(p, EPI_ELU);
    }
    // dec.6 with the mel epilogue: the decoder's output to `mel`, normalised to `norm`
    void dec6(float *in, int M, DynPtr mel, float *norm) {
        GemmParams p = lin_params(m->dec[3], S(in, H), M, mel);
        p.y2 = S(norm, X); p.mean = m->mean_mel; p.stdv = m->std_mel;
        K(p, EPI_MEL);
    }
    // phi_x.2 / phi_x.4 behind phi_x.0 (or the folded layer) in g1
    void phi_x24() {
        elu(m->phi_x[1], S(g1, H), B, g2);
        elu(m->phi_x[2], S(g2, H), B, g3);
    }
    // The GRU cell on the state in `hbuf`: everything but the segments.  all_h: all_h[:, t+1] (bvrnn.py:205), or null
    GemmParams gru_cell(DynPtr h_in, DynPtr h_out, DynPtr all_h) const {
        GemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = B; p.N = H; p.gate_rows = H;
        p.y = h_out;
        p.y2 = all_h;
        p.aux = h_in;
        return p;
    }
    GemmParams gru_cell(float *hbuf, DynPtr all_h) const { return gru_cell(h_cur(hbuf), h_next(hbuf), all_h); }
    // ... as one launch over cat([phi_x, phi_z]) (bvrnn.py:206) and h: three gate-interleaved K-segments, summed in the order given
    GemmSeg gru_x(DynPtr px) const { return mkseg(px, m->w_ih_il, 2 * H / 16, H, 0); }
    GemmSeg gru_z(DynPtr pz) const { return mkseg(pz, m->w_ih_il + (size_t)(H / 16) * 3 * 256, 2 * H / 16, H, 0); }
    GemmSeg gru_h(DynPtr h) const { return mkseg(h, m->w_hh_il, H / 16, H, 1); }
    void gru(GemmSeg s0, GemmSeg s1, GemmSeg s2, float *hbuf, DynPtr all_h) { gru(s0, s1, s2, h_cur(hbuf), h_next(hbuf), all_h); }
    void gru(GemmSeg s0, GemmSeg s1, GemmSeg s2, DynPtr h_in, DynPtr h_out, DynPtr all_h) {
        GemmParams p = gru_cell(h_in, h_out, all_h);
        p.nseg = 3;
        p.gate_il = 1;
        p.seg[0] = s0; p.seg[1] = s1; p.seg[2] = s2;
        p.bias0 = m->b_ih; p.bias1 = m->b_hh;
        K(p, EPI_GRU);
    }
};

}  // namespace

namespace bvc {

// The operation sequence of ONE frame.  Every pointer is either workspace-static, frame-indexed through
// the call descriptor, or parity-indexed (GRU state), so the same sequence serves every frame and
// every call: it is captured once into a hipGraph.
//   encode (bvrnn.py:187-206): enc -> sigmoid/round/mask -> phi_z -> dec -> phi_x(norm) -> GRU
//   decode (bvrnn.py:222-227): [phi_z batched over all frames beforehand] dec -> phi_x(norm) -> GRU
//   conceal (bvc_bvrnn_decode_conceal): prior -> sigmoid/round/mask, SELECTED against the received codes -> phi_z -> ... as encode
//   entropy (bvc_bvrnn_entropy_unpack): conceal's step, layer for layer, with the frame's range decoder behind the code epilogue: it
//     reads p_t (DS_PROB) and overwrites the frame's DS_CODES with the decoded bits, which phi_z then reads
//   closed-loop rates (bvc_bvrnn_encode_vbr): enc -> sigmoid/round -> K masked candidates -> phi_z -> dec on K * B rows -> select -> ... as encode
//     (build_vbr_step below; never folded: dec.6 must exist to be measured)
// Side branch: the halves of the split dot products that do not depend on the current frame's chain -
// dec.0[:, H:] h, W_hh h + b_hh, W_ih[:, H:] phi_z + b_ih - run concurrently with the chain (which is
// latency-bound), so the GRU kernel on the critical path only streams W_ih[:, :H].
std::vector<StepNode> build_step(const bvc_model *m, const Workspace &w, int B, int kind_and_fold, const EntropyStep *es) {
    const int kind = kind_and_fold & STEP_KIND_MASK;
    const bool fold = (kind_and_fold & STEP_FOLD) != 0;       // dec.6 -> norm -> phi_x.0 as one layer (bvc_model::px0_dec3)
    const bool conceal_like = kind == STEP_CONCEAL || kind == STEP_ENTROPY;
    const bool enc_like = kind == STEP_ENCODE || conceal_like;            // phi_z is computed inside the step
    StepBuilder b(m, w, B, g_kprobe.enabled);
    const int H = b.H, Z = b.Z, X = b.X;
    std::vector<StepNode> &plan = b.plan;
    const DynPtr h_cur = b.h_cur(w.hbuf);
    auto S = StepBuilder::S;
    const bool side = m->side_branch;
    auto REC = [&](int branch, int ev) { GemmParams z; memset(&z, 0, sizeof(z)); if (side) plan.push_back(StepNode{OP_RECORD, branch, ev, z, 0}); };
    auto WAIT = [&](int branch, int ev) { GemmParams z; memset(&z, 0, sizeof(z)); if (side) plan.push_back(StepNode{OP_WAIT, branch, ev, z, 0}); };
    // --- side-branch kernels (plain linears into natural [B][.] partial buffers)
    // dec.0.weight[:, H:] @ h (no bias: added on the main branch); W_hh @ h + b_hh; W_ih[:, H:] @ phi_z + b_ih
    auto side_dec0h = [&]() { b.K(half_params(m->dec[0], H / 16, h_cur, H, B, dp_static(w.part_d, H), false), EPI_LINEAR, BR_SIDE); };
    auto side_hh = [&]() { b.K(mat_params(h_cur, m->w_hh, H / 16, H, B, 3 * H, m->b_hh, dp_static(w.part_h, 3 * H)), EPI_LINEAR, BR_SIDE); };
    auto side_ihz = [&](DynPtr pz) {
        b.K(mat_params(pz, m->w_ih + (size_t)(H / 16) * 256, 2 * H / 16, H, B, 3 * H, m->b_ih, dp_static(w.part_i, 3 * H)), EPI_LINEAR, BR_SIDE);
    };

    DynPtr pz_final = enc_like ? S(b.pz3, H) : dp_frame(DS_PZ, H, 0, 1);
    if (conceal_like) {
        // p_t = prior(h_t) (bvrnn.py:68-73): no pre-computed half, the first layer's bias is its own; the code epilogue SELECTS between the
        // received codes (DS_NOISE carries them) and the generated bits, by the selector in DS_BITS; p_t goes to DS_PROB
        b.elu(m->prior[0], h_cur, B, b.e1);
        b.elu(m->prior[1], S(b.e1, H), B, b.e2);
        GemmParams p = lin_params(m->prior[2], S(b.e2, H), B, dp_frame(DS_CODES, Z));
        p.sample = CS_SELECT;
        p.aux = dp_frame(DS_BITS, 1);
        p.y2 = dp_frame(DS_NOISE, Z);
        p.y3 = dp_frame(DS_PROB, Z);
        b.K(p, EPI_CODE);
        if (kind == STEP_ENTROPY && es) {
            GemmParams z; memset(&z, 0, sizeof(z));
            VbrStep v; memset(&v, 0, sizeof(v));
            plan.push_back(StepNode{OP_ENTROPY_DECODE, BR_MAIN, -1, z, 0, v, *es});
        }
    }
    if (kind == STEP_ENCODE) {
        b.enc02(h_cur);
        GemmParams p = lin_params(m->enc[2], S(b.e2, H), B, dp_frame(DS_CODES, Z));
        p.var_bit = m->cfg.var_bit;
        p.aux = dp_frame(DS_BITS, 1);
        p.y3 = dp_frame(DS_PROB, Z);
        b.K(p, EPI_CODE);
    }
    if (enc_like) {
        b.phi_z(dp_frame(DS_CODES, Z), B, b.pz1, b.pz2, b.pz3);
        REC(BR_MAIN, EV_PZ);
    }
    if (side) {      // dec.0 on the critical path only sees phi_z; the h half arrives from the side branch
        GemmParams p = half_params(m->dec[0], 0, pz_final, H, B, S(b.d1, H), true);
        p.aux = dp_static(w.part_d, H);
        WAIT(BR_MAIN, EV_DEC0H);
        b.K(p, EPI_ELU);
    } else if (kind == STEP_DECODE_PRE) {
        // dec.0([phi_z, h]) = (dec.0[:, :H] phi_z + b) [all frames, batched] + dec.0[:, H:] h
        GemmParams p = half_params(m->dec[0], H / 16, h_cur, H, B, S(b.d1, H), false);
        p.aux = dp_frame(DS_PARTD, H);
        b.K(p, EPI_ELU);
    } else {
        // both halves in the step: the h half first, then the phi_z half, chunk by chunk into the same accumulators (the order of the
        // persistent kernel, whose filler quanta have dec.0[:, H:] h summed before phi_z exists)
        b.dec0(b.dec0_h(h_cur), b.dec0_z(pz_final), B, b.d1);
    }
    if (fold) {
        // one launch less per frame: u = ELU(dec.4) (decode: also kept for all frames - dec.6(u), the decoder's output, is one batched
        // GEMM behind the recurrence), then phi_x.0(norm(dec.6(u))) as the one folded layer
        b.dec24(b.d1, B, b.d2, b.d3, dp_frame(!enc_like ? DS_KEEP : DS_KEEP_ENC, H));       // (encode: a null slot unless the fused forward wants mel^)
        b.elu(m->px0_dec3, S(b.d3, H), B, b.g1);
    } else {
        b.dec24(b.d1, B, b.d2, b.d3);
        b.dec6(b.d3, B, dp_frame(DS_MEL, X), b.dn);      // (encode: a null slot unless the fused forward wants mel^)
        b.elu(m->phi_x[0], S(b.dn, X), B, b.g1);
    }
    b.phi_x24();
    {
        const DynPtr all_h = (kind == STEP_ENCODE) ? dp_frame(DS_ALLH, H, 1) : dp_null();
        if (side) {
            GemmParams p = b.gru_cell(w.hbuf, all_h);
            p.nseg = 1;
            p.seg[0] = mkseg(S(b.g3, H), m->w_ih, 2 * H / 16, H, 0);                    // W_ih[:, :H] @ phi_x_gen
            p.part_i = w.part_i; p.part_h = w.part_h; p.ldpart = 3LL * H;
            WAIT(BR_MAIN, EV_GATES);
            b.K(p, EPI_GRU_PART);
        } else if (kind == STEP_DECODE_PRE) {
            GemmParams p = b.gru_cell(w.hbuf, all_h);
            p.nseg = 2;                                                               // W_ih[:, H:] phi_z + b_ih comes in through y3
            p.gate_il = 1;
            p.seg[0] = b.gru_x(S(b.g3, H));
            p.seg[1] = b.gru_h(h_cur);
            p.bias0 = nullptr; p.bias1 = m->b_hh;
            p.y3 = dp_frame(DS_PARTG, 3 * H);
            b.K(p, EPI_GRU);
        } else {
            // the phi_z third first (its input exists first: the persistent kernel sums it ahead)
            b.gru(b.gru_z(pz_final), b.gru_x(S(b.g3, H)), b.gru_h(h_cur), w.hbuf, all_h);
        }
    }
    if (side) {
        // side-branch operations, inserted at the positions where their inputs exist: step start for the
        // two h products; after phi_z for the W_ih half (encode) or step start (decode: phi_z is batched)
        std::vector<StepNode> main_ops;
        main_ops.swap(plan);
        REC(BR_MAIN, EV_START);
        WAIT(BR_SIDE, EV_START);
        side_dec0h();
        REC(BR_SIDE, EV_DEC0H);
        side_hh();
        if (kind == STEP_DECODE) { side_ihz(pz_final); REC(BR_SIDE, EV_GATES); }      // (enc_like: behind EV_PZ, below)
        for (const StepNode &n : main_ops) {
            plan.push_back(n);
            if (n.op == OP_RECORD && n.event == EV_PZ) {        // encode: phi_z ready
                WAIT(BR_SIDE, EV_PZ);
                side_ihz(pz_final);
                REC(BR_SIDE, EV_GATES);
            }
        }
    }
    return plan;
}

// One frame of bvc_bvrnn_encode_vbr: STEP_ENCODE with the rate chosen inside the frame.  Main branch only, and always the unfolded
// layer list - dec.6 must exist to be measured, so `encode_fold` does not apply here:
//   enc.0-4 at B rows (the phi_x half pre-computed: encode_prologue), the code written WITHOUT a mask to a scratch matrix
//   candidates: the K masked copies and h_t K times over, candidate row k * B + b
//   phi_z.0-4, dec.0-6 at K * B rows in one launch each (the kernels' results do not depend on the row count); dec.0 sums its h half
//     before its phi_z half, as build_step does
//   select: D of every rung, the first within the target, the frame's outputs, the chosen rows gathered back into B-row operands
//   phi_x.0-4 and the GRU at B rows, as build_step does
std::vector<StepNode> build_vbr_step(const bvc_model *m, const Workspace &w, const VbrWorkspace &vw, int B, int nrungs) {
    StepBuilder b(m, w, B, g_kprobe.enabled);
    const int H = b.H, Z = b.Z, X = b.X;
    const int KB = nrungs * B;
    const DynPtr h_cur = b.h_cur(w.hbuf);
    auto S = StepBuilder::S;
    VbrStep v;
    memset(&v, 0, sizeof(v));
    v.desc = w.desc; v.call = vw.call;
    v.B = B; v.K = nrungs; v.Z = Z; v.H = H; v.X = X;
    v.zraw = vw.zraw; v.hbuf = w.hbuf; v.MH = b.MH;
    v.zc = vw.zc; v.hrep = vw.hrep;
    v.melk = vw.melk; v.dnk = vw.dnk; v.pzk = vw.pz[2];
    v.pzsel = vw.pzsel; v.dnsel = vw.dnsel;
    auto V = [&](int op) { GemmParams z; memset(&z, 0, sizeof(z)); b.plan.push_back(StepNode{op, BR_MAIN, -1, z, 0, v}); };
    b.enc02(h_cur);
    {
        GemmParams p = lin_params(m->enc[2], S(b.e2, H), B, S(vw.zraw, Z));     // var_bit off: the mask is the candidates' business
        p.y3 = dp_frame(DS_PROB, Z);
        b.K(p, EPI_CODE);
    }
    V(OP_VBR_CANDIDATES);
    b.phi_z(S(vw.zc, Z), KB, vw.pz[0], vw.pz[1], vw.pz[2]);
    b.dec0(b.dec0_h(S(vw.hrep, H)), b.dec0_z(S(vw.pz[2], H)), KB, vw.d[0]);
    b.dec24(vw.d[0], KB, vw.d[1], vw.d[2]);
    b.dec6(vw.d[2], KB, dp_static(vw.melk, X), vw.dnk);      // natural rows: the select kernel reads them band by band
    V(OP_VBR_SELECT);
    b.elu(m->phi_x[0], S(vw.dnsel, X), B, b.g1);
    b.phi_x24();
    b.gru(b.gru_z(S(vw.pzsel, H)), b.gru_x(S(b.g3, H)), b.gru_h(h_cur), w.hbuf, dp_frame(DS_ALLH, H, 1));
    return b.plan;
}

// ---- BVRNN.forward (bvrnn.py:86-160): the training-time pass, forward values only --------------------
// One frame conditioned on state `sel` (0: h, the teacher-forced state; 1: h2, the state fed with generated
// features).  h2 lives in part_i (the side-branch buffer, unused here), both states ping-pong by frame parity.
// Never carries probes (two plans alternate: the probes index by a fixed kernel count per step).  Its concatenated inputs are summed
// in the order of torch.cat: dec.0 over [phi_z, h], the GRU over [phi_x, phi_z], h.
// tape (the backward pass, backward.hip): the frame's states come from and go to the tape's own matrices instead of the two ping-pong
// buffers, and `w` is a copy of the workspace whose scratch vectors are the frame's own; the kernels and their order are the same.
std::vector<StepNode> build_forward_step(const bvc_model *m, const Workspace &w, int B, int sel, bool greedy,
                                         bool update_h, bool update_h2, const ForwardTape *tape) {
    StepBuilder b(m, w, B, false);
    const int H = b.H, Z = b.Z, X = b.X;
    float *hb[2] = {w.hbuf, w.part_i};
    auto S = StepBuilder::S;
    const DynPtr h_in[2] = {tape ? S(tape->h_in[0], H) : b.h_cur(hb[0]), tape ? S(tape->h_in[1], H) : b.h_cur(hb[1])};
    const DynPtr h_out[2] = {tape ? S(tape->h_out[0], H) : b.h_next(hb[0]), tape ? S(tape->h_out[1], H) : b.h_next(hb[1])};
    const DynPtr hs = h_in[sel];
    const DynPtr px = dp_frame(DS_PX, H, 0, 1);
    // enc_t and the sample (bvrnn.py:115-129)
    b.K(lin2_params(m->enc[0], px, H, hs, H, B, S(b.e1, H)), EPI_ELU);
    b.elu(m->enc[1], S(b.e1, H), B, b.e2);
    {
        GemmParams p = lin_params(m->enc[2], S(b.e2, H), B, dp_frame(DS_CODES, Z));
        p.var_bit = m->cfg.var_bit;
        p.sample = greedy ? CS_GREEDY : CS_SAMPLE;
        p.aux = dp_frame(DS_BITS, 1);
        p.y2 = greedy ? dp_null() : dp_frame(DS_NOISE, Z);
        p.y3 = dp_frame(DS_PROB, Z);
        b.K(p, EPI_CODE);
    }
    // prior_t (bvrnn.py:116,119)
    b.elu(m->prior[0], hs, B, b.q1);
    b.elu(m->prior[1], S(b.q1, H), B, b.q2);
    b.K(lin_params(m->prior[2], S(b.q2, H), B, dp_frame(DS_PRIOR, Z)), EPI_SIGMOID);
    // phi_z, dec (bvrnn.py:131-137)
    b.phi_z(dp_frame(DS_CODES, Z), B, b.pz1, b.pz2, b.pz3);
    b.dec0(b.dec0_z(S(b.pz3, H)), b.dec0_h(hs), B, b.d1);
    b.dec24(b.d1, B, b.d2, b.d3);
    b.dec6(b.d3, B, dp_frame(DS_MEL, X), b.dn);
    auto gru = [&](DynPtr xin, int which) { b.gru(b.gru_x(xin), b.gru_z(S(b.pz3, H)), b.gru_h(h_in[which]), h_in[which], h_out[which], dp_null()); };
    if (update_h) gru(px, 0);                                        // h  <- GRU([phi_x_t, phi_z_t], h)      bvrnn.py:142-143
    if (update_h2) {                                                 // h2 <- GRU([phi_x_t_gen, phi_z_t], h2) bvrnn.py:139,144-145
        b.elu(m->phi_x[0], S(b.dn, X), B, b.g1);
        b.phi_x24();
        gru(S(b.g3, H), 1);
    }
    return b.plan;
}

int count_kernels(const std::vector<StepNode> &plan) {
    int n = 0;
    for (const StepNode &s : plan) n += (s.op == OP_KERNEL);
    return n;
}

// Launch `nsteps` consecutive frames; the frame counter is advanced ONCE at the end: frame k of the
// group runs with the static offset tstep = k baked into its kernel arguments.  With side == nullptr
// everything runs in plan order on `s` (the plan order respects every dependency).
int launch_steps(const bvc_model *m, const std::vector<StepNode> &plan, const Workspace &w, int nsteps, hipStream_t s,
                 hipStream_t side) {
    int rc;
    for (int k = 0; k < nsteps; ++k)
        for (const StepNode &n : plan) {
            hipStream_t st = (n.branch == BR_SIDE && side) ? side : s;
            if (n.op == OP_KERNEL) {
                GemmParams p = n.p;
                p.tstep = k;
                if ((rc = launch_gemm_skinny(p, n.epi, st, m->mtw))) return rc;
            } else if (n.op == OP_VBR_CANDIDATES) {
                if ((rc = launch_vbr_candidates(n.v, k, st))) return rc;
            } else if (n.op == OP_VBR_SELECT) {
                if ((rc = launch_vbr_select(n.v, k, st))) return rc;
            } else if (n.op == OP_ENTROPY_DECODE) {
                if ((rc = launch_entropy_decode_step(n.e, k, st))) return rc;
            } else if (side) {
                if (n.op == OP_RECORD) BVC_HIP_TRY(hipEventRecord(m->cap_events[n.event], st));
                else                   BVC_HIP_TRY(hipStreamWaitEvent(st, m->cap_events[n.event], 0));
            }
        }
    return launch_step_advance(w.desc, nsteps, s);
}

constexpr int GRAPH_STEPS = 8;

constexpr size_t GRAPH_CACHE_ENTRIES = 64;      // (kind, batch, workspace) triples kept per model; least recently used goes first

// Returns the cached graph pair for (kind, B, workspace), capturing it on first use.  Caller holds m->graph_mu.
static int get_step_graph(const bvc_model *m, const Workspace &w, void *ws_base, int B, int kind,
                   const std::vector<StepNode> &plan, bvc_model::StepGraph **out) {
    void *probe = g_kprobe.enabled ? (void *)g_kprobe.dev : nullptr;
    for (auto it = m->graphs.begin(); it != m->graphs.end(); ++it)
        if (it->kind == kind && it->B == B && it->ws == ws_base && it->probe == probe) {
            m->graphs.splice(m->graphs.begin(), m->graphs, it);          // most recently used first
            *out = &m->graphs.front();
            return BVC_OK;
        }
    if (!m->cap_stream) BVC_HIP_TRY(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
    if (!m->side_stream) BVC_HIP_TRY(hipStreamCreateWithFlags(&m->side_stream, hipStreamNonBlocking));
    while ((int)m->cap_events.size() < EV_COUNT) {
        hipEvent_t e;
        BVC_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m->cap_events.push_back(e);
    }
    bvc_model::StepGraph sg{kind, B, ws_base, probe, nullptr, nullptr, nullptr};
    for (int which = 0; which < 2; ++which) {
        hipGraph_t graph = nullptr;
        g_capturing = true;
        hipError_t e = hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal);
        int rc = BVC_OK;
        if (e == hipSuccess) rc = launch_steps(m, plan, w, which ? GRAPH_STEPS : 1, m->cap_stream, m->side_branch ? m->side_stream : nullptr);
        // always close the capture, also when a launch inside it failed, so the stream stays usable
        hipError_t e2 = (e == hipSuccess) ? hipStreamEndCapture(m->cap_stream, &graph) : e;
        g_capturing = false;
        if (rc) { if (graph) (void)hipGraphDestroy(graph); if (sg.exec1) (void)hipGraphExecDestroy(sg.exec1); return rc; }
        if (e2 != hipSuccess || !graph) {
            if (sg.exec1) (void)hipGraphExecDestroy(sg.exec1);
            set_error("hipGraph capture failed: %s", hipGetErrorString(e2));
            return BVC_EHIP;
        }
        hipGraphExec_t ex = nullptr;
        BVC_HIP_TRY(hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0));
        BVC_HIP_TRY(hipGraphDestroy(graph));
        (which ? sg.execN : sg.exec1) = ex;
    }
    BVC_HIP_TRY(hipEventCreateWithFlags(&sg.idle, hipEventDisableTiming));
    while (m->graphs.size() >= GRAPH_CACHE_ENTRIES) {       // bound the cache: the least recently used entry goes, once it is idle
        bvc_model::StepGraph &old = m->graphs.back();
        (void)hipEventSynchronize(old.idle);                  // (never recorded: returns at once)
        (void)hipGraphExecDestroy(old.exec1); (void)hipGraphExecDestroy(old.execN); (void)hipEventDestroy(old.idle);
        m->graphs.pop_back();
    }
    m->graphs.push_front(sg);
    *out = &m->graphs.front();
    return BVC_OK;
}

// Does the launch-per-layer schedule of this call fold the hop?  Whenever the model does (`encode_fold` / `decode_fold`), streaming hops
// included: every schedule runs the same layer list, so that their results are the same bits.
int step_fold(const bvc_model *m, bool encode) {
    if (!m->px0_dec3.wp || m->side_branch) return 0;
    return (encode ? m->encode_fold : m->decode_fold) ? STEP_FOLD : 0;
}

// (begin_call was given count_kernels(plan) kernels per step)
int run_recurrence(const bvc_model *m, const Workspace &w, void *ws_base, int B, int64_t T, int kind, const std::vector<StepNode> &plan,
                   hipStream_t s) {
    auto eager = [&]() { int e = BVC_OK; for (int64_t t = 0; !e && t < T; ++t) e = launch_steps(m, plan, w, 1, s, nullptr); return e; };
    Capture cap = capture_state(s);
    if (cap == CAP_FAILED) { (void)hipGetLastError(); cap = CAP_NONE; }
    // a caller's capture takes the kernels directly (no graph of our own is built, replayed or marked idle inside it)
    if (!m->use_graph || g_stream_tick || cap != CAP_NONE) return eager();
    std::lock_guard<std::mutex> lk(m->graph_mu);          // cache look-up, replay and the idle mark are one critical section
    bvc_model::StepGraph *g = nullptr;
    if (int rc = get_step_graph(m, w, ws_base, B, kind, plan, &g)) {
        if (rc != BVC_EHIP) return rc;
        // stream capture unavailable (e.g. the caller is itself capturing): same kernels, launched eagerly
        (void)hipGetLastError();
        return eager();
    }
    int64_t t = 0;
    for (; t + GRAPH_STEPS <= T; t += GRAPH_STEPS) BVC_HIP_TRY(hipGraphLaunch(g->execN, s));
    for (; t < T; ++t) BVC_HIP_TRY(hipGraphLaunch(g->exec1, s));
    BVC_HIP_TRY(hipEventRecord(g->idle, s));
    return BVC_OK;
}

int begin_call(const bvc_model *m, const Workspace &w, const CallDesc &v, int steps_nodes, bool probes, hipStream_t s) {
    CallDesc d = v;
    d.t = 0;
    d.nodes_per_step = steps_nodes;
    if (probes) {
        const size_t need = (size_t)2 * d.T * steps_nodes;
        if (need > g_kprobe.capacity) { set_error("kprobe buffer too small for T=%lld", (long long)d.T); return BVC_EINVAL; }
        {
            // first half: start stamps (atomicMin, so all ones); second half: end stamps (atomicMax, so zero)
            BVC_HIP_TRY(hipMemsetAsync(g_kprobe.dev, 0xFF, need / 2 * sizeof(unsigned long long), s));
            BVC_HIP_TRY(hipMemsetAsync(g_kprobe.dev + need / 2, 0, need / 2 * sizeof(unsigned long long), s));
            g_kprobe.T = d.T; g_kprobe.nodes = steps_nodes;
        }
    }
    return launch_set_desc(w.desc, d, s);
}

}  // namespace bvc
