// The BVRNN recurrence: the launch-per-layer step plan with its hipGraph cache, the persistent-kernel launch with its tickets and
// fences, the all-frame prologues, and the drivers of encode, decode, the concealing decoder and the training-time forward pass.
#include "bvc_host.h"

using namespace bvc;

namespace {

// One operation of a step: a kernel on the main or the side branch, or an event record / wait that
// forks and joins the two branches (they become graph dependencies under stream capture).
enum { OP_KERNEL = 0, OP_RECORD = 1, OP_WAIT = 2, OP_VBR_CANDIDATES = 3, OP_VBR_SELECT = 4 };   // _VBR_*: the two kernels of k_vbr.hip (v)
enum { BR_MAIN = 0, BR_SIDE = 1 };
struct StepNode { int op; int branch; int event; GemmParams p; int epi; VbrStep v; };
enum { STEP_ENCODE = 0, STEP_DECODE = 1, STEP_DECODE_PRE = 2, STEP_CONCEAL = 3, STEP_ENCODE_VBR = 4 };   // _PRE: phi_z halves of dec.0 / GRU arrive pre-computed
                                                                  // _CONCEAL: the concealing decoder - the encode step with the prior net in the encoder's place
                                                                  // _VBR: the encode step with K candidate rungs per frame (build_vbr_step)
enum { STEP_KIND_MASK = 0xF, STEP_FOLD = 0x10, STEP_RUNGS_SHIFT = 8 };   // | STEP_FOLD: the folded hop (step_fold below); | K << STEP_RUNGS_SHIFT: the rungs of a
                                                                  // _VBR step (part of the graph-cache key: the candidate launches have K * B rows)
constexpr int64_t SMALL_T_FRAMES = 4;          // up to this many frames per call the all-frame MLPs run frame by frame on the recurrent-layer kernel
enum { EV_START = 0, EV_DEC0H = 1, EV_PZ = 2, EV_GATES = 3, EV_COUNT = 4 };

// The operation sequence of ONE frame.  Every pointer is either workspace-static, frame-indexed through
// the call descriptor, or parity-indexed (GRU state), so the same sequence serves every frame and
// every call: it is captured once into a hipGraph.  Internal activations are kept in MFMA fragment
// order (packed=1) so every operand load is a coalesced 1 KiB read.
//   encode (bvrnn.py:187-206): enc -> sigmoid/round/mask -> phi_z -> dec -> phi_x(norm) -> GRU
//   decode (bvrnn.py:222-227): [phi_z batched over all frames beforehand] dec -> phi_x(norm) -> GRU
//   conceal (bvc_bvrnn_decode_conceal): prior -> sigmoid/round/mask, SELECTED against the received codes -> phi_z -> ... as encode
//   closed-loop rates (bvc_bvrnn_encode_vbr): enc -> sigmoid/round -> K masked candidates -> phi_z -> dec on K * B rows -> select -> ... as encode
//     (build_vbr_step below; never folded: dec.6 must exist to be measured)
// Side branch: the halves of the split dot products that do not depend on the current frame's chain -
// dec.0[:, H:] h, W_hh h + b_hh, W_ih[:, H:] phi_z + b_ih - run concurrently with the chain (which is
// latency-bound), so the GRU kernel on the critical path only streams W_ih[:, :H].
std::vector<StepNode> build_step(const bvc_model *m, const Workspace &w, int B, int kind_and_fold) {
    const int kind = kind_and_fold & STEP_KIND_MASK;
    const bool fold = (kind_and_fold & STEP_FOLD) != 0;       // dec.6 -> norm -> phi_x.0 as one layer (bvc_model::px0_dec3)
    const bool enc_like = kind == STEP_ENCODE || kind == STEP_CONCEAL;    // phi_z is computed inside the step
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    std::vector<StepNode> plan;
    const long long MH = (long long)((B + 15) / 16) * 16 * H;
    const DynPtr h_cur = dp_parity(w.hbuf, H, MH, 0, 1);
    const DynPtr h_next = dp_parity(w.hbuf + MH, H, -MH, 0, 1);
    float *e1 = w.step[0], *e2 = w.step[1];
    float *pz1 = w.step[2], *pz2 = w.step[3], *pz3 = w.step[4];
    float *d1 = w.step[5], *d2 = w.step[6], *d3 = w.step[7], *dn = w.step[8];
    float *g1 = w.step[9], *g2 = w.step[10], *g3 = w.step[11];
    auto S = [&](float *p, int ld) { return dp_static(p, ld, 1); };
    const bool side = m->side_branch;
    int node = 0;
    auto K = [&](int branch, GemmParams p, int epi) {
        p.desc = w.desc; p.node = node++;
        p.probe = g_kprobe.enabled ? g_kprobe.dev : nullptr;
        finish(p);
        plan.push_back(StepNode{OP_KERNEL, branch, -1, p, epi});
    };
    auto REC = [&](int branch, int ev) { GemmParams z; memset(&z, 0, sizeof(z)); if (side) plan.push_back(StepNode{OP_RECORD, branch, ev, z, 0}); };
    auto WAIT = [&](int branch, int ev) { GemmParams z; memset(&z, 0, sizeof(z)); if (side) plan.push_back(StepNode{OP_WAIT, branch, ev, z, 0}); };
    // --- side-branch kernels (plain linears into natural [B][.] partial buffers)
    // dec.0.weight[:, H:] @ h (no bias: added on the main branch); W_hh @ h + b_hh; W_ih[:, H:] @ phi_z + b_ih
    auto side_dec0h = [&]() { K(BR_SIDE, half_params(m->dec[0], H / 16, h_cur, H, B, dp_static(w.part_d, H), false), EPI_LINEAR); };
    auto side_hh = [&]() { K(BR_SIDE, mat_params(h_cur, m->w_hh, H / 16, H, B, 3 * H, m->b_hh, dp_static(w.part_h, 3 * H)), EPI_LINEAR); };
    auto side_ihz = [&](DynPtr pz) {
        K(BR_SIDE, mat_params(pz, m->w_ih + (size_t)(H / 16) * 256, 2 * H / 16, H, B, 3 * H, m->b_ih, dp_static(w.part_i, 3 * H)), EPI_LINEAR);
    };

    DynPtr pz_final = enc_like ? S(pz3, H) : dp_frame(DS_PZ, H, 0, 1);
    if (kind == STEP_CONCEAL) {
        // p_t = prior(h_t) (bvrnn.py:68-73): no pre-computed half, the first layer's bias is its own; the code epilogue SELECTS between the
        // received codes (DS_NOISE carries them) and the generated bits, by the selector in DS_BITS; p_t goes to DS_PROB
        K(BR_MAIN, lin_params(m->prior[0], h_cur, B, S(e1, H)), EPI_ELU);
        K(BR_MAIN, lin_params(m->prior[1], S(e1, H), B, S(e2, H)), EPI_ELU);
        GemmParams p = lin_params(m->prior[2], S(e2, H), B, dp_frame(DS_CODES, Z));
        p.sample = CS_SELECT;
        p.aux = dp_frame(DS_BITS, 1);
        p.y2 = dp_frame(DS_NOISE, Z);
        p.y3 = dp_frame(DS_PROB, Z);
        K(BR_MAIN, p, EPI_CODE);
    }
    if (kind == STEP_ENCODE) {
        {   // enc.0([phi_x, h]) = (enc.0[:, :H] phi_x + b) [all frames beforehand: encode_prologue] + enc.0[:, H:] h, as in the persistent kernel
            GemmParams p = half_params(m->enc[0], H / 16, h_cur, H, B, S(e1, H), false);
            p.aux = dp_frame(DS_PARTD, H);
            K(BR_MAIN, p, EPI_ELU);
        }
        K(BR_MAIN, lin_params(m->enc[1], S(e1, H), B, S(e2, H)), EPI_ELU);
        {
            GemmParams p = lin_params(m->enc[2], S(e2, H), B, dp_frame(DS_CODES, Z));
            p.var_bit = m->cfg.var_bit;
            p.aux = dp_frame(DS_BITS, 1);
            p.y3 = dp_frame(DS_PROB, Z);
            K(BR_MAIN, p, EPI_CODE);
        }
    }
    if (enc_like) {
        K(BR_MAIN, lin_params(m->phi_z[0], dp_frame(DS_CODES, Z), B, S(pz1, H)), EPI_ELU);
        K(BR_MAIN, lin_params(m->phi_z[1], S(pz1, H), B, S(pz2, H)), EPI_ELU);
        K(BR_MAIN, lin_params(m->phi_z[2], S(pz2, H), B, S(pz3, H)), EPI_ELU);
        REC(BR_MAIN, EV_PZ);
    }
    if (side) {      // dec.0 on the critical path only sees phi_z; the h half arrives from the side branch
        GemmParams p = half_params(m->dec[0], 0, pz_final, H, B, S(d1, H), true);
        p.aux = dp_static(w.part_d, H);
        WAIT(BR_MAIN, EV_DEC0H);
        K(BR_MAIN, p, EPI_ELU);
    } else if (kind == STEP_DECODE_PRE) {
        // dec.0([phi_z, h]) = (dec.0[:, :H] phi_z + b) [all frames, batched] + dec.0[:, H:] h
        GemmParams p = half_params(m->dec[0], H / 16, h_cur, H, B, S(d1, H), false);
        p.aux = dp_frame(DS_PARTD, H);
        K(BR_MAIN, p, EPI_ELU);
    } else {
        // both halves in the step: the h half first, then the phi_z half, chunk by chunk into the same accumulators (the order of the
        // persistent kernel, whose filler quanta have dec.0[:, H:] h summed before phi_z exists)
        GemmParams p = lin_params(m->dec[0], h_cur, B, S(d1, H));
        p.nseg = 2;
        p.seg[0] = mkseg(h_cur, m->dec[0].wp + (size_t)(H / 16) * 256, 2 * H / 16, H, 0);
        p.seg[1] = mkseg(pz_final, m->dec[0].wp, 2 * H / 16, H, 0);
        K(BR_MAIN, p, EPI_ELU);
    }
    K(BR_MAIN, lin_params(m->dec[1], S(d1, H), B, S(d2, H)), EPI_ELU);
    if (fold) {
        // one launch less per frame: u = ELU(dec.4) (decode: also kept for all frames - dec.6(u), the decoder's output, is one batched
        // GEMM behind the recurrence), then phi_x.0(norm(dec.6(u))) as the one folded layer
        GemmParams p = lin_params(m->dec[2], S(d2, H), B, S(d3, H));
        p.y2 = dp_frame(!enc_like ? DS_KEEP : DS_KEEP_ENC, H);       // (encode: a null slot unless the fused forward wants mel^)
        K(BR_MAIN, p, EPI_ELU);
        K(BR_MAIN, lin_params(m->px0_dec3, S(d3, H), B, S(g1, H)), EPI_ELU);
    } else {
        K(BR_MAIN, lin_params(m->dec[2], S(d2, H), B, S(d3, H)), EPI_ELU);
        GemmParams p = lin_params(m->dec[3], S(d3, H), B, dp_frame(DS_MEL, X));      // (encode: a null slot unless the fused forward wants mel^)
        p.y2 = S(dn, X); p.mean = m->mean_mel; p.stdv = m->std_mel;
        K(BR_MAIN, p, EPI_MEL);
        K(BR_MAIN, lin_params(m->phi_x[0], S(dn, X), B, S(g1, H)), EPI_ELU);
    }
    K(BR_MAIN, lin_params(m->phi_x[1], S(g1, H), B, S(g2, H)), EPI_ELU);
    K(BR_MAIN, lin_params(m->phi_x[2], S(g2, H), B, S(g3, H)), EPI_ELU);
    {
        GemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = B; p.N = H; p.gate_rows = H;
        p.y = h_next;
        p.y2 = (kind == STEP_ENCODE) ? dp_frame(DS_ALLH, H, 1) : dp_null();   // all_h[:, t+1] (bvrnn.py:205)
        p.aux = h_cur;
        if (side) {
            p.nseg = 1;
            p.seg[0] = mkseg(S(g3, H), m->w_ih, 2 * H / 16, H, 0);                    // W_ih[:, :H] @ phi_x_gen
            p.part_i = w.part_i; p.part_h = w.part_h; p.ldpart = 3LL * H;
            WAIT(BR_MAIN, EV_GATES);
            K(BR_MAIN, p, EPI_GRU_PART);
        } else if (kind == STEP_DECODE_PRE) {
            p.nseg = 2;                                                               // W_ih[:, H:] phi_z + b_ih comes in through y3
            p.gate_il = 1;
            p.seg[0] = mkseg(S(g3, H), m->w_ih_il, 2 * H / 16, H, 0);
            p.seg[1] = mkseg(h_cur, m->w_hh_il, H / 16, H, 1);
            p.bias0 = nullptr; p.bias1 = m->b_hh;
            p.y3 = dp_frame(DS_PARTG, 3 * H);
            K(BR_MAIN, p, EPI_GRU);
        } else {
            p.nseg = 3;
            p.gate_il = 1;
            // cat([phi_x_gen, phi_z]) bvrnn.py:206; the phi_z third first (its input exists first: the persistent kernel sums it ahead)
            p.seg[0] = mkseg(pz_final, m->w_ih_il + (size_t)(H / 16) * 3 * 256, 2 * H / 16, H, 0);
            p.seg[1] = mkseg(S(g3, H), m->w_ih_il, 2 * H / 16, H, 0);
            p.seg[2] = mkseg(h_cur, m->w_hh_il, H / 16, H, 1);
            p.bias0 = m->b_ih; p.bias1 = m->b_hh;
            K(BR_MAIN, p, EPI_GRU);
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
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    const int KB = nrungs * B;
    std::vector<StepNode> plan;
    const long long MH = (long long)((B + 15) / 16) * 16 * H;
    const DynPtr h_cur = dp_parity(w.hbuf, H, MH, 0, 1);
    const DynPtr h_next = dp_parity(w.hbuf + MH, H, -MH, 0, 1);
    float *e1 = w.step[0], *e2 = w.step[1], *g1 = w.step[9], *g2 = w.step[10], *g3 = w.step[11];
    auto S = [&](float *p, int ld) { return dp_static(p, ld, 1); };
    int node = 0;
    auto K = [&](GemmParams p, int epi) {
        p.desc = w.desc; p.node = node++;
        p.probe = g_kprobe.enabled ? g_kprobe.dev : nullptr;
        finish(p);
        plan.push_back(StepNode{OP_KERNEL, BR_MAIN, -1, p, epi});
    };
    VbrStep v;
    memset(&v, 0, sizeof(v));
    v.desc = w.desc; v.call = vw.call;
    v.B = B; v.K = nrungs; v.Z = Z; v.H = H; v.X = X;
    v.zraw = vw.zraw; v.hbuf = w.hbuf; v.MH = MH;
    v.zc = vw.zc; v.hrep = vw.hrep;
    v.melk = vw.melk; v.dnk = vw.dnk; v.pzk = vw.pz[2];
    v.pzsel = vw.pzsel; v.dnsel = vw.dnsel;
    auto V = [&](int op) { GemmParams z; memset(&z, 0, sizeof(z)); plan.push_back(StepNode{op, BR_MAIN, -1, z, 0, v}); };
    {
        GemmParams p = half_params(m->enc[0], H / 16, h_cur, H, B, S(e1, H), false);
        p.aux = dp_frame(DS_PARTD, H);
        K(p, EPI_ELU);
    }
    K(lin_params(m->enc[1], S(e1, H), B, S(e2, H)), EPI_ELU);
    {
        GemmParams p = lin_params(m->enc[2], S(e2, H), B, S(vw.zraw, Z));     // var_bit off: the mask is the candidates' business
        p.y3 = dp_frame(DS_PROB, Z);
        K(p, EPI_CODE);
    }
    V(OP_VBR_CANDIDATES);
    K(lin_params(m->phi_z[0], S(vw.zc, Z), KB, S(vw.pz[0], H)), EPI_ELU);
    K(lin_params(m->phi_z[1], S(vw.pz[0], H), KB, S(vw.pz[1], H)), EPI_ELU);
    K(lin_params(m->phi_z[2], S(vw.pz[1], H), KB, S(vw.pz[2], H)), EPI_ELU);
    {
        GemmParams p = lin_params(m->dec[0], S(vw.hrep, H), KB, S(vw.d[0], H));
        p.nseg = 2;
        p.seg[0] = mkseg(S(vw.hrep, H), m->dec[0].wp + (size_t)(H / 16) * 256, 2 * H / 16, H, 0);
        p.seg[1] = mkseg(S(vw.pz[2], H), m->dec[0].wp, 2 * H / 16, H, 0);
        K(p, EPI_ELU);
    }
    K(lin_params(m->dec[1], S(vw.d[0], H), KB, S(vw.d[1], H)), EPI_ELU);
    K(lin_params(m->dec[2], S(vw.d[1], H), KB, S(vw.d[2], H)), EPI_ELU);
    {
        GemmParams p = lin_params(m->dec[3], S(vw.d[2], H), KB, dp_static(vw.melk, X));      // natural rows: the select kernel reads them band by band
        p.y2 = S(vw.dnk, X); p.mean = m->mean_mel; p.stdv = m->std_mel;
        K(p, EPI_MEL);
    }
    V(OP_VBR_SELECT);
    K(lin_params(m->phi_x[0], S(vw.dnsel, X), B, S(g1, H)), EPI_ELU);
    K(lin_params(m->phi_x[1], S(g1, H), B, S(g2, H)), EPI_ELU);
    K(lin_params(m->phi_x[2], S(g2, H), B, S(g3, H)), EPI_ELU);
    {
        GemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = B; p.N = H; p.gate_rows = H;
        p.y = h_next;
        p.y2 = dp_frame(DS_ALLH, H, 1);
        p.aux = h_cur;
        p.nseg = 3;
        p.gate_il = 1;
        p.seg[0] = mkseg(S(vw.pzsel, H), m->w_ih_il + (size_t)(H / 16) * 3 * 256, 2 * H / 16, H, 0);
        p.seg[1] = mkseg(S(g3, H), m->w_ih_il, 2 * H / 16, H, 0);
        p.seg[2] = mkseg(h_cur, m->w_hh_il, H / 16, H, 1);
        p.bias0 = m->b_ih; p.bias1 = m->b_hh;
        K(p, EPI_GRU);
    }
    return plan;
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
int get_step_graph(const bvc_model *m, const Workspace &w, void *ws_base, int B, int kind,
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
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    // a caller's capture takes the kernels directly (no graph of our own is built, replayed or marked idle inside it)
    if (!m->use_graph || g_stream_tick || cs != hipStreamCaptureStatusNone) return eager();
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

int begin_call(const bvc_model *m, const Workspace &w, const CallDesc &v, int steps_nodes, hipStream_t s) {
    CallDesc d = v;
    d.t = 0;
    d.nodes_per_step = steps_nodes;
    if (g_kprobe.enabled) {
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

// ---- persistent recurrence (k_flow.hip): hop tables and launch -----------------------------------------
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

// The persistent kernel needs all its workgroups resident at once (they wait for each other), so launches from
// different streams are serialised through one event: at most one is in flight per process and device.
constexpr int FLOW_MAX_TICKETS = 2;
hipEvent_t g_flow_ev[16][FLOW_MAX_TICKETS] = {};
unsigned long long g_flow_n[16] = {};
// RS_AUTO: the end of the last recurrence-bearing call on this device (any model of this process) and the stream it ran on.
// A call that starts while the previous one - issued on ANOTHER stream - is still running has company: batches are in flight
// on several streams, where the launch-per-layer chains of the streams interleave on the chip while persistent launches (each takes
// every compute unit) would run one after the other.  The switch is sticky for AUTO_HOLD calls so that all streams change together.
struct LastCall { hipEvent_t ev = nullptr; hipStream_t s = nullptr; bool any = false; int hold = 0; };
LastCall g_last_call[16];
constexpr int AUTO_HOLD = 2;

// Which schedule does THIS call take?  0: launch per layer; else utterance groups per workgroup of the persistent kernel.
// Called once per recurrence-bearing call (run_encode / run_decode); mark_call_end() follows at its end.
int flow_chains(const bvc_model *m, int B, hipStream_t s) {
    if (m->census_due && (!g_stream_tick || g_tick_flow)) {               // a time-out was reported: is a full grid still co-resident?  (synchronises: error path only)
        hipStreamCaptureStatus cs0 = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs0) == hipSuccess && cs0 == hipStreamCaptureStatusNone) {
            m->census_due = false;
            (void)flow_census(m);
        } else {
            (void)hipGetLastError();
        }
    }
    const int chains = flow_chains_static(m, B);
    if (!chains) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
    // a caller's capture: the persistent launch cannot be captured (its one-at-a-time ticket is a host-side wait on an event
    // recorded outside the capture, and replays would skip it): captured calls take the launch-per-layer kernels
    if (cs != hipStreamCaptureStatusNone) return 0;
    if (m->recurrence != RS_AUTO) return chains;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return chains; }
    std::lock_guard<std::mutex> lk(g_flow_mu);
    LastCall &lc = g_last_call[dev & 15];
    const bool company = lc.any && lc.s != s && hipEventQuery(lc.ev) == hipErrorNotReady;
    (void)hipGetLastError();
    if (company) lc.hold = AUTO_HOLD;
    else if (lc.hold > 0) --lc.hold;
    return (company || lc.hold > 0) ? 0 : chains;
}

// Fences (bvc_flow_fence): work a caller issued on some stream - an RCCL collective that holds compute units while it waits for
// its peers, say - that must have finished before the next persistent launch starts.  A small ring; a persistent launch
// waits for every pending entry (later launches wait for that launch through the ticket).
constexpr int FLOW_FENCES = 8;
struct FlowFence { hipEvent_t ev = nullptr; bool pending = false; };
FlowFence g_fence[16][FLOW_FENCES];
unsigned g_fence_n[16] = {};

int mark_call_end(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return BVC_OK; }
    int dev = 0;
    BVC_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_flow_mu);
    LastCall &lc = g_last_call[dev & 15];
    if (!lc.ev) BVC_HIP_TRY(hipEventCreateWithFlags(&lc.ev, hipEventDisableTiming));
    BVC_HIP_TRY(hipEventRecord(lc.ev, s));
    lc.s = s; lc.any = true;
    return BVC_OK;
}

inline float *flow_buf(const Workspace &w, int id, int parity) { return w.flow + (size_t)(id * 2 + parity) * w.flow_slot; }

// dec.6 over the kept u = ELU(dec.4) of all frames (the folded hop): the decoder's output mel^ (bvrnn.py:224-225)
int decode_epilogue(const bvc_model *m, const float *keep, int B, int64_t T, float *d_mel, hipStream_t s) {
    const int H = m->cfg.h_dim, X = m->cfg.num_mels;
    const int BT = (int)((long long)B * T);
    if (T <= SMALL_T_FRAMES)
        return launch_gemm_skinny(lin_params(m->dec[3], dp_static(keep, H), BT, dp_static(d_mel, X)), EPI_LINEAR, s, m->mtw);
    return launch_gemm_batched(keep, H, m->dec[3].w, H, m->dec[3].b, BT, X, H, 0, d_mel, X, s);
}

// All T frames of BVRNN.encode (encode = true) or BVRNN.decode in one launch.  w.part_dec0 (and w.part_gru for decode)
// must hold the pre-computed halves; h0 may be null (zero state).
int run_flow(const bvc_model *m, const Workspace &w, bool encode, int chains, const float *d_h0, int B, int64_t T, const float *d_bits,
             float *d_codes, float *d_prob, float *d_all_h, float *d_mel, float *d_hT, hipStream_t s, const float *d_codes_in = nullptr) {
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    const int mt16 = ((B + 15) / 16) * 16;
    const bool conceal = d_codes_in != nullptr;        // the concealing decoder (encode = true: its program is encode's; d_bits = the selector)
    int rc;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        BVC_HIP_TRY(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) { set_error("the persistent recurrence cannot be captured into a graph"); return BVC_EINVAL; }
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
        int dev = 0;
        BVC_HIP_TRY(hipGetDevice(&dev));
        dev &= 15;
        const int tickets = sw.tickets;
        hipEvent_t &ev = g_flow_ev[dev][g_flow_n[dev] % tickets];        // the launch `tickets` launches ago must have finished
        if (!ev) BVC_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (g_flow_n[dev] >= (unsigned long long)tickets) BVC_HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        for (auto &f : g_fence[dev])
            if (f.pending) { BVC_HIP_TRY(hipStreamWaitEvent(s, f.ev, 0)); f.pending = false; }
        ProbeScope probe(PK_LINEAR, s);
        if ((rc = launch_flow(a, w.flow_args, m->flow_perh, encode, sw.fill && !m->flow_debug_nofill && a.MG == 1, s, fused_prepare, conceal))) return rc;
        BVC_HIP_TRY(hipEventRecord(ev, s));
        ++g_flow_n[dev];
    }
    if (d_hT && (rc = launch_repack_rows(flow_buf(w, FB_H, (int)(T & 1)), d_hT, H, B, H, 1, s))) return rc;
    // folded decode: the decoder's output dec.6(u_t) for all frames at once (bvrnn.py:224-225)
    if (a.pxc.w && d_mel && (rc = decode_epilogue(m, w.pxB, B, T, d_mel, s))) return rc;
    return BVC_OK;
}

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
    const int mt16 = ((B + 15) / 16) * 16;
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
        const DynPtr x = dp_static_frames(w.pxA, H, (long long)((B + 15) / 16) * 16 * H, 1);
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
        const DynPtr pz = dp_static_frames(w.pxA, H, (long long)((B + 15) / 16) * 16 * H, 1);
        return launch_frames(m, mat_params(pz, m->w_ih + (size_t)(H / 16) * 256, 2 * H / 16, H, B, 3 * H, m->b_ih, dp_static_frames(w.part_gru, T * 3 * H, 3 * H)),
                             EPI_LINEAR, T, s);
    }
    return launch_gemm_batched(w.pxC, H, m->w_ih_nat + H, 2 * H, m->b_ih, (int)((long long)B * T), 3 * H, H, 0, w.part_gru, 3 * H, s);
}

// The launch-per-layer schedule of one call, from the initial state to the final one: T frames of the step `kind` over the descriptor
// `d`, whose slots the caller has filled.  all_h[:, 0] = h0 where the call returns the states (DS_ALLH).  mel_out (folded hop only): the
// step kept u = ELU(dec.4) of every frame in w.pxB; dec.6(u), the decoder's output, goes there for all frames at once.
int run_layers(const bvc_model *m, const Workspace &w, void *ws_base, CallDesc &d, int kind, const float *d_h0, int B, int64_t T,
               float *d_hT, float *mel_out, hipStream_t s) {
    const int H = m->cfg.h_dim;
    const long long MH = (long long)((B + 15) / 16) * 16 * H;
    int rc;
    // the GRU state lives fragment-packed in hbuf[parity of the frame counter]; h0 (or zero) goes to parity 0
    if ((rc = d_h0 ? launch_repack_rows(d_h0, w.hbuf, H, B, H, 0, s) : launch_fill(w.hbuf, 0.0f, MH, s))) return rc;
    if (d.p[DS_ALLH] && (rc = launch_repack_rows(w.hbuf, d.p[DS_ALLH], (long long)T * H, B, H, 1, s))) return rc;
    d.T = T;
    const std::vector<StepNode> plan = build_step(m, w, B, kind);
    if ((rc = begin_call(m, w, d, count_kernels(plan), s))) return rc;
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

// ---- BVRNN.forward (bvrnn.py:86-160): the training-time pass, forward values only --------------------
// One frame conditioned on state `sel` (0: h, the teacher-forced state; 1: h2, the state fed with generated
// features).  h2 lives in part_i (the side-branch buffer, unused here), both states ping-pong by frame parity.
std::vector<StepNode> build_forward_step(const bvc_model *m, const Workspace &w, int B, int sel, bool greedy,
                                         bool update_h, bool update_h2) {
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    std::vector<StepNode> plan;
    const long long MH = (long long)((B + 15) / 16) * 16 * H;
    float *hb[2] = {w.hbuf, w.part_i};
    auto cur = [&](int which) { return dp_parity(hb[which], H, MH, 0, 1); };
    auto nxt = [&](int which) { return dp_parity(hb[which] + MH, H, -MH, 0, 1); };
    float *e1 = w.step[0], *e2 = w.step[1];
    float *pz1 = w.step[2], *pz2 = w.step[3], *pz3 = w.step[4];
    float *d1 = w.step[5], *d2 = w.step[6], *d3 = w.step[7], *dn = w.step[8];
    float *g1 = w.step[9], *g2 = w.step[10], *g3 = w.step[11];
    float *q1 = w.step[12], *q2 = w.step[13];
    auto S = [&](float *p, int ld) { return dp_static(p, ld, 1); };
    int node = 0;
    auto K = [&](GemmParams p, int epi) {
        p.desc = w.desc; p.node = node++; p.probe = nullptr;
        finish(p);
        plan.push_back(StepNode{OP_KERNEL, BR_MAIN, -1, p, epi});
    };
    const DynPtr hs = cur(sel);
    // enc_t and the sample (bvrnn.py:115-129)
    K(lin2_params(m->enc[0], dp_frame(DS_PX, H, 0, 1), H, hs, H, B, S(e1, H)), EPI_ELU);
    K(lin_params(m->enc[1], S(e1, H), B, S(e2, H)), EPI_ELU);
    {
        GemmParams p = lin_params(m->enc[2], S(e2, H), B, dp_frame(DS_CODES, Z));
        p.var_bit = m->cfg.var_bit;
        p.sample = greedy ? CS_GREEDY : CS_SAMPLE;
        p.aux = dp_frame(DS_BITS, 1);
        p.y2 = greedy ? dp_null() : dp_frame(DS_NOISE, Z);
        p.y3 = dp_frame(DS_PROB, Z);
        K(p, EPI_CODE);
    }
    // prior_t (bvrnn.py:116,119)
    K(lin_params(m->prior[0], hs, B, S(q1, H)), EPI_ELU);
    K(lin_params(m->prior[1], S(q1, H), B, S(q2, H)), EPI_ELU);
    K(lin_params(m->prior[2], S(q2, H), B, dp_frame(DS_PRIOR, Z)), EPI_SIGMOID);
    // phi_z, dec (bvrnn.py:131-137)
    K(lin_params(m->phi_z[0], dp_frame(DS_CODES, Z), B, S(pz1, H)), EPI_ELU);
    K(lin_params(m->phi_z[1], S(pz1, H), B, S(pz2, H)), EPI_ELU);
    K(lin_params(m->phi_z[2], S(pz2, H), B, S(pz3, H)), EPI_ELU);
    K(lin2_params(m->dec[0], S(pz3, H), H, hs, H, B, S(d1, H)), EPI_ELU);
    K(lin_params(m->dec[1], S(d1, H), B, S(d2, H)), EPI_ELU);
    K(lin_params(m->dec[2], S(d2, H), B, S(d3, H)), EPI_ELU);
    {
        GemmParams p = lin_params(m->dec[3], S(d3, H), B, dp_frame(DS_MEL, X));
        p.y2 = S(dn, X); p.mean = m->mean_mel; p.stdv = m->std_mel;
        K(p, EPI_MEL);
    }
    auto gru = [&](DynPtr xin, int which) {
        GemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = B; p.N = H; p.gate_rows = H;
        p.y = nxt(which);
        p.y2 = dp_null();
        p.aux = cur(which);
        p.nseg = 3;
        p.gate_il = 1;
        p.seg[0] = mkseg(xin, m->w_ih_il, 2 * H / 16, H, 0);
        p.seg[1] = mkseg(S(pz3, H), m->w_ih_il + (size_t)(H / 16) * 3 * 256, 2 * H / 16, H, 0);
        p.seg[2] = mkseg(cur(which), m->w_hh_il, H / 16, H, 1);
        p.bias0 = m->b_ih; p.bias1 = m->b_hh;
        K(p, EPI_GRU);
    };
    if (update_h) gru(dp_frame(DS_PX, H, 0, 1), 0);                 // h  <- GRU([phi_x_t, phi_z_t], h)      bvrnn.py:142-143
    if (update_h2) {                                                 // h2 <- GRU([phi_x_t_gen, phi_z_t], h2) bvrnn.py:139,144-145
        K(lin_params(m->phi_x[0], S(dn, X), B, S(g1, H)), EPI_ELU);
        K(lin_params(m->phi_x[1], S(g1, H), B, S(g2, H)), EPI_ELU);
        K(lin_params(m->phi_x[2], S(g2, H), B, S(g3, H)), EPI_ELU);
        gru(S(g3, H), 1);
    }
    return plan;
}

}  // namespace

namespace bvc {

thread_local bool g_stream_tick = false;
thread_local bool g_tick_flow = false;
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
        const bool fold = (kind & STEP_FOLD) != 0;
        if (d_melhat) {                                   // folded: keep ELU(dec.4) of every frame, dec.6 behind the recurrence; else dec.6's own output
            if (fold) d.p[DS_KEEP_ENC] = w.pxB;
            else d.p[DS_MEL] = d_melhat;
        }
        return run_layers(m, w, ws_base, d, kind, d_h0, B, T, d_hT, fold ? d_melhat : nullptr, s);
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
    const size_t mb = (size_t)((B + 15) / 16) * 16, mk = (size_t)((K * B + 15) / 16) * 16;
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
    v->total = off;
}

// BVRNN.encode with the bits of every frame chosen inside the frame (build_vbr_step).  Always the launch-per-layer schedule, whatever
// `recurrence` says: the persistent kernel has no candidate rows.  h_ladder: K ascending bit counts, checked by the caller.
int run_encode_vbr(const bvc_model *m, const Workspace &w, const VbrWorkspace &v, void *ws_base, const float *d_mel, const float *d_tau,
                   const int *h_ladder, int K, const float *d_h0, int B, int64_t T, float *d_codes, float *d_bits, float *d_all_h,
                   float *d_hT, float *d_prob, float *d_dist, float *d_dec, hipStream_t s) {
    return end_call(s, [&]() -> int {
        const int H = m->cfg.h_dim;
        const long long MH = (long long)((B + 15) / 16) * 16 * H;
        int rc;
        if ((rc = launch_normalize_rows(d_mel, m->mean_mel, m->std_mel, (long long)B * T, m->cfg.num_mels, w.yn, s))) return rc;
        if ((rc = encode_prologue(m, w, B, T, s))) return rc;
        if ((rc = launch_fill(v.zraw, 0.0f, (long long)v.floats, s))) return rc;      // rows of a fragment behind the last candidate read as zeros
        VbrCall c;
        memset(&c, 0, sizeof(c));
        c.y = d_mel; c.tau = d_tau; c.codes = d_codes; c.bits = d_bits; c.dist = d_dist; c.dec = d_dec;
        for (int k = 0; k < K; ++k) c.ladder[k] = h_ladder[k];
        if ((rc = launch_vbr_set_call(v.call, c, s))) return rc;
        CallDesc d;
        memset(&d, 0, sizeof(d));
        d.p[DS_PARTD] = w.part_dec0; d.p[DS_PROB] = d_prob; d.p[DS_ALLH] = d_all_h;
        d.T = T;
        if ((rc = d_h0 ? launch_repack_rows(d_h0, w.hbuf, H, B, H, 0, s) : launch_fill(w.hbuf, 0.0f, MH, s))) return rc;
        if (d_all_h && (rc = launch_repack_rows(w.hbuf, d_all_h, (long long)T * H, B, H, 1, s))) return rc;      // all_h[:, 0] = h0
        const std::vector<StepNode> plan = build_vbr_step(m, w, v, B, K);
        if ((rc = begin_call(m, w, d, count_kernels(plan), s))) return rc;
        if ((rc = run_recurrence(m, w, ws_base, B, T, STEP_ENCODE_VBR | (K << STEP_RUNGS_SHIFT), plan, s))) return rc;
        if (d_hT && (rc = launch_repack_rows(w.hbuf + (T & 1) * MH, d_hT, H, B, H, 1, s))) return rc;
        return BVC_OK;
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
        d.p[DS_MEL] = d_mel;
        const int kind = (pre ? STEP_DECODE_PRE : STEP_DECODE) | step_fold(m, false);
        const bool fold = (kind & STEP_FOLD) != 0;
        if (fold) d.p[DS_KEEP] = w.pxB;                   // (idle once the batched phi_z layers are through)
        return run_layers(m, w, ws_base, d, kind, d_h0, B, T, d_hT, fold ? d_mel : nullptr, s);
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
        const bool fold = (kind & STEP_FOLD) != 0;
        if (fold) d.p[DS_KEEP_ENC] = w.pxB;               // ELU(dec.4) of every frame; dec.6, the decoder's output, behind the recurrence
        else d.p[DS_MEL] = d_mel;
        return run_layers(m, w, ws_base, d, kind, d_h0, B, T, d_hT, fold ? d_mel : nullptr, s);
    });
}

int run_forward(const bvc_model *m, const Workspace &w, const float *d_mel, const float *d_bits,
                const uint8_t *h_use_gen, bool update_h, bool update_h2, const float *d_noise, int B, int64_t T,
                float *d_dec, float *d_kld, float *d_z, float *d_prob, float *d_prior, hipStream_t s) {
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
    const long long MH = (long long)((B + 15) / 16) * 16 * H;
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
    const bool kp = g_kprobe.enabled;                 // the in-kernel probes index by a fixed kernel count per step
    g_kprobe.enabled = false;
    rc = begin_call(m, w, d, count_kernels(plan0), s);
    for (int64_t t = 0; !rc && t < T; ++t) rc = launch_steps(m, h_use_gen[t] ? plan1 : plan0, w, 1, s, nullptr);
    g_kprobe.enabled = kp;
    if (rc) return rc;
    return launch_kld_frames(prob, prior, m->cfg.var_bit ? d_bits : nullptr, B, T, Z, d_kld, s);
}

}  // namespace bvc

extern "C" {

int bvc_flow_fence(void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    BVC_HIP_TRY(hipStreamIsCapturing(s, &cs));
    if (cs != hipStreamCaptureStatusNone) { set_error("bvc_flow_fence: not while the stream is being captured"); return BVC_EINVAL; }
    int dev = 0;
    BVC_HIP_TRY(hipGetDevice(&dev));
    dev &= 15;
    std::lock_guard<std::mutex> lk(g_flow_mu);
    FlowFence &f = g_fence[dev][g_fence_n[dev]++ % FLOW_FENCES];
    if (!f.ev) BVC_HIP_TRY(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    // a slot that is still pending holds a fence nobody has waited for yet (more than FLOW_FENCES fences without a persistent launch in
    // between): order this stream behind it first, so that the new record implies the old one
    if (f.pending) BVC_HIP_TRY(hipStreamWaitEvent(s, f.ev, 0));
    BVC_HIP_TRY(hipEventRecord(f.ev, s));
    f.pending = true;
    return BVC_OK;
}

}  // extern "C"
