// The backward pass of BVRNN.forward (bvc_bvrnn_backward): the vector-Jacobian product of run_forward at the gradients of a loss with
// respect to all_dec_mean and to the scalar kld, for the 36 trainable tensors and, on request, the input mel.
//
//   forward with a tape   run_forward itself (the same launches, so the same bits), every frame into scratch vectors and states of its
//                         own; the tape is then unpacked into natural matrices with frame-major rows t * B + b
//   reverse recurrence    frame T-1 down to 0, carrying d h and d h2.  dX = dY W is the recurrent-layer kernel as it stands (EPI_LINEAR)
//                         over the fragment-packed TRANSPOSED weight; its addend sums what meets at one tensor.  The activations, the
//                         sampler with the KLD, the mel normalisation and the GRU cell are the row-wise kernels of k_backward.hip; the
//                         GRU's gate sums and the two logits are computed again from the tape, and every sigmoid's p and 1 - p from
//                         those, each to its own precision.  Every layer's pre-activation gradient dY is
//                         kept for all frames.
//   all frames at once    d phi_x of all frames back through phi_x.4 / .2 / .0 (batched GEMM on the transposed natural weights), and
//                         every weight gradient dW = dY^T X (launch_weight_grad) with its bias gradient (column sums) - one launch per
//                         tensor over all T B rows (the GRU's and phi_x's over the rows of both their uses), in a fixed order.
// Nothing accumulates into d_grads: every tensor is written once.  No atomics anywhere, so two calls give the same bits.
#include "recurrence.h"

using namespace bvc;

namespace {

enum { L_PX0, L_PX2, L_PX4, L_PZ0, L_PZ2, L_PZ4, L_EN0, L_EN2, L_EN4, L_PR0, L_PR2, L_PR4, L_DE0, L_DE2, L_DE4, L_DE6, L_WIH, L_WHH, L_COUNT };
// the step scratch vectors in tape order (Workspace::step as StepBuilder names them)
enum { TS_E1, TS_E2, TS_PZ1, TS_PZ2, TS_PZ3, TS_D1, TS_D2, TS_D3, TS_DN, TS_G1, TS_G2, TS_G3, TS_Q1, TS_Q2 };

size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// The workspace behind the ordinary one.  Stacked matrices (2 T B rows) hold the teacher-forced use in rows [0, T B) and the
// generated-feature use in [T B, 2 T B): phi_x's layers (all frames | inside the frame) and the GRU (chain h | chain h2).
struct Bwd {
    float *tape; size_t slot;
    float *state[2];
    float *dec, *kld, *z, *prob, *prior;                   // the forward outputs the caller did not ask for
    float *YD, *P[3], *E[2], *Q[2], *PZ[3], *D[3], *Zf, *HS, *Hh;       // layer inputs X
    float *EL, *QL;                                        // the encoder's and the prior's logits of all frames, computed again
    float *dP[3], *dE[2], *dQ[2], *dPZ[3], *dD[3], *dEL, *dQL, *dDD, *dGI, *dGH;     // pre-activation gradients dY
    float *GI, *GH, *dH[2][2], *dHdir, *gPZ[2], *gHS[2], *gDN, *gZ, *gYN, *wg;
    size_t total;
};

void carve_backward(const bvc_model *m, int B, int64_t T, char *base, Bwd *b) {
    const size_t H = m->cfg.h_dim, X = m->cfg.num_mels, Z = m->cfg.z_dim;
    const size_t TB = (size_t)B * (size_t)T, mt16 = pad16((size_t)B), vmax = std::max(H, X);
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float *p = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(base) + off);
        off += up256(nfloats * sizeof(float));
        return p;
    };
    b->slot = up256(mt16 * vmax * sizeof(float)) / sizeof(float);
    b->tape = take((size_t)T * FORWARD_TAPE_SLOTS * b->slot);
    b->state[0] = take(2 * ((size_t)T + 1) * mt16 * H);
    b->state[1] = b->state[0] + ((size_t)T + 1) * mt16 * H;
    b->dec = take(TB * X); b->kld = take((size_t)T); b->z = take(TB * Z); b->prob = take(TB * Z); b->prior = take(TB * Z);
    b->YD = take(2 * TB * X);
    for (int i = 0; i < 3; ++i) b->P[i] = take(2 * TB * H);
    for (int i = 0; i < 2; ++i) { b->E[i] = take(TB * H); b->Q[i] = take(TB * H); }
    b->PZ[0] = take(TB * H); b->PZ[1] = take(TB * H); b->PZ[2] = take(2 * TB * H);
    for (int i = 0; i < 3; ++i) b->D[i] = take(TB * H);
    b->Zf = take(TB * Z); b->HS = take(TB * H); b->Hh = take(2 * TB * H);
    b->EL = take(TB * Z); b->QL = take(TB * Z);
    for (int i = 0; i < 3; ++i) b->dP[i] = take(2 * TB * H);
    for (int i = 0; i < 2; ++i) { b->dE[i] = take(TB * H); b->dQ[i] = take(TB * H); }
    for (int i = 0; i < 3; ++i) { b->dPZ[i] = take(TB * H); b->dD[i] = take(TB * H); }
    b->dEL = take(TB * Z); b->dQL = take(TB * Z); b->dDD = take(TB * X);
    b->dGI = take(2 * TB * 3 * H); b->dGH = take(2 * TB * 3 * H);
    b->GI = take((size_t)B * 3 * H); b->GH = take((size_t)B * 3 * H);
    for (int c = 0; c < 2; ++c) for (int i = 0; i < 2; ++i) b->dH[c][i] = take((size_t)B * H);
    b->dHdir = take((size_t)B * H);
    for (int i = 0; i < 2; ++i) { b->gPZ[i] = take((size_t)B * H); b->gHS[i] = take((size_t)B * H); }
    b->gDN = take((size_t)B * X); b->gZ = take((size_t)B * Z); b->gYN = take(TB * X);
    // the chunk sums of a weight gradient: chunks <= ceil(512 / tiles) + 1 and tiles * 4096 >= N K, so chunks * N K <= 512 * 4096 + N K
    b->wg = take((size_t)512 * 4096 + 6 * H * H + 3 * H * X);
    b->total = off;
}

const char *const GRAD_NAMES[GRAD_ENTRIES] = {
    "phi_x.0.weight", "phi_x.0.bias", "phi_x.2.weight", "phi_x.2.bias", "phi_x.4.weight", "phi_x.4.bias",
    "phi_z.0.weight", "phi_z.0.bias", "phi_z.2.weight", "phi_z.2.bias", "phi_z.4.weight", "phi_z.4.bias",
    "enc.0.weight", "enc.0.bias", "enc.2.weight", "enc.2.bias", "enc.4.weight", "enc.4.bias",
    "prior.0.weight", "prior.0.bias", "prior.2.weight", "prior.2.bias", "prior.4.weight", "prior.4.bias",
    "dec.0.weight", "dec.0.bias", "dec.2.weight", "dec.2.bias", "dec.4.weight", "dec.4.bias", "dec.6.weight", "dec.6.bias",
    "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"};

// y (M, N) = x (M, K = lt.in) W[:, n0 : n0 + N] (+ add): a forward layer over rows n0 .. of the transposed weight
int dx(const bvc_model *m, const Linear &lt, int n0, int N, const float *x, int M, float *y, const float *add, hipStream_t s) {
    GemmParams p = mat_params(dp_static(x, lt.in), lt.wp + (size_t)(n0 / 16) * (lt.in / 16) * 256, lt.in / 16, lt.in, M, N, nullptr, dp_static(y, N));
    if (add) p.aux = dp_static(add, N);
    return launch_gemm_skinny(p, EPI_LINEAR, s, m->mtw);
}

}  // namespace

namespace bvc {

int grad_layout(const bvc_config &c, GradEntry *out, long long *total) {
    const long long H = c.h_dim, X = c.num_mels, Z = c.z_dim;
    const long long shape[16][2] = {{H, X}, {H, H}, {H, H}, {H, Z}, {H, H}, {H, H}, {H, 2 * H}, {H, H}, {Z, H}, {H, H}, {H, H}, {Z, H},
                                    {H, 2 * H}, {H, H}, {H, H}, {X, H}};       // (out, in) in GRAD_NAMES order
    long long off = 0;
    int n = 0;
    auto put = [&](long long numel) { if (out) out[n] = GradEntry{GRAD_NAMES[n], off, numel}; off += numel; ++n; };
    for (int i = 0; i < 16; ++i) { put(shape[i][0] * shape[i][1]); put(shape[i][0]); }
    put(3 * H * 2 * H); put(3 * H * H); put(3 * H); put(3 * H);
    if (total) *total = off;
    return n;
}

size_t backward_extra_bytes(const bvc_model *m, int B, int64_t T) {
    Bwd b;
    carve_backward(m, B, T, nullptr, &b);
    return b.total;
}

// The transposed weights, once per model: W (out, in) -> natural (in, out) and its fragment-packing.  Synchronises the stream once, so
// that a later call on another stream finds them complete.
int backward_prepare(const bvc_model *m, hipStream_t s) {
    std::lock_guard<std::mutex> lk(m->bwd_mu);
    if (m->bwd_ready) return BVC_OK;
    if (capture_state(s) != CAP_NONE) { set_error("bvc_bvrnn_backward: call bvc_bvrnn_backward_prepare before capturing the first call"); return BVC_EINVAL; }
    const int H = m->cfg.h_dim;
    auto alloc = [&](size_t nfloats, float **p) -> int {
        BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), nfloats * sizeof(float)));
        m->bwd_allocs.push_back(*p);
        return BVC_OK;
    };
    auto make = [&](const float *w_nat, int out, int in, Linear *lt) -> int {
        float *t = nullptr, *p = nullptr;
        int rc;
        if ((rc = alloc((size_t)in * out, &t)) || (rc = alloc((size_t)in * out, &p))) return rc;
        if ((rc = launch_transpose(w_nat, out, in, t, s))) return rc;
        if ((rc = launch_repack_rows(t, p, out, in, out, 0, s))) return rc;
        lt->w = t; lt->wp = p; lt->b = nullptr; lt->in = out; lt->out = in;
        return BVC_OK;
    };
    int rc = BVC_OK;
    const Linear *groups[5] = {m->phi_x, m->phi_z, m->enc, m->prior, m->dec};
    for (int g = 0, k = 0; g < 5 && !rc; ++g)
        for (int i = 0; i < (g == 4 ? 4 : 3) && !rc; ++i, ++k) rc = make(groups[g][i].w, groups[g][i].out, groups[g][i].in, &m->bwd_t[k]);
    if (!rc) rc = make(m->w_ih_nat, 3 * H, 2 * H, &m->bwd_t[L_WIH]);
    float *whh = nullptr;
    if (!rc) rc = alloc((size_t)3 * H * H, &whh);
    if (!rc) rc = launch_repack_rows(m->w_hh, whh, H, 3 * H, H, 1, s);        // (the model keeps W_hh packed only)
    if (!rc) rc = make(whh, 3 * H, H, &m->bwd_t[L_WHH]);
    if (rc) return rc;
    BVC_HIP_TRY(hipStreamSynchronize(s));
    m->bwd_ready = true;
    return BVC_OK;
}

int run_backward(const bvc_model *m, const Workspace &w, char *extra, const BackwardCall &c, hipStream_t s) {
    const int H = m->cfg.h_dim, X = m->cfg.num_mels, Z = m->cfg.z_dim, B = c.B;
    const int64_t T = c.T;
    const size_t TB = (size_t)B * (size_t)T;
    const long long MH = (long long)pad16(B) * H;
    int rc;
    if ((rc = backward_prepare(m, s))) return rc;
    Bwd b;
    carve_backward(m, B, T, extra, &b);
    const Linear *lt = m->bwd_t;
    float *z = c.d_z ? c.d_z : b.z, *prob = c.d_prob ? c.d_prob : b.prob, *prior = c.d_prior ? c.d_prior : b.prior;

    // ---- forward with a tape
    if ((rc = launch_fill(b.state[0], 0.0f, 2 * (T + 1) * MH, s))) return rc;
    const ForwardTapeSpec spec = {b.tape, b.slot, {b.state[0], b.state[1]}};
    if ((rc = run_forward(m, w, c.d_mel, c.d_bits, c.h_use_gen, c.update_h, c.update_h2, c.d_noise, B, T, c.d_dec ? c.d_dec : b.dec,
                          c.d_kld ? c.d_kld : b.kld, z, prob, prior, s, &spec)))
        return rc;
    auto untape = [&](int k, int n, float *dst) { return launch_unpack_frames(b.tape + (size_t)k * b.slot, (long long)FORWARD_TAPE_SLOTS * b.slot, T, B, n, dst, s); };
    if ((rc = untape(TS_E1, H, b.E[0])) || (rc = untape(TS_E2, H, b.E[1])) || (rc = untape(TS_Q1, H, b.Q[0])) || (rc = untape(TS_Q2, H, b.Q[1]))) return rc;
    for (int i = 0; i < 3; ++i)
        if ((rc = untape(TS_PZ1 + i, H, b.PZ[i])) || (rc = untape(TS_D1 + i, H, b.D[i]))) return rc;
    if ((rc = forward_tape_phi_x(m, w, B, T, b.P[0], b.P[1], b.P[2], s))) return rc;
    if ((rc = launch_reorder_rows(w.yn, B, T, X, b.YD, 0, nullptr, s))) return rc;
    if ((rc = launch_reorder_rows(z, B, T, Z, b.Zf, 0, nullptr, s))) return rc;
    // the logits behind enc_t and prior_t (the forward keeps the probabilities only, and 1 - p from a rounded p has lost the precision
    // the derivative p (1 - p) of a saturated unit needs)
    if ((rc = launch_gemm_batched(b.E[1], H, m->enc[2].w, H, m->enc[2].b, (int)TB, Z, H, 0, b.EL, Z, s))) return rc;
    if ((rc = launch_gemm_batched(b.Q[1], H, m->prior[2].w, H, m->prior[2].b, (int)TB, Z, H, 0, b.QL, Z, s))) return rc;
    if (c.update_h2) {
        if ((rc = untape(TS_DN, X, b.YD + TB * X))) return rc;
        for (int i = 0; i < 3; ++i) if ((rc = untape(TS_G1 + i, H, b.P[i] + TB * H))) return rc;
        BVC_HIP_TRY(hipMemcpyAsync(b.PZ[2] + TB * H, b.PZ[2], TB * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    for (int ch = 0; ch < 2; ++ch)
        if ((rc = launch_unpack_frames(b.state[ch], MH, T, B, H, b.Hh + ch * TB * H, s))) return rc;
    for (int64_t t = 0; t < T; ++t)      // the state every frame's networks read
        BVC_HIP_TRY(hipMemcpyAsync(b.HS + (size_t)t * B * H, b.Hh + ((c.h_use_gen[t] ? TB : 0) + (size_t)t * B) * H, (size_t)B * H * sizeof(float),
                                   hipMemcpyDeviceToDevice, s));

    // ---- the reverse recurrence
    const float *bits = m->cfg.var_bit ? c.d_bits : nullptr;
    const float scale = c.g_kld / ((float)T * (float)B);
    int cur[2] = {0, 0};
    for (int ch = 0; ch < 2; ++ch) if ((rc = launch_fill(b.dH[ch][0], 0.0f, (long long)B * H, s))) return rc;
    const long long BH = (long long)B * H;
    // one chain's GRU cell at frame t: rows r of the stacked matrices; x1 = its phi_x input.  Leaves d h_t (through the cell) in the
    // chain's carry, d x1 in dP[2] rows r, and adds d phi_z to gpz
    const float *gpz = nullptr;
    int pzi = 0;
    auto gru_cell = [&](int ch, size_t r, size_t o) -> int {
        const float *x1 = b.P[2] + r * H, *x2 = b.PZ[2] + o * H, *h = b.Hh + r * H;
        float *dgi = b.dGI + r * 3 * H, *dgh = b.dGH + r * 3 * H;
        int e;
        GemmParams p = mat_params(dp_static(x1, H), m->w_ih, 2 * H / 16, H, B, 3 * H, m->b_ih, dp_static(b.GI, 3 * H));
        p.nseg = 2;
        p.seg[1] = mkseg(dp_static(x2, H), m->w_ih + (size_t)(H / 16) * 256, 2 * H / 16, H, 0);
        finish(p);
        if ((e = launch_gemm_skinny(p, EPI_LINEAR, s, m->mtw))) return e;
        if ((e = launch_gemm_skinny(mat_params(dp_static(h, H), m->w_hh, H / 16, H, B, 3 * H, m->b_hh, dp_static(b.GH, 3 * H)), EPI_LINEAR, s, m->mtw))) return e;
        if ((e = launch_gru_bwd(b.dH[ch][cur[ch]], b.GI, b.GH, h, B, H, dgi, dgh, b.dHdir, s))) return e;
        if ((e = dx(m, lt[L_WHH], 0, H, dgh, B, b.dH[ch][cur[ch] ^ 1], b.dHdir, s))) return e;
        cur[ch] ^= 1;
        if ((e = dx(m, lt[L_WIH], 0, H, dgi, B, b.dP[2] + r * H, nullptr, s))) return e;
        if ((e = dx(m, lt[L_WIH], H, H, dgi, B, b.gPZ[pzi], gpz, s))) return e;
        gpz = b.gPZ[pzi]; pzi ^= 1;
        return BVC_OK;
    };
    // dY -> ELU' in place -> through the transposed layer
    auto back = [&](int layer, int N, float *dy, const float *y, long long n, float *out) -> int {
        if (int e = launch_elu_bwd(dy, y, dy, n, s)) return e;
        return dx(m, lt[layer], 0, N, dy, B, out, nullptr, s);
    };
    for (int64_t t = T - 1; t >= 0; --t) {
        const size_t o = (size_t)t * B, r2 = TB + o;
        const int sel = c.h_use_gen[t] ? 1 : 0;
        gpz = nullptr;
        const float *gdn = nullptr;
        bool px_written = false;
        if (c.update_h2) {      // h2 <- GRU([phi_x(norm(dec_t)), phi_z_t], h2): back to dec_t through the frame's own phi_x
            if ((rc = gru_cell(1, r2, o))) return rc;
            if ((rc = back(L_PX4, H, b.dP[2] + r2 * H, b.P[2] + r2 * H, BH, b.dP[1] + r2 * H))) return rc;
            if ((rc = back(L_PX2, H, b.dP[1] + r2 * H, b.P[1] + r2 * H, BH, b.dP[0] + r2 * H))) return rc;
            if ((rc = back(L_PX0, X, b.dP[0] + r2 * H, b.P[0] + r2 * H, BH, b.gDN))) return rc;
            gdn = b.gDN;
        }
        if (c.update_h) {       // h <- GRU([phi_x_t, phi_z_t], h)
            if ((rc = gru_cell(0, o, o))) return rc;
            px_written = true;
        }
        // dec.6 .. dec.0 over [phi_z, hs]
        if ((rc = launch_mel_bwd(c.d_gdec, T, t, gdn, m->std_mel, B, X, b.dDD + o * X, s))) return rc;
        if ((rc = dx(m, lt[L_DE6], 0, H, b.dDD + o * X, B, b.dD[2] + o * H, nullptr, s))) return rc;
        if ((rc = back(L_DE4, H, b.dD[2] + o * H, b.D[2] + o * H, BH, b.dD[1] + o * H))) return rc;
        if ((rc = back(L_DE2, H, b.dD[1] + o * H, b.D[1] + o * H, BH, b.dD[0] + o * H))) return rc;
        if ((rc = launch_elu_bwd(b.dD[0] + o * H, b.D[0] + o * H, b.dD[0] + o * H, BH, s))) return rc;
        if ((rc = dx(m, lt[L_DE0], 0, H, b.dD[0] + o * H, B, b.gPZ[pzi], gpz, s))) return rc;
        gpz = b.gPZ[pzi]; pzi ^= 1;
        if ((rc = dx(m, lt[L_DE0], H, H, b.dD[0] + o * H, B, b.gHS[0], b.dH[sel][cur[sel]], s))) return rc;
        // phi_z.4 .. phi_z.0, the sample and the KLD
        if ((rc = launch_elu_bwd(gpz, b.PZ[2] + o * H, b.dPZ[2] + o * H, BH, s))) return rc;
        if ((rc = dx(m, lt[L_PZ4], 0, H, b.dPZ[2] + o * H, B, b.dPZ[1] + o * H, nullptr, s))) return rc;
        if ((rc = back(L_PZ2, H, b.dPZ[1] + o * H, b.PZ[1] + o * H, BH, b.dPZ[0] + o * H))) return rc;
        if ((rc = back(L_PZ0, Z, b.dPZ[0] + o * H, b.PZ[0] + o * H, BH, b.gZ))) return rc;
        if ((rc = launch_code_bwd(b.gZ, b.EL + o * Z, b.QL + o * Z, bits, T, t, B, Z, scale, b.dEL + o * Z, b.dQL + o * Z, s))) return rc;
        // enc.4 .. enc.0 over [phi_x_t, hs]
        if ((rc = dx(m, lt[L_EN4], 0, H, b.dEL + o * Z, B, b.dE[1] + o * H, nullptr, s))) return rc;
        if ((rc = back(L_EN2, H, b.dE[1] + o * H, b.E[1] + o * H, BH, b.dE[0] + o * H))) return rc;
        if ((rc = launch_elu_bwd(b.dE[0] + o * H, b.E[0] + o * H, b.dE[0] + o * H, BH, s))) return rc;
        if ((rc = dx(m, lt[L_EN0], 0, H, b.dE[0] + o * H, B, b.dP[2] + o * H, px_written ? b.dP[2] + o * H : nullptr, s))) return rc;
        if ((rc = dx(m, lt[L_EN0], H, H, b.dE[0] + o * H, B, b.gHS[1], b.gHS[0], s))) return rc;
        // prior.4 .. prior.0 over hs; the sum is the carry of the chain the frame was conditioned on
        if ((rc = dx(m, lt[L_PR4], 0, H, b.dQL + o * Z, B, b.dQ[1] + o * H, nullptr, s))) return rc;
        if ((rc = back(L_PR2, H, b.dQ[1] + o * H, b.Q[1] + o * H, BH, b.dQ[0] + o * H))) return rc;
        if ((rc = launch_elu_bwd(b.dQ[0] + o * H, b.Q[0] + o * H, b.dQ[0] + o * H, BH, s))) return rc;
        if ((rc = dx(m, lt[L_PR0], 0, H, b.dQ[0] + o * H, B, b.dH[sel][cur[sel] ^ 1], b.gHS[1], s))) return rc;
        cur[sel] ^= 1;
    }

    // ---- all frames at once: phi_x of the input, then every weight and bias gradient
    const long long NTB = (long long)TB * H;
    if ((rc = launch_elu_bwd(b.dP[2], b.P[2], b.dP[2], NTB, s))) return rc;
    if ((rc = launch_gemm_batched(b.dP[2], H, lt[L_PX4].w, H, nullptr, (int)TB, H, H, 0, b.dP[1], H, s))) return rc;
    if ((rc = launch_elu_bwd(b.dP[1], b.P[1], b.dP[1], NTB, s))) return rc;
    if ((rc = launch_gemm_batched(b.dP[1], H, lt[L_PX2].w, H, nullptr, (int)TB, H, H, 0, b.dP[0], H, s))) return rc;
    if ((rc = launch_elu_bwd(b.dP[0], b.P[0], b.dP[0], NTB, s))) return rc;
    if (c.d_gmel) {
        if ((rc = launch_gemm_batched(b.dP[0], H, lt[L_PX0].w, H, nullptr, (int)TB, X, H, 0, b.gYN, X, s))) return rc;
        if ((rc = launch_reorder_rows(b.gYN, B, T, X, c.d_gmel, 1, m->std_mel, s))) return rc;
    }
    GradEntry ge[GRAD_ENTRIES];
    grad_layout(m->cfg, ge, nullptr);
    // entry 2 i: the weight of linear i (N, K total), entry 2 i + 1 its bias; X0 / X1: the (one or two) parts of its input, K0 columns first
    auto linear_grads = [&](int i, const float *dy, int M, int N, const float *x0, int K0, const float *x1, int K1) -> int {
        float *gw = c.d_grads + ge[2 * i].offset;
        int e;
        if ((e = launch_weight_grad(dy, x0, M, N, K0, gw, b.wg, s, K0 + K1))) return e;
        if (x1 && (e = launch_weight_grad(dy, x1, M, N, K1, gw + K0, b.wg, s, K0 + K1))) return e;
        return launch_col_sum(dy, M, N, c.d_grads + ge[2 * i + 1].offset, s);
    };
    const int M1 = (int)TB, Mp = c.update_h2 ? 2 * M1 : M1;
    if ((rc = linear_grads(L_PX0, b.dP[0], Mp, H, b.YD, X, nullptr, 0)) || (rc = linear_grads(L_PX2, b.dP[1], Mp, H, b.P[0], H, nullptr, 0)) ||
        (rc = linear_grads(L_PX4, b.dP[2], Mp, H, b.P[1], H, nullptr, 0)))
        return rc;
    if ((rc = linear_grads(L_PZ0, b.dPZ[0], M1, H, b.Zf, Z, nullptr, 0)) || (rc = linear_grads(L_PZ2, b.dPZ[1], M1, H, b.PZ[0], H, nullptr, 0)) ||
        (rc = linear_grads(L_PZ4, b.dPZ[2], M1, H, b.PZ[1], H, nullptr, 0)))
        return rc;
    if ((rc = linear_grads(L_EN0, b.dE[0], M1, H, b.P[2], H, b.HS, H)) || (rc = linear_grads(L_EN2, b.dE[1], M1, H, b.E[0], H, nullptr, 0)) ||
        (rc = linear_grads(L_EN4, b.dEL, M1, Z, b.E[1], H, nullptr, 0)))
        return rc;
    if ((rc = linear_grads(L_PR0, b.dQ[0], M1, H, b.HS, H, nullptr, 0)) || (rc = linear_grads(L_PR2, b.dQ[1], M1, H, b.Q[0], H, nullptr, 0)) ||
        (rc = linear_grads(L_PR4, b.dQL, M1, Z, b.Q[1], H, nullptr, 0)))
        return rc;
    if ((rc = linear_grads(L_DE0, b.dD[0], M1, H, b.PZ[2], H, b.HS, H)) || (rc = linear_grads(L_DE2, b.dD[1], M1, H, b.D[0], H, nullptr, 0)) ||
        (rc = linear_grads(L_DE4, b.dD[2], M1, H, b.D[1], H, nullptr, 0)) || (rc = linear_grads(L_DE6, b.dDD, M1, X, b.D[2], H, nullptr, 0)))
        return rc;
    // the GRU: the rows of the chains that ran
    const size_t r0 = c.update_h ? 0 : TB;
    const int Mg = (c.update_h ? M1 : 0) + (c.update_h2 ? M1 : 0);
    const float *dgi = b.dGI + r0 * 3 * H, *dgh = b.dGH + r0 * 3 * H;
    float *g_ih = c.d_grads + ge[32].offset;
    if ((rc = launch_weight_grad(dgi, b.P[2] + r0 * H, Mg, 3 * H, H, g_ih, b.wg, s, 2 * H))) return rc;
    if ((rc = launch_weight_grad(dgi, b.PZ[2] + r0 * H, Mg, 3 * H, H, g_ih + H, b.wg, s, 2 * H))) return rc;
    if ((rc = launch_weight_grad(dgh, b.Hh + r0 * H, Mg, 3 * H, H, c.d_grads + ge[33].offset, b.wg, s))) return rc;
    if ((rc = launch_col_sum(dgi, Mg, 3 * H, c.d_grads + ge[34].offset, s))) return rc;
    return launch_col_sum(dgh, Mg, 3 * H, c.d_grads + ge[35].offset, s);
}

}  // namespace bvc
