// The optimiser of the mel coder (include/bvcodec.h): bvc_bvrnn_params_get / _set, which read and rewrite a live model's 36 trainable
// tensors as one flat device buffer in bvc_bvrnn_grad_layout order, and bvc_optimizer_*, an AdamW step on that buffer from the flat
// gradients bvc_bvrnn_backward writes.  A rewrite goes to EVERY form of the weights the model's kernels read - what build_bvrnn
// (model_build.hip) uploads, and the transposed copies of backward_prepare (backward.hip) once they exist - at the addresses they
// already have, stream-ordered: the next call on any schedule, a captured step graph included, runs on the new values, and the model
// is bit for bit the one bvc_model_create builds from them.  The kernels are k_optimizer.hip's, launch_repack_rows and
// launch_transpose.  Host only.
#include <cmath>
#include <initializer_list>
#include <memory>

#include "recurrence.h"

using namespace bvc;

struct bvc_optimizer {
    bvc_model *m = nullptr;
    long long total = 0;
    int64_t step = 0;
    float *exp_avg = nullptr, *exp_avg_sq = nullptr;
    double *partial = nullptr;         // the norm's chunk sums
    float *scal = nullptr;             // [0] the clip factor, [1] the norm
    ~bvc_optimizer() {
        for (void *p : {(void *)exp_avg, (void *)exp_avg_sq, (void *)partial, (void *)scal})
            if (p) (void)hipFree(p);
    }
};

namespace {

enum { E_WIH = 32, E_WHH = 33, E_BIH = 34, E_BHH = 35, E_PX0 = 0, E_DE6 = 30 };

struct Layout { GradEntry e[GRAD_ENTRIES]; long long total; };
Layout layout_of(const bvc_model *m) {
    Layout l;
    grad_layout(m->cfg, l.e, &l.total);
    return l;
}

// the 16 Linears in grad_layout order: entry 2 i is the weight of lin[i], entry 2 i + 1 its bias
void linears(const bvc_model *m, const Linear **lin) {
    const Linear *groups[5] = {m->phi_x, m->phi_z, m->enc, m->prior, m->dec};
    for (int g = 0, k = 0; g < 5; ++g)
        for (int i = 0; i < (g == 4 ? 4 : 3); ++i, ++k) lin[k] = &groups[g][i];
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The tensors the model keeps in their natural layout, to (dir 0) or from (dir 1) the flat buffer: one launch.  W_hh is not among them.
int copy_natural(const bvc_model *m, const Layout &l, float *flat, int dir, hipStream_t s) {
    const Linear *lin[16];
    linears(m, lin);
    CopySegments segs;
    segs.n = 0;
    auto put = [&](const float *model_ptr, int entry) {
        float *f = flat + l.e[entry].offset, *mp = const_cast<float *>(model_ptr);
        segs.s[segs.n++] = dir == 0 ? CopySegment{mp, f, l.e[entry].numel} : CopySegment{f, mp, l.e[entry].numel};
    };
    for (int i = 0; i < 16; ++i) { put(lin[i]->w, 2 * i); put(lin[i]->b, 2 * i + 1); }
    put(m->w_ih_nat, E_WIH); put(m->b_ih, E_BIH); put(m->b_hh, E_BHH);
    return launch_copy_segments(segs, s);
}

int params_get(const bvc_model *m, const Layout &l, float *d_params, hipStream_t s) {
    const int H = m->cfg.h_dim;
    if (int rc = copy_natural(m, l, d_params, 0, s)) return rc;
    return launch_repack_rows(m->w_hh, d_params + l.e[E_WHH].offset, H, 3 * H, H, 1, s);        // (the model keeps W_hh packed only)
}

// every derived form from the master copy, in place
int rewrite(const bvc_model *m, const Layout &l, hipStream_t s) {
    const int H = m->cfg.h_dim, X = m->cfg.num_mels;
    float *P = m->master;
    auto mut = [](const float *p) { return const_cast<float *>(p); };
    int rc;
    if ((rc = copy_natural(m, l, P, 1, s))) return rc;
    const Linear *lin[16];
    linears(m, lin);
    for (int i = 0; i < 16; ++i)
        if ((rc = launch_repack_rows(P + l.e[2 * i].offset, mut(lin[i]->wp), lin[i]->in, lin[i]->out, lin[i]->in, 0, s))) return rc;
    const float *wih = P + l.e[E_WIH].offset, *whh = P + l.e[E_WHH].offset;
    if ((rc = launch_repack_rows(wih, mut(m->w_ih), 2 * H, 3 * H, 2 * H, 0, s))) return rc;
    if ((rc = launch_pack_gru_interleaved(wih, H, 2 * H, mut(m->w_ih_il), s))) return rc;
    if ((rc = launch_repack_rows(whh, mut(m->w_hh), H, 3 * H, H, 0, s))) return rc;
    if ((rc = launch_pack_gru_interleaved(whh, H, H, mut(m->w_hh_il), s))) return rc;
    if ((rc = launch_fold_px0_dec3(P + l.e[E_PX0].offset, P + l.e[E_PX0 + 1].offset, P + l.e[E_DE6].offset, P + l.e[E_DE6 + 1].offset, m->mean_mel,
                                   m->std_mel, H, X, mut(m->px0_dec3.wp), mut(m->px0_dec3.b), s)))
        return rc;
    // the transposed copies of the backward pass, if they exist (else the first backward builds them from the values of that time)
    std::lock_guard<std::mutex> lk(m->bwd_mu);
    if (!m->bwd_ready) return BVC_OK;
    for (int k = 0; k < 18; ++k) {
        const Linear &t = m->bwd_t[k];                   // (in, out) swapped: W is (t.in, t.out)
        const float *w = k < 16 ? P + l.e[2 * k].offset : (k == 16 ? wih : whh);
        if ((rc = launch_transpose(w, t.in, t.out, mut(t.w), s))) return rc;
        if ((rc = launch_repack_rows(t.w, mut(t.wp), t.in, t.out, t.in, 0, s))) return rc;
    }
    return BVC_OK;
}

// The master copy exists.  fill: a new one gets the model's values (and the stream is synchronised once, so that a later call on
// another stream finds it complete); without fill the caller overwrites all of it.
int ensure_master(const bvc_model *m, const Layout &l, bool fill, const char *fn, hipStream_t s) {
    std::lock_guard<std::mutex> lk(m->bwd_mu);
    if (m->master) return BVC_OK;
    if (capture_state(s) != CAP_NONE) { set_error("%s: the first call on a model allocates: not inside a stream capture", fn); return BVC_EINVAL; }
    float *p = nullptr;
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), (size_t)l.total * sizeof(float)));
    if (fill) {
        int rc = params_get(m, l, p, s);
        if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("%s: hipStreamSynchronize failed", fn); rc = BVC_EHIP; }
        if (rc) { (void)hipFree(p); return rc; }
    }
    m->master = p;
    return BVC_OK;
}

int params_set(const bvc_model *m, const Layout &l, const float *d_params, hipStream_t s) {
    if (int rc = ensure_master(m, l, false, "bvc_bvrnn_params_set", s)) return rc;
    if (d_params != m->master)
        BVC_HIP_TRY(hipMemcpyAsync(m->master, d_params, (size_t)l.total * sizeof(float), hipMemcpyDeviceToDevice, s));
    return rewrite(m, l, s);
}

int check_model(const bvc_model *m, const void *buf, const char *fn) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (!buf) { set_error("%s: null argument", fn); return BVC_EINVAL; }
    if (!aligned16(buf)) { set_error("%s: the flat buffer must be 16-byte aligned", fn); return BVC_EINVAL; }
    return need_prior(m, fn);
}

}  // namespace

extern "C" {

int bvc_bvrnn_params_get(const bvc_model *m, float *d_params, void *stream) {
    if (int rc = check_model(m, d_params, "bvc_bvrnn_params_get")) return rc;
    return params_get(m, layout_of(m), d_params, (hipStream_t)stream);
}

int bvc_bvrnn_params_set(bvc_model *m, const float *d_params, void *stream) {
    if (int rc = check_model(m, d_params, "bvc_bvrnn_params_set")) return rc;
    return params_set(m, layout_of(m), d_params, (hipStream_t)stream);
}

int bvc_optimizer_create(bvc_model *m, bvc_optimizer **out) {
    if (!out) { set_error("null out pointer"); return BVC_EINVAL; }
    *out = nullptr;
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (int rc = need_prior(m, "bvc_optimizer_create")) return rc;
    std::unique_ptr<bvc_optimizer> o(new bvc_optimizer());
    o->m = m;
    o->total = layout_of(m).total;
    const size_t bytes = (size_t)o->total * sizeof(float);
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->exp_avg), bytes));
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->exp_avg_sq), bytes));
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->partial), (size_t)norm_chunks(o->total) * sizeof(double)));
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->scal), 16));
    BVC_HIP_TRY(hipMemset(o->exp_avg, 0, bytes));
    BVC_HIP_TRY(hipMemset(o->exp_avg_sq, 0, bytes));
    BVC_HIP_TRY(hipDeviceSynchronize());
    *out = o.release();
    return BVC_OK;
}

void bvc_optimizer_destroy(bvc_optimizer *opt) { delete opt; }

int bvc_optimizer_step(bvc_optimizer *opt, const bvc_adamw_config *cfg, const float *d_grads, float *d_grad_norm, void *stream) {
    if (!opt) { set_error("null optimizer"); return BVC_EINVAL; }
    if (!cfg || !d_grads) { set_error("bvc_optimizer_step: null argument"); return BVC_EINVAL; }
    if (!aligned16(d_grads)) { set_error("bvc_optimizer_step: the flat buffer must be 16-byte aligned"); return BVC_EINVAL; }
    if (!(cfg->lr >= 0.0) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) || !(cfg->eps > 0.0) ||
        !(cfg->weight_decay >= 0.0) || std::isnan(cfg->max_grad_norm)) {
        set_error("bvc_optimizer_step: lr >= 0, betas in [0, 1), eps > 0 and weight_decay >= 0 expected (lr=%g betas=(%g, %g) eps=%g weight_decay=%g)",
                  cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay);
        return BVC_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (capture_state(s) != CAP_NONE) { set_error("bvc_optimizer_step: not inside a stream capture (the step's scalars change with every step)"); return BVC_EINVAL; }
    const bvc_model *m = opt->m;
    const Layout l = layout_of(m);
    int rc;
    if ((rc = ensure_master(m, l, true, "bvc_optimizer_step", s))) return rc;
    const double t = (double)(opt->step + 1);
    const double bc1 = 1.0 - std::pow(cfg->beta1, t), bc2 = 1.0 - std::pow(cfg->beta2, t);
    const AdamScalars a = {(float)(1.0 - cfg->lr * cfg->weight_decay), (float)cfg->beta1, (float)(1.0 - cfg->beta1), (float)cfg->beta2,
                           (float)(1.0 - cfg->beta2), (float)(cfg->lr / bc1), (float)std::sqrt(bc2), (float)cfg->eps};
    if ((rc = launch_grad_norm(d_grads, l.total, (float)cfg->max_grad_norm, opt->partial, opt->scal, d_grad_norm, s))) return rc;
    if ((rc = launch_adam(m->master, opt->exp_avg, opt->exp_avg_sq, d_grads, opt->scal, l.total, a, s))) return rc;
    ++opt->step;
    return rewrite(m, l, s);
}

int bvc_optimizer_state_get(const bvc_optimizer *opt, int64_t *step, float *d_exp_avg, float *d_exp_avg_sq, void *stream) {
    if (!opt) { set_error("null optimizer"); return BVC_EINVAL; }
    const size_t bytes = (size_t)opt->total * sizeof(float);
    if (step) *step = opt->step;
    if (d_exp_avg) BVC_HIP_TRY(hipMemcpyAsync(d_exp_avg, opt->exp_avg, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_exp_avg_sq) BVC_HIP_TRY(hipMemcpyAsync(d_exp_avg_sq, opt->exp_avg_sq, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BVC_OK;
}

int bvc_optimizer_state_set(bvc_optimizer *opt, const int64_t *step, const float *d_exp_avg, const float *d_exp_avg_sq, void *stream) {
    if (!opt) { set_error("null optimizer"); return BVC_EINVAL; }
    if (step && *step < 0) { set_error("bvc_optimizer_state_set: negative step count"); return BVC_EINVAL; }
    const size_t bytes = (size_t)opt->total * sizeof(float);
    if (step) opt->step = *step;
    if (d_exp_avg) BVC_HIP_TRY(hipMemcpyAsync(opt->exp_avg, d_exp_avg, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_exp_avg_sq) BVC_HIP_TRY(hipMemcpyAsync(opt->exp_avg_sq, d_exp_avg_sq, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BVC_OK;
}

int bvc_test_folded_hop(const bvc_model *m, float *d_w, float *d_b, void *stream) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (!d_w || !d_b) { set_error("bvc_test_folded_hop: null argument"); return BVC_EINVAL; }
    const int H = m->cfg.h_dim;
    if (int rc = launch_repack_rows(m->px0_dec3.wp, d_w, H, H, H, 1, (hipStream_t)stream)) return rc;
    BVC_HIP_TRY(hipMemcpyAsync(d_b, m->px0_dec3.b, (size_t)H * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BVC_OK;
}

}  // extern "C"
