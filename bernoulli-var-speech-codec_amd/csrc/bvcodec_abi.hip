// C ABI of libbvcodec_hip.so (include/bvcodec.h): the error text, the two probe systems, the offline entry points, the small
// utilities and the test hooks.  Host-side only: the model is made in model_build.hip (from what weight_pack.h computes) and used through model.hip, the recurrence is in recurrence.hip, step_plan.hip and flow_launch.hip, the generator in
// generator.hip, the streaming session in stream_codec.hip and the kernels in k_*.hip.
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "bvc_host.h"

namespace bvc {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- sampled hipEvent probes around kernel launches (bench instrumentation, off by default)
struct ProbeState {
    int kind = PK_NONE, every = 1, counter = 0, used = 0;
    std::vector<hipEvent_t> ev;          // pairs
};
static ProbeState g_probe;
thread_local bool g_capturing = false;
KProbe g_kprobe;

ProbeScope::ProbeScope(int kind, hipStream_t stream) : s(stream), slot(-1) {
    if (g_probe.kind != kind || g_capturing) return;
    if ((g_probe.counter++ % g_probe.every) != 0) return;
    if ((size_t)(g_probe.used + 1) * 2 > g_probe.ev.size()) return;
    slot = g_probe.used++;
    (void)hipEventRecord(g_probe.ev[2 * slot], s);
}
ProbeScope::~ProbeScope() {
    if (slot >= 0) (void)hipEventRecord(g_probe.ev[2 * slot + 1], s);
}

}  // namespace bvc

using namespace bvc;

namespace {

__global__ void tap_copy_kernel(const float *src, float *dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// The start of a compute entry point, in the order in which its errors are reported: the sticky status of an earlier persistent launch;
// the prior net where the call needs one (prior_fn: its name for the message); with L, the frame count *T of L samples; the
// workspace, carved into *w; and last the entry's own argument test, whose result the caller passes as args_ok (`bad`: its message).
int enter(const bvc_model *m, int B, const int64_t *L, int64_t *T, void *d_ws, size_t ws_bytes, Workspace *w, bool args_ok,
          const char *bad = "null argument", const char *prior_fn = nullptr) {
    if (int rc = sticky_status(m)) return rc;
    if (prior_fn) if (int rc = need_prior(m, prior_fn)) return rc;
    if (L) {
        if (!m) { set_error("null model"); return BVC_EINVAL; }
        *T = bvc_num_frames(m, *L);
        if (*T <= 0) { set_error("input too short for reflect padding (L=%lld)", (long long)*L); return BVC_EINVAL; }
    }
    if (int rc = check_ws(m, B, *T, d_ws, ws_bytes, w)) return rc;
    if (!args_ok) { set_error("%s", bad); return BVC_EINVAL; }
    return BVC_OK;
}
const char *const BAD_LENGTH = "null argument or non-positive length";

// the checks of a closed-loop call that need no tensor, in the order in which they are reported; on success the two workspaces are carved
int enter_vbr(const bvc_model *m, int B, int64_t T, const int32_t *h_ladder, int K, void *d_ws, size_t ws_bytes, Workspace *w,
              VbrWorkspace *v, const char *fn) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (int rc = sticky_status(m)) return rc;
    if (B <= 0 || T <= 0) { set_error("B and T must be positive (B=%d, T=%lld)", B, (long long)T); return BVC_EINVAL; }
    if (!m->cfg.var_bit) { set_error("%s: a fixed-rate model (var_bit = 0) has no bit mask to choose", fn); return BVC_EINVAL; }
    if (!h_ladder || K < 1 || K > VBR_MAX_RUNGS) { set_error("%s: the ladder takes 1 to %d rungs (K=%d)", fn, VBR_MAX_RUNGS, K); return BVC_EINVAL; }
    for (int k = 0; k < K; ++k)
        if (h_ladder[k] < 0 || h_ladder[k] > m->cfg.z_dim || (k && h_ladder[k] <= h_ladder[k - 1])) {
            set_error("%s: rung %d = %d: bit counts in [0, %d], strictly ascending", fn, k, h_ladder[k], m->cfg.z_dim);
            return BVC_EINVAL;
        }
    carve_vbr(m, B, K, static_cast<char *>(d_ws), v);
    carve(m, B, T, static_cast<char *>(d_ws) + v->total, w);
    if (!d_ws || ws_bytes < v->total + w->total) {
        set_error("%s: workspace too small: %zu bytes given, %zu needed (bvc_vbr_workspace_bytes)", fn, ws_bytes, v->total + w->total);
        return BVC_EINVAL;
    }
    return BVC_OK;
}

// the checks of an entropy-coded call that need no tensor, in the order in which they are reported; on success the workspaces are carved:
// the decode node's state, the ordinary workspace behind it, the prior's probabilities behind that (*prob)
int enter_entropy(const bvc_model *m, int B, int64_t T, int64_t segment, int64_t stride, void *d_ws, size_t ws_bytes, Workspace *w,
                  EntropyWorkspace *e, float **prob, const char *fn) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (int rc = sticky_status(m)) return rc;
    if (int rc = need_prior(m, fn)) return rc;
    if (B <= 0 || T <= 0) { set_error("B and T must be positive (B=%d, T=%lld)", B, (long long)T); return BVC_EINVAL; }
    if (segment < 1) { set_error("%s: segment = %lld: a segment holds at least one frame", fn, (long long)segment); return BVC_EINVAL; }
    if (stride < 0 || stride > 0x7FFFFFFFll) { set_error("%s: stride = %lld outside [0, 2^31)", fn, (long long)stride); return BVC_EINVAL; }
    if (m->cfg.z_dim > 3 * m->cfg.h_dim) { set_error("%s: z_dim > 3 h_dim is not supported", fn); return BVC_EINVAL; }
    carve_entropy(m, B, T, static_cast<char *>(d_ws), e);
    carve(m, B, T, static_cast<char *>(d_ws) + e->total, w);
    const size_t need = e->total + w->total + e->prob_bytes;
    if (!d_ws || ws_bytes < need) {
        set_error("%s: workspace too small: %zu bytes given, %zu needed (bvc_entropy_workspace_bytes)", fn, ws_bytes, need);
        return BVC_ENOMEM;
    }
    *prob = reinterpret_cast<float *>(static_cast<char *>(d_ws) + e->total + w->total);
    return BVC_OK;
}

// sizes that the host can read (pinned memory) are checked before anything is launched; the kernels take any other bad entry as 0 bytes
int check_host_sizes(const int32_t *sizes, long long n, int64_t stride, const char *fn) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, sizes) != hipSuccess) { (void)hipGetLastError(); return BVC_OK; }
    if (at.type != hipMemoryTypeHost) return BVC_OK;
    for (long long i = 0; i < n; ++i)
        if (sizes[i] < 0 || sizes[i] > stride) {
            set_error("%s: sizes[%lld] = %d outside [0, stride = %lld]", fn, i, (int)sizes[i], (long long)stride);
            return BVC_EINVAL;
        }
    return BVC_OK;
}

EntropyCall entropy_call(const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, int64_t T, int64_t segment) {
    const int64_t S = segment < T ? segment : T;
    return EntropyCall{d_data, d_sizes, stride, (int)S, (int)((T + S - 1) / S)};
}

}  // namespace

// =================================================================================================
extern "C" {

int bvc_abi_version(void) { return BVC_ABI_VERSION; }
const char *bvc_last_error(void) { return g_err; }

int64_t bvc_num_frames(const bvc_model *m, int64_t L) {
    if (!m) return BVC_EINVAL;
    const bvc_config &c = m->cfg;
    const int64_t pr = c.n_fft - c.pad_left - c.hop;
    if (L <= c.pad_left || L <= pr) return BVC_EINVAL;       // reflect padding needs pad < L
    return (L + c.pad_left + pr - c.n_fft) / c.hop + 1;
}

int64_t bvc_vocoder_length(const bvc_model *m, int64_t T) {
    if (!m || T <= 0) return BVC_EINVAL;
    return stage_len(m, T, m->cfg.n_up - 1);
}

size_t bvc_workspace_bytes(const bvc_model *m, int32_t B, int64_t T) {
    if (!m || B <= 0 || T <= 0) return 0;
    Workspace w;
    carve(m, B, T, nullptr, &w);
    return w.total;
}

int bvc_stft_logmel(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, float *d_mel,
                    void *stream) {
    if (int st_ = sticky_status(m)) return st_;
    if (!m || !d_wav || !d_mel) { set_error("null argument"); return BVC_EINVAL; }
    const int64_t T = bvc_num_frames(m, L);
    if (B <= 0 || T <= 0) { set_error("input too short for reflect padding (L=%lld)", (long long)L); return BVC_EINVAL; }
    return launch_stft_logmel(m->fe, d_wav, B, L, T, m->cfg.pad_left, scale, d_mel, (hipStream_t)stream);
}

int bvc_bvrnn_encode(const bvc_model *m, const float *d_mel, const float *d_bits, const float *d_h0, int32_t B,
                     int64_t T, float *d_codes, float *d_all_h, float *d_hT, float *d_prob, void *d_ws,
                     size_t ws_bytes, void *stream) {
    Workspace w;
    if (int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_mel && d_codes)) return rc;
    return run_encode(m, w, d_ws, d_mel, d_bits, d_h0, B, T, d_codes, d_all_h, d_hT, d_prob, (hipStream_t)stream);
}

int bvc_bvrnn_decode(const bvc_model *m, const float *d_codes, const float *d_h0, int32_t B, int64_t T, float *d_mel,
                     float *d_hT, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    if (int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_codes && d_mel)) return rc;
    return run_decode(m, w, d_ws, d_codes, d_h0, B, T, d_mel, d_hT, (hipStream_t)stream);
}

int bvc_bvrnn_decode_conceal(const bvc_model *m, const float *d_codes, const uint8_t *d_present, const float *d_bits, const float *d_h0,
                             int32_t B, int64_t T, float *d_mel, float *d_hT, float *d_codes_out, float *d_prior, void *d_ws,
                             size_t ws_bytes, void *stream) {
    Workspace w;
    int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_codes && d_present && d_mel, "null argument", "bvc_bvrnn_decode_conceal");
    if (rc) return rc;
    if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_conceal_select(d_present, T, m->cfg.var_bit ? d_bits : nullptr, (float)m->cfg.z_dim, nullptr, B, T, w.bits, s))) return rc;
    return run_decode_conceal(m, w, d_ws, d_codes, w.bits, d_h0, B, T, d_mel, d_hT, d_codes_out, d_prior, s);
}

int bvc_decode_conceal(const bvc_model *m, const float *d_codes, const uint8_t *d_present, float bits_per_frame, int32_t B, int64_t T,
                       int64_t length, float out_scale_div, float *d_wav, float *d_codes_out, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_codes && d_present && d_wav && length > 0, BAD_LENGTH, "bvc_decode_conceal");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_conceal_select(d_present, T, nullptr, m->cfg.var_bit ? bits_per_frame : (float)m->cfg.z_dim, nullptr, B, T, w.bits, s))) return rc;
    if ((rc = run_decode_conceal(m, w, d_ws, d_codes, w.bits, nullptr, B, T, w.mel, nullptr, d_codes_out, nullptr, s))) return rc;
    return run_vocoder(m, w, w.mel, B, T, length, out_scale_div, d_wav, -1, nullptr, nullptr, nullptr, s);
}

// ---- entropy-coded wire format: the coder on given tensors, the sender's pass, the receive program and the whole decoder
int64_t bvc_entropy_stride(int32_t z_dim, int64_t segment) {
    if (z_dim <= 0 || segment < 1) return BVC_EINVAL;
    return entropy_stride(z_dim, segment);
}

size_t bvc_entropy_workspace_bytes(const bvc_model *m, int32_t B, int64_t T) {
    if (!m || B <= 0 || T <= 0) return 0;
    Workspace w;
    EntropyWorkspace e;
    carve(m, B, T, nullptr, &w);
    carve_entropy(m, B, T, nullptr, &e);
    return e.total + w.total + e.prob_bytes;
}

int bvc_entropy_encode(const float *d_codes, const float *d_prob, const float *d_bits, float bits_per_frame, int32_t B, int64_t T,
                       int32_t z_dim, int64_t segment, uint8_t *d_data, int64_t stride, int32_t *d_sizes, void *stream) {
    if (!d_codes || !d_prob || !d_sizes || (!d_data && stride > 0)) { set_error("bvc_entropy_encode: null argument"); return BVC_EINVAL; }
    return launch_entropy_encode(d_codes, d_prob, d_bits, bits_per_frame, B, T, z_dim, segment, d_data, stride, d_sizes, (hipStream_t)stream);
}

int bvc_entropy_decode(const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, const float *d_prob, const float *d_bits,
                       float bits_per_frame, int32_t B, int64_t T, int32_t z_dim, int64_t segment, float *d_codes, void *stream) {
    if (!d_codes || !d_prob || !d_sizes || (!d_data && stride > 0)) { set_error("bvc_entropy_decode: null argument"); return BVC_EINVAL; }
    if (B > 0 && T > 0 && segment >= 1)
        if (int rc = check_host_sizes(d_sizes, (long long)B * ((T + (segment < T ? segment : T) - 1) / (segment < T ? segment : T)), stride, "bvc_entropy_decode")) return rc;
    return launch_entropy_decode(d_data, stride, d_sizes, d_prob, d_bits, bits_per_frame, B, T, z_dim, segment, d_codes, (hipStream_t)stream);
}

int bvc_bvrnn_entropy_pack(const bvc_model *m, const float *d_codes, const float *d_bits, const float *d_h0, int32_t B, int64_t T,
                           int64_t segment, uint8_t *d_data, int64_t stride, int32_t *d_sizes, float *d_hT, float *d_prior, void *d_ws,
                           size_t ws_bytes, void *stream) {
    const char *fn = "bvc_bvrnn_entropy_pack";
    Workspace w;
    EntropyWorkspace e;
    float *prob = nullptr;
    int rc = enter_entropy(m, B, T, segment, stride, d_ws, ws_bytes, &w, &e, &prob, fn);
    if (rc) return rc;
    if (!d_codes || !d_sizes || (!d_data && stride > 0)) { set_error("%s: null argument", fn); return BVC_EINVAL; }
    if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (d_prior) prob = d_prior;
    // the concealing pass with every frame present, on whatever schedule the model takes (its probabilities are the same bits on each);
    // its captured steps are keyed by the ordinary workspace's own base
    if ((rc = launch_fill(w.bits, -1.0f, (long long)B * T, s))) return rc;
    if ((rc = run_decode_conceal(m, w, static_cast<char *>(d_ws) + e.total, d_codes, w.bits, d_h0, B, T, w.mel, d_hT, nullptr, prob, s))) return rc;
    return launch_entropy_encode(d_codes, prob, m->cfg.var_bit ? d_bits : nullptr, (float)m->cfg.z_dim, B, T, m->cfg.z_dim, segment, d_data,
                                 stride, d_sizes, s);
}

int bvc_bvrnn_entropy_unpack(const bvc_model *m, const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, const float *d_bits,
                             const float *d_h0, int32_t B, int64_t T, int64_t segment, float *d_codes, float *d_mel, float *d_hT,
                             float *d_prior, void *d_ws, size_t ws_bytes, void *stream) {
    const char *fn = "bvc_bvrnn_entropy_unpack";
    Workspace w;
    EntropyWorkspace e;
    float *prob = nullptr;
    int rc = enter_entropy(m, B, T, segment, stride, d_ws, ws_bytes, &w, &e, &prob, fn);
    if (rc) return rc;
    if (!d_sizes || !d_mel || (!d_data && stride > 0)) { set_error("%s: null argument", fn); return BVC_EINVAL; }
    if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
    const EntropyCall call = entropy_call(d_data, stride, d_sizes, T, segment);
    if ((rc = check_host_sizes(d_sizes, (long long)B * call.nseg, stride, fn))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_entropy_bits(m->cfg.var_bit ? d_bits : nullptr, (float)m->cfg.z_dim, (long long)B * T, w.bits, s))) return rc;
    return run_entropy_unpack(m, w, e, d_ws, call, w.bits, d_h0, B, T, d_codes, d_mel, d_hT, d_prior, s);
}

int bvc_decode_entropy(const bvc_model *m, const uint8_t *d_data, int64_t stride, const int32_t *d_sizes, float bits_per_frame, int32_t B,
                       int64_t T, int64_t segment, int64_t length, float out_scale_div, float *d_wav, float *d_codes, void *d_ws,
                       size_t ws_bytes, void *stream) {
    const char *fn = "bvc_decode_entropy";
    Workspace w;
    EntropyWorkspace e;
    float *prob = nullptr;
    int rc = enter_entropy(m, B, T, segment, stride, d_ws, ws_bytes, &w, &e, &prob, fn);
    if (rc) return rc;
    if (!d_sizes || !d_wav || (!d_data && stride > 0) || length <= 0) { set_error("%s: %s", fn, BAD_LENGTH); return BVC_EINVAL; }
    const EntropyCall call = entropy_call(d_data, stride, d_sizes, T, segment);
    if ((rc = check_host_sizes(d_sizes, (long long)B * call.nseg, stride, fn))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_entropy_bits(nullptr, m->cfg.var_bit ? bits_per_frame : (float)m->cfg.z_dim, (long long)B * T, w.bits, s))) return rc;
    if ((rc = run_entropy_unpack(m, w, e, d_ws, call, w.bits, nullptr, B, T, d_codes, w.mel, nullptr, nullptr, s))) return rc;
    return run_vocoder(m, w, w.mel, B, T, length, out_scale_div, d_wav, -1, nullptr, nullptr, nullptr, s);
}

int bvc_bvrnn_forward(const bvc_model *m, const float *d_mel, const float *d_bits, const uint8_t *h_use_gen,
                      int32_t update_h, int32_t update_h2, const float *d_noise, int32_t B, int64_t T, float *d_dec,
                      float *d_kld, float *d_z, float *d_prob, float *d_prior, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    if (int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_mel && h_use_gen && d_dec && d_kld)) return rc;
    if (!update_h && !update_h2) { set_error("bvc_bvrnn_forward: at least one state must be updated"); return BVC_EINVAL; }
    for (int64_t t = 0; t < T; ++t)
        if ((h_use_gen[t] && !update_h2) || (!h_use_gen[t] && !update_h)) {
            set_error("bvc_bvrnn_forward: frame %lld is conditioned on a state that is never updated", (long long)t);
            return BVC_EINVAL;
        }
    return run_forward(m, w, d_mel, d_bits, h_use_gen, update_h != 0, update_h2 != 0, d_noise, B, T, d_dec, d_kld, d_z,
                       d_prob, d_prior, (hipStream_t)stream);
}

size_t bvc_bvrnn_backward_workspace_bytes(const bvc_model *m, int32_t B, int64_t T) {
    if (!m || B <= 0 || T <= 0) return 0;
    Workspace w;
    carve(m, B, T, nullptr, &w);
    return w.total + backward_extra_bytes(m, B, T);
}

int bvc_bvrnn_grad_layout(const bvc_config *cfg, const char **names, int64_t *offsets, int64_t *numels, int32_t capacity, int32_t *count,
                          int64_t *total) {
    if (!cfg || cfg->h_dim < 16 || cfg->z_dim < 16 || cfg->num_mels < 16) { set_error("bvc_bvrnn_grad_layout: no configuration, or not a coder's"); return BVC_EINVAL; }
    GradEntry ge[GRAD_ENTRIES];
    long long tot = 0;
    const int n = grad_layout(*cfg, ge, &tot);
    if (count) *count = n;
    if (total) *total = tot;
    if ((names || offsets || numels) && capacity < n) { set_error("bvc_bvrnn_grad_layout: room for %d entries, %d needed", (int)capacity, n); return BVC_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = ge[i].name;
        if (offsets) offsets[i] = ge[i].offset;
        if (numels) numels[i] = ge[i].numel;
    }
    return BVC_OK;
}

int bvc_bvrnn_backward_prepare(const bvc_model *m, void *stream) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (int rc = need_prior(m, "bvc_bvrnn_forward")) return rc;
    return backward_prepare(m, (hipStream_t)stream);
}

int bvc_bvrnn_backward(const bvc_model *m, const float *d_mel, const float *d_bits, const uint8_t *h_use_gen, int32_t update_h,
                       int32_t update_h2, const float *d_noise, int32_t B, int64_t T, const float *d_gdec, float g_kld, float *d_grads,
                       float *d_gmel, float *d_dec, float *d_kld, float *d_z, float *d_prob, float *d_prior, void *d_ws, size_t ws_bytes,
                       void *stream) {
    // the refusals of bvc_bvrnn_forward, with its messages and before anything is launched, then this call's own
    Workspace w;
    if (int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_mel && h_use_gen && d_gdec && d_grads)) return rc;
    const size_t need = w.total + backward_extra_bytes(m, B, T);
    if (ws_bytes < need) { set_error("workspace too small: %zu bytes given, %zu needed", ws_bytes, need); return BVC_ENOMEM; }
    if (int rc = need_prior(m, "bvc_bvrnn_forward")) return rc;
    if (m->cfg.var_bit && !d_bits) { set_error("bits per frame required when var_bit=1"); return BVC_EINVAL; }
    if (m->cfg.z_dim > m->cfg.h_dim) { set_error("bvc_bvrnn_forward: z_dim > h_dim is not supported"); return BVC_EINVAL; }
    if (!update_h && !update_h2) { set_error("bvc_bvrnn_forward: at least one state must be updated"); return BVC_EINVAL; }
    for (int64_t t = 0; t < T; ++t)
        if ((h_use_gen[t] && !update_h2) || (!h_use_gen[t] && !update_h)) {
            set_error("bvc_bvrnn_forward: frame %lld is conditioned on a state that is never updated", (long long)t);
            return BVC_EINVAL;
        }
    if ((long long)B * T * 3 * m->cfg.h_dim * 2 > INT32_MAX) { set_error("bvc_bvrnn_backward: B T = %lld rows is more than one call takes", (long long)B * T); return BVC_EINVAL; }
    const BackwardCall c = {d_mel, d_bits, h_use_gen, update_h != 0, update_h2 != 0, d_noise, B, T, d_gdec, g_kld,
                            d_grads, d_gmel, d_dec, d_kld, d_z, d_prob, d_prior};
    return run_backward(m, w, static_cast<char *>(d_ws) + w.total, c, (hipStream_t)stream);
}

int bvc_bigvgan(const bvc_model *m, const float *d_mel, int32_t B, int64_t T, int64_t length, float out_scale_div,
                float *d_wav, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    if (int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_mel && d_wav && length > 0, BAD_LENGTH)) return rc;
    return run_vocoder(m, w, d_mel, B, T, length, out_scale_div, d_wav, -1, nullptr, nullptr, nullptr,
                       (hipStream_t)stream);
}

int bvc_encode(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, float bits_per_frame,
               float *d_codes, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int64_t T = 0;
    int rc = enter(m, B, &L, &T, d_ws, ws_bytes, &w, d_wav && d_codes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_stft_logmel(m->fe, d_wav, B, L, T, m->cfg.pad_left, scale, w.mel, s))) return rc;
    if ((rc = launch_fill(w.bits, bits_per_frame, (long long)B * T, s))) return rc;
    return run_encode(m, w, d_ws, w.mel, w.bits, nullptr, B, T, d_codes, nullptr, nullptr, nullptr, s);
}

// ---- closed-loop rate selection: the workspace is the candidates' frame buffers followed by the ordinary workspace (carve_vbr)
size_t bvc_vbr_workspace_bytes(const bvc_model *m, int32_t B, int64_t T, int32_t K) {
    if (!m || B <= 0 || T <= 0 || K < 1 || K > VBR_MAX_RUNGS) return 0;
    Workspace w;
    VbrWorkspace v;
    carve(m, B, T, nullptr, &w);
    carve_vbr(m, B, K, nullptr, &v);
    return v.total + w.total;
}

// the cap's own checks, behind enter_vbr's: 0 with *cap filled in
static int enter_cap(const char *fn, const int32_t *h_ladder, int32_t rate_q8, int32_t burst_q8, const int32_t *d_tok0, int32_t *d_tokT,
                     VbrCap *cap) {
    if (rate_q8 < 0 || burst_q8 < 0) { set_error("%s: rate_q8 = %d, burst_q8 = %d: neither may be negative", fn, (int)rate_q8, (int)burst_q8); return BVC_EINVAL; }
    if ((long long)burst_q8 < (long long)h_ladder[0] * 256) {
        set_error("%s: a bucket of %d/256 bits never holds rung 0 (%d bits)", fn, (int)burst_q8, (int)h_ladder[0]);
        return BVC_EINVAL;
    }
    *cap = VbrCap{1, rate_q8, burst_q8, d_tok0, d_tokT};
    return BVC_OK;
}

static int encode_vbr_mel(const char *fn, const bvc_model *m, const float *d_mel, const float *d_target, const int32_t *h_ladder, int32_t K,
                          const float *d_h0, int32_t B, int64_t T, float *d_codes, float *d_bits, float *d_all_h, float *d_hT, float *d_prob,
                          float *d_dist, float *d_dec, void *d_ws, size_t ws_bytes, void *stream, bool capped, int32_t rate_q8, int32_t burst_q8,
                          const int32_t *d_tok0, int32_t *d_tokT) {
    Workspace w;
    VbrWorkspace v;
    VbrCap cap{0, 0, 0, nullptr, nullptr};
    if (int rc = enter_vbr(m, B, T, h_ladder, K, d_ws, ws_bytes, &w, &v, fn)) return rc;
    if (!d_mel || !d_target || !d_codes || !d_bits) { set_error("null argument"); return BVC_EINVAL; }
    if (capped) if (int rc = enter_cap(fn, h_ladder, rate_q8, burst_q8, d_tok0, d_tokT, &cap)) return rc;
    return run_encode_vbr(m, w, v, d_ws, d_mel, d_target, h_ladder, K, d_h0, B, T, d_codes, d_bits, d_all_h, d_hT, d_prob, d_dist, d_dec,
                          (hipStream_t)stream, &cap);
}

static int encode_vbr_wav(const char *fn, const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, const float *d_target,
                          const int32_t *h_ladder, int32_t K, float *d_codes, float *d_bits, void *d_ws, size_t ws_bytes, void *stream,
                          bool capped, int32_t rate_q8, int32_t burst_q8) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    const int64_t T = bvc_num_frames(m, L);
    if (T <= 0) { set_error("input too short for reflect padding (L=%lld)", (long long)L); return BVC_EINVAL; }
    Workspace w;
    VbrWorkspace v;
    VbrCap cap{0, 0, 0, nullptr, nullptr};
    int rc = enter_vbr(m, B, T, h_ladder, K, d_ws, ws_bytes, &w, &v, fn);
    if (rc) return rc;
    if (!d_wav || !d_target || !d_codes || !d_bits) { set_error("null argument"); return BVC_EINVAL; }
    if (capped && (rc = enter_cap(fn, h_ladder, rate_q8, burst_q8, nullptr, nullptr, &cap))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_stft_logmel(m->fe, d_wav, B, L, T, m->cfg.pad_left, scale, w.mel, s))) return rc;
    return run_encode_vbr(m, w, v, d_ws, w.mel, d_target, h_ladder, K, nullptr, B, T, d_codes, d_bits, nullptr, nullptr, nullptr, nullptr,
                          nullptr, s, &cap);
}

int bvc_bvrnn_encode_vbr(const bvc_model *m, const float *d_mel, const float *d_target, const int32_t *h_ladder, int32_t K,
                         const float *d_h0, int32_t B, int64_t T, float *d_codes, float *d_bits, float *d_all_h, float *d_hT,
                         float *d_prob, float *d_dist, float *d_dec, void *d_ws, size_t ws_bytes, void *stream) {
    return encode_vbr_mel("bvc_bvrnn_encode_vbr", m, d_mel, d_target, h_ladder, K, d_h0, B, T, d_codes, d_bits, d_all_h, d_hT, d_prob, d_dist,
                          d_dec, d_ws, ws_bytes, stream, false, 0, 0, nullptr, nullptr);
}

int bvc_bvrnn_encode_vbr_capped(const bvc_model *m, const float *d_mel, const float *d_target, const int32_t *h_ladder, int32_t K,
                                const float *d_h0, int32_t B, int64_t T, float *d_codes, float *d_bits, float *d_all_h, float *d_hT,
                                float *d_prob, float *d_dist, float *d_dec, void *d_ws, size_t ws_bytes, void *stream, int32_t rate_q8,
                                int32_t burst_q8, const int32_t *d_tok0, int32_t *d_tokT) {
    return encode_vbr_mel("bvc_bvrnn_encode_vbr_capped", m, d_mel, d_target, h_ladder, K, d_h0, B, T, d_codes, d_bits, d_all_h, d_hT, d_prob,
                          d_dist, d_dec, d_ws, ws_bytes, stream, true, rate_q8, burst_q8, d_tok0, d_tokT);
}

int bvc_encode_vbr(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, const float *d_target,
                   const int32_t *h_ladder, int32_t K, float *d_codes, float *d_bits, void *d_ws, size_t ws_bytes, void *stream) {
    return encode_vbr_wav("bvc_encode_vbr", m, d_wav, B, L, scale, d_target, h_ladder, K, d_codes, d_bits, d_ws, ws_bytes, stream, false, 0, 0);
}

int bvc_encode_vbr_capped(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, const float *d_target,
                          const int32_t *h_ladder, int32_t K, float *d_codes, float *d_bits, void *d_ws, size_t ws_bytes, void *stream,
                          int32_t rate_q8, int32_t burst_q8) {
    return encode_vbr_wav("bvc_encode_vbr_capped", m, d_wav, B, L, scale, d_target, h_ladder, K, d_codes, d_bits, d_ws, ws_bytes, stream, true,
                          rate_q8, burst_q8);
}

int bvc_forward(const bvc_model *m, const float *d_wav, int32_t B, int64_t L, float scale, float bits_per_frame, int64_t length,
                float out_scale_div, float *d_codes, float *d_wav_out, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int64_t T = 0;
    int rc = enter(m, B, &L, &T, d_ws, ws_bytes, &w, d_wav && d_wav_out && length > 0, BAD_LENGTH);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_stft_logmel(m->fe, d_wav, B, L, T, m->cfg.pad_left, scale, w.mel, s))) return rc;
    if ((rc = launch_fill(w.bits, bits_per_frame, (long long)B * T, s))) return rc;
    // the encoder's recurrence runs the decoder of every frame anyway (bvrnn.py:198-204): its outputs ARE what BVRNN.decode(codes) would
    // compute over again from the same states.  w.mel has been consumed (normalised into another buffer) before the first of them is
    // written; codes nobody asked for go to a workspace tensor that encode does not use.
    float *codes = d_codes ? d_codes : w.part_gru;
    if ((rc = run_encode(m, w, d_ws, w.mel, w.bits, nullptr, B, T, codes, nullptr, nullptr, nullptr, s, w.mel))) return rc;
    return run_vocoder(m, w, w.mel, B, T, length, out_scale_div, d_wav_out, -1, nullptr, nullptr, nullptr, s);
}

int bvc_decode(const bvc_model *m, const float *d_codes, int32_t B, int64_t T, int64_t length, float out_scale_div,
               float *d_wav, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_codes && d_wav && length > 0, BAD_LENGTH);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = run_decode(m, w, d_ws, d_codes, nullptr, B, T, w.mel, nullptr, s))) return rc;
    return run_vocoder(m, w, w.mel, B, T, length, out_scale_div, d_wav, -1, nullptr, nullptr, nullptr, s);
}

int bvc_encode_ragged(const bvc_model *m, const float *d_wav, const int64_t *d_lengths, int32_t B, int64_t L, float scale,
                      const float *d_bits, float bits_per_frame, float *d_codes, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int64_t T = 0;
    int rc = enter(m, B, &L, &T, d_ws, ws_bytes, &w, d_wav && d_lengths && d_codes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long *lens = reinterpret_cast<const long long *>(d_lengths);
    const int pl = m->cfg.pad_left;
    // every row runs all T frames through the coder; its frames behind T_b see the log floor and no bits, and are discarded
    if ((rc = launch_stft_logmel(m->fe, d_wav, B, L, T, pl, scale, w.mel, s, lens))) return rc;
    if ((rc = launch_ragged_bits(w.bits, d_bits, bits_per_frame, lens, B, L, T, pl, s))) return rc;
    if ((rc = run_encode(m, w, d_ws, w.mel, w.bits, nullptr, B, T, d_codes, nullptr, nullptr, nullptr, s))) return rc;
    if (!m->cfg.var_bit) return launch_ragged_mask(d_codes, lens, B, L, T, m->cfg.z_dim, pl, s);     // (var_bit: 0 bits did it)
    return BVC_OK;
}

int bvc_decode_ragged(const bvc_model *m, const float *d_codes, const int64_t *d_frames, int32_t B, int64_t T,
                      const int64_t *d_lengths, int64_t n_max, float out_scale_div, float *d_wav, void *d_ws, size_t ws_bytes,
                      void *stream) {
    Workspace w;
    int rc = enter(m, B, nullptr, &T, d_ws, ws_bytes, &w, d_codes && d_frames && d_lengths && d_wav && n_max > 0,
                   "null argument or non-positive n_max");
    if (rc) return rc;
    if (m->noncausal) { set_error("bvc_decode_ragged: %s (a row's end would read the next row's frames)", not_causal(m)); return BVC_EINVAL; }
    if (n_max > bvc_vocoder_length(m, T)) {
        set_error("n_max %lld exceeds the generator's %lld samples for T=%lld", (long long)n_max,
                  (long long)bvc_vocoder_length(m, T), (long long)T);
        return BVC_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = run_decode(m, w, d_ws, d_codes, nullptr, B, T, w.mel, nullptr, s))) return rc;
    // the bounds table goes to the normalised-mel buffer, which only encode uses: (n_up + 1) * B int64 <= B * T * num_mels floats
    long long *lim = reinterpret_cast<long long *>(w.yn);
    if ((size_t)(m->cfg.n_up + 1) * 2 > (size_t)T * m->cfg.num_mels) { set_error("ragged decode: no room for the bounds"); return BVC_EINVAL; }
    if ((rc = launch_ragged_limits(lim, reinterpret_cast<const long long *>(d_frames), reinterpret_cast<const long long *>(d_lengths),
                                   B, T, n_max, m->cfg.n_up, m->cfg.up_rates, s))) return rc;
    return run_vocoder(m, w, w.mel, B, T, n_max, out_scale_div, d_wav, -1, nullptr, nullptr, nullptr, s, lim);
}

#ifdef BVC_PHASE_PROBE
int bvc_phase_probe_read(unsigned long long *out, int reset) { return bvc::phase_probe_read(out, reset); }
#endif

int bvc_probe_begin(int32_t kind, int32_t sample_every, int32_t max_samples) {
    if (kind <= PK_NONE || kind > PK_POST || sample_every < 1 || max_samples < 1) {
        set_error("bvc_probe_begin: bad arguments");
        return BVC_EINVAL;
    }
    while ((int)g_probe.ev.size() < 2 * max_samples) {
        hipEvent_t e;
        BVC_HIP_TRY(hipEventCreate(&e));
        g_probe.ev.push_back(e);
    }
    g_probe.kind = kind; g_probe.every = sample_every; g_probe.counter = 0; g_probe.used = 0;
    return BVC_OK;
}

int bvc_probe_end(double *mean_us, double *min_us, int32_t *n_samples) {
    g_probe.kind = PK_NONE;
    BVC_HIP_TRY(hipDeviceSynchronize());
    double sum = 0.0, mn = 1e30;
    for (int i = 0; i < g_probe.used; ++i) {
        float ms = 0.0f;
        BVC_HIP_TRY(hipEventElapsedTime(&ms, g_probe.ev[2 * i], g_probe.ev[2 * i + 1]));
        sum += ms * 1e3;
        if (ms * 1e3 < mn) mn = ms * 1e3;
    }
    if (mean_us) *mean_us = g_probe.used ? sum / g_probe.used : 0.0;
    if (min_us) *min_us = g_probe.used ? mn : 0.0;
    if (n_samples) *n_samples = g_probe.used;
    return BVC_OK;
}

int bvc_resample_poly(const float *d_x, int32_t B, int64_t L_in, const double *d_h, int32_t ntaps, int32_t up, int32_t down,
                      int64_t n_pre_remove, float *d_y, int64_t n_out, void *stream) {
    if (!d_x || !d_h || !d_y || B <= 0 || L_in <= 0 || ntaps <= 0 || up < 1 || down < 1 || n_pre_remove < 0 || n_out <= 0) {
        set_error("bvc_resample_poly: bad arguments");
        return BVC_EINVAL;
    }
    return launch_resample_poly(d_x, B, L_in, d_h, ntaps, up, down, n_pre_remove, d_y, n_out, (hipStream_t)stream);
}

int bvc_peak_normalize(float *d_x, int32_t B, int64_t L, void *stream) {
    if (!d_x || B <= 0 || L <= 0) { set_error("bvc_peak_normalize: bad arguments"); return BVC_EINVAL; }
    return launch_peak_normalize(d_x, B, L, (hipStream_t)stream);
}

int bvc_pack_codes(const float *d_codes, int32_t B, int64_t T, int32_t z_dim, int32_t nbits, uint8_t *d_bytes, void *stream) {
    if (!d_codes || !d_bytes || B <= 0 || T <= 0 || z_dim <= 0 || nbits < 0 || nbits > z_dim) {
        set_error("bvc_pack_codes: bad arguments");
        return BVC_EINVAL;
    }
    return launch_pack_codes(d_codes, (long long)B * T, z_dim, nbits, d_bytes, (hipStream_t)stream);
}

int bvc_unpack_codes(const uint8_t *d_bytes, int32_t B, int64_t T, int32_t z_dim, int32_t nbits, float *d_codes, void *stream) {
    if (!d_codes || (!d_bytes && nbits > 0) || B <= 0 || T <= 0 || z_dim <= 0 || nbits < 0 || nbits > z_dim) {
        set_error("bvc_unpack_codes: bad arguments");
        return BVC_EINVAL;
    }
    return launch_unpack_codes(d_bytes, (long long)B * T, z_dim, nbits, d_codes, (hipStream_t)stream);
}

int bvc_pack_codes_vbr(const float *d_codes, const float *d_bits, int32_t B, int64_t T, int32_t z_dim, uint8_t *d_bytes, int32_t *d_sizes,
                       void *stream) {
    if (!d_codes || !d_bits || !d_bytes || B <= 0 || T <= 0 || z_dim <= 0 || z_dim > 255) {
        set_error("bvc_pack_codes_vbr: bad arguments (the bit count of a frame is one byte: z_dim <= 255)");
        return BVC_EINVAL;
    }
    return launch_pack_codes_vbr(d_codes, d_bits, (long long)B * T, z_dim, d_bytes, d_sizes, (hipStream_t)stream);
}

int bvc_unpack_codes_vbr(const uint8_t *d_bytes, int32_t B, int64_t T, int32_t z_dim, float *d_codes, float *d_bits, void *stream) {
    if (!d_bytes || !d_codes || B <= 0 || T <= 0 || z_dim <= 0 || z_dim > 255) {
        set_error("bvc_unpack_codes_vbr: bad arguments (the bit count of a frame is one byte: z_dim <= 255)");
        return BVC_EINVAL;
    }
    return launch_unpack_codes_vbr(d_bytes, (long long)B * T, z_dim, d_codes, d_bits, (hipStream_t)stream);
}

// test helpers (allocate + synchronise): the select kernel alone, on one frame; d_tok != null: under the cap, the (B) buckets in place
static int test_vbr_select(const char *fn, const float *d_melhat, const float *d_y, const float *d_tau, const int32_t *h_ladder, int32_t K,
                           int32_t B, int32_t num_mels, float *d_dist, int32_t *d_choice, float *d_bits, void *stream, int32_t rate_q8,
                           int32_t burst_q8, int32_t *d_tok) {
    if (!d_melhat || !d_y || !d_tau || !h_ladder || !d_dist || !d_choice || !d_bits || B <= 0 || num_mels <= 0 || K < 1 || K > VBR_MAX_RUNGS) {
        set_error("%s: bad arguments", fn);
        return BVC_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    VbrCall c;
    memset(&c, 0, sizeof(c));
    c.y = d_y; c.tau = d_tau; c.dist = d_dist; c.bits = d_bits; c.choice = d_choice;
    for (int k = 0; k < K; ++k) c.ladder[k] = h_ladder[k];
    if (d_tok) { c.capped = 1; c.rate_q8 = rate_q8; c.burst_q8 = burst_q8; c.tok = d_tok; }
    VbrCall *dc = nullptr;
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dc), sizeof(VbrCall)));
    int rc = launch_vbr_set_call(dc, c, s);
    VbrStep a;
    memset(&a, 0, sizeof(a));
    a.call = dc; a.B = B; a.K = K; a.X = num_mels; a.melk = d_melhat;
    if (!rc) rc = launch_vbr_select(a, 0, s);
    const hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(dc);
    if (!rc && e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); rc = BVC_EHIP; }
    return rc;
}

int bvc_test_vbr_select(const float *d_melhat, const float *d_y, const float *d_tau, const int32_t *h_ladder, int32_t K, int32_t B,
                        int32_t num_mels, float *d_dist, int32_t *d_choice, float *d_bits, void *stream) {
    return test_vbr_select("bvc_test_vbr_select", d_melhat, d_y, d_tau, h_ladder, K, B, num_mels, d_dist, d_choice, d_bits, stream, 0, 0, nullptr);
}

int bvc_test_vbr_select_capped(const float *d_melhat, const float *d_y, const float *d_tau, const int32_t *h_ladder, int32_t K, int32_t B,
                               int32_t num_mels, float *d_dist, int32_t *d_choice, float *d_bits, void *stream, int32_t rate_q8,
                               int32_t burst_q8, int32_t *d_tok) {
    if (!d_tok || rate_q8 < 0 || burst_q8 < 0) { set_error("bvc_test_vbr_select_capped: bad arguments"); return BVC_EINVAL; }
    return test_vbr_select("bvc_test_vbr_select_capped", d_melhat, d_y, d_tau, h_ladder, K, B, num_mels, d_dist, d_choice, d_bits, stream,
                           rate_q8, burst_q8, d_tok);
}

int bvc_kprobe_enable(int32_t on) {
    if (on && !g_kprobe.dev) {
        const size_t cap = (size_t)FLOW_STAMPS * 16 * 4096;     // up to 4096 frames x 16 nodes (x stamp kinds of the persistent kernel)
        BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g_kprobe.dev), cap * sizeof(unsigned long long)));
        g_kprobe.capacity = cap;
    }
    g_kprobe.enabled = on != 0;
    return BVC_OK;
}

int bvc_kprobe_read(int32_t node_lo, int32_t node_hi, double *mean_us, double *min_us, int32_t *n_samples) {
    BVC_HIP_TRY(hipDeviceSynchronize());
    double sum = 0.0, mn = 1e30;
    int n = 0;
    if (g_kprobe.dev && g_kprobe.T > 0) {
        const size_t cnt = (size_t)2 * g_kprobe.T * g_kprobe.nodes;
        std::vector<unsigned long long> h(cnt);
        BVC_HIP_TRY(hipMemcpy(h.data(), g_kprobe.dev, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (long long t = 0; t < g_kprobe.T; ++t)
            for (int k = node_lo; k < node_hi && k < g_kprobe.nodes; ++k) {
                const unsigned long long a = h[t * g_kprobe.nodes + k], b = h[cnt / 2 + t * g_kprobe.nodes + k];
                if (b <= a) continue;
                const double us = (double)(b - a) * 0.01;        // 100 MHz ticks
                sum += us; if (us < mn) mn = us; ++n;
            }
    }
    if (mean_us) *mean_us = n ? sum / n : 0.0;
    if (min_us) *min_us = n ? mn : 0.0;
    if (n_samples) *n_samples = n;
    return BVC_OK;
}

// Raw stamps of the persistent recurrence's probing wave: mean / min of (stamp kind `to` - stamp kind `from`) over the frames,
// for the layers [node_lo, node_hi).  from = -1: `to` of layer k against stamp 1 (published) of layer k - 1, i.e. since the
// previous layer's output left.
int bvc_kprobe_read_span(int32_t from, int32_t to, int32_t node_lo, int32_t node_hi, double *mean_us, double *min_us, int32_t *n_samples) {
    BVC_HIP_TRY(hipDeviceSynchronize());
    double sum = 0.0, mn = 1e30;
    int n = 0;
    if (from < -1 || from >= FLOW_STAMPS || to < 0 || to >= FLOW_STAMPS) { set_error("bvc_kprobe_read_span: stamp kinds are 0..%d", FLOW_STAMPS - 1); return BVC_EINVAL; }
    if (g_kprobe.dev && g_kprobe.T > 0 && (size_t)FLOW_STAMPS * g_kprobe.T * g_kprobe.nodes <= g_kprobe.capacity) {
        const size_t per = (size_t)g_kprobe.T * g_kprobe.nodes, cnt = (size_t)FLOW_STAMPS * per;
        std::vector<unsigned long long> h(cnt);
        BVC_HIP_TRY(hipMemcpy(h.data(), g_kprobe.dev, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (long long t = 0; t < g_kprobe.T; ++t)
            for (int k = node_lo; k < node_hi && k < g_kprobe.nodes; ++k) {
                unsigned long long a = 0;
                if (from >= 0) a = h[(size_t)from * per + t * g_kprobe.nodes + k];
                else {
                    // from the previous layer's "published" stamp: the nearest earlier node that was stamped at all (with the folded hop the
                    // program has no dec.6 node: its slot stays empty), wrapping into the previous frame's last layer
                    long long idx = t * g_kprobe.nodes + k - 1;
                    for (int back = 0; back < g_kprobe.nodes && idx >= 0 && !a; ++back, --idx) a = h[per + idx];
                    if (!a) continue;
                }
                const unsigned long long b = h[(size_t)to * per + t * g_kprobe.nodes + k];
                if (!a || b <= a) continue;
                const double us = (double)(b - a) * 0.01;        // 100 MHz ticks
                sum += us; if (us < mn) mn = us; ++n;
            }
    }
    if (mean_us) *mean_us = n ? sum / n : 0.0;
    if (min_us) *min_us = n ? mn : 0.0;
    if (n_samples) *n_samples = n;
    return BVC_OK;
}

int bvc_test_linear(const float *d_x, const float *d_w, const float *d_bias, int32_t M, int32_t N, int32_t K,
                    int32_t act, float *d_y, void *stream) {
    // test helper (allocates + synchronises): packs the natural weight on the device first
    if (K % 16 || N % 16) { set_error("bvc_test_linear: N and K must be multiples of 16"); return BVC_EINVAL; }
    float *wp = nullptr;
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&wp), (size_t)N * K * sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    // W[N][K] natural == "matrix with N rows of length K": its B-operand packing equals the A-operand packing
    int rc = launch_repack_rows(d_w, wp, K, N, K, 0, s);
    Linear l; l.w = d_w; l.wp = wp; l.b = d_bias; l.in = K; l.out = N;
    if (!rc) rc = launch_gemm_skinny(lin_params(l, dp_static(d_x, K), M, dp_static(d_y, N)), act ? EPI_ELU : EPI_LINEAR, s);
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(wp);
    if (!rc && e != hipSuccess) { set_error("bvc_test_linear: %s", hipGetErrorString(e)); rc = BVC_EHIP; }
    return rc;
}

int bvc_test_linear_batched(const float *d_x, const float *d_w, const float *d_bias, int32_t M, int32_t N, int32_t K,
                            int32_t act, float *d_y, void *stream) {
    return launch_gemm_batched(d_x, K, d_w, K, d_bias, M, N, K, act, d_y, N, (hipStream_t)stream);
}

int bvc_test_weight_grad(const float *d_dy, const float *d_x, int32_t M, int32_t N, int32_t K, float *d_dw, int64_t *out_cut, void *stream) {
    // test helper (allocates + synchronises); the shape is checked first, on the host, so that a refusal can be had without a device
    const char *fn = "bvc_test_weight_grad";
    if (M < 1 || N < 16 || K < 16 || N % 16 || K % 16) { set_error("%s: M = %d, N = %d, K = %d: N and K must be multiples of 16, M at least 1", fn, M, N, K); return BVC_EINVAL; }
    if (!d_dy || !d_x || !d_dw || ((uintptr_t)d_dy | (uintptr_t)d_x | (uintptr_t)d_dw) % 16) { set_error("%s: the matrices must be there and 16-byte aligned", fn); return BVC_EINVAL; }
    const WeightGradCut c = weight_grad_cut(M, N, K);
    if (out_cut) { out_cut[0] = c.chunks; out_cut[1] = c.chunk_rows; }
    float *ws = nullptr;
    if (c.ws_floats) BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ws), c.ws_floats * sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_weight_grad(d_dy, d_x, M, N, K, d_dw, ws, s);
    hipError_t e = hipStreamSynchronize(s);
    if (ws) (void)hipFree(ws);
    if (!rc && e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); rc = BVC_EHIP; }
    return rc;
}

int bvc_test_skinny_pick(int32_t M, int32_t epi, int32_t gate_il, int32_t mtw, int32_t latency, int32_t *out) {
    if (!out || M < 1 || epi < EPI_LINEAR || epi > EPI_SIGMOID) { set_error("bvc_test_skinny_pick: bad arguments"); return BVC_EINVAL; }
    if (gate_il && epi != EPI_GRU) { set_error("bvc_test_skinny_pick: gate-interleaved weights are for the GRU launch only"); return BVC_EINVAL; }
    const SkinnyPick k = skinny_pick(M, epi, gate_il, mtw, latency != 0);
    out[0] = k.id; out[1] = k.mtw;
    return BVC_OK;
}

int bvc_test_skinny_counts(int64_t *out) {
    if (!out) { set_error("bvc_test_skinny_counts: bad arguments"); return BVC_EINVAL; }
    long long n[2 * SK_COUNT];
    skinny_launch_counts(n);
    for (int i = 0; i < 2 * SK_COUNT; ++i) out[i] = n[i];
    return BVC_OK;
}

int bvc_test_linear_tiles(const float *d_x, const float *d_w, const float *d_bias, int32_t M, int32_t N, int32_t K, int32_t act,
                          int32_t mtw, int32_t frames, float *d_y, void *stream) {
    // test helper (allocates + synchronises): bvc_test_linear with the caller's row tiles per workgroup, over `frames` frames
    const char *fn = "bvc_test_linear_tiles";
    if (K % 16 || N % 16 || K < 16 || N < 16) { set_error("%s: N and K must be multiples of 16", fn); return BVC_EINVAL; }
    if (frames < 1) { set_error("%s: frames = %d, at least one", fn, frames); return BVC_EINVAL; }
    if (!d_x || !d_w || !d_y || M < 1 || (long long)M * K > INT32_MAX || (long long)M * N > INT32_MAX) { set_error("%s: bad arguments", fn); return BVC_EINVAL; }
    float *wp = nullptr;
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&wp), (size_t)N * K * sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_repack_rows(d_w, wp, K, N, K, 0, s);
    Linear l; l.w = d_w; l.wp = wp; l.b = d_bias; l.in = K; l.out = N;
    GemmParams p = lin_params(l, dp_static_frames(d_x, K, (long long)M * K), M, dp_static_frames(d_y, N, (long long)M * N));
    p.frames = frames;                 // 1: the one-frame kernel (which never reads the frame stride), else the frame in grid.y
    if (!rc) rc = launch_gemm_skinny(p, act ? EPI_ELU : EPI_LINEAR, s, mtw);
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(wp);
    if (!rc && e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); rc = BVC_EHIP; }
    return rc;
}

int bvc_test_tile_plan(int32_t kind, int64_t rows, int32_t column_blocks, int32_t ks, int32_t mode, int64_t *out) {
    if (!out || kind < 0 || kind > 1) { set_error("bvc_test_tile_plan: bad arguments"); return BVC_EINVAL; }
    const bool last = mode == -1, legacy = mode == 1;
    const int force = mode >= 16 ? mode : 0;
    if (kind == 0) {
        const GemmSwitches sw = gemm_switches();
        const GemmCut c = last ? g_last_gemm_cut : gemm_batched_cut((int)rows, column_blocks * 128, force, legacy, sw.no_tail, sw.no_quarter);
        out[0] = c.height; out[1] = c.full_blocks; out[2] = c.tail_height; out[3] = c.tiles; out[4] = c.rounds; out[5] = c.cost100;
        return BVC_OK;
    }
    const TilePlan c = last ? g_last_amp_cut : amp_pair_cut(rows, column_blocks, ks, force, legacy);
    out[0] = c.height; out[1] = c.height ? c.tiles / (column_blocks > 0 && !last ? column_blocks : 1) : 0; out[2] = 0;
    out[3] = c.tiles; out[4] = c.rounds; out[5] = c.cost * 100;
    return BVC_OK;
}

int bvc_test_snakebeta(const float *d_x, int64_t n, float alpha, float beta, float *d_y, void *stream) {
    if (!d_x || !d_y || n <= 0) { set_error("bvc_test_snakebeta: bad arguments"); return BVC_EINVAL; }
    const float a = (float)std::exp((double)alpha);                                  // as make_conv() derives them
    const float ib = 1.0f / ((float)std::exp((double)beta) + 0.000000001f);
    return launch_snakebeta_test(d_x, n, a, ib, d_y, (hipStream_t)stream);
}

int bvc_test_stft_logmel(const bvc_model *m, const float *d_wav, const int64_t *d_lengths, int32_t B, int64_t L, int64_t T,
                         int32_t pad_left, float scale, float *d_mel, void *stream) {
    // test helper (synchronises): ONE launch of the front-end with the caller's frame count and left padding.  The shape is checked
    // first, on the host and without the model, so that a refusal can be had without a device.
    const char *fn = "bvc_test_stft_logmel";
    if (pad_left < 0 || pad_left > 768) { set_error("%s: pad_left %d outside [0, 768]", fn, pad_left); return BVC_EINVAL; }
    if (T < 1) { set_error("%s: T = %lld, at least one frame", fn, (long long)T); return BVC_EINVAL; }
    if (B < 1 || L < 1 || T > (int64_t)1 << 40) { set_error("%s: B = %d, L = %lld, T = %lld", fn, B, (long long)L, (long long)T); return BVC_EINVAL; }
    // frame t reads the padded samples 256 t - pad_left + [0, 1024); one reflection maps i < 0 to -i and i >= L to 2 (L - 1) - i
    const long long last = 256 * (long long)(T - 1) - pad_left + 1023;
    if (pad_left >= L || last > 2 * ((long long)L - 1)) {
        set_error("%s: T = %lld frames at pad_left = %d read the reflected sample %lld outside [0, L = %lld)", fn, (long long)T, pad_left,
                  pad_left >= L ? (long long)pad_left : 2 * ((long long)L - 1) - last, (long long)L);
        return BVC_EINVAL;
    }
    if (d_lengths && T > ragged_frames(L, L, pad_left)) {
        set_error("%s: with lengths T = %lld exceeds the %lld frames of a full row", fn, (long long)T, ragged_frames(L, L, pad_left));
        return BVC_EINVAL;
    }
    if (!m || !d_wav || !d_mel) { set_error("%s: null argument", fn); return BVC_EINVAL; }
    if (int st_ = sticky_status(m)) return st_;
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_stft_logmel(m->fe, d_wav, B, L, T, pad_left, scale, d_mel, s, reinterpret_cast<const long long *>(d_lengths));
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); rc = BVC_EHIP; }
    return rc;
}

int bvc_test_vocoder_tap(const bvc_model *m, const float *d_mel, int32_t B, int64_t T, int32_t which, float *d_out,
                         int64_t *out_numel_per_batch, void *d_ws, size_t ws_bytes, void *stream) {
    Workspace w;
    int rc = check_ws(m, B, T, d_ws, ws_bytes, &w);
    if (rc) return rc;
    if (which < 0 || which > 2 * m->cfg.n_up) { set_error("tap index out of range"); return BVC_EINVAL; }
    const float *tap = nullptr;
    int64_t len = 0;
    int ch = 0;
    int64_t tap_bs = 0;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = run_vocoder(m, w, d_mel, B, T, 1, 1.0f, nullptr, which, &tap, &len, &ch, s, nullptr, &tap_bs))) return rc;
    const long long n = (long long)B * len * ch;
    if (out_numel_per_batch) *out_numel_per_batch = len * ch;
    if (d_out && tap_bs != len * ch) return copy_rows(tap, tap_bs, d_out, len * ch, len * ch, B, s);     // a symmetric stage's view
    if (d_out) {
        hipLaunchKernelGGL(tap_copy_kernel, dim3(1024), dim3(256), 0, s, tap, d_out, n);
        BVC_HIP_TRY(hipGetLastError());
    }
    return BVC_OK;
}

int bvc_test_vocoder_layer(const bvc_model *m, int32_t kind, int32_t stage, int32_t block, int32_t iteration, const float *d_x,
                           int32_t B, int64_t L, float *d_out, int32_t epi, const float *d_acc, int32_t window, int64_t row_begin,
                           int64_t t_origin, int64_t length, float div, int64_t *out_info, void *stream) {
    // test helper (synchronises): ONE launch of the generator on the caller's input, through the launchers and the packed weights of the path
    if (!m || !d_x || !d_out || B <= 0 || L <= 0) { set_error("bvc_test_vocoder_layer: bad arguments"); return BVC_EINVAL; }
    const bvc_config &c = m->cfg;
    hipStream_t s = (hipStream_t)stream;
    int64_t rows = 0, ch = 0;
    int rc = BVC_OK;
    g_last_amp_launch = {0, 0, 0};
    switch (kind) {
        case 0:                                                              // conv_pre (as run_vocoder launches it)
            rows = L; ch = c.upsample_initial_channel;
            rc = launch_conv_mfma(m->conv_pre, d_x, L, d_out, L, B, CE_STORE, nullptr, nullptr, 1.0f, s, nullptr, nullptr, 0, m->pre_sym ? 3 : 0);
            break;
        case 1:                                                              // upsampler `stage`: 2-tap conv with u * C columns over L + 1 rows
            if (stage < 0 || stage >= c.n_up) { set_error("bvc_test_vocoder_layer: no upsampler %d", stage); return BVC_EINVAL; }
            rows = (L + 1) * c.up_rates[stage]; ch = m->stage_ch[stage];
            if (m->stage_sym[stage]) {
                // a symmetric upsampler: the causal rows into a buffer of this call, then the view the stage works on - L * rate rows from
                // row rate / 2 on - into d_out
                const int u = c.up_rates[stage];
                const long long full = rows * ch;
                float *tmp = nullptr;
                if (hipMalloc(reinterpret_cast<void **>(&tmp), (size_t)B * full * sizeof(float)) != hipSuccess) {
                    (void)hipGetLastError();
                    set_error("bvc_test_vocoder_layer: cannot allocate the causal rows"); return BVC_ENOMEM;
                }
                rows = L * u;
                rc = launch_conv_mfma(m->ups[stage], d_x, L, tmp, L + 1, B, CE_STORE, nullptr, nullptr, 1.0f, s);
                if (!rc) rc = copy_rows(tmp + (long long)(u / 2) * ch, full, d_out, rows * ch, rows * ch, B, s);
                const hipError_t e1 = hipStreamSynchronize(s);
                (void)hipFree(tmp);
                if (!rc && e1 != hipSuccess) { set_error("bvc_test_vocoder_layer: %s", hipGetErrorString(e1)); rc = BVC_EHIP; }
                break;
            }
            rc = launch_conv_mfma(m->ups[stage], d_x, L, d_out, L + 1, B, CE_STORE, nullptr, nullptr, 1.0f, s);
            break;
        case 2: {                                                            // AMP pair (stage, block, iteration)
            if (stage < 0 || stage >= c.n_up || block < 0 || block >= c.n_resk || iteration < 0 || iteration >= 3) {
                set_error("bvc_test_vocoder_layer: no AMP pair (%d, %d, %d)", stage, block, iteration); return BVC_EINVAL; }
            if (epi < CE_RES || epi > CE_RES_ACC_DIV || (epi >= CE_RES_ACC && !d_acc)) {
                set_error("bvc_test_vocoder_layer: epilogue %d (1 residual, 2 + running sum, 3 + running sum, / kernels; 2 and 3 need d_acc)", epi);
                return BVC_EINVAL; }
            if (!m->fused_amp) { set_error("bvc_test_vocoder_layer: the model runs its AMP pairs unfused"); return BVC_EINVAL; }
            if (window && m->noncausal) { set_error("bvc_test_vocoder_layer: %s - no streaming window", not_causal(m)); return BVC_EINVAL; }
            if (window && (row_begin < 0 || row_begin >= L)) { set_error("bvc_test_vocoder_layer: row_begin outside the buffer"); return BVC_EINVAL; }
            const AmpPair &ap = m->amp[stage][block][iteration];
            rows = L; ch = m->stage_ch[stage];
            const long long bs = (long long)L * ch;
            ConvWindow w{bs, bs, row_begin, t_origin};
            rc = launch_amp_pair(ap.c1, ap.c2, d_x, L, d_out, B, epi, d_acc, (float)c.n_resk, s, window ? &w : nullptr, m->amp_kernels,
                                 m->stage_sym[stage]);
            break;
        }
        case 3:                                                              // activation_post -> conv_post -> tanh -> / div, first `length` samples
            rows = length < L ? length : L; ch = 1;
            if (rows <= 0) { set_error("bvc_test_vocoder_layer: length %lld", (long long)length); return BVC_EINVAL; }
            rc = launch_conv_post(d_x, L, m->post_c, m->post_ks, m->post_w, m->post_b, m->post_a, m->post_ib, div, d_out, rows, B, s,
                                  nullptr, nullptr, m->post_up, m->post_down, m->post_sym);
            break;
        default: set_error("bvc_test_vocoder_layer: kind %d", kind); return BVC_EINVAL;
    }
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error("bvc_test_vocoder_layer: %s", hipGetErrorString(e)); rc = BVC_EHIP; }
    if (out_info) {
        out_info[0] = rows; out_info[1] = ch;
        out_info[2] = g_last_amp_launch.tiles; out_info[3] = g_last_amp_launch.workgroups; out_info[4] = g_last_amp_launch.tile_rows;
    }
    return rc;
}

int bvc_test_amp_pair_window(const bvc_model *m, int32_t stage, int32_t block, int32_t iteration, const float *d_x, int32_t B,
                             int64_t L_in, float *d_out, int32_t epi, const float *d_acc, int64_t row_begin, int64_t row_end,
                             int64_t t_origin, int64_t *out_info, void *stream) {
    // test helper (synchronises): ONE launch of a symmetric pair in a look-ahead window, as stream_advance (generator.hip) makes it
    if (!m || !d_x || !d_out || B <= 0 || L_in <= 0) { set_error("bvc_test_amp_pair_window: bad arguments"); return BVC_EINVAL; }
    const bvc_config &c = m->cfg;
    if (stage < 0 || stage >= c.n_up || block < 0 || block >= c.n_resk || iteration < 0 || iteration >= 3) {
        set_error("bvc_test_amp_pair_window: no AMP pair (%d, %d, %d)", stage, block, iteration); return BVC_EINVAL; }
    if (epi < CE_RES || epi > CE_RES_ACC_DIV || (epi >= CE_RES_ACC && !d_acc)) { set_error("bvc_test_amp_pair_window: epilogue %d", epi); return BVC_EINVAL; }
    if (m->antialiased) { set_error("bvc_test_amp_pair_window: %s", not_causal(m)); return BVC_EINVAL; }
    if (!m->stage_sym[stage]) { set_error("bvc_test_amp_pair_window: stage %d is not symmetric", stage); return BVC_EINVAL; }
    if (row_begin < 0 || row_end < row_begin || row_end > L_in) { set_error("bvc_test_amp_pair_window: rows [%lld, %lld) of %lld", (long long)row_begin, (long long)row_end, (long long)L_in); return BVC_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    g_last_amp_launch = {0, 0, 0};
    const AmpPair &ap = m->amp[stage][block][iteration];
    const long long bs = (long long)L_in * m->stage_ch[stage];
    ConvWindow w{bs, bs, row_begin, t_origin};
    w.lookahead = true; w.row_end = row_end;
    int rc = launch_amp_pair(ap.c1, ap.c2, d_x, L_in, d_out, B, epi, d_acc, (float)c.n_resk, s, &w, m->amp_kernels, true);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error("bvc_test_amp_pair_window: %s", hipGetErrorString(e)); rc = BVC_EHIP; }
    if (out_info) {
        out_info[0] = L_in; out_info[1] = m->stage_ch[stage];
        out_info[2] = g_last_amp_launch.tiles; out_info[3] = g_last_amp_launch.workgroups; out_info[4] = g_last_amp_launch.tile_rows;
    }
    return rc;
}

}  // extern "C"
