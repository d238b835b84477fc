// What every call runs on a model: the workspace layout, the sticky status of the persistent recurrence, its residency census, and the
// option and status entry points.  The model itself is made in model_build.hip.
#include <algorithm>
#include <cstdio>

#include "bvc_host.h"

using namespace bvc;

namespace {

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// length after upsampler `stage`: a symmetric one drops the u-row tail; causal: as if no stage were symmetric
int64_t stage_rows(const bvc_model *m, int64_t T, int stage, bool causal) {
    int64_t L = T;
    for (int i = 0; i <= stage; ++i) L = (!causal && (size_t)i < m->stage_sym.size() && m->stage_sym[i] ? L : L + 1) * m->cfg.up_rates[i];
    return L;
}

// Takes the sticky status word of the persistent kernels (no synchronisation): a code that is there is cleared, and the residency
// census runs again before the next persistent launch
unsigned take_status(const bvc_model *m) {
    const unsigned v = m->h_status ? *m->h_status : 0u;
    if (v) { *m->h_status = 0u; m->census_due = true; }
    return v;
}

// The status word as a result: BVC_ETIMEOUT with the frame and the layer it names between the caller's two halves of the sentence;
// together: followed by what a persistent launch needs
int report_status(const bvc_model *m, uint32_t *code, const char *whose, const char *what, bool together) {
    const unsigned v = take_status(m);
    if (code) *code = v;
    if (!v) return BVC_OK;
    set_error("a persistent recurrence kernel%s gave up waiting (frame %u, layer %u): %s%s", whose, (v & 0x7FFFFFFFu) >> 4, (v & 15u), what,
              together ? ".  All its workgroups must be resident together - is another process using this GPU?" : "");
    return BVC_ETIMEOUT;
}

}  // namespace

namespace bvc {

const char *const NOT_CAUSAL = "the model has anti-aliased activations: a filtered AMP block looks 30 rows ahead, so the generator is not causal";

const char *const NOT_CAUSAL_SYM = "the model has symmetric layers: a symmetric layer reads as many rows ahead as behind, so the generator is not causal";
const char *not_causal(const bvc_model *m) { return m->antialiased ? NOT_CAUSAL : NOT_CAUSAL_SYM; }

// ---- persistent recurrence (k_flow.hip): hop tables and launch -----------------------------------------
// Is the model laid out for the persistent kernel?  (h_dim a multiple of 128 up to 1024 or below 128; narrow z / mel layers)
int build_flow(bvc_model *m) {
    const int H = m->cfg.h_dim, Z = m->cfg.z_dim, X = m->cfg.num_mels;
    m->flow_perh = flow_perh(H);
    if (Z > 128 || X > 128) m->flow_perh = 0;
    if (!m->flow_perh) return BVC_OK;
    void *st = nullptr, *dst = nullptr;
    BVC_HIP_TRY(hipHostMalloc(&st, 64, hipHostMallocMapped | hipHostMallocCoherent));
    memset(st, 0, 64);
    m->h_status = static_cast<volatile unsigned *>(st);
    BVC_HIP_TRY(hipHostGetDevicePointer(&dst, st, 0));
    m->d_status = static_cast<unsigned *>(dst);
    int dev = 0;
    BVC_HIP_TRY(hipGetDevice(&dev));
    BVC_HIP_TRY(hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, dev));
    int rc = flow_kernels_init();
    if (rc) return rc;
    return flow_census(m);
}

int64_t stage_len(const bvc_model *m, int64_t T, int stage) { return stage_rows(m, T, stage, false); }

void carve(const bvc_model *m, int B, int64_t T, char *base, Workspace *w) {
    const bvc_config &c = m->cfg;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float *p = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(base) + off);     // (base is null where only the size is asked for)
        off += align_up(nfloats * sizeof(float));
        return p;
    };
    const size_t BT = (size_t)B * (size_t)T;
    const int H = c.h_dim;
    const int vmax = std::max(H, c.num_mels), dmax = std::max(vmax, c.z_dim);
    const size_t mt16 = (size_t)pad16(B);                      // fragment-packed matrices hold whole 16-row tiles
    // buffers referenced by the captured step graphs come first: their offsets depend on B only, so a
    // graph captured for (B, workspace) stays valid for every T
    for (int i = 0; i < 16; ++i) w->step[i] = take(mt16 * vmax);
    w->hbuf = take(2 * mt16 * H);
    w->part_i = take(mt16 * 3 * H);
    w->part_h = take(mt16 * 3 * H);
    w->part_d = take(mt16 * H);
    w->desc = reinterpret_cast<CallDesc *>(take(64));
    w->flow_slot = mt16 * (size_t)dmax;
    w->flow = take((size_t)FB_COUNT * 2 * w->flow_slot);
    w->flow_args = reinterpret_cast<FlowArgs *>(take((sizeof(FlowArgs) + 3) / 4));
    w->yn = take(BT * c.num_mels);
    w->pxA = take(mt16 * (size_t)T * H);                       // final phi_x / phi_z: frame-packed
    w->pxB = take(mt16 * (size_t)T * H);                       // intermediates of the batched MLPs: frame-major rows
    w->pxC = take(mt16 * (size_t)T * H);
    w->mel = take(BT * c.num_mels);
    w->bits = take(BT);
    w->part_dec0 = take(BT * H);
    w->part_gru = take(BT * 3 * H);
    size_t maxel = 0;                                           // the causal lengths: upper bounds of a symmetric generator's, whose
    for (int i = 0; i < c.n_up; ++i)                            // stages work on views of the causal upsampler results
        maxel = std::max(maxel, (size_t)stage_rows(m, T, i, true) * m->stage_ch[i]);
    w->y0 = take((size_t)B * T * c.upsample_initial_channel);
    w->X = take((size_t)B * maxel);
    w->P = take((size_t)B * maxel);
    w->Q = take((size_t)B * maxel);
    w->U = take((size_t)B * maxel);
    w->XS = take((size_t)B * maxel);
    w->total = off;
}

int check_ws(const bvc_model *m, int B, int64_t T, void *d_ws, size_t ws_bytes, Workspace *w) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (B <= 0 || T <= 0) { set_error("B and T must be positive (B=%d, T=%lld)", B, (long long)T); return BVC_EINVAL; }
    carve(m, B, T, static_cast<char *>(d_ws), w);
    if (!d_ws || ws_bytes < w->total) {
        set_error("workspace too small: %zu bytes given, %zu needed", ws_bytes, w->total);
        return BVC_ENOMEM;
    }
    return BVC_OK;
}

// Reads the sticky status word (no synchronisation): the first call after a persistent kernel gave up reports it.
int sticky_status(const bvc_model *m) {
    if (!m) return BVC_OK;
    return report_status(m, nullptr, " of an earlier call", "the results of that call are invalid", true);
}

int need_prior(const bvc_model *m, const char *fn) {
    if (m && !m->has_prior) { set_error("%s: the model was created without the prior.* tensors", fn); return BVC_EMISSING; }
    return BVC_OK;
}

// One-off at model creation: can a full persistent grid (one workgroup per compute unit the device reports) be resident at
// once?  flow_census_kernel has the recurrence kernels' footprint - 512 threads, every VGPR, the filler kernels' LDS -: every
// workgroup adds itself to a counter and waits (bounded) until all have.  A CU mask, a partition mode or another tenant of the
// device that keeps workgroups from becoming co-resident shows up here; the model then stays on the launch-per-layer schedule
// (flow_resident = false).
int flow_census(const bvc_model *m) {
    m->flow_resident = false;
    const int ntg = flow_grid_tiles(m);
    int slots = m->cu_count / ntg;
    if (slots <= 0) return BVC_OK;
    std::lock_guard<std::mutex> lk(g_flow_mu);           // (no persistent launch of this process starts beside the census)
    if (!m->census_ctr) BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m->census_ctr), 64));
    unsigned *ctr = m->census_ctr;
    // a stream of the library's own, synchronised on its own: neither the null stream nor hipDeviceSynchronize() is legal while
    // another thread captures a graph
    if (!m->census_stream) BVC_HIP_TRY(hipStreamCreateWithFlags(&m->census_stream, hipStreamNonBlocking));
    const ModelSwitches sw = model_switches();
    if (sw.census_oversubscribe) slots += 1;             // tests: a grid the device cannot hold
    const int grid = ntg * slots;
    unsigned h[2] = {0u, 0u};
    for (int attempt = 0; attempt < 2; ++attempt) {
        BVC_HIP_TRY(hipMemsetAsync(ctr, 0, 64, m->census_stream));
        // ~50 ms: a workgroup that has to queue behind a resident one shows up as a time-out
        const int rc = launch_flow_census(ctr, grid, 200000u, m->census_stream);
        hipError_t e = hipStreamSynchronize(m->census_stream);
        if (e == hipSuccess) e = hipMemcpy(h, ctr, sizeof(h), hipMemcpyDeviceToHost);
        if (rc) return rc;
        BVC_HIP_TRY(e);
        m->flow_resident = h[0] == (unsigned)grid && h[1] == 0u;
        if (m->flow_resident || attempt == 1) break;
        // "device busy" is not "grid does not fit": work of this process on other streams (another model serving, say) holds
        // compute units for a while - let it drain and count once more before giving the persistent schedule up for good
        if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); break; }       // (illegal under a capture: keep the first answer)
    }
    if (!m->flow_resident && !sw.quiet)
        fprintf(stderr, "bvcodec: residency census: %u of %d recurrence workgroups became co-resident (%u gave up) - this model stays on the "
                        "launch-per-layer schedule (get_option \"flow_resident\" = 0).  Is another process using this GPU?\n", h[0] - h[1], grid, h[1]);
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int bvc_model_set_option(bvc_model *m, const char *name, int32_t value) {
    if (!m || !name) { set_error("bvc_model_set_option: null argument"); return BVC_EINVAL; }
    if (strcmp(name, "recurrence") == 0) {
        // 0: persistent kernel for every call, 1: one launch per layer for every call, 2 (default): automatic - persistent while
        // calls come one at a time, launch per layer while calls of several streams overlap (see flow_chains)
        if (value < 0 || value > 2) { set_error("bvc_model_set_option: recurrence must be 0 (persistent), 1 (layers) or 2 (auto)"); return BVC_EINVAL; }
        m->recurrence = value;
        return BVC_OK;
    }
    if (strcmp(name, "flow_spin_limit") == 0) {            // polls before a wait inside the persistent kernel gives up (tests)
        if (value < 1) { set_error("bvc_model_set_option: flow_spin_limit must be positive"); return BVC_EINVAL; }
        m->flow_spin_limit = (unsigned)value;
        return BVC_OK;
    }
    // flags.  flow_debug_withhold, tests only: workgroup 0 of every persistent launch does nothing; flow_debug_nofill, tests only: the layer
    // program without filler quanta; decode_fold, 1 (default): dec.6 -> norm -> phi_x.0 as one layer in the persistent decode kernel;
    // encode_fold: the same in the persistent encode kernel
    for (const auto &f : {std::make_pair("flow_debug_withhold", &m->flow_debug_withhold), std::make_pair("flow_debug_nofill", &m->flow_debug_nofill),
                          std::make_pair("decode_fold", &m->decode_fold), std::make_pair("encode_fold", &m->encode_fold)})
        if (strcmp(name, f.first) == 0) { *f.second = value != 0; return BVC_OK; }
    // 1 (default): C = 16 AMP pairs on the persistent kernel / C = 8 AMP pairs on the two-rows-per-tile kernel; 0: generic kernel.  Same bits
    for (const auto &k : {std::make_pair("vocoder_c16_kernel", AMPK_C16), std::make_pair("vocoder_full_tiles", AMPK_C8)})
        if (strcmp(name, k.first) == 0) { m->amp_kernels = value ? (m->amp_kernels | k.second) : (m->amp_kernels & ~k.second); return BVC_OK; }
    set_error("bvc_model_set_option: unknown option '%s'", name);
    return BVC_EINVAL;
}

int bvc_model_get_option(const bvc_model *m, const char *name, int32_t *value) {
    if (!m || !name || !value) { set_error("bvc_model_get_option: null argument"); return BVC_EINVAL; }
    if (strcmp(name, "recurrence") == 0) { *value = m->recurrence; return BVC_OK; }
    if (strcmp(name, "decode_fold") == 0) { *value = m->decode_fold; return BVC_OK; }
    if (strcmp(name, "encode_fold") == 0) { *value = m->encode_fold; return BVC_OK; }
    if (strcmp(name, "flow_resident") == 0) { *value = m->flow_resident ? 1 : 0; return BVC_OK; }       // result of the residency census
    if (strcmp(name, "flow_supported") == 0) { *value = m->flow_perh > 0 ? 1 : 0; return BVC_OK; }    // h_dim laid out for the persistent kernel
    if (strcmp(name, "compute_units") == 0) { *value = m->cu_count; return BVC_OK; }
    set_error("bvc_model_get_option: unknown option '%s'", name);
    return BVC_EINVAL;
}

int bvc_model_status(const bvc_model *m, uint32_t *code) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    if (m->h_status) BVC_HIP_TRY(hipDeviceSynchronize());
    return report_status(m, code, "", "its results are invalid", false);
}

int bvc_model_poll_status(const bvc_model *m, uint32_t *code) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    return report_status(m, code, "", "the results of the call that has just been synchronised are invalid", true);
}

}  // extern "C"
