// Host-only trace of the coder's recurrence schedule, for a sanitizer build (no GPU, no kernel is launched):
//     hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I bernoulli-var-speech-codec_amd/csrc \
//         tools/step_plan_check.hip -o tools/step_plan_check && tools/step_plan_check > trace.txt
// It writes every step plan node by node, the persistent kernel's hop tables, and the launch trace of whole calls of the five drivers,
// as text that is the same from run to run: pointers are printed as offsets into a fake model (M), a fake workspace (W), the caller's
// tensors (C) and the probe buffer (P), all of them reserved address space that is never read or written.  The use: a change of the
// host side that must not change a launch is built twice, once with -DSTEP_PLAN_SOURCE='"<the earlier recurrence.hip>"' (a single
// source of that revision, e.g. from `git show`), once without (the three sources of this tree), and the two traces are compared with
// `cmp`.  The earlier revision's trace is the reference, never a table written by hand.
// The schedule's sources are included as text; what they need from the rest of the library is stubbed here: every launch_* writes one
// line with its name and every argument, and so do the HIP calls the eager paths make (no device is asked for anything).
// Left out: the hipGraph cache and its replay (get_step_graph needs a real capture), and the residency census.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// ---- the HIP calls of the eager paths, traced instead of made
static hipError_t t_hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus *cs);
static hipError_t t_hipGetLastError();
static hipError_t t_hipGetDevice(int *dev);
static hipError_t t_hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
static hipError_t t_hipEventRecord(hipEvent_t e, hipStream_t s);
static hipError_t t_hipEventQuery(hipEvent_t e);
static hipError_t t_hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
static hipError_t t_hipMemsetAsync(void *p, int v, size_t n, hipStream_t s);
#define hipStreamIsCapturing t_hipStreamIsCapturing
#define hipGetLastError t_hipGetLastError
#define hipGetDevice t_hipGetDevice
#define hipEventCreateWithFlags t_hipEventCreateWithFlags
#define hipEventRecord t_hipEventRecord
#define hipEventQuery t_hipEventQuery
#define hipStreamWaitEvent t_hipStreamWaitEvent
#define hipMemsetAsync t_hipMemsetAsync

#ifdef STEP_PLAN_SOURCE
#include STEP_PLAN_SOURCE
#else
#include "../bernoulli-var-speech-codec_amd/csrc/step_plan.hip"
#include "../bernoulli-var-speech-codec_amd/csrc/flow_launch.hip"
#include "../bernoulli-var-speech-codec_amd/csrc/recurrence.hip"
#endif

using namespace bvc;

// ---- reserved address space, and pointers as text
static const size_t REGION = (size_t)1 << 32;
static char *g_region[4];                                   // M, W, C, P
static const char REGION_NAME[] = "MWCP";
static size_t g_used[4];
static float *take(int region, size_t nfloats) {            // distinct, 256-byte aligned, with a gap behind
    float *p = reinterpret_cast<float *>(g_region[region] + g_used[region]);
    g_used[region] += (nfloats * sizeof(float) + 4096 + 255) / 256 * 256;
    if (g_used[region] > REGION) { fprintf(stderr, "region %c is full\n", REGION_NAME[region]); exit(2); }
    return p;
}
static int g_unknown = 0;
static const char *P(const void *p) {
    static char buf[64][40];
    static int n = 0;
    char *b = buf[n++ & 63];
    const char *c = static_cast<const char *>(p);
    if (!p) return "0";
    for (int r = 0; r < 4; ++r)
        if (c >= g_region[r] && c < g_region[r] + REGION) { snprintf(b, 40, "%c+%zx", REGION_NAME[r], (size_t)(c - g_region[r])); return b; }
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    if (v < 0x10000) { snprintf(b, 40, "#%zx", (size_t)v); return b; }      // a fake stream or event handle
    ++g_unknown;
    return "?";
}

static long g_launch_lines = 0;
static void line(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    ++g_launch_lines;
}

static void put(const DynPtr &d) { printf("{%s ld %d poff %d meta %x dim %d}", P(d.base), d.ld, d.poff, d.meta, d.dim); }
static void put(const GemmSeg &s) { printf("{w %s wnb %d K %d x ", P(s.w), s.wnb, s.K); put(s.x); printf(" grp %d pad %d}", s.grp, s.pad_); }
static void put(const GemmParams &p) {
    printf("M %d N %d nb %d gate_rows %d nseg %d var_bit %d sample %d gate_il %d bias0 %s bias1 %s", p.M, p.N, p.nb_total, p.gate_rows, p.nseg,
           p.var_bit, p.sample, p.gate_il, P(p.bias0), P(p.bias1));
    for (int i = 0; i < 3; ++i) { printf(" seg%d ", i); put(p.seg[i]); }
    printf(" y "); put(p.y); printf(" y2 "); put(p.y2); printf(" y3 "); put(p.y3); printf(" aux "); put(p.aux);
    printf(" part_i %s part_h %s ldpart %lld mean %s stdv %s desc %s probe %s node %d tstep %d frames %d", P(p.part_i), P(p.part_h), p.ldpart,
           P(p.mean), P(p.stdv), P(p.desc), P(p.probe), p.node, p.tstep, p.frames);
}
static void put(const VbrStep &v) {
    printf("desc %s call %s B %d K %d Z %d H %d X %d zraw %s hbuf %s MH %lld zc %s hrep %s melk %s dnk %s pzk %s pzsel %s dnsel %s", P(v.desc),
           P(v.call), v.B, v.K, v.Z, v.H, v.X, P(v.zraw), P(v.hbuf), v.MH, P(v.zc), P(v.hrep), P(v.melk), P(v.dnk), P(v.pzk), P(v.pzsel), P(v.dnsel));
}
static void put(const CallDesc &d) {
    for (int i = 0; i < DS_NSLOT; ++i) printf("p%d %s ", i, P(d.p[i]));
    printf("T %lld t %d nodes %d", d.T, d.t, d.nodes_per_step);
}
static void put(const FlowLin &f) { printf("{w %s bias %s wnb %d pad %d}", P(f.w), P(f.bias), f.wnb, f.pad_); }
static void put(const FlowArgs &a) {
    const FlowLin *l = &a.enc0h;
    static const char *const names[] = {"enc0h", "enc1", "enc2", "pz0", "pz1", "pz2", "dec0h", "dec0z", "dec1", "dec2", "dec3", "px0", "px1", "px2"};
    static_assert(offsetof(FlowArgs, px2) - offsetof(FlowArgs, enc0h) == 13 * sizeof(FlowLin), "the fourteen layers lie in a row");
    for (int i = 0; i < 14; ++i) { printf("%s ", names[i]); put(l[i]); printf(" "); }
    printf("pxc "); put(a.pxc);
    printf(" w_hh %s w_ihx %s w_ihz %s b_ih %s b_hh %s hb %d zb %d xb %d flow %s slot_bytes %u B %d MT %d NTG %d T %lld part0 %s part_gru %s codes %s prob %s"
           " bits %s all_h %s mel %s mean %s stdv %s var_bit %d status %s spin %u probe %s probe_nodes %d probe_first %d probe_wg %d probe_wave %d hot_w %d"
           " MG %d withhold %d keep %s codes_in %s",
           P(a.w_hh), P(a.w_ihx), P(a.w_ihz), P(a.b_ih), P(a.b_hh), a.hb, a.zb, a.xb, P(a.flow), a.slot_bytes, a.B, a.MT, a.NTG, a.T, P(a.part0),
           P(a.part_gru), P(a.codes), P(a.prob), P(a.bits), P(a.all_h), P(a.mel), P(a.mean), P(a.stdv), a.var_bit, P(a.status), a.spin_limit,
           P(a.probe), a.probe_nodes, a.probe_first, a.probe_wg, a.probe_wave, a.dbg_hot_w, a.MG, a.dbg_withhold, P(a.keep), P(a.codes_in));
}

// ---- what the sources need from the rest of the library
static char g_msg[512];
namespace bvc {
thread_local bool g_capturing = false;
KProbe g_kprobe;
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }
ProbeScope::ProbeScope(int kind, hipStream_t stream) : s(stream), slot(-1) { line("ProbeScope kind %d s %s\n", kind, P(stream)); }
ProbeScope::~ProbeScope() {}
int flow_census(const bvc_model *) { line("flow_census\n"); return BVC_OK; }

int launch_gemm_skinny(const GemmParams &p, int epi, hipStream_t s, int mtw) {
    printf("launch_gemm_skinny epi %d s %s mtw %d ", epi, P(s), mtw); put(p); line("\n");
    return BVC_OK;
}
int launch_step_advance(CallDesc *d, int by, hipStream_t s) { line("launch_step_advance d %s by %d s %s\n", P(d), by, P(s)); return BVC_OK; }
int launch_set_desc(CallDesc *d, const CallDesc &v, hipStream_t s) {
    printf("launch_set_desc d %s s %s ", P(d), P(s)); put(v); line("\n");
    return BVC_OK;
}
int launch_gemm_batched(const float *x, long long ldx, const float *w, long long ldw, const float *bias, int M, int N, int K, int act, float *y,
                        long long ldy, hipStream_t s, int out_mode, long long frames_T, int mt16) {
    line("launch_gemm_batched x %s ldx %lld w %s ldw %lld bias %s M %d N %d K %d act %d y %s ldy %lld s %s out_mode %d frames_T %lld mt16 %d\n", P(x), ldx,
         P(w), ldw, P(bias), M, N, K, act, P(y), ldy, P(s), out_mode, frames_T, mt16);
    return BVC_OK;
}
int launch_normalize_rows(const float *y, const float *mean, const float *stdv, long long rows, int n, float *out, hipStream_t s) {
    line("launch_normalize_rows y %s mean %s stdv %s rows %lld n %d out %s s %s\n", P(y), P(mean), P(stdv), rows, n, P(out), P(s));
    return BVC_OK;
}
int launch_fill(float *p, float v, long long n, hipStream_t s) { line("launch_fill p %s v %g n %lld s %s\n", P(p), v, n, P(s)); return BVC_OK; }
int launch_fill_u32(unsigned *p, unsigned v, long long n, hipStream_t s) { line("launch_fill_u32 p %s v %x n %lld s %s\n", P(p), v, n, P(s)); return BVC_OK; }
int launch_kld_frames(const float *prob, const float *prior, const float *bits, int B, long long T, int Z, float *kld, hipStream_t s) {
    line("launch_kld_frames prob %s prior %s bits %s B %d T %lld Z %d kld %s s %s\n", P(prob), P(prior), P(bits), B, T, Z, P(kld), P(s));
    return BVC_OK;
}
int launch_repack_rows(const float *src, float *dst, long long ld_natural, int rows, int n, int dir, hipStream_t s) {
    line("launch_repack_rows src %s dst %s ld %lld rows %d n %d dir %d s %s\n", P(src), P(dst), ld_natural, rows, n, dir, P(s));
    return BVC_OK;
}
int launch_flow(const FlowArgs &a, FlowArgs *d_args, int perh, bool encode, bool fill, hipStream_t s, bool args_resident, bool conceal) {
    printf("launch_flow d_args %s perh %d encode %d fill %d s %s args_resident %d conceal %d ", P(d_args), perh, (int)encode, (int)fill, P(s),
           (int)args_resident, (int)conceal);
    put(a); line("\n");
    return BVC_OK;
}
int launch_flow_prepare(const FlowArgs &a, FlowArgs *d_args, unsigned *flow, long long n_flow, long long n_h0, const float *d_h0, int B, int H,
                        hipStream_t s) {
    printf("launch_flow_prepare d_args %s flow %s n_flow %lld n_h0 %lld d_h0 %s B %d H %d s %s ", P(d_args), P(flow), n_flow, n_h0, P(d_h0), B, H, P(s));
    put(a); line("\n");
    return BVC_OK;
}
int launch_vbr_set_call(VbrCall *d, const VbrCall &v, hipStream_t s) {
    printf("launch_vbr_set_call d %s s %s y %s tau %s codes %s bits %s dist %s dec %s choice %s ladder", P(d), P(s), P(v.y), P(v.tau), P(v.codes), P(v.bits),
           P(v.dist), P(v.dec), P(v.choice));
    for (int k = 0; k < VBR_MAX_RUNGS; ++k) printf(" %d", v.ladder[k]);
    line("\n");
    return BVC_OK;
}
int launch_vbr_candidates(const VbrStep &a, int tstep, hipStream_t s) { printf("launch_vbr_candidates tstep %d s %s ", tstep, P(s)); put(a); line("\n"); return BVC_OK; }
int launch_vbr_select(const VbrStep &a, int tstep, hipStream_t s) { printf("launch_vbr_select tstep %d s %s ", tstep, P(s)); put(a); line("\n"); return BVC_OK; }
}  // namespace bvc

static uintptr_t g_events = 0;
static hipError_t t_hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus *cs) { *cs = hipStreamCaptureStatusNone; line("hipStreamIsCapturing s %s\n", P(s)); return hipSuccess; }
static hipError_t t_hipGetLastError() { line("hipGetLastError\n"); return hipSuccess; }
static hipError_t t_hipGetDevice(int *dev) { *dev = 3; line("hipGetDevice\n"); return hipSuccess; }
static hipError_t t_hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
    *e = reinterpret_cast<hipEvent_t>(0xE00 + ++g_events);
    line("hipEventCreateWithFlags -> %s flags %u\n", P(*e), flags);
    return hipSuccess;
}
static hipError_t t_hipEventRecord(hipEvent_t e, hipStream_t s) { line("hipEventRecord e %s s %s\n", P(e), P(s)); return hipSuccess; }
static hipError_t t_hipEventQuery(hipEvent_t e) { line("hipEventQuery e %s\n", P(e)); return hipSuccess; }
static hipError_t t_hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) { line("hipStreamWaitEvent s %s e %s flags %u\n", P(s), P(e), flags); return hipSuccess; }
static hipError_t t_hipMemsetAsync(void *p, int v, size_t n, hipStream_t s) { line("hipMemsetAsync p %s v %d n %zu s %s\n", P(p), v, n, P(s)); return hipSuccess; }

// ---- the fake model and workspace
static Linear fake_linear(int in, int out) {
    Linear l;
    l.w = take(0, (size_t)in * out); l.wp = take(0, (size_t)in * out); l.b = take(0, out); l.in = in; l.out = out;
    return l;
}
static void fake_model(bvc_model *m, int H, int Z, int X, int var_bit) {
    memset(&m->cfg, 0, sizeof m->cfg);
    m->cfg.h_dim = H; m->cfg.z_dim = Z; m->cfg.num_mels = X; m->cfg.var_bit = var_bit;
    m->mean_mel = take(0, X); m->std_mel = take(0, X);
    const int in_x[3] = {X, H, H}, in_z[3] = {Z, H, H}, in_e[3] = {2 * H, H, H}, out_e[3] = {H, H, Z}, in_p[3] = {H, H, H};
    for (int i = 0; i < 3; ++i) {
        m->phi_x[i] = fake_linear(in_x[i], H);
        m->phi_z[i] = fake_linear(in_z[i], H);
        m->enc[i] = fake_linear(in_e[i], out_e[i]);
        m->prior[i] = fake_linear(in_p[i], out_e[i]);
    }
    m->dec[0] = fake_linear(2 * H, H); m->dec[1] = fake_linear(H, H); m->dec[2] = fake_linear(H, H); m->dec[3] = fake_linear(H, X);
    m->px0_dec3 = fake_linear(H, H);
    m->has_prior = true;
    m->w_ih = take(0, (size_t)6 * H * H); m->w_hh = take(0, (size_t)3 * H * H); m->b_ih = take(0, 3 * H); m->b_hh = take(0, 3 * H);
    m->w_ih_il = take(0, (size_t)6 * H * H); m->w_hh_il = take(0, (size_t)3 * H * H); m->w_ih_nat = take(0, (size_t)6 * H * H);
    m->d_status = reinterpret_cast<unsigned *>(take(0, 1));
    m->use_graph = false;
    m->recurrence = RS_LAYERS;
    m->cu_count = 256;
    m->flow_perh = 1;
    m->flow_resident = true;
}
static void fake_workspace(Workspace *w, int B, int64_t T, int H, int Z, int X) {
    memset(w, 0, sizeof *w);
    const size_t mt16 = (size_t)(B + 15) / 16 * 16, big = (size_t)mt16 * T * (3 * H + Z + X);
    w->yn = take(1, big); w->pxA = take(1, big); w->pxB = take(1, big); w->pxC = take(1, big);
    for (float *&p : w->step) p = take(1, mt16 * (3 * H + Z + X));
    w->hbuf = take(1, 2 * mt16 * H);
    w->part_i = take(1, mt16 * 3 * H); w->part_h = take(1, mt16 * 3 * H); w->part_d = take(1, mt16 * H);
    w->desc = reinterpret_cast<CallDesc *>(take(1, sizeof(CallDesc)));
    w->mel = take(1, big); w->bits = take(1, big);
    w->part_dec0 = take(1, big); w->part_gru = take(1, big);
    w->flow_slot = mt16 * (size_t)(H > X ? H : X);
    w->flow = take(1, (size_t)FB_COUNT * 2 * w->flow_slot);
    w->flow_args = reinterpret_cast<FlowArgs *>(take(1, sizeof(FlowArgs)));
}

static long g_plans = 0, g_nodes = 0;
static void put_plan(const char *what, const std::vector<StepNode> &plan) {
    printf("plan %s: %zu nodes, %d kernels\n", what, plan.size(), count_kernels(plan));
    ++g_plans;
    for (const StepNode &n : plan) {
        printf("  node op %d branch %d event %d epi %d | ", n.op, n.branch, n.event, n.epi); put(n.p); printf(" | "); put(n.v); printf("\n");
        ++g_nodes;
    }
}

static int g_failed = 0;
static void call(const char *what, int rc) {
    printf("call %s -> %d%s%s\n", what, rc, rc ? " " : "", rc ? g_msg : "");
    if (rc) ++g_failed;
}

int main() {
    for (char *&r : g_region) {
        void *p = mmap(nullptr, REGION, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { perror("mmap"); return 2; }
        r = static_cast<char *>(p);
    }
    g_kprobe.dev = reinterpret_cast<unsigned long long *>(take(3, 1 << 20));
    g_kprobe.capacity = (size_t)1 << 20;
    hipStream_t s = reinterpret_cast<hipStream_t>(0x51), s2 = reinterpret_cast<hipStream_t>(0x52);
    char what[256];
    const int Z = 64, X = 80;
    for (int H : {64, 128})
        for (int var_bit : {0, 1})
            for (int B : {5, 17}) {
                for (size_t &u : g_used) u = 0;                  // the same addresses for every configuration
                (void)take(3, 1 << 20);
                bvc_model m;
                fake_model(&m, H, Z, X, var_bit);
                Workspace w;
                VbrWorkspace vw[2];
                const int RUNGS[2] = {1, 3};
                for (int i = 0; i < 2; ++i) carve_vbr(&m, B, RUNGS[i], reinterpret_cast<char *>(take(1, (size_t)1 << 22)), &vw[i]);
                fake_workspace(&w, B, 21, H, Z, X);
                printf("==== h_dim %d var_bit %d B %d\n", H, var_bit, B);
                // ---- every plan
                for (bool probes : {false, true}) {
                    g_kprobe.enabled = probes;
                    for (bool side : {false, true}) {
                        m.side_branch = side;
                        for (int kind : {STEP_ENCODE, STEP_DECODE, STEP_DECODE_PRE, STEP_CONCEAL})
                            for (int fold : {0, (int)STEP_FOLD}) {
                                snprintf(what, sizeof what, "build_step kind %d fold %d side %d probes %d", kind, fold != 0, (int)side, (int)probes);
                                put_plan(what, build_step(&m, w, B, kind | fold));
                            }
                    }
                    m.side_branch = false;
                    for (int i = 0; i < 2; ++i) {
                        snprintf(what, sizeof what, "build_vbr_step K %d probes %d", RUNGS[i], (int)probes);
                        put_plan(what, build_vbr_step(&m, w, vw[i], B, RUNGS[i]));
                    }
                    for (int sel : {0, 1})
                        for (bool greedy : {false, true})
                            for (int upd : {1, 2, 3}) {
                                snprintf(what, sizeof what, "build_forward_step sel %d greedy %d update_h %d update_h2 %d probes %d", sel, (int)greedy, upd & 1, upd >> 1, (int)probes);
                                put_plan(what, build_forward_step(&m, w, B, sel, greedy, (upd & 1) != 0, (upd & 2) != 0));
                            }
                }
                g_kprobe.enabled = false;
                // ---- the hop tables
                for (int fold : {1, 0}) {
                    m.encode_fold = m.decode_fold = fold;
                    for (int program = 0; program < 3; ++program) {         // encode, decode, conceal
                        FlowArgs a;
                        memset(&a, 0, sizeof a);
                        flow_layers(&m, program != 1, &a, program == 2);
                        printf("hops program %d fold %d: ", program, fold); put(a); printf("\n");
                    }
                }
                // ---- whole calls: the launch-per-layer schedule, eager; then the persistent schedule's host side
                float *mel = take(2, 1 << 16), *bits = take(2, 1 << 16), *h0 = take(2, 1 << 16), *codes = take(2, 1 << 16), *all_h = take(2, 1 << 16),
                      *hT = take(2, 1 << 16), *prob = take(2, 1 << 16), *melhat = take(2, 1 << 16), *tau = take(2, 1 << 16), *dist = take(2, 1 << 16),
                      *dec = take(2, 1 << 16), *sel = take(2, 1 << 16), *codes_out = take(2, 1 << 16), *prior = take(2, 1 << 16), *noise = take(2, 1 << 16),
                      *kld = take(2, 1 << 16), *zz = take(2, 1 << 16);
                void *ws_base = g_region[1];
                const int ladder[3] = {16, 32, 64};
                uint8_t use_gen[21];
                for (int t = 0; t < 21; ++t) use_gen[t] = (uint8_t)((t * 5 % 3) == 1);
                for (int schedule : {(int)RS_LAYERS, (int)RS_PERSISTENT, (int)RS_AUTO})
                    for (int64_t T : {(int64_t)3, (int64_t)21})
                        for (bool probes : {false, true})
                            for (int fold : {1, 0})
                                for (bool side : {false, true}) {
                                    if (side && (schedule != RS_LAYERS || probes)) continue;
                                    m.recurrence = schedule; m.side_branch = side; m.encode_fold = m.decode_fold = fold;
                                    g_kprobe.enabled = probes;
                                    printf("---- schedule %d T %lld probes %d fold %d side %d\n", schedule, (long long)T, (int)probes, fold, (int)side);
                                    hipStream_t st = (T == 3) ? s : s2;          // (RS_AUTO: the last call ran on another stream)
                                    call("run_encode", run_encode(&m, w, ws_base, mel, bits, h0, B, T, codes, all_h, hT, prob, st, nullptr));
                                    call("run_encode zero state, melhat", run_encode(&m, w, ws_base, mel, bits, nullptr, B, T, codes, nullptr, nullptr, prob, st, melhat));
                                    call("run_encode no bits", run_encode(&m, w, ws_base, mel, nullptr, h0, B, T, codes, all_h, hT, prob, st, nullptr));
                                    for (int i = 0; i < 2; ++i)
                                        call("run_encode_vbr", run_encode_vbr(&m, w, vw[i], ws_base, mel, tau, ladder, RUNGS[i], i ? h0 : nullptr, B, T, codes, bits,
                                                                              i ? all_h : nullptr, i ? hT : nullptr, prob, i ? dist : nullptr, i ? dec : nullptr, st));
                                    for (bool pre : {true, false}) {
                                        m.precomp_pz = pre;
                                        call(pre ? "run_decode precomp" : "run_decode in-step phi_z", run_decode(&m, w, ws_base, codes, pre ? h0 : nullptr, B, T, mel, pre ? hT : nullptr, st));
                                    }
                                    m.precomp_pz = true;
                                    call("run_decode_conceal", run_decode_conceal(&m, w, ws_base, codes, sel, h0, B, T, mel, hT, codes_out, prior, st));
                                    call("run_decode_conceal bare", run_decode_conceal(&m, w, ws_base, codes, sel, nullptr, B, T, mel, nullptr, nullptr, nullptr, st));
                                    if (schedule != RS_LAYERS) call("bvc_flow_fence", bvc_flow_fence(s2));
                                    if (schedule != RS_LAYERS) continue;
                                    for (int upd : {1, 2, 3}) {
                                        call("run_forward sampled", run_forward(&m, w, mel, bits, use_gen, (upd & 1) != 0, (upd & 2) != 0, noise, B, T, dec, kld, zz, prob, prior, st));
                                        call("run_forward greedy, own buffers", run_forward(&m, w, mel, bits, use_gen, (upd & 1) != 0, (upd & 2) != 0, nullptr, B, T, dec, kld, nullptr, nullptr, nullptr, st));
                                    }
                                }
                g_kprobe.enabled = false;
            }
    // refusals stay what they are (var_bit without bits is one of the calls above: it counts as failed there)
    printf("step_plan_check: %ld plans, %ld nodes, %ld launch lines, %d refused calls, %d unknown pointers\n", g_plans, g_nodes, g_launch_lines, g_failed, g_unknown);
    fprintf(stderr, "step_plan_check: %ld plans, %ld nodes, %ld launch lines, %d refused calls, %d unknown pointers\n", g_plans, g_nodes, g_launch_lines, g_failed, g_unknown);
    return g_unknown != 0;
}
