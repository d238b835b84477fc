// Host-only check of the persistent recurrence's launch table, for a sanitizer build (no GPU, no kernel is launched):
//     hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/flow_host_check.hip -o tools/flow_host_check
// The filler and the plain form of a program give the same bits by design, so no parity test notices a launch that picks the wrong
// twin: this program does.  For every PERH x program x filler on / off, and for the interleaved chains x folded / unfolded, what
// flow_pick returns must be the instantiation written out by hand below (the ladders of if / else this table replaced), with the
// LDS bytes those ladders passed and the bytes FlowLds lays out for the form; the refused combinations keep code and message; the
// capped grid size of the fill kernels is the expression it replaced.
// The two sources are included as text; what they need from the rest of the library is stubbed here.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../bernoulli-var-speech-codec_amd/csrc/k_flow.hip"
#include "../bernoulli-var-speech-codec_amd/csrc/k_flow_support.hip"

static char g_msg[256];
namespace bvc {
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }
}  // namespace bvc

using namespace bvc;

struct Want { int perh; bool encode, fill, conceal, chains, folded; FlowFn fn; size_t lds; };
constexpr size_t PLAIN = 65536, FILL = 147472, MULTI = 131072;       // FLOW_LDS, FLOW_LDS_FILL, FLOW_LDS_MULTI of the ladders
static const Want WANT[] = {
    //perh encode fill conceal chains folded
    {1, true, true, true, false, false, bvrnn_flow_kernel<1, true, true, 8, false, -1, true>, FILL},
    {1, true, false, true, false, false, bvrnn_flow_kernel<1, true, false, 8, false, -1, true>, PLAIN},
    {1, true, true, false, false, false, bvrnn_flow_kernel<1, true, true, 8, false, -1, false>, FILL},
    {1, true, false, false, false, false, bvrnn_flow_kernel<1, true, false, 8, false, -1, false>, PLAIN},
    {1, false, true, false, false, false, bvrnn_flow_kernel<1, false, true, 8, false, -1, false>, FILL},
    {1, false, false, false, false, false, bvrnn_flow_kernel<1, false, false, 8, false, -1, false>, PLAIN},
    {2, true, true, true, false, false, bvrnn_flow_kernel<2, true, true, 8, false, -1, true>, FILL},
    {2, true, false, true, false, false, bvrnn_flow_kernel<2, true, false, 8, false, -1, true>, PLAIN},
    {2, true, true, false, false, false, bvrnn_flow_kernel<2, true, true, 8, false, -1, false>, FILL},
    {2, true, false, false, false, false, bvrnn_flow_kernel<2, true, false, 8, false, -1, false>, PLAIN},
    {2, false, true, false, false, false, bvrnn_flow_kernel<2, false, true, 8, false, -1, false>, FILL},
    {2, false, false, false, false, false, bvrnn_flow_kernel<2, false, false, 8, false, -1, false>, PLAIN},
    {4, true, true, true, false, false, bvrnn_flow_kernel<4, true, true, 8, false, -1, true>, FILL},
    {4, true, false, true, false, false, bvrnn_flow_kernel<4, true, false, 8, false, -1, true>, PLAIN},
    {4, true, true, false, false, false, bvrnn_flow_kernel<4, true, true, 8, false, -1, false>, FILL},
    {4, true, false, false, false, false, bvrnn_flow_kernel<4, true, false, 8, false, -1, false>, PLAIN},
    {4, false, true, false, false, false, bvrnn_flow_kernel<4, false, true, 8, false, -1, false>, FILL},
    {4, false, false, false, false, false, bvrnn_flow_kernel<4, false, false, 8, false, -1, false>, PLAIN},
    {8, true, true, true, false, false, bvrnn_flow_kernel<8, true, true, 8, false, -1, true>, FILL},
    {8, true, false, true, false, false, bvrnn_flow_kernel<8, true, false, 8, false, -1, true>, PLAIN},
    {8, true, true, false, false, false, bvrnn_flow_kernel<8, true, true, 8, false, -1, false>, FILL},
    {8, true, false, false, false, false, bvrnn_flow_kernel<8, true, false, 8, false, -1, false>, PLAIN},
    {8, false, true, false, false, false, bvrnn_flow_kernel<8, false, true, 8, false, -1, false>, FILL},
    {8, false, false, false, false, false, bvrnn_flow_kernel<8, false, false, 8, false, -1, false>, PLAIN},
    // interleaved chains (the filler request is ignored there)
    {8, true, false, true, true, true, bvrnn_flow_kernel<8, true, false, 8, true, 1, true>, MULTI},
    {8, true, false, true, true, false, bvrnn_flow_kernel<8, true, false, 8, true, 0, true>, MULTI},
    {8, true, false, false, true, true, bvrnn_flow_kernel<8, true, false, 8, true, 1, false>, MULTI},
    {8, true, false, false, true, false, bvrnn_flow_kernel<8, true, false, 8, true, 0, false>, MULTI},
    {8, false, false, false, true, true, bvrnn_flow_kernel<8, false, false, 8, true, 1, false>, MULTI},
    {8, false, false, false, true, false, bvrnn_flow_kernel<8, false, false, 8, true, 0, false>, MULTI},
};

static float g_dummy[4];
static FlowArgs args_for(bool conceal, bool chains, bool folded) {
    FlowArgs a;
    memset(&a, 0, sizeof a);
    a.MG = chains ? 3 : 1; a.MT = 5; a.NTG = 64;
    if (folded) a.pxc.w = g_dummy;
    if (conceal) { a.codes_in = g_dummy; a.codes = g_dummy; a.bits = g_dummy; }
    return a;
}

static int refused(const char *what, const FlowArgs &a, int perh, bool encode, bool fill, bool conceal, const char *msg) {
    g_msg[0] = 0;
    const int rc = launch_flow(a, nullptr, perh, encode, fill, nullptr, true, conceal);
    if (rc == BVC_EINVAL && strcmp(g_msg, msg) == 0) return 0;
    printf("%s: rc %d, message \"%s\"\n", what, rc, g_msg);
    return 1;
}

int main() {
    int bad = 0, picks = 0, entries = 0, refusals = 0, grids = 0;
    for (const Want &w : WANT) {
        const FlowArgs a = args_for(w.conceal, w.chains, w.folded);
        for (bool fill : {false, true}) {
            if (!w.chains && fill != w.fill) continue;     // (chains: either request takes the same kernel)
            const FlowKernel *k = flow_pick(a, w.perh, w.encode, fill, w.conceal);
            ++picks;
            const int form = w.chains ? (w.folded ? FF_CHAINS_FOLDED : FF_CHAINS) : (w.fill ? FF_FILL : FF_PLAIN);
            if (!k || k->fn != w.fn || k->lds != w.lds || k->lds != FlowLds<8>::bytes(form) || k->form != form) {
                printf("perh %d encode %d fill %d conceal %d chains %d folded %d: entry %p lds %zu, wanted %p lds %zu\n", w.perh, (int)w.encode, (int)fill,
                       (int)w.conceal, (int)w.chains, (int)w.folded, k ? (void *)k->fn : nullptr, k ? k->lds : (size_t)0, (void *)w.fn, w.lds);
                ++bad;
            }
        }
    }
    // the table: every entry is one of the 30 above, once; none beyond a compute unit's LDS
    for (const FlowKernel &k : FLOW_KERNELS) {
        ++entries;
        int named = 0, same_fn = 0;
        for (const Want &w : WANT) named += w.fn == k.fn;
        for (const FlowKernel &o : FLOW_KERNELS) same_fn += o.fn == k.fn;
        if (!k.fn || named != 1 || same_fn != 1 || k.lds > 160 * 1024 || flow_kernel(k.perh, k.program, k.form) != &k) {
            printf("table entry perh %d program %d form %d: fn %p named %d times, in the table %d times, lds %zu\n", k.perh, k.program, k.form, (void *)k.fn, named, same_fn, k.lds);
            ++bad;
        }
    }
    if (entries != (int)(sizeof WANT / sizeof WANT[0])) { printf("%d table entries\n", entries); ++bad; }
    if (FlowLds<8>::bytes(FF_FILL) != FILL || FlowLds<8>::bytes(FF_PLAIN) != PLAIN || FlowLds<8>::bytes(FF_CHAINS) != MULTI) { printf("layout totals\n"); ++bad; }
    // refusals: code and message
    {
        const char *m_conceal = "launch_flow: the concealing program needs the encode layout, codes and a selector";
        const char *m_chains = "launch_flow: interleaved chains are built for h_dim 1024 only";
        FlowArgs c = args_for(true, false, false);
        bad += refused("conceal on the decode layout", c, 8, false, true, true, m_conceal); ++refusals;
        FlowArgs nc = c; nc.codes_in = nullptr;
        bad += refused("conceal without received codes", nc, 8, true, true, true, m_conceal); ++refusals;
        nc = c; nc.codes = nullptr;
        bad += refused("conceal without codes", nc, 8, true, true, true, m_conceal); ++refusals;
        nc = c; nc.bits = nullptr;
        bad += refused("conceal without a selector", nc, 8, true, true, true, m_conceal); ++refusals;
        for (int perh : {1, 2, 4}) {
            bad += refused("chains at PERH != 8", args_for(false, true, false), perh, true, false, false, m_chains); ++refusals;
            bad += refused("concealing chains at PERH != 8", args_for(true, true, true), perh, true, false, true, m_chains); ++refusals;
        }
        for (int perh : {0, 3, 16, -1}) {
            char want[64];
            snprintf(want, sizeof want, "launch_flow: unsupported blocks per wave %d", perh);
            for (bool enc : {false, true})
                for (bool fill : {false, true}) { bad += refused("unsupported PERH", args_for(false, false, false), perh, enc, fill, false, want); ++refusals; }
        }
    }
    // the capped grid size against the expression written out in both launches before
    for (long long n : {0LL, 1LL, 255LL, 256LL, 257LL, 2048LL * 256, 2048LL * 256 + 1, 1LL << 30}) {
        const int was = (int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
        ++grids;
        if (flow_fill_blocks(n) != was) { printf("grid for n = %lld: %d, was %d\n", n, flow_fill_blocks(n), was); ++bad; }
    }
    for (int h : {16, 64, 112, 128, 256, 512, 1024})
        if (flow_perh(h) != 0 && !flow_kernel(flow_perh(h), FP_ENCODE, FF_PLAIN)) { printf("flow_perh(%d) has no kernel\n", h); ++bad; }
    printf("flow_host_check: %d picks, %d table entries, %d refusals, %d grid sizes, %d failures\n", picks, entries, refusals, grids, bad);
    return bad != 0;
}
