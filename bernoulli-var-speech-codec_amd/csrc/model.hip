// The model: weight upload and re-layout into MFMA fragment order, the workspace layout, the residency census of the persistent
// recurrence, and the bvc_model_* entry points.
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>

#include "bvc_host.h"

using namespace bvc;

namespace {

typedef std::map<std::string, const bvc_tensor *> TensorMap;

template <typename T>
int upload_raw(bvc_model *m, const T *h, int64_t n, const T **dev) {
    void *d = nullptr;
    const size_t bytes = (size_t)n * sizeof(T);
    BVC_HIP_TRY(hipMalloc(&d, bytes ? bytes : 16));
    m->allocs.push_back(d);
    if (bytes) BVC_HIP_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    *dev = static_cast<const T *>(d);
    return BVC_OK;
}
template <typename T>
int upload(bvc_model *m, const std::vector<T> &host, const T **dev) { return upload_raw(m, host.data(), (int64_t)host.size(), dev); }

const bvc_tensor *find(const TensorMap &tm, const std::string &name, int64_t numel) {
    auto it = tm.find(name);
    if (it == tm.end()) { set_error("missing tensor '%s'", name.c_str()); return nullptr; }
    if (it->second->numel != numel || !it->second->h_data) {
        set_error("tensor '%s' has %lld elements, expected %lld", name.c_str(),
                  (long long)it->second->numel, (long long)numel);
        return nullptr;
    }
    return it->second;
}

// Linear weight W[N][K] (row-major) -> MFMA B-operand fragment order [N/16][K/16][lane][4]:
// lane = ((k%16)/4)*16 + n%16 holds W[n][k..k+3]; one (n-tile, k-block) pair is 1 KiB contiguous.
std::vector<float> pack_linear(const float *W, int N, int K) {
    std::vector<float> p((size_t)N * K);
    const int nb = K / 16;
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k)
            p[((((size_t)(n >> 4) * nb + (k >> 4)) * 64 + ((k & 15) >> 2) * 16 + (n & 15)) << 2) + (k & 3)] = W[(size_t)n * K + k];
    return p;
}

// GRU weight W[3H][K] (gates r, z, n stacked, PyTorch order) -> [H/16][K/16][gate][lane][4]: the three gates' fragments of
// one (feature tile, k-block) are 3 KiB contiguous.  With the gates 4-8 MB apart (pack_linear) a wave's three loads per
// k-block hit the same L2 channel; interleaved, the GRU launch is 10 % shorter alone and 24 % in the aggregate of three
// concurrent chains (tools/gru_splitk_bench.hip).
std::vector<float> pack_gru_interleaved(const float *W, int H, int K) {
    std::vector<float> p((size_t)3 * H * K);
    const int nb = K / 16;
    for (int q = 0; q < 3; ++q)
        for (int n = 0; n < H; ++n)
            for (int k = 0; k < K; ++k)
                p[(((((size_t)(n >> 4) * nb + (k >> 4)) * 3 + q) * 64 + ((k & 15) >> 2) * 16 + (n & 15)) << 2) + (k & 3)] =
                    W[((size_t)q * H + n) * K + k];
    return p;
}

int load_linear(bvc_model *m, const TensorMap &tm, const std::string &name, int in, int out, Linear *l) {
    const bvc_tensor *w = find(tm, name + ".weight", (int64_t)in * out);
    if (!w) return BVC_EMISSING;
    const bvc_tensor *b = find(tm, name + ".bias", out);
    if (!b) return BVC_EMISSING;
    l->in = in; l->out = out;
    int rc;
    if ((rc = upload_raw(m, w->h_data, w->numel, &l->w))) return rc;          // natural: batched GEMM
    if ((rc = upload(m, pack_linear(w->h_data, out, in), &l->wp))) return rc;  // packed: recurrent kernels
    return upload_raw(m, b->h_data, b->numel, &l->b);
}

// Conv1d weight W[cout][cin][ks] -> MFMA B fragments [ks][cin/4][ntiles][64]
std::vector<float> pack_conv(const float *W, int cout, int cin, int ks) {
    const int c4 = cin / 4, ntiles = (cout + 15) / 16;
    std::vector<float> p((size_t)ks * c4 * ntiles * 64, 0.0f);
    for (int j = 0; j < ks; ++j)
        for (int cg = 0; cg < c4; ++cg)
            for (int nt = 0; nt < ntiles; ++nt)
                for (int l = 0; l < 64; ++l) {
                    const int co = nt * 16 + (l & 15), ci = cg * 4 + (l >> 4);
                    if (co < cout)
                        p[(((size_t)j * c4 + cg) * ntiles + nt) * 64 + l] = W[((size_t)co * cin + ci) * ks + j];
                }
    return p;
}

// Conv1d weight W[cout][cin][ks] -> [ks][cin/16][ntiles][64][4]: the fragments of pack_conv for four consecutive k-steps side by side
std::vector<float> pack_conv_k4(const float *W, int cout, int cin, int ks) {
    const int g4 = cin / 16, ntiles = (cout + 15) / 16;
    std::vector<float> p((size_t)ks * g4 * ntiles * 64 * 4, 0.0f);
    for (int j = 0; j < ks; ++j)
        for (int q = 0; q < g4; ++q)
            for (int nt = 0; nt < ntiles; ++nt)
                for (int l = 0; l < 64; ++l)
                    for (int u = 0; u < 4; ++u) {
                        const int co = nt * 16 + (l & 15), ci = (q * 4 + u) * 4 + (l >> 4);
                        if (co < cout)
                            p[((((size_t)j * g4 + q) * ntiles + nt) * 64 + l) * 4 + u] = W[((size_t)co * cin + ci) * ks + j];
                    }
    return p;
}

// Conv1d weight W[8][8][ks] -> B fragments [ks+1][2][64] of the two-rows-per-tile form (k_vocoder.hip, amp_pair8_kernel):
// column n = p*8 + co of k-step k holds W[co][ci][k - p] (zero outside the kernel)
std::vector<float> pack_conv_two_rows(const float *W, int ks) {
    std::vector<float> p((size_t)(ks + 1) * 2 * 64, 0.0f);
    for (int k = 0; k <= ks; ++k)
        for (int cg = 0; cg < 2; ++cg)
            for (int l = 0; l < 64; ++l) {
                const int n = l & 15, pr = n >> 3, co = n & 7, ci = cg * 4 + (l >> 4), j = k - pr;
                if (j >= 0 && j < ks) p[((size_t)k * 2 + cg) * 64 + l] = W[((size_t)co * 8 + ci) * ks + j];
            }
    return p;
}

// ConvTranspose1d weight W[cin][cout][2u] -> 2-tap conv with u*cout columns (polyphase form)
std::vector<float> convt_as_conv(const float *W, int cin, int cout, int u) {
    const int k = 2 * u, ncol = u * cout;
    std::vector<float> v((size_t)ncol * cin * 2);
    for (int p = 0; p < u; ++p)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) {
                const size_t n = (size_t)p * cout + co;
                v[(n * cin + ci) * 2 + 0] = W[((size_t)ci * cout + co) * k + p + u];   // tap on in[q-1]
                v[(n * cin + ci) * 2 + 1] = W[((size_t)ci * cout + co) * k + p];       // tap on in[q]
            }
    return v;
}

int make_conv(bvc_model *m, const float *W, const float *bias, int nbias_rep, int cout, int cin, int ks, int dil,
              const float *alpha, const float *beta, ConvLayer *c) {
    c->cin = cin; c->cout = cout; c->ntiles = (cout + 15) / 16; c->ks = ks; c->dil = dil;
    c->act_a = c->act_ib = nullptr;
    c->aa_up = c->aa_down = nullptr;
    int rc;
    std::vector<float> wp = pack_conv(W, cout, cin, ks);
    if ((rc = upload(m, wp, &c->wp))) return rc;
    c->wp2 = nullptr;
    c->wp4 = nullptr;
    if (cin == cout && cin >= 32 && cin % 16 == 0 && alpha && (rc = upload(m, pack_conv_k4(W, cout, cin, ks), &c->wp4))) return rc;
    if (cin == 8 && cout == 8 && (rc = upload(m, pack_conv_two_rows(W, ks), &c->wp2))) return rc;
    std::vector<float> b((size_t)cout);
    const int per = cout / nbias_rep;
    for (int i = 0; i < cout; ++i) b[i] = bias[i % per];
    if ((rc = upload(m, b, &c->bias))) return rc;
    if (alpha) {
        std::vector<float> a(cin), ib(cin);
        for (int i = 0; i < cin; ++i) {
            a[i] = (float)std::exp((double)alpha[i]);                      // torch.exp(alpha)
            const float eb = (float)std::exp((double)beta[i]);
            ib[i] = 1.0f / (eb + 0.000000001f);                            // activations.py:116
        }
        if ((rc = upload(m, a, &c->act_a))) return rc;
        if ((rc = upload(m, ib, &c->act_ib))) return rc;
    }
    return BVC_OK;
}

int build_frontend(bvc_model *m, const TensorMap &tm) {
    const bvc_config &c = m->cfg;
    const int nfft = c.n_fft, nbins = nfft / 2 + 1;
    const double PI = 3.14159265358979323846;
    std::vector<float> win(nfft);
    auto itw = tm.find("hann_window");
    if (itw != tm.end() && itw->second->numel == nfft) {
        memcpy(win.data(), itw->second->h_data, sizeof(float) * nfft);
    } else {
        for (int n = 0; n < nfft; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * n / nfft));
    }
    std::vector<float2> tw1(8 * 64), tw2(64), tws(nbins);
    for (int k = 0; k < 8; ++k)
        for (int l = 0; l < 64; ++l) {
            const double a = -2.0 * PI * (double)(l * k) / 512.0;
            tw1[k * 64 + l] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) {
            const double a = -2.0 * PI * (double)(n * k) / 64.0;
            tw2[k * 8 + n] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    for (int k = 0; k < nbins; ++k) {
        const double a = -2.0 * PI * (double)k / 1024.0;
        tws[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    const bvc_tensor *mb = find(tm, "mel_basis", (int64_t)c.num_mels * nbins);
    if (!mb) return BVC_EMISSING;
    std::vector<int> st(c.num_mels), ln(c.num_mels), off(c.num_mels);
    std::vector<float> w;
    int kmax = 1;
    for (int j = 0; j < c.num_mels; ++j) {
        const float *row = mb->h_data + (size_t)j * nbins;
        int lo = -1, hi = -1;
        for (int k = 0; k < nbins; ++k)
            if (row[k] != 0.0f) { if (lo < 0) lo = k; hi = k; }
        if (lo < 0) { lo = 0; hi = -1; }
        st[j] = lo; ln[j] = hi - lo + 1; off[j] = (int)w.size();
        for (int k = lo; k <= hi; ++k) w.push_back(row[k]);
        if (hi + 1 > kmax) kmax = hi + 1;
    }
    FrontendTables &t = m->fe;
    int rc;
    if ((rc = upload(m, win, &t.window))) return rc;
    if ((rc = upload(m, tw1, &t.tw1))) return rc;
    if ((rc = upload(m, tw2, &t.tw2))) return rc;
    if ((rc = upload(m, tws, &t.tws))) return rc;
    if ((rc = upload(m, st, &t.mel_start))) return rc;
    if ((rc = upload(m, ln, &t.mel_len))) return rc;
    if ((rc = upload(m, off, &t.mel_off))) return rc;
    if ((rc = upload(m, w, &t.mel_w))) return rc;
    t.num_mels = c.num_mels;
    t.kmax = kmax;
    return BVC_OK;
}

int build_bvrnn(bvc_model *m, const TensorMap &tm) {
    const int X = m->cfg.num_mels, H = m->cfg.h_dim, Z = m->cfg.z_dim;
    int rc;
    const bvc_tensor *t;
    if (!(t = find(tm, "mean_mel", X))) return BVC_EMISSING;
    if ((rc = upload_raw(m, t->h_data, X, &m->mean_mel))) return rc;
    if (!(t = find(tm, "std_mel", X))) return BVC_EMISSING;
    if ((rc = upload_raw(m, t->h_data, X, &m->std_mel))) return rc;
    const int px_in[3] = {X, H, H}, pz_in[3] = {Z, H, H}, en_in[3] = {2 * H, H, H}, en_out[3] = {H, H, Z};
    const int de_in[4] = {2 * H, H, H, H}, de_out[4] = {H, H, H, X};
    for (int i = 0; i < 3; ++i) {
        const std::string idx = std::to_string(2 * i);
        if ((rc = load_linear(m, tm, "phi_x." + idx, px_in[i], H, &m->phi_x[i]))) return rc;
        if ((rc = load_linear(m, tm, "phi_z." + idx, pz_in[i], H, &m->phi_z[i]))) return rc;
        if ((rc = load_linear(m, tm, "enc." + idx, en_in[i], en_out[i], &m->enc[i]))) return rc;
    }
    for (int i = 0; i < 4; ++i)
        if ((rc = load_linear(m, tm, "dec." + std::to_string(2 * i), de_in[i], de_out[i], &m->dec[i]))) return rc;
    if (tm.count("prior.0.weight")) {        // training-time prior net (bvrnn.py:68-73): needed by bvc_bvrnn_forward only
        const int pr_out[3] = {H, H, Z};
        for (int i = 0; i < 3; ++i)
            if ((rc = load_linear(m, tm, "prior." + std::to_string(2 * i), H, pr_out[i], &m->prior[i]))) return rc;
        m->has_prior = true;
    }
    {   // px0_dec3: W = phi_x.0.W diag(1/std) dec.6.W  (H x H),  b = phi_x.0.W ((dec.6.b - mean) / std) + phi_x.0.b, in float64
        const float *wp0 = tm.at("phi_x.0.weight")->h_data, *bp0 = tm.at("phi_x.0.bias")->h_data;      // [H][X], [H]
        const float *wd6 = tm.at("dec.6.weight")->h_data, *bd6 = tm.at("dec.6.bias")->h_data;          // [X][H], [X]
        const float *mean = tm.at("mean_mel")->h_data, *stdv = tm.at("std_mel")->h_data;
        std::vector<float> wc((size_t)H * H), bc((size_t)H);
        std::vector<double> row((size_t)H);
        for (int n = 0; n < H; ++n) {
            std::fill(row.begin(), row.end(), 0.0);
            double b = (double)bp0[n];
            for (int j = 0; j < X; ++j) {
                const double f = (double)wp0[(size_t)n * X + j] / (double)stdv[j];
                b += f * ((double)bd6[j] - (double)mean[j]);
                const float *wr = wd6 + (size_t)j * H;
                for (int k = 0; k < H; ++k) row[k] += f * (double)wr[k];
            }
            for (int k = 0; k < H; ++k) wc[(size_t)n * H + k] = (float)row[k];
            bc[n] = (float)b;
        }
        if (getenv("BVC_DECODE_FOLD") && getenv("BVC_DECODE_FOLD")[0] == '0') m->decode_fold = 0;     // A/B runs (tools/flow_variants.py)
        if (getenv("BVC_ENCODE_FOLD") && getenv("BVC_ENCODE_FOLD")[0] == '0') m->encode_fold = 0;
        m->px0_dec3.in = H; m->px0_dec3.out = H;
        m->px0_dec3.w = nullptr;                                   // (only the recurrent kernels use it)
        if ((rc = upload(m, pack_linear(wc.data(), H, H), &m->px0_dec3.wp))) return rc;
        if ((rc = upload(m, bc, &m->px0_dec3.b))) return rc;
    }
    if (!(t = find(tm, "rnn.weight_ih_l0", (int64_t)3 * H * 2 * H))) return BVC_EMISSING;
    if ((rc = upload(m, pack_linear(t->h_data, 3 * H, 2 * H), &m->w_ih))) return rc;
    if ((rc = upload(m, pack_gru_interleaved(t->h_data, H, 2 * H), &m->w_ih_il))) return rc;
    if ((rc = upload_raw(m, t->h_data, t->numel, &m->w_ih_nat))) return rc;
    if (!(t = find(tm, "rnn.weight_hh_l0", (int64_t)3 * H * H))) return BVC_EMISSING;
    if ((rc = upload(m, pack_linear(t->h_data, 3 * H, H), &m->w_hh))) return rc;
    if ((rc = upload(m, pack_gru_interleaved(t->h_data, H, H), &m->w_hh_il))) return rc;
    if (!(t = find(tm, "rnn.bias_ih_l0", 3 * H))) return BVC_EMISSING;
    if ((rc = upload_raw(m, t->h_data, t->numel, &m->b_ih))) return rc;
    if (!(t = find(tm, "rnn.bias_hh_l0", 3 * H))) return BVC_EMISSING;
    if ((rc = upload_raw(m, t->h_data, t->numel, &m->b_hh))) return rc;
    return BVC_OK;
}

// where the generator wraps its SnakeBeta in Activation1d: optional tensors "layers_antialias" (n_up values, non-zero = the stage's
// AMP blocks) and "antialias_post" (one value); bvc_config keeps its layout.  A flagged activation `name` has the reference's keys
// name.act.alpha / name.act.beta / name.upsample.filter / name.downsample.lowpass.filter (alias_free_torch/act.py:18-20), a plain
// one name.alpha / name.beta: a checkpoint of the other layout is missing tensors either way.
int find_activation(bvc_model *m, const TensorMap &tm, const std::string &name, int ch, bool filtered, const bvc_tensor **alpha,
                    const bvc_tensor **beta, const float **up, const float **down) {
    const std::string mid = filtered ? ".act" : "";
    if (!(*alpha = find(tm, name + mid + ".alpha", ch))) return BVC_EMISSING;
    if (!(*beta = find(tm, name + mid + ".beta", ch))) return BVC_EMISSING;
    *up = *down = nullptr;
    if (!filtered) return BVC_OK;
    const bvc_tensor *fu, *fd;
    if (!(fu = find(tm, name + ".upsample.filter", 12))) return BVC_EMISSING;
    if (!(fd = find(tm, name + ".downsample.lowpass.filter", 12))) return BVC_EMISSING;
    int rc;
    if ((rc = upload_raw(m, fu->h_data, 12, up))) return rc;
    return upload_raw(m, fd->h_data, 12, down);
}

int build_vocoder(bvc_model *m, const TensorMap &tm) {
    const bvc_config &c = m->cfg;
    int rc;
    const bvc_tensor *w, *b;
    std::vector<bool> stage_aa(c.n_up, false);
    bool post_aa = false;
    if (tm.count("layers_antialias")) {
        const bvc_tensor *t = find(tm, "layers_antialias", c.n_up);
        if (!t) return BVC_EMISSING;
        for (int i = 0; i < c.n_up; ++i) stage_aa[i] = t->h_data[i] != 0.0f;
    }
    if (tm.count("antialias_post")) {
        const bvc_tensor *t = find(tm, "antialias_post", 1);
        if (!t) return BVC_EMISSING;
        post_aa = t->h_data[0] != 0.0f;
    }
    // symmetric paddings: optional tensors "layers_sym" (n_up values), "pre_sym" and "post_sym" (one value each); no keys of their own
    m->stage_sym.assign(c.n_up, false);
    if (tm.count("layers_sym")) {
        const bvc_tensor *t = find(tm, "layers_sym", c.n_up);
        if (!t) return BVC_EMISSING;
        for (int i = 0; i < c.n_up; ++i) m->stage_sym[i] = t->h_data[i] != 0.0f;
    }
    for (const char *key : {"pre_sym", "post_sym"})
        if (tm.count(key)) {
            const bvc_tensor *t = find(tm, key, 1);
            if (!t) return BVC_EMISSING;
            (key[1] == 'r' ? m->pre_sym : m->post_sym) = t->h_data[0] != 0.0f;
        }
    m->symmetric = m->pre_sym || m->post_sym;
    bool stages_sym = false;
    for (int i = 0; i < c.n_up; ++i) {
        stages_sym = stages_sym || m->stage_sym[i];
        if (m->stage_sym[i] && stage_aa[i]) {
            set_error("stage %d is symmetric and anti-aliased: filtered stages are implemented as causal stages only", i);
            return BVC_EINVAL;
        }
    }
    m->symmetric = m->symmetric || stages_sym;
    if (m->post_sym && post_aa) { set_error("post_sym with antialias_post: a filtered activation_post is implemented in front of a causal conv_post only"); return BVC_EINVAL; }
    if (stages_sym) {
        for (int j = 0; j < c.n_resk; ++j)
            if (c.res_kernels[j] % 2 == 0) { set_error("a symmetric stage needs odd resblock kernel sizes (got %d)", c.res_kernels[j]); return BVC_EINVAL; }
        for (int i = 0; i < c.n_up; ++i)
            if (m->stage_sym[i] && c.up_rates[i] % 2) { set_error("a symmetric upsampler needs an even rate (got %d)", c.up_rates[i]); return BVC_EINVAL; }
        if (!m->fused_amp) { set_error("symmetric stages run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)"); return BVC_EINVAL; }
    }
    // wide stages (128 / 256 channels, generators of 256 / 512 initial channels) exist as causal, unfiltered, fused pairs only
    for (int i = 0; i < c.n_up; ++i) {
        const int C = c.upsample_initial_channel >> (i + 1);
        if (C < 128) continue;
        if (m->stage_sym[i]) { set_error("stage %d has %d channels: symmetric layers (layers_sym) are implemented on stages of 64 channels at most", i, C); return BVC_EINVAL; }
        if (stage_aa[i]) { set_error("stage %d has %d channels: anti-aliased activations (layers_antialias) are implemented on stages of 64 channels at most", i, C); return BVC_EINVAL; }
        if (!m->fused_amp) { set_error("stage %d has %d channels: wide stages run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)", i, C); return BVC_EINVAL; }
    }
    m->antialiased = post_aa;
    for (int i = 0; i < c.n_up; ++i) m->antialiased = m->antialiased || stage_aa[i];
    m->noncausal = m->antialiased || m->symmetric;
    if (m->antialiased && !m->fused_amp) { set_error("anti-aliased activations run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)"); return BVC_EINVAL; }
    const int c0 = c.upsample_initial_channel;
    if (!(w = find(tm, "conv_pre.weight", (int64_t)c0 * c.num_mels * 7))) return BVC_EMISSING;
    if (!(b = find(tm, "conv_pre.bias", c0))) return BVC_EMISSING;
    if ((rc = make_conv(m, w->h_data, b->h_data, 1, c0, c.num_mels, 7, 1, nullptr, nullptr, &m->conv_pre))) return rc;
    int ch = c0;
    m->ups.resize(c.n_up);
    m->amp.resize(c.n_up);
    m->stage_ch.resize(c.n_up);
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i], cin = ch, cout = ch / 2;
        const std::string nm = "ups." + std::to_string(i) + ".1";
        if (!(w = find(tm, nm + ".weight", (int64_t)cin * cout * 2 * u))) return BVC_EMISSING;
        if (!(b = find(tm, nm + ".bias", cout))) return BVC_EMISSING;
        std::vector<float> wv = convt_as_conv(w->h_data, cin, cout, u);
        if ((rc = make_conv(m, wv.data(), b->h_data, u, u * cout, cin, 2, 1, nullptr, nullptr, &m->ups[i]))) return rc;
        ch = cout;
        m->stage_ch[i] = ch;
        m->amp[i].resize(c.n_resk);
        for (int j = 0; j < c.n_resk; ++j) {
            const int ks = c.res_kernels[j];
            const std::string pre = "resblocks." + std::to_string(i * c.n_resk + j);
            m->amp[i][j].resize(3);
            for (int d = 0; d < 3; ++d) {
                const bvc_tensor *a1, *b1, *a2, *b2, *w1, *bb1, *w2, *bb2;
                const std::string ds = std::to_string(d);
                const float *up1, *down1, *up2, *down2;
                if ((rc = find_activation(m, tm, pre + ".activations." + std::to_string(2 * d), ch, stage_aa[i], &a1, &b1, &up1, &down1))) return rc;
                if ((rc = find_activation(m, tm, pre + ".activations." + std::to_string(2 * d + 1), ch, stage_aa[i], &a2, &b2, &up2, &down2))) return rc;
                if (!(w1 = find(tm, pre + ".convs1." + ds + ".weight", (int64_t)ch * ch * ks))) return BVC_EMISSING;
                if (!(bb1 = find(tm, pre + ".convs1." + ds + ".bias", ch))) return BVC_EMISSING;
                if (!(w2 = find(tm, pre + ".convs2." + ds + ".weight", (int64_t)ch * ch * ks))) return BVC_EMISSING;
                if (!(bb2 = find(tm, pre + ".convs2." + ds + ".bias", ch))) return BVC_EMISSING;
                AmpPair &ap = m->amp[i][j][d];
                if ((rc = make_conv(m, w1->h_data, bb1->h_data, 1, ch, ch, ks, c.res_dilations[j][d], a1->h_data,
                                    b1->h_data, &ap.c1))) return rc;
                if ((rc = make_conv(m, w2->h_data, bb2->h_data, 1, ch, ch, ks, 1, a2->h_data, b2->h_data, &ap.c2)))
                    return rc;
                ap.c1.aa_up = up1; ap.c1.aa_down = down1; ap.c2.aa_up = up2; ap.c2.aa_down = down2;
            }
        }
    }
    m->post_c = ch;
    const bvc_tensor *pa, *pb;
    if ((rc = find_activation(m, tm, "activation_post", ch, post_aa, &pa, &pb, &m->post_up, &m->post_down))) return rc;
    std::vector<float> a(ch), ib(ch);
    for (int i = 0; i < ch; ++i) {
        a[i] = (float)std::exp((double)pa->h_data[i]);
        ib[i] = 1.0f / ((float)std::exp((double)pb->h_data[i]) + 0.000000001f);
    }
    if ((rc = upload(m, a, &m->post_a))) return rc;
    if ((rc = upload(m, ib, &m->post_ib))) return rc;
    if (!(w = find(tm, "conv_post.weight", (int64_t)ch * 7))) return BVC_EMISSING;
    if (!(b = find(tm, "conv_post.bias", 1))) return BVC_EMISSING;
    if ((rc = upload_raw(m, w->h_data, w->numel, &m->post_w))) return rc;
    if ((rc = upload_raw(m, b->h_data, 1, &m->post_b))) return rc;
    return BVC_OK;
}

int check_config(const bvc_config *c) {
    if (!c) { set_error("null config"); return BVC_EINVAL; }
    if (c->n_fft != 1024 || c->hop != 256) { set_error("front-end kernel needs n_fft=1024, hop=256"); return BVC_EINVAL; }
    if (c->pad_left < 0 || c->pad_left > c->n_fft - c->hop) { set_error("pad_left out of range"); return BVC_EINVAL; }
    if (c->num_mels % 16 || c->h_dim % 16 || c->z_dim % 16 || c->num_mels > 128 || c->num_mels < 16 || c->h_dim < 16 || c->z_dim < 16) {
        set_error("num_mels/h_dim/z_dim must be positive multiples of 16 (num_mels <= 128)"); return BVC_EINVAL; }
    if (c->n_up < 1 || c->n_up > 8 || c->n_resk < 1 || c->n_resk > 4) { set_error("bad n_up / n_resk"); return BVC_EINVAL; }
    int ch = c->upsample_initial_channel;
    if (ch != 512 && ch != 256 && ch != 128 && ch != 64 && ch != 32 && ch != 16) { set_error("unsupported upsample_initial_channel %d (16, 32, 64, 128, 256 or 512)", ch); return BVC_EINVAL; }
    for (int i = 0; i < c->n_up; ++i) {
        if (c->up_kernels[i] != 2 * c->up_rates[i]) { set_error("upsample kernel must be 2*rate"); return BVC_EINVAL; }
        ch /= 2;
        if (ch < 8) { set_error("too many upsampling stages for %d initial channels", c->upsample_initial_channel); return BVC_EINVAL; }
    }
    if (ch != 8 && ch != 16 && ch != 32) { set_error("final channel count must be 8, 16 or 32 (got %d)", ch); return BVC_EINVAL; }
    if (c->num_mels != 80) { set_error("conv_pre kernel is built for num_mels=80"); return BVC_EINVAL; }
    return BVC_OK;
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

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

// Takes the sticky status word of the persistent kernels (no synchronisation): a code that is there is cleared, and the residency
// census runs again before the next persistent launch
unsigned take_status(const bvc_model *m) {
    const unsigned v = m->h_status ? *m->h_status : 0u;
    if (v) { *m->h_status = 0u; m->census_due = true; }
    return v;
}

}  // namespace

namespace bvc {

const char *const NOT_CAUSAL = "the model has anti-aliased activations: a filtered AMP block looks 30 rows ahead, so the generator is not causal";

const char *const NOT_CAUSAL_SYM = "the model has symmetric layers: a symmetric layer reads as many rows ahead as behind, so the generator is not causal";
const char *not_causal(const bvc_model *m) { return m->antialiased ? NOT_CAUSAL : NOT_CAUSAL_SYM; }

int64_t stage_len(const bvc_model *m, int64_t T, int stage) {    // length after upsampler `stage`: a symmetric one drops the u-row tail
    int64_t L = T;
    for (int i = 0; i <= stage; ++i) L = ((size_t)i < m->stage_sym.size() && m->stage_sym[i] ? L : L + 1) * m->cfg.up_rates[i];
    return L;
}

void carve(const bvc_model *m, int B, int64_t T, char *base, Workspace *w) {
    const bvc_config &c = m->cfg;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float *p = reinterpret_cast<float *>(base + off);
        off += align_up(nfloats * sizeof(float));
        return p;
    };
    const size_t BT = (size_t)B * (size_t)T;
    const int H = c.h_dim;
    const int vmax = H > c.num_mels ? H : c.num_mels;
    const size_t mt16 = (size_t)((B + 15) / 16) * 16;          // fragment-packed matrices hold whole 16-row tiles
    // buffers referenced by the captured step graphs come first: their offsets depend on B only, so a
    // graph captured for (B, workspace) stays valid for every T
    for (int i = 0; i < 16; ++i) w->step[i] = take(mt16 * vmax);
    w->hbuf = take(2 * mt16 * H);
    w->part_i = take(mt16 * 3 * H);
    w->part_h = take(mt16 * 3 * H);
    w->part_d = take(mt16 * H);
    w->desc = reinterpret_cast<CallDesc *>(take(64));
    {
        int dmax = H > c.num_mels ? H : c.num_mels;
        if (c.z_dim > dmax) dmax = c.z_dim;
        w->flow_slot = mt16 * (size_t)dmax;
        w->flow = take((size_t)FB_COUNT * 2 * w->flow_slot);
        w->flow_args = reinterpret_cast<FlowArgs *>(take((sizeof(FlowArgs) + 3) / 4));
    }
    w->yn = take(BT * c.num_mels);
    w->pxA = take(mt16 * (size_t)T * H);                       // final phi_x / phi_z: frame-packed
    w->pxB = take(mt16 * (size_t)T * H);                       // intermediates of the batched MLPs: frame-major rows
    w->pxC = take(mt16 * (size_t)T * H);
    w->mel = take(BT * c.num_mels);
    w->bits = take(BT);
    w->part_dec0 = take(BT * H);
    w->part_gru = take(BT * 3 * H);
    size_t maxel = 0;
    for (int i = 0; i < c.n_up; ++i) {
        int64_t Lc = T;                                         // the causal lengths: upper bounds of a symmetric generator's, whose
        for (int k = 0; k <= i; ++k) Lc = (Lc + 1) * c.up_rates[k];     // stages work on views of the causal upsampler results
        const size_t e = (size_t)Lc * m->stage_ch[i];
        if (e > maxel) maxel = e;
    }
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
    const unsigned v = m ? take_status(m) : 0u;
    if (!v) return BVC_OK;
    set_error("a persistent recurrence kernel of an earlier call gave up waiting (frame %u, layer %u): the results of that call "
              "are invalid.  All its workgroups must be resident together - is another process using this GPU?",
              (v & 0x7FFFFFFFu) >> 4, (v & 15u));
    return BVC_ETIMEOUT;
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
    if (getenv("BVC_FLOW_CENSUS_OVERSUBSCRIBE")) slots += 1;             // tests: a grid the device cannot hold
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
    if (!m->flow_resident && !getenv("BVC_QUIET"))
        fprintf(stderr, "bvcodec: residency census: %u of %d recurrence workgroups became co-resident (%u gave up) - this model stays on the "
                        "launch-per-layer schedule (get_option \"flow_resident\" = 0).  Is another process using this GPU?\n", h[0] - h[1], grid, h[1]);
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int bvc_model_create(const bvc_config *cfg, const bvc_tensor *tensors, int32_t n_tensors, bvc_model **out) {
    if (!out) { set_error("null out pointer"); return BVC_EINVAL; }
    *out = nullptr;
    int rc = check_config(cfg);
    if (rc) return rc;
    if (!tensors || n_tensors <= 0) { set_error("no tensors given"); return BVC_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: the gfx950 kernels cannot run (there is no CPU fallback)");
        return BVC_ENODEVICE;
    }
    TensorMap tm;
    for (int i = 0; i < n_tensors; ++i)
        if (tensors[i].name) tm[tensors[i].name] = &tensors[i];
    std::unique_ptr<bvc_model> m(new bvc_model());
    m->cfg = *cfg;
    if ((rc = conv_kernels_init())) return rc;
    if ((rc = skinny_kernels_init())) return rc;
    {
        const char *ng = getenv("BVC_NO_GRAPH");
        m->use_graph = !(ng && ng[0] == '1');
        const char *sb = getenv("BVC_SIDE_BRANCH");
        m->side_branch = (sb && sb[0] == '1');
        const char *mw = getenv("BVC_MTW");
        if (mw && (mw[0] == '2' || mw[0] == '4')) m->mtw = mw[0] - '0';
        const char *ua = getenv("BVC_UNFUSED_AMP");
        m->fused_amp = !(ua && ua[0] == '1');
        m->amp_kernels = amp_kernels_default();
        const char *np = getenv("BVC_NO_PRECOMP");
        m->precomp_pz = !(np && np[0] == '1') && !m->side_branch;
    }
    if ((rc = build_frontend(m.get(), tm))) return rc;
    if ((rc = build_bvrnn(m.get(), tm))) return rc;
    {
        const char *rr = getenv("BVC_RECURRENCE");
        m->recurrence = (rr && strcmp(rr, "layers") == 0) ? RS_LAYERS : (rr && strcmp(rr, "persistent") == 0) ? RS_PERSISTENT : RS_AUTO;
    }
    if ((rc = build_flow(m.get()))) return rc;
    if ((rc = build_vocoder(m.get(), tm))) return rc;
    BVC_HIP_TRY(hipDeviceSynchronize());
    *out = m.release();
    return BVC_OK;
}

void bvc_model_destroy(bvc_model *m) { delete m; }

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
    const unsigned v = take_status(m);
    if (code) *code = v;
    if (v) {
        set_error("a persistent recurrence kernel gave up waiting (frame %u, layer %u): its results are invalid",
                  (v & 0x7FFFFFFFu) >> 4, (v & 15u));
        return BVC_ETIMEOUT;
    }
    return BVC_OK;
}

int bvc_model_poll_status(const bvc_model *m, uint32_t *code) {
    if (!m) { set_error("null model"); return BVC_EINVAL; }
    const unsigned v = take_status(m);
    if (code) *code = v;
    if (v) {
        set_error("a persistent recurrence kernel gave up waiting (frame %u, layer %u): the results of the call that has just been "
                  "synchronised are invalid.  All its workgroups must be resident together - is another process using this GPU?",
                  (v & 0x7FFFFFFFu) >> 4, (v & 15u));
        return BVC_ETIMEOUT;
    }
    return BVC_OK;
}

}  // extern "C"
