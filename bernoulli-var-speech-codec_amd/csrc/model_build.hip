// Model creation: the configuration check, the reading of the checkpoint (one tensor reader, TensorReader), the three builders that map
// it to device memory (what they upload is computed by weight_pack.h), the generator's layout check, the environment switches of the
// model (model_switches) and bvc_model_create / bvc_model_destroy.  What every call runs is in model.hip.
#include <map>
#include <memory>

#include "bvc_host.h"
#include "weight_pack.h"

using namespace bvc;

namespace {

typedef std::map<std::string, const bvc_tensor *> TensorMap;

// n elements of host memory into an allocation of the model's own; the device pointer may have another element type (float2 tables
// are built as interleaved floats)
template <typename T, typename D>
int upload_raw(bvc_model *m, const T *h, int64_t n, const D **dev) {
    void *d = nullptr;
    const size_t bytes = (size_t)n * sizeof(T);
    BVC_HIP_TRY(hipMalloc(&d, bytes ? bytes : 16));
    m->allocs.push_back(d);
    if (bytes) BVC_HIP_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    *dev = static_cast<const D *>(d);
    return BVC_OK;
}
template <typename T, typename D>
int upload(bvc_model *m, const std::vector<T> &host, const D **dev) { return upload_raw(m, host.data(), (int64_t)host.size(), dev); }

// a SnakeBeta as the checkpoint has it: alpha / beta in host memory, the two filters of an anti-aliased one on the device
struct Activation { const float *alpha = nullptr, *beta = nullptr, *up = nullptr, *down = nullptr; };

int make_conv(bvc_model *m, const float *W, const float *bias, int nbias_rep, int cout, int cin, int ks, int dil, const Activation *act,
              ConvLayer *c) {
    c->cin = cin; c->cout = cout; c->ntiles = (cout + 15) / 16; c->ks = ks; c->dil = dil;
    c->act_a = c->act_ib = nullptr;
    c->aa_up = act ? act->up : nullptr;
    c->aa_down = act ? act->down : nullptr;
    int rc;
    if ((rc = upload(m, pack_conv(W, cout, cin, ks), &c->wp))) return rc;
    c->wp2 = nullptr;
    c->wp4 = nullptr;
    if (cin == cout && cin >= 32 && cin % 16 == 0 && act && (rc = upload(m, pack_conv_k4(W, cout, cin, ks), &c->wp4))) return rc;
    if (cin == 8 && cout == 8 && (rc = upload(m, pack_conv_two_rows(W, ks), &c->wp2))) return rc;
    std::vector<float> b((size_t)cout);
    const int per = cout / nbias_rep;
    for (int i = 0; i < cout; ++i) b[i] = bias[i % per];
    if ((rc = upload(m, b, &c->bias))) return rc;
    if (act) {
        std::vector<float> a, ib;
        snake_params(act->alpha, act->beta, cin, &a, &ib);
        if ((rc = upload(m, a, &c->act_a))) return rc;
        if ((rc = upload(m, ib, &c->act_ib))) return rc;
    }
    return BVC_OK;
}

// Reads the checkpoint into a model.  Every member returns a BVC_* code with the error text set: a tensor that is missing or has
// another element count is BVC_EMISSING, raised where the tensor is read.
struct TensorReader {
    bvc_model *m;
    const TensorMap &tm;

    bool has(const std::string &name) const { return tm.count(name) != 0; }
    const bvc_tensor *find(const std::string &name, int64_t numel) const {
        auto it = tm.find(name);
        if (it == tm.end()) { set_error("missing tensor '%s'", name.c_str()); return nullptr; }
        if (it->second->numel != numel || !it->second->h_data) {
            set_error("tensor '%s' has %lld elements, expected %lld", name.c_str(), (long long)it->second->numel, (long long)numel);
            return nullptr;
        }
        return it->second;
    }
    // a tensor as it is; host: where its elements are in host memory (for what is derived from them)
    int vec(const std::string &name, int64_t numel, const float **dev, const float **host = nullptr) const {
        const bvc_tensor *t = find(name, numel);
        if (!t) return BVC_EMISSING;
        if (host) *host = t->h_data;
        return upload_raw(m, t->h_data, numel, dev);
    }
    int linear(const std::string &name, int in, int out, Linear *l) const {
        const bvc_tensor *w = find(name + ".weight", (int64_t)in * out);
        if (!w) return BVC_EMISSING;
        const bvc_tensor *b = find(name + ".bias", out);
        if (!b) return BVC_EMISSING;
        l->in = in; l->out = out;
        int rc;
        if ((rc = upload_raw(m, w->h_data, w->numel, &l->w))) return rc;          // natural: batched GEMM
        if ((rc = upload(m, pack_linear(w->h_data, out, in), &l->wp))) return rc;  // packed: recurrent kernels
        return upload_raw(m, b->h_data, b->numel, &l->b);
    }
    // name.weight [cout][cin][ks] and name.bias [cout] as a ConvLayer behind the activation `act` (or none).  up > 1: the tensors are a
    // ConvTranspose1d's, weight [cin][cout / up][2 up] and bias [cout / up]; the layer is its polyphase form, ks = 2
    int conv(const std::string &name, int cout, int cin, int ks, int dil, const Activation *act, ConvLayer *c, int up = 1) const {
        const bvc_tensor *w = find(name + ".weight", (int64_t)cout * cin * ks);
        if (!w) return BVC_EMISSING;
        const bvc_tensor *b = find(name + ".bias", cout / up);
        if (!b) return BVC_EMISSING;
        if (up == 1) return make_conv(m, w->h_data, b->h_data, 1, cout, cin, ks, dil, act, c);
        return make_conv(m, convt_as_conv(w->h_data, cin, cout / up, up).data(), b->h_data, up, cout, cin, ks, dil, act, c);
    }
    // Where the generator wraps its SnakeBeta in Activation1d: optional tensors "layers_antialias" (n_up values, non-zero = the stage's
    // AMP blocks) and "antialias_post" (one value); bvc_config keeps its layout.  A flagged activation `name` has the reference's keys
    // name.act.alpha / name.act.beta / name.upsample.filter / name.downsample.lowpass.filter (alias_free_torch/act.py:18-20), a plain
    // one name.alpha / name.beta: a checkpoint of the other layout is missing tensors either way.
    int activation(const std::string &name, int ch, bool filtered, Activation *a) const {
        const std::string mid = filtered ? ".act" : "";
        const bvc_tensor *t;
        if (!(t = find(name + mid + ".alpha", ch))) return BVC_EMISSING;
        a->alpha = t->h_data;
        if (!(t = find(name + mid + ".beta", ch))) return BVC_EMISSING;
        a->beta = t->h_data;
        a->up = a->down = nullptr;
        if (!filtered) return BVC_OK;
        const bvc_tensor *fu, *fd;
        if (!(fu = find(name + ".upsample.filter", 12))) return BVC_EMISSING;
        if (!(fd = find(name + ".downsample.lowpass.filter", 12))) return BVC_EMISSING;
        int rc;
        if ((rc = upload_raw(m, fu->h_data, 12, &a->up))) return rc;
        return upload_raw(m, fd->h_data, 12, &a->down);
    }
    // an optional tensor of n flags (non-zero = set); out keeps its values where the checkpoint has none
    int flags(const char *name, int n, bool *out) const {
        if (!has(name)) return BVC_OK;
        const bvc_tensor *t = find(name, n);
        if (!t) return BVC_EMISSING;
        for (int i = 0; i < n; ++i) out[i] = t->h_data[i] != 0.0f;
        return BVC_OK;
    }
};

int build_frontend(const TensorReader &r) {
    bvc_model *m = r.m;
    const bvc_config &c = m->cfg;
    const int nfft = c.n_fft, nbins = nfft / 2 + 1;
    auto itw = r.tm.find("hann_window");
    const bool own_window = itw != r.tm.end() && itw->second->numel == nfft;
    const std::vector<float> win = own_window ? std::vector<float>(itw->second->h_data, itw->second->h_data + nfft) : hann_window(nfft);
    const Twiddles tw = fft_twiddles(nbins);
    const bvc_tensor *mb = r.find("mel_basis", (int64_t)c.num_mels * nbins);
    if (!mb) return BVC_EMISSING;
    const MelRows mel = compact_mel_bank(mb->h_data, c.num_mels, nbins);
    FrontendTables &t = m->fe;
    int rc;
    if ((rc = upload(m, win, &t.window))) return rc;
    if ((rc = upload(m, tw.tw1, &t.tw1))) return rc;
    if ((rc = upload(m, tw.tw2, &t.tw2))) return rc;
    if ((rc = upload(m, tw.tws, &t.tws))) return rc;
    if ((rc = upload(m, mel.start, &t.mel_start))) return rc;
    if ((rc = upload(m, mel.len, &t.mel_len))) return rc;
    if ((rc = upload(m, mel.off, &t.mel_off))) return rc;
    if ((rc = upload(m, mel.w, &t.mel_w))) return rc;
    t.num_mels = c.num_mels;
    t.kmax = mel.kmax;
    return BVC_OK;
}

int build_bvrnn(const TensorReader &r) {
    bvc_model *m = r.m;
    const int X = m->cfg.num_mels, H = m->cfg.h_dim, Z = m->cfg.z_dim;
    int rc;
    const float *mean, *stdv;
    if ((rc = r.vec("mean_mel", X, &m->mean_mel, &mean))) return rc;
    if ((rc = r.vec("std_mel", X, &m->std_mel, &stdv))) return rc;
    const int px_in[3] = {X, H, H}, pz_in[3] = {Z, H, H}, en_in[3] = {2 * H, H, H}, en_out[3] = {H, H, Z};
    const int de_in[4] = {2 * H, H, H, H}, de_out[4] = {H, H, H, X};
    for (int i = 0; i < 3; ++i) {
        const std::string idx = std::to_string(2 * i);
        if ((rc = r.linear("phi_x." + idx, px_in[i], H, &m->phi_x[i]))) return rc;
        if ((rc = r.linear("phi_z." + idx, pz_in[i], H, &m->phi_z[i]))) return rc;
        if ((rc = r.linear("enc." + idx, en_in[i], en_out[i], &m->enc[i]))) return rc;
    }
    for (int i = 0; i < 4; ++i)
        if ((rc = r.linear("dec." + std::to_string(2 * i), de_in[i], de_out[i], &m->dec[i]))) return rc;
    if (r.has("prior.0.weight")) {        // training-time prior net (bvrnn.py:68-73): needed by bvc_bvrnn_forward only
        const int pr_out[3] = {H, H, Z};
        for (int i = 0; i < 3; ++i)
            if ((rc = r.linear("prior." + std::to_string(2 * i), H, pr_out[i], &m->prior[i]))) return rc;
        m->has_prior = true;
    }
    {   // the folded hop px0_dec3 (only the recurrent kernels use it: no natural copy)
        const FoldedLinear f = fold_px0_dec3(r.tm.at("phi_x.0.weight")->h_data, r.tm.at("phi_x.0.bias")->h_data, r.tm.at("dec.6.weight")->h_data,
                                             r.tm.at("dec.6.bias")->h_data, mean, stdv, H, X);
        m->px0_dec3.in = H; m->px0_dec3.out = H;
        m->px0_dec3.w = nullptr;
        if ((rc = upload(m, pack_linear(f.w.data(), H, H), &m->px0_dec3.wp))) return rc;
        if ((rc = upload(m, f.b, &m->px0_dec3.b))) return rc;
    }
    const bvc_tensor *t;
    if (!(t = r.find("rnn.weight_ih_l0", (int64_t)3 * H * 2 * H))) return BVC_EMISSING;
    if ((rc = upload(m, pack_linear(t->h_data, 3 * H, 2 * H), &m->w_ih))) return rc;
    if ((rc = upload(m, pack_gru_interleaved(t->h_data, H, 2 * H), &m->w_ih_il))) return rc;
    if ((rc = upload_raw(m, t->h_data, t->numel, &m->w_ih_nat))) return rc;
    if (!(t = r.find("rnn.weight_hh_l0", (int64_t)3 * H * H))) return BVC_EMISSING;
    if ((rc = upload(m, pack_linear(t->h_data, 3 * H, H), &m->w_hh))) return rc;
    if ((rc = upload(m, pack_gru_interleaved(t->h_data, H, H), &m->w_hh_il))) return rc;
    if ((rc = r.vec("rnn.bias_ih_l0", 3 * H, &m->b_ih))) return rc;
    return r.vec("rnn.bias_hh_l0", 3 * H, &m->b_hh);
}

// What the generator's kernels exist for, checked once the flag tensors are read; the refusals come in this order.  The one place
// that derives antialiased / symmetric / noncausal.
struct Causality { bool antialiased, symmetric, noncausal; };
int check_layout(const bvc_config &c, const bool *stage_aa, bool post_aa, const bool *stage_sym, bool pre_sym, bool post_sym, bool fused_amp,
                 Causality *out) {
    bool stages_sym = false, stages_aa = false;
    for (int i = 0; i < c.n_up; ++i) {
        stages_sym = stages_sym || stage_sym[i];
        stages_aa = stages_aa || stage_aa[i];
        if (stage_sym[i] && stage_aa[i]) {
            set_error("stage %d is symmetric and anti-aliased: filtered stages are implemented as causal stages only", i);
            return BVC_EINVAL;
        }
    }
    if (post_sym && post_aa) { set_error("post_sym with antialias_post: a filtered activation_post is implemented in front of a causal conv_post only"); return BVC_EINVAL; }
    if (stages_sym) {
        for (int j = 0; j < c.n_resk; ++j)
            if (c.res_kernels[j] % 2 == 0) { set_error("a symmetric stage needs odd resblock kernel sizes (got %d)", c.res_kernels[j]); return BVC_EINVAL; }
        for (int i = 0; i < c.n_up; ++i)
            if (stage_sym[i] && c.up_rates[i] % 2) { set_error("a symmetric upsampler needs an even rate (got %d)", c.up_rates[i]); return BVC_EINVAL; }
        if (!fused_amp) { set_error("symmetric stages run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)"); return BVC_EINVAL; }
    }
    // wide stages (128 / 256 channels, generators of 256 / 512 initial channels) exist as causal, unfiltered, fused pairs only
    for (int i = 0; i < c.n_up; ++i) {
        const int C = c.upsample_initial_channel >> (i + 1);
        if (C < 128) continue;
        if (stage_sym[i]) { set_error("stage %d has %d channels: symmetric layers (layers_sym) are implemented on stages of 64 channels at most", i, C); return BVC_EINVAL; }
        if (stage_aa[i]) { set_error("stage %d has %d channels: anti-aliased activations (layers_antialias) are implemented on stages of 64 channels at most", i, C); return BVC_EINVAL; }
        if (!fused_amp) { set_error("stage %d has %d channels: wide stages run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)", i, C); return BVC_EINVAL; }
    }
    out->antialiased = post_aa || stages_aa;
    out->symmetric = pre_sym || post_sym || stages_sym;
    out->noncausal = out->antialiased || out->symmetric;
    if (out->antialiased && !fused_amp) { set_error("anti-aliased activations run in the fused AMP kernels only (BVC_UNFUSED_AMP is set)"); return BVC_EINVAL; }
    return BVC_OK;
}

int build_vocoder(const TensorReader &r) {
    bvc_model *m = r.m;
    const bvc_config &c = m->cfg;
    int rc;
    // symmetric paddings: optional tensors "layers_sym" (n_up values), "pre_sym" and "post_sym" (one value each); no keys of their own
    bool stage_aa[8] = {}, stage_sym[8] = {}, post_aa = false;                  // (n_up <= 8: check_config)
    if ((rc = r.flags("layers_antialias", c.n_up, stage_aa))) return rc;
    if ((rc = r.flags("antialias_post", 1, &post_aa))) return rc;
    if ((rc = r.flags("layers_sym", c.n_up, stage_sym))) return rc;
    if ((rc = r.flags("pre_sym", 1, &m->pre_sym))) return rc;
    if ((rc = r.flags("post_sym", 1, &m->post_sym))) return rc;
    m->stage_sym.assign(stage_sym, stage_sym + c.n_up);
    Causality cz;
    if ((rc = check_layout(c, stage_aa, post_aa, stage_sym, m->pre_sym, m->post_sym, m->fused_amp, &cz))) return rc;
    m->antialiased = cz.antialiased; m->symmetric = cz.symmetric; m->noncausal = cz.noncausal;
    if ((rc = r.conv("conv_pre", c.upsample_initial_channel, c.num_mels, 7, 1, nullptr, &m->conv_pre))) return rc;
    int ch = c.upsample_initial_channel;
    m->ups.resize(c.n_up);
    m->amp.resize(c.n_up);
    m->stage_ch.resize(c.n_up);
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i];
        if ((rc = r.conv("ups." + std::to_string(i) + ".1", u * (ch / 2), ch, 2, 1, nullptr, &m->ups[i], u))) return rc;
        ch /= 2;
        m->stage_ch[i] = ch;
        m->amp[i].resize(c.n_resk);
        for (int j = 0; j < c.n_resk; ++j) {
            const std::string pre = "resblocks." + std::to_string(i * c.n_resk + j);
            m->amp[i][j].resize(3);
            for (int d = 0; d < 3; ++d) {
                const std::string ds = std::to_string(d);
                Activation a1, a2;
                if ((rc = r.activation(pre + ".activations." + std::to_string(2 * d), ch, stage_aa[i], &a1))) return rc;
                if ((rc = r.activation(pre + ".activations." + std::to_string(2 * d + 1), ch, stage_aa[i], &a2))) return rc;
                AmpPair &ap = m->amp[i][j][d];
                if ((rc = r.conv(pre + ".convs1." + ds, ch, ch, c.res_kernels[j], c.res_dilations[j][d], &a1, &ap.c1))) return rc;
                if ((rc = r.conv(pre + ".convs2." + ds, ch, ch, c.res_kernels[j], 1, &a2, &ap.c2))) return rc;
            }
        }
    }
    m->post_c = ch;
    Activation post;
    if ((rc = r.activation("activation_post", ch, post_aa, &post))) return rc;
    m->post_up = post.up; m->post_down = post.down;
    std::vector<float> a, ib;
    snake_params(post.alpha, post.beta, ch, &a, &ib);
    if ((rc = upload(m, a, &m->post_a))) return rc;
    if ((rc = upload(m, ib, &m->post_ib))) return rc;
    const bvc_tensor *w, *b;
    if (!(w = r.find("conv_post.weight", (int64_t)ch * 7))) return BVC_EMISSING;
    if (!(b = r.find("conv_post.bias", 1))) return BVC_EMISSING;
    if ((rc = upload_raw(m, w->h_data, w->numel, &m->post_w))) return rc;
    return upload_raw(m, b->h_data, 1, &m->post_b);
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

}  // namespace

namespace bvc {

// ---- the environment switches of the model (host only), all read here and nowhere else:
//   at bvc_model_create (the model keeps what it read)
//                       BVC_NO_GRAPH=1         the launch-per-layer recurrence is launched eagerly, no hipGraph replay (first character '1')
//                       BVC_SIDE_BRANCH=1      the side-branch step plan; with it no pre-computed phi_z halves (first character '1')
//                       BVC_MTW=2|4            16-row tiles per workgroup in the recurrent kernels (first character '2' or '4'; else 1)
//                       BVC_UNFUSED_AMP=1      the generator's AMP pairs as separate convs (first character '1')
//                       BVC_NO_PRECOMP=1       decode: phi_z inside the step instead of batched over all frames (first character '1')
//                       BVC_RECURRENCE=layers|persistent   the recurrence schedule (the whole string; anything else: auto)
//                       BVC_DECODE_FOLD=0, BVC_ENCODE_FOLD=0   the persistent kernels without the folded hop px0_dec3 (first character '0';
//                                              A/B runs, tools/flow_variants.py)
//   at every residency census (flow_census)
//                       BVC_FLOW_CENSUS_OVERSUBSCRIBE   tests: a grid the device cannot hold (present, whatever its value)
//                       BVC_QUIET              no line on stderr when the census fails (present, whatever its value)
ModelSwitches model_switches() {
    auto first = [](const char *name, char c) { const char *v = getenv(name); return v && v[0] == c; };
    ModelSwitches sw;
    sw.use_graph = !first("BVC_NO_GRAPH", '1');
    sw.side_branch = first("BVC_SIDE_BRANCH", '1');
    sw.mtw = first("BVC_MTW", '2') ? 2 : first("BVC_MTW", '4') ? 4 : 1;
    sw.fused_amp = !first("BVC_UNFUSED_AMP", '1');
    sw.precomp = !first("BVC_NO_PRECOMP", '1');
    const char *rr = getenv("BVC_RECURRENCE");
    sw.recurrence = (rr && strcmp(rr, "layers") == 0) ? RS_LAYERS : (rr && strcmp(rr, "persistent") == 0) ? RS_PERSISTENT : RS_AUTO;
    sw.decode_fold = !first("BVC_DECODE_FOLD", '0');
    sw.encode_fold = !first("BVC_ENCODE_FOLD", '0');
    sw.census_oversubscribe = getenv("BVC_FLOW_CENSUS_OVERSUBSCRIBE") != nullptr;
    sw.quiet = getenv("BVC_QUIET") != nullptr;
    return sw;
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
    const ModelSwitches sw = model_switches();
    m->use_graph = sw.use_graph;
    m->side_branch = sw.side_branch;
    m->mtw = sw.mtw;
    m->fused_amp = sw.fused_amp;
    m->amp_kernels = amp_kernels_default();
    m->precomp_pz = sw.precomp && !sw.side_branch;
    m->decode_fold = sw.decode_fold;
    m->encode_fold = sw.encode_fold;
    m->recurrence = sw.recurrence;
    const TensorReader r{m.get(), tm};
    if ((rc = build_frontend(r))) return rc;
    if ((rc = build_bvrnn(r))) return rc;
    if ((rc = build_flow(m.get()))) return rc;
    if ((rc = build_vocoder(r))) return rc;
    BVC_HIP_TRY(hipDeviceSynchronize());
    *out = m.release();
    return BVC_OK;
}

void bvc_model_destroy(bvc_model *m) { delete m; }

}  // extern "C"
