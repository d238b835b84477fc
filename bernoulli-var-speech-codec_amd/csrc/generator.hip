// The generator (BigVGAN): the offline pass over a whole utterance, the incremental, history-buffer pass of the streaming paths, and the
// same behind a look-ahead window, which admits symmetric layers.
#include <algorithm>
#include <memory>

#include "bvc_host.h"

using namespace bvc;

namespace {

// Iteration d of AMP block j: where its pair writes and how it ends.  Iterations 0 and 1 go to the block's own P and Q with the plain
// residual; the last one goes to the stage's running sum XS - the first block stores, the others add, the last divides by the block count.
enum { AMP_P = 0, AMP_Q = 1, AMP_XS = 2 };
struct AmpTarget { int buf, epi; };
inline AmpTarget amp_target(const bvc_config &c, int j, int d) {
    if (d < 2) return {d == 0 ? AMP_P : AMP_Q, CE_RES};
    if (j == 0 || c.n_resk == 1) return {AMP_XS, CE_RES};
    return {AMP_XS, j + 1 < c.n_resk ? CE_RES_ACC : CE_RES_ACC_DIV};
}

// (one workgroup per (tensor, stream) with four 16-byte pieces in flight per thread measured slower: 67 against 56 us at 256 streams)
__global__ __launch_bounds__(256) void stream_rotate_kernel(const RotEntry *__restrict__ tab, int k, int parity) {
    const RotEntry e = tab[blockIdx.z];
    const long long n4 = (long long)e.H * e.C / 4;
    const float4 *src = reinterpret_cast<const float4 *>(e.buf[parity] + (long long)blockIdx.y * e.bs +
                                                         (long long)k * e.rate * e.C);
    float4 *dst = reinterpret_cast<float4 *>(e.buf[parity ^ 1] + (long long)blockIdx.y * e.bs);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void stream_rows_in_kernel(const float *__restrict__ src, long long src_bs,
                                                             float *__restrict__ dst, long long dst_bs, long long n) {
    const float *s = src + (long long)blockIdx.y * src_bs;
    float *d = dst + (long long)blockIdx.y * dst_bs;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) d[i] = s[i];
}

int stream_push(bvc_vocoder_stream *st, const float *d_mel, int k, float div, float *d_wav, hipStream_t s) {
    const bvc_model *m = st->m;
    const bvc_config &c = m->cfg;
    const int B = st->B, p = st->parity;
    int rc;
    auto bs = [](const StreamTensor &t) { return t.rows * t.C; };
    // first row of this hop's window of a tensor (its history; the new rows follow)
    auto at = [&](const StreamTensor &t) { return t.buf[p] + (long long)st->cursor * t.rate * t.C; };
    // new mel rows behind the history
    stream_rows_in_kernel<<<dim3((unsigned)((k * st->mel.C + 255) / 256), B), 256, 0, s>>>(
        d_mel, (long long)k * st->mel.C, at(st->mel) + (long long)st->mel.H * st->mel.C, bs(st->mel), (long long)k * st->mel.C);
    BVC_HIP_TRY(hipGetLastError());
    // conv_pre: mel rows [Hm, Hm+k) -> y0 rows [Hy, Hy+k)
    {
        ConvWindow w{bs(st->mel), bs(st->y0), st->mel.H, 0};
        float *out = at(st->y0) + (long long)(st->y0.H - st->mel.H) * st->y0.C;
        if ((rc = launch_conv_mfma(m->conv_pre, at(st->mel), st->mel.H + k, out, st->mel.H + k, B, CE_STORE, nullptr,
                                   nullptr, 1.0f, s, &w))) return rc;
    }
    const StreamTensor *prev = &st->y0;
    long long rate_prev = 1;
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i];
        const StreamTensor &X = st->X[i], &XS = st->XS[i];
        // transposed conv as a 2-tap conv over the view (rows/u, u*C): view row q <-> X rows [u*q, u*q+u)
        {
            const long long hq = X.H / u;                              // history rows of the view
            const long long nq = rate_prev * k;                        // new view rows
            ConvWindow w{bs(*prev), bs(X), hq, 0};
            const float *in = at(*prev) + (long long)(prev->H - hq) * prev->C;
            if ((rc = launch_conv_mfma(m->ups[i], in, hq + nq, at(X), hq + nq, B, CE_STORE, nullptr, nullptr, 1.0f, s, &w))) return rc;
        }
        const long long L = X.H + (long long)X.rate * k;
        // t_origin only decides which rows lie before the start of the signal; from STREAM_WARM_FRAMES frames on none
        // does, so the value is frozen there (a hop captured into a hipGraph then replays with identical arguments)
        const long long fr = st->frames < STREAM_WARM_FRAMES ? st->frames : STREAM_WARM_FRAMES;
        ConvWindow w{bs(X), bs(X), X.H, (long long)X.rate * fr - X.H};
        if (st->d_age) { w.t_origin = -(long long)X.H; w.row_age = st->d_age; w.age_rate = X.rate; }    // per row, read by the kernel
        for (int j = 0; j < c.n_resk; ++j) {
            const StreamTensor &P = st->P[i * c.n_resk + j], &Q = st->Q[i * c.n_resk + j];
            float *const bufs[3] = {at(P), at(Q), at(XS)};
            const float *cur = at(X);
            for (int d = 0; d < 3; ++d) {
                const AmpPair &ap = m->amp[i][j][d];
                const AmpTarget t = amp_target(c, j, d);
                float *const dst = bufs[t.buf];
                const int epi = t.epi;
                if ((rc = launch_amp_pair(ap.c1, ap.c2, cur, L, dst, B, epi, at(XS), (float)c.n_resk, s, &w, m->amp_kernels))) return rc;
                cur = dst;
            }
        }
        prev = &XS;
        rate_prev = X.rate;
    }
    {
        ConvWindow w{bs(*prev), 0, prev->H, 0};
        if ((rc = launch_conv_post(at(*prev), prev->H + rate_prev * k, m->post_c, m->post_ks, m->post_w, m->post_b,
                                   m->post_a, m->post_ib, div, d_wav, rate_prev * k, B, s, &w))) return rc;
    }
    if (!st->slide) {
        stream_rotate_kernel<<<dim3((unsigned)((st->max_hc4 + 255) / 256), B, st->n_ten), 256, 0, s>>>(st->d_tab, k, p);
        st->parity ^= 1;
    } else {
        st->cursor += k;                                     // the next hop's window starts behind this hop's rows
        if (st->cursor + st->kmax > st->cap_frames) {        // no room for another hop: history back to the front (the twin buffer IS the buffer)
            stream_rotate_kernel<<<dim3((unsigned)((st->max_hc4 + 255) / 256), B, st->n_ten), 256, 0, s>>>(st->d_tab, st->cursor, 0);
            st->cursor = 0;
        }
    }
    BVC_HIP_TRY(hipGetLastError());
    st->frames += k;
    return BVC_OK;
}

// ---- the look-ahead window: symmetric layers behind a bounded delay --------------------------------
// After n frames, rows [0, rate * n - lag) of a tensor are final (its frontier; below zero: none yet).  By the reference's paddings:
// mel 0; y0 3 where conv_pre is symmetric; X_i = u_i * lag(previous tensor), + u_i / 2 behind a symmetric upsampler (the view
// [u/2, u/2 + L u) of the causal rows); an iteration of a symmetric AMP block adds its reach (ks-1)(d+1)/2, so P and Q of a block lag
// by the partial sums and XS by the longest block's sum (`spread`: all three blocks add to the same rows); the waveform 3 more where
// conv_post is symmetric.  config.stream_lags (Python) is the same table.
inline long long amp_reach(const AmpPair &ap) { return (long long)(ap.c1.ks - 1) * (ap.c1.dil + 1) / 2; }
void stream_lags(const bvc_model *m, bvc_vocoder_stream *st) {
    const bvc_config &c = m->cfg;
    st->lag_y0 = m->pre_sym ? (m->conv_pre.ks - 1) / 2 : 0;
    st->lag_post = m->post_sym ? (m->post_ks - 1) / 2 : 0;
    long long lag = st->lag_y0, tail = 0;
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i];
        const bool sym = m->stage_sym[i];
        lag = lag * u + (sym ? u / 2 : 0);
        tail = sym ? tail * u : (tail + 1) * u;
        st->lag_x.push_back(lag);
        st->tail.push_back(tail);
        long long spread = 0;
        for (int j = 0; j < c.n_resk; ++j) {
            const long long r0 = sym ? amp_reach(m->amp[i][j][0]) : 0, r1 = sym ? amp_reach(m->amp[i][j][1]) : 0;
            const long long r2 = sym ? amp_reach(m->amp[i][j][2]) : 0;
            st->lag_p.push_back(r0);
            st->lag_q.push_back(r0 + r1);
            spread = std::max(spread, r0 + r1 + r2);
        }
        st->spread.push_back(spread);
        lag += spread;
    }
    st->delay = lag + st->lag_post;
}

__global__ __launch_bounds__(256) void stream_rows_zero_kernel(float *__restrict__ dst, long long dst_bs, long long n) {
    float *d = dst + (long long)blockIdx.y * dst_bs;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) d[i] = 0.0f;
}

inline long long not_below_zero(long long v) { return v > 0 ? v : 0; }

// samples a push of k frames (k >= 1) or the flush (k == -1) writes per row
int64_t stream_samples(const bvc_vocoder_stream *st, int k) {
    const long long spf = st->X.back().rate, n0 = st->frames;
    if (!st->lookahead) return k > 0 ? spf * k : 0;
    const long long done = not_below_zero(spf * n0 - st->delay);
    if (k > 0) return not_below_zero(spf * (n0 + k) - st->delay) - done;
    return n0 == 0 ? 0 : spf * n0 + st->tail.back() - done;
}

// One push (k new frames) or the flush (k = 0) of a look-ahead state.  Every tensor advances from its frontier at the old frame count to its
// frontier at the new one - at the flush to its true length, with the offline rules of the signal's end: rows behind it read as zeros.
// The launches are the causal windowed ones with their rows relabelled: conv_pre by 3 (its causal row t + 3 is row t), an upsampler by
// u / 2 (in buffer rows the same launch as the causal one: the histories are multiples of u), conv_post by 3.  What relabelling cannot
// give is the start of a symmetric upsampler's signal: its first group of u rows begins u / 2 rows before row 0, and those are zeroed
// behind the launch (the pairs read rows before the signal as zeros).  Its end needs nothing: the pairs' descriptor ends at the true length.
int stream_advance(bvc_vocoder_stream *st, const float *d_mel, int k, bool flush, float div, float *d_wav, hipStream_t s) {
    const bvc_model *m = st->m;
    const bvc_config &c = m->cfg;
    const int B = st->B, p = st->parity;
    const long long n0 = st->frames, n1 = n0 + k;
    int rc;
    if (flush && n0 == 0) { st->flushed = true; return BVC_OK; }
    auto bs = [](const StreamTensor &t) { return t.rows * t.C; };
    auto at = [&](const StreamTensor &t) { return t.buf[p]; };
    if (k > 0) {
        stream_rows_in_kernel<<<dim3((unsigned)((k * st->mel.C + 255) / 256), B), 256, 0, s>>>(
            d_mel, (long long)k * st->mel.C, at(st->mel) + (long long)st->mel.H * st->mel.C, bs(st->mel), (long long)k * st->mel.C);
        BVC_HIP_TRY(hipGetLastError());
    }
    // the tensor the next layer reads: its frontiers before and after this call, the row its buffer starts at, its true length at n0 frames
    struct Prev { const StreamTensor *t; long long f0, f1, origin, len; };
    Prev pv;
    {
        // launch row r is causal row n0 - Hm + r = row n0 - Hm + r - lag_y0 of y0
        const long long sh = st->lag_y0, g0 = n0 - st->mel.H;
        const long long lo = not_below_zero(n0 - sh) + sh, hi = flush ? n0 + sh : not_below_zero(n1 - sh) + sh;
        ConvWindow w{bs(st->mel), bs(st->y0), lo - g0, 0};
        float *out = at(st->y0) + (long long)(st->y0.H - st->mel.H) * st->y0.C;
        if (hi > lo && (rc = launch_conv_mfma(m->conv_pre, at(st->mel), n1 - g0, out, hi - g0, B, CE_STORE, nullptr, nullptr, 1.0f, s, &w))) return rc;
        pv = {&st->y0, n0 - sh, n1 - sh, n0 - sh - st->y0.H, n0};
    }
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i];
        const bool sym = m->stage_sym[i];
        const StreamTensor &X = st->X[i], &XS = st->XS[i];
        const long long H = X.H, hq = H / u, h = sym ? u / 2 : 0;
        const long long fx0 = u * pv.f0 - h, fx1 = u * pv.f1 - h, origin = fx0 - H;
        const long long Li = sym ? u * pv.len : u * (pv.len + 1);
        {
            // groups of u rows: group q is rows [u q - h, u q - h + u) of X and reads rows q - 1 and q of the previous tensor
            const long long qlo = not_below_zero(pv.f0), qhi = flush ? pv.len + 1 : not_below_zero(pv.f1);
            const long long lin = flush ? pv.len : not_below_zero(pv.f1);
            const long long hh = std::min(hq, pv.f0 - pv.origin), g0 = pv.f0 - hh;       // launch row r is group g0 + r
            ConvWindow w{bs(*pv.t), bs(X), qlo - g0, 0};
            const float *in = at(*pv.t) + (g0 - pv.origin) * pv.t->C;
            float *out = at(X) + (hq - hh) * u * X.C;
            if (qhi > qlo && (rc = launch_conv_mfma(m->ups[i], in, lin - g0, out, qhi - g0, B, CE_STORE, nullptr, nullptr, 1.0f, s, &w))) return rc;
            if (sym && qlo == 0 && qhi > 0) {                  // group 0 was written: its first u / 2 rows lie before the signal
                stream_rows_zero_kernel<<<dim3((unsigned)((h * X.C + 255) / 256), B), 256, 0, s>>>(at(X) + (-h - origin) * X.C, bs(X), h * X.C);
                BVC_HIP_TRY(hipGetLastError());
            }
        }
        // rows of the stage -> buffer rows: minus origin.  rel: how far a tensor's frontier lies before X's
        auto lo_of = [&](long long rel) { return not_below_zero(fx0 - rel) - origin; };
        auto hi_of = [&](long long rel) { return (flush ? Li : not_below_zero(fx1 - rel)) - origin; };
        for (int j = 0; j < c.n_resk; ++j) {
            const StreamTensor &P = st->P[i * c.n_resk + j], &Q = st->Q[i * c.n_resk + j];
            float *const bufs[3] = {at(P), at(Q), at(XS)};
            const long long rels[3] = {st->lag_p[i * c.n_resk + j], st->lag_q[i * c.n_resk + j], st->spread[i]};
            const float *cur = at(X);
            long long cur_rel = 0;
            for (int d = 0; d < 3; ++d) {
                const AmpPair &ap = m->amp[i][j][d];
                const AmpTarget t = amp_target(c, j, d);
                float *const dst = bufs[t.buf];
                const long long rb = lo_of(rels[t.buf]), re = hi_of(rels[t.buf]);
                if (re > rb) {
                    ConvWindow w{bs(X), bs(X), rb, origin};
                    w.lookahead = sym; w.row_end = re;
                    if ((rc = launch_amp_pair(ap.c1, ap.c2, cur, sym ? hi_of(cur_rel) : re, dst, B, t.epi, at(XS), (float)c.n_resk, s, &w,
                                              m->amp_kernels, sym))) return rc;
                }
                cur = dst;
                cur_rel = rels[t.buf];
            }
        }
        pv = {&XS, fx0 - st->spread[i], fx1 - st->spread[i], origin, Li};
    }
    {
        // launch row r is row origin + r of the last stage; sample t reads its rows t + lag_post - 6 .. t + lag_post
        const long long sh = st->lag_post;
        const long long lo = not_below_zero(pv.f0 - sh), hi = flush ? pv.len : not_below_zero(pv.f1 - sh);
        const long long lin = (flush ? pv.len : not_below_zero(pv.f1)) - pv.origin;
        ConvWindow w{bs(*pv.t), 0, lo + sh - pv.origin, 0};
        if (hi > lo) {
            if (!d_wav) { set_error("bvc_vocoder_stream: null output for %lld samples", hi - lo); return BVC_EINVAL; }
            if ((rc = launch_conv_post(at(*pv.t), lin, m->post_c, m->post_ks, m->post_w, m->post_b, m->post_a, m->post_ib, div, d_wav,
                                       hi - lo, B, s, &w))) return rc;
        }
    }
    if (flush) { st->flushed = true; return BVC_OK; }
    stream_rotate_kernel<<<dim3((unsigned)((st->max_hc4 + 255) / 256), B, st->n_ten), 256, 0, s>>>(st->d_tab, k, p);
    BVC_HIP_TRY(hipGetLastError());
    st->parity ^= 1;
    st->frames += k;
    return BVC_OK;
}

}  // namespace

namespace bvc {

// Runs the generator; stop_after: -1 = everything, otherwise the tap index of bvc_test_vocoder_tap.
// lim: nullptr, or the (n_up + 1) x B bounds of a mixed-length batch (launch_ragged_limits): the upsamplers' input rows per item, then
// the samples each item keeps of `length`.
// A symmetric stage (layers_sym[i]) works on a VIEW of the causal upsampler result: ConvTranspose1d(padding = (k-u)/2), k = 2u, is rows
// [u/2, u/2 + Lin u) of the (Lin+1) u causal rows, so the stage's x starts u/2 rows into w.X, has L = Lin u rows and the full buffer's
// batch stride; P, Q and XS take the same stride, which the next upsampler (or conv_post) reads them with.  The pair kernel's descriptor
// ends at the view's L rows: the u/2 discarded rows behind them - not zeros in memory - read as zeros.
int run_vocoder(const bvc_model *m, const Workspace &w, const float *d_mel, int B, int64_t T, int64_t length,
                float div, float *d_wav, int stop_after, const float **tap, int64_t *tap_len, int *tap_ch,
                hipStream_t s, const long long *lim, int64_t *tap_bs) {
    const bvc_config &c = m->cfg;
    int rc;
    if (lim && m->noncausal) { set_error("mixed-length decode: %s", not_causal(m)); return BVC_EINVAL; }
    auto give = [&](const float *p, int64_t len, int ch, int64_t bs) { *tap = p; *tap_len = len; *tap_ch = ch; if (tap_bs) *tap_bs = bs; return BVC_OK; };
    // pad[6,0] (pre_sym: [3,3]) + conv_pre (models.py:209-213); input is already time-major (B,T,80)
    if ((rc = launch_conv_mfma(m->conv_pre, d_mel, T, w.y0, T, B, CE_STORE, nullptr, nullptr, 1.0f, s, nullptr, nullptr, 0, m->pre_sym ? 3 : 0))) return rc;
    if (stop_after == 0) return give(w.y0, T, c.upsample_initial_channel, T * c.upsample_initial_channel);
    const float *cur_in = w.y0;
    int64_t Lin = T, in_bs = 0;                                         // in_bs: the input's batch stride where it is not dense
    for (int i = 0; i < c.n_up; ++i) {
        const int C = m->stage_ch[i], u = c.up_rates[i];
        const bool sym = m->stage_sym[i];
        const int64_t Lfull = (Lin + 1) * u, L = sym ? Lin * u : Lfull;
        const int64_t bs = sym ? Lfull * C : 0;                         // 0: dense, L * C
        // ConvTranspose1d as a 2-tap conv with u*C columns over Lin+1 rows (models.py:216-217)
        if ((rc = launch_conv_mfma(m->ups[i], cur_in, Lin, w.X, Lin + 1, B, CE_STORE, nullptr, nullptr, 1.0f, s, nullptr,
                                   lim ? lim + (size_t)i * B : nullptr, in_bs))) return rc;
        const float *const x0 = sym ? w.X + (size_t)(u / 2) * C : w.X;
        if (stop_after == 1 + 2 * i) return give(x0, L, C, sym ? bs : L * C);
        float *const bufs[3] = {w.P, w.Q, w.XS};
        for (int j = 0; j < c.n_resk; ++j) {                            // three parallel AMP blocks
            const float *cur = x0;
            for (int d = 0; d < 3; ++d) {
                const AmpPair &ap = m->amp[i][j][d];
                if (!m->fused_amp && (rc = launch_conv_mfma(ap.c1, cur, L, w.U, L, B, CE_STORE, nullptr, nullptr, 1.0f, s))) return rc;
                const AmpTarget t = amp_target(c, j, d);
                float *const dst = bufs[t.buf];
                const int epi = t.epi;
                if (m->fused_amp) {
                    if ((rc = launch_amp_pair(ap.c1, ap.c2, cur, L, dst, B, epi, w.XS, (float)c.n_resk, s, nullptr, m->amp_kernels, sym, bs))) return rc;
                } else if ((rc = launch_conv_mfma(ap.c2, w.U, L, dst, L, B, epi, cur, w.XS, (float)c.n_resk, s))) return rc;
                cur = dst;
            }
        }
        if (stop_after == 2 + 2 * i) return give(w.XS, L, C, sym ? bs : L * C);
        cur_in = w.XS;
        Lin = L;
        in_bs = bs;
    }
    const int64_t n_out = length < Lin ? length : Lin;
    if (in_bs && m->post_up) {                               // the filtered conv_post reads a dense signal: the symmetric last stage's rows move up
        if ((rc = copy_rows(cur_in, in_bs, w.P, Lin * m->post_c, Lin * m->post_c, B, s))) return rc;
        cur_in = w.P; in_bs = 0;
    }
    return launch_conv_post(cur_in, Lin, m->post_c, m->post_ks, m->post_w, m->post_b, m->post_a, m->post_ib, div,
                            d_wav, n_out, B, s, nullptr, lim ? lim + (size_t)c.n_up * B : nullptr, m->post_up, m->post_down,
                            m->post_sym, in_bs);
}

// dst[b][0 .. n) = src[b][0 .. n) for B items src_bs / dst_bs floats apart
int copy_rows(const float *src, long long src_bs, float *dst, long long dst_bs, long long n, int B, hipStream_t s) {
    if (B <= 0 || n <= 0) return BVC_OK;
    const long long blocks = (n + 255) / 256;
    stream_rows_in_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096), B), 256, 0, s>>>(src, src_bs, dst, dst_bs, n);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// lookahead: the state of bvc_vocoder_stream_create_lookahead (twin buffers only).  A stage's history grows from STREAM_H by the spread of
// the lags inside it, so that the last iteration of a block, which writes `spread` rows before X's frontier, still finds its reach
// behind it; every buffer has room for the rows of the flush, from the tensor's frontier to its true length.
int vocoder_stream_create(const bvc_model *m, int32_t B, int32_t max_frames_per_push, bool slide, bvc_vocoder_stream **out, bool lookahead) {
    const char *const fn = lookahead ? "bvc_vocoder_stream_create_lookahead" : "bvc_vocoder_stream_create";
    if (!m || !out || B <= 0 || max_frames_per_push <= 0 || (lookahead && slide)) { set_error("%s: bad arguments", fn); return BVC_EINVAL; }
    if (lookahead ? m->antialiased : m->noncausal) {
        if (m->antialiased) set_error("%s: %s", fn, not_causal(m));
        else set_error("%s: %s (bvc_vocoder_stream_create_lookahead streams it behind bvc_vocoder_lookahead samples of delay)", fn, not_causal(m));
        return BVC_EINVAL;
    }
    const bvc_config &c = m->cfg;
    // the history must cover every receptive field and stay aligned with the transposed-conv views
    long long rate = 1;
    for (int i = 0; i < c.n_up; ++i) {
        const int u = c.up_rates[i];
        if (STREAM_H % u) { set_error("streaming vocoder: upsample rate %d does not divide the history (%d)", u, STREAM_H); return BVC_EINVAL; }
        for (int j = 0; j < c.n_resk; ++j)
            for (int d = 0; d < 3; ++d) {
                const AmpPair &ap = m->amp[i][j][d];
                if ((ap.c1.ks - 1) * ap.c1.dil + (ap.c2.ks - 1) * ap.c2.dil > STREAM_H) {
                    set_error("streaming vocoder: AMP receptive field exceeds the history"); return BVC_EINVAL;
                }
            }
        rate *= u;
    }
    if (m->post_ks - 1 > STREAM_H) { set_error("streaming vocoder: conv_post kernel exceeds the history"); return BVC_EINVAL; }
    std::unique_ptr<bvc_vocoder_stream> st(new bvc_vocoder_stream());
    st->m = m; st->B = B; st->kmax = max_frames_per_push;
    st->slide = slide;
    st->lookahead = lookahead;
    std::vector<int> hist(c.n_up, STREAM_H);               // history rows per stage
    std::vector<long long> room_flush(c.n_up, 0);          // rows of the flush beyond the history
    if (lookahead) {
        stream_lags(m, st.get());
        for (int i = 0; i < c.n_up; ++i) {
            const int u = c.up_rates[i];
            hist[i] = STREAM_H + (int)st->spread[i];
            while (hist[i] % u || hist[i] % 4) ++hist[i];
            room_flush[i] = st->lag_x[i] + st->tail[i] + u;
            // every launch's reach-back lies inside the history: checked, not clamped
            long long back = 0;
            for (int j = 0; j < c.n_resk; ++j)
                for (int d = 0; d < 3; ++d)
                    back = std::max(back, m->stage_sym[i] ? amp_reach(m->amp[i][j][d]) : (long long)(m->amp[i][j][d].c1.ks - 1) * (m->amp[i][j][d].c1.dil + 1));
            const long long prev_left = i == 0 ? 1 : hist[i - 1] - st->spread[i - 1];
            if (hist[i] - st->spread[i] < back || prev_left < 1 || (i + 1 == c.n_up && hist[i] - st->spread[i] < m->post_ks - 1)) {
                set_error("%s: the history of stage %d (%d rows) does not cover its look-ahead (%lld) and reach (%lld)", fn, i, hist[i], st->spread[i], back);
                return BVC_EINVAL;
            }
        }
    }
    // frames of room behind the history: 32 (16 hops of one or two frames between two moves of the histories; 2.2 GB of buffers at 256 streams),
    // more only where longer hops need it
    st->cap_frames = slide ? std::max(2 * max_frames_per_push + 8, 32) : max_frames_per_push;
    const long long room = st->cap_frames;
    auto mk = [&](int C, int H, int r, long long flush_rows = 0) {
        StreamTensor t; t.buf[0] = t.buf[1] = nullptr; t.C = C; t.H = H; t.rate = r; t.rows = H + std::max((long long)r * room, flush_rows); return t;
    };
    st->mel = mk(c.num_mels, (m->conv_pre.ks - 1) * m->conv_pre.dil, 1);
    st->y0 = mk(c.upsample_initial_channel, std::max(hist[0] / c.up_rates[0], st->mel.H), 1, st->lag_y0);
    rate = 1;
    for (int i = 0; i < c.n_up; ++i) {
        rate *= c.up_rates[i];
        for (auto *v : {&st->X, &st->XS}) v->push_back(mk(m->stage_ch[i], hist[i], (int)rate, room_flush[i]));
        for (int j = 0; j < c.n_resk; ++j)
            for (auto *v : {&st->P, &st->Q}) v->push_back(mk(m->stage_ch[i], hist[i], (int)rate, room_flush[i]));
    }
    std::vector<StreamTensor *> all = {&st->mel, &st->y0};
    for (auto *v : {&st->X, &st->XS, &st->P, &st->Q})
        for (auto &t : *v) all.push_back(&t);
    size_t total = 0;
    const int copies = slide ? 1 : 2;
    for (auto *t : all) {
        total += copies * (size_t)B * t->rows * t->C;
        // moving the history back to the front must not overlap itself: it happens with more than cap_frames - 2 kmax frames behind it
        if (slide && (long long)(st->cap_frames - 2 * st->kmax + 1) * t->rate < t->H) { set_error("streaming vocoder: sliding window too short for its history"); return BVC_EINVAL; }
    }
    if (hipMalloc(reinterpret_cast<void **>(&st->pool), total * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("streaming vocoder: cannot allocate %zu bytes of history buffers", total * sizeof(float));
        return BVC_ENOMEM;
    }
    st->pool_floats = total;
    size_t off = 0;
    std::vector<RotEntry> tab;
    for (auto *t : all) {
        for (int q = 0; q < copies; ++q) { t->buf[q] = st->pool + off; off += (size_t)B * t->rows * t->C; }
        if (slide) t->buf[1] = t->buf[0];
        RotEntry e; e.buf[0] = t->buf[0]; e.buf[1] = t->buf[1]; e.bs = t->rows * t->C; e.C = t->C; e.H = t->H; e.rate = t->rate; e.pad_ = 0;
        tab.push_back(e);
        if ((t->H * t->C) % 4) { set_error("streaming vocoder: history of a tensor is not a multiple of 4 floats"); return BVC_EINVAL; }
        st->max_hc4 = std::max(st->max_hc4, t->H * t->C / 4);
    }
    st->n_ten = (int)tab.size();
    BVC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&st->d_tab), tab.size() * sizeof(RotEntry)));
    BVC_HIP_TRY(hipMemcpy(st->d_tab, tab.data(), tab.size() * sizeof(RotEntry), hipMemcpyHostToDevice));
    BVC_HIP_TRY(hipMemset(st->pool, 0, total * sizeof(float)));
    *out = st.release();
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int bvc_vocoder_stream_create(const bvc_model *m, int32_t B, int32_t max_frames_per_push, bvc_vocoder_stream **out) {
    return vocoder_stream_create(m, B, max_frames_per_push, false, out);
}

int64_t bvc_vocoder_lookahead(const bvc_model *m) {
    if (!m || m->antialiased) return -1;
    bvc_vocoder_stream st;
    stream_lags(m, &st);
    return st.delay;
}

int bvc_vocoder_stream_create_lookahead(const bvc_model *m, int32_t B, int32_t max_frames_per_push, bvc_vocoder_stream **out) {
    return vocoder_stream_create(m, B, max_frames_per_push, false, out, true);
}

int64_t bvc_vocoder_stream_samples(const bvc_vocoder_stream *st, int32_t k) {
    if (!st || st->flushed || (k != -1 && (k <= 0 || k > st->kmax))) return 0;
    return stream_samples(st, k);
}

int bvc_vocoder_stream_flush(bvc_vocoder_stream *st, float out_scale_div, float *d_wav, void *stream) {
    if (!st) { set_error("null stream state"); return BVC_EINVAL; }
    if (int st_ = sticky_status(st->m)) return st_;
    if (!st->lookahead) { set_error("bvc_vocoder_stream_flush: the state was not made by bvc_vocoder_stream_create_lookahead"); return BVC_EINVAL; }
    if (st->flushed) { set_error("bvc_vocoder_stream_flush: the stream is flushed; only bvc_vocoder_stream_reset is legal"); return BVC_EINVAL; }
    return stream_advance(st, nullptr, 0, true, out_scale_div, d_wav, (hipStream_t)stream);
}

void bvc_vocoder_stream_destroy(bvc_vocoder_stream *st) { delete st; }

int bvc_vocoder_stream_reset(bvc_vocoder_stream *st, void *stream) {
    if (!st) { set_error("null stream state"); return BVC_EINVAL; }
    BVC_HIP_TRY(hipMemsetAsync(st->pool, 0, st->pool_floats * sizeof(float), (hipStream_t)stream));
    st->parity = 0; st->frames = 0; st->cursor = 0; st->flushed = false;
    return BVC_OK;
}

int bvc_vocoder_stream_push(bvc_vocoder_stream *st, const float *d_mel, int32_t k, float out_scale_div, float *d_wav,
                            void *stream) {
    if (!st || !d_mel || (!d_wav && !st->lookahead)) { set_error("null argument"); return BVC_EINVAL; }
    if (int st_ = sticky_status(st->m)) return st_;
    if (k <= 0 || k > st->kmax) { set_error("bvc_vocoder_stream_push: k=%d outside 1..%d", (int)k, st->kmax); return BVC_EINVAL; }
    if (st->flushed) { set_error("bvc_vocoder_stream_push: the stream is flushed; only bvc_vocoder_stream_reset is legal"); return BVC_EINVAL; }
    if (st->lookahead) return stream_advance(st, d_mel, k, false, out_scale_div, d_wav, (hipStream_t)stream);
    return stream_push(st, d_mel, k, out_scale_div, d_wav, (hipStream_t)stream);
}

}  // extern "C"
