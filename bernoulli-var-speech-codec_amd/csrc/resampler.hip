// bvc_resampler_* (include/bvcodec.h): the host side of the streaming resampler - the filter design, the rows' book and the two
// launches of a push.  One object serves both forms of the ABI: a table of filters, one per rate, and a rate per row; the single-rate
// form is the table of one, and differs in the calls it takes and the kernel it launches.  Host only; the kernels are in
// k_resample_stream.hip.
#include <cmath>

#include "bvc_internal.h"

using namespace bvc;

namespace {

// ---- the filter: bvcodec.preprocess.design(rate_out, rate_in), i.e. what scipy.signal.resample_poly(x, rate_out, rate_in) designs
struct Geometry { int up, down, half_len, n_pre_pad, n_pre_remove, ntaps, H; };

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

bool geometry(int rate_in, int rate_out, Geometry *g) {
    if (rate_in <= 0 || rate_out <= 0) return false;
    const int d = gcd_i(rate_in, rate_out);
    g->up = rate_out / d; g->down = rate_in / d;
    const int max_rate = g->up > g->down ? g->up : g->down;
    if (max_rate > (1 << 20)) return false;                  // (coprime rates of millions: 20 * max_rate taps)
    g->half_len = 10 * max_rate;
    g->n_pre_pad = g->down - g->half_len % g->down;
    g->n_pre_remove = (g->half_len + g->n_pre_pad) / g->down;
    g->ntaps = g->n_pre_pad + 2 * g->half_len + 1;
    g->H = (g->ntaps + g->up - 1) / g->up;
    return true;
}

// numpy's i0 on [0, 8] (Clenshaw's Chebyshev series, the coefficients of Cephes' i0 as numpy.i0 carries them), in numpy's order
const double I0A[30] = {
    -4.4153416464793395e-18, 3.3307945188222384e-17, -2.431279846547955e-16, 1.715391285555133e-15, -1.1685332877993451e-14,
    7.676185498604936e-14, -4.856446783111929e-13, 2.95505266312964e-12, -1.726826291441556e-11, 9.675809035373237e-11,
    -5.189795601635263e-10, 2.6598237246823866e-09, -1.300025009986248e-08, 6.046995022541919e-08, -2.670793853940612e-07,
    1.1173875391201037e-06, -4.4167383584587505e-06, 1.6448448070728896e-05, -5.754195010082104e-05, 0.00018850288509584165,
    -0.0005763755745385824, 0.0016394756169413357, -0.004324309995050576, 0.010546460394594998, -0.02373741480589947,
    0.04930528423967071, -0.09490109704804764, 0.17162090152220877, -0.3046826723431984, 0.6767952744094761};

double i0_small(double x) {
#pragma clang fp contract(off)
    const double y = x / 2.0 - 2.0;
    double b0 = I0A[0], b1 = 0.0, b2 = 0.0;
    for (int i = 1; i < 30; ++i) { b2 = b1; b1 = b0; b0 = y * b1 - b2 + I0A[i]; }
    return std::exp(x) * (0.5 * (b0 - b2));
}

// numpy's pairwise sum, the inner loop of add.reduce over contiguous float64 (blocks of 128 with eight partial sums)
double pairwise_sum(const double *a, long long n) {
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (long long i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

// numpy's sum of a contiguous float64 array: the reduction hands its inner loop 8192 elements at a time (numpy's buffer size), so
// the pairwise sums of those blocks are added up from left to right; up to 8192 elements it is one pairwise sum
double numpy_sum(const double *a, long long n) {
#pragma clang fp contract(off)
    const long long block = 8192;
    double res = 0.0;
    for (long long i = 0; i < n; i += block) res += pairwise_sum(a + i, n - i < block ? n - i : block);
    return res;
}

// h (g.ntaps doubles): n_pre_pad zeros, then firwin(2 half_len + 1, 1 / max_rate, window=("kaiser", 5.0)) * up, as preprocess.design
// computes it in numpy float64, operation for operation.  Equal rates: the unit impulse (preprocess.resample_poly copies there).
void design_taps(const Geometry &g, double *h) {
#pragma clang fp contract(off)
    const int numtaps = 2 * g.half_len + 1;
    double *w = h + g.n_pre_pad;
    for (int i = 0; i < g.n_pre_pad; ++i) h[i] = 0.0;
    if (g.up == 1 && g.down == 1) {
        for (int i = 0; i < numtaps; ++i) w[i] = i == g.half_len ? 1.0 : 0.0;
        return;
    }
    const double pi = 3.141592653589793;
    const double cutoff = 1.0 / (double)(g.up > g.down ? g.up : g.down);
    const double alpha = (numtaps - 1) / 2.0, beta = 5.0, i0_beta = i0_small(beta);
    for (int i = 0; i < numtaps; ++i) {
        const double m = (double)i - alpha;
        const double cm = cutoff * m;
        const double y = pi * (cm == 0.0 ? 1.0e-20 : cm);
        const double sinc = std::sin(y) / y;
        const double q = ((double)i - alpha) / alpha;
        const double kaiser = i0_small(std::fabs(beta * std::sqrt(1.0 - q * q))) / i0_beta;
        w[i] = cutoff * sinc * kaiser;
    }
    const double sum = numpy_sum(w, numtaps);
    for (int i = 0; i < numtaps; ++i) w[i] = w[i] / sum * (double)g.up;
}

enum { ROW_IDLE = 0, ROW_RUNNING = 1, ROW_ENDED = 2 };
const int FMT_MASK = 15;

}  // namespace

struct bvc_resampler {
    int B = 0, fmt_in = 0, fmt_out = 0;
    bool delayed = false;
    bool multi = false;                                      // made by bvc_resampler_create_multi: it takes the calls of that form, and the table kernel
    // one filter per rate and the longest chunk at each; a single-rate object is the table of one: rate 0, hist_stride == gs[0].H
    int n_rates = 0;
    Geometry gs[RS_MAX_RATES] = {};
    int max_ins[RS_MAX_RATES] = {};
    double *d_hs[RS_MAX_RATES] = {};
    float *d_hist = nullptr;
    RsRow *d_ctl = nullptr;
    int hist_stride = 0;                                     // floats between two rows' histories: the largest H of the table
    // the book: what the device holds for a row once the pending changes have been sent (rate: the row's filter, from open to idle)
    struct Row { int state = ROW_IDLE; long long n = 0; int start = 0, valid = -1; bool dirty = false, reset = false; int rate = 0; };
    std::vector<Row> rows;
    int n_dirty = 0;
    ~bvc_resampler() {
        for (double *p : d_hs) if (p) (void)hipFree(p);
        if (d_hist) (void)hipFree(d_hist);
        if (d_ctl) (void)hipFree(d_ctl);
    }
};

namespace {

int row_arg(const bvc_resampler *r, int row, const char *fn) {
    if (!r) { set_error("%s: null resampler", fn); return BVC_EINVAL; }
    if (row < 0 || row >= r->B) { set_error("%s: row %d outside 0..%d", fn, row, r->B - 1); return BVC_EINVAL; }
    return BVC_OK;
}

// open, push and set_taps come in a single-rate and a multi-rate form: BVC_EINVAL for the form that is not the object's
int kind_arg(const bvc_resampler *r, bool multi, const char *fn, const char *other) {
    if (!r) { set_error("%s: null resampler", fn); return BVC_EINVAL; }
    if (r->multi == multi) return BVC_OK;
    set_error("%s: a %s resampler takes %s", fn, multi ? "single-rate" : "multi-rate", other);
    return BVC_EINVAL;
}

bool pcm_formats_ok(int fmt_in, int fmt_out) {
    const int fo = fmt_out & FMT_MASK;
    return (fmt_in == BVC_PCM_F32 || fmt_in == BVC_PCM_S16) && (fo == BVC_PCM_F32 || fo == BVC_PCM_S16) &&
           !(fmt_out & ~(FMT_MASK | BVC_PCM_DELAYED));
}

bool fits_lds(const Geometry &g, int max_in) { return (size_t)(g.H + (long long)max_in) * sizeof(float) <= 64 * 1024; }

// The object of either create, for n validated filters and the longest chunk at each: the book, the device's buffers, the designed taps,
// zero histories, idle rows.  BVC_ENODEVICE and the host's BVC_ENOMEM are reported here.  A failing device call is BVC_EHIP with its
// error in e (allocated: the buffers were all there) and the object freed: each create maps that to its own code and text.
struct Created { int rc; hipError_t e; bool allocated; };

Created create(const char *fn, int B, int n, const Geometry *gs, const int32_t *max_in, int fmt_in, int fmt_out, bool multi, bvc_resampler **out) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        set_error("%s: no HIP device", fn);
        return {BVC_ENODEVICE, hipSuccess, false};
    }
    bvc_resampler *r = new (std::nothrow) bvc_resampler;
    if (!r) { set_error("%s: out of host memory", fn); return {BVC_ENOMEM, hipSuccess, false}; }
    r->B = B; r->fmt_in = fmt_in; r->fmt_out = fmt_out & FMT_MASK; r->delayed = (fmt_out & BVC_PCM_DELAYED) != 0;
    r->multi = multi; r->n_rates = n;
    for (int q = 0; q < n; ++q) {
        r->gs[q] = gs[q]; r->max_ins[q] = max_in[q];
        if (gs[q].H > r->hist_stride) r->hist_stride = gs[q].H;
    }
    r->rows.resize(B);
    const size_t hist_bytes = (size_t)B * r->hist_stride * sizeof(float), ctl_bytes = (size_t)B * sizeof(RsRow);
    const std::vector<RsRow> ctl(B, RsRow{0, 0, 0, -1, 0});
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->d_hist), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->d_ctl), ctl_bytes);
    for (int q = 0; q < n && e == hipSuccess; ++q) e = hipMalloc(reinterpret_cast<void **>(&r->d_hs[q]), (size_t)gs[q].ntaps * sizeof(double));
    const bool allocated = e == hipSuccess;
    for (int q = 0; q < n && e == hipSuccess; ++q) {
        std::vector<double> h(gs[q].ntaps);
        design_taps(gs[q], h.data());
        e = hipMemcpy(r->d_hs[q], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemset(r->d_hist, 0, hist_bytes);
    if (e == hipSuccess) e = hipMemcpy(r->d_ctl, ctl.data(), ctl_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete r;
        return {BVC_EHIP, e, allocated};
    }
    *out = r;
    return {BVC_OK, hipSuccess, true};
}

void mark(bvc_resampler *r, bvc_resampler::Row &w) {
    if (!w.dirty) { w.dirty = true; ++r->n_dirty; }
}

// open and open_rate behind their kind_arg: an idle row starts at `offset` of the next chunk with the filter of `rate`
int open_row(bvc_resampler *r, const char *fn, int row, int rate, int offset) {
    if (int rc = row_arg(r, row, fn)) return rc;
    bvc_resampler::Row &w = r->rows[row];
    if (w.state == ROW_RUNNING) { set_error("%s: row %d is running", fn, row); return BVC_EINVAL; }
    if (rate < 0 || rate >= r->n_rates) { set_error("%s: rate_index %d outside 0..%d", fn, rate, r->n_rates - 1); return BVC_EINVAL; }
    if (offset < 0 || offset > r->max_ins[rate]) { set_error("%s: offset %d outside 0..%d", fn, offset, r->max_ins[rate]); return BVC_EINVAL; }
    w.state = ROW_RUNNING; w.n = 0; w.start = offset; w.valid = -1; w.reset = true; w.rate = rate;
    mark(r, w);
    return BVC_OK;
}

// the changed rows -> device, RS_LIST rows per launch, ahead of the push or flush on its stream
int send_changes(bvc_resampler *r, hipStream_t s) {
    RsUpdateList l;
    l.n = 0;
    for (int b = 0; b < r->B && r->n_dirty > 0; ++b) {
        bvc_resampler::Row &w = r->rows[b];
        if (!w.dirty) continue;
        l.e[l.n++] = RsUpdate{b, w.state == ROW_RUNNING ? 1 : 0, w.start, w.valid, w.reset ? 1 : 0, w.rate, {0, 0}};
        w.dirty = w.reset = false;
        --r->n_dirty;
        if (l.n == RS_LIST) {
            if (int rc = launch_rs_update(l, r->d_ctl, r->d_hist, r->hist_stride, s)) return rc;
            l.n = 0;
        }
    }
    r->n_dirty = 0;
    return launch_rs_update(l, r->d_ctl, r->d_hist, r->hist_stride, s);
}

// A push of n_in[q] samples to the rows of rate q, as the kernels take it: the block of every rate and the call's longest
RsCallMulti push_call(const bvc_resampler *r, const void *d_x, long long xs, const int32_t *n_in, void *d_y, long long ys, long long yoff) {
    RsCallMulti c{d_x, xs, d_y, ys, yoff, {}, {}, 0, r->hist_stride, r->fmt_in, r->fmt_out, r->delayed ? 1 : 0, -1};
    for (int q = 0; q < r->n_rates; ++q) {
        c.n_in[q] = n_in[q];
        c.n_fill[q] = (int)rs_ceil_mul(n_in[q], r->gs[q].up, r->gs[q].down);
        if (c.n_fill[q] > c.n_fill_max) c.n_fill_max = c.n_fill[q];
    }
    return c;
}

RsFilter filter_of(const bvc_resampler *r, int q) {
    const Geometry &g = r->gs[q];
    return RsFilter{r->d_hs[q], g.ntaps, g.up, g.down, g.n_pre_remove, g.H};
}

// The launch of a push or flush, staging the largest H_q + n_in[q] floats of the call (a flush: the H of the row's rate): the
// single-rate kernel with the one filter and its form of the call for a single-rate object, the table kernel for the other
int launch(const bvc_resampler *r, const RsCallMulti &c, hipStream_t s) {
    int lds_floats = c.flush_row >= 0 ? r->gs[r->rows[c.flush_row].rate].H : 0;
    for (int q = 0; q < r->n_rates && c.flush_row < 0; ++q)
        if (r->gs[q].H + c.n_in[q] > lds_floats) lds_floats = r->gs[q].H + c.n_in[q];
    if (!r->multi) {
        const RsCall c1{c.x, c.xs, c.y, c.ys, c.yoff, c.n_in[0], c.n_fill_max, c.fmt_in, c.fmt_out, c.delayed, c.flush_row};
        return launch_rs_push(filter_of(r, 0), c1, lds_floats, r->d_ctl, r->d_hist, r->B, s);
    }
    RsFilterTable t{};
    t.n = r->n_rates;
    for (int q = 0; q < r->n_rates; ++q) t.f[q] = filter_of(r, q);
    return launch_rs_push_multi(t, c, lds_floats, r->d_ctl, r->d_hist, r->B, s);
}

// push and push_multi behind their argument checks: the rows' starts and ends against their chunks, the pending changes, the launch,
// and the book - the outputs the push gave every row, by the kernel's arithmetic
int push_rows(bvc_resampler *r, const char *fn, const RsCallMulti &c, int32_t *h_counts, hipStream_t s) {
    for (int b = 0; b < r->B; ++b) {
        const bvc_resampler::Row &w = r->rows[b];
        if (w.state == ROW_RUNNING && (w.start > c.n_in[w.rate] || w.valid > c.n_in[w.rate])) {
            set_error("%s: row %d starts at %d / ends at %d of a chunk of %d", fn, b, w.start, w.valid, c.n_in[w.rate]);
            return BVC_EINVAL;
        }
    }
    if (r->n_dirty > 0) { if (int rc = send_changes(r, s)) return rc; }
    if (int rc = launch(r, c, s)) return rc;
    for (int b = 0; b < r->B; ++b) {
        bvc_resampler::Row &w = r->rows[b];
        int count = 0;
        if (w.state == ROW_RUNNING) {
            const Geometry &g = r->gs[w.rate];
            const long long n1 = w.n + ((w.valid >= 0 ? w.valid : c.n_in[w.rate]) - w.start);
            count = (int)(rs_count(n1, g.up, g.down, g.n_pre_remove, r->delayed) - rs_count(w.n, g.up, g.down, g.n_pre_remove, r->delayed));
            w.n = n1; w.start = 0;
            if (w.valid >= 0) { w.state = ROW_ENDED; w.valid = -1; }
        }
        if (h_counts) h_counts[b] = count;
    }
    return BVC_OK;
}

}  // namespace

extern "C" {

int64_t bvc_resampler_count(int32_t rate_in, int32_t rate_out, int64_t n_inputs) {
    Geometry g;
    if (!geometry(rate_in, rate_out, &g) || n_inputs < 0) { set_error("bvc_resampler_count: rates must be positive, n_inputs not negative"); return BVC_EINVAL; }
    return rs_count(n_inputs, g.up, g.down, g.n_pre_remove, false);
}

int bvc_resampler_lag(int32_t rate_in, int32_t rate_out, int32_t *n_pre_remove, int32_t *history) {
    Geometry g;
    if (!geometry(rate_in, rate_out, &g)) { set_error("bvc_resampler_lag: rates must be positive"); return BVC_EINVAL; }
    if (n_pre_remove) *n_pre_remove = g.n_pre_remove;
    if (history) *history = g.H;
    return BVC_OK;
}

int bvc_resampler_taps(int32_t rate_in, int32_t rate_out, double *h_taps, int32_t capacity) {
    Geometry g;
    if (!geometry(rate_in, rate_out, &g)) { set_error("bvc_resampler_taps: rates must be positive"); return BVC_EINVAL; }
    if (h_taps && capacity >= g.ntaps) design_taps(g, h_taps);
    return g.ntaps;
}

int bvc_resampler_create(int32_t B, int32_t rate_in, int32_t rate_out, int32_t max_in, int32_t fmt_in, int32_t fmt_out, bvc_resampler **out) {
    const char *fn = "bvc_resampler_create";
    Geometry g;
    if (!out || B <= 0 || max_in <= 0 || !geometry(rate_in, rate_out, &g) || !pcm_formats_ok(fmt_in, fmt_out)) {
        set_error("%s: B, max_in and both rates must be positive, the formats BVC_PCM_F32 or BVC_PCM_S16", fn);
        return BVC_EINVAL;
    }
    if (!fits_lds(g, max_in)) {
        set_error("%s: history %d + max_in %d samples do not fit the 64 KiB of LDS a push stages them in", fn, g.H, (int)max_in);
        return BVC_EINVAL;
    }
    const Created c = create(fn, B, 1, &g, &max_in, fmt_in, fmt_out, false, out);
    if (c.rc != BVC_EHIP) return c.rc;
    if (!c.allocated) { set_error("%s: device allocation failed", fn); return BVC_ENOMEM; }      // (whatever the device gave as the reason)
    set_error("%s: %s", fn, hipGetErrorString(c.e));
    return BVC_EHIP;
}

void bvc_resampler_destroy(bvc_resampler *r) { delete r; }

int bvc_resampler_set_taps(bvc_resampler *r, const double *h_taps, int32_t ntaps) {
    if (int rc = kind_arg(r, false, "bvc_resampler_set_taps", "bvc_resampler_set_taps_rate")) return rc;
    if (!h_taps || ntaps != r->gs[0].ntaps) {
        set_error("bvc_resampler_set_taps: null argument, or not the %d taps of the design", r->gs[0].ntaps);
        return BVC_EINVAL;
    }
    BVC_HIP_TRY(hipMemcpy(r->d_hs[0], h_taps, (size_t)ntaps * sizeof(double), hipMemcpyHostToDevice));
    return BVC_OK;
}

int bvc_resampler_open(bvc_resampler *r, int32_t row, int32_t offset_in_next_push) {
    if (int rc = kind_arg(r, false, "bvc_resampler_open", "bvc_resampler_open_rate")) return rc;
    return open_row(r, "bvc_resampler_open", row, 0, offset_in_next_push);
}

int bvc_resampler_close(bvc_resampler *r, int32_t row) {
    if (int rc = row_arg(r, row, "bvc_resampler_close")) return rc;
    bvc_resampler::Row &w = r->rows[row];
    if (w.state == ROW_IDLE) return BVC_OK;
    w.state = ROW_IDLE; w.start = 0; w.valid = -1;
    mark(r, w);
    return BVC_OK;
}

int bvc_resampler_end(bvc_resampler *r, int32_t row, int32_t n_valid_in_next_push) {
    if (int rc = row_arg(r, row, "bvc_resampler_end")) return rc;
    bvc_resampler::Row &w = r->rows[row];
    if (w.state != ROW_RUNNING) { set_error("bvc_resampler_end: row %d is not running", (int)row); return BVC_EINVAL; }
    if (n_valid_in_next_push < w.start || n_valid_in_next_push > r->max_ins[w.rate]) {
        set_error("bvc_resampler_end: %d samples outside %d..%d", (int)n_valid_in_next_push, w.start, r->max_ins[w.rate]);
        return BVC_EINVAL;
    }
    w.valid = n_valid_in_next_push;
    mark(r, w);
    return BVC_OK;
}

int bvc_resampler_push(bvc_resampler *r, const void *d_x, int64_t x_row_stride, int32_t n_in, void *d_y, int64_t y_row_stride,
                       int64_t y_offset, int32_t *h_counts, void *stream) {
    if (int rc = kind_arg(r, false, "bvc_resampler_push", "bvc_resampler_push_multi")) return rc;
    if (!d_x || !d_y) { set_error("bvc_resampler_push: null argument"); return BVC_EINVAL; }
    if (n_in < 0 || n_in > r->max_ins[0]) { set_error("bvc_resampler_push: n_in %d outside 0..%d (max_in)", (int)n_in, r->max_ins[0]); return BVC_EINVAL; }
    const RsCallMulti c = push_call(r, d_x, x_row_stride, &n_in, d_y, y_row_stride, y_offset);
    if (x_row_stride < n_in || y_row_stride < c.n_fill_max || y_offset < 0) {
        set_error("bvc_resampler_push: a row of d_x holds n_in = %d samples, a row of d_y ceil(n_in up / down) = %d behind y_offset >= 0", (int)n_in, c.n_fill_max);
        return BVC_EINVAL;
    }
    return push_rows(r, "bvc_resampler_push", c, h_counts, (hipStream_t)stream);
}

int bvc_resampler_flush(bvc_resampler *r, int32_t row, void *d_y_row, int32_t *count, void *stream) {
    if (int rc = row_arg(r, row, "bvc_resampler_flush")) return rc;
    bvc_resampler::Row &w = r->rows[row];
    if (w.state == ROW_IDLE) { set_error("bvc_resampler_flush: row %d is idle", (int)row); return BVC_EINVAL; }
    const Geometry &g = r->gs[w.rate];
    const long long done = rs_count(w.n, g.up, g.down, g.n_pre_remove, r->delayed);
    const long long all = rs_ceil_mul(w.n, g.up, g.down) + (r->delayed ? g.n_pre_remove : 0);
    const int n = (int)(all - done);                         // <= n_pre_remove
    if (n > 0 && !d_y_row) { set_error("bvc_resampler_flush: null d_y_row for %d samples", n); return BVC_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (r->n_dirty > 0) { if (int rc = send_changes(r, s)) return rc; }       // (a row opened since the last push is reset first)
    w.state = ROW_IDLE; w.start = 0; w.valid = -1;           // the kernel leaves the device's copy of the row idle; its rate stays
    const RsCallMulti c{nullptr, 0, d_y_row, 0, 0, {}, {}, n, r->hist_stride, r->fmt_in, r->fmt_out, r->delayed ? 1 : 0, row};
    if (int rc = launch(r, c, s)) return rc;
    if (count) *count = n;
    return BVC_OK;
}

// ---- the multi-rate form: one filter per rate, a rate per row
int bvc_resampler_create_multi(int32_t B, int32_t n_rates, const int32_t *rates, int32_t fixed_rate, int32_t direction, const int32_t *max_in,
                               int32_t fmt_in, int32_t fmt_out, bvc_resampler **out) {
    const char *fn = "bvc_resampler_create_multi";
    if (!out || !rates || !max_in || B <= 0 || n_rates < 1 || n_rates > RS_MAX_RATES || (direction != 0 && direction != 1) ||
        !pcm_formats_ok(fmt_in, fmt_out)) {
        set_error("%s: B must be positive, n_rates 1..%d, direction 0 or 1, the formats BVC_PCM_F32 or BVC_PCM_S16", fn, RS_MAX_RATES);
        return BVC_EINVAL;
    }
    Geometry gs[RS_MAX_RATES];
    for (int q = 0; q < n_rates; ++q) {
        for (int p = 0; p < q; ++p)
            if (rates[p] == rates[q]) { set_error("%s: rate %d is listed twice", fn, (int)rates[q]); return BVC_EINVAL; }
        if (max_in[q] <= 0 || !geometry(direction ? fixed_rate : rates[q], direction ? rates[q] : fixed_rate, &gs[q])) {
            set_error("%s: rate %d: the rates and max_in must be positive", fn, (int)rates[q]);
            return BVC_EINVAL;
        }
        if (!fits_lds(gs[q], max_in[q])) {
            set_error("%s: rate %d: history %d + max_in %d samples do not fit the 64 KiB of LDS a push stages them in", fn, (int)rates[q],
                      gs[q].H, (int)max_in[q]);
            return BVC_EINVAL;
        }
    }
    const Created c = create(fn, B, n_rates, gs, max_in, fmt_in, fmt_out, true, out);
    if (c.rc != BVC_EHIP) return c.rc;
    set_error("%s: %s", fn, hipGetErrorString(c.e));
    return c.e == hipErrorOutOfMemory ? BVC_ENOMEM : BVC_EHIP;                                    // (only where the device says so)
}

int bvc_resampler_set_taps_rate(bvc_resampler *r, int32_t rate_index, const double *h_taps, int32_t ntaps) {
    if (int rc = kind_arg(r, true, "bvc_resampler_set_taps_rate", "bvc_resampler_set_taps")) return rc;
    if (rate_index < 0 || rate_index >= r->n_rates || !h_taps || ntaps != r->gs[rate_index].ntaps) {
        set_error("bvc_resampler_set_taps_rate: rate_index %d outside 0..%d, null taps, or not the taps of that rate's design", (int)rate_index,
                  r->n_rates - 1);
        return BVC_EINVAL;
    }
    BVC_HIP_TRY(hipMemcpy(r->d_hs[rate_index], h_taps, (size_t)ntaps * sizeof(double), hipMemcpyHostToDevice));
    return BVC_OK;
}

int bvc_resampler_open_rate(bvc_resampler *r, int32_t row, int32_t rate_index, int32_t offset_in_next_push) {
    if (int rc = kind_arg(r, true, "bvc_resampler_open_rate", "bvc_resampler_open")) return rc;
    return open_row(r, "bvc_resampler_open_rate", row, rate_index, offset_in_next_push);
}

int bvc_resampler_push_multi(bvc_resampler *r, const void *d_x, int64_t x_row_stride, const int32_t *n_in, void *d_y, int64_t y_row_stride,
                             int64_t y_offset, int32_t *h_counts, void *stream) {
    if (int rc = kind_arg(r, true, "bvc_resampler_push_multi", "bvc_resampler_push")) return rc;
    if (!d_x || !d_y || !n_in) { set_error("bvc_resampler_push_multi: null argument"); return BVC_EINVAL; }
    int n_in_max = 0;
    for (int q = 0; q < r->n_rates; ++q) {
        if (n_in[q] < 0 || n_in[q] > r->max_ins[q]) {
            set_error("bvc_resampler_push_multi: n_in[%d] = %d outside 0..%d (max_in)", q, (int)n_in[q], r->max_ins[q]);
            return BVC_EINVAL;
        }
        if (n_in[q] > n_in_max) n_in_max = n_in[q];
    }
    const RsCallMulti c = push_call(r, d_x, x_row_stride, n_in, d_y, y_row_stride, y_offset);
    if (x_row_stride < n_in_max || y_row_stride < c.n_fill_max || y_offset < 0) {
        set_error("bvc_resampler_push_multi: a row of d_x holds the longest chunk, %d samples, a row of d_y the longest block, %d, behind y_offset >= 0",
                  n_in_max, c.n_fill_max);
        return BVC_EINVAL;
    }
    return push_rows(r, "bvc_resampler_push_multi", c, h_counts, (hipStream_t)stream);
}

}  // extern "C"
