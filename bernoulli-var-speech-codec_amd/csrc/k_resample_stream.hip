// Streaming rational-rate resampler for gfx950: resample_poly_kernel (k_frontend.hip) a chunk at a time, for B rows with lives of
// their own.  The sum of one output is that kernel's, term for term: pos = (m + n_pre_remove) * down, newest input i = pos / up,
// first tap k = pos - i * up, acc += h[k] * (double)x[i] with k ascending by `up` and i descending, one (float)acc - so what a row
// has been given after any chunking is a bit-exact prefix of the offline call on that row's own signal.
//
// One workgroup per row, one thread per output sample (a push of a 20 ms hop has a few hundred).  The row's history - the last
// H = ceil(ntaps / up) inputs - and its part of the chunk are staged in LDS as float32, so the 20 to 60 taps of an output read LDS;
// the taps come from global memory through the phase's stride (one phase per output, L2-resident).  The workgroup then writes the
// new history and the row's input count back: no other workgroup reads them, so one launch serves all rows without a second buffer.
//
// resample_stream_multi_kernel is the same launch for rows that each have a rate of their own: the filters travel as a table in the
// kernel's arguments, a row's control word names its entry, and a call has a chunk length per entry.  The two kernels are entry points
// that choose a row's filter; what they do with the row is the one rs_row, so a row gets the same bits from either.
#include "bvc_internal.h"

namespace bvc {

namespace {

__device__ __forceinline__ float rs_load(const void *x, long long idx, int fmt) {
    if (fmt == BVC_PCM_S16) return (float)static_cast<const short *>(x)[idx] * (1.0f / 32768.0f);      // exact
    return static_cast<const float *>(x)[idx];
}

// s16 = clamp(rintf(v * 32768), -32768, 32767) of the float32 the f32 path stores; NaN gives 0
__device__ __forceinline__ void rs_store(void *y, long long idx, float v, int fmt) {
    if (fmt == BVC_PCM_S16) {
        const float q = fminf(fmaxf(rintf(v * 32768.0f), -32768.0f), 32767.0f);
        static_cast<short *>(y)[idx] = v != v ? (short)0 : (short)q;
    } else {
        static_cast<float *>(y)[idx] = v;
    }
}

// Output m of a row's stream from the staged inputs: sx[t] is input N0 - H + t, N1 inputs have arrived, lo is the oldest staged one.
__device__ __forceinline__ float rs_walk(const RsFilter &f, const float *sx, long long m, long long N0, long long N1, long long lo) {
    const long long pos = (m + f.n_pre_remove) * f.down;
    long long i = pos / f.up;
    int k = (int)(pos - i * f.up);
    if (i >= N1) { const long long skip = i - (N1 - 1); i -= skip; k += (int)(skip * f.up); }   // a flush: zeros behind the end
    double acc = 0.0;
    for (; k < f.ntaps && i >= lo; k += f.up, --i) acc += f.h[k] * (double)sx[(int)(i - N0) + f.H];
    return (float)acc;
}

// Row changes since the last push: one workgroup per changed row, ahead of the push on its stream.
__global__ __launch_bounds__(64) void rs_update_kernel(RsUpdateList l, RsRow *__restrict__ ctl, float *__restrict__ hist, int H) {
    const RsUpdate u = l.e[blockIdx.x];
    if (u.reset)
        for (int t = threadIdx.x; t < H; t += blockDim.x) hist[(long long)u.row * H + t] = 0.0f;
    if (threadIdx.x == 0) {
        RsRow r = ctl[u.row];
        if (u.reset) { r.n = 0; r.rate = u.rate; }
        r.run = u.run; r.start = u.start; r.valid = u.valid;
        ctl[u.row] = r;
    }
}

// A row's push or flush behind the idle-row exit, for both kernels: filter f, a chunk of n_in samples, a block of n_fill outputs at most,
// stored with zeros behind them up to n_store; the row's history lies `stride` floats from its neighbours', `rate` is what it keeps.
template <typename Call>
__device__ __forceinline__ void rs_row(const RsFilter &f, const Call &c, const RsRow &r, int b, long long ybase, int n_in, int n_fill, int n_store,
                                       int stride, int rate, RsRow *__restrict__ ctl, float *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    float *sx = reinterpret_cast<float *>(rs_smem);
    const bool flush = c.flush_row >= 0;
    const int tid = threadIdx.x;
    // the row's samples of this chunk: [start, end)
    int end = flush ? 0 : (r.valid >= 0 && r.valid < n_in ? r.valid : n_in);
    int start = flush ? 0 : (r.start < end ? r.start : end);
    if (start < 0) start = 0;
    const int n_new = end - start;
    const int H = f.H;
    for (int t = tid; t < H; t += blockDim.x) sx[t] = hist[(long long)b * stride + t];
    for (int j = tid; j < n_new; j += blockDim.x) sx[H + j] = rs_load(c.x, (long long)b * c.xs + start + j, c.fmt_in);
    __syncthreads();
    // sx[t] is input N0 - H + t of the row's stream; inputs in front of the stream (index < 0) are not part of any sum
    const long long N0 = r.n, N1 = N0 + n_new;
    const long long q0 = rs_count(N0, f.up, f.down, f.n_pre_remove, c.delayed != 0);
    const long long q1 = flush ? rs_ceil_mul(N0, f.up, f.down) + (c.delayed ? f.n_pre_remove : 0)
                               : rs_count(N1, f.up, f.down, f.n_pre_remove, c.delayed != 0);
    long long count = q1 - q0;
    if (count > n_fill) count = n_fill;                      // (the host sizes n_fill from the same arithmetic: never taken)
    const long long lo = N0 - H > 0 ? N0 - H : 0;
    for (int j = tid; j < n_store; j += blockDim.x) {
        float out = 0.0f;
        const long long m = q0 + j - (c.delayed ? f.n_pre_remove : 0);     // delayed: n_pre_remove zeros lead the row's stream
        if (j < count && m >= 0) out = rs_walk(f, sx, m, N0, N1, lo);
        rs_store(c.y, ybase + j, out, c.fmt_out);
    }
    __syncthreads();
    if (flush) {                                              // the row is idle afterwards; its history is reset when it is opened
        if (tid == 0) { RsRow w = r; w.run = 0; w.start = 0; w.valid = -1; ctl[b] = w; }
        return;
    }
    for (int t = tid; t < H; t += blockDim.x) hist[(long long)b * stride + t] = sx[n_new + t];
    if (tid == 0) {
        RsRow w;
        w.n = N1; w.run = r.valid >= 0 ? 0 : 1; w.start = 0; w.valid = -1; w.rate = rate;
        ctl[b] = w;
    }
}

// grid = B rows (a push) or 1 (the flush of row c.flush_row); dynamic LDS: (H + n_in) floats
__global__ __launch_bounds__(256) void resample_stream_kernel(RsFilter f, RsCall c, RsRow *__restrict__ ctl, float *__restrict__ hist) {
    const bool flush = c.flush_row >= 0;
    const int b = flush ? c.flush_row : (int)blockIdx.x;
    const RsRow r = ctl[b];
    const long long ybase = (flush ? 0 : (long long)b * c.ys) + c.yoff;
    if (!flush && !r.run) {                                   // an idle row: zeros out, its input is never read
        for (int j = threadIdx.x; j < c.n_fill; j += blockDim.x) rs_store(c.y, ybase + j, 0.0f, c.fmt_out);
        return;
    }
    rs_row(f, c, r, b, ybase, c.n_in, c.n_fill, c.n_fill, f.H, 0, ctl, hist);
}

// The same for rows with a rate each: row b's filter is tab.f[its rate], its chunk c.n_in[rate] long, its history c.H_max floats from
// its neighbours'.  grid = B rows or 1 (a flush); dynamic LDS: the largest H_r + n_in[r] floats of the call (a flush: the row's H)
__global__ __launch_bounds__(256) void resample_stream_multi_kernel(RsFilterTable tab, RsCallMulti c, RsRow *__restrict__ ctl,
                                                                    float *__restrict__ hist) {
    const bool flush = c.flush_row >= 0;
    const int b = flush ? c.flush_row : (int)blockIdx.x;
    const RsRow r = ctl[b];
    const long long ybase = (flush ? 0 : (long long)b * c.ys) + c.yoff;
    if (!flush && !r.run) {                                   // an idle row: zeros out, its input is never read
        for (int j = threadIdx.x; j < c.n_fill_max; j += blockDim.x) rs_store(c.y, ybase + j, 0.0f, c.fmt_out);
        return;
    }
    RsFilter f = tab.f[0];                                     // (a chain of selects on the row's index: the table stays in the arguments)
    int n_in = c.n_in[0], n_fill = c.n_fill[0];
#pragma unroll
    for (int q = 1; q < RS_MAX_RATES; ++q)
        if (r.rate == q) { f = tab.f[q]; n_in = c.n_in[q]; n_fill = c.n_fill[q]; }
    if (flush) n_fill = c.n_fill_max;                        // (a flush: the row's rest)
    rs_row(f, c, r, b, ybase, n_in, n_fill, c.n_fill_max, c.H_max, r.rate, ctl, hist);
}

}  // namespace

int launch_rs_update(const RsUpdateList &l, RsRow *ctl, float *hist, int H, hipStream_t s) {
    if (l.n <= 0) return BVC_OK;
    hipLaunchKernelGGL(rs_update_kernel, dim3(l.n), dim3(64), 0, s, l, ctl, hist, H);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_rs_push(const RsFilter &f, const RsCall &c, int lds_floats, RsRow *ctl, float *hist, int B, hipStream_t s) {
    hipLaunchKernelGGL(resample_stream_kernel, dim3(c.flush_row >= 0 ? 1 : B), dim3(256), (size_t)lds_floats * sizeof(float), s, f, c, ctl, hist);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_rs_push_multi(const RsFilterTable &t, const RsCallMulti &c, int lds_floats, RsRow *ctl, float *hist, int B, hipStream_t s) {
    hipLaunchKernelGGL(resample_stream_multi_kernel, dim3(c.flush_row >= 0 ? 1 : B), dim3(256), (size_t)lds_floats * sizeof(float), s, t, c,
                       ctl, hist);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
