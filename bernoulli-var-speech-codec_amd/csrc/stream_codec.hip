#include <algorithm>
#include <memory>
#include <utility>

#include "bvc_host.h"

using namespace bvc;

// ---- whole-hop streaming codec (BASELINE configs[4]) -----------------------------------------------------
// B parallel streams, a fixed hop of new samples per tick; one tick = front-end of the frames the hop completes ->
// BVRNN.encode (state carried) -> BVRNN.decode (state carried) -> incremental vocoder.  Everything a tick touches
// lives at fixed device addresses and everything that changes from tick to tick (how many samples are buffered)
// is DEVICE state, so a tick with k new frames and vocoder parity p is the same launch sequence every time: it is
// captured once per (k, p) into a hipGraph and replayed.
namespace {

struct StreamDev { int fill; int pad_[3]; };             // samples buffered: sbuf[:, 0] is sample 256*F - 256, F = frames emitted

// row_off[b]: the row's delay in samples (its hop lands that far behind the session's fill level), < 0 for an idle row, whose hop is
// zeros whatever the caller's d_in holds; = cap for a row that drains (sc_finish_kernel): n <= 0 below, nothing is written
__global__ __launch_bounds__(256) void sc_append_kernel(const StreamDev *__restrict__ st, const float *__restrict__ xin, int hop,
                                                        float *__restrict__ sbuf, int cap, const int *__restrict__ row_off) {
    const int fill = st->fill;
    const int off = row_off[blockIdx.y];
    const int at = fill + (off < 0 ? 0 : off);
    float *d = sbuf + (long long)blockIdx.y * cap + at;
    const float *x = xin + (long long)blockIdx.y * hop;
    const int n = hop < cap - at ? hop : cap - at;
    if (off < 0) { for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = 0.0f; }
    else         { for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = x[i]; }
}
// first tick only: samples -256..-1 of the reflect padding (meldataset.py:72-81): x[-i] = x[i]
__global__ __launch_bounds__(256) void sc_reflect_left_kernel(float *__restrict__ sbuf, int cap, int pad) {
    float *d = sbuf + (long long)blockIdx.x * cap;
    for (int i = 1 + threadIdx.x; i <= pad; i += 256) d[pad - i] = d[pad + i];
}
__global__ __launch_bounds__(256) void sc_shift_kernel(const float *__restrict__ src, long long sstride, int soff,
                                                       float *__restrict__ dst, long long dstride, int n) {
    const float *a = src + (long long)blockIdx.y * sstride + soff;
    float *d = dst + (long long)blockIdx.y * dstride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = a[i];
}
// end of a tick: the fill level, and every row's age (frames since its own start, capped at `warm`: see bvc_vocoder_stream::d_age)
__global__ void sc_advance_kernel(StreamDev *st, int delta, int *__restrict__ age, int B, int k, int warm) {
    if (threadIdx.x == 0) st->fill += delta;
    if (k > 0)
        for (int b = threadIdx.x; b < B; b += blockDim.x) { const int a = age[b] + k; age[b] = a < warm ? a : warm; }
}

// ---- slots: rows of a session that are opened, closed and re-rated while the others keep running ----
// The host keeps the book; what changed since the last tick travels as a kernel argument (up to SC_LIST rows per launch).
const int SC_LIST = 64;
enum { SC_SET_OFF = 1, SC_ZERO_TAIL = 2, SC_SET_BITS = 4 };
struct SlotUpdate { int row, off, flags; float bits; };
struct SlotUpdateList { int n; int pad_[3]; SlotUpdate e[SC_LIST]; };
struct SlotRowList { int n; int pad_[3]; int row[SC_LIST]; };

// before the append of a tick: new delay / idle mark, the closed stream's tail out of the sample buffer, bits per frame in every
// (B, k) layout (bits_base: the layouts k = 1 .. kmax one behind the other)
__global__ __launch_bounds__(256) void sc_slot_update_kernel(SlotUpdateList l, const StreamDev *__restrict__ st, int *__restrict__ row_off,
                                                             float *__restrict__ sbuf, int cap, float *__restrict__ bits_base, int B, int kmax) {
    const SlotUpdate u = l.e[blockIdx.x];
    if ((u.flags & SC_SET_OFF) && threadIdx.x == 0) row_off[u.row] = u.off;
    if (u.flags & SC_ZERO_TAIL) {
        float *d = sbuf + (long long)u.row * cap;
        for (int i = st->fill + threadIdx.x; i < cap; i += 256) d[i] = 0.0f;
    }
    if (u.flags & SC_SET_BITS) {
        const int tri = kmax * (kmax + 1) / 2;             // layout k starts B * k (k - 1) / 2 floats in; entry i of the triangle is (k, j)
        for (int i = threadIdx.x; i < tri; i += 256) {
            int k = 1, j = i;
            while (j >= k) { j -= k; ++k; }
            bits_base[(long long)B * (k * (k - 1) / 2) + (long long)u.row * k + j] = u.bits;
        }
    }
}

// the tick that emits frame 0 of the rows in `l`, after the append: what a new session has at tick 0, for those rows only.
// blockIdx.y < n_ten: that tensor's history rows of the generator (both copies, where the windows stand); blockIdx.y == n_ten: the left
// reflect padding x[-i] = x[i] (the row's sample 0 sits `pad` samples into the buffer: its frame 0 is the first of this tick), both GRU
// states, the row's age.  A session that runs one half (bvc_stream_codec_create_dir) resets that half: h_dec != nullptr is the decoder half
// (generator histories, h_dec, age), h_enc != nullptr the encoder half (left reflect padding, h_enc; alone it is launched with n_ten = 0).
__global__ __launch_bounds__(256) void sc_slot_start_kernel(SlotRowList l, const RotEntry *__restrict__ tab, int n_ten, int cursor,
                                                            float *__restrict__ sbuf, int cap, int pad, float *__restrict__ h_enc,
                                                            float *__restrict__ h_dec, int Hd, int *__restrict__ age) {
    const int row = l.row[blockIdx.z];
    if ((int)blockIdx.y < n_ten) {
        const RotEntry e = tab[blockIdx.y];
        const long long n4 = (long long)e.H * e.C / 4;
        const long long at = (long long)row * e.bs + (long long)cursor * e.rate * e.C;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = 0; q < (e.buf[1] == e.buf[0] ? 1 : 2); ++q) {
            float4 *d = reinterpret_cast<float4 *>(e.buf[q] + at);
            for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) d[i] = z;
        }
        return;
    }
    if (blockIdx.x == 0) {
        if (h_enc) {
            float *d = sbuf + (long long)row * cap;
            for (int i = 1 + threadIdx.x; i <= pad; i += 256) d[pad - i] = d[pad + i];
        }
        if (h_dec && threadIdx.x == 0) age[row] = 0;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Hd; i += gridDim.x * 256) {
        if (h_enc) h_enc[(long long)row * Hd + i] = 0.0f;
        if (h_dec) h_dec[(long long)row * Hd + i] = 0.0f;
    }
}

// ... and in a session that chooses its own rates under a cap (bvc_stream_codec_create_vbr) those rows' buckets are full again
__global__ void sc_tok_start_kernel(SlotRowList l, int *__restrict__ tok, int full) {
    if ((int)threadIdx.x < l.n) tok[l.row[threadIdx.x]] = full;
}

// end of a stream (bvc_stream_codec_finish), after the append of the tick that takes its last hop: of that hop only the first n_last
// samples (SlotUpdate::off) are the stream's.  Directly behind them the right reflect padding of the front-end (meldataset.py:72-81):
// with e = the index one behind the last sample, d[e + i] = d[e - 2 - i], i = 0 .. rpad - 1; zeros from there to the end of the row (the
// rest of the hop is never used); and the row is marked as draining: row_off = cap, with which sc_append_kernel writes nothing (its n
// is <= 0), so whatever the session holds for the row stays where it is while the row rides along.  The host has checked that the
// stream is longer than rpad + 1 samples (all of them are still in the buffer: the frames that would drop them need the padding).
__global__ __launch_bounds__(256) void sc_finish_kernel(SlotUpdateList l, const StreamDev *__restrict__ st, int *__restrict__ row_off,
                                                        float *__restrict__ sbuf, int cap, int rpad) {
    const SlotUpdate u = l.e[blockIdx.x];
    float *d = sbuf + (long long)u.row * cap;
    const int off = row_off[u.row];
    int e = st->fill + (off < 0 ? 0 : off) + u.off;
    e = e < rpad + 1 ? rpad + 1 : (e > cap ? cap : e);      // never out of the row, whatever the state says
    const int pe = e + rpad < cap ? e + rpad : cap;
    for (int i = e + threadIdx.x; i < pe; i += 256) d[i] = d[2 * e - 2 - i];
    for (int i = pe + threadIdx.x; i < cap; i += 256) d[i] = 0.0f;
    __syncthreads();                                         // every lane has read row_off
    if (threadIdx.x == 0) row_off[u.row] = cap;
}

// ---- repair window (bvc_stream_codec_set_repair / _late): a receive session keeps, for the ticks that hold its last W frames, the decoder
// state in front of the tick and what the tick was given (bytes, present, bits per frame), so that a packet that arrives late can be put
// where it belonged and the recurrence replayed from there.  Ring slot r of tick t = t % n; per slot h (B, Hd), packets (B, kmax,
// bpf), present (B, kmax), bits (B, kmax), the slots `hs` floats / `pks` bytes / `prs` bytes / `bs` floats apart.
const int SC_LATE_BYTES = 16;                            // bytes per frame a late packet can carry in a kernel argument (z_dim <= 128)
const int SC_CHUNKS = 64;                                // ticks a replay can span: the window is at most 64 frames
struct LateEntry { int row, slot, j, pad_; unsigned char bytes[SC_LATE_BYTES]; };
struct LateList { int n; int pad_[3]; LateEntry e[SC_LIST]; };
struct ReplayChunk { int slot, k, off; };                // ring slot, frames of that tick, (row, frame) pairs of the pass in front of it
struct ReplayPlan { int n_chunks, n_rows, row0, pad_; int row[SC_LIST]; ReplayChunk c[SC_CHUNKS]; };

// one launch per receive tick of a session with a window, behind the tick's row starts: everything the tick is about to read
__global__ __launch_bounds__(256) void sc_snapshot_kernel(const float *__restrict__ h_dec, long long n_h4, float *__restrict__ ring_h,
                                                          const unsigned char *__restrict__ pk, long long n_pk, unsigned char *__restrict__ ring_pk,
                                                          const unsigned char *__restrict__ pr, long long n_pr, unsigned char *__restrict__ ring_pr,
                                                          unsigned char *__restrict__ host_pr, const float *__restrict__ bits_k,
                                                          float *__restrict__ ring_bits, int B, int k, int kmax) {
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long i = i0; i < n_h4; i += step) reinterpret_cast<float4 *>(ring_h)[i] = reinterpret_cast<const float4 *>(h_dec)[i];
    const long long n_pk16 = n_pk / 16;
    for (long long i = i0; i < n_pk16; i += step) reinterpret_cast<uint4 *>(ring_pk)[i] = reinterpret_cast<const uint4 *>(pk)[i];
    for (long long i = n_pk16 * 16 + i0; i < n_pk; i += step) ring_pk[i] = pk[i];
    for (long long i = i0; i < n_pr; i += step) { const unsigned char v = pr[i]; ring_pr[i] = v; host_pr[i] = v; }
    for (long long i = i0; i < (long long)B * k; i += step) { const long long b = i / k; ring_bits[b * kmax + (i - b * k)] = bits_k[i]; }
}

// the late packets queued since the last tick: bytes and present = 1 into the ring
__global__ __launch_bounds__(64) void sc_late_patch_kernel(LateList l, unsigned char *__restrict__ ring_pk, long long pks,
                                                           unsigned char *__restrict__ ring_pr, long long prs, int kmax, int bpf) {
    const LateEntry e = l.e[blockIdx.x];
    const long long f = (long long)e.row * kmax + e.j;
    if ((int)threadIdx.x < bpf) ring_pk[e.slot * pks + f * bpf + threadIdx.x] = e.bytes[threadIdx.x];
    if (threadIdx.x == 0) ring_pr[e.slot * prs + f] = 1;
}

// a replay pass: the listed rows' ring entries of the pass's ticks into a compact batch, tick after tick ((B', k) each, B' = the rows of
// the whole pass, this launch's first row being compact row row0), and their snapshot states of the first tick.  blockIdx = (tick, row).
__global__ __launch_bounds__(256) void sc_replay_gather_kernel(ReplayPlan p, const float *__restrict__ ring_h, long long hs,
                                                               const unsigned char *__restrict__ ring_pk, long long pks,
                                                               const unsigned char *__restrict__ ring_pr, long long prs,
                                                               const float *__restrict__ ring_bits, long long bs, int Hd, int kmax, int bpf,
                                                               float *__restrict__ r_h, unsigned char *__restrict__ r_pk,
                                                               unsigned char *__restrict__ r_pr, float *__restrict__ r_bits) {
    const ReplayChunk c = p.c[blockIdx.x];
    const int row = p.row[blockIdx.y], bp = p.row0 + (int)blockIdx.y;
    const long long src = (long long)row * kmax, dst = (long long)c.off + (long long)bp * c.k;
    for (int i = threadIdx.x; i < c.k * bpf; i += 256) r_pk[dst * bpf + i] = ring_pk[c.slot * pks + src * bpf + i];
    for (int i = threadIdx.x; i < c.k; i += 256) {
        r_pr[dst + i] = ring_pr[c.slot * prs + src + i];
        r_bits[dst + i] = ring_bits[c.slot * bs + src + i];
    }
    if (blockIdx.x == 0) {
        const float4 *a = reinterpret_cast<const float4 *>(ring_h + c.slot * hs + (long long)row * Hd);
        float4 *d = reinterpret_cast<float4 *>(r_h + (long long)bp * Hd);
        for (int i = threadIdx.x; i < Hd / 4; i += 256) d[i] = a[i];
    }
}

// the pass's states back into the rows of a (B, Hd) tensor: the snapshot of the next retained tick, or h_dec itself
__global__ __launch_bounds__(256) void sc_replay_scatter_kernel(SlotRowList l, int row0, const float *__restrict__ r_h, float *__restrict__ dst, int Hd) {
    const float4 *a = reinterpret_cast<const float4 *>(r_h + (long long)(row0 + (int)blockIdx.x) * Hd);
    float4 *d = reinterpret_cast<float4 *>(dst + (long long)l.row[blockIdx.x] * Hd);
    for (int i = threadIdx.x; i < Hd / 4; i += 256) d[i] = a[i];
}

}  // namespace

struct bvc_stream_codec {
    const bvc_model *m = nullptr;
    int B = 0, hop = 0, kmax = 0, cap = 0;
    float bits = 0.0f, scale = 1.0f, out_div = 1.0f;
    int fill = 0;                       // host mirror of StreamDev::fill (same arithmetic)
    int64_t frames = 0, ticks = 0;
    bool first = true;
    // device memory (one allocation)
    char *pool = nullptr;
    StreamDev *d_state = nullptr;
    float *d_in = nullptr, *sbuf = nullptr, *stmp = nullptr, *mel = nullptr, *bitsbuf = nullptr, *codes = nullptr, *melhat = nullptr,
          *wav = nullptr, *h_enc = nullptr, *h_dec = nullptr;
    void *ws = nullptr; size_t ws_bytes = 0;
    bvc_vocoder_stream *voc = nullptr;
    // slots: each row is a stream of its own (see include/bvcodec.h).  Device side: row_off (delay in samples, < 0 idle), age (frames
    // since the row's start, capped), bitsbuf = the bits per (row, frame) in every (B, k) layout, k = 1 .. kmax, one behind the other
    // (bits_of(k)): a tick - and a graph captured for its k - reads the layout of its own frame count.
    struct Slot {
        bool open = true, started = true;
        int delay = 0, pending = 0;     // pending: SC_* flags that the next tick sends to the device
        int64_t frame0 = 0;             // session frame that is the stream's frame 0
        float bits = 0.0f;
        int last_count = 0;             // frames of the last tick that belong to the stream, and the stream's index of the first
        int64_t last_frame0 = 0;
        int64_t open_tick = 0;          // the tick that took the stream's first hop
        int fin_last = -1;              // bvc_stream_codec_finish: samples of the next tick's hop that are the stream's last (-1: none asked)
        int64_t end_frame = -1;         // draining: the session frame behind the stream's last one (-1: not draining)
    };
    std::vector<Slot> slots;
    int *row_off = nullptr, *age = nullptr;
    int max_delay = 0;
    int n_pending = 0, n_waiting = 0;   // slots with pending flags / open slots whose frame 0 is still to come
    int n_finishing = 0;                // slots whose finish the next tick carries out
    // directed sessions (bvc_stream_codec_create_dir): SEND has no decoder half (h_dec, melhat, wav, voc are null), RECV no encoder half
    // (d_in, sbuf, stmp, mel, h_enc are null).  packets (B, kmax, bpf) / present (B, kmax): the wire side of both.
    int dir = BVC_STREAM_DUPLEX, bpf = 0;
    uint8_t *packets = nullptr, *present = nullptr;
    float *bits_of(int k) const { return bitsbuf + (size_t)B * (k * (k - 1) / 2); }
    const float *tick_bits(int k) const { return m->cfg.var_bit ? bits_of(k) : nullptr; }     // a fixed-rate model reads no bit counts
    hipGraphExec_t graph[2][8][2] = {}; // [conceal][k][vocoder parity]
    int conceal = 0;                    // receive sessions: 0 = a lost frame is a frame of no bits, 1 = generated from the prior (bvc_stream_codec_set_conceal)
    // repair window (bvc_stream_codec_set_repair; receive sessions): w = 0 is off, nothing is allocated and no tick launches more.  Owns the
    // ring, the replay's buffers, the host mirror and the events; bvc_stream_codec_set_repair builds one aside and moves it in.
    struct RepairMem {                  // (plain values: a move swaps them as one)
        int w = 0, n = 0;               // frames of the window / ticks the ring holds
        char *pool = nullptr;
        float *ring_h = nullptr, *ring_bits = nullptr, *r_h = nullptr, *r_bits = nullptr, *r_sel = nullptr, *r_codes = nullptr;
        uint8_t *ring_pk = nullptr, *ring_pr = nullptr, *r_pk = nullptr, *r_pr = nullptr;
        uint8_t *h_present = nullptr, *d_hpresent = nullptr;    // host-mapped mirror of ring_pr: what `late` looks at (and marks)
        int *r_zero = nullptr;          // row_off of a replay: every (row, frame) of the compact batch belongs to a running stream
        long long hs = 0, pks = 0, prs = 0, bs = 0;
    };
    struct RepairWindow : RepairMem {
        struct RingTick { int64_t f0 = 0; int k = 0; bool valid = false; hipEvent_t ev = nullptr; };    // session frames [f0, f0 + k)
        struct LateReq { int row, slot, j; int64_t tick; unsigned char bytes[SC_LATE_BYTES]; };
        std::vector<RingTick> ring;     // slot of tick t: t % n
        std::vector<LateReq> late;      // taken since the last tick: the next tick applies them
        RepairWindow() = default;
        RepairWindow(RepairWindow &&o) noexcept { swap(o); }
        RepairWindow &operator=(RepairWindow &&o) noexcept { swap(o); return *this; }     // o leaves with what this held, and releases it
        void swap(RepairWindow &o) noexcept { std::swap<RepairMem>(*this, o); ring.swap(o.ring); late.swap(o.late); }
        // forgets what the ring holds (set_conceal, set_repair: a frame is replayed by the program that first decoded it, or not at all)
        void clear() { for (auto &t : ring) t.valid = false; late.clear(); }
        ~RepairWindow() {
            for (auto &t : ring) if (t.ev) (void)hipEventDestroy(t.ev);
            if (pool) (void)hipFree(pool);
            if (h_present) (void)hipHostFree(h_present);
        }
    };
    RepairWindow rep;
    bool tick_retained(const RepairWindow::RingTick &t) const { return t.valid && t.f0 + t.k > frames - rep.w; }
    // sessions that choose their own rates and / or speak the wire with a bit count per frame (bvc_stream_codec_create_vbr).  SEND and
    // DUPLEX: a slot's `bits` and `bitsbuf` hold the slot's TARGET (the (B, k) layouts are what run_encode_vbr reads as tau), the tick's
    // bit counts go to vbits (B, k), and from there to last_bits / sizes (B, kmax); tok (B) are the rows' buckets.  RECV: the unpack reads
    // each frame's header, `bits` stays the count a lost frame is concealed with.
    bool vbr = false;
    bool choosing() const { return vbr && dir != BVC_STREAM_RECV; }
    int K = 0, ladder[VBR_MAX_RUNGS] = {};
    int rate_q8 = 0, burst_q8 = -1;     // burst_q8 < 0: no cap
    char *vws = nullptr;                // the candidates' frame buffers (carve_vbr), apart from the ordinary workspace `ws`
    float *vbits = nullptr, *last_bits = nullptr;
    int *sizes = nullptr, *tok = nullptr;
    bool use_graph = true;
    bool tick_flow = true;      // the ticks' recurrences on the persistent kernel where it is available (BVC_STREAM_FLOW=0: never)
    ~bvc_stream_codec() {
        for (auto &gc : graph) for (auto &gk : gc) for (auto g : gk) if (g) (void)hipGraphExecDestroy(g);
        if (voc) bvc_vocoder_stream_destroy(voc);
        if (pool) (void)hipFree(pool);
    }
};

namespace {

// Where a stream that joins a running session starts.  `samples` = samples per row the session has taken so far (ticks * hop_samples).
// Frame f reads samples [hop f - pad, hop f - pad + n_fft), so the tick that completes it is the first whose samples reach
// hop f - pad + n_fft.  The stream's sample 0 must be a session frame boundary hop * f0 not before its arrival; f0 is made the FIRST frame
// of its tick, so that the row's reset lies between two ticks: the smallest such f0 >= ceil(samples / hop).  delay = hop * f0 - samples.
// (bvcodec.streaming.join_plan is the same arithmetic; tests/test_stream_slots_cpu.py checks it against a simulation of the schedule.)
int64_t tick_of_frame(int64_t f, int hop_samples, const bvc_config &c) {
    const int64_t need = c.hop * f - c.pad_left + c.n_fft;
    return (need + hop_samples - 1) / hop_samples - 1;
}
void join_plan(int64_t samples, int hop_samples, const bvc_config &c, int *delay, int64_t *frame0, int64_t *tick0) {
    int64_t f = (samples + c.hop - 1) / c.hop;
    while (f > 0 && tick_of_frame(f - 1, hop_samples, c) == tick_of_frame(f, hop_samples, c)) ++f;
    *delay = (int)(c.hop * f - samples);
    *frame0 = f;
    if (tick0) *tick0 = tick_of_frame(f, hop_samples, c);
}

// Items 0 .. n - 1 to the device in lists of up to SC_LIST entries.  fill(l, i) adds item i's entry to l, or none, and does the host's
// bookkeeping for it; it returns BVC_OK, an error code, or LIST_DONE when no later item has an entry.  launch(l, first) sends a full
// list, or the last partial one; `first` entries went in the launches before it.  Stops at the first error code.
const int LIST_DONE = 1;
template <class List, class Fill, class Launch>
int send_lists(int n, Fill fill, Launch launch) {
    List l;
    l.n = 0;
    int first = 0;
    auto flush = [&]() -> int {
        if (l.n == 0) return BVC_OK;
        launch(l, first);
        BVC_HIP_TRY(hipGetLastError());
        first += l.n;
        l.n = 0;
        return BVC_OK;
    };
    for (int i = 0; i < n; ++i) {
        int rc = fill(l, i);
        if (rc == LIST_DONE) break;
        if (rc || (l.n == SC_LIST && (rc = flush()))) return rc;
    }
    return flush();
}

// pending slot changes -> device, in one launch per SC_LIST slots (before the tick's append)
int stream_send_pending(bvc_stream_codec *st, hipStream_t s) {
    const int rc = send_lists<SlotUpdateList>(st->B, [&](SlotUpdateList &l, int b) -> int {
        if (st->n_pending <= 0) return LIST_DONE;
        bvc_stream_codec::Slot &sl = st->slots[b];
        if (!sl.pending) return BVC_OK;
        l.e[l.n++] = SlotUpdate{b, sl.open ? sl.delay : -1, st->sbuf ? sl.pending : (sl.pending & ~SC_ZERO_TAIL), sl.bits};   // (a receive session has no samples)
        sl.pending = 0;
        --st->n_pending;
        return BVC_OK;
    }, [&](const SlotUpdateList &l, int) {
        sc_slot_update_kernel<<<dim3(l.n), 256, 0, s>>>(l, st->d_state, st->row_off, st->sbuf, st->cap, st->bitsbuf, st->B, st->kmax);
    });
    if (!rc) st->n_pending = 0;                              // (every pending slot has been visited: a guard against a miscount)
    return rc;
}

// the rows whose frame 0 is the first frame of this tick (frames [f_begin, f_begin + k)): per-row reset, after the append
int stream_start_rows(bvc_stream_codec *st, int64_t f_begin, int k, hipStream_t s) {
    const bvc_config &c = st->m->cfg;
    const bvc_vocoder_stream *v = st->voc;
    // the halves the session runs.  With a decoder half one blockIdx.y per generator tensor and one more; a send session has no generator
    // (voc is null exactly there: bvc_stream_codec_create_dir makes it for the decoder half): n_ten = 0 and a grid of its own.  The
    // pointers of a half that is not there are null in the session already, and a receive session's cap is 0.
    const bool enc = st->dir != BVC_STREAM_RECV;
    const int n_ten = v ? v->n_ten : 0;
    const unsigned gx = v ? (unsigned)std::max(1, std::min(16, (v->max_hc4 + 255) / 256)) : 4u;
    return send_lists<SlotRowList>(st->B, [&](SlotRowList &l, int b) -> int {
        if (st->n_waiting <= 0) return LIST_DONE;
        bvc_stream_codec::Slot &sl = st->slots[b];
        if (!sl.open || sl.started || sl.frame0 >= f_begin + k) return BVC_OK;
        if (sl.frame0 != f_begin) { set_error("bvc_stream_codec_tick: slot %d starts inside a tick (frame %lld of %lld+%d)", b, (long long)sl.frame0, (long long)f_begin, k); return BVC_EINVAL; }
        sl.started = true;
        --st->n_waiting;
        l.row[l.n++] = b;
        return BVC_OK;
    }, [&](const SlotRowList &l, int) {
        sc_slot_start_kernel<<<dim3(gx, (unsigned)n_ten + 1, (unsigned)l.n), 256, 0, s>>>(
            l, v ? v->d_tab : nullptr, n_ten, v && v->slide ? v->cursor : 0, st->sbuf, st->cap, enc ? c.pad_left : 0, st->h_enc, st->h_dec,
            c.h_dim, st->age);
        if (st->choosing() && st->burst_q8 >= 0) sc_tok_start_kernel<<<1, SC_LIST, 0, s>>>(l, st->tok, st->burst_q8);
    });
}

// the rows whose stream ends with the hop this tick has just appended (bvc_stream_codec_finish): right reflect padding behind the last
// sample, the row drains from here on.  One launch per SC_LIST rows, only in such a tick.
int stream_finish_rows(bvc_stream_codec *st, hipStream_t s) {
    const bvc_config &c = st->m->cfg;
    const int rc = send_lists<SlotUpdateList>(st->B, [&](SlotUpdateList &l, int b) -> int {
        if (st->n_finishing <= 0) return LIST_DONE;
        bvc_stream_codec::Slot &sl = st->slots[b];
        if (sl.fin_last < 0) return BVC_OK;
        // n samples in all -> bvc_num_frames(n) = n / hop frames, the same as the offline call
        const int64_t n = (st->ticks - sl.open_tick) * st->hop + sl.fin_last;
        sl.end_frame = sl.frame0 + n / c.hop;
        l.e[l.n++] = SlotUpdate{b, sl.fin_last, 0, 0.0f};
        sl.fin_last = -1;
        --st->n_finishing;
        return BVC_OK;
    }, [&](const SlotUpdateList &l, int) {
        sc_finish_kernel<<<dim3(l.n), 256, 0, s>>>(l, st->d_state, st->row_off, st->sbuf, st->cap, c.n_fft - c.hop - c.pad_left);
    });
    if (!rc) st->n_finishing = 0;
    return rc;
}

// the decode half of a tick, or of a tick that a replay decodes again: k frames of B rows from state h to state h, the mel frames to
// melhat.  A session that conceals generates the frames that `sel` marks and writes what it filled in back into `codes`.  (check_ws only
// adds up offsets on the host, the same ones for the same (B, k): a tick that has laid its workspace out already pays that sum twice.)
int decode_frames(bvc_stream_codec *st, int B, int k, float *codes, const float *sel, float *h, hipStream_t s) {
    Workspace w;
    if (int rc = check_ws(st->m, B, k, st->ws, st->ws_bytes, &w)) return rc;
    if (st->conceal) return run_decode_conceal(st->m, w, st->ws, codes, sel, h, B, k, st->melhat, h, codes, nullptr, s);
    return run_decode(st->m, w, st->ws, codes, h, B, k, st->melhat, h, s);
}

// the encode half of a tick of a session that chooses its own rates: every row's rungs tried inside the frame against the row's target
// (its (B, k) layout in bitsbuf) and bucket, state h_enc to h_enc; then one launch for the wire (a send session: a duplex one has no
// packet buffer), the bytes worth sending and the bit counts of the tick
int encode_frames_vbr(bvc_stream_codec *st, const Workspace &w, int k, hipStream_t s) {
    const bvc_model *m = st->m;
    VbrWorkspace v;
    carve_vbr(m, st->B, st->K, st->vws, &v);
    const VbrCap cap{st->burst_q8 >= 0, st->rate_q8, st->burst_q8, st->tok, st->tok};
    if (int rc = run_encode_vbr(m, w, v, st->ws, st->mel, st->bits_of(k), st->ladder, st->K, st->h_enc, st->B, k, st->codes, st->vbits, nullptr,
                                st->h_enc, nullptr, nullptr, nullptr, s, &cap)) return rc;
    return launch_pack_rows_vbr(st->codes, st->vbits, st->B, k, m->cfg.z_dim, st->kmax, st->packets, st->sizes, st->last_bits, s);
}

// the launches of one tick with k new frames (k > 0), in stream order
int stream_tick_body(bvc_stream_codec *st, int k, hipStream_t s) {
    const bvc_model *m = st->m;
    const int B = st->B;
    int rc;
    Workspace w;
    if ((rc = check_ws(m, B, k, st->ws, st->ws_bytes, &w))) return rc;
    if (st->dir == BVC_STREAM_RECV) {
        // the wire -> codes: every row's own bit count, 0.5 for what did not arrive and for idle rows
        // (the wire with a bit count per frame: the count is the frame's header, a frame that is not there is a frame of no bits)
        if (st->vbr) rc = launch_unpack_rows_vbr(st->packets, st->present, st->row_off, B, k, m->cfg.z_dim, st->kmax, st->codes, st->last_bits, s);
        else rc = launch_unpack_rows(st->packets, st->present, st->tick_bits(k), st->row_off, B, k, m->cfg.z_dim, st->kmax, st->codes, s);
        if (rc) return rc;
        // lost frames of open rows are generated with the row's bit count (all z bits on a fixed-rate model); idle rows keep their 0.5
        if (st->conceal && (rc = launch_conceal_select(st->present, st->kmax, st->tick_bits(k), (float)m->cfg.z_dim, st->row_off, B, k, w.bits, s))) return rc;
    } else {
        // front-end on the sample buffer: frame j of this tick reads sbuf[:, 256 j : 256 j + 1024)
        if ((rc = launch_stft_logmel(m->fe, st->sbuf, B, st->cap, k, 0, st->scale, st->mel, s))) return rc;
        // drop the 256 k samples no later frame reads (through a scratch copy: the ranges overlap)
        const int keep = st->cap - 256 * k;
        sc_shift_kernel<<<dim3((unsigned)((keep + 255) / 256), B), 256, 0, s>>>(st->sbuf, st->cap, 256 * k, st->stmp, st->cap, keep);
        sc_shift_kernel<<<dim3((unsigned)((keep + 255) / 256), B), 256, 0, s>>>(st->stmp, st->cap, 0, st->sbuf, st->cap, keep);
        BVC_HIP_TRY(hipGetLastError());
        if (st->choosing()) {
            if ((rc = encode_frames_vbr(st, w, k, s))) return rc;
            if (st->dir == BVC_STREAM_SEND) return BVC_OK;
        } else {
            if ((rc = run_encode(m, w, st->ws, st->mel, st->tick_bits(k), st->h_enc, B, k, st->codes, nullptr, st->h_enc, nullptr, s))) return rc;
            if (st->dir == BVC_STREAM_SEND)                  // codes -> the wire, and that is the tick
                return launch_pack_rows(st->codes, st->tick_bits(k), B, k, m->cfg.z_dim, st->kmax, st->packets, s);
        }
    }
    if ((rc = decode_frames(st, B, k, st->codes, w.bits, st->h_dec, s))) return rc;
    return bvc_vocoder_stream_push(st->voc, st->melhat, k, st->out_div, st->wav, s);
}

int slot_arg(bvc_stream_codec *st, int32_t slot, const char *fn) {
    if (!st) { set_error("%s: null stream codec", fn); return BVC_EINVAL; }
    if (slot < 0 || slot >= st->B) { set_error("%s: slot %d outside 0..%d", fn, (int)slot, st->B - 1); return BVC_EINVAL; }
    return BVC_OK;
}
void slot_mark(bvc_stream_codec *st, bvc_stream_codec::Slot &sl, int flags) {
    if (!sl.pending) ++st->n_pending;
    sl.pending |= flags;
}

// one tick's body with k > 0 frames on the session's schedule: launched eagerly, or replayed from the hipGraph of its (k, vocoder parity)
int stream_run_body(bvc_stream_codec *st, int k, hipStream_t s) {
    const int B = st->B;
    int rc = BVC_OK;
    const int parity = st->voc ? st->voc->parity : 0;
    const bool slide = st->voc && st->voc->slide;
    // Which schedule?  Where the persistent recurrence kernel is available (flow_chains_static: the model's option, the
    // residency census, the batch) the tick is launched eagerly and its two recurrences are one persistent launch each - at 256
    // streams 1.53 ms per tick against 1.69 ms for the launch-per-layer recurrence, which gains nothing from a graph on the GPU
    // side (1.68 eager / 1.70 replayed; the replay only saves host time).  Otherwise (recurrence = layers, no resident grid,
    // BVC_STREAM_FLOW=0) the warm tick is one hipGraph of launch-per-layer kernels as before.  Same bits either way.
    const bool tick_flow = st->tick_flow && flow_chains_static(st->m, B) != 0;
    const bool warm = !tick_flow && !slide && st->use_graph && s != nullptr && st->frames >= STREAM_WARM_FRAMES;     // (the default stream cannot be captured)
    TickFlags flags(tick_flow);
    if (!warm) {
        rc = stream_tick_body(st, k, s);
    } else {
        hipGraphExec_t &ge = st->graph[st->conceal][k][parity];
        if (!ge) {                                       // first warm tick of this shape: capture it (the capture does not execute)
            hipGraph_t graph = nullptr;
            const int vp = parity; const int64_t vf = st->voc ? st->voc->frames : 0;
            g_capturing = true;
            hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) rc = stream_tick_body(st, k, s);
            hipError_t e2 = (e == hipSuccess) ? hipStreamEndCapture(s, &graph) : e;
            g_capturing = false;
            if (st->voc) { st->voc->parity = vp; st->voc->frames = vf; }  // the captured push advanced the host-side bookkeeping: undo, the replay redoes it
            if (!rc && (e2 != hipSuccess || !graph)) { set_error("bvc_stream_codec_tick: hipGraph capture failed: %s", hipGetErrorString(e2)); rc = BVC_EHIP; }
            if (!rc && hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0) != hipSuccess) { set_error("bvc_stream_codec_tick: hipGraphInstantiate failed"); rc = BVC_EHIP; }
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (!rc) {
            if (hipGraphLaunch(ge, s) != hipSuccess) { set_error("bvc_stream_codec_tick: hipGraphLaunch failed"); rc = BVC_EHIP; }
            if (st->voc) { st->voc->parity ^= 1; st->voc->frames += k; }  // what stream_push() does on the host side
        }
    }
    return rc;
}

// ---- repair window, host side ----
// a receive tick of a session with a window, behind stream_start_rows and outside the tick's body (a graph tick replays unchanged; the ring
// position is an argument): the state in front of the tick and what the tick reads.  The event tells `late` when the host mirror is there.
int stream_snapshot(bvc_stream_codec *st, int k, hipStream_t s) {
    bvc_stream_codec::RepairWindow &rw = st->rep;
    const int B = st->B, r = (int)(st->ticks % rw.n);
    auto &t = rw.ring[r];
    t.f0 = st->frames; t.k = k; t.valid = true;
    const long long n_h4 = (long long)B * st->m->cfg.h_dim / 4, n_pk = (long long)B * st->kmax * st->bpf, n_pr = (long long)B * st->kmax;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(1024, (n_h4 + 255) / 256));
    sc_snapshot_kernel<<<dim3(grid), 256, 0, s>>>(st->h_dec, n_h4, rw.ring_h + r * rw.hs, st->packets, n_pk, rw.ring_pk + r * rw.pks, st->present, n_pr,
                                                  rw.ring_pr + r * rw.prs, rw.d_hpresent + r * rw.prs, st->bits_of(k), rw.ring_bits + r * rw.bs, B, k,
                                                  st->kmax);
    BVC_HIP_TRY(hipGetLastError());
    BVC_HIP_TRY(hipEventRecord(t.ev, s));
    return BVC_OK;
}

// Head of a receive tick, outside any graph: the late packets taken since the last tick go into the ring, and every row that got one is
// decoded again from the snapshot in front of its earliest late frame up to now, tick by tick as the session's ticks did it (the same
// launches on (B', k) of the ring's bytes, present marks and bits per frame - a row decodes to the same bits alone or in a batch, a tick
// to the same bits whatever came in one call before it).  Rows with the same first tick form one pass.  Behind every tick of a pass the
// rows' states go into the next tick's snapshot (a later late packet of the row then starts from a repaired state), behind the last
// into h_dec.  The mel frames go to melhat, which the tick overwrites; the filled codes stay in the replay's own buffer.
// (bvcodec.streaming.repair_plan states the same acceptance and pass arithmetic.)
int stream_apply_late(bvc_stream_codec *st, hipStream_t s) {
    const bvc_model *m = st->m;
    const bvc_config &c = m->cfg;
    bvc_stream_codec::RepairWindow &rw = st->rep;
    const int B = st->B;
    int rc = send_lists<LateList>((int)rw.late.size(), [&](LateList &l, int i) -> int {
        const auto &q = rw.late[i];
        LateEntry &e = l.e[l.n++];
        e.row = q.row; e.slot = q.slot; e.j = q.j; e.pad_ = 0;
        memcpy(e.bytes, q.bytes, SC_LATE_BYTES);
        return BVC_OK;
    }, [&](const LateList &l, int) { sc_late_patch_kernel<<<dim3(l.n), 64, 0, s>>>(l, rw.ring_pk, rw.pks, rw.ring_pr, rw.prs, st->kmax, st->bpf); });
    if (rc) return rc;
    // every row's first tick, and the passes: oldest first (their rows are disjoint, the order does not matter to the result)
    std::vector<int64_t> first(B, -1);
    for (const auto &q : rw.late) if (first[q.row] < 0 || q.tick < first[q.row]) first[q.row] = q.tick;
    rw.late.clear();
    std::vector<int64_t> starts;
    for (int b = 0; b < B; ++b) if (first[b] >= 0) starts.push_back(first[b]);
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    for (int64_t t0 : starts) {
        std::vector<int> rows;
        for (int b = 0; b < B; ++b) if (first[b] == t0) rows.push_back(b);
        const int Bp = (int)rows.size(), n_chunks = (int)(st->ticks - t0);
        if (n_chunks < 1 || n_chunks > SC_CHUNKS || n_chunks > rw.n) { set_error("bvc_stream_codec_tick_recv: internal replay span %d", n_chunks); return BVC_EINVAL; }
        ReplayPlan p;
        p.n_chunks = n_chunks; p.pad_ = 0;
        int frames = 0;
        for (int i = 0; i < n_chunks; ++i) {
            const int r = (int)((t0 + i) % rw.n);
            if (!rw.ring[r].valid) { set_error("bvc_stream_codec_tick_recv: internal replay through a tick that is not retained"); return BVC_EINVAL; }
            p.c[i] = ReplayChunk{r, rw.ring[r].k, Bp * frames};
            frames += rw.ring[r].k;
        }
        if (frames > rw.w + st->kmax - 1) { set_error("bvc_stream_codec_tick_recv: internal replay length %d", frames); return BVC_EINVAL; }
        // the pass's rows in groups of SC_LIST: row0 is the group's first compact row
        auto put_row = [&](SlotRowList &l, int i) -> int { l.row[l.n++] = rows[i]; return BVC_OK; };
        if ((rc = send_lists<SlotRowList>(Bp, put_row, [&](const SlotRowList &l, int row0) {
                p.row0 = row0; p.n_rows = l.n;
                std::copy(l.row, l.row + l.n, p.row);
                sc_replay_gather_kernel<<<dim3((unsigned)n_chunks, (unsigned)l.n), 256, 0, s>>>(
                    p, rw.ring_h, rw.hs, rw.ring_pk, rw.pks, rw.ring_pr, rw.prs, rw.ring_bits, rw.bs, c.h_dim, st->kmax, st->bpf, rw.r_h, rw.r_pk,
                    rw.r_pr, rw.r_bits);
            }))) return rc;
        // every (row, frame) of the pass is a row of one frame to these two: the ring's bits per frame, not the slots' current ones
        const int N = Bp * frames;
        const float *bits = c.var_bit ? rw.r_bits : nullptr;
        if ((rc = launch_unpack_rows(rw.r_pk, rw.r_pr, bits, rw.r_zero, N, 1, c.z_dim, 1, rw.r_codes, s))) return rc;
        if (st->conceal && (rc = launch_conceal_select(rw.r_pr, 1, bits, (float)c.z_dim, nullptr, N, 1, rw.r_sel, s))) return rc;
        TickFlags flags(st->tick_flow && flow_chains_static(m, Bp) != 0);
        for (int i = 0; i < n_chunks; ++i) {
            if ((rc = decode_frames(st, Bp, p.c[i].k, rw.r_codes + (size_t)p.c[i].off * c.z_dim, rw.r_sel + p.c[i].off, rw.r_h, s))) return rc;
            float *dst = i + 1 < n_chunks ? rw.ring_h + p.c[i + 1].slot * rw.hs : st->h_dec;
            rc = send_lists<SlotRowList>(Bp, put_row, [&](const SlotRowList &l, int row0) {
                sc_replay_scatter_kernel<<<dim3((unsigned)l.n), 256, 0, s>>>(l, row0, rw.r_h, dst, c.h_dim);
            });
            if (rc) { set_error("bvc_stream_codec_tick_recv: the replay's scatter launch failed"); return rc; }
        }
    }
    return BVC_OK;
}

// The tail of a tick of k frames: the fill level and the rows' ages on the device, what bvc_stream_codec_slot_frames answers, the
// session's counts.  The slot loop is written for a send-side tick; a receive tick has k > 0 and no slot that drains (finish is refused
// there, end_frame stays -1), with which it comes to last_count = k and last_frame0 = frames - frame0 for every running stream.
int end_tick(bvc_stream_codec *st, int k, int fill_delta, hipStream_t s) {
    sc_advance_kernel<<<1, 64, 0, s>>>(st->d_state, fill_delta, st->age, st->B, k, (int)STREAM_WARM_FRAMES);
    BVC_HIP_TRY(hipGetLastError());
    for (auto &sl : st->slots) {
        const bool live = sl.open && sl.started && k > 0;
        sl.last_count = live ? k : 0;
        sl.last_frame0 = live ? st->frames - sl.frame0 : 0;
        if (sl.end_frame < 0) continue;
        // a draining stream: only the frames below its end are its own, and with the last of them the row is idle of its own accord
        // (what a close does: the next tick clears what the row still holds)
        if (st->frames + sl.last_count > sl.end_frame) sl.last_count = (int)(sl.end_frame - st->frames);
        if (st->frames + k >= sl.end_frame) {
            sl.open = false; sl.started = false; sl.delay = 0; sl.end_frame = -1;
            slot_mark(st, sl, SC_SET_OFF | SC_ZERO_TAIL);
        }
    }
    st->frames += k;
    st->ticks += 1;
    return BVC_OK;
}

// one device allocation cut into regions, each 256-byte aligned: take() while the sizes are added up, at<T>() once there is a base
struct PoolLayout {
    size_t bytes = 0;
    size_t take(size_t n) { const size_t o = bytes; bytes += (n + 255) & ~(size_t)255; return o; }
    template <class T> static T *at(char *base, size_t off) { return reinterpret_cast<T *>(base + off); }
};

}  // namespace

extern "C" {

int bvc_stream_codec_create(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale,
                            float out_scale_div, bvc_stream_codec **out) {
    return bvc_stream_codec_create_dir(m, B, hop_samples, bits_per_frame, scale, out_scale_div, BVC_STREAM_DUPLEX, out);
}

// what bvc_stream_codec_create_vbr adds to a session (checked by it); null: the fixed wire, rates set by the caller
struct VbrSession { const int32_t *ladder; int K; float target; int rate_q8, burst_q8; };
static int stream_codec_create(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale, float out_scale_div,
                               int32_t direction, const VbrSession *vs, bvc_stream_codec **out);

int bvc_stream_codec_create_dir(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale,
                                float out_scale_div, int32_t direction, bvc_stream_codec **out) {
    return stream_codec_create(m, B, hop_samples, bits_per_frame, scale, out_scale_div, direction, nullptr, out);
}

int bvc_stream_codec_create_vbr(const bvc_model *m, int32_t B, int32_t hop_samples, const int32_t *h_ladder, int32_t K, float target,
                                int32_t rate_q8, int32_t burst_q8, float bits_per_frame, float scale, float out_scale_div, int32_t direction,
                                bvc_stream_codec **out) {
    const char *fn = "bvc_stream_codec_create_vbr";
    if (!m || !out) { set_error("%s: bad arguments", fn); return BVC_EINVAL; }
    if (!m->cfg.var_bit) { set_error("%s: a fixed-rate model (var_bit = 0) has no bit mask to choose", fn); return BVC_EINVAL; }
    if (m->cfg.z_dim > 255) { set_error("%s: the bit count of a frame is one byte: z_dim <= 255", fn); return BVC_EINVAL; }
    VbrSession vs{h_ladder, K, target, rate_q8, burst_q8};
    if (direction == BVC_STREAM_RECV) {
        if (h_ladder || K != 0) { set_error("%s: a receive session takes no ladder (NULL, 0)", fn); return BVC_EINVAL; }
        if (!(bits_per_frame >= 0.0f)) { set_error("%s: bits per frame must not be negative", fn); return BVC_EINVAL; }
        vs.burst_q8 = -1;
    } else {
        if (!h_ladder || K < 1 || K > VBR_MAX_RUNGS) { set_error("%s: the ladder takes 1 to %d rungs (K=%d)", fn, VBR_MAX_RUNGS, (int)K); return BVC_EINVAL; }
        for (int k = 0; k < K; ++k)
            if (h_ladder[k] < 0 || h_ladder[k] > m->cfg.z_dim || (k && h_ladder[k] <= h_ladder[k - 1])) {
                set_error("%s: rung %d = %d: bit counts in [0, %d], strictly ascending", fn, k, (int)h_ladder[k], m->cfg.z_dim);
                return BVC_EINVAL;
            }
        if (burst_q8 >= 0 && (rate_q8 < 0 || (long long)burst_q8 < (long long)h_ladder[0] * 256)) {
            set_error("%s: rate_q8 = %d must not be negative, and a bucket of %d/256 bits must hold rung 0 (%d bits)", fn, (int)rate_q8, (int)burst_q8, (int)h_ladder[0]);
            return BVC_EINVAL;
        }
        if (burst_q8 < 0) vs.burst_q8 = -1;
        bits_per_frame = target;                             // what a slot's `bits` holds in such a session
    }
    return stream_codec_create(m, B, hop_samples, bits_per_frame, scale, out_scale_div, direction, &vs, out);
}

static int stream_codec_create(const bvc_model *m, int32_t B, int32_t hop_samples, float bits_per_frame, float scale, float out_scale_div,
                               int32_t direction, const VbrSession *vs, bvc_stream_codec **out) {
    if (direction != BVC_STREAM_DUPLEX && direction != BVC_STREAM_SEND && direction != BVC_STREAM_RECV) {
        set_error("bvc_stream_codec_create_dir: direction %d is none of BVC_STREAM_DUPLEX / _SEND / _RECV", (int)direction); return BVC_EINVAL;
    }
    const bool enc = direction != BVC_STREAM_RECV, dec = direction != BVC_STREAM_SEND;
    if (!enc) hop_samples = 0;                               // a receive tick is given whole frames
    if (!m || !out || B <= 0 || (enc && hop_samples <= 0)) { set_error("bvc_stream_codec_create: bad arguments"); return BVC_EINVAL; }
    if (dec && m->noncausal) { set_error("bvc_stream_codec_create: %s", not_causal(m)); return BVC_EINVAL; }
    const bvc_config &c = m->cfg;
    if (enc && hop_samples <= c.pad_left) { set_error("bvc_stream_codec_create: the hop must exceed the left reflect padding (%d samples)", c.pad_left); return BVC_EINVAL; }
    std::unique_ptr<bvc_stream_codec> st(new bvc_stream_codec());
    st->m = m; st->B = B; st->hop = hop_samples; st->bits = bits_per_frame; st->scale = scale; st->out_div = out_scale_div;
    st->dir = direction; st->bpf = (c.z_dim + 7) / 8;
    size_t vws_bytes = 0;
    if (vs) {
        st->vbr = true; st->bpf = 1 + (c.z_dim + 7) / 8;     // a frame's bit count in front of its bytes
        st->K = enc ? vs->K : 0; st->rate_q8 = vs->rate_q8; st->burst_q8 = vs->burst_q8;
        for (int k = 0; k < st->K; ++k) st->ladder[k] = vs->ladder[k];
        if (enc) { VbrWorkspace v; carve_vbr(m, B, st->K, nullptr, &v); vws_bytes = v.total; }
    }
    // a receive tick takes up to 7 frames: whatever one tick of a send session emits (its own limit, the size of the graph table)
    st->kmax = enc ? (hop_samples + c.hop - 1) / c.hop + 1 : 7;
    if (st->kmax > 7) { set_error("bvc_stream_codec_create: hop too long (%d frames per tick)", st->kmax); return BVC_EINVAL; }
    // the longest delay a joining stream can get (join_plan): the pattern of frames per tick repeats after hop / gcd(hop, hop_samples) ticks
    for (int64_t t = 0; enc && t <= c.hop; ++t) {
        int d; int64_t f0;
        join_plan(t * hop_samples, hop_samples, c, &d, &f0, nullptr);
        st->max_delay = std::max(st->max_delay, d);
    }
    // room for the window, the frames of a tick, a hop behind the longest delay - and with it for the right reflect padding of a stream
    // that ends (bvc_stream_codec_finish): it ends at most fill + max_delay + hop_samples with fill < n_fft, and the n_fft - hop - pad_left
    // = 512 samples behind that are within the hop * kmax >= 512 counted here
    st->cap = enc ? c.n_fft + c.hop * st->kmax + hop_samples + st->max_delay : 0;
    st->ws_bytes = bvc_workspace_bytes(m, B, st->kmax);
    int spf = 1;                                             // samples per frame
    for (int i = 0; i < c.n_up; ++i) spf *= c.up_rates[i];
    PoolLayout pl;
    // (a half that the session does not run gets no memory: its pointers stay null)
    const size_t one = enc ? 1 : 0, two = dec ? 1 : 0, wire = direction != BVC_STREAM_DUPLEX ? 1 : 0;
    const size_t o_state = pl.take(sizeof(StreamDev)), o_in = pl.take(one * B * hop_samples * 4), o_sbuf = pl.take(one * B * st->cap * 4),
                 o_stmp = pl.take(one * B * st->cap * 4), o_mel = pl.take(one * B * st->kmax * c.num_mels * 4),
                 o_bits = pl.take((size_t)B * (st->kmax * (st->kmax + 1) / 2) * 4), o_rowoff = pl.take((size_t)B * 4), o_age = pl.take((size_t)B * 4), o_codes = pl.take((size_t)B * st->kmax * c.z_dim * 4),
                 o_melhat = pl.take(two * B * st->kmax * c.num_mels * 4), o_wav = pl.take(two * B * st->kmax * spf * 4),
                 o_he = pl.take(one * B * c.h_dim * 4), o_hd = pl.take(two * B * c.h_dim * 4), o_ws = pl.take(st->ws_bytes),
                 o_pk = pl.take(wire * B * st->kmax * st->bpf), o_pr = pl.take(wire * B * st->kmax);
    const size_t vb = vs ? 1 : 0;
    const size_t o_vws = pl.take(vws_bytes), o_vbits = pl.take(vb * B * st->kmax * 4), o_lbits = pl.take(vb * B * st->kmax * 4),
                 o_sizes = pl.take(vb * B * st->kmax * 4), o_tok = pl.take(vb * B * 4);
    if (hipMalloc(reinterpret_cast<void **>(&st->pool), pl.bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("bvc_stream_codec_create: cannot allocate %zu bytes", pl.bytes);
        return BVC_ENOMEM;
    }
    BVC_HIP_TRY(hipMemset(st->pool, 0, pl.bytes));
    char *p = st->pool;
    st->d_state = pl.at<StreamDev>(p, o_state);
    st->bitsbuf = pl.at<float>(p, o_bits); st->codes = pl.at<float>(p, o_codes); st->ws = p + o_ws;
    if (enc) {
        st->d_in = pl.at<float>(p, o_in); st->sbuf = pl.at<float>(p, o_sbuf); st->stmp = pl.at<float>(p, o_stmp);
        st->mel = pl.at<float>(p, o_mel); st->h_enc = pl.at<float>(p, o_he);
    }
    if (dec) { st->melhat = pl.at<float>(p, o_melhat); st->wav = pl.at<float>(p, o_wav); st->h_dec = pl.at<float>(p, o_hd); }
    if (wire) { st->packets = pl.at<uint8_t>(p, o_pk); st->present = pl.at<uint8_t>(p, o_pr); }
    if (vs) {
        st->vws = p + o_vws; st->vbits = pl.at<float>(p, o_vbits); st->last_bits = pl.at<float>(p, o_lbits);
        st->sizes = pl.at<int>(p, o_sizes); st->tok = pl.at<int>(p, o_tok);
    }
    st->row_off = pl.at<int>(p, o_rowoff); st->age = pl.at<int>(p, o_age);          // zero: every slot open, delay 0, age 0
    st->slots.assign(B, bvc_stream_codec::Slot());
    for (auto &sl : st->slots) sl.bits = bits_per_frame;
    int rc;
    if ((rc = launch_fill(st->bitsbuf, bits_per_frame, (long long)B * (st->kmax * (st->kmax + 1) / 2), nullptr))) return rc;
    if (st->choosing() && st->burst_q8 >= 0 && (rc = launch_vbr_tok(st->tok, nullptr, st->burst_q8, B, nullptr))) return rc;   // full buckets
    st->fill = c.pad_left;                                   // room for the left reflect padding of frame 0
    StreamDev init{st->fill, {0, 0, 0}};
    BVC_HIP_TRY(hipMemcpy(st->d_state, &init, sizeof(init), hipMemcpyHostToDevice));
    { const char *ng = getenv("BVC_STREAM_NO_GRAPH"); st->use_graph = !(ng && ng[0] == '1'); }
    { const char *tf = getenv("BVC_STREAM_FLOW"); st->tick_flow = !(tf && tf[0] == '0'); }
    if (st->choosing()) st->tick_flow = false;               // the candidates are not in the persistent kernel: launch-per-layer ticks
    // ticks that are launched eagerly (persistent recurrence) let the generator's windows slide through their buffers instead of moving
    // every history back after every hop (56 us of a 1.5 ms tick at 256 streams); BVC_STREAM_SLIDE=0: never
    const char *sl = getenv("BVC_STREAM_SLIDE");
    const bool slide = st->tick_flow && flow_chains_static(m, B) != 0 && !(sl && sl[0] == '0');
    if (dec) {
        if ((rc = vocoder_stream_create(m, B, st->kmax, slide, &st->voc))) return rc;
        st->voc->d_age = st->age;
    }
    if (!enc) st->first = false;                             // no sample buffer, no left padding to write
    BVC_HIP_TRY(hipDeviceSynchronize());
    *out = st.release();
    return BVC_OK;
}

void bvc_stream_codec_destroy(bvc_stream_codec *st) { delete st; }

int bvc_stream_codec_buffers(bvc_stream_codec *st, float **d_in, float **d_codes, float **d_wav, int32_t *max_frames_per_tick) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (d_in) *d_in = st->d_in;
    if (d_codes) *d_codes = st->codes;
    if (d_wav) *d_wav = st->wav;
    if (max_frames_per_tick) *max_frames_per_tick = st->kmax;
    return BVC_OK;
}

int bvc_stream_codec_packets(bvc_stream_codec *st, uint8_t **d_packets, uint8_t **d_present, int32_t *bytes_per_frame) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (d_packets) *d_packets = st->packets;
    if (d_present) *d_present = st->present;
    if (bytes_per_frame) *bytes_per_frame = st->bpf;
    return BVC_OK;
}

int bvc_stream_codec_open(bvc_stream_codec *st, int32_t slot, float bits_per_frame, int32_t *delay_samples) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_open")) return rc;
    bvc_stream_codec::Slot &sl = st->slots[slot];
    if (sl.open) { set_error("bvc_stream_codec_open: slot %d is open", (int)slot); return BVC_EINVAL; }
    if (st->choosing()) bits_per_frame = st->bits;          // the session's default target (the argument is ignored); the bucket fills at frame 0
    else if (!(bits_per_frame >= 0.0f)) { set_error("bvc_stream_codec_open: bits per frame must not be negative"); return BVC_EINVAL; }
    if (st->dir == BVC_STREAM_RECV) { sl.delay = 0; sl.frame0 = st->frames; }     // frame-aligned: frame 0 is the first frame of the next tick
    else join_plan(st->ticks * st->hop, st->hop, st->m->cfg, &sl.delay, &sl.frame0, nullptr);
    sl.open = true; sl.started = false; sl.bits = bits_per_frame;
    sl.last_count = 0; sl.last_frame0 = 0;
    sl.open_tick = st->ticks; sl.fin_last = -1; sl.end_frame = -1;
    ++st->n_waiting;
    slot_mark(st, sl, SC_SET_OFF | SC_SET_BITS);
    if (delay_samples) *delay_samples = sl.delay;
    return BVC_OK;
}

int bvc_stream_codec_close(bvc_stream_codec *st, int32_t slot) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_close")) return rc;
    bvc_stream_codec::Slot &sl = st->slots[slot];
    if (!sl.open) { set_error("bvc_stream_codec_close: slot %d is idle", (int)slot); return BVC_EINVAL; }
    if (!sl.started) --st->n_waiting;
    if (sl.fin_last >= 0) --st->n_finishing;                 // a finish that no tick has carried out yet is dropped with the stream,
    sl.open = false; sl.started = false; sl.delay = 0;       // and so is the rest of a stream that drains
    sl.last_count = 0; sl.last_frame0 = 0;
    sl.fin_last = -1; sl.end_frame = -1;
    auto &late = st->rep.late;                               // late packets of the stream that no tick has applied go with it
    late.erase(std::remove_if(late.begin(), late.end(), [&](const bvc_stream_codec::RepairWindow::LateReq &q) { return q.row == slot; }), late.end());
    slot_mark(st, sl, SC_SET_OFF | SC_ZERO_TAIL);
    return BVC_OK;
}

int bvc_stream_codec_finish(bvc_stream_codec *st, int32_t slot, int32_t n_last) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_finish")) return rc;
    if (st->dir == BVC_STREAM_RECV) { set_error("bvc_stream_codec_finish: a receive session has no samples to flush (close the slot)"); return BVC_EINVAL; }
    bvc_stream_codec::Slot &sl = st->slots[slot];
    const bvc_config &c = st->m->cfg;
    if (!sl.open || !sl.started) { set_error("bvc_stream_codec_finish: slot %d is %s", (int)slot, sl.open ? "waiting for its frame 0" : "idle"); return BVC_EINVAL; }
    if (sl.fin_last >= 0 || sl.end_frame >= 0) { set_error("bvc_stream_codec_finish: slot %d is draining already", (int)slot); return BVC_EINVAL; }
    if (n_last < 0 || n_last > st->hop) { set_error("bvc_stream_codec_finish: n_last %d outside 0..%d", (int)n_last, st->hop); return BVC_EINVAL; }
    const int64_t n = (st->ticks - sl.open_tick) * st->hop + n_last;
    if (n <= c.n_fft - c.hop - c.pad_left) { set_error("bvc_stream_codec_finish: a stream of %lld samples is too short for the right reflect padding", (long long)n); return BVC_EINVAL; }
    sl.fin_last = n_last;
    ++st->n_finishing;
    return BVC_OK;
}

int bvc_stream_codec_slot_state(bvc_stream_codec *st, int32_t slot, int32_t *state) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_slot_state")) return rc;
    const bvc_stream_codec::Slot &sl = st->slots[slot];
    if (state) *state = !sl.open ? 0 : (!sl.started ? 1 : ((sl.fin_last >= 0 || sl.end_frame >= 0) ? 3 : 2));
    return BVC_OK;
}

int bvc_stream_codec_set_bits(bvc_stream_codec *st, int32_t slot, float bits_per_frame) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_set_bits")) return rc;
    if (!st->m->cfg.var_bit) { set_error("bvc_stream_codec_set_bits: the model has a fixed bitrate (var_bit = 0)"); return BVC_EINVAL; }
    if (st->choosing()) { set_error("bvc_stream_codec_set_bits: the session chooses its own rates (bvc_stream_codec_set_target)"); return BVC_EINVAL; }
    bvc_stream_codec::Slot &sl = st->slots[slot];
    if (!sl.open) { set_error("bvc_stream_codec_set_bits: slot %d is idle", (int)slot); return BVC_EINVAL; }
    if (!(bits_per_frame >= 0.0f)) { set_error("bvc_stream_codec_set_bits: bits per frame must not be negative"); return BVC_EINVAL; }
    sl.bits = bits_per_frame;
    slot_mark(st, sl, SC_SET_BITS);
    return BVC_OK;
}

int bvc_stream_codec_set_target(bvc_stream_codec *st, int32_t slot, float target) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_set_target")) return rc;
    if (!st->choosing()) { set_error("bvc_stream_codec_set_target: not a session that chooses its own rates (bvc_stream_codec_create_vbr, SEND or DUPLEX)"); return BVC_EINVAL; }
    bvc_stream_codec::Slot &sl = st->slots[slot];
    if (!sl.open) { set_error("bvc_stream_codec_set_target: slot %d is idle", (int)slot); return BVC_EINVAL; }
    sl.bits = target;                                        // (any float: +inf is rung 0, -inf or a NaN the top rung)
    slot_mark(st, sl, SC_SET_BITS);
    return BVC_OK;
}

int bvc_stream_codec_sizes(bvc_stream_codec *st, int32_t **d_sizes) {
    if (!st || !st->vbr) { set_error("bvc_stream_codec_sizes: not a session of bvc_stream_codec_create_vbr"); return BVC_EINVAL; }
    if (d_sizes) *d_sizes = st->sizes;
    return BVC_OK;
}

int bvc_stream_codec_bits(bvc_stream_codec *st, float **d_bits) {
    if (!st || !st->vbr) { set_error("bvc_stream_codec_bits: not a session of bvc_stream_codec_create_vbr"); return BVC_EINVAL; }
    if (d_bits) *d_bits = st->last_bits;
    return BVC_OK;
}

int bvc_stream_codec_slot_frames(bvc_stream_codec *st, int32_t slot, int32_t *first, int32_t *count, int64_t *stream_frame0) {
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_slot_frames")) return rc;
    const bvc_stream_codec::Slot &sl = st->slots[slot];
    if (first) *first = 0;                                   // a stream's frame 0 is the first frame of its tick
    if (count) *count = sl.last_count;
    if (stream_frame0) *stream_frame0 = sl.last_frame0;
    return BVC_OK;
}

int bvc_stream_codec_tick(bvc_stream_codec *st, int32_t *n_frames, void *stream) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (int st_ = sticky_status(st->m)) return st_;
    if (st->dir == BVC_STREAM_RECV) { set_error("bvc_stream_codec_tick: a receive session takes packets (bvc_stream_codec_tick_recv)"); return BVC_EINVAL; }
    const bvc_config &c = st->m->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int B = st->B;
    // the hop joins the sample buffer (device-side fill level), frame 0's left reflect padding once the first samples are there
    if (st->n_pending > 0) { if (int rc_ = stream_send_pending(st, s)) return rc_; }
    sc_append_kernel<<<dim3((unsigned)((st->hop + 255) / 256), B), 256, 0, s>>>(st->d_state, st->d_in, st->hop, st->sbuf, st->cap, st->row_off);
    if (st->first) {
        sc_reflect_left_kernel<<<dim3(B), 256, 0, s>>>(st->sbuf, st->cap, c.pad_left);
        st->first = false;
    }
    BVC_HIP_TRY(hipGetLastError());
    if (st->n_finishing > 0) { if (int rc_ = stream_finish_rows(st, s)) return rc_; }
    const int fill = st->fill + st->hop;
    const int k = fill >= c.n_fft ? (fill - c.n_fft) / c.hop + 1 : 0;
    if (k > st->kmax) { set_error("bvc_stream_codec_tick: internal frame count %d", k); return BVC_EINVAL; }
    int rc = BVC_OK;
    if (k > 0 && st->n_waiting > 0 && (rc = stream_start_rows(st, st->frames, k, s))) return rc;
    if (k > 0 && (rc = stream_run_body(st, k, s))) return rc;
    if ((rc = end_tick(st, k, st->hop - c.hop * k, s))) return rc;
    st->fill = fill - c.hop * k;
    if (n_frames) *n_frames = k;
    return BVC_OK;
}

int bvc_stream_codec_tick_recv(bvc_stream_codec *st, int32_t n_frames, void *stream) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (int st_ = sticky_status(st->m)) return st_;
    if (st->dir != BVC_STREAM_RECV) { set_error("bvc_stream_codec_tick_recv: not a receive session (bvc_stream_codec_tick)"); return BVC_EINVAL; }
    if (n_frames < 1 || n_frames > st->kmax) { set_error("bvc_stream_codec_tick_recv: n_frames %d outside 1..%d", (int)n_frames, st->kmax); return BVC_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int k = n_frames;
    int rc = BVC_OK;
    if (st->n_pending > 0 && (rc = stream_send_pending(st, s))) return rc;
    if (!st->rep.late.empty() && (rc = stream_apply_late(st, s))) return rc;
    if (st->n_waiting > 0 && (rc = stream_start_rows(st, st->frames, k, s))) return rc;
    if (st->rep.w > 0 && (rc = stream_snapshot(st, k, s))) return rc;
    if ((rc = stream_run_body(st, k, s))) return rc;
    return end_tick(st, k, 0, s);                            // (every row's age: the generator reads it)
}

int bvc_stream_codec_set_conceal(bvc_stream_codec *st, int32_t mode) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (int st_ = sticky_status(st->m)) return st_;
    if (st->dir != BVC_STREAM_RECV) { set_error("bvc_stream_codec_set_conceal: not a receive session"); return BVC_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("bvc_stream_codec_set_conceal: mode %d is neither 0 (no bits) nor 1 (prior)", (int)mode); return BVC_EINVAL; }
    if (int rc_ = need_prior(st->m, "bvc_stream_codec_set_conceal")) return rc_;
    st->conceal = mode;                                      // host bookkeeping: the next tick reads it
    st->rep.clear();                                         // the two programs agree only to rounding: no replay across the switch
    return BVC_OK;
}

int bvc_stream_codec_set_repair(bvc_stream_codec *st, int32_t window_frames) {
    if (!st) { set_error("null stream codec"); return BVC_EINVAL; }
    if (st->dir != BVC_STREAM_RECV) { set_error("bvc_stream_codec_set_repair: not a receive session"); return BVC_EINVAL; }
    if (st->vbr) { set_error("bvc_stream_codec_set_repair: the window's ring has the fixed wire's packet width (not a bvc_stream_codec_create_vbr session)"); return BVC_EINVAL; }
    if (window_frames < 0 || window_frames > 64) { set_error("bvc_stream_codec_set_repair: window of %d frames outside 0..64", (int)window_frames); return BVC_EINVAL; }
    if (window_frames > 0 && st->bpf > SC_LATE_BYTES) { set_error("bvc_stream_codec_set_repair: frames of %d bytes (at most %d)", st->bpf, SC_LATE_BYTES); return BVC_EINVAL; }
    if (window_frames == st->rep.w) { st->rep.clear(); return BVC_OK; }
    if (window_frames == 0) { BVC_HIP_TRY(hipDeviceSynchronize()); st->rep = bvc_stream_codec::RepairWindow(); return BVC_OK; }
    // the ring (a tick holds at least one frame: at most W ticks are retained) and the replay's compact batch, (B, T') with T' up to
    // W + kmax - 1 frames: the oldest retained tick holds one of the last W frames and up to kmax - 1 older ones.  A pass runs tick by
    // tick, so the recurrences find their workspace in the session's own.
    const bvc_config &c = st->m->cfg;
    const int W = window_frames, B = st->B, kmax = st->kmax, Tm = W + kmax - 1;
    bvc_stream_codec::RepairWindow rw;                       // built aside: whatever fails, it goes with what it got and the session is as before
    rw.w = rw.n = W;
    rw.hs = (long long)B * c.h_dim; rw.pks = pad16((long long)B * kmax * st->bpf); rw.prs = pad16((long long)B * kmax); rw.bs = (long long)B * kmax;
    PoolLayout pl;
    const size_t o_h = pl.take((size_t)W * rw.hs * 4), o_pk = pl.take((size_t)W * rw.pks), o_pr = pl.take((size_t)W * rw.prs), o_bits = pl.take((size_t)W * rw.bs * 4),
                 o_rh = pl.take((size_t)rw.hs * 4), o_rpk = pl.take((size_t)B * Tm * st->bpf), o_rpr = pl.take((size_t)B * Tm), o_rbits = pl.take((size_t)B * Tm * 4),
                 o_rsel = pl.take((size_t)B * Tm * 4), o_rcodes = pl.take((size_t)B * Tm * c.z_dim * 4), o_rzero = pl.take((size_t)B * Tm * 4);
    rw.ring.resize(W);
    bool ok = hipMalloc(reinterpret_cast<void **>(&rw.pool), pl.bytes) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&rw.h_present), (size_t)W * rw.prs, hipHostMallocMapped) == hipSuccess;
    ok = ok && hipHostGetDevicePointer(reinterpret_cast<void **>(&rw.d_hpresent), rw.h_present, 0) == hipSuccess;
    for (auto &t : rw.ring) ok = ok && hipEventCreateWithFlags(&t.ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemset(rw.pool, 0, pl.bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("bvc_stream_codec_set_repair: cannot allocate %zu bytes for a window of %d frames", pl.bytes, W);
        return BVC_ENOMEM;
    }
    memset(rw.h_present, 0, (size_t)W * rw.prs);
    char *p = rw.pool;
    rw.ring_h = pl.at<float>(p, o_h); rw.ring_pk = pl.at<uint8_t>(p, o_pk); rw.ring_pr = pl.at<uint8_t>(p, o_pr); rw.ring_bits = pl.at<float>(p, o_bits);
    rw.r_h = pl.at<float>(p, o_rh); rw.r_pk = pl.at<uint8_t>(p, o_rpk); rw.r_pr = pl.at<uint8_t>(p, o_rpr); rw.r_bits = pl.at<float>(p, o_rbits);
    rw.r_sel = pl.at<float>(p, o_rsel); rw.r_codes = pl.at<float>(p, o_rcodes); rw.r_zero = pl.at<int>(p, o_rzero);
    st->rep = std::move(rw);                                 // (the window the session had goes with rw)
    return BVC_OK;
}

int bvc_stream_codec_late(bvc_stream_codec *st, int32_t slot, int64_t stream_frame, const uint8_t *packet, int32_t *taken) {
    if (taken) *taken = 0;
    if (int rc = slot_arg(st, slot, "bvc_stream_codec_late")) return rc;
    if (st->dir != BVC_STREAM_RECV) { set_error("bvc_stream_codec_late: not a receive session"); return BVC_EINVAL; }
    if (st->vbr) { set_error("bvc_stream_codec_late: no repair window on the wire with a bit count per frame"); return BVC_EINVAL; }
    if (!packet) { set_error("bvc_stream_codec_late: null packet"); return BVC_EINVAL; }
    const bvc_stream_codec::Slot &sl = st->slots[slot];
    if (st->rep.w <= 0 || !sl.open || !sl.started || stream_frame < 0) return BVC_OK;      // no window, or no running stream of which this is a frame
    if (stream_frame >= st->frames - sl.frame0) return BVC_OK;                               // not decoded yet: it belongs into the next tick
    const int64_t f = sl.frame0 + stream_frame;             // the session's count
    bvc_stream_codec::RepairWindow &rw = st->rep;
    const int64_t n_ticks = std::min<int64_t>(st->ticks, rw.n);
    for (int64_t t = st->ticks - n_ticks; t < st->ticks; ++t) {
        const int r = (int)(t % rw.n);
        auto &rt = rw.ring[r];
        if (!st->tick_retained(rt) || f < rt.f0 || f >= rt.f0 + rt.k) continue;
        BVC_HIP_TRY(hipEventSynchronize(rt.ev));             // the tick's snapshot has written the mirror
        uint8_t *pr = rw.h_present + r * rw.prs + (size_t)slot * st->kmax + (f - rt.f0);
        if (*pr) return BVC_OK;                              // it arrived in time, or late once already
        *pr = 1;
        bvc_stream_codec::RepairWindow::LateReq q;
        q.row = slot; q.slot = r; q.j = (int)(f - rt.f0); q.tick = t;
        memset(q.bytes, 0, sizeof(q.bytes));
        memcpy(q.bytes, packet, (size_t)st->bpf);
        rw.late.push_back(q);
        if (taken) *taken = 1;
        return BVC_OK;
    }
    return BVC_OK;                                           // older than the window (or from before a set_conceal / set_repair)
}

}  // extern "C"
