// Internal declarations shared by the gfx950 kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/bvcodec.h"

namespace bvc {

void set_error(const char *fmt, ...);

#define BVC_HIP_TRY(expr)                                                              \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            bvc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return BVC_EHIP;                                                           \
        }                                                                              \
    } while (0)

// ------------------------------------------------------------------ in-situ kernel timing (bench only)
// bvc_probe_begin(kind, every, max) makes every `every`-th launch of kernel family `kind` be
// bracketed by a hipEvent pair on its own stream; bvc_probe_end() reports the mean elapsed time.
enum ProbeKind { PK_NONE = 0, PK_LINEAR = 1, PK_GRU = 2, PK_CONV = 3, PK_BATCHED = 4, PK_STFT = 5, PK_POST = 6 };
struct ProbeScope {
    hipStream_t s; int slot;
    ProbeScope(int kind, hipStream_t stream);
    ~ProbeScope();
};

// ------------------------------------------------------------------ skinny / recurrent GEMM (k_gemm.hip; shared device helpers: k_gemm.h)
// Per-call dynamic state, resident in device memory.  The recurrent-step kernels are captured ONCE
// into a hipGraph and replayed for every frame, so nothing that changes per call or per frame may be a
// kernel argument: caller tensors are reached through this descriptor and the frame index `t` is a
// device-side counter advanced by step_advance_kernel at the end of every step.
enum DescSlot { DS_PX = 0, DS_CODES = 1, DS_BITS = 2, DS_PROB = 3, DS_ALLH = 4, DS_MEL = 5, DS_PZ = 6, DS_NOISE = 7, DS_NSLOT = 8,
                DS_PRIOR = DS_ALLH /* BVRNN.forward has no all_h output: the slot carries the prior probabilities */,
                DS_PARTD = DS_PX, DS_PARTG = DS_CODES /* decode has neither: pre-computed phi_z halves of dec.0 / of the GRU input */,
                DS_KEEP = DS_PROB /* decode with the folded hop: ELU(dec.4) of all frames, (B,T,H) */,
                DS_KEEP_ENC = DS_PZ /* ... and encode's, when the fused forward wants the decoder's output (encode has no phi_z tensor) */ };
struct CallDesc {
    float *p[DS_NSLOT];              // base pointers of the (B, T, dim) tensors of this call (may be null)
    long long T;                     // frames per utterance
    int t;                           // current frame
    int nodes_per_step;              // kernels per step (probe slot = t * nodes_per_step + node)
};

// A pointer whose value depends on the frame counter.
//   kind 0 (static) : base, row stride ld
//   kind 1 (frame)  : desc->p[sel] + (t + toff) * dim, row stride T * dim; invalid outside [0, T) or if null
//   kind 2 (parity) : base + (((t + toff) & 1) ? poff : 0), row stride ld      (GRU state ping-pong)
//   packed != 0: the [M][ld] matrix is stored in MFMA A-operand fragment order
//       [m/16][k/16][lane = ((k%16)/4)*16 + m%16][k%4]   (one 16x16 block = 1 KiB contiguous),
//       so a wave's operand load is one fully coalesced 1 KiB read; frame tensors then hold one such
//       packed [M][dim] matrix per frame.
struct DynPtr {
    float *base;
    int ld;                       // row stride in floats (static / parity kinds)
    int poff;                     // parity kind: offset added when ((t + toff) & 1); static kind: floats between the frames of a multi-frame launch (GemmParams::frames)
    int meta;                     // kind | packed << 4 | sel << 8 | (toff + 8) << 16
    int dim;                      // frame kind: floats per frame row
};
inline int dp_meta(int kind, int packed, int sel, int toff) { return kind | (packed << 4) | (sel << 8) | ((toff + 8) << 16); }
inline DynPtr dp_static(const float *p, long long ld, int packed = 0) { return DynPtr{const_cast<float *>(p), (int)ld, 0, dp_meta(0, packed, 0, 0), 0}; }
// static pointer of a launch that covers several frames at once (grid.y = frame): frame f reads / writes base + f * fstride
inline DynPtr dp_static_frames(const float *p, long long ld, long long fstride, int packed = 0) { return DynPtr{const_cast<float *>(p), (int)ld, (int)fstride, dp_meta(0, packed, 0, 0), 0}; }
inline DynPtr dp_frame(int sel, int dim, int toff = 0, int packed = 0) { return DynPtr{nullptr, 0, 0, dp_meta(1, packed, sel, toff), dim}; }
inline DynPtr dp_parity(float *p, long long ld, long long poff, int flip, int packed = 0) { return DynPtr{p, (int)ld, (int)poff, dp_meta(2, packed, 0, flip), 0}; }
inline DynPtr dp_null() { return DynPtr{nullptr, 0, 0, 0, 0}; }
inline int dp_kind(const DynPtr &d) { return d.meta & 15; }
inline int dp_packed(const DynPtr &d) { return (d.meta >> 4) & 1; }

// One K-segment of a (possibly concatenated) input:  acc[grp] += x[M,K] @ w[rows,K]^T
struct GemmSeg {
    const float *w;      // weights in MFMA B-operand fragment order [n/16][k/16][lane][4], already offset
                         // to this segment's first k-block
    int          wnb;    // k-blocks (of 16) per weight row, i.e. floats between n-tiles / 256
    int          K;      // multiple of 16
    DynPtr       x;      // [M][ld]
    int          grp;    // accumulator group (0: input part, 1: hidden part of the GRU)
    int          pad_;
};

enum GemmEpi {
    EPI_LINEAR = 0,      // y = acc + bias
    EPI_ELU = 1,         // y = elu(acc + bias)
    EPI_CODE = 2,        // p = sigmoid(acc+bias); z = rint(p); masked by bits  (bvrnn.py:189-194)
    EPI_MEL = 3,         // y = acc + bias (mel frame) ; y2 = (y - mean) / std  (bvrnn.py:202-204)
    EPI_GRU = 4,         // PyTorch GRU cell, 3 gates x 2 groups (whole cell in one launch)
    EPI_GRU_PART = 5,    // GRU cell whose hidden part and phi_z part were pre-computed on the side branch:
                         //   gi = acc + y2part (W_ih[:, H:] phi_z + b_ih), gh = y3part (W_hh h + b_hh)
    EPI_SIGMOID = 6      // y = sigmoid(acc + bias)   (prior net, bvrnn.py:68-73)
};
// EPI_CODE variants (GemmParams::sample): what is rounded and which value z takes
enum CodeSample {
    CS_ENCODE = 0,       // z = round(p)                              BVRNN.encode (bvrnn.py:191)
    CS_GREEDY = 1,       // z = (round(p) - p) + p                    BVRNN.forward greedy (bvrnn.py:124), straight-through value
    CS_SAMPLE = 2,       // z = (round((u - 0.5) + p) - p) + p        Bernoulli sampler (bvrnn.py:126), u from y2
    CS_SELECT = 3        // z = selector < 0 ? received code (y2) : round(p) masked to `selector` bits: the concealing decoder; p is the
                         // prior's.  aux = the selector per row (launch_conceal_select), whatever var_bit says
};

// The first 16 dwords (M .. seg[0].x) hold everything a layer needs to map its tile and issue the operand
// loads of its first segment, so they can be pre-loaded into SGPRs at dispatch (build with
// BVC_KERNARG_PRELOAD=1 -> -mllvm -amdgpu-kernarg-preload-count=16; worth 0.3 us per layer in
// tools/skinny_bench, neutral in the full schedule, hence off by default).
struct GemmParams {
    int     M, N;              // N = outputs per gate (multiple of 16)
    int     nb_total;          // sum over segments of K/16
    int     gate_rows;         // row distance between gates inside w (GRU: h_dim); bias index stride
    GemmSeg seg[3];
    int     nseg;
    int     var_bit;
    int     sample;            // EPI_CODE: CodeSample
    int     gate_il;           // weights are gate-interleaved [n/16][k/16][gate][lane][4] (GRU launches)
    const float *bias0;        // group 0 bias [gates*N] (may be null)
    const float *bias1;        // group 1 bias (GRU only)
    DynPtr  y, y2, y3;         // outputs (y2/y3 optional); EPI_CODE with CS_SAMPLE: y2 = uniform noise INPUT, with CS_SELECT: the received codes (INPUT)
    DynPtr  aux;               // CODE: bits per frame (one per row); GRU: previous h; LINEAR/ELU: optional addend (natural [M][N])
                               // GRU: y3 (if valid) = pre-computed part of the input gates gi, natural [M][3*gate_rows]
    const float *part_i; const float *part_h; long long ldpart;   // GRU_PART: side-branch partial sums [M][3H]
    const float *mean; const float *stdv; // MEL epilogue
    const CallDesc *desc;      // null for stand-alone launches (all pointers static)
    unsigned long long *probe; // in-kernel timing slots, set only in the probe variant of a step graph
    int     node;              // index of this kernel inside its step (probe slot)
    int     tstep;             // static frame offset inside an unrolled multi-step graph: t = desc->t + tstep
    int     frames;            // > 1: the same layer for several independent frames in ONE launch (grid.y; every pointer static, see dp_static_frames)
};

int launch_gemm_skinny(const GemmParams &p, int epi, hipStream_t s, int mtw = 1);
int skinny_kernels_init();
// The instantiations of the recurrent-layer kernel (the table in k_gemm.hip) and the rule by which launch_gemm_skinny chooses one:
// a pure function of the row count, the epilogue, the weight layout, the row tiles per workgroup the caller asks for and the
// BVC_LATENCY switch (host only, no HIP calls).  mtw of the answer: the row tiles per workgroup of the kernel that runs.
enum SkinnyId { SK_GRU, SK_GRU_IL, SK_GRU_IL2, SK_GRU_PART, SK_LIN, SK_LIN_LATENCY, SK_LIN2, SK_LIN4, SK_COUNT };
struct SkinnyPick { SkinnyId id; int mtw; };
SkinnyPick skinny_pick(int M, int epi, int gate_il, int mtw, bool latency);
// host-side launches of this process per kernel (tests): [id] one-frame launches, [SK_COUNT + id] multi-frame ones.  A launch
// captured into a graph counts once, at capture
void skinny_launch_counts(long long *out);
int launch_step_advance(CallDesc *d, int by, hipStream_t s);
int launch_set_desc(CallDesc *d, const CallDesc &v, hipStream_t s);

// ------------------------------------------------------------------ how a launch is cut into tiles (host only, no HIP calls)
// The MFMA-bound kernels run fixed-height tiles on a fixed number of workgroup slots, every tile takes the same time, and a
// grid that ends in a partly filled round pays for a whole one.  tile_plan() picks, among the compiled tile heights, the one
// that minimises rounds x (height + fixed): tiles = column_blocks x ceil(rows / (height - overlap)), rounds = ceil(tiles / slots).
// `fixed` (rows) stands for what a tile costs whatever its height - prologue, halo, epilogue - and is fitted per kernel from
// two measured heights (profiles/tile_rounds.md).  overlap: rows of a tile that produce no output (the causal halo ks - 1 of
// the AMP pair; 0 for the GEMM).  Ties go to the taller tile.  No candidate or no rows: height 0.
struct TilePlan { int height; long long tiles, rounds, cost; };
inline TilePlan tile_plan(long long rows, long long column_blocks, const int *heights, const int *slots_for_height, int n,
                          int fixed, int overlap = 0) {
    TilePlan best = {0, 0, 0, 0};
    if (rows <= 0 || column_blocks <= 0) return best;
    for (int i = 0; i < n; ++i) {
        const int h = heights[i], out_rows = h - overlap, slots = slots_for_height[i];
        if (out_rows <= 0 || slots <= 0) continue;
        const long long tiles = column_blocks * ((rows + out_rows - 1) / out_rows);
        const long long rounds = (tiles + slots - 1) / slots;
        const long long cost = rounds * (h + fixed);
        if (best.height == 0 || cost < best.cost || (cost == best.cost && h > best.height)) best = {h, tiles, rounds, cost};
    }
    return best;
}
// The batched GEMM's cut: one launch of `height`-row tiles (tail_height 0), or full_blocks row blocks of 128 followed by a second
// launch of tail_height-row tiles for the rows of the last, partly filled round.  cost100: the model's cost in hundredths of a row.
// A pure function of its arguments (k_gemm_batched.hip): no_tail / no_quarter take the two-launch cut or its quarter tiles out.
struct GemmCut { int height; int full_blocks; int tail_height; long long tiles, rounds, cost100; };
GemmCut gemm_batched_cut(int M, int N, int force_height = 0, bool legacy = false, bool no_tail = false, bool no_quarter = false);
// The environment switches of the batched GEMM, read by gemm_switches() alone (which says when): BVC_NO_LDS_GEMM, BVC_NO_GEMM_TAIL,
// BVC_NO_GEMM_QUARTER, BVC_TILE_TRACE, BVC_TILE_CUT=legacy, BVC_GEMM_BM (its text, or null)
struct GemmSwitches { bool no_lds, no_tail, no_quarter, trace, legacy; const char *gemm_bm; };
GemmSwitches gemm_switches();
// The offline C = 64 AMP pair's cut: rows per workgroup tile (a compiled TR) for L output rows x B items
TilePlan amp_pair_cut(long long L, int B, int ks, int force_height = 0, bool legacy = false);
// what the last launch_gemm_batched / offline C = 64 launch_amp_pair of this process chose (tests)
bool tile_cut_legacy();
void tile_trace(const char *what, long long rows, long long cols, int height, int tail_height, long long tiles, int slots, long long rounds);
extern GemmCut g_last_gemm_cut;
extern TilePlan g_last_amp_cut;

// ------------------------------------------------------------------ batched GEMM (k_gemm_batched.hip)
// batched GEMM over all frames: y = act(x @ w^T + bias), M large.  out_mode (GemmOut) says where the rows go:
// see out_index() in k_gemm_batched.hip.  frames_T = frames per utterance, mt16 = utterances rounded up to 16.
enum GemmOut { GO_NATURAL = 0, GO_FRAME_MAJOR_ROWS = 1, GO_PACKED_FRAMES = 2, GO_PACKED_FROM_UTT = 3 };
int launch_gemm_batched(const float *x, long long ldx, const float *w, long long ldw, const float *bias,
                        int M, int N, int K, int act, float *y, long long ldy, hipStream_t s,
                        int out_mode = GO_NATURAL, long long frames_T = 0, int mt16 = 0);
// ------------------------------------------------------------------ row-wise utilities (k_rows.hip)
// yn = (y - mean) / std over rows of length n (bvrnn.py:173)
int launch_normalize_rows(const float *y, const float *mean, const float *stdv, long long rows, int n,
                          float *out, hipStream_t s);
int launch_fill(float *p, float v, long long n, hipStream_t s);
// per-frame KL term of BVRNN.forward (bvrnn.py:148-157): kld[t] = mean_b sum_j mask * elem(prob, prior)
int launch_kld_frames(const float *prob, const float *prior, const float *bits, int B, long long T, int Z, float *kld,
                      hipStream_t s);
int launch_copy_rows(const float *src, long long lds, float *dst, long long ldd, int rows, int n, hipStream_t s);
// natural [rows][n] (row stride ld) <-> fragment-packed [rows/16][n/16][64][4]; dir 0: pack, 1: unpack
int launch_repack_rows(const float *src, float *dst, long long ld_natural, int rows, int n, int dir, hipStream_t s);

// ------------------------------------------------------------------ backward pass (k_backward.hip)
// How the M summed rows of a weight gradient are cut: `chunks` chunks of `chunk_rows` rows, their sums in ws_floats floats of
// workspace (0: one chunk, written in place).  A function of (M, N, K) alone: it fixes the order of summation.
struct WeightGradCut { int chunks, chunk_rows; size_t ws_floats; };
WeightGradCut weight_grad_cut(int M, int N, int K);
// dW (N, K) = dY (M, N)^T X (M, K), overwritten; natural dense matrices, N and K multiples of 16
int launch_weight_grad(const float *dY, const float *X, int M, int N, int K, float *dW, float *ws, hipStream_t s, long long ldo = 0);
// The row-wise kernels of the reverse recurrence (natural matrices; frame-major rows are t * B + b, utterance-major rows b * T + t):
// T taped fragment-packed [mt16][n] matrices `fstride` floats apart -> frame-major rows
int launch_unpack_frames(const float *src, long long fstride, long long T, int B, int n, float *dst, hipStream_t s);
// dir 0: utterance-major -> frame-major, 1: back; scale (may be null): divided by scale[column] on the way
int launch_reorder_rows(const float *src, int B, long long T, int n, float *dst, int dir, const float *scale, hipStream_t s);
int launch_transpose(const float *src, int R, int C, float *dst, hipStream_t s);
// out = dy * ELU'(from the output y); out may be dy
int launch_elu_bwd(const float *dy, const float *y, float *out, long long total, hipStream_t s);
// out (B, X) = gdec[:, t] + gdn / std (gdn may be null)
int launch_mel_bwd(const float *gdec, long long T, long long t, const float *gdn, const float *stdv, int B, int X, float *out, hipStream_t s);
// frame t of the straight-through sample and the KLD, back to the encoder's and the prior's logits xe, xq (B, Z); scale = g_kld / (T B)
int launch_code_bwd(const float *gz, const float *xe, const float *xq, const float *bits, long long T, long long t, int B, int Z,
                    float scale, float *d_enc_logit, float *d_prior_logit, hipStream_t s);
// the GRU cell from its gate sums gi, gh (B, 3H), the state h it started from and the gradient of the state it produced
int launch_gru_bwd(const float *dhn, const float *gi, const float *gh, const float *h, int B, int H, float *dgi, float *dgh, float *dh_direct,
                   hipStream_t s);
// out (N) = column sums of dY (M, N), rows in a fixed order
int launch_col_sum(const float *dY, int M, int N, float *out, hipStream_t s);

// ------------------------------------------------------------------ optimiser step and in-place weight rewrite (k_optimizer.hip)
// up to COPY_SEGMENTS copies in one launch: n floats (a multiple of 4) from src to dst, both 16-byte aligned
constexpr int COPY_SEGMENTS = 40;
struct CopySegment { const float *src; float *dst; long long n; };
struct CopySegments { CopySegment s[COPY_SEGMENTS]; int n; };
int launch_copy_segments(const CopySegments &segs, hipStream_t s);
// weight_pack.h's pack_gru_interleaved and fold_px0_dec3 on device tensors, the same bits; the fold writes W fragment-packed
int launch_pack_gru_interleaved(const float *W, int H, int K, float *out, hipStream_t s);
int launch_fold_px0_dec3(const float *wp0, const float *bp0, const float *wd6, const float *bd6, const float *mean, const float *stdv, int H,
                         int X, float *wp_out, float *b_out, hipStream_t s);
// The 2-norm of `total` floats (a multiple of 4) in two stages with float64 accumulators: chunks of NORM_CHUNK floats into partial
// (norm_chunks(total) doubles), then one workgroup.  scal[0] = min(1, max_norm / (norm + 1e-6)) (1 where max_norm <= 0), scal[1] = the
// norm, also to norm_out if given.
constexpr int NORM_CHUNK = 8192;
int norm_chunks(long long total);
int launch_grad_norm(const float *g, long long total, float max_norm, double *partial, float *scal, float *norm_out, hipStream_t s);
// One AdamW step over `total` floats, per element in f32 and in this order, every operation rounded on its own:
//   p *= decay;  m = b1 m + one_b1 g;  v = b2 v + (one_b2 g) g;  p -= step_size (m / (sqrt(v) / bc2_sqrt + eps)),  g = scal[0] * the gradient
struct AdamScalars { float decay, b1, one_b1, b2, one_b2, step_size, bc2_sqrt, eps; };
int launch_adam(float *p, float *m, float *v, const float *g, const float *scal, long long total, const AdamScalars &a, hipStream_t s);

// ------------------------------------------------------------------ persistent recurrence (k_flow.hip, k_flow_support.hip)
// All frames of BVRNN.encode / BVRNN.decode in one launch; layers are chained by "poisoned buffer" dataflow
// (see k_flow_handoff.h).  Activations live in the flow region of the workspace: FlowBuf id, frame parity ->
// flow + (id * 2 + parity) * slot_bytes, each a fragment-packed [MT16][dim] matrix.
constexpr unsigned FLOW_POISON = 0xFFFFDEADu;      // a NaN bit pattern no layer may publish as data
constexpr int FLOW_STAMPS = 6;                     // stamp kinds per layer and frame (k_flow_layers.h: flow_stamp)
enum FlowEpi { FE_ELU = 0, FE_CODE = 1, FE_MEL = 2, FE_GRU = 3, FE_ELU_KEEP = 4, FE_CODE_SEL = 5 };   // FE_ELU_KEEP: ELU, and the result also goes to FlowArgs::keep
                                                                                     // FE_CODE_SEL: FE_CODE of the concealing decoder (CS_SELECT)
enum FlowBuf { FB_H = 0, FB_E1, FB_E2, FB_ZC, FB_Q1, FB_Q2, FB_Q3, FB_D1, FB_D2, FB_D3, FB_DN, FB_G1, FB_G2, FB_G3, FB_COUNT };
struct FlowLin {         // one K-segment of a layer as the persistent kernel sees it (32-/64-bit fields: scalar loads)
    const float *w;      // packed weights [n/16][k/16][lane][4], offset to the segment's first k-block
    const float *bias;   // [N] or null
    int wnb;             // k-blocks per weight row
    int pad_;
};
struct FlowArgs {
    // layers of the step in dependency order (encode: bvrnn.py:187-206, decode: bvrnn.py:222-227).  enc0h / dec0h: the
    // halves of enc.0 / dec.0 that multiply h (the other halves are batched over all frames beforehand: part0);
    // dec0z: the phi_z half of dec.0, used by encode only (there the bias of dec.0 travels in dec0h).
    FlowLin enc0h, enc1, enc2, pz0, pz1, pz2, dec0h, dec0z, dec1, dec2, dec3, px0, px1, px2;
    const float *w_hh, *w_ihx, *w_ihz;      // GRU, gate-interleaved [n/16][k/16][gate][lane][4]: W_hh, W_ih[:, :H], W_ih[:, H:]
    const float *b_ih, *b_hh;
    int hb, zb, xb;                         // h_dim / 16, z_dim / 16, num_mels / 16
    float *flow; unsigned slot_bytes;
    int B, MT, NTG;                         // utterances, utterance groups of 16, feature tiles covered by the grid
    long long T;
    const float *part0;                     // (B,T,H) pre-computed half of the first layer (+ its bias)
    const float *part_gru;                  // decode: (B,T,3H) pre-computed phi_z half of the GRU input gates (+ b_ih)
    float *codes, *prob; const float *bits; float *all_h; float *mel;
    const float *mean, *stdv;
    int var_bit;
    unsigned *status; unsigned spin_limit;
    unsigned long long *probe;              // bench only: [FLOW_STAMPS][T][nodes] s_memrealtime stamps of one wave (0 layer entry, 1 exit, 2.. diagnostics)
    int probe_nodes, probe_first;           // layers per frame, id of the first one
    int probe_wg, probe_wave;               // which workgroup / wave stamps (BVC_PROBE_WG / BVC_PROBE_WAVE, default 0 / 0)
    int dbg_hot_w;                          // experiments only (BVC_FLOW_HOTW=1): every weight request hits the same blocks (wrong results)
    int MG;                                 // utterance groups (chains) per workgroup; 1 = one chain (B <= 16 * CUs / feature tiles)
    int dbg_withhold;                       // tests only: workgroup 0 returns at once
    // the folded hop (model.hip: build_bvrnn): dec.6 has no activation, so phi_x.0(norm(dec.6(u))) is ONE affine map
    // of u = ELU(dec.4(.)) followed by the ELU: pxc = (phi_x.0.W diag(1/std) dec.6.W, phi_x.0.W ((dec.6.b - mean) / std) + phi_x.0.b).
    // The kernel then runs dec.4 -> pxc -> phi_x.2 ... (one wide layer instead of the two narrow hops dec.6, phi_x.0); decode stores u for
    // all frames in `keep` (B,T,H), and dec.6 itself - the decoder's output - is one batched GEMM over `keep` behind the launch.
    FlowLin pxc;                            // w == null: the layers as the reference lists them
    float *keep;
    // the concealing decoder (the third program, CONCEAL): the encode program with prior.{0,2,4} in enc0h / enc1 / enc2 (enc0h with its own
    // bias, no part0), `bits` = the selector per (utterance, frame) (launch_conceal_select) and the received codes; `codes` takes the
    // filled codes (may be codes_in itself), `prob` the prior's probabilities
    const float *codes_in;
};
// The persistent kernels' dynamic LDS, defined once: the kernel takes its regions' offsets from here (in floats; NW waves per workgroup,
// a wave's partial 16 x 16 tile is 256 floats), the launch table its bytes per form, the census kernel the filler form's bytes.
enum FlowForm { FF_PLAIN = 0, FF_FILL = 1, FF_CHAINS = 2, FF_CHAINS_FOLDED = 3 };      // chains: several utterance groups per workgroup (FlowArgs::MG > 1)
template <int NW>
struct FlowLds {
    static constexpr int partials = 0;                          // [2][NW][256] layer partials, slot = hop & 1
    static constexpr int gru = partials + 2 * NW * 256;         // [NW][6][256] GRU partials
    static constexpr int plain_end = gru + NW * 6 * 256;
    static constexpr int chain = plain_end;                     // chains: [2][4][NW][256] partial tiles of a group of chains
    static constexpr int chain_end = chain + 2 * 4 * NW * 256;
    // Filler kernels: the waves' operand stashes lie over the GRU partials - the stashes are dead from the last quantum (layer 9) to the
    // next frame's first layer, whose operand, h(t+1), exists only after wave 0 has read the partials
    static constexpr int stash = gru;                           // [NW][8][256], a wave's blocks at stride PERH * 256
    static constexpr int park = stash + NW * 8 * 256;           // [NW][8][256] the first layer's parked weights (BVC_FLOW_PARKL)
    static constexpr int flag = park + NW * 8 * 256;            // hop count of wave 0's last publishing store (BVC_FLOW_PARTNER_WAIT), 16 bytes
    static constexpr int fill_end = flag + 4;
    static constexpr size_t bytes(int form) { return sizeof(float) * (form == FF_PLAIN ? plain_end : form == FF_FILL ? fill_end : chain_end); }
};
static_assert(FlowLds<8>::bytes(FF_PLAIN) == 64 * 1024 && FlowLds<8>::bytes(FF_CHAINS) == 128 * 1024 && FlowLds<8>::bytes(FF_CHAINS_FOLDED) == 128 * 1024 &&
              FlowLds<8>::bytes(FF_FILL) == 144 * 1024 + 16, "64 / 128 / 144 KiB (+ the flag) of a compute unit's 160");
int flow_kernels_init();
int flow_census_init();       // (k_flow_support.hip; called by flow_kernels_init)
int flow_perh(int h_dim);
int launch_flow_set_args(const FlowArgs &a, FlowArgs *d_args, hipStream_t s);         // the device copy of the arguments alone (k_flow_support.hip)
int launch_flow(const FlowArgs &a, FlowArgs *d_args, int perh, bool encode, bool fill, hipStream_t s, bool args_resident = false,
                bool conceal = false);
// sentinel fill of the flow region + initial state into its first buffer + the device copy of the arguments, in one kernel
int launch_flow_prepare(const FlowArgs &a, FlowArgs *d_args, unsigned *flow, long long n_flow, long long n_h0, const float *d_h0, int B, int H,
                        hipStream_t s);
int launch_flow_census(unsigned *ctr, int grid, unsigned spin_limit, hipStream_t s);   // ctr[0] arrivals, ctr[1] workgroups that gave up
int launch_fill_u32(unsigned *p, unsigned v, long long n, hipStream_t s);

// ------------------------------------------------------------------ front-end (k_frontend.hip)
struct FrontendTables {          // device pointers
    const float *window;         // [1024]
    const float2 *tw1;           // [8][64]  W_512^(lane*k0)
    const float2 *tw2;           // [8][8]   W_64^(n0*k1)
    const float2 *tws;           // [513]    e^{-2 pi i k / 1024}
    const int   *mel_start;      // [num_mels]
    const int   *mel_len;        // [num_mels]
    const int   *mel_off;        // [num_mels] offset into mel_w
    const float *mel_w;          // packed non-zero weights
    int num_mels;
    int kmax;                    // highest bin with non-zero weight (+1)
};
// lens (B) or nullptr: row b holds lens[b] valid samples of its L (mixed-length batch: ragged_frames below)
int launch_stft_logmel(const FrontendTables &t, const float *wav, int B, long long L, long long T,
                       int pad_left, float scale, float *mel, hipStream_t s, const long long *lens = nullptr);
// Frames of an utterance of `len` valid samples in a row of L: bvc_num_frames of len clamped into [0, L] (n_fft = 1024 and hop = 256,
// which check_config enforces), 0 where the reflect padding does not fit.  The per-row lengths of a mixed-length batch live on the
// device, so the kernels that read them clamp instead of validating.
__host__ __device__ inline long long ragged_frames(long long len, long long L, int pad_left) {
    len = len < 0 ? 0 : (len > L ? L : len);
    const long long pr = 1024 - 256 - pad_left;
    if (len <= pad_left || len <= pr) return 0;
    return (len + pad_left + pr - 1024) / 256 + 1;
}
// mixed-length batch: bits (B, T) = d_bits[b] (or dflt) on row b's live frames, 0 behind them; codes (B, T, z) = 0.5 behind them
int launch_ragged_bits(float *bits, const float *d_bits, float dflt, const long long *lens, int B, long long L, long long T,
                       int pad_left, hipStream_t s);
int launch_ragged_mask(float *codes, const long long *lens, int B, long long L, long long T, int z, int pad_left, hipStream_t s);

int launch_resample_poly(const float *x, int B, long long Lin, const double *h, int ntaps, int up, int down,
                         long long n_pre_remove, float *y, long long n_out, hipStream_t s);
int launch_peak_normalize(float *x, int B, long long L, hipStream_t s);

// ---- streaming resampler (k_resample_stream.hip; its host side, bvc_resampler_*, is resampler.hip)
// Outputs that N inputs of a row complete: E(N) = max(0, ceil(N up / down) - n_pre_remove); the lag-delayed stream
// zeros(n_pre_remove) ++ y has ceil(N up / down) of its samples then.  The one copy, for the host's counts and the kernel's.
__host__ __device__ inline long long rs_ceil_mul(long long n, int up, int down) { return (n * up + down - 1) / down; }
__host__ __device__ inline long long rs_count(long long n, int up, int down, int n_pre_remove, bool delayed) {
    const long long c = rs_ceil_mul(n, up, down);
    return delayed ? c : (c > n_pre_remove ? c - n_pre_remove : 0);
}
struct RsRow { long long n; int run, start, valid, rate; };      // device state of a row: inputs so far; running; where it starts in the
                                                                // next chunk; how many of that chunk's samples are its (-1: all); the
                                                                // index of its filter in a multi-rate resampler's table (else 0)
const int RS_LIST = 64;                                         // row changes per launch: they travel as a kernel argument
struct RsUpdate { int row, run, start, valid, reset, rate, pad_[2]; };    // rate: taken over where reset is set (the row is opened)
struct RsUpdateList { int n; int pad_[3]; RsUpdate e[RS_LIST]; };
struct RsFilter { const double *h; int ntaps, up, down, n_pre_remove, H; };      // H = ceil(ntaps / up) inputs of history per row
struct RsCall { const void *x; long long xs; void *y; long long ys, yoff; int n_in, n_fill, fmt_in, fmt_out, delayed, flush_row; };
// a multi-rate resampler: one filter per rate, the row's index in RsRow.rate; the rows' histories lie H_max = max H apart.  A call has
// a chunk length and an output block per rate, n_fill[r] = ceil(n_in[r] up_r / down_r); every row's block is written up to n_fill_max
// (a flush: the row's rest, n_fill_max samples)
const int RS_MAX_RATES = 8;
struct RsFilterTable { RsFilter f[RS_MAX_RATES]; int n; };
struct RsCallMulti { const void *x; long long xs; void *y; long long ys, yoff; int n_in[RS_MAX_RATES], n_fill[RS_MAX_RATES];
                     int n_fill_max, H_max, fmt_in, fmt_out, delayed, flush_row; };
int launch_rs_update(const RsUpdateList &l, RsRow *ctl, float *hist, int H, hipStream_t s);
int launch_rs_push(const RsFilter &f, const RsCall &c, int lds_floats, RsRow *ctl, float *hist, int B, hipStream_t s);
int launch_rs_push_multi(const RsFilterTable &t, const RsCallMulti &c, int lds_floats, RsRow *ctl, float *hist, int B, hipStream_t s);

int launch_pack_codes(const float *codes, long long frames, int z, int nbits, unsigned char *out, hipStream_t s);
int launch_unpack_codes(const unsigned char *in, long long frames, int z, int nbits, float *codes, hipStream_t s);
// the same wire format with every row's own bit count (directed streaming sessions): packets (B, kstride, nbytes) with nbytes = ceil(z / 8)
// for every row, codes (B, k, z); bits (B, k) = bits per (row, frame) (nullptr: z everywhere), row_off[b] < 0 = idle row
int launch_pack_rows(const float *codes, const float *bits, int B, int k, int z, int kstride, unsigned char *out, hipStream_t s);
int launch_unpack_rows(const unsigned char *in, const unsigned char *present, const float *bits, const int *row_off, int B, int k,
                       int z, int kstride, float *codes, hipStream_t s);
// the concealing decoder's selector, one float per (row, frame): -1 where the frame arrived (present (B, k) bytes, row stride kstride) or the
// row is idle (row_off[b] < 0; row_off may be null), else the bits a generated frame gets: bits[b * k + t] (or dflt if bits is null), not below 0
int launch_conceal_select(const unsigned char *present, long long kstride, const float *bits, float dflt, const int *row_off, int B,
                          long long k, float *sel, hipStream_t s);

// ------------------------------------------------------------------ closed-loop rate selection (k_vbr.hip)
// bvc_bvrnn_encode_vbr: per frame the encoder tries the rungs of a ladder of bit counts - the K masked copies of the frame's code
// run phi_z and dec as K * B rows (candidate row k * B + b) of the recurrent-layer GEMM - and keeps the first rung whose decoded mel
// lies within the frame's target: D_k = mean_j |d^k_j - y_j| <= tau, else the last rung.
constexpr int VBR_MAX_RUNGS = 8;
// The caller's tensors and the ladder of one call, resident in the call's workspace: like the CallDesc they are no kernel arguments,
// because the step is captured once and replayed.  The frame counter and T are the CallDesc's.
struct VbrCall {
    const float *y;                  // (B,T,X) the mel the call encodes
    const float *tau;                // (B,T) distortion targets
    float *codes;                    // (B,T,Z) the chosen rung's code
    float *bits;                     // (B,T) its bit count
    float *dist;                     // (B,T,K) D of every rung, or null
    float *dec;                      // (B,T,X) the chosen rung's decoded mel, or null
    int *choice;                     // (B,T) the chosen rung, or null (the test hook)
    int ladder[VBR_MAX_RUNGS];       // bit counts, ascending
    // the rate cap (bvc_bvrnn_encode_vbr_capped): an integer token bucket per row in q8 (1/256 bit).  Per frame, behind today's choice
    // k_target: tok = min(burst, tok + rate); a = the largest k with ladder[k] * 256 <= tok (0 if none); k* = min(k_target, a);
    // tok = max(0, tok - ladder[k*] * 256).  capped == 0: none of it runs.
    int capped, rate_q8, burst_q8;
    int *tok;                        // (B) the rows' buckets, carried from frame to frame (and from call to call by the caller)
};
// the cap of one call as the host passes it on: tok0 (B) or null = full buckets, tokT (B) or null; tok0 == tokT is fine
struct VbrCap { int capped, rate_q8, burst_q8; const int *tok0; int *tokT; };
// One frame's buffers (workspace-static; fragment-packed unless stated) and sizes: the arguments of the two kernels.
struct VbrStep {
    const CallDesc *desc;            // null: a stand-alone launch on (B, 1, .) tensors (the test hook)
    const VbrCall *call;
    int B, K, Z, H, X;
    const float *zraw;               // [mt16(B)][Z] round(p) of the frame, no mask
    const float *hbuf; long long MH; // the GRU state ping-pong: h_t = hbuf + (t & 1) * MH, [mt16(B)][H]
    float *zc;                       // [mt16(K B)][Z] the K masked copies
    float *hrep;                     // [mt16(K B)][H] h_t, K times
    const float *melk;               // natural [K B][X] dec.6 of the candidates
    const float *dnk;                // [mt16(K B)][X] ... normalised (may be null)
    const float *pzk;                // [mt16(K B)][H] phi_z of the candidates (may be null)
    float *pzsel;                    // [mt16(B)][H] the chosen rows of pzk
    float *dnsel;                    // [mt16(B)][X] the chosen rows of dnk
};
int launch_vbr_set_call(VbrCall *d, const VbrCall &v, hipStream_t s);
int launch_vbr_candidates(const VbrStep &a, int tstep, hipStream_t s);
int launch_vbr_select(const VbrStep &a, int tstep, hipStream_t s);
// the wire format with a per-frame bit count: a frame is 1 + ceil(z / 8) bytes - its bit count n, ceil(n / 8) bytes of bits in
// launch_pack_codes order, zeros; sizes (frames) = 1 + ceil(n / 8)
int launch_pack_codes_vbr(const float *codes, const float *bits, long long frames, int z, unsigned char *out, int *sizes, hipStream_t s);
int launch_unpack_codes_vbr(const unsigned char *in, long long frames, int z, float *codes, float *bits, hipStream_t s);
// dst[b] = src ? src[b] : fill, b < B (the buckets of a capped call; dst == src: nothing)
int launch_vbr_tok(int *dst, const int *src, int fill, int B, hipStream_t s);
// that wire inside a streaming tick (bvc_stream_codec_create_vbr): codes (B, k, z), bits (B, k); frame j of row b at
// (b * kstride + j) * (1 + ceil(z / 8)) of the packet buffer, sizes / bits_out (B, kstride) (each may be null; so may `out`).  Unpack: a
// frame that is not present, or of an idle row (row_off[b] < 0), is a frame of no bits
int launch_pack_rows_vbr(const float *codes, const float *bits, int B, int k, int z, int kstride, unsigned char *out, int *sizes,
                         float *bits_out, hipStream_t s);
int launch_unpack_rows_vbr(const unsigned char *in, const unsigned char *present, const int *row_off, int B, int k, int z, int kstride,
                           float *codes, float *bits_out, hipStream_t s);

// ------------------------------------------------------------------ entropy-coded wire format (k_entropy.hip)
// A binary range coder with carry propagation under the prior net's probabilities: 32-bit range, 33-bit low, 16-bit probabilities
// q = clamp(rint(p * 65536), 1, 65535) = P(bit = 1), one independent stream per (row, segment of S frames).  Position n of frame t
// is coded when bits[b, t] > n (the mask rule of EPI_CODE), the coded bit is code > 0.5, a position without a bit decodes to 0.5.
// data (B, nseg, stride) bytes, sizes (B, nseg) int32, nseg = ceil(T / S); the first emitted byte (always 0) is not stored, trailing
// zeros are stripped, and the decoder reads 0 at or beyond `size` - so no read leaves a segment and no write its stride.
inline long long entropy_stride(int z_dim, long long segment) { return 2 * segment * z_dim + segment / 16 + 8; }
// The caller's stream of one receive call, resident in the call's workspace (like VbrCall: the step is captured once and replayed)
struct EntropyCall {
    const unsigned char *data;       // (B, nseg, stride)
    const int *sizes;                // (B, nseg); an entry outside [0, stride] reads as 0 bytes
    long long stride;
    int segment, nseg;
};
// The decode node of a frame (OP_ENTROPY_DECODE): p_t from DS_PROB, the row's bit count from DS_BITS, z_t to DS_CODES (natural
// (B,T,Z) floats); per row the coder's state - code, range, bytes consumed, unused - re-initialised where t % segment == 0
struct EntropyStep {
    const CallDesc *desc;
    const EntropyCall *call;
    unsigned *state;                 // [B][4]
    int B, Z;
};
int launch_entropy_set_call(EntropyCall *d, const EntropyCall &v, hipStream_t s);
int launch_entropy_decode_step(const EntropyStep &a, int tstep, hipStream_t s);
// the coder on given tensors: codes / prob (B,T,Z), bits (B,T) or null = bits_per_frame everywhere.  Encode clears data first; a segment
// that does not fit `stride` gets size -1
int launch_entropy_encode(const float *codes, const float *prob, const float *bits, float bits_per_frame, int B, long long T, int Z,
                          long long segment, unsigned char *data, long long stride, int *sizes, hipStream_t s);
int launch_entropy_decode(const unsigned char *data, long long stride, const int *sizes, const float *prob, const float *bits,
                          float bits_per_frame, int B, long long T, int Z, long long segment, float *codes, hipStream_t s);
// sel (B,T) = the bit count of every frame as the code epilogue's selector takes it: bits (or dflt where null), not below 0
int launch_entropy_bits(const float *bits, float dflt, long long n, float *sel, hipStream_t s);

// ------------------------------------------------------------------ vocoder (k_vocoder.hip; the AMP pairs: k_vocoder_amp.hip)
struct ConvLayer {               // one causal conv as implicit GEMM on fp32 MFMA
    int cin;                     // input channels (multiple of 4)
    int cout;                    // real output columns
    int ntiles;                  // ceil(cout/16)
    int ks;                      // taps
    int dil;
    const float *wp;             // packed B fragments [ks][cin/4][ntiles][64]
    const float *wp4;            // cin == cout, a multiple of 16, >= 32: [ks][cin/16][ntiles][64][4] - a lane's fragments of four consecutive k-steps as ONE
                                 // 16-byte granule (amp_pair_kernel's streamed weights: a quarter of the load instructions), else nullptr
    const float *wp2;            // cin == cout == 8 only: two-output-rows-per-tile form [ks+1][2][64] (amp_pair8_kernel), else nullptr
    const float *bias;           // [cout] (for ConvT: bias replicated per phase)
    const float *act_a;          // exp(alpha) per input channel or nullptr (no input activation)
    const float *act_ib;         // 1/(exp(beta)+1e-9)
    const float *aa_up;          // the input activation is anti-aliased (Activation1d): its 12-tap upsample.filter and
    const float *aa_down;        // downsample.lowpass.filter, else nullptr
};
enum ConvEpi { CE_STORE = 0, CE_RES = 1, CE_RES_ACC = 2, CE_RES_ACC_DIV = 3 };
// Streaming window: the tensors are (B, rows, C) buffers whose first rows are history; only rows from
// row_begin on are computed.  t_origin = global time of buffer row 0 (for the zero-before-start rule).
#ifdef BVC_PHASE_PROBE
int phase_probe_read(unsigned long long *out, int reset);   // debugging builds only (tools/phase_probe.py)
#endif
struct ConvWindow {
    long long in_bs, out_bs, row_begin, t_origin;
    // AMP pairs of a session whose rows start at different times: row b's t_origin is t_origin + age_rate * row_age[b] (device memory)
    const int *row_age = nullptr;
    int age_rate = 0;
    // a symmetric AMP pair in a look-ahead window: Lin ends the rows it may read, row_end <= Lin the rows it writes
    bool lookahead = false;
    long long row_end = 0;
};
// in (B, Lin, cin) channels-last; out (B, Lout, cout).  Output row r reads input rows
// r - (ks-1)*dil ... r  (rows outside [0,Lin) are zero).  res/acc have the layout of out.
int conv_kernels_init();
// stage-specific AMP kernels a launch may take (per model): C = 8 pairs on the two-rows-per-tile kernel, C = 16 pairs on the persistent
// kernel with swapped operands; without the bit the generic amp_pair_kernel runs (same bits)
enum : unsigned { AMPK_C8 = 1u, AMPK_C16 = 2u, AMPK_ALL = 3u };
unsigned amp_kernels_default();
// what the last launch_amp_pair of this process launched (tests): tiles that have work, workgroups in the grid (the generic kernel: the
// tiles padded to a multiple of 8, one tile each; the persistent C = 8 / C = 16 kernels: at most the device's slots, each walking over
// tiles), valid output rows per tile.  A launch that had nothing to do leaves the record alone.
struct AmpLaunch { long long tiles, workgroups; int tile_rows; };
extern AmpLaunch g_last_amp_launch;
int launch_snakebeta_test(const float *x, long long n, float a, float ib, float *y, hipStream_t s);
// row_lim (B) or nullptr: input rows of item b from row_lim[b] on read as zeros (a mixed-length batch; row_lim[b] <= Lin)
int launch_conv_mfma(const ConvLayer &c, const float *in, long long Lin, float *out, long long Lout,
                     int B, int epi, const float *res, const float *acc, float divisor, hipStream_t s,
                     const ConvWindow *win = nullptr, const long long *row_lim = nullptr,
                     long long in_bs = 0,      // floats between the input's batch items where that is not Lin * cin (offline: a symmetric stage's view)
                     int shift = 0);           // 3: conv_pre of a pre_sym generator, out[t] = b + sum_j w[j] in[t - 3 + j] (pad [3, 3]); offline
// one fused AMPBlock1 iteration: out = x + conv2(S2(conv1_dil(S1(x)))) (+acc, /divisor per epi); c2.dil == 1
// layers with aa_up / aa_down (both layers of a pair or none): S1 and S2 are anti-aliased, the generic kernel's AA form runs
// (valid rows per tile TR - (ks-1) - 10) and win must be null - the pair reads x[t - (ks-1)(d+1) - 10 .. t + 10]
int launch_amp_pair(const ConvLayer &c1, const ConvLayer &c2, const float *x, long long L, float *out, int B, int epi,
                    const float *acc, float divisor, hipStream_t s, const ConvWindow *win = nullptr, unsigned kernels = AMPK_ALL,
                    bool sym = false,         // symmetric pair (ks odd): the generic kernel's SYM form, out[t] reads x[t - h .. t + h], h = (ks-1)(d+1)/2;
                    long long bs = 0);        // win must be null or a look-ahead window.  bs: floats between the batch items of x / out / acc where that is not L * C
                                              // (sym only: the stage works on a view of the upsampler's rows; rows outside [0, L) read as zeros)
// SnakeBeta -> causal conv C->1 (k taps) -> tanh -> / div -> first n_out samples
// n_rows (B) or nullptr: item b keeps its first n_rows[b] samples, the rest of its n_out are 0
int launch_conv_post(const float *in, long long Lin, int C, int ks, const float *w, const float *bias,
                     const float *act_a, const float *act_ib, float div, float *wav, long long n_out,
                     int B, hipStream_t s, const ConvWindow *win = nullptr, const long long *n_rows = nullptr,
                     const float *aa_up = nullptr, const float *aa_down = nullptr,    // anti-aliased activation_post: offline, equal lengths
                     bool sym = false,         // post_sym: pad [3, 3], sample t reads rows t - 3 .. t + 3 (7 taps; offline, equal lengths, not filtered)
                     long long in_bs = 0);     // floats between the input's batch items where that is not Lin * C (offline)
// mixed-length decode: lim ((n_up + 1) x B) = per-item input rows of the upsamplers, L_0 = frames[b] (clamped into [0, T]),
// L_i = (L_{i-1} + 1) * up_rates[i-1], then the samples kept, min(lengths[b], L_{n_up}) clamped into [0, n_max] (0 without frames)
int launch_ragged_limits(long long *lim, const long long *frames, const long long *lengths, int B, long long T, long long n_max,
                         int n_up, const int *up_rates, hipStream_t s);

}  // namespace bvc
