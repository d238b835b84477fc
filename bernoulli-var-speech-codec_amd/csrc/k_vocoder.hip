// Causal-tiny BigVGAN kernels for gfx950.
//
// Every convolution of the generator (conv_pre models.py:212-213, the four ConvTranspose1d
// upsamplers :216-217, the 72 AMPBlock1 convolutions :103-121) runs through ONE kernel template:
// a causal 1-D convolution written as an implicit GEMM on the fp32-input MFMA
// (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation):
//
//      out[t, co] = bias[co] + sum_{j<ks} sum_{ci} W[co, ci, j] * act(in[t - (ks-1-j)*dil, ci])
//      M = 16 time steps, N = 16 output channels, K = 4 input channels of one tap.
//
// Activations live in HBM channels-last (B, L, C), so a time tile plus its causal halo is ONE
// contiguous span: it is loaded with coalesced float4 reads, SnakeBeta (activations.py:107-120) is
// applied on the way in, and the tile is parked in LDS with a row stride of C+2 floats, which
// makes the MFMA A-operand reads (16 rows x 4 channels per instruction) bank-conflict free.
// B operands (weights) are pre-packed on the host in MFMA fragment order, so every weight fetch is
// one coalesced 256-B read that stays L1/L2 resident.  The epilogue fuses bias, the AMP residual
// add, the running sum over the three parallel resblocks and the final /3 (models.py:219-225).
//
// A ConvTranspose1d with kernel 2*stride is the same kernel: its polyphase form
//      out[q*u + p, co] = b[co] + sum_ci in[q, ci] W[ci, co, p] + in[q-1, ci] W[ci, co, p+u]
// is a 2-tap causal convolution with u*Cout output columns whose (B, Lin+1, u*Cout) result IS the
// (B, (Lin+1)*u, Cout) channels-last signal.
#include "k_vocoder.h"

namespace bvc {

struct ConvArgs {
    const float *in;  long long Lin;
    float *out;       long long Lout;
    long long in_bs, out_bs;      // floats between consecutive batch items of in / out (res, acc like out)
    long long row_begin;          // first output row to compute (rows before it are history: streaming)
    const float *res; const float *acc;
    const float *wp;  const float *bias;
    const float *act_a; const float *act_ib;
    float divisor;
    int epi, ks, dil, cout, ntiles, tiles_per_batch;
    const long long *row_lim;     // (B) input rows of each batch item (mixed-length batches), or nullptr: Lin for all
};

// CIN: input channels; NTW: 16-column tiles per wave; MT: 16-row tiles per wave.  The four waves of a workgroup split the
// rows (each wave MT row tiles x the same NTW column tiles) or, NSPLIT, the columns (all waves the same MT row tiles, each its
// own NTW column tiles): the second form is for streaming hops, whose one or two new frames are a handful of rows.
// SHIFT: the input window starts SHIFT rows later - conv_pre of a pre_sym generator pads [3, 3] instead of [6, 0] (models.py:209-213),
// out[t] = b + sum_j w[j] in[t - (ks-1) + SHIFT + j]; rows behind the input's end are zeros like the rows before its start.
template <int CIN, int NTW, int MT, bool NSPLIT = false, int SHIFT = 0>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int S = CIN + 2;                 // LDS row stride (floats): (S/2) odd -> conflict-free
    constexpr int TT = (NSPLIT ? 1 : 4) * MT * 16;   // output rows per workgroup
    constexpr int C4 = CIN / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.tiles_per_batch;
    const long long t0 = a.row_begin + (long long)(blockIdx.x % a.tiles_per_batch) * TT;
    const int ntile0 = NSPLIT ? (blockIdx.y * 4 + wave) * NTW : blockIdx.y * NTW;
    const int halo = (a.ks - 1) * a.dil;
    const int rows = TT + halo;
    const long long lin = a.row_lim ? a.row_lim[b] : a.Lin;       // (uniform: one scalar load per workgroup at most)

    // ---- stage the activated input span [t0-halo, t0+TT) in LDS
    const float *inb = a.in + (long long)b * a.in_bs;
    for (int idx = tid; idx < rows * C4; idx += 256) {
        const int row = idx / C4, c4 = idx - row * C4;
        const long long tg = t0 - halo + SHIFT + row;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (tg >= 0 && tg < lin) {
            v = *reinterpret_cast<const f32x4 *>(inb + tg * CIN + c4 * 4);
            if (a.act_a) {
                const f32x4 aa = *reinterpret_cast<const f32x4 *>(a.act_a + c4 * 4);
                const f32x4 bb = *reinterpret_cast<const f32x4 *>(a.act_ib + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2 o2 = snakebeta2((f32x2){v[e], v[e + 1]}, (f32x2){aa[e], aa[e + 1]}, (f32x2){bb[e], bb[e + 1]});
                    v[e] = o2[0]; v[e + 1] = o2[1];
                }
            }
        }
        park16<S>(tile, row, c4 * 4, v);
    }
    __syncthreads();

    f32x4 acc[MT][NTW];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NTW; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int mbase = NSPLIT ? 0 : wave * MT * 16;
    const float *wl = a.wp + (long long)ntile0 * 64 + lane;
    const long long kstride = (long long)a.ntiles * 64;          // floats per k-step in the packed weights
    bool nok[NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) nok[n] = (ntile0 + n) < a.ntiles;

    for (int j = 0; j < a.ks; ++j) {
        const float *arow = tile + (mbase + r + j * a.dil) * S + g;
        const float *wj = wl + (long long)j * C4 * kstride;
        constexpr int CGU = (C4 % 8 == 0) ? 8 : (C4 % 5 == 0) ? 5 : (C4 % 4 == 0) ? 4 : (C4 % 2 == 0) ? 2 : 1;
#pragma unroll 1
        for (int cg0 = 0; cg0 < C4; cg0 += CGU) {
            float bw[CGU][NTW];
#pragma unroll
            for (int u = 0; u < CGU; ++u)
#pragma unroll
                for (int n = 0; n < NTW; ++n)
                    bw[u][n] = nok[n] ? wj[(long long)(cg0 + u) * kstride + n * 64] : 0.0f;
#pragma unroll
            for (int u = 0; u < CGU; ++u) {
                float av[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) av[i] = arow[i * 16 * S + (cg0 + u) * 4];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int n = 0; n < NTW; ++n)
                        acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[u][n], av[i], acc[i][n], 0, 0, 0);      // tile of out^T (below)
            }
        }
    }

    // ---- epilogue.  The operands are swapped (weights as A, activations as B), so acc[i][n][e] = out[row mbase+16i+r][col 16(ntile0+n)+4g+e]:
    // a lane's four results are four consecutive channels of one output row - one 16-byte store (cout is a multiple of 4).
    const long long ob = (long long)b * a.out_bs;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const long long t = t0 + mbase + i * 16 + r;
        if (t >= a.Lout) continue;
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            const int col = (ntile0 + n) * 16 + g * 4;
            if (col >= a.cout) continue;
            const long long o = ob + t * a.cout + col;
            f32x4 v = acc[i][n] + *reinterpret_cast<const f32x4 *>(a.bias + col);
            if (a.epi >= CE_RES) v = v + *reinterpret_cast<const f32x4 *>(a.res + o);        // x = xt + x      (models.py:119)
            if (a.epi >= CE_RES_ACC) v = *reinterpret_cast<const f32x4 *>(a.acc + o) + v;    // xs += resblock  (models.py:224)
            divide_if(a.epi == CE_RES_ACC_DIV, v, a.divisor);                                // xs / num_kernels (models.py:225)
            *reinterpret_cast<f32x4 *>(a.out + o) = v;
        }
    }
}

template <int CIN, int NTW, int MT, bool NSPLIT = false, int SHIFT = 0>
static int launch_one(const ConvArgs &a, int B, hipStream_t s) {
    constexpr int TT = (NSPLIT ? 1 : 4) * MT * 16;
    ConvArgs k = a;
    k.tiles_per_batch = (int)((a.Lout - a.row_begin + TT - 1) / TT);
    if (k.tiles_per_batch <= 0) return BVC_OK;
    const size_t lds = (size_t)(TT + (a.ks - 1) * a.dil) * (CIN + 2) * sizeof(float);
    if (lds > 160 * 1024) { set_error("conv tile needs %zu B of LDS", lds); return BVC_EINVAL; }
    constexpr int NPW = NTW * (NSPLIT ? 4 : 1);            // column tiles per workgroup
    dim3 grid((unsigned)(k.tiles_per_batch * (long long)B), (unsigned)((a.ntiles + NPW - 1) / NPW));
    auto kern = conv_mfma_kernel<CIN, NTW, MT, NSPLIT, SHIFT>;
    ProbeScope probe(PK_CONV, s);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, k);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// Allow > 64 KiB of dynamic LDS for every instantiation (called once from bvc_model_create, so the
// compute entry points stay free of non-stream API calls).
template <int CIN, int NTW, int MT, bool NSPLIT = false, int SHIFT = 0>
static int allow_big_lds() {
    BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(conv_mfma_kernel<CIN, NTW, MT, NSPLIT, SHIFT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return BVC_OK;
}

// test helper: y[i] = SnakeBeta(x[i]) with one (exp(alpha), 1/(exp(beta)+1e-9)) pair, through the same device functions the
// generator uses: the packed form on elements 4k, 4k+1, the scalar form on 4k+2, 4k+3
__global__ void snakebeta_test_kernel(const float *__restrict__ x, long long n, float a, float ib, float *__restrict__ y) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < n; i += (long long)gridDim.x * blockDim.x * 2) {
        if (i + 1 < n && !(i & 2)) {
            const f32x2 v = snakebeta2((f32x2){x[i], x[i + 1]}, splat2(a), splat2(ib));
            y[i] = v[0];
            y[i + 1] = v[1];
        } else {
            y[i] = snakebeta(x[i], a, ib);
            if (i + 1 < n) y[i + 1] = snakebeta(x[i + 1], a, ib);
        }
    }
}

int launch_snakebeta_test(const float *x, long long n, float a, float ib, float *y, hipStream_t s) {
    if (n <= 0) return BVC_OK;
    hipLaunchKernelGGL(snakebeta_test_kernel, dim3(256), dim3(256), 0, s, x, n, a, ib, y);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int conv_kernels_init() {
    int rc;
    if ((rc = amp_kernels_init())) return rc;
    if ((rc = allow_big_lds<512, 4, 1>())) return rc;
    if ((rc = allow_big_lds<512, 4, 1, true>())) return rc;
    if ((rc = allow_big_lds<256, 4, 2>())) return rc;
    if ((rc = allow_big_lds<256, 4, 1, true>())) return rc;
    if ((rc = allow_big_lds<128, 4, 2>())) return rc;
    if ((rc = allow_big_lds<80, 4, 2>())) return rc;
    if ((rc = allow_big_lds<80, 4, 2, false, 3>())) return rc;
    if ((rc = allow_big_lds<64, 4, 2>())) return rc;
    if ((rc = allow_big_lds<32, 2, 4>())) return rc;
    if ((rc = allow_big_lds<16, 1, 4>())) return rc;
    if ((rc = allow_big_lds<8, 1, 4>())) return rc;
    return BVC_OK;
}

int launch_conv_mfma(const ConvLayer &c, const float *in, long long Lin, float *out, long long Lout, int B,
                     int epi, const float *res, const float *acc, float divisor, hipStream_t s, const ConvWindow *win,
                     const long long *row_lim, long long in_bs, int shift) {
    if (B <= 0 || Lout <= 0) return BVC_OK;
    if (c.cout % 4) { set_error("conv_mfma: %d output columns (the epilogue stores 16-byte granules)", c.cout); return BVC_EINVAL; }
    ConvArgs a;
    a.in = in; a.Lin = Lin; a.out = out; a.Lout = Lout; a.res = res; a.acc = acc;
    a.in_bs = win ? win->in_bs : (in_bs ? in_bs : Lin * c.cin);
    a.out_bs = win ? win->out_bs : Lout * c.cout;
    a.row_begin = win ? win->row_begin : 0;
    a.wp = c.wp; a.bias = c.bias; a.act_a = c.act_a; a.act_ib = c.act_ib;
    a.divisor = divisor; a.epi = epi; a.ks = c.ks; a.dil = c.dil; a.cout = c.cout; a.ntiles = c.ntiles;
    a.tiles_per_batch = 0;
    a.row_lim = row_lim;
    if (shift) {                                            // conv_pre of a pre_sym generator: the 7-tap window centred, offline
        if (shift != 3 || c.cin != 80 || c.ks != 7 || c.dil != 1 || win || row_lim) { set_error("conv_mfma: a shifted window is conv_pre's (80 channels, 7 taps, shift 3)"); return BVC_EINVAL; }
        return launch_one<80, 4, 2, false, 3>(a, B, s);
    }
    // streaming hops: one or two new frames = at most 16 rows in front of the first two upsamplers; the row-split tiles (64 rows
    // and more per workgroup) would compute mostly rows nobody reads, so the waves split the columns instead
    if (win && Lout - a.row_begin <= 16) {
        switch (c.cin) {
            case 512: return launch_one<512, 4, 1, true>(a, B, s);
            case 256: return launch_one<256, 4, 1, true>(a, B, s);
            case 128: return launch_one<128, 4, 1, true>(a, B, s);
            case 80:  return launch_one<80, 2, 1, true>(a, B, s);
            case 64:  return launch_one<64, 4, 1, true>(a, B, s);
            default: break;
        }
    }
    switch (c.cin) {
        case 512: return launch_one<512, 4, 1>(a, B, s);     // ConvT 512->8x256: 64 rows (65 x 514 floats = 133.6 KB; 128 rows would need 265 KB)
        case 256: return launch_one<256, 4, 2>(a, B, s);     // ConvT 256->8x128 (129 x 258 floats = 133.1 KB)
        case 128: return launch_one<128, 4, 2>(a, B, s);     // ConvT 128->8x64
        case 80:  return launch_one<80, 4, 2>(a, B, s);      // conv_pre 80->128
        case 64:  return launch_one<64, 4, 2>(a, B, s);      // AMP C=64, ConvT 64->8x32
        case 32:  return launch_one<32, 2, 4>(a, B, s);      // AMP C=32, ConvT 32->2x16
        case 16:  return launch_one<16, 1, 4>(a, B, s);      // AMP C=16, ConvT 16->2x8
        case 8:   return launch_one<8, 1, 4>(a, B, s);       // AMP C=8
        default:
            set_error("conv_mfma: unsupported input channel count %d", c.cin);
            return BVC_EINVAL;
    }
}

// ------------------------------------------------------------------------------------------------
// activation_post -> pad[6,0] -> conv_post (C -> 1) -> tanh -> [:length] -> / SCALING
// (models.py:228-238, bvrnn_codec_model.py:71).  VALU kernel: C*ks = 56 MACs per sample (C = 8; 112 / 224 behind a generator of
// 256 / 512 initial channels, whose last stage has 16 / 32 channels).
// SHIFT: the window starts SHIFT rows later (post_sym pads [3, 3], models.py:230-233); rows behind the last read as zeros either way.
template <int C, int SHIFT = 0>
__global__ __launch_bounds__(256) void conv_post_kernel(const float *__restrict__ in, long long Lin, int ks,
                                                        const float *__restrict__ w, const float *__restrict__ bias,
                                                        const float *__restrict__ act_a,
                                                        const float *__restrict__ act_ib, float div,
                                                        float *__restrict__ wav, long long n_out,
                                                        int tiles_per_batch, long long in_bs, long long row_begin,
                                                        const long long *__restrict__ n_rows) {
    extern __shared__ __attribute__((aligned(16))) float tile[];     // [(256 + ks-1)][C]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_batch;
    const long long t0 = row_begin + (long long)(blockIdx.x % tiles_per_batch) * 256;     // input row of output 0 of the tile
    const int halo = ks - 1;
    const float *inb = in + (long long)b * in_bs;
    for (int idx = tid; idx < (256 + halo) * C; idx += 256) {
        const int row = idx / C, c = idx - row * C;
        const long long tg = t0 - halo + SHIFT + row;
        float v = 0.0f;
        if (tg >= 0 && tg < Lin) v = snakebeta(inb[tg * C + c], act_a[c], act_ib[c]);
        tile[idx] = v;
    }
    __syncthreads();
    const long long t = t0 + tid - row_begin;                        // output sample index
    if (t >= n_out) return;
    if (n_rows && t >= n_rows[b]) { wav[(long long)b * n_out + t] = 0.0f; return; }       // behind a mixed-length batch item's end
    float acc = 0.0f;
    for (int j = 0; j < ks; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) acc = fmaf(w[c * ks + j], tile[(tid + j) * C + c], acc);
    wav[(long long)b * n_out + t] = tanhf(acc + bias[0]) / div;
}

// The same with an anti-aliased activation_post (antialias_post): the raw rows [t0 - (ks-1) - 5, t0 + 256 + 5) are parked first and
// aa_rows turns them into the tile the conv reads (rows before time 0 zero, the signal's ends replicated).
template <int C>
__global__ __launch_bounds__(256) void conv_post_aa_kernel(const float *__restrict__ in, long long Lin, int ks,
                                                           const float *__restrict__ w, const float *__restrict__ bias,
                                                           const float *__restrict__ act_a, const float *__restrict__ act_ib,
                                                           const float *__restrict__ fu, const float *__restrict__ fd, float div,
                                                           float *__restrict__ wav, long long n_out, int tiles_per_batch) {
    extern __shared__ __attribute__((aligned(16))) float tile[];     // [(256 + ks-1)][C] activated, then [(256 + ks-1 + 10)][C] raw
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_batch;
    const long long t0 = (long long)(blockIdx.x % tiles_per_batch) * 256;
    const int halo = ks - 1, nact = 256 + halo, nraw = nact + 10;
    float *raw = tile + nact * C;
    const float *inb = in + (long long)b * Lin * C;
    const int first = (int)(t0 - halo) - 5;
    for (int idx = tid; idx < nraw * C; idx += 256) {
        const long long tg = first + idx / C;
        raw[idx] = (tg >= 0 && tg < Lin) ? inb[tg * C + (idx % C)] : 0.0f;
    }
    __syncthreads();
    aa_rows<C>(raw, first, nraw, Lin, tile, first + 5, nact, C, act_a, act_ib, fu, fd);
    __syncthreads();
    const long long t = t0 + tid;
    if (t >= n_out) return;
    float acc = 0.0f;
    for (int j = 0; j < ks; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) acc = fmaf(w[c * ks + j], tile[(tid + j) * C + c], acc);
    wav[(long long)b * n_out + t] = tanhf(acc + bias[0]) / div;
}

int launch_conv_post(const float *in, long long Lin, int C, int ks, const float *w, const float *bias,
                     const float *act_a, const float *act_ib, float div, float *wav, long long n_out, int B,
                     hipStream_t s, const ConvWindow *win, const long long *n_rows, const float *aa_up, const float *aa_down,
                     bool sym, long long in_bs) {
    if (B <= 0 || n_out <= 0) return BVC_OK;
    if (C != 8 && C != 16 && C != 32) { set_error("conv_post: unsupported channel count %d", C); return BVC_EINVAL; }
    const int tiles = (int)((n_out + 255) / 256);
    if (aa_up || aa_down) {
        if (sym || in_bs) { set_error("conv_post: an anti-aliased activation_post stands in front of a causal conv_post, on a dense signal"); return BVC_EINVAL; }
        if (!aa_up || !aa_down || win || n_rows) { set_error("conv_post: an anti-aliased activation_post has no streaming window and no mixed lengths"); return BVC_EINVAL; }
        if (Lin + 512 > 0x7FFFFFFFll) { set_error("conv_post: %lld rows are beyond the anti-aliased kernel's row index", Lin); return BVC_EINVAL; }
        const size_t lds_aa = (size_t)(2 * (256 + ks - 1) + 10) * C * sizeof(float);
        ProbeScope probe(PK_POST, s);
        auto kern = C == 8 ? conv_post_aa_kernel<8> : C == 16 ? conv_post_aa_kernel<16> : conv_post_aa_kernel<32>;
        if (C == 32) {                                         // (2 x 262 + 10) x 32 floats = 68 KB
            static bool attr = false;
            if (!attr) { BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(conv_post_aa_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * (long long)B)), dim3(256), lds_aa, s, in, Lin, ks,
                           w, bias, act_a, act_ib, aa_up, aa_down, div, wav, n_out, tiles);
        BVC_HIP_TRY(hipGetLastError());
        return BVC_OK;
    }
    const size_t lds = (size_t)(256 + ks - 1) * C * sizeof(float);
    if (sym && (win || n_rows || ks != 7)) { set_error("conv_post: a symmetric conv_post has 7 taps, no streaming window and no mixed lengths"); return BVC_EINVAL; }
    ProbeScope probe(PK_POST, s);
    // causal and symmetric form: the same launch (a symmetric conv_post has no window), the kernel with its window 3 rows later
    auto kern = sym ? (C == 8 ? conv_post_kernel<8, 3> : C == 16 ? conv_post_kernel<16, 3> : conv_post_kernel<32, 3>)
                    : (C == 8 ? conv_post_kernel<8> : C == 16 ? conv_post_kernel<16> : conv_post_kernel<32>);
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * (long long)B)), dim3(256), lds, s, in, Lin, ks,
                       w, bias, act_a, act_ib, div, wav, n_out, tiles, win ? win->in_bs : (in_bs ? in_bs : Lin * C), win ? win->row_begin : 0, n_rows);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// Per-item bounds of a mixed-length decode (one thread per item).  Item b alone would run the generator on frames[b] frames: its
// upsampler i reads L_i rows, L_0 = frames[b], L_{i+1} = (L_i + 1) * u_i, and row L_i (one past its end, which the equal-length
// batch holds another frame in) must read as zero.  Everything else in the generator is causal, so those rows below the bound are
// already the item's own.
struct UpRates { int u[8]; };
__global__ void ragged_limits_kernel(long long *__restrict__ lim, const long long *__restrict__ frames,
                                     const long long *__restrict__ lengths, int B, long long T, long long n_max, int n_up, UpRates r) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long f = frames[b] < 0 ? 0 : (frames[b] > T ? T : frames[b]);
    long long L = f;
    for (int i = 0; i < n_up; ++i) {
        lim[(long long)i * B + b] = L;
        L = (L + 1) * r.u[i];
    }
    long long n = lengths[b] < L ? lengths[b] : L;
    n = f == 0 ? 0 : (n < 0 ? 0 : (n > n_max ? n_max : n));
    lim[(long long)n_up * B + b] = n;
}

int launch_ragged_limits(long long *lim, const long long *frames, const long long *lengths, int B, long long T, long long n_max,
                         int n_up, const int *up_rates, hipStream_t s) {
    if (B <= 0) return BVC_OK;
    if (n_up > 8) { set_error("ragged limits: %d upsamplers", n_up); return BVC_EINVAL; }
    UpRates r;
    for (int i = 0; i < 8; ++i) r.u[i] = i < n_up ? up_rates[i] : 0;
    hipLaunchKernelGGL(ragged_limits_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lim, frames, lengths, B, T, n_max, n_up, r);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}
}  // namespace bvc
