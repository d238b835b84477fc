// Kernels of the backward pass (the program: backward.hip): the row-wise ones at the end of the file, and in front of them the weight
// gradient of a linear layer, dW[N][K] = sum over rows m of dY[m][n] * X[m][k]: an
// f32-in / f32-accumulate MFMA GEMM whose summed dimension is the ROW index of both operands, so both are read by rows from their
// natural layouts and nothing is transposed.
//
// One order of summation per output, a function of (M, N, K) alone - weight_grad_cut below:
//   * the M rows are cut into S chunks of `chunk_rows` rows (a multiple of WG_BLOCK; the last chunk takes what is left);
//   * inside a chunk the rows are taken in blocks of WG_BLOCK = 128: a block is ONE fmaf chain in row order from zero (the MFMA is a
//     k-ordered fmaf chain, 4 rows an instruction), and the block sums are added, in block order, to the chunk's sum;
//   * the chunk sums are added in chunk order, from zero (weight_grad_reduce_kernel), where S > 1.
// No atomics, no arrival order: two calls give the same bits.  The two levels are there for the error, not the speed: one chain over
// 11 000 rows wanders ~0.4 u M against a result of ~sqrt(M), blocks of 128 bring that to ~0.4 u (sqrt(128 M) + M / sqrt(128)).
#include "k_gemm.h"

namespace bvc {

namespace {

constexpr int WG_TILE = 64;           // output tile of a workgroup: 64 (n) x 64 (k), a 32 x 32 quarter per wave = 2 x 2 MFMA tiles
constexpr int WG_ROWS = 16;           // rows of dY / X staged per trip (4 MFMA steps of 4 rows)
constexpr int WG_LD = 80;             // LDS row stride in floats: the 4 rows a wave reads at once fall 16 banks apart
constexpr int WG_BLOCK = 128;         // rows per fmaf chain
constexpr int WG_MIN_CHUNK = 256;     // a chunk is worth a workgroup from here on
constexpr int WG_TARGET_WGS = 512;    // workgroups wanted where the output alone has fewer tiles (two per CU)

}  // namespace

WeightGradCut weight_grad_cut(int M, int N, int K) {
    const long long tiles = (long long)((N + WG_TILE - 1) / WG_TILE) * ((K + WG_TILE - 1) / WG_TILE);
    long long want = (WG_TARGET_WGS + tiles - 1) / tiles;
    const long long most = (M + WG_MIN_CHUNK - 1) / WG_MIN_CHUNK;
    if (want > most) want = most;
    if (want < 1) want = 1;
    long long rows = (M + want - 1) / want;
    rows = (rows + WG_BLOCK - 1) / WG_BLOCK * WG_BLOCK;
    WeightGradCut c;
    c.chunk_rows = (int)rows;
    c.chunks = (int)((M + rows - 1) / rows);
    c.ws_floats = c.chunks > 1 ? (size_t)c.chunks * N * K : 0;
    return c;
}

// grid (column tiles of K, row tiles of N, chunks); part: [chunk][N][ldo] (the result itself where there is one chunk)
__global__ __launch_bounds__(256) void weight_grad_kernel(const float *__restrict__ dY, const float *__restrict__ X, int M, int N, int K,
                                                          int chunk_rows, float *__restrict__ part, long long ldo, long long part_stride) {
    __shared__ float sA[WG_ROWS * WG_LD], sB[WG_ROWS * WG_LD];
    const int k0 = blockIdx.x * WG_TILE, n0 = blockIdx.y * WG_TILE;
    const int m_lo = blockIdx.z * chunk_rows;
    const int m_hi = min(M, m_lo + chunk_rows);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (wave >> 1) * 32, kw = (wave & 1) * 32;
    // staging: thread -> row tid / 16 of the trip, floats 4 (tid % 16) .. + 3 of the tile's 64 columns (N and K are multiples of 16: a
    // float4 is inside the matrix or outside it as a whole)
    const int lr = tid >> 4, lc = (tid & 15) * 4;
    const bool a_in = n0 + lc < N, b_in = k0 + lc < K;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int m, float4 &va, float4 &vb) {
        va = zero4; vb = zero4;
        if (m + lr < m_hi) {          // rows behind the chunk read as zeros
            if (a_in) va = *reinterpret_cast<const float4 *>(dY + (long long)(m + lr) * N + n0 + lc);
            if (b_in) vb = *reinterpret_cast<const float4 *>(X + (long long)(m + lr) * K + k0 + lc);
        }
    };
    f32x4 tot[2][2], acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) { tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float4 va, vb;
    fetch(m_lo, va, vb);
    const int fr = lane >> 4, fc = lane & 15;       // operand lane map of v_mfma_f32_16x16x4_f32: summed index lane / 16, the other lane % 16
    for (int m = m_lo; m < m_hi; m += WG_ROWS) {
        __syncthreads();                              // the last trip's operand reads are through
        *reinterpret_cast<float4 *>(sA + lr * WG_LD + lc) = va;
        *reinterpret_cast<float4 *>(sB + lr * WG_LD + lc) = vb;
        __syncthreads();
        if (m + WG_ROWS < m_hi) fetch(m + WG_ROWS, va, vb);       // the next trip's rows, in flight under the products
#pragma unroll
        for (int q = 0; q < WG_ROWS / 4; ++q) {
            const float *ra = sA + (q * 4 + fr) * WG_LD + nw + fc;
            const float *rb = sB + (q * 4 + fr) * WG_LD + kw + fc;
            const float a0 = ra[0], a1 = ra[16], b0 = rb[0], b1 = rb[16];
            acc[0][0] = mfma16(a0, b0, acc[0][0]);
            acc[0][1] = mfma16(a0, b1, acc[0][1]);
            acc[1][0] = mfma16(a1, b0, acc[1][0]);
            acc[1][1] = mfma16(a1, b1, acc[1][1]);
        }
        if ((m - m_lo + WG_ROWS) % WG_BLOCK == 0 || m + WG_ROWS >= m_hi) {      // a block's chain ends: its sum joins the chunk's
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) { tot[i][j] += acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
    }
    // C/D lane map: column lane % 16 (k), rows 4 (lane / 16) + register (n)
    float *out = part + (long long)blockIdx.z * part_stride;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + kw + j * 16 + fc;
            if (k >= K) continue;
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + nw + i * 16 + fr * 4 + r;
                if (n < N) out[(long long)n * ldo + k] = tot[i][j][r];
            }
        }
}

// out[row][col] = part[0][i] + part[1][i] + ... in chunk order, i = row * K + col
__global__ void weight_grad_reduce_kernel(const float *__restrict__ part, int chunks, long long n, int K, long long ldo, float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int c = 0; c < chunks; ++c) v += part[(long long)c * n + i];
        out[i / K * ldo + i % K] = v;
    }
}

// dW (N, K) = dY (M, N)^T X (M, K), overwritten.  ws: weight_grad_cut(M, N, K).ws_floats floats (unused where that is 0).  All three
// matrices natural, 16-byte aligned, dY and X dense; N and K multiples of 16.  ldo: the row stride of dW (0: K) - a column block of a
// wider gradient, for a layer over a concatenated input.
int launch_weight_grad(const float *dY, const float *X, int M, int N, int K, float *dW, float *ws, hipStream_t s, long long ldo) {
    if (!ldo) ldo = K;
    if (M < 1 || N < 16 || K < 16 || N % 16 || K % 16) { set_error("weight gradient: M = %d, N = %d, K = %d (N and K multiples of 16)", M, N, K); return BVC_EINVAL; }
    const WeightGradCut c = weight_grad_cut(M, N, K);
    if (c.chunks > 1 && !ws) { set_error("weight gradient: no workspace for %d chunks", c.chunks); return BVC_EINVAL; }
    const dim3 grid((K + WG_TILE - 1) / WG_TILE, (N + WG_TILE - 1) / WG_TILE, c.chunks);
    hipLaunchKernelGGL(weight_grad_kernel, grid, dim3(256), 0, s, dY, X, M, N, K, c.chunk_rows, c.chunks > 1 ? ws : dW,
                       c.chunks > 1 ? (long long)K : ldo, (long long)N * K);
    BVC_HIP_TRY(hipGetLastError());
    if (c.chunks > 1) {
        const long long n = (long long)N * K;
        const long long blocks = (n + 255) / 256;
        hipLaunchKernelGGL(weight_grad_reduce_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, ws, c.chunks, n, K, ldo, dW);
        BVC_HIP_TRY(hipGetLastError());
    }
    return BVC_OK;
}

// ---- row-wise kernels of the reverse recurrence ------------------------------------------------------------------------------
// Every matrix natural; "frame-major" rows are t * B + b, "utterance-major" rows b * T + t (the caller's tensors).
namespace {

int blocks_for(long long total) {
    const long long blocks = (total + 255) / 256;
    return (int)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}

#define BWD_LOOP(i, total) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

// the taped activations: T fragment-packed [mt16][n] matrices, `fstride` floats apart -> frame-major rows
__global__ void unpack_frames_kernel(const float *__restrict__ src, long long fstride, long long T, int B, int n, float *__restrict__ dst) {
    const long long total = T * B * n;
    BWD_LOOP(i, total) {
        const int c = (int)(i % n);
        const long long r = i / n;
        const int b = (int)(r % B);
        dst[i] = src[(r / B) * fstride + packed_off(b, c, n)];
    }
}

// utterance-major <-> frame-major rows; dir 0: dst frame-major.  scale (may be null): the element is divided by scale[column]
__global__ void reorder_rows_kernel(const float *__restrict__ src, int B, long long T, int n, float *__restrict__ dst, int dir,
                                    const float *__restrict__ scale) {
    const long long total = T * B * n;
    BWD_LOOP(i, total) {
        const int c = (int)(i % n);
        const long long r = i / n;                       // frame-major row
        const long long u = (r % B) * T + r / B;         // the same row, utterance-major
        const float v = dir == 0 ? src[u * n + c] : src[i];
        (dir == 0 ? dst[i] : dst[u * n + c]) = scale ? v / scale[c] : v;
    }
}

// (R, C) -> (C, R)
__global__ void transpose_kernel(const float *__restrict__ src, int R, int C, float *__restrict__ dst) {
    const long long total = (long long)R * C;
    BWD_LOOP(i, total) dst[(i % C) * R + i / C] = src[i];
}

// ELU from its output: out = dy * (y > 0 ? 1 : y + 1)   (out may be dy)
__global__ void elu_bwd_kernel(const float *dy, const float *__restrict__ y, float *out, long long total) {
    BWD_LOOP(i, total) {
        const float v = y[i];
        out[i] = dy[i] * (v > 0.0f ? 1.0f : v + 1.0f);
    }
}

// d dec_t = the caller's gradient of frame t (utterance-major tensor) + what the generated-feature path sends back through
// (d - mean) / std (gdn, may be null)
__global__ void mel_bwd_kernel(const float *__restrict__ gdec, long long T, long long t, const float *__restrict__ gdn,
                               const float *__restrict__ stdv, int B, int X, float *__restrict__ out) {
    BWD_LOOP(i, (long long)B * X) {
        const int c = (int)(i % X);
        const long long b = i / X;
        float v = gdec[(b * T + t) * X + c];
        if (gdn) v += gdn[i] / stdv[c];
        out[i] = v;
    }
}

// s = sigmoid(x) and s1 = 1 - s = sigmoid(-x), each to its own relative precision: 1 - s taken from the rounded s loses it where the
// unit saturates (an ulp of s against 1 - s), and s s1 is the derivative every gradient behind a saturated unit is scaled by
__device__ __forceinline__ void sigmoid_pair(float x, float &s, float &s1) {
    const float t = expf(-fabsf(x));
    const float big = 1.0f / (1.0f + t), small = t / (1.0f + t);
    s = x >= 0.0f ? big : small;
    s1 = x >= 0.0f ? small : big;
}

// Frame t of the sampler and the KLD (bvrnn.py:124-129,148-157), back to the two logits xe, xq (B, Z) (computed again from the tape:
// the forward keeps the probabilities only).  z = mask * (round(.) - e.detach() + e) + 0.5 (1 - mask): d z / d e = mask.
// kld = mean_t mean_b sum_j mask * ke: scale = g_kld / (T B).  torch.clip(x, 1e-3) passes the gradient where x >= 1e-3 (the boundary
// included).
__global__ void code_bwd_kernel(const float *__restrict__ gz, const float *__restrict__ xe, const float *__restrict__ xq,
                                const float *__restrict__ bits, long long T, long long t, int B, int Z, float scale,
                                float *__restrict__ d_enc_logit, float *__restrict__ d_prior_logit) {
    BWD_LOOP(i, (long long)B * Z) {
        const int j = (int)(i % Z);
        const long long b = i / Z;
        const float mask = (!bits || bits[b * T + t] > (float)j) ? 1.0f : 0.0f;
        float e, e1, q, q1;
        sigmoid_pair(xe[i], e, e1);
        sigmoid_pair(xq[i], q, q1);
        const float c = 1e-3f;
        const float ce = fmaxf(e, c), cq = fmaxf(q, c), ce1 = fmaxf(e1, c), cq1 = fmaxf(q1, c);
        // d ke / d e = [log ce - log ce1] - [log cq - log cq1] + ([e >= c] e / ce - [e1 >= c] e1 / ce1).  Where nothing is clipped the
        // brackets are the logits themselves and the last term is 1 - 1: written as such, because ke is nearly flat where enc_t is near
        // prior_t, and four rounded logarithms of 0.5 and a "+ 1 - 1" in float32 then cost five digits of a small difference.
        const float le = (e >= c && e1 >= c) ? xe[i] : logf(ce) - logf(ce1);
        const float lq = (q >= c && q1 >= c) ? xq[i] : logf(cq) - logf(cq1);
        const float de_kld = (le - lq) + ((e >= c ? e / ce : 0.0f) - (e1 >= c ? e1 / ce1 : 0.0f));
        // d ke / d prior, times prior (1 - prior): -e q1 [q >= c] q / cq + e1 q [q1 >= c] q1 / cq1, = q - e where nothing is clipped
        const float dq_logit = (q >= c && q1 >= c) ? q - e : (q1 >= c ? e1 * q * (q1 / cq1) : 0.0f) - (q >= c ? e * q1 * (q / cq) : 0.0f);
        const float g = scale * mask;
        d_enc_logit[i] = (gz[i] * mask + g * de_kld) * e * e1;
        d_prior_logit[i] = g * dq_logit;
    }
}

// The GRU cell (PyTorch's: r, z, n gates; h' = (h - n) z + n) from its recomputed gate sums gi = W_ih x + b_ih, gh = W_hh h + b_hh
// (B, 3H) and the gradient of h': d gi, d gh (B, 3H) and the direct term dh' z (B, H)
__global__ void gru_bwd_kernel(const float *__restrict__ dhn, const float *__restrict__ gi, const float *__restrict__ gh,
                               const float *__restrict__ h, int B, int H, float *__restrict__ dgi, float *__restrict__ dgh,
                               float *__restrict__ dh_direct) {
    BWD_LOOP(i, (long long)B * H) {
        const int c = (int)(i % H);
        const long long b = i / H, o = b * 3 * H + c;
        float r, r1, z, z1;
        sigmoid_pair(gi[o] + gh[o], r, r1);
        sigmoid_pair(gi[o + H] + gh[o + H], z, z1);
        const float ghn = gh[o + 2 * H];
        const float an = gi[o + 2 * H] + r * ghn;
        const float n = tanhf(an);
        const float tn = expf(-2.0f * fabsf(an));
        const float sech2 = 4.0f * tn / ((1.0f + tn) * (1.0f + tn));          // 1 - tanh^2, to its own relative precision
        const float d = dhn[i];
        const float dan = d * z1 * sech2;
        const float daz = d * (h[i] - n) * z * z1;
        const float dar = dan * ghn * r * r1;
        dgi[o] = dar; dgi[o + H] = daz; dgi[o + 2 * H] = dan;
        dgh[o] = dar; dgh[o + H] = daz; dgh[o + 2 * H] = dan * r;
        dh_direct[i] = d * z;
    }
}

// bias gradient: the column sums of dY (M, N), rows in blocks of WG_BLOCK as the weight gradient takes them
__global__ void col_sum_kernel(const float *__restrict__ dY, int M, int N, float *__restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float tot = 0.0f;
    for (int m0 = 0; m0 < M; m0 += WG_BLOCK) {
        float acc = 0.0f;
        const int m1 = min(M, m0 + WG_BLOCK);
        for (int m = m0; m < m1; ++m) acc += dY[(long long)m * N + n];
        tot += acc;
    }
    out[n] = tot;
}

}  // namespace

#define BWD_LAUNCH(kernel, total, ...)                                                              \
    do {                                                                                            \
        if ((total) <= 0) return BVC_OK;                                                            \
        hipLaunchKernelGGL(kernel, dim3(blocks_for(total)), dim3(256), 0, s, __VA_ARGS__);          \
        BVC_HIP_TRY(hipGetLastError());                                                             \
        return BVC_OK;                                                                              \
    } while (0)

int launch_unpack_frames(const float *src, long long fstride, long long T, int B, int n, float *dst, hipStream_t s) {
    BWD_LAUNCH(unpack_frames_kernel, T * B * n, src, fstride, T, B, n, dst);
}
int launch_reorder_rows(const float *src, int B, long long T, int n, float *dst, int dir, const float *scale, hipStream_t s) {
    BWD_LAUNCH(reorder_rows_kernel, T * B * n, src, B, T, n, dst, dir, scale);
}
int launch_transpose(const float *src, int R, int C, float *dst, hipStream_t s) {
    BWD_LAUNCH(transpose_kernel, (long long)R * C, src, R, C, dst);
}
int launch_elu_bwd(const float *dy, const float *y, float *out, long long total, hipStream_t s) {
    BWD_LAUNCH(elu_bwd_kernel, total, dy, y, out, total);
}
int launch_mel_bwd(const float *gdec, long long T, long long t, const float *gdn, const float *stdv, int B, int X, float *out, hipStream_t s) {
    BWD_LAUNCH(mel_bwd_kernel, (long long)B * X, gdec, T, t, gdn, stdv, B, X, out);
}
int launch_code_bwd(const float *gz, const float *xe, const float *xq, const float *bits, long long T, long long t, int B, int Z,
                    float scale, float *d_enc_logit, float *d_prior_logit, hipStream_t s) {
    BWD_LAUNCH(code_bwd_kernel, (long long)B * Z, gz, xe, xq, bits, T, t, B, Z, scale, d_enc_logit, d_prior_logit);
}
int launch_gru_bwd(const float *dhn, const float *gi, const float *gh, const float *h, int B, int H, float *dgi, float *dgh, float *dh_direct,
                   hipStream_t s) {
    BWD_LAUNCH(gru_bwd_kernel, (long long)B * H, dhn, gi, gh, h, B, H, dgi, dgh, dh_direct);
}
int launch_col_sum(const float *dY, int M, int N, float *out, hipStream_t s) {
    if (M <= 0 || N <= 0) return BVC_OK;
    hipLaunchKernelGGL(col_sum_kernel, dim3((N + 255) / 256), dim3(256), 0, s, dY, M, N, out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
