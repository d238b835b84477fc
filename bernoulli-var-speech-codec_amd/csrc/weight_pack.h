// The host arithmetic that decides every bit the kernels read from a model: the re-layouts of the weights into MFMA fragment order, the
// float64 fold of dec.6 -> norm -> phi_x.0, the SnakeBeta parameters, the sparse rows of the mel bank and the front end's tables.
// Pure functions of their arguments: no HIP header, no bvc_model, any host C++17 compiler (model_build.hip uploads what they return;
// tools/model_image_check.hip checks the re-layouts against the layout comments below).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace bvc {

// Linear weight W[N][K] (row-major) -> MFMA B-operand fragment order [N/16][K/16][lane][4]:
// lane = ((k%16)/4)*16 + n%16 holds W[n][k..k+3]; one (n-tile, k-block) pair is 1 KiB contiguous.
inline std::vector<float> pack_linear(const float *W, int N, int K) {
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
inline std::vector<float> pack_gru_interleaved(const float *W, int H, int K) {
    std::vector<float> p((size_t)3 * H * K);
    const int nb = K / 16;
    for (int q = 0; q < 3; ++q)
        for (int n = 0; n < H; ++n)
            for (int k = 0; k < K; ++k)
                p[(((((size_t)(n >> 4) * nb + (k >> 4)) * 3 + q) * 64 + ((k & 15) >> 2) * 16 + (n & 15)) << 2) + (k & 3)] =
                    W[((size_t)q * H + n) * K + k];
    return p;
}

// Conv1d weight W[cout][cin][ks] -> MFMA B fragments [ks][cin/4][ntiles][64]: lane l of tile nt holds W[nt*16 + l%16][cg*4 + l/16][j]
// (zero where the column is beyond cout)
inline std::vector<float> pack_conv(const float *W, int cout, int cin, int ks) {
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
inline std::vector<float> pack_conv_k4(const float *W, int cout, int cin, int ks) {
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
inline std::vector<float> pack_conv_two_rows(const float *W, int ks) {
    std::vector<float> p((size_t)(ks + 1) * 2 * 64, 0.0f);
    for (int k = 0; k <= ks; ++k)
        for (int cg = 0; cg < 2; ++cg)
            for (int l = 0; l < 64; ++l) {
                const int n = l & 15, pr = n >> 3, co = n & 7, ci = cg * 4 + (l >> 4), j = k - pr;
                if (j >= 0 && j < ks) p[((size_t)k * 2 + cg) * 64 + l] = W[((size_t)co * 8 + ci) * ks + j];
            }
    return p;
}

// ConvTranspose1d weight W[cin][cout][2u] -> 2-tap conv with u*cout columns (polyphase form): column p*cout + co, [ncol][cin][2]
inline std::vector<float> convt_as_conv(const float *W, int cin, int cout, int u) {
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

// px0_dec3: W = phi_x.0.W diag(1/std) dec.6.W  (H x H),  b = phi_x.0.W ((dec.6.b - mean) / std) + phi_x.0.b, in float64
// wp0 [H][X], bp0 [H]: phi_x.0;  wd6 [X][H], bd6 [X]: dec.6;  w [H][H] (natural), b [H]
struct FoldedLinear { std::vector<float> w, b; };
inline FoldedLinear fold_px0_dec3(const float *wp0, const float *bp0, const float *wd6, const float *bd6, const float *mean,
                                  const float *stdv, int H, int X) {
    FoldedLinear f{std::vector<float>((size_t)H * H), std::vector<float>((size_t)H)};
    std::vector<double> row((size_t)H);
    for (int n = 0; n < H; ++n) {
        std::fill(row.begin(), row.end(), 0.0);
        double b = (double)bp0[n];
        for (int j = 0; j < X; ++j) {
            const double g = (double)wp0[(size_t)n * X + j] / (double)stdv[j];
            b += g * ((double)bd6[j] - (double)mean[j]);
            const float *wr = wd6 + (size_t)j * H;
            for (int k = 0; k < H; ++k) row[k] += g * (double)wr[k];
        }
        for (int k = 0; k < H; ++k) f.w[(size_t)n * H + k] = (float)row[k];
        f.b[n] = (float)b;
    }
    return f;
}

// SnakeBeta's log-scale parameters as the kernels take them: a = exp(alpha), ib = 1 / (exp(beta) + 1e-9)
inline void snake_params(const float *alpha, const float *beta, int n, std::vector<float> *a, std::vector<float> *ib) {
    a->resize((size_t)n);
    ib->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        (*a)[i] = (float)std::exp((double)alpha[i]);                   // torch.exp(alpha)
        const float eb = (float)std::exp((double)beta[i]);
        (*ib)[i] = 1.0f / (eb + 0.000000001f);                         // activations.py:116
    }
}

// The mel bank [num_mels][nbins] as sparse rows: filter j is len[j] weights from bin start[j] on, at w[off[j]] (an empty filter:
// start 0, len 0); kmax = the highest bin with a non-zero weight, plus one (at least 1)
struct MelRows { std::vector<int> start, len, off; std::vector<float> w; int kmax; };
inline MelRows compact_mel_bank(const float *bank, int num_mels, int nbins) {
    MelRows r{std::vector<int>(num_mels), std::vector<int>(num_mels), std::vector<int>(num_mels), {}, 1};
    for (int j = 0; j < num_mels; ++j) {
        const float *row = bank + (size_t)j * nbins;
        int lo = -1, hi = -1;
        for (int k = 0; k < nbins; ++k)
            if (row[k] != 0.0f) { if (lo < 0) lo = k; hi = k; }
        if (lo < 0) { lo = 0; hi = -1; }
        r.start[j] = lo; r.len[j] = hi - lo + 1; r.off[j] = (int)r.w.size();
        for (int k = lo; k <= hi; ++k) r.w.push_back(row[k]);
        if (hi + 1 > r.kmax) r.kmax = hi + 1;
    }
    return r;
}

const double PACK_PI = 3.14159265358979323846;

// the periodic Hann window a checkpoint without "hann_window" gets
inline std::vector<float> hann_window(int nfft) {
    std::vector<float> win((size_t)nfft);
    for (int n = 0; n < nfft; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PACK_PI * n / nfft));
    return win;
}

// The front end's twiddles as interleaved (cos, sin) floats, the bytes of the kernels' float2 tables:
// tw1 [8][64] W_512^(lane*k0), tw2 [8][8] W_64^(n0*k1), tws [nbins] e^{-2 pi i k / 1024}
struct Twiddles { std::vector<float> tw1, tw2, tws; };
inline Twiddles fft_twiddles(int nbins) {
    Twiddles t{std::vector<float>(2 * 8 * 64), std::vector<float>(2 * 64), std::vector<float>(2 * (size_t)nbins)};
    auto put = [](std::vector<float> &v, size_t i, double a) { v[2 * i] = (float)std::cos(a); v[2 * i + 1] = (float)std::sin(a); };
    for (int k = 0; k < 8; ++k)
        for (int l = 0; l < 64; ++l) put(t.tw1, (size_t)k * 64 + l, -2.0 * PACK_PI * (double)(l * k) / 512.0);
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) put(t.tw2, (size_t)k * 8 + n, -2.0 * PACK_PI * (double)(n * k) / 64.0);
    for (int k = 0; k < nbins; ++k) put(t.tws, (size_t)k, -2.0 * PACK_PI * (double)k / 1024.0);
    return t;
}

}  // namespace bvc
