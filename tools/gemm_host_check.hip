// Host-only check of the batched GEMM's launch choices, for a sanitizer build (no GPU, no kernel is launched):
//     hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/gemm_host_check.hip -o tools/gemm_host_check
// Prints gemm_batched_cut over rows, column blocks, forced heights, both cut modes and the four states of the tail / quarter
// switches (one line per cut, for a line-by-line comparison of two builds), then walks the table of the LDS kernels: every
// (family, ACT, BM, ROWVEC) the launch can ask for resolves, and every entry's LDS size is what its kernel lays out.
// The batched source is included as text; what it needs from the rest of the library is stubbed here.
#include <cstdarg>
#include <cstdio>

#include "../bernoulli-var-speech-codec_amd/csrc/k_gemm_batched.hip"

namespace bvc {
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
ProbeScope::ProbeScope(int, hipStream_t stream) : s(stream), slot(-1) {}
ProbeScope::~ProbeScope() {}
}  // namespace bvc

int main() {
    using namespace bvc;
    int bad = 0, cuts = 0, entries = 0;
    for (bool no_tail : {false, true})
        for (bool no_q : {false, true})
            for (int M : {0, 1, 5, 111, 300, 11129, 27520, 55104, 110080, 1 << 22})
                for (int nb : {0, 1, 8, 24})
                    for (int force : {0, 100, 112, 128, 144})
                        for (bool legacy : {false, true}) {
                            const GemmCut c = gemm_batched_cut(M, nb * 128, force, legacy, no_tail, no_q);
                            ++cuts;
                            printf("cut no_tail=%d no_quarter=%d M=%d N=%d force=%d legacy=%d: height %d full_blocks %d tail_height %d tiles %lld rounds %lld cost100 %lld\n",
                                   (int)no_tail, (int)no_q, M, nb * 128, force, (int)legacy, c.height, c.full_blocks, c.tail_height, c.tiles, c.rounds, c.cost100);
                            if (c.height == 0) continue;
                            // what launch_batched_cut asks the table for with this cut
                            const int tail = c.tail_height == 32 ? 32 : 64;
                            for (int act : {0, 1})
                                for (bool rv : {false, true})
                                    if (!batched_kernel(legacy ? GF_LDS : GF_COLS, act, legacy ? 128 : c.height, rv) || !batched_kernel(GF_LDS, act, tail, rv)) {
                                        printf("no kernel for the cut above (act %d rowvec %d)\n", act, (int)rv); ++bad;
                                    }
                            if ((no_tail || (force && !legacy)) && c.tail_height != 0) { printf("a tail where none may be\n"); ++bad; }
                            if (c.tail_height == 0 && (long long)c.full_blocks * c.height < M) { printf("rows not covered\n"); ++bad; }
                        }
    for (const BatchedKernel &k : BATCHED_KERNELS) {
        ++entries;
        const size_t need = (size_t)2 * (k.bm + 128) * 36 * sizeof(float);        // [2][A BM x 36 | B 128 x 36] floats
        if (!k.fn || k.lds() != need || k.lds() > 160 * 1024 || batched_kernel(k.family, k.act, k.bm, k.rowvec) != &k) {
            printf("table entry family %d act %d bm %d rowvec %d: fn %p lds %zu (needs %zu)\n", k.family, k.act, k.bm, (int)k.rowvec, (void *)k.fn, k.lds(), need);
            ++bad;
        }
    }
    for (int fam : {GF_LDS, GF_COLS})
        for (int bm : {128, 64, 32, 144, 112})
            for (int act : {0, 1})
                for (bool rv : {false, true}) {
                    const bool compiled = fam == GF_LDS ? (bm == 128 || bm == 64 || bm == 32) : (bm == 144 || bm == 128 || bm == 112);
                    if ((batched_kernel(fam, act, bm, rv) != nullptr) != compiled) { printf("table: family %d bm %d act %d rowvec %d\n", fam, bm, act, (int)rv); ++bad; }
                }
    printf("gemm_host_check: %d cuts, %d table entries, %d failures\n", cuts, entries, bad);
    return bad != 0;
}
