// Host-only check of the vocoder's launch choices, for a sanitizer build (no GPU, no kernel is launched):
//     hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/amp_host_check.hip -o tools/amp_host_check
// amp_pair_cut over lengths, batches, taps and forced heights, and the (ks, dilation) dispatcher amp_shape over the generator's nine
// pairs and pairs it does not have.  The AMP source is included as text; what it needs from the rest of the library is stubbed here.
#include <cstdarg>
#include <cstdio>

#include "../bernoulli-var-speech-codec_amd/csrc/k_vocoder_amp.hip"

namespace bvc {
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
ProbeScope::ProbeScope(int, hipStream_t stream) : s(stream), slot(-1) {}
ProbeScope::~ProbeScope() {}
bool tile_cut_legacy() { return false; }
void tile_trace(const char *, long long, long long, int, int, long long, int, long long) {}
}  // namespace bvc

int main() {
    using namespace bvc;
    int bad = 0, cuts = 0;
    for (long long L : {0ll, 1ll, 5ll, 117ll, 118ll, 3448ll, 1000003ll})
        for (int B : {0, 1, 3, 64})
            for (int ks : {3, 7, 11})
                for (int force : {0, 64, 80, 96, 112, 128})
                    for (bool legacy : {false, true}) {
                        const TilePlan p = amp_pair_cut(L, B, ks, force, legacy);
                        ++cuts;
                        const bool none = L <= 0 || B <= 0 || force == 64;
                        if (none != (p.height == 0)) { printf("cut L=%lld B=%d ks=%d force=%d: height %d\n", L, B, ks, force, p.height); ++bad; }
                        if (p.height && (p.tiles != B * ((L + p.height - ks) / (p.height - (ks - 1))) || (force && p.height != force))) {
                            printf("cut L=%lld B=%d ks=%d force=%d: height %d tiles %lld\n", L, B, ks, force, p.height, p.tiles); ++bad;
                        }
                    }
    int seen = 0;
    for (int ks : {3, 7, 11})
        for (int d : {1, 3, 5}) {
            const int got = amp_shape(ks, d, [](auto ks_c, auto d_c) { return decltype(ks_c)::value * 100 + decltype(d_c)::value; });
            if (got != ks * 100 + d) { printf("amp_shape(%d, %d) = %d\n", ks, d, got); ++bad; }
            ++seen;
        }
    for (int ks : {0, 5, 9, 13})
        for (int d : {1, 2, 7})
            if (amp_shape(ks, d, [](auto, auto) { return 0; }) != -1) { printf("amp_shape(%d, %d) found a shape\n", ks, d); ++bad; }
    if (amp_shape(7, 2, [](auto, auto) { return 0; }) != -1 || amp_shape(11, 0, [](auto, auto) { return 0; }) != -1) { printf("amp_shape took an unsupported dilation\n"); ++bad; }
    if (!amp_shapes_all([](auto, auto) { return 1; }) || amp_shapes_all([](auto ks_c, auto) { return decltype(ks_c)::value == 7 ? -1 : 1; })) { printf("amp_shapes_all\n"); ++bad; }
    printf("amp_host_check: %d cuts, %d shapes, %d failures\n", cuts, seen, bad);
    return bad != 0;
}
