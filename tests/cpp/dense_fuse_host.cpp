// tests/test_dense_fuse_ref.py: sfm-gms_amd/csrc/dense_fuse_core.h built for the host as a stand-alone program, so that the arithmetic
// the kernels run can be held against tests/dense_fuse_ref.py without a device, plain and under sanitizers.
//   dense_fuse_host IN OUT
// IN (little endian): int32 n_src, n_nb, channels, tol16, min_support, fused_cap; int32 neighbors [n_src][n_nb]; then per source
//   int32 width, height, filtered16, min_disp16, cap, count, has_color, has_view, has_reg; gms_rectify_plan; gms_sfm_view;
//   gms_sfm_pair_reg; int16 disp16 [height][width]; uint8 valid [height][width]; float xyz [cap][3]; uint8 color [cap][channels]
//   when has_color.
// OUT: int32 counts [n_src + 1]; with k = min(total, fused_cap): float xyz [k][3]; uint8 color [k][channels]; int32 source [k],
//   index [k]; uint8 support [k], conflict [k].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_fuse_core.h"

namespace {

struct Held {
    gms_rectify_plan plan;
    gms_sfm_view view;
    gms_sfm_pair_reg reg;
    int32_t count;
    std::vector<int16_t> disp;
    std::vector<uint8_t> valid, color;
    std::vector<float> xyz;
};

template <class T>
bool get(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
bool put(FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[6];
    if (!get(f, h, 6)) return 4;
    const int n_src = h[0], n_nb = h[1], channels = h[2], tol16 = h[3], min_support = h[4], fused_cap = h[5];
    if (n_src < 1 || n_src > 4096 || n_nb < 1 || n_nb > fuse::kMaxNeighbors || (channels != 1 && channels != 3) || fused_cap < 0) return 5;
    std::vector<int32_t> nb((size_t)n_src * n_nb);
    if (!get(f, nb.data(), nb.size())) return 4;
    std::vector<Held> held((size_t)n_src);
    std::vector<gms_dense_fuse_src> src((size_t)n_src);
    long long max_cap = 1;
    for (int i = 0; i < n_src; ++i) {
        int32_t s[9];
        Held& H = held[(size_t)i];
        if (!get(f, s, 9) || !get(f, &H.plan, 1) || !get(f, &H.view, 1) || !get(f, &H.reg, 1)) return 4;
        if (s[0] < 1 || s[0] > rect::kMaxSide || s[1] < 1 || s[1] > rect::kMaxSide || s[4] < 0 || s[4] > (1 << 24)) return 5;
        const size_t px = (size_t)s[0] * (size_t)s[1], cap = (size_t)s[4];
        H.disp.resize(px), H.valid.resize(px), H.xyz.resize(3 * cap + 3), H.color.resize(s[6] ? channels * cap + 1 : 1);
        H.count = s[5];
        if (!get(f, H.disp.data(), px) || !get(f, H.valid.data(), px) || !get(f, H.xyz.data(), 3 * cap) ||
            (s[6] && !get(f, H.color.data(), channels * cap)))
            return 4;
        src[(size_t)i] = {H.disp.data(), H.valid.data(), &H.plan, H.xyz.data(), s[6] ? H.color.data() : nullptr, &H.count, s[7] ? &H.view : nullptr,
                          s[8] ? &H.reg : nullptr, s[0], s[1], s[2], s[3], s[4], 0};
        if (s[4] > max_cap) max_cap = s[4];
    }
    std::fclose(f);
    if (!fuse::call_args_ok(n_src, max_cap, n_nb, channels, tol16, min_support, fused_cap)) return 6;
    const size_t cap = (size_t)fused_cap;
    std::vector<float> xyz(3 * cap + 1);
    std::vector<uint8_t> color(channels * cap + 1), support(cap + 1), conflict(cap + 1);
    std::vector<int32_t> source(cap + 1), index(cap + 1), counts((size_t)n_src + 1);
    fuse::fuse_host(src.data(), n_src, max_cap, nb.data(), n_nb, channels, tol16, min_support, fused_cap, xyz.data(), color.data(), source.data(),
                    index.data(), support.data(), conflict.data(), counts.data());
    const size_t k = (size_t)(counts[(size_t)n_src] < fused_cap ? counts[(size_t)n_src] : fused_cap);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 3;
    const bool ok = put(o, counts.data(), counts.size()) && put(o, xyz.data(), 3 * k) && put(o, color.data(), channels * k) && put(o, source.data(), k) &&
                    put(o, index.data(), k) && put(o, support.data(), k) && put(o, conflict.data(), k);
    return std::fclose(o) == 0 && ok ? 0 : 7;
}
