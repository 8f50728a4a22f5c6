// tests/test_cpp_dense_fuse_shim.py: mi355::fuseDense (sfm-gms_amd/include/mi355_gms.hpp) on the case of an input file, printing the
// counts on one line and FNV-1a checksums of: the points, the colours, the sources, the indices, the supports and the conflicts.
// Input: the format of tests/cpp/dense_fuse_host.cpp (header, neighbours, then per source its record, plan, view, registration, maps,
// points and colours). No arguments: prints usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

template <class T>
static bool get(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "dense_fuse_shim_main CASE.bin");
    if (!f) return 2;
    int32_t h[6];
    if (!get(f, h, 6) || h[0] < 1 || h[0] > 4096 || h[1] < 1 || h[1] > 32 || (h[2] != 1 && h[2] != 3)) return 2;
    const int n_src = h[0], n_nb = h[1], channels = h[2];
    std::vector<int32_t> nb((size_t)n_src * n_nb);
    if (!get(f, nb.data(), nb.size())) return 2;
    std::vector<mi355::FuseSource> src((size_t)n_src);
    for (mi355::FuseSource& s : src) {
        int32_t r[9];
        if (!get(f, r, 9) || !get(f, &s.plan, 1) || !get(f, &s.view, 1) || !get(f, &s.reg, 1)) return 2;
        if (r[0] < 1 || r[0] > 8192 || r[1] < 1 || r[1] > 8192 || r[4] < 0 || r[4] > (1 << 24)) return 2;
        const size_t px = (size_t)r[0] * (size_t)r[1], cap = (size_t)r[4];
        s.width = r[0], s.height = r[1];
        s.filtered16 = r[2], s.min_disp16 = r[3], s.count = r[5], s.has_view = r[7] != 0, s.has_reg = r[8] != 0;
        s.disp16.resize(px), s.valid.resize(px), s.points.resize(3 * cap), s.colors.resize(r[6] ? channels * cap : 0);
        if (!get(f, s.disp16.data(), px) || !get(f, s.valid.data(), px) || !get(f, s.points.data(), 3 * cap) || !get(f, s.colors.data(), s.colors.size()))
            return 2;
    }
    std::fclose(f);
    const mi355::FusedCloud c = mi355::fuseDense(src, channels, h[3], h[4], h[5], nb, n_nb);
    for (size_t i = 0; i < c.counts.size(); ++i) std::printf(i ? " %d" : "%d", c.counts[i]);
    std::printf("\n%llu\n%llu\n%llu\n%llu\n%llu\n%llu\n", fnv(c.points.data(), 4 * c.points.size()), fnv(c.colors.data(), c.colors.size()),
                fnv(c.source.data(), 4 * c.source.size()), fnv(c.index.data(), 4 * c.index.size()), fnv(c.support.data(), c.support.size()),
                fnv(c.conflict.data(), c.conflict.size()));
    return 0;
}
