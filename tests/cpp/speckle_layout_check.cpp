// tests/test_speckle_ref.py: the speckle filter's workspaces as plain arithmetic, no device: ws_layout.h's SpeckleLayout and
// DensePairsFilteredLayout swept over sizes for order, overlap, alignment and size, and the tile constants of speckle_core.h.
// Prints "speckle_layout: ok" or the first violation.
#include <cstddef>
#include <cstdio>

#include "speckle_core.h"
#include "ws_layout.h"

static int fail(const char* what, int a, int b, int c)
{
    std::printf("speckle_layout: %s at %d %d %d\n", what, a, b, c);
    return 1;
}

int main()
{
    static_assert(spk::kTileW <= 128 && spk::kTileH <= 64 && (spk::kTileW & (spk::kTileW - 1)) == 0 && spk::kTilePx % spk::kBlock == 0,
                  "a tile of at most 128 x 64, a power-of-two width, whole rounds of the workgroup");
    static_assert(spk::kTilePx * 10 <= 64 * 1024, "values, labels and sizes of a tile fit the LDS of a workgroup");
    const int sides[] = {1, 2, 63, 64, 65, 131, 1920, 8192};
    for (int w : sides)
        for (int h : sides)
            for (int n : {1, 3, 8, 65535}) {
                const size_t px = (size_t)n * (size_t)w * (size_t)h;
                const gms::SpeckleLayout L = gms::speckle_layout(n, w, h);
                if (L.label != 0 || L.size < L.label + 4 * px || L.total < L.size + 4 * px) return fail("order", w, h, n);
                if (L.size % 256 || L.total % 256) return fail("alignment", w, h, n);
                if (L.total > 8 * px + 512) return fail("size", w, h, n);
                if (n > 8) continue;
                for (int channels : {1, 3}) {
                    const size_t sgm = 4096 + 77;
                    const gms::DensePairsLayout P = gms::dense_pairs_layout(n, w, h, channels, w, h, sgm);
                    const gms::DensePairsFilteredLayout F = gms::dense_pairs_filtered_layout(n, w, h, channels, w, h, sgm);
                    if (F.pairs.grey != P.grey || F.pairs.sgm != P.sgm || F.pairs.cloud != P.cloud || F.pairs.total != P.total)
                        return fail("the unfiltered regions moved", w, h, n);
                    if (F.speckle < P.total || F.speckle % 256 || F.total < F.speckle + L.total || F.total > P.total + L.total + 512)
                        return fail("the filter's region", w, h, n);
                }
            }
    std::printf("speckle_layout: ok\n");
    return 0;
}
