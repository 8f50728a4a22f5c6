// tests/test_cpp_dense_shim.py: the dense stage's records and workspaces as plain arithmetic, no device: gms_rectify_plan's layout
// (what types.RECTIFY_PLAN_DTYPE and tests/rectify_ref.py assume), and ws_layout.h's DenseCloudLayout / DensePairsLayout swept over
// sizes for order, overlap, alignment and size. Prints "dense_layout: ok" or the first violation.
#include <cstddef>
#include <cstdio>

#include "ws_layout.h"

static int fail(const char* what, int a, int b, int c)
{
    std::printf("dense_layout: %s at %d %d %d\n", what, a, b, c);
    return 1;
}

int main()
{
    static_assert(sizeof(gms_rectify_plan) == 200 && offsetof(gms_rectify_plan, R2) == 72 && offsetof(gms_rectify_plan, fx) == 144 &&
                      offsetof(gms_rectify_plan, B) == 176 && offsetof(gms_rectify_plan, out_w) == 184 && offsetof(gms_rectify_plan, status) == 196,
                  "gms_rectify_plan: R1, R2, fx, fy, cx, cy, B, out_w, out_h, turn, status");
    const int sides[] = {1, 2, 19, 31, 32, 33, 70, 1023, 1024, 1025, 8192};
    for (int w : sides)
        for (int h : sides)
            for (int n : {1, 3, 65535}) {
                const int nb = gms::dense_cloud_blocks(w, h);
                if ((size_t)nb * gms::kDenseScanBlock < (size_t)w * h || ((size_t)nb - 1) * gms::kDenseScanBlock >= (size_t)w * h) return fail("blocks", w, h, n);
                const gms::DenseCloudLayout c = gms::dense_cloud_layout(n, w, h);
                if (c.blocks != 0 || c.total < 4 * (size_t)n * nb || c.total % 256) return fail("cloud layout", w, h, n);
                for (int ch : {1, 3}) {
                    const size_t sgm = 4096 + 256 * (size_t)(w % 7);
                    const gms::DensePairsLayout p = gms::dense_pairs_layout(n, w, h, ch, h, w, sgm);
                    const size_t grey = ch == 3 ? 2 * (size_t)n * w * h : 0;
                    if (p.grey != 0 || p.sgm < p.grey + grey || p.cloud < p.sgm + sgm || p.total < p.cloud + gms::dense_cloud_layout(n, h, w).total)
                        return fail("pairs layout order", w, h, n);
                    if (p.sgm % 256 || p.cloud % 256 || p.total % 256) return fail("pairs layout alignment", w, h, n);
                }
            }
    std::printf("dense_layout: ok\n");
    return 0;
}
