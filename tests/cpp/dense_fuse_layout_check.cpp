// tests/test_dense_fuse_ref.py: the fusion's record and workspace as plain arithmetic, no device: gms_dense_fuse_src's layout (what
// types.DENSE_FUSE_SRC_DTYPE assumes) and ws_layout.h's DenseFuseLayout swept over sizes for order, overlap, alignment and size.
// Prints "dense_fuse_layout: ok" or the first violation.
#include <cstddef>
#include <cstdio>

#include "ws_layout.h"

static int fail(const char* what, int a, int b)
{
    std::printf("dense_fuse_layout: %s at %d %d\n", what, a, b);
    return 1;
}

int main()
{
    static_assert(sizeof(gms_dense_fuse_src) == 88 && offsetof(gms_dense_fuse_src, d_valid) == 8 && offsetof(gms_dense_fuse_src, d_plan) == 16 &&
                      offsetof(gms_dense_fuse_src, d_xyz) == 24 && offsetof(gms_dense_fuse_src, d_color) == 32 &&
                      offsetof(gms_dense_fuse_src, d_count) == 40 && offsetof(gms_dense_fuse_src, d_view) == 48 &&
                      offsetof(gms_dense_fuse_src, d_reg) == 56 && offsetof(gms_dense_fuse_src, width) == 64 &&
                      offsetof(gms_dense_fuse_src, filtered16) == 72 && offsetof(gms_dense_fuse_src, cap) == 80,
                  "gms_dense_fuse_src: eight pointers, then width, height, filtered16, min_disp16, cap, reserved");
    const int caps[] = {1, 2, 1023, 1024, 1025, 4097, 266240, 1 << 20, 8192 * 8192};
    for (int cap : caps)
        for (int n : {1, 2, 3, 33, 31}) {
            if ((long long)n * cap > 2147483647LL) continue;
            const size_t nb = (size_t)gms::dense_fuse_blocks(cap);
            if (nb * gms::kFuseBlockPoints < (size_t)cap || (nb - 1) * gms::kFuseBlockPoints >= (size_t)cap) return fail("blocks", cap, n);
            const gms::DenseFuseLayout L = gms::dense_fuse_layout(n, cap);
            if (L.blocks != 0 || L.marks < L.blocks + 4 * nb * n || L.total < L.marks + 2 * nb * n * gms::kFuseBlockPoints) return fail("order", cap, n);
            if (L.marks % 256 || L.total % 256) return fail("alignment", cap, n);
            if (L.total > 4 * nb * n + 2 * nb * n * gms::kFuseBlockPoints + 512) return fail("size", cap, n);
        }
    std::printf("dense_fuse_layout: ok\n");
    return 0;
}
