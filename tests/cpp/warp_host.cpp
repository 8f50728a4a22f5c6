// tests/test_warp_ref.py: sfm-gms_amd/csrc/warp_core.h built for the host, so that the arithmetic the kernels run can be held against
// tests/warp_ref.py without a device. With -DWARP_HOST_MAIN: a stand-alone program (for a sanitizer run) that resizes and rotates
// a small noise image, at sizes that reach every clamp, and prints a checksum.
#include <cstdio>
#include <vector>

#include "warp_core.h"

extern "C" {

void warp_host_resize(const uint8_t* src, int sw, int sh, int channels, long long src_pitch, uint8_t* dst, int dw, int dh, long long dst_pitch)
{
    warp::resize_image(src, sw, sh, channels, src_pitch, dst, dw, dh, dst_pitch);
}

void warp_host_warp_affine(const uint8_t* src, int sw, int sh, int channels, long long src_pitch, const double* M, uint8_t* dst, int dw,
                           int dh, long long dst_pitch)
{
    warp::warp_affine_image(src, sw, sh, channels, src_pitch, M, dst, dw, dh, dst_pitch);
}

void warp_host_rotation_matrix(double cx, double cy, double angle, double scale, double* M) { warp::rotation_matrix_2d(cx, cy, angle, scale, M); }

void warp_host_invert(const double* F, double* M) { warp::invert_affine(F, M); }

int warp_host_args_ok(int n, int sw, int sh, int channels, long long src_pitch, int dw, int dh, long long dst_pitch)
{
    return warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) ? 1 : 0;
}

}  // extern "C"

#ifdef WARP_HOST_MAIN
int main()
{
    const int sw = 37, sh = 23, C = 3;
    std::vector<uint8_t> src((size_t)sw * sh * C);
    uint32_t s = 12345u;
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    unsigned long long sum = 0;
    const int sizes[][2] = {{1, 1}, {37, 23}, {130, 70}, {5, 4}, {74, 46}};
    for (const auto& d : sizes) {
        std::vector<uint8_t> dst((size_t)d[0] * d[1] * C);
        warp::resize_image(src.data(), sw, sh, C, sw * C, dst.data(), d[0], d[1], d[0] * C);
        for (uint8_t v : dst) sum = sum * 31 + v;
    }
    std::vector<uint8_t> half((size_t)18 * 11 * C);
    warp::resize_image(src.data(), 36, 22, C, sw * C, half.data(), 18, 11, 18 * C);   // the 2 x 2 mean, on a pitched source
    for (uint8_t v : half) sum = sum * 31 + v;
    const double angles[] = {0, 30, 90, 180, -75};
    for (double a : angles) {
        double M[6];
        warp::rotation_matrix_2d(sw / 2., sh / 2., a, a == -75 ? 0.6 : 1.0, M);
        std::vector<uint8_t> dst((size_t)50 * 40 * C);
        warp::warp_affine_image(src.data(), sw, sh, C, sw * C, M, dst.data(), 50, 40, 50 * C);
        for (uint8_t v : dst) sum = sum * 31 + v;
    }
    const double singular[6] = {1, 2, 3, 2, 4, 5}, far[6] = {1, 0, 1e7, 0, 1, -1e7};
    for (const double* M : {singular, far}) {
        std::vector<uint8_t> dst((size_t)9 * 7 * C);
        warp::warp_affine_image(src.data(), sw, sh, C, sw * C, M, dst.data(), 9, 7, 9 * C);
        for (uint8_t v : dst) sum = sum * 31 + v;
    }
    std::printf("warp_host: checksum %llu\n", sum);
    return 0;
}
#endif
