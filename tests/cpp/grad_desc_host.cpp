// tests/cpp/grad_desc_host.cpp -- a host build of sfm-gms_amd/csrc/grad_desc_core.h for the CPU tests (tests/test_grad_desc_ref.py).
// The product library only runs grad_desc_core.h on the GPU; this exposes its steps to ctypes. With -DGRAD_DESC_MAIN it is a
// stand-alone program (its own main) for a sanitizer build: the saturated patch and the 33 x 33 image, rows summed to one number.
#include "grad_desc_core.h"

#include <stddef.h>

namespace gd = gms::gd;

extern "C" {

void gd_host_window_table(int32_t* out) { for (int r2 = 0; r2 <= gd::kR2; ++r2) out[r2] = gd::window_weight(r2); }
void gd_host_dir_table(int32_t* c, int32_t* s) { for (int b = 0; b < 32; ++b) { c[b] = gd::dir_c(b); s[b] = gd::dir_s(b); } }
int gd_host_max_cell_weight(void) { return gd::kMaxCellWeight; }
int gd_host_max_part(void) { return gd::kMaxPart; }

// the 5 x 5 box sums as the detector leaves them: 0 where the window leaves the image
void gd_host_box(const uint8_t* img, int w, int h, uint16_t* S)
{
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int sum = 0;
            if (x >= 2 && x < w - 2 && y >= 2 && y < h - 2)
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) sum += img[(size_t)(y + dy) * w + (x + dx)];
            S[(size_t)y * w + x] = (uint16_t)sum;
        }
}

// the detector's direction bin at (x, y) of an image: moments over the disc of radius 15
int gd_host_direction(const uint8_t* img, int w, int x, int y)
{
    int m10 = 0, m01 = 0;
    for (int dy = -15; dy <= 15; ++dy)
        for (int dx = -15; dx <= 15; ++dx)
            if (dx * dx + dy * dy <= 225) {
                const int v = img[(size_t)(y + dy) * w + (x + dx)];
                m10 += dx * v;
                m01 += dy * v;
            }
    return gd::direction_bin(m10, m01);
}

// rows [n][128] at (x, y, bin) triples; returns the number of keypoints refused (outside the keypoint region or a bad bin: row untouched)
int gd_host_rows(const uint16_t* S, int w, int h, const int32_t* xyb, int n, float* rows)
{
    int refused = 0;
    for (int k = 0; k < n; ++k) {
        const int x = xyb[3 * k], y = xyb[3 * k + 1], b = xyb[3 * k + 2];
        if (x < gd::kBorder || y < gd::kBorder || x >= w - gd::kBorder || y >= h - gd::kBorder || b < 0 || b > 31) {
            ++refused;
            continue;
        }
        gd::describe_row(S, w, x, y, b, rows + (size_t)k * gd::kDim);
    }
    return refused;
}
}

#ifdef GRAD_DESC_MAIN
#include <stdio.h>
#include <vector>

static double run_case(const std::vector<uint8_t>& img, int w, int h)
{
    std::vector<uint16_t> S((size_t)w * h);
    gd_host_box(img.data(), w, h, S.data());
    std::vector<int32_t> xyb;
    for (int y = gd::kBorder; y < h - gd::kBorder; ++y)
        for (int x = gd::kBorder; x < w - gd::kBorder; ++x)
            for (int b = 0; b < 32; ++b) { xyb.push_back(x); xyb.push_back(y); xyb.push_back(b); }
    const int n = (int)(xyb.size() / 3);
    std::vector<float> rows((size_t)n * gd::kDim);
    if (gd_host_rows(S.data(), w, h, xyb.data(), n, rows.data()) != 0) return -1.0;
    double sum = 0;
    for (float v : rows) sum += v;
    return sum;
}

int main()
{
    // 33 x 33 noise (one legal position) from a small generator, then a 35 x 35 patch of 0 / 255 steps: the largest gradients
    std::vector<uint8_t> noise(33 * 33), steps(35 * 35);
    uint32_t state = 12345u;
    for (auto& v : noise) { state = state * 1664525u + 1013904223u; v = (uint8_t)(state >> 24); }
    for (int y = 0; y < 35; ++y)
        for (int x = 0; x < 35; ++x) steps[(size_t)y * 35 + x] = ((x / 5 + y / 5) & 1) ? 255 : 0;
    const double a = run_case(noise, 33, 33), b = run_case(steps, 35, 35);
    printf("grad_desc_host: noise %.0f steps %.0f\n", a, b);
    return a > 0 && b > 0 ? 0 : 1;
}
#endif
