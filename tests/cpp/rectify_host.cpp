// tests/test_rectify_ref.py: sfm-gms_amd/csrc/rectify_core.h built for the host, so that the arithmetic the kernels run can be held
// against tests/rectify_ref.py without a device. With -DRECTIFY_HOST_MAIN: a stand-alone program (for a sanitizer run) that plans,
// rectifies and reprojects a small noise image under poses that throw taps outside on every side, and prints a checksum.
#include <cstdio>
#include <vector>

#include "rectify_core.h"

extern "C" {

void rectify_host_plan(const gms_camera* cam, const double* R, const double* t, int W, int H, int out_w, int out_h, gms_rectify_plan* plan)
{
    rect::make_plan(rect::camera_of(*cam), R, t, W, H, out_w, out_h, *plan);
}

void rectify_host_identity_plan(const gms_camera* cam, int W, int H, gms_rectify_plan* plan) { rect::identity_plan(rect::camera_of(*cam), W, H, *plan); }

void rectify_host_q(const gms_rectify_plan* plan, double* Q) { rect::plan_q(*plan, Q); }

// out [dh][dw][5]: ix, iy, fx, fy, front
void rectify_host_positions(const gms_camera* cam, const gms_rectify_plan* plan, int which, int dw, int dh, int32_t* out)
{
    const rect::Camera c = rect::camera_of(*cam);
    const double* Rk = which == 2 ? plan->R2 : plan->R1;
    for (int v = 0; v < dh; ++v)
        for (int u = 0; u < dw; ++u) {
            double row[3], col[3];
            rect::row_terms(Rk, rect::norm_coord(v, plan->cy, plan->fy), row);
            rect::col_terms(Rk, rect::norm_coord(u, plan->cx, plan->fx), col);
            rect::Src s = {0, 0, 0, 0, 0};
            if (plan->status == GMS_OK) s = rect::source_pos(c, col, row);
            int32_t* o = out + ((long long)v * dw + u) * 5;
            o[0] = s.ix, o[1] = s.iy, o[2] = s.fx, o[3] = s.fy, o[4] = s.front;
        }
}

void rectify_host_image(const gms_camera* cam, const gms_rectify_plan* plan, int which, const uint8_t* src, int sw, int sh, int channels,
                        long long src_pitch, uint8_t* dst, int dw, int dh, long long dst_pitch, uint8_t* valid)
{
    rect::rectify_image(src, sw, sh, channels, src_pitch, rect::camera_of(*cam), *plan, which, dst, dw, dh, dst_pitch, valid);
}

// the points of one map in raster order, the first cap written; returns the count of all
int rectify_host_cloud(const int16_t* disp, const uint8_t* valid, int W, int H, const gms_rectify_plan* plan, int filtered16, int min_disp16,
                       const double* S, const gms_sfm_view* view, int cap, float* xyz, int32_t* pixel)
{
    int n = 0;
    if (plan->status != GMS_OK) return 0;
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const long long i = (long long)v * W + u;
            if (!rect::is_point(disp[i], filtered16, min_disp16, valid[i])) continue;
            if (n < cap) {
                rect::cloud_point(*plan, u, v, disp[i], S, view, xyz + 3 * n);
                pixel[n] = (int32_t)i;
            }
            ++n;
        }
    return n;
}

}  // extern "C"

#ifdef RECTIFY_HOST_MAIN
int main()
{
    const int sw = 37, sh = 23, C = 3;
    std::vector<uint8_t> src((size_t)sw * sh * C);
    uint32_t s = 12345u;
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    const gms_camera cam = {40.0, 41.0, 18.2, 11.1, 0.1, -0.05, 0.01, -0.02, 0.03};
    const double c = 0.984807753012208, sn = 0.17364817766693033;   // 10 degrees
    const double poses[][12] = {
        {1, 0, 0, 0, 1, 0, 0, 0, 1, -1, 0, 0},       {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.3, 1, 0.1},   {c, -sn, 0, sn, c, 0, 0, 0, 1, 1, 0.2, 0.3},
        {c, 0, sn, 0, 1, 0, -sn, 0, c, -1, 0.5, -0.4}, {1, 0, 0, 0, c, -sn, 0, sn, c, 0, -1, 0.2}, {-1, 0, 0, 0, -1, 0, 0, 0, 1, 1, 0, 0},
        {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0, 1},      {1e300, 0, 0, 0, 1e300, 0, 0, 0, 1, 1e300, 0, 0}};
    unsigned long long sum = 0;
    for (const auto& p : poses) {
        gms_rectify_plan plan;
        rect::make_plan(rect::camera_of(cam), p, p + 9, sw, sh, 0, 0, plan);
        sum = sum * 31 + (unsigned)plan.status + (unsigned)plan.turn;
        const int dw = plan.status == GMS_OK ? plan.out_w + 3 : 9, dh = plan.status == GMS_OK ? plan.out_h + 2 : 7;
        for (int which = 1; which <= 2; ++which) {
            std::vector<uint8_t> dst((size_t)dw * dh * C), valid((size_t)dw * dh);
            rect::rectify_image(src.data(), sw, sh, C, sw * C, rect::camera_of(cam), plan, which, dst.data(), dw, dh, dw * C, valid.data());
            for (uint8_t v : dst) sum = sum * 31 + v;
            std::vector<int16_t> disp((size_t)dw * dh);
            for (size_t i = 0; i < disp.size(); ++i) disp[i] = (int16_t)((int)(i % 97) - 20);
            std::vector<float> xyz(3 * 50);
            std::vector<int32_t> pixel(50);
            const double S = 1.5;
            gms_sfm_view G = {{c, -sn, 0, sn, c, 0, 0, 0, 1}, {0.1, 0.2, 0.3}, 1, 0};
            sum = sum * 31 + (unsigned)rectify_host_cloud(disp.data(), valid.data(), dw, dh, &plan, -16, 16, &S, which == 2 ? &G : nullptr, 50,
                                                          xyz.data(), pixel.data());
        }
    }
    // wild plans by hand: a huge focal length, a camera far outside, not-a-number entries
    gms_rectify_plan wild;
    rect::identity_plan(rect::camera_of(cam), sw, sh, wild);
    const double bad[] = {1e-300, -1e300, 1e12, 0.0, NAN, INFINITY};
    for (double b : bad) {
        wild.fx = b;
        wild.cx = -b;
        wild.R1[2] = b;
        std::vector<uint8_t> dst((size_t)11 * 9 * C), valid((size_t)11 * 9);
        rect::rectify_image(src.data(), sw, sh, C, sw * C, rect::camera_of(cam), wild, 1, dst.data(), 11, 9, 11 * C, valid.data());
        for (uint8_t v : dst) sum = sum * 31 + v;
    }
    std::printf("rectify_host: checksum %llu\n", sum);
    return 0;
}
#endif
