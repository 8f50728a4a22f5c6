// grad_desc_kernels.hip -- the gradient descriptor (arithmetic in grad_desc_core.h, numpy statement
// tests/grad_desc_ref.py) for gfx950: 128-float rows of SIFT's structure and format at the detector's keypoints, which the L2 matcher
// takes on its int8 matrix-core path. The detector itself (detect_kernels.hip) is unchanged and has run before this kernel: the box sums
// of the keypoint's level are in its workspace, and so is its list of level positions.
//
//   grad_describe_kernel   one wave per keypoint, four keypoints per workgroup. The 529 samples go over the 64 lanes (nine rounds); a
//                          sample adds to at most eight of the wave's 128 int32 accumulators in LDS with integer atomics -- integer adds
//                          commute, so the sums do not depend on timing. Both normalisation sums are 64-bit wave reductions; a lane
//                          stores two floats of the row as one 8-byte store. LDS: 2 KiB per workgroup.
//     kFromLevel   the keypoints of one pyramid level: position from det_emit_kernel's list, the direction bin from the record that
//                  det_describe_kernel wrote (angle = 11.25 * bin is exact in fp32, so bin = 4 * angle / 45 is; the fp32 pt is not read).
//     kAtRecords   the caller's keypoints (compute()): the detector's status rule, the direction recomputed from the moments and
//                  written to the record's angle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "grad_desc_core.h"

namespace gms {
namespace {

enum { kAtRecords = 0, kFromLevel = 1 };
struct GradLevel {
    const int32_t* level_counts;   // [level][image]: survivors of the levels
    int level, n_images, out_stride;
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((long long)v, d);
    return v;
}

template <int MODE>
__global__ void __launch_bounds__(256)
grad_describe_kernel(const uint8_t* __restrict__ images, const uint16_t* __restrict__ box, int w, int h, const uint32_t* __restrict__ list,
                     const int32_t* __restrict__ counts, int max_keypoints, gms_keypoint* __restrict__ kp, float* __restrict__ rows,
                     int32_t* __restrict__ status, GradLevel lv)
{
    __shared__ int32_t hist[4][gd::kDim];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, img = (int)blockIdx.y;
    const int k = (int)blockIdx.x * 4 + wave;
    const int n = counts != nullptr ? min(counts[img], max_keypoints) : max_keypoints;
    bool active = k < n;   // wave-uniform, as everything that follows from it; no wave leaves before the two barriers
    const size_t plane = (size_t)w * h;
    size_t slot = 0;
    int x = 0, y = 0, bin = 0;
    if (active) {
        if constexpr (MODE == kFromLevel) {
            int before = 0;
            for (int j = 0; j < lv.level; ++j) before += lv.level_counts[(size_t)j * lv.n_images + img];
            slot = (size_t)img * lv.out_stride + before + k;
            const uint32_t xy = list[((size_t)img * max_keypoints + k) * 2];
            x = (int)(xy & 0xFFFFu); y = (int)(xy >> 16);
            bin = ((int)(kp[slot].angle * 4.0f) / 45) & 31;
        } else {
            slot = (size_t)k;
            const float fx = kp[slot].x, fy = kp[slot].y;
            x = (int)fx; y = (int)fy;
            active = (float)x == fx && (float)y == fy && x >= kBorder && y >= kBorder && x < w - kBorder && y < h - kBorder;
            if (!active) {   // the caller sees the flag, the row stays as it was
                if (lane == 0) atomicMax(status, 1);
            } else {
                const uint8_t* __restrict__ im = images + (size_t)img * plane;
                int m10 = 0, m01 = 0;
                for (int i = lane; i < 31 * 31; i += 64) {
                    const int dy = i / 31 - 15, dx = i % 31 - 15;
                    if (dx * dx + dy * dy <= 225) {
                        const int v = im[(size_t)(y + dy) * w + (x + dx)];
                        m10 += dx * v;
                        m01 += dy * v;
                    }
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    m10 += __shfl_xor(m10, d);
                    m01 += __shfl_xor(m01, d);
                }
                bin = gd::direction_bin(m10, m01);
                if (lane == 0) kp[slot].angle = 11.25f * (float)bin;
            }
        }
    }
    hist[wave][lane] = 0;
    hist[wave][lane + 64] = 0;
    __syncthreads();
    if (active) {
        const uint16_t* __restrict__ bx = box + (size_t)img * plane;
        const int c = gd::dir_c(bin), s = gd::dir_s(bin);
        int32_t* acc = hist[wave];
        for (int i = lane; i < gd::kSamples; i += 64)
            gd::accumulate_sample(bx, w, x, y, c, s, i, [acc](int idx, int v) { atomicAdd(&acc[idx], v); });
    }
    __syncthreads();
    if (!active) return;
    int32_t v0 = hist[wave][2 * lane], v1 = hist[wave][2 * lane + 1];
    const uint64_t n1 = gd::isqrt64(wave_sum((uint64_t)((int64_t)v0 * v0) + (uint64_t)((int64_t)v1 * v1)));
    v0 = gd::clip_value(v0, n1);
    v1 = gd::clip_value(v1, n1);
    const uint64_t n2 = gd::isqrt64(wave_sum((uint64_t)((int64_t)v0 * v0) + (uint64_t)((int64_t)v1 * v1)));
    *reinterpret_cast<float2*>(rows + slot * gd::kDim + 2 * lane) = make_float2(gd::quantise(v0, n2), gd::quantise(v1, n2));
}

}  // namespace

// The pyramid call that also writes these rows needs no workspace region of its own: this kernel runs behind each level's describe kernel
// and reads what that level left -- the box sums and the list in the level's detect_layout, the direction in the keypoint record.
// the rows of one pyramid level's keypoints, after detect_level has run on that level in `d_det_ws` (detect_layout of the level)
hipError_t launch_grad_level(int n_images, int w, int h, int quota, void* d_det_ws, const int32_t* d_level_counts, int level, int out_stride,
                             gms_keypoint* d_kp, float* d_rows128, hipStream_t stream)
{
    if (n_images <= 0 || quota <= 0) return hipSuccess;
    const DetectLayout L = detect_layout(w, h, n_images, quota);
    const GradLevel lv = {d_level_counts, level, n_images, out_stride};
    hipLaunchKernelGGL(grad_describe_kernel<kFromLevel>, dim3((quota + 3) / 4, n_images), dim3(256), 0, stream, (const uint8_t*)nullptr,
                       ws_ptr<uint16_t>(d_det_ws, L.box), w, h, ws_ptr<uint32_t>(d_det_ws, L.list), d_level_counts + (size_t)level * n_images, quota,
                       d_kp, d_rows128, (int32_t*)nullptr, lv);
    return hipGetLastError();
}

// compute(): directions and 128-float rows at the caller's keypoints of ONE image; the status rule of launch_describe
hipError_t launch_describe_grad(const uint8_t* d_image, int w, int h, gms_keypoint* d_kp, int n, void* d_ws, float* d_rows128, int32_t* d_status,
                                hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(d_status, 0, 4, stream);
    if (e != hipSuccess) return e;
    e = launch_detect_maps(d_image, 1, w, h, d_ws, stream);
    if (e != hipSuccess) return e;
    if (n > 0)
        hipLaunchKernelGGL(grad_describe_kernel<kAtRecords>, dim3((n + 3) / 4, 1), dim3(256), 0, stream, d_image,
                           ws_ptr<uint16_t>(d_ws, detect_layout(w, h, 1, 0).box), w, h, (const uint32_t*)nullptr, (const int32_t*)nullptr, n, d_kp,
                           d_rows128, d_status, GradLevel{});
    return hipGetLastError();
}

}  // namespace gms
