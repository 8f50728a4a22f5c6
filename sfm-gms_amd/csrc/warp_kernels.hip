// warp_kernels.hip -- cv::resize (INTER_LINEAR, and the exact 2 x 2 mean when both axes halve) and cv::warpAffine (INTER_LINEAR,
// BORDER_CONSTANT 0) for a batch of n equally sized 8-bit images of 1 or 3 interleaved channels. The arithmetic is
// warp_core.h's; tests/warp_ref.py states it in numpy, and every output byte equals it.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback, no workspace (graph-capturable):
//   resize_linear_kernel  a 256-byte x 16-row tile of the destination per workgroup. A lane owns 4 adjacent bytes of the row: it works
//                         out their column taps once and keeps them for the tile's rows; the tile's 16 row taps are worked out once, in
//                         LDS.
//   resize_area2_kernel   the same tile; one-channel rows that are 8-byte aligned are read as two dwords per source row.
//   warp_affine_kernel    the same tile. Every lane inverts the image's forward matrix itself (read from device memory, so that a
//                         captured graph follows new matrices); the column parts of the source position are kept per lane, the row
//                         parts per tile row in LDS. Each of the four taps is bounds-checked, so nothing outside the source is read.
// The 4 bytes go out as one dword where the address is 4-byte aligned and the row has them, else byte by byte (the row's tail, and
// rows whose pitch leaves them unaligned). These are gather kernels: the reads are byte loads that the caches coalesce.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "warp_core.h"

namespace gms {
namespace {

constexpr int kBlock = 256, kLaneBytes = 4, kTileBytes = 64 * kLaneBytes, kTY = 16;

struct WarpArgs {
    const uint8_t* src;
    uint8_t* dst;
    const double* M;  // warpAffine: forward matrices, m_stride doubles apart (0: one for all images)
    int64_t src_stride, dst_stride;
    int sw, sh, dw, dh, C, sp, dp, m_stride;
};

// 4 bytes of a destination row at byte b0 of `row_bytes`: one dword where aligned and whole, else the bytes that exist
__device__ __forceinline__ void store4(uint8_t* __restrict__ row, int b0, int row_bytes, const int v[kLaneBytes])
{
    uint8_t* p = row + b0;
    if (b0 + kLaneBytes <= row_bytes && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kLaneBytes; j++)
            if (b0 + j < row_bytes) p[j] = (uint8_t)v[j];
    }
}

__global__ void __launch_bounds__(kBlock)
resize_linear_kernel(WarpArgs a)
{
    __shared__ int s_r0[kTY], s_r1[kTY], s_b0[kTY], s_b1[kTY];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row_bytes = a.dw * a.C;
    const int y0 = blockIdx.y * kTY, b0 = blockIdx.x * kTileBytes + lane * kLaneBytes;
    if (tid < kTY && y0 + tid < a.dh) {
        const warp::Tap b = warp::axis_tap(y0 + tid, warp::axis_scale(a.dh, a.sh), a.sh, false);
        s_r0[tid] = warp::clampi(b.s, 0, a.sh - 1);
        s_r1[tid] = warp::clampi(b.s + 1, 0, a.sh - 1);
        s_b0[tid] = b.w0;
        s_b1[tid] = b.w1;
    }
    __syncthreads();
    if (b0 >= row_bytes) return;
    const double scx = warp::axis_scale(a.dw, a.sw);
    int o0[kLaneBytes], o1[kLaneBytes];
    warp::Tap t[kLaneBytes];
#pragma unroll
    for (int j = 0; j < kLaneBytes; j++) {
        const int b = min(b0 + j, row_bytes - 1);  // (bytes past the row are computed from its last byte and not stored)
        const int x = b / a.C, c = b - x * a.C;
        t[j] = warp::axis_tap(x, scx, a.sw, true);
        o0[j] = t[j].s * a.C + c;
        o1[j] = min(t[j].s + 1, a.sw - 1) * a.C + c;
    }
    const uint8_t* __restrict__ src = a.src + (int64_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ dst = a.dst + (int64_t)blockIdx.z * a.dst_stride;
    for (int ty = wave; ty < kTY && y0 + ty < a.dh; ty += kBlock / 64) {
        const uint8_t* __restrict__ r0 = src + (int64_t)s_r0[ty] * a.sp;
        const uint8_t* __restrict__ r1 = src + (int64_t)s_r1[ty] * a.sp;
        warp::Tap b;
        b.s = 0;
        b.w0 = s_b0[ty];
        b.w1 = s_b1[ty];
        int v[kLaneBytes];
#pragma unroll
        for (int j = 0; j < kLaneBytes; j++)
            v[j] = warp::resize_v(warp::resize_h(r0[o0[j]], r0[o1[j]], t[j]), warp::resize_h(r1[o0[j]], r1[o1[j]], t[j]), b);
        store4(dst + (int64_t)(y0 + ty) * a.dp, b0, row_bytes, v);
    }
}

__global__ void __launch_bounds__(kBlock)
resize_area2_kernel(WarpArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row_bytes = a.dw * a.C;
    const int y0 = blockIdx.y * kTY, b0 = blockIdx.x * kTileBytes + lane * kLaneBytes;
    if (b0 >= row_bytes) return;
    int o[kLaneBytes];  // the source byte of the 2 x 2 block's first pixel
#pragma unroll
    for (int j = 0; j < kLaneBytes; j++) {
        const int b = min(b0 + j, row_bytes - 1);
        const int x = b / a.C, c = b - x * a.C;
        o[j] = 2 * x * a.C + c;
    }
    const uint8_t* __restrict__ src = a.src + (int64_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ dst = a.dst + (int64_t)blockIdx.z * a.dst_stride;
    const bool whole = a.C == 1 && b0 + kLaneBytes <= row_bytes;
    for (int ty = wave; ty < kTY && y0 + ty < a.dh; ty += kBlock / 64) {
        const uint8_t* __restrict__ r0 = src + (int64_t)(2 * (y0 + ty)) * a.sp;
        const uint8_t* __restrict__ r1 = r0 + a.sp;
        int v[kLaneBytes];
        if (whole && ((reinterpret_cast<uintptr_t>(r0 + 2 * b0) | reinterpret_cast<uintptr_t>(r1 + 2 * b0)) & 7u) == 0) {
            const uint2 p = *reinterpret_cast<const uint2*>(r0 + 2 * b0), q = *reinterpret_cast<const uint2*>(r1 + 2 * b0);
            const uint32_t w[4] = {p.x & 0xffffu, p.x >> 16, p.y & 0xffffu, p.y >> 16};
            const uint32_t z[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
#pragma unroll
            for (int j = 0; j < kLaneBytes; j++) v[j] = warp::area2(w[j] & 0xff, w[j] >> 8, z[j] & 0xff, z[j] >> 8);
        } else {
#pragma unroll
            for (int j = 0; j < kLaneBytes; j++) v[j] = warp::area2(r0[o[j]], r0[o[j] + a.C], r1[o[j]], r1[o[j] + a.C]);
        }
        store4(dst + (int64_t)(y0 + ty) * a.dp, b0, row_bytes, v);
    }
}

__global__ void __launch_bounds__(kBlock)
warp_affine_kernel(WarpArgs a)
{
    __shared__ long long s_X0[kTY], s_Y0[kTY];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row_bytes = a.dw * a.C;
    const int y0 = blockIdx.y * kTY, b0 = blockIdx.x * kTileBytes + lane * kLaneBytes;
    const double* __restrict__ Fp = a.M + (int64_t)blockIdx.z * a.m_stride;
    double F[6], M[6];
#pragma unroll
    for (int i = 0; i < 6; i++) F[i] = Fp[i];
    warp::invert_affine(F, M);
    if (tid < kTY) {
        s_X0[tid] = warp::row_base(M[1], M[2], y0 + tid);
        s_Y0[tid] = warp::row_base(M[4], M[5], y0 + tid);
    }
    __syncthreads();
    if (b0 >= row_bytes) return;
    int ad[kLaneBytes], bd[kLaneBytes], ch[kLaneBytes];
#pragma unroll
    for (int j = 0; j < kLaneBytes; j++) {
        const int b = min(b0 + j, row_bytes - 1);
        const int x = b / a.C;
        ch[j] = b - x * a.C;
        ad[j] = warp::col_delta(M[0], x);
        bd[j] = warp::col_delta(M[3], x);
    }
    const uint8_t* __restrict__ src = a.src + (int64_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ dst = a.dst + (int64_t)blockIdx.z * a.dst_stride;
    for (int ty = wave; ty < kTY && y0 + ty < a.dh; ty += kBlock / 64) {
        const long long X0 = s_X0[ty], Y0 = s_Y0[ty];
        int v[kLaneBytes];
#pragma unroll
        for (int j = 0; j < kLaneBytes; j++) {
            const warp::Pos p = warp::position(X0, Y0, ad[j], bd[j]);
            v[j] = warp::blend(warp::tap_at(src, a.sw, a.sh, a.C, a.sp, p.ix, p.iy, ch[j]),
                               warp::tap_at(src, a.sw, a.sh, a.C, a.sp, p.ix + 1, p.iy, ch[j]),
                               warp::tap_at(src, a.sw, a.sh, a.C, a.sp, p.ix, p.iy + 1, ch[j]),
                               warp::tap_at(src, a.sw, a.sh, a.C, a.sp, p.ix + 1, p.iy + 1, ch[j]), p.fx, p.fy);
        }
        store4(dst + (int64_t)(y0 + ty) * a.dp, b0, row_bytes, v);
    }
}

dim3 tile_grid(int dw, int dh, int C, int n)
{
    return dim3((uint32_t)((dw * C + kTileBytes - 1) / kTileBytes), (uint32_t)((dh + kTY - 1) / kTY), (uint32_t)n);
}

}  // namespace

hipError_t launch_resize(const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, uint8_t* d_dst, int dw, int dh,
                         int dst_pitch, hipStream_t stream)
{
    const WarpArgs a{d_src, d_dst, nullptr, (int64_t)src_pitch * sh, (int64_t)dst_pitch * dh, sw, sh, dw, dh, channels, src_pitch, dst_pitch, 0};
    if (warp::is_area2(sw, sh, dw, dh))
        hipLaunchKernelGGL(resize_area2_kernel, tile_grid(dw, dh, channels, n), dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(resize_linear_kernel, tile_grid(dw, dh, channels, n), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_warp_affine(const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, const double* d_M, int n_matrices,
                              uint8_t* d_dst, int dw, int dh, int dst_pitch, hipStream_t stream)
{
    const WarpArgs a{d_src, d_dst, d_M, (int64_t)src_pitch * sh, (int64_t)dst_pitch * dh, sw, sh, dw, dh, channels, src_pitch, dst_pitch,
                     n_matrices == 1 ? 0 : 6};
    hipLaunchKernelGGL(warp_affine_kernel, tile_grid(dw, dh, channels, n), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gms
