// rectify_kernels.hip -- a dense cloud from a posed pair: the rectifying plans of a batch of pairs, the rectified
// images of n 8-bit images of 1 or 3 interleaved channels, and the points of n disparity maps. The arithmetic is rectify_core.h's;
// tests/rectify_ref.py states it in numpy, and every output byte equals it.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback (graph-capturable):
//   rectify_plan_kernel  one lane per pair: R, t and the status come from the two-view records in device memory.
//   rectify_kernel       warp_affine_kernel's shape: a 256-byte x 16-row tile of the destination per workgroup, a lane owns 4 adjacent
//                        bytes of a row. Every lane reads its image's plan from device memory (a captured graph follows new poses).
//                        The column part of the ray is kept per lane, the row part per tile row in LDS; what is left per pixel is the
//                        division by z, the distortion polynomial and the rounding, in fp64, done once per pixel (a lane's 4 bytes are
//                        4 pixels of one channel or 2 of three). Each of the four taps is bounds-checked before its address is formed.
//   cloud_count_kernel, cloud_scan_kernel, cloud_write_kernel
//                        the ordered compaction: points per block of 1024 pixels, their exclusive prefix per pair (one workgroup per
//                        pair), then every block ranks its own points and writes those below `cap`. No atomic decides a position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "rectify_core.h"
#include "ws_layout.h"

namespace gms {
namespace {

constexpr int kBlock = 256, kLaneBytes = 4, kTileBytes = 64 * kLaneBytes, kTY = 16;

__global__ void __launch_bounds__(kBlock)
rectify_plan_kernel(const gms_two_view* __restrict__ tv, int n, rect::Camera cam, int W, int H, int ow, int oh,
                    gms_rectify_plan* __restrict__ out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    gms_rectify_plan P;
    if (tv[i].status == GMS_OK) {
        double R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = tv[i].R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = tv[i].t[k];
        rect::make_plan(cam, R, t, W, H, ow, oh, P);
    } else {
        rect::zero_plan(P, GMS_ERR_NO_MODEL);
    }
    out[i] = P;
}

struct RectifyArgs {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* valid;  // optional: dense [n][dh][dw]
    const gms_rectify_plan* plans;
    rect::Camera cam;
    int64_t src_stride, dst_stride;
    int sw, sh, dw, dh, C, sp, dp, plan_stride, which;
};

__global__ void __launch_bounds__(kBlock)
rectify_kernel(RectifyArgs a)
{
    __shared__ double s_row[kTY][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row_bytes = a.dw * a.C;
    const int y0 = blockIdx.y * kTY, b0 = blockIdx.x * kTileBytes + lane * kLaneBytes;
    const gms_rectify_plan* __restrict__ P = a.plans + (int64_t)blockIdx.z * a.plan_stride;
    const double* __restrict__ Rp = a.which == 2 ? P->R2 : P->R1;
    double Rk[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rk[i] = Rp[i];
    const double pfx = P->fx, pfy = P->fy, pcx = P->cx, pcy = P->cy;
    const bool plan_ok = P->status == GMS_OK;
    if (tid < kTY) {
        double r[3];
        rect::row_terms(Rk, rect::norm_coord(y0 + tid, pcy, pfy), r);
        s_row[tid][0] = r[0];
        s_row[tid][1] = r[1];
        s_row[tid][2] = r[2];
    }
    __syncthreads();
    if (b0 >= row_bytes) return;
    int px[kLaneBytes], ch[kLaneBytes];
    double col[kLaneBytes][3];
#pragma unroll
    for (int j = 0; j < kLaneBytes; j++) {
        const int b = min(b0 + j, row_bytes - 1);  // (bytes past the row are computed from its last byte and not stored)
        px[j] = b / a.C;
        ch[j] = b - px[j] * a.C;
        rect::col_terms(Rk, rect::norm_coord(px[j], pcx, pfx), col[j]);
    }
    const uint8_t* __restrict__ src = a.src + (int64_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ dst = a.dst + (int64_t)blockIdx.z * a.dst_stride;
    uint8_t* __restrict__ valid = a.valid ? a.valid + (int64_t)blockIdx.z * a.dw * a.dh : nullptr;
    for (int ty = wave; ty < kTY && y0 + ty < a.dh; ty += kBlock / 64) {
        const double row[3] = {s_row[ty][0], s_row[ty][1], s_row[ty][2]};
        int v[kLaneBytes];
        rect::Src s = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kLaneBytes; j++) {
            if (plan_ok && (j == 0 || px[j] != px[j - 1])) s = rect::source_pos(a.cam, col[j], row);
            v[j] = rect::sample(src, a.sw, a.sh, a.C, a.sp, s, ch[j]);
            if (valid && ch[j] == 0 && b0 + j < row_bytes) valid[(int64_t)(y0 + ty) * a.dw + px[j]] = (uint8_t)rect::all_taps_inside(s, a.sw, a.sh);
        }
        uint8_t* p = dst + (int64_t)(y0 + ty) * a.dp + b0;
        if (b0 + kLaneBytes <= row_bytes && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < kLaneBytes; j++)
                if (b0 + j < row_bytes) p[j] = (uint8_t)v[j];
        }
    }
}

// ---- the cloud --------------------------------------------------------------------------------------------------------------------------
struct CloudArgs {
    const int16_t* disp;   // [n][H][W]
    const uint8_t* valid;  // [n][H][W]
    const uint8_t* image;  // optional: rows image_pitch apart
    const gms_rectify_plan* plans;
    const gms_pair* pairs;  // the three of a registration: all or none
    const gms_sfm_pair_reg* reg;
    const gms_sfm_view* views;
    int32_t* blocks;  // workspace: [n][n_blocks] counts, then their exclusive prefix in place
    float* xyz;
    uint8_t* color;
    int32_t* pixel;
    int32_t* count;
    int W, H, C, image_pitch, n_blocks, filtered16, min_disp16, cap, n_frames;
};

constexpr int kPerLane = rect::kScanBlock / kBlock;

__device__ __forceinline__ bool pair_has_points(const CloudArgs& a, int pair)
{
    return a.plans[pair].status == GMS_OK &&
           (!a.reg || (a.reg[pair].status == GMS_OK && (uint32_t)a.pairs[pair].frame_a < (uint32_t)a.n_frames));
}

// the flags of this lane's kPerLane adjacent pixels (bit j: pixel first + j is a point) -> their number
__device__ __forceinline__ int lane_flags(const CloudArgs& a, int pair, int64_t first, bool live, int& bits)
{
    const int64_t px = (int64_t)a.W * a.H;
    bits = 0;
    int n = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int64_t i = first + j;
        if (live && i < px && rect::is_point(a.disp[pair * px + i], a.filtered16, a.min_disp16, a.valid[pair * px + i])) {
            bits |= 1 << j;
            n++;
        }
    }
    return n;
}

__global__ void __launch_bounds__(kBlock)
cloud_count_kernel(CloudArgs a)
{
    __shared__ int s_n[kBlock / 64];
    const int pair = blockIdx.y, tid = threadIdx.x;
    int bits;
    int n = lane_flags(a, pair, (int64_t)blockIdx.x * rect::kScanBlock + tid * kPerLane, pair_has_points(a, pair), bits);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((tid & 63) == 0) s_n[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) a.blocks[(int64_t)pair * a.n_blocks + blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// exclusive prefix sum of kBlock values, one per lane, through LDS; returns the lane's prefix, total: the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* s, int& total)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const int incl = s[tid];
    total = s[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kBlock)
cloud_scan_kernel(CloudArgs a)
{
    __shared__ int s[kBlock];
    const int pair = blockIdx.x, tid = threadIdx.x;
    int32_t* __restrict__ b = a.blocks + (int64_t)pair * a.n_blocks;
    int carry = 0;
    for (int base = 0; base < a.n_blocks; base += kBlock) {
        const int i = base + tid;
        const int v = i < a.n_blocks ? b[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, s, total);
        if (i < a.n_blocks) b[i] = carry + ex;
        carry += total;
    }
    if (tid == 0) a.count[pair] = carry;
}

__global__ void __launch_bounds__(kBlock)
cloud_write_kernel(CloudArgs a)
{
    __shared__ int s[kBlock];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * rect::kScanBlock + tid * kPerLane;
    int bits, total;
    const int n = lane_flags(a, pair, first, pair_has_points(a, pair), bits);
    int rank = a.blocks[(int64_t)pair * a.n_blocks + blockIdx.x] + block_exclusive_scan(n, s, total);
    if (!bits) return;
    const gms_rectify_plan P = a.plans[pair];
    const int64_t px = (int64_t)a.W * a.H;
    const gms_sfm_view* G = a.reg ? a.views + a.pairs[pair].frame_a : nullptr;
    const double S = a.reg ? a.reg[pair].S : 0.0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        if (!(bits & (1 << j))) continue;
        if (rank < a.cap) {
            const int64_t i = first + j, slot = (int64_t)pair * a.cap + rank;
            const int v = (int)(i / a.W), u = (int)(i - (int64_t)v * a.W);
            float xyz[3];
            rect::cloud_point(P, u, v, a.disp[pair * px + i], &S, G, xyz);
            a.xyz[3 * slot] = xyz[0];
            a.xyz[3 * slot + 1] = xyz[1];
            a.xyz[3 * slot + 2] = xyz[2];
            a.pixel[slot] = (int32_t)i;
            if (a.color) {
                const uint8_t* c = a.image + ((int64_t)pair * a.H + v) * a.image_pitch + (int64_t)u * a.C;
                for (int k = 0; k < a.C; k++) a.color[slot * a.C + k] = c[k];
            }
        }
        rank++;
    }
}

static_assert(rect::kScanBlock == kDenseScanBlock && kPerLane * kBlock == rect::kScanBlock, "the layout and the kernels cut the same blocks");

}  // namespace

hipError_t launch_rectify_plan(const gms_camera& camera, const gms_two_view* d_tv, int n_pairs, int W, int H, int out_w, int out_h,
                               gms_rectify_plan* d_plans, hipStream_t stream)
{
    hipLaunchKernelGGL(rectify_plan_kernel, dim3((uint32_t)((n_pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, d_tv, n_pairs,
                       rect::camera_of(camera), W, H, out_w, out_h, d_plans);
    return hipGetLastError();
}

hipError_t launch_rectify(const gms_camera& camera, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch,
                          const gms_rectify_plan* d_plans, int n_plans, int which, uint8_t* d_dst, int dw, int dh, int dst_pitch,
                          uint8_t* d_valid, hipStream_t stream)
{
    const RectifyArgs a{d_src, d_dst, d_valid, d_plans, rect::camera_of(camera), (int64_t)src_pitch * sh, (int64_t)dst_pitch * dh,
                        sw, sh, dw, dh, channels, src_pitch, dst_pitch, n_plans == 1 ? 0 : 1, which};
    const dim3 grid((uint32_t)((dw * channels + kTileBytes - 1) / kTileBytes), (uint32_t)((dh + kTY - 1) / kTY), (uint32_t)n);
    hipLaunchKernelGGL(rectify_kernel, grid, dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

size_t dense_cloud_ws_bytes(int n_pairs, int W, int H) { return dense_cloud_layout(n_pairs, W, H).total; }

hipError_t launch_dense_cloud(const int16_t* d_disp16, const uint8_t* d_valid, const uint8_t* d_image, int channels, int image_pitch,
                              int n_pairs, int W, int H, const gms_rectify_plan* d_plans, int filtered16, int min_disp16,
                              const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws, int cap,
                              float* d_xyz, uint8_t* d_color, int32_t* d_pixel, int32_t* d_count, hipStream_t stream)
{
    const DenseCloudLayout L = dense_cloud_layout(n_pairs, W, H);
    const int nb = dense_cloud_blocks(W, H);
    const CloudArgs a{d_disp16, d_valid, d_image, d_plans, d_pairs, d_reg, d_views, ws_ptr<int32_t>(d_ws, L.blocks), d_xyz,
                      d_image ? d_color : nullptr, d_pixel, d_count, W, H, channels, image_pitch, nb, filtered16, min_disp16, cap, n_frames};
    hipLaunchKernelGGL(cloud_count_kernel, dim3((uint32_t)nb, (uint32_t)n_pairs), dim3(kBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3((uint32_t)n_pairs), dim3(kBlock), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cloud_write_kernel, dim3((uint32_t)nb, (uint32_t)n_pairs), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gms
