// calib_kernels.hip -- chessboard corner candidates and cornerSubPix for a batch of n equally sized 8-bit grey images, pitch = width,
// back to back. The arithmetic is calib_core.h's; tests/calib_ref.py states it in numpy, and every candidate record
// equals it.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback (graph-capturable):
//   chess_response_kernel  a 64 x 16 tile of R per workgroup. The tile's pixels with a halo of 8 come in as aligned dwords, each row
//                          from the 4-byte boundary at or below its first pixel, the row's shift remembered (rows start at any byte
//                          address: pitch = width). S = box5(box5(image)) is separable: per axis the 9 taps 1 2 3 4 5 4 3 2 1. The
//                          row pass (uint16, <= 25 * 255) and the column pass (S, int32) both stay in LDS; R goes out once, 4 B / pixel.
//   chess_nms_kernel       a 64 x 16 tile of R with a halo of 8 in LDS; the 17-wide row maxima once, then per pixel the maxima of
//                          the rows above, the rows below, the row's left and the row's right. A peak's rank key (R, then raster
//                          order) is appended to the image's list: one atomic per workgroup reserves its slots. The list's order is
//                          not fixed, and need not be: the keys of an image are distinct and the next kernel ranks them.
//   chess_rank_kernel      a peak's rank = the number of larger keys; ranks below max_candidates are written as records. Exact for
//                          any ties, since the raster order is part of the key. The list is short (<= one peak per 9 x 9 pixels).
//   corner_subpix_kernel   one lane per corner, fp64, calib::subpix_refine. 540 corners: not a hot kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "calib_core.h"
#include "gms_kernels.h"
#include "ws_layout.h"

namespace gms {
namespace {

constexpr int kTW = 64, kTH = 16, kHalo = 8;          // image halo: 4 (arm) + 2 + 2 (the two box sums)
constexpr int kIW = kTW + 2 * kHalo, kIH = kTH + 2 * kHalo;   // 80 x 32 pixels
constexpr int kRowDwords = (kIW + 3 + 3) / 4;         // 80 pixels from a shift of up to 3: 21 dwords
constexpr int kSW = kTW + 2 * calib::kArm, kSH = kTH + 2 * calib::kArm;   // S: 72 x 24

__global__ void __launch_bounds__(256)
chess_response_kernel(const uint8_t* __restrict__ images, int w, int h, uint32_t* __restrict__ R)
{
    __shared__ uint32_t s_img[kIH][kRowDwords + 1];
    __shared__ int s_shift[kIH];
    __shared__ uint16_t s_row[kIH][kSW + 2];   // the 9 row taps, at S's columns, for every image row of the tile
    __shared__ int s_S[kSH][kSW + 1];
    const size_t plane = (size_t)w * h;
    const uint8_t* __restrict__ img = images + (size_t)blockIdx.z * plane;
    const int x0 = (int)blockIdx.x * kTW, y0 = (int)blockIdx.y * kTH, tid = (int)threadIdx.x;
    // pixels (x0 - 8 .., y0 - 8 ..): dword k of a row holds the bytes from `first + 4 k`, first = the row's address rounded down
    for (int i = tid; i < kIH * kRowDwords; i += 256) {
        const int ly = i / kRowDwords, k = i - ly * kRowDwords;
        const int y = min(max(y0 + ly - kHalo, 0), h - 1);   // (clamped reads: such values only reach pixels whose R is forced to 0)
        const uint8_t* row = img + (size_t)y * w;
        const uintptr_t start = reinterpret_cast<uintptr_t>(row) + (uintptr_t)(intptr_t)(x0 - kHalo);
        const int shift = (int)(start & 3u);
        const int xs = x0 - kHalo - shift + 4 * k;          // the pixel of the dword's first byte
        uint32_t v;
        if (xs >= 0 && xs + 3 < w) {
            v = *reinterpret_cast<const uint32_t*>(row + xs);   // aligned: (row + x0 - 8 - shift) is, and 4 k keeps it
        } else {
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)row[min(max(xs + j, 0), w - 1)] << (8 * j);
        }
        s_img[ly][k] = v;
        if (k == 0) s_shift[ly] = shift;
    }
    __syncthreads();
    // row pass: P[ly][c] = sum_t tap[t] * pixel(x0 - 4 + c - 4 + t): 72 columns x 32 rows
    for (int i = tid; i < kIH * kSW; i += 256) {
        const int ly = i / kSW, c = i - ly * kSW;
        const uint8_t* px = reinterpret_cast<const uint8_t*>(s_img[ly]) + s_shift[ly] + c;   // pixel x0 - 8 + c: the window's first
        int s = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) s += (t < 5 ? t + 1 : 9 - t) * (int)px[t];
        s_row[ly][c] = (uint16_t)s;
    }
    __syncthreads();
    // column pass: S[r][c] for rows y0 - 4 + r
    for (int i = tid; i < kSH * kSW; i += 256) {
        const int r = i / kSW, c = i - r * kSW;
        int s = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) s += (t < 5 ? t + 1 : 9 - t) * (int)s_row[r + t][c];
        s_S[r][c] = s;
    }
    __syncthreads();
    const int lx = tid & 63, ry = tid >> 6;
    constexpr int d = calib::kArm;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = ry + 4 * j, x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        uint32_t r = 0;
        if (calib::inner(x, y, w, h)) {
            const int cx = lx + d, cy = ly + d;
            r = calib::response_of(s_S[cy][cx], s_S[cy][cx + d], s_S[cy][cx - d], s_S[cy + d][cx], s_S[cy - d][cx], s_S[cy + d][cx + d],
                                   s_S[cy - d][cx - d], s_S[cy - d][cx + d], s_S[cy + d][cx - d]);
        }
        R[(size_t)blockIdx.z * plane + (size_t)y * w + x] = r;
    }
}

__global__ void __launch_bounds__(256)
chess_nms_kernel(const uint32_t* __restrict__ R, int w, int h, uint32_t cap, uint64_t* __restrict__ list, uint32_t* __restrict__ n_list)
{
    constexpr int r8 = calib::kNmsR;
    __shared__ uint32_t s_R[kIH][kIW + 1];
    __shared__ uint32_t s_max[kIH][kTW + 1];   // maxima of the 17 pixels around column lx, for every row of the halo
    __shared__ uint32_t s_count, s_base;
    const size_t plane = (size_t)w * h;
    const uint32_t* __restrict__ Ri = R + (size_t)blockIdx.z * plane;
    const int x0 = (int)blockIdx.x * kTW, y0 = (int)blockIdx.y * kTH, tid = (int)threadIdx.x;
    if (tid == 0) s_count = 0;
    for (int i = tid; i < kIH * kIW; i += 256) {
        const int ly = i / kIW, lx = i - ly * kIW;
        const int x = x0 + lx - r8, y = y0 + ly - r8;
        s_R[ly][lx] = (x >= 0 && y >= 0 && x < w && y < h) ? Ri[(size_t)y * w + x] : 0u;   // nothing outside the image competes
    }
    __syncthreads();
    for (int i = tid; i < kIH * kTW; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t <= 2 * r8; ++t) m = max(m, s_R[ly][lx + t]);
        s_max[ly][lx] = m;
    }
    __syncthreads();
    const int lx = tid & 63, ry = tid >> 6;
    uint32_t mine[4], slot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = ry + 4 * j, x = x0 + lx, y = y0 + ly;
        const uint32_t r = s_R[ly + r8][lx + r8];
        bool peak = r > 0 && x < w && y < h;
        if (peak) {   // greater than everything earlier in raster order, not smaller than anything later
            uint32_t above = 0, below = 0, left = 0, right = 0;
#pragma unroll
            for (int t = 0; t < r8; ++t) {
                above = max(above, s_max[ly + t][lx]);
                below = max(below, s_max[ly + r8 + 1 + t][lx]);
                left = max(left, s_R[ly + r8][lx + t]);
                right = max(right, s_R[ly + r8][lx + r8 + 1 + t]);
            }
            peak = r > above && r > left && r >= right && r >= below;
        }
        mine[j] = peak ? r : 0u;
        slot[j] = peak ? atomicAdd(&s_count, 1u) : 0u;
    }
    __syncthreads();
    if (tid == 0 && s_count != 0) s_base = atomicAdd(&n_list[blockIdx.z], s_count);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (mine[j] == 0) continue;
        const uint32_t at = s_base + slot[j];
        if (at < cap)   // (always: calib::peak_capacity bounds the peaks of an image)
            list[(size_t)blockIdx.z * cap + at] = calib::rank_key(mine[j], (uint32_t)((y0 + ry + 4 * j) * w + x0 + lx));
    }
}

__global__ void __launch_bounds__(256)
chess_rank_kernel(const uint64_t* __restrict__ list, const uint32_t* __restrict__ n_list, uint32_t cap, int w, int max_candidates,
                  gms_chess_candidate* __restrict__ out, int32_t* __restrict__ counts)
{
    __shared__ uint64_t s_keys[256];
    const int img = (int)blockIdx.y, tid = (int)threadIdx.x;
    const uint32_t n = min(n_list[img], cap);
    if (blockIdx.x == 0 && tid == 0) counts[img] = (int32_t)min(n, (uint32_t)max_candidates);
    if (blockIdx.x * 256u >= n) return;   // (the whole workgroup)
    const uint64_t* __restrict__ keys = list + (size_t)img * cap;
    const uint32_t i = blockIdx.x * 256u + (uint32_t)tid;
    const uint64_t mine = i < n ? keys[i] : 0ull;
    uint32_t rank = 0;
    for (uint32_t base = 0; base < n; base += 256u) {
        __syncthreads();
        s_keys[tid] = base + (uint32_t)tid < n ? keys[base + (uint32_t)tid] : 0ull;
        __syncthreads();
        const uint32_t m = min(256u, n - base);
        for (uint32_t k = 0; k < m; ++k) rank += s_keys[k] > mine ? 1u : 0u;
    }
    if (i < n && rank < (uint32_t)max_candidates) {
        const uint32_t raster = 0xffffffffu - (uint32_t)mine;
        gms_chess_candidate c;
        c.x = (int32_t)(raster % (uint32_t)w);
        c.y = (int32_t)(raster / (uint32_t)w);
        c.response = (uint32_t)(mine >> 32);
        out[(size_t)img * max_candidates + rank] = c;
    }
}

__global__ void __launch_bounds__(64)
corner_subpix_kernel(const uint8_t* __restrict__ images, int n_images, int w, int h, const int32_t* __restrict__ image_of,
                     double* __restrict__ corners, int n_corners, int max_iter, double eps, int32_t* __restrict__ status)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n_corners) return;
    const int im = image_of ? image_of[i] : 0;
    if (im < 0 || im >= n_images) {   // the corner stays; nothing is read
        if (status) status[i] = calib::kSubpixLeftImage;
        return;
    }
    double ox, oy, last;
    const int st = calib::subpix_refine(images + (size_t)im * w * h, w, h, w, corners[2 * i], corners[2 * i + 1], max_iter, eps, ox, oy, last);
    corners[2 * i] = ox;
    corners[2 * i + 1] = oy;
    if (status) status[i] = st;
}

}  // namespace

size_t chess_candidates_ws_bytes(int n, int w, int h) { return chess_layout(n, w, h).total; }

hipError_t launch_chess_candidates(const uint8_t* d_images, int n, int w, int h, int max_candidates, void* d_ws,
                                   gms_chess_candidate* d_out, int32_t* d_counts, hipStream_t stream)
{
    const ChessLayout lay = chess_layout(n, w, h);
    const uint32_t cap = (uint32_t)calib::peak_capacity(w, h);
    uint32_t* n_list = ws_ptr<uint32_t>(d_ws, lay.n_list);
    hipError_t e = hipMemsetAsync(n_list, 0, (size_t)n * 4, stream);
    if (e != hipSuccess) return e;
    if (cap == 0) return hipMemsetAsync(d_counts, 0, (size_t)n * 4, stream);   // no inner pixel: R = 0 everywhere
    const dim3 tiles((uint32_t)((w + kTW - 1) / kTW), (uint32_t)((h + kTH - 1) / kTH), (uint32_t)n);
    hipLaunchKernelGGL(chess_response_kernel, tiles, dim3(256), 0, stream, d_images, w, h, ws_ptr<uint32_t>(d_ws, lay.R));
    hipLaunchKernelGGL(chess_nms_kernel, tiles, dim3(256), 0, stream, ws_ptr<uint32_t>(d_ws, lay.R), w, h, cap, ws_ptr<uint64_t>(d_ws, lay.list),
                       n_list);
    hipLaunchKernelGGL(chess_rank_kernel, dim3((cap + 255u) / 256u, (uint32_t)n), dim3(256), 0, stream, ws_ptr<uint64_t>(d_ws, lay.list), n_list,
                       cap, w, max_candidates, d_out, d_counts);
    return hipGetLastError();
}

hipError_t launch_corner_subpix(const uint8_t* d_images, int n_images, int w, int h, const int32_t* d_image_of, double* d_corners,
                                int n_corners, int max_iter, double eps, int32_t* d_status, hipStream_t stream)
{
    hipLaunchKernelGGL(corner_subpix_kernel, dim3((uint32_t)((n_corners + 63) / 64)), dim3(64), 0, stream, d_images, n_images, w, h, d_image_of,
                       d_corners, n_corners, max_iter, eps, d_status);
    return hipGetLastError();
}

}  // namespace gms
