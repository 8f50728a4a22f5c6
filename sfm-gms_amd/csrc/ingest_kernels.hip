// ingest_kernels.hip -- the two steps between a caller's photographs and the resident tables, for gfx950.
//
// The reference hands BGR Mats to every entry point and gets per-image keypoint vectors back from detectAndCompute
// (FeatureMatchUtil.cpp:9-12; SfMUtil.cpp:4-23). Here the detector takes grey planes and leaves [n, max_keypoints] blocks; the tables
// (gms_normalize_device, gms_bf_prepare_device, gms_logos_prepare_device) take all frames back to back with an offset per frame.
//
//   bgr_to_gray_kernel   n images of h x w x 3 bytes (B, G, R interleaved, pitch = 3 * width) -> n grey planes (pitch = width):
//                        grey = (299 R + 587 G + 114 B + 500) / 1000 in integers. With pitch = width the planes of a batch are one run of
//                        n * w * h bytes and the input one run of three times as many, so the kernel works on the run: a thread makes
//                        four pixels as one aligned 4-byte store, the run starts (address of its first pixel) & 3 pixels into the first
//                        group, and the pixels of the first and last group that fall inside the run are stored one by one. The twelve
//                        source bytes of a group come as four aligned 4-byte loads joined by the byte shift of their address.
//   pack_scan_kernel     frame_off[0] = 0, frame_off[i + 1] = frame_off[i] + min(max(counts[i], 0), max_keypoints): one workgroup,
//                        every thread a run of the counts, the runs' sums scanned through LDS.
//   pack_move_kernel     image i's records (28 B), 32-byte rows and 128-float rows from slot i * max_keypoints of the blocks to slot
//                        frame_off[i] of the packed arrays. Per image and array one run of bytes (a multiple of 4): 16-byte stores on
//                        the destination's 16-byte grid -- with one 16-byte load where the source is on it too (always for the rows of
//                        16-byte aligned buffers), four 4-byte loads where not (records: 28 B) -- and single 4-byte words at the ends.
//                        Nothing behind frame_off[n] is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"

namespace gms {
namespace {

constexpr int kGreyThreads = 256, kMoveThreads = 256, kScanThreads = 1024;
constexpr size_t kGreyBlocks = 4096;   // 4 Mi pixels a sweep: two waves of workgroups on 256 CUs at full occupancy
constexpr size_t kKpBytes = sizeof(gms_keypoint), kRow32Bytes = 32, kRow128Bytes = 512;

// the aligned 4 bytes at `a`, of which only those inside [lo, hi) are read (the others come back as 0)
__device__ __forceinline__ uint32_t load_word_inside(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a >= lo && a + 4 <= hi) return *reinterpret_cast<const uint32_t*>(a);
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b)
        if (a + b >= lo && a + b < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + b) << (8 * b);
    return v;
}

__device__ __forceinline__ uint32_t grey_of(uint32_t b, uint32_t g, uint32_t r) { return (299u * r + 587u * g + 114u * b + 500u) / 1000u; }

__global__ void __launch_bounds__(kGreyThreads)
bgr_to_gray_kernel(const uint8_t* __restrict__ bgr, size_t n_pixels, uint8_t* __restrict__ gray)
{
    const uintptr_t lo = reinterpret_cast<uintptr_t>(bgr), hi = lo + 3 * n_pixels;
    const int64_t shift = (int64_t)(reinterpret_cast<uintptr_t>(gray) & 3);
    const int64_t n = (int64_t)n_pixels, n_groups = (n + shift + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kGreyThreads + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * kGreyThreads) {
        const int64_t p0 = 4 * g - shift;   // first pixel of the group; gray + p0 is 4-byte aligned
        if (p0 >= 0 && p0 + 3 < n) {
            const uintptr_t src = lo + 3 * (uintptr_t)p0, a = src & ~(uintptr_t)3;
            const unsigned s = 8u * (unsigned)(src & 3);
            const uint32_t d0 = load_word_inside(a, lo, hi), d1 = load_word_inside(a + 4, lo, hi), d2 = load_word_inside(a + 8, lo, hi);
            const uint32_t d3 = s != 0 ? load_word_inside(a + 12, lo, hi) : 0u;
            // the twelve bytes from src on: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
            const uint32_t w0 = (uint32_t)((((uint64_t)d1 << 32) | d0) >> s), w1 = (uint32_t)((((uint64_t)d2 << 32) | d1) >> s);
            const uint32_t w2 = (uint32_t)((((uint64_t)d3 << 32) | d2) >> s);
            const uint32_t g0 = grey_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
            const uint32_t g1 = grey_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
            const uint32_t g2 = grey_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
            const uint32_t g3 = grey_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
            *reinterpret_cast<uint32_t*>(gray + p0) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        } else {
            for (int q = 0; q < 4; ++q) {
                const int64_t p = p0 + q;
                if (p >= 0 && p < n) gray[p] = (uint8_t)grey_of(bgr[3 * p], bgr[3 * p + 1], bgr[3 * p + 2]);
            }
        }
    }
}

__global__ void __launch_bounds__(kScanThreads)
pack_scan_kernel(const int32_t* __restrict__ counts, int n, int max_keypoints, int64_t* __restrict__ frame_off)
{
    __shared__ int64_t base[kScanThreads];   // (65535 images of up to 2^31 - 1 keypoints: 64-bit sums)
    const int tid = (int)threadIdx.x, per = (n + kScanThreads - 1) / kScanThreads;   // per <= 64
    int64_t sum = 0;
    for (int i = 0; i < per; ++i) {
        const int k = tid * per + i;
        if (k < n) sum += min(max(counts[k], 0), max_keypoints);
    }
    base[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {   // Hillis-Steele inclusive scan
        const int64_t before = tid >= d ? base[tid - d] : 0;
        __syncthreads();
        base[tid] += before;
        __syncthreads();
    }
    int64_t run = base[tid] - sum;   // exclusive prefix of this thread's images
    for (int i = 0; i < per; ++i) {
        const int k = tid * per + i;
        if (k < n) {
            if (k == 0) frame_off[0] = 0;
            run += min(max(counts[k], 0), max_keypoints);
            frame_off[k + 1] = run;
        }
    }
}

// `bytes` (a multiple of 4) from src to dst, both 4-byte aligned, by the threads `t` of `nt`
__device__ __forceinline__ void move_run(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t bytes, size_t t, size_t nt)
{
    const size_t head = min(bytes, (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));   // up to dst's 16-byte grid
    const size_t n16 = (bytes - head) / 16, tail = head + 16 * n16;
    const uint32_t* __restrict__ s4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* __restrict__ d4 = reinterpret_cast<uint32_t*>(dst);
    for (size_t i = t; i < head / 4; i += nt) d4[i] = s4[i];
    if (((reinterpret_cast<uintptr_t>(src) + head) & 15u) == 0) {
        const uint4* __restrict__ s16 = reinterpret_cast<const uint4*>(src + head);
        uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
        for (size_t i = t; i < n16; i += nt) d16[i] = s16[i];
    } else {
        const uint32_t* __restrict__ sw = s4 + head / 4;
        uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
        for (size_t i = t; i < n16; i += nt) d16[i] = make_uint4(sw[4 * i], sw[4 * i + 1], sw[4 * i + 2], sw[4 * i + 3]);
    }
    for (size_t i = tail / 4 + t; i < bytes / 4; i += nt) d4[i] = s4[i];
}

__global__ void __launch_bounds__(kMoveThreads)
pack_move_kernel(const uint8_t* __restrict__ kp_blocks, const uint8_t* __restrict__ rows32_blocks, const uint8_t* __restrict__ rows128_blocks,
                 int max_keypoints, const int64_t* __restrict__ frame_off, uint8_t* __restrict__ kp, uint8_t* __restrict__ rows32,
                 uint8_t* __restrict__ rows128)
{
    const size_t img = blockIdx.y;
    const size_t off = (size_t)frame_off[img], count = (size_t)frame_off[img + 1] - off, slot = img * (size_t)max_keypoints;
    if (count == 0) return;
    const size_t t = (size_t)blockIdx.x * kMoveThreads + threadIdx.x, nt = (size_t)gridDim.x * kMoveThreads;
    move_run(kp_blocks + slot * kKpBytes, kp + off * kKpBytes, count * kKpBytes, t, nt);
    if (rows32 != nullptr) move_run(rows32_blocks + slot * kRow32Bytes, rows32 + off * kRow32Bytes, count * kRow32Bytes, t, nt);
    if (rows128 != nullptr) move_run(rows128_blocks + slot * kRow128Bytes, rows128 + off * kRow128Bytes, count * kRow128Bytes, t, nt);
}

}  // namespace

hipError_t launch_bgr_to_gray(const uint8_t* d_bgr, int n, int w, int h, uint8_t* d_gray, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const size_t n_pixels = (size_t)n * w * h, groups = (n_pixels + 3 + 3) / 4;
    const size_t blocks = (groups + kGreyThreads - 1) / kGreyThreads;   // at most kGreyBlocks: a thread then takes several groups
    hipLaunchKernelGGL(bgr_to_gray_kernel, dim3((unsigned)(blocks < kGreyBlocks ? blocks : kGreyBlocks)), dim3(kGreyThreads), 0, stream, d_bgr, n_pixels, d_gray);
    return hipGetLastError();
}

hipError_t launch_detect_pack(const gms_keypoint* d_kp_blocks, const uint8_t* d_rows32_blocks, const float* d_rows128_blocks, const int32_t* d_counts,
                              int n, int max_keypoints, gms_keypoint* d_kp, uint8_t* d_rows32, float* d_rows128, int64_t* d_frame_off,
                              hipStream_t stream)
{
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_counts, n, max_keypoints, d_frame_off);
    if (max_keypoints > 0) {
        // an image's longest run, in 16-byte units, over workgroups of 256 threads with four units a thread; at most 256 of them an image
        const size_t units = (size_t)max_keypoints * (d_rows128 != nullptr ? kRow128Bytes : kRow32Bytes) / 16;
        const size_t bx = (units + 4 * kMoveThreads - 1) / (4 * kMoveThreads);
        hipLaunchKernelGGL(pack_move_kernel, dim3((unsigned)(bx < 256 ? bx : 256), (unsigned)n), dim3(kMoveThreads), 0, stream,
                           reinterpret_cast<const uint8_t*>(d_kp_blocks), d_rows32_blocks, reinterpret_cast<const uint8_t*>(d_rows128_blocks),
                           max_keypoints, d_frame_off, reinterpret_cast<uint8_t*>(d_kp), d_rows32, reinterpret_cast<uint8_t*>(d_rows128));
    }
    return hipGetLastError();
}

}  // namespace gms
