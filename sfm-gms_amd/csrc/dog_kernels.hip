// dog_kernels.hip -- the difference-of-Gaussians detector of the pyramid keypoint source (arithmetic in
// dog_core.h, numpy statement tests/dog_ref.py) for gfx950. One kernel takes the place of det_maps_kernel + det_nms_kernel in a level's
// chain (detect_kernels.hip): it writes the candidate plane, the 5 x 5 box sums and the level's score histogram, and everything behind
// it -- cut-off, row counts, scan, emit, describe, the gradient rows -- is the FAST source's, unchanged.
//
//   dog_maps_kernel   a 64 x 16 output tile per 256-thread workgroup, fused, nothing but LDS between the steps:
//     load   the 80 x 32 pixels around the tile (halo 1 + 7), coordinates clamped to the image (those values are never used), packed
//            four to a dword; four more columns so that the row pass can work on whole dwords.
//     rows   H_0..H_3 at 68 x 32 positions: a thread makes four neighbouring columns of one row from five dwords of pixels (18 bytes)
//            and stores each blur's four u16 as one 8-byte store.
//     cols   B_0..B_3 at 68 x 18 positions: a thread makes the same four columns of one row from 2 r + 1 8-byte loads per blur. Work
//            item i reads from byte 8 i of a plane (+ a row offset): consecutive lanes, consecutive banks.
//     test   a thread takes two neighbouring columns of two rows. The three layers on the 4 x 4 positions those four pixels see are
//            formed once in registers from 32 dword loads (two u16 each), then the candidate rule of dog_core.h; the 5 x 5 box sums
//            come from 12 dword loads of pixels (six row sums per column, shared by the two rows). Sub-dword LDS loads cost the
//            cycles of a dword load, and the kernel is bound by its LDS instructions, so everything is read as dwords.
//     hist   scores counted in LDS, one global atomic per bin that the tile touched.
//   dog_maps_kernel<true>   the same, and at every candidate the code of dog_core.h's refine (offsets in 1/16 pixel and 1/16 layer) as a
//            2-byte store into a plane of its own: the layers are in registers at that point.
//   LDS: 2 688 (pixels) + 17 408 (H) + 9 792 (B) + 1 024 (histogram) = 30 912 bytes: five workgroups per CU.
//   HBM: 1 byte in, 3 bytes out per pixel (+ the halo re-reads, which the L2 serves).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dog_core.h"
#include "gms_kernels.h"

namespace gms {
namespace {

constexpr int kTileW = 64, kTileH = 16;
constexpr int kPixW = 84, kPixH = kTileH + 2 * dog::kReach;    // 80 columns used by the tile + 4 for whole-dword work; 32 rows
constexpr int kQuads = 17, kPlaneW = 4 * kQuads;               // 66 columns are needed (tile + 1 each side); 68 are made
constexpr int kHRows = kPixH, kBRows = kTileH + 2;             // 32 and 18
static_assert(kTileW + 2 <= kPlaneW && kPlaneW + 2 * dog::kMaxRadius + 2 <= kPixW, "a quad of columns reads 18 pixel bytes");
static_assert(kBRows + 2 * dog::kMaxRadius == kHRows, "the column pass reads exactly the rows the row pass made");

template <int J>
__device__ __forceinline__ void row_pass(const int (&px)[20], uint16_t* __restrict__ dst)
{
    uint64_t packed = 0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int s = dog::weighted_sum<J>([&](int i) { return px[dog::kMaxRadius + o + i]; });
        packed |= (uint64_t)(uint32_t)dog::round_h(s) << (16 * o);
    }
    *reinterpret_cast<uint64_t*>(dst) = packed;
}

template <int J>
__device__ __forceinline__ void col_pass(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst)
{
    // src: this quad of the blur's H plane at the first row of the 15-row window; the blur's own rows are centred in it
    constexpr int r = dog::radius(J);
    uint64_t rows[2 * r + 1];
#pragma unroll
    for (int i = 0; i <= 2 * r; ++i) rows[i] = *reinterpret_cast<const uint64_t*>(src + (size_t)(dog::kMaxRadius - r + i) * kPlaneW);
    uint64_t packed = 0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int s = dog::weighted_sum<J>([&](int i) { return (int)((rows[r + i] >> (16 * o)) & 0xFFFFu); });
        packed |= (uint64_t)(uint32_t)dog::round_v(s) << (16 * o);
    }
    *reinterpret_cast<uint64_t*>(dst) = packed;
}

// kRefine: the code of dog::refine at every candidate goes to `codes` as well, from the layers the candidate rule has just read. A
// level's describe kernel reads a code only where the candidate plane is non-zero, so nothing else is stored; with cand == nullptr
// (the code planes alone) every pixel is stored, 0 where there is no candidate, and no candidate plane.
template <bool kRefine>
__global__ void __launch_bounds__(256)
dog_maps_kernel(const uint8_t* __restrict__ images, int w, int h, int contrast, uint8_t* __restrict__ cand, uint16_t* __restrict__ box,
                uint32_t* __restrict__ hist, uint16_t* __restrict__ codes)
{
    __shared__ __attribute__((aligned(16))) uint32_t pix[kPixH][kPixW / 4];
    __shared__ __attribute__((aligned(16))) uint16_t H[dog::kBlurs][kHRows][kPlaneW];
    __shared__ __attribute__((aligned(16))) uint16_t B[dog::kBlurs][kBRows][kPlaneW];
    __shared__ uint32_t lh[256];
    const int tid = (int)threadIdx.x;
    const size_t plane = (size_t)w * h;
    const uint8_t* __restrict__ img = images + (size_t)blockIdx.z * plane;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    lh[tid] = 0;
    // load: pixel column c of the tile is image column x0 - 8 + c, row r is image row y0 - 8 + r
    for (int i = tid; i < kPixH * (kPixW / 4); i += 256) {
        const int r = i / (kPixW / 4), q = i - r * (kPixW / 4);
        const uint8_t* __restrict__ row = img + (size_t)min(max(y0 - dog::kReach + r, 0), h - 1) * w;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (uint32_t)row[min(max(x0 - dog::kReach + 4 * q + b, 0), w - 1)] << (8 * b);
        pix[r][q] = v;
    }
    __syncthreads();
    // rows: H column c is image column x0 - 1 + c = pixel column c + 7; it reads pixel columns c .. c + 14
    for (int i = tid; i < kHRows * kQuads; i += 256) {
        const int r = i / kQuads, q = i - r * kQuads;
        int px[20];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const uint32_t v = pix[r][q + d];
#pragma unroll
            for (int b = 0; b < 4; ++b) px[4 * d + b] = (int)((v >> (8 * b)) & 0xFFu);
        }
        row_pass<0>(px, &H[0][r][4 * q]);
        row_pass<1>(px, &H[1][r][4 * q]);
        row_pass<2>(px, &H[2][r][4 * q]);
        row_pass<3>(px, &H[3][r][4 * q]);
    }
    __syncthreads();
    // cols: B row r is image row y0 - 1 + r = H row r + 7; it reads H rows r .. r + 14
    for (int i = tid; i < kBRows * kQuads; i += 256) {
        const int r = i / kQuads, q = i - r * kQuads;
        col_pass<0>(&H[0][r][4 * q], &B[0][r][4 * q]);
        col_pass<1>(&H[1][r][4 * q], &B[1][r][4 * q]);
        col_pass<2>(&H[2][r][4 * q], &B[2][r][4 * q]);
        col_pass<3>(&H[3][r][4 * q], &B[3][r][4 * q]);
    }
    __syncthreads();
    // test: output (lx, ly) is B position (lx + 1, ly + 1) and pixel position (lx + 8, ly + 8). A thread: columns 2 p, 2 p + 1 of rows
    // 2 v, 2 v + 1; the 4 x 4 B positions and the 6 x 6 pixels they see are read as whole dwords
    const int p2 = 2 * (tid & 31), ly0 = 2 * (tid >> 5);
    if (x0 + p2 < w && y0 + ly0 < h) {
        bool any_in = false;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int x = x0 + p2 + (o & 1), y = y0 + ly0 + (o >> 1);
            any_in = any_in || (x >= kBorder && x < w - kBorder && y >= kBorder && y < h - kBorder);
        }
        int d[dog::kLayers][4][4];
        if (any_in) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int b[dog::kBlurs][4];
#pragma unroll
                for (int k = 0; k < dog::kBlurs; ++k) {
                    const uint32_t* q = reinterpret_cast<const uint32_t*>(&B[k][ly0 + r][p2]);
                    const uint32_t lo = q[0], hi = q[1];
                    b[k][0] = (int)(lo & 0xFFFFu); b[k][1] = (int)(lo >> 16); b[k][2] = (int)(hi & 0xFFFFu); b[k][3] = (int)(hi >> 16);
                }
#pragma unroll
                for (int k = 0; k < dog::kLayers; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) d[k][r][c] = b[k + 1][c] - b[k][c];
            }
        }
        // 5 x 5 box sums: the six row sums per column that the two rows share; pixel columns p2 + 6 .. p2 + 11 from two aligned dwords
        const int c0 = p2 + dog::kReach - 2, sh = 8 * (c0 & 3);
        int rs[2][6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const uint32_t* q = &pix[ly0 + dog::kReach - 2 + r][c0 >> 2];
            const uint64_t v = ((uint64_t)q[0] | ((uint64_t)q[1] << 32)) >> sh;   // (c0 & 3 is 0 or 2: the six bytes are inside the two dwords)
            int px[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) px[i] = (int)((v >> (8 * i)) & 0xFFu);
            const int mid = px[1] + px[2] + px[3] + px[4];
            rs[0][r] = px[0] + mid;
            rs[1][r] = mid + px[5];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int ox = o & 1, oy = o >> 1, x = x0 + p2 + ox, y = y0 + ly0 + oy;
            if (x >= w || y >= h) continue;
            int sc = 0;
            if (x >= kBorder && x < w - kBorder && y >= kBorder && y < h - kBorder)
                sc = dog::candidate(contrast, [&](int k, int dx, int dy) { return d[k][oy + 1 + dy][ox + 1 + dx]; });
            const size_t at = (size_t)blockIdx.z * plane + (size_t)y * w + x;
            if constexpr (kRefine) {
                if (sc)
                    codes[at] = (uint16_t)dog::refine([&](int k, int dx, int dy) { return d[k][oy + 1 + dy][ox + 1 + dx]; }).code();
                else if (cand == nullptr)
                    codes[at] = 0;
            }
            if (!kRefine || cand != nullptr) cand[at] = (uint8_t)sc;
            if (sc) atomicAdd(&lh[sc], 1u);
            const int bs = (x >= 2 && x < w - 2 && y >= 2 && y < h - 2) ? rs[ox][oy] + rs[ox][oy + 1] + rs[ox][oy + 2] + rs[ox][oy + 3] + rs[ox][oy + 4] : 0;
            if (box != nullptr) box[at] = (uint16_t)bs;
        }
    }
    __syncthreads();
    if (hist != nullptr && lh[tid] != 0) atomicAdd(&hist[(size_t)blockIdx.z * 256 + tid], lh[tid]);
}

}  // namespace

// candidate plane and, unless nullptr, box sums and score histogram of n_images images of one size: what detect_level's later kernels read.
// d_codes != nullptr: the refinement's code plane as well, where d_cand is non-zero, or (d_cand == nullptr: the code planes alone) on every pixel
hipError_t launch_dog_maps(const uint8_t* d_images, int n_images, int w, int h, int contrast, uint8_t* d_cand, uint16_t* d_box, uint32_t* d_hist,
                           uint16_t* d_codes, hipStream_t stream)
{
    if (n_images <= 0) return hipSuccess;
    const dim3 grid((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, n_images);
    if (d_codes == nullptr)
        hipLaunchKernelGGL(dog_maps_kernel<false>, grid, dim3(256), 0, stream, d_images, w, h, contrast, d_cand, d_box, d_hist, d_codes);
    else
        hipLaunchKernelGGL(dog_maps_kernel<true>, grid, dim3(256), 0, stream, d_images, w, h, contrast, d_cand, d_box, d_hist, d_codes);
    return hipGetLastError();
}

}  // namespace gms
