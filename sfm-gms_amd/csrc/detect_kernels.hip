// detect_kernels.hip -- the keypoint source in front of the matcher: single-scale FAST-9 corners + steered-BRIEF rows, for gfx950.
//
// What the reference does here is OpenCV's (FeatureMatchUtil.cpp:9-12 SIFT::create(10000)->detectAndCompute;
// DisparityUtil.cpp:108,123-138 ORB::create(), detectAndCompute or compute() at every pixel): a binary dependency. This is the
// build's own minimal detector in its place, defined in integer arithmetic so that every result is
// exact: same keypoints, same order, same bits on every run and against the CPU statement of the definition.
//
//   image      8-bit grey, row-major, pitch = width; n_images of one size back to back. Keypoints sit at x in [16, W-16), y in [16, H-16).
//   FAST-9     d_i = I(circle_i) - I(p) on the 16-pixel circle of radius 3; score = max over the 16 arcs of nine contiguous pixels of
//              min d (bright arc) or min -d (dark arc), floored at 0 = the largest t for which the pixel still is a FAST-9 corner.
//              Candidate: score > threshold and score > all 8 neighbours' scores.
//   selection  the max_keypoints highest scores, equal scores in raster order; output in raster order (no sort: a 256-bin histogram
//              gives the cut-off score, per-row counts and a scan give every survivor its slot).
//   smoothing  S = 5 x 5 box sum (u16).
//   direction  integer moments over the disc of radius 15, the best of 32 directions by integer dot product; angle = 11.25 * bin.
//   rows       256 comparisons S(p + a_k) < S(p + b_k) of a fixed pseudo-random pattern (disc of radius 12) turned by the bin.
// Output: cv::KeyPoint records {x, y, 31, angle, score, 0, -1} and 32-byte rows -- what gms_frame_table / gms_bf_prepare_device take.
//
// Kernels (one launch each, every image of the batch in grid.y / grid.z):
//   det_maps_kernel      64 x 16 pixel tile (+3 halo) through LDS: FAST score (u8) and box sum (u16) per pixel. HBM: 1 B in, 3 B out.
//   det_nms_kernel       3 x 3 non-maximum suppression on the score image -> candidate image, per-image score histogram.
//   det_cut_kernel       the cut-off score and the quota of candidates AT the cut-off, from the histogram.
//   det_rows_kernel      per image row: candidates above / at the cut-off.
//   det_scan_kernel      exclusive scan of those over the rows.
//   det_emit_kernel      per image row: survivors to their slots (x, y, score), raster order.
//   det_describe_kernel  one wave per keypoint: moments by wave reduction, direction, 256 comparisons by four ballots.
// The same detector over an image pyramid (launch_detect_pyramid) adds
//   pyr_resize_kernel    a level from the level below it: integer bilinear, source rows through LDS, 4-byte loads and stores.
//   det_describe_kernel  in its per-level form: records behind the earlier levels', pt mapped to level 0, size and octave set.
//   (with d_rows128: grad_desc_kernels.hip's kernel behind every level's describe kernel -- DESIGN.md section 4.7c)
//   (with dog_contrast >= 0: dog_kernels.hip's dog_maps_kernel in the place of det_maps_kernel + det_nms_kernel -- DESIGN.md section 4.7d;
//    with refine: its form that stores the refinement's codes, and det_describe_kernel's form that reads them)
//   pyr_clear_kernel     zeroes the levels' counts and histograms; pyr_counts_kernel: the per-image and per-level counts for the caller.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dog_core.h"
#include "gms_kernels.h"

namespace gms {
namespace {

constexpr int kBins = 32;
constexpr int kTests = 256;
constexpr int kTileW = 64, kTileH = 16, kHalo = 3;

struct DirTable { int c[kBins], s[kBins]; };
__constant__ const DirTable kDir = {
    {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0, -799, -1567, -2276, -2896, -3406, -3784, -4017,
     -4096, -4017, -3784, -3406, -2896, -2276, -1567, -799, 0, 799, 1567, 2276, 2896, 3406, 3784, 4017},
    {0, 799, 1567, 2276, 2896, 3406, 3784, 4017, 4096, 4017, 3784, 3406, 2896, 2276, 1567, 799,
     0, -799, -1567, -2276, -2896, -3406, -3784, -4017, -4096, -4017, -3784, -3406, -2896, -2276, -1567, -799}};

// The comparison pattern, generated at compile time: a 32-bit linear congruential generator (1664525, 1013904223, seed 0x2545F491),
// coordinates (state >> 16) % 25 - 12, points outside the disc of radius 12 drawn again, b drawn again while it equals a.
struct Pattern { int8_t p[kTests][4]; };
constexpr Pattern make_pattern()
{
    Pattern t{};
    uint32_t state = 0x2545F491u;
    auto coord = [&state]() {
        state = state * 1664525u + 1013904223u;
        return (int)((state >> 16) % 25u) - 12;
    };
    for (int k = 0; k < kTests; ++k) {
        int ax = 0, ay = 0, bx = 0, by = 0;
        do { ax = coord(); ay = coord(); } while (ax * ax + ay * ay > 144);
        do {
            do { bx = coord(); by = coord(); } while (bx * bx + by * by > 144);
        } while (bx == ax && by == ay);
        t.p[k][0] = (int8_t)ax; t.p[k][1] = (int8_t)ay; t.p[k][2] = (int8_t)bx; t.p[k][3] = (int8_t)by;
    }
    return t;
}
__constant__ const Pattern kPattern = make_pattern();

__device__ __forceinline__ int min3i(int a, int b, int c) { return min(a, min(b, c)); }

// ---- FAST score + box sum ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
det_maps_kernel(const uint8_t* __restrict__ images, int w, int h, uint8_t* __restrict__ score, uint16_t* __restrict__ box)
{
    constexpr int LW = kTileW + 2 * kHalo, LH = kTileH + 2 * kHalo;   // 70 x 22
    __shared__ uint8_t tile[LH][LW + 2];
    const size_t plane = (size_t)w * h;
    const uint8_t* __restrict__ img = images + (size_t)blockIdx.z * plane;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int x = min(max(x0 + lx - kHalo, 0), w - 1), y = min(max(y0 + ly - kHalo, 0), h - 1);   // (clamped reads: values there are never used)
        tile[ly][lx] = img[(size_t)y * w + x];
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & 63, ry = (int)threadIdx.x >> 6;   // a thread: one column, rows ry, ry + 4, ry + 8, ry + 12
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = ry + 4 * j, x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const int cx = lx + kHalo, cy = ly + kHalo;
        int sc = 0;
        if (x >= kBorder && x < w - kBorder && y >= kBorder && y < h - kBorder) {
            const int p = tile[cy][cx];
            int d[16];
            d[0] = tile[cy - 3][cx] - p;      d[1] = tile[cy - 3][cx + 1] - p;  d[2] = tile[cy - 2][cx + 2] - p;  d[3] = tile[cy - 1][cx + 3] - p;
            d[4] = tile[cy][cx + 3] - p;      d[5] = tile[cy + 1][cx + 3] - p;  d[6] = tile[cy + 2][cx + 2] - p;  d[7] = tile[cy + 3][cx + 1] - p;
            d[8] = tile[cy + 3][cx] - p;      d[9] = tile[cy + 3][cx - 1] - p;  d[10] = tile[cy + 2][cx - 2] - p; d[11] = tile[cy + 1][cx - 3] - p;
            d[12] = tile[cy][cx - 3] - p;     d[13] = tile[cy - 1][cx - 3] - p; d[14] = tile[cy - 2][cx - 2] - p; d[15] = tile[cy - 3][cx - 1] - p;
            // window minima / maxima by doubling: 2, 4, 8, then the ninth value
            int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { lo2[i] = min(d[i], d[(i + 1) & 15]); hi2[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
            for (int i = 0; i < 16; ++i) { lo4[i] = min(lo2[i], lo2[(i + 2) & 15]); hi4[i] = max(hi2[i], hi2[(i + 2) & 15]); }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int lo9 = min3i(lo4[i], lo4[(i + 4) & 15], d[(i + 8) & 15]);
                const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
                sc = max(sc, max(lo9, -hi9));
            }
        }
        score[(size_t)blockIdx.z * plane + (size_t)y * w + x] = (uint8_t)sc;
        int bs = 0;
        if (x >= 2 && x < w - 2 && y >= 2 && y < h - 2) {
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) bs += tile[cy + dy][cx + dx];
        }
        box[(size_t)blockIdx.z * plane + (size_t)y * w + x] = (uint16_t)bs;
    }
}

// ---- non-maximum suppression + histogram of the candidates' scores --------------------------------------------------------------------
__global__ void __launch_bounds__(256)
det_nms_kernel(const uint8_t* __restrict__ score, int w, int h, int threshold, uint8_t* __restrict__ cand, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const size_t plane = (size_t)w * h;
    const uint8_t* __restrict__ sc = score + (size_t)blockIdx.z * plane;
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    if (x < w && y < h) {
        int keep = 0;
        if (x >= kBorder && x < w - kBorder && y >= kBorder && y < h - kBorder) {   // (so every neighbour is inside the image)
            const int s = sc[(size_t)y * w + x];
            if (s > threshold) {
                const uint8_t* r0 = sc + (size_t)(y - 1) * w + x;
                const uint8_t* r1 = r0 + w;
                const uint8_t* r2 = r1 + w;
                const int m = max(max(max(r0[-1], r0[0]), max(r0[1], r1[-1])), max(max(r1[1], r2[-1]), max(r2[0], r2[1])));
                if (s > m) keep = s;
            }
        }
        cand[(size_t)blockIdx.z * plane + (size_t)y * w + x] = (uint8_t)keep;
        if (keep) atomicAdd(&lh[keep], 1u);
    }
    __syncthreads();
    if (lh[threadIdx.x] != 0) atomicAdd(&hist[(size_t)blockIdx.z * 256 + threadIdx.x], lh[threadIdx.x]);
}

// cut[img] = {cut-off score, quota at the cut-off, keypoints kept, candidates}
__global__ void __launch_bounds__(256)
det_cut_kernel(const uint32_t* __restrict__ hist, int max_keypoints, int32_t* __restrict__ cut, int32_t* __restrict__ counts)
{
    __shared__ uint32_t above[257];   // above[s] = candidates with score >= s
    const uint32_t* hh = hist + (size_t)blockIdx.x * 256;
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        above[256] = 0;
        for (int s = 255; s >= 0; --s) {
            run += hh[s];
            above[s] = run;
        }
    }
    __syncthreads();
    const uint32_t total = above[0];
    int32_t* out = cut + (size_t)blockIdx.x * 4;
    if (total <= (uint32_t)max_keypoints) {
        if (threadIdx.x == 0) {
            out[0] = 0; out[1] = 0; out[2] = (int32_t)total; out[3] = (int32_t)total;
            counts[blockIdx.x] = (int32_t)total;
        }
        return;
    }
    // the score s with above[s + 1] < max_keypoints <= above[s] (unique; s >= 1 because no candidate scores 0)
    const int s = (int)threadIdx.x;
    if (above[s + 1] < (uint32_t)max_keypoints && above[s] >= (uint32_t)max_keypoints) {
        out[0] = s; out[1] = max_keypoints - (int32_t)above[s + 1]; out[2] = max_keypoints; out[3] = (int32_t)total;
        counts[blockIdx.x] = max_keypoints;
    }
}

// per row: [0] candidates above the cut-off, [1] at it
__global__ void __launch_bounds__(64)
det_rows_kernel(const uint8_t* __restrict__ cand, int w, int h, const int32_t* __restrict__ cut, uint32_t* __restrict__ rows)
{
    const int y = (int)blockIdx.x, img = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int c = cut[(size_t)img * 4];
    const uint8_t* __restrict__ row = cand + (size_t)img * w * h + (size_t)y * w;
    uint32_t gt = 0, eq = 0;
    for (int x = lane; x < w; x += 64) {
        const int s = row[x];
        gt += s > c ? 1u : 0u;
        eq += (s == c && s != 0) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        gt += (uint32_t)__shfl_xor((int)gt, d);
        eq += (uint32_t)__shfl_xor((int)eq, d);
    }
    if (lane == 0) {
        rows[((size_t)img * h + y) * 2] = gt;
        rows[((size_t)img * h + y) * 2 + 1] = eq;
    }
}

// exclusive scan over the rows, in place: rows[y] = {candidates above the cut-off before row y, candidates at it before row y}
__global__ void __launch_bounds__(1024)
det_scan_kernel(uint32_t* __restrict__ rows, int h)
{
    __shared__ uint32_t part[2][1024];
    uint32_t* r = rows + (size_t)blockIdx.x * h * 2;
    const int tid = (int)threadIdx.x, per = (h + 1023) / 1024;
    uint32_t a = 0, b = 0;
    for (int i = 0; i < per; ++i) {
        const int y = tid * per + i;
        if (y < h) { a += r[2 * y]; b += r[2 * y + 1]; }
    }
    part[0][tid] = a; part[1][tid] = b;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // Hillis-Steele inclusive scan
        const uint32_t pa = tid >= d ? part[0][tid - d] : 0u, pb = tid >= d ? part[1][tid - d] : 0u;
        __syncthreads();
        part[0][tid] += pa; part[1][tid] += pb;
        __syncthreads();
    }
    uint32_t ra = part[0][tid] - a, rb = part[1][tid] - b;   // exclusive prefix of this thread's rows
    for (int i = 0; i < per; ++i) {
        const int y = tid * per + i;
        if (y < h) {
            const uint32_t ca = r[2 * y], cb = r[2 * y + 1];
            r[2 * y] = ra; r[2 * y + 1] = rb;
            ra += ca; rb += cb;
        }
    }
}

// survivors of a row to their slots: slot = (above before) + min(at-cut before, quota) + rank inside the row
__global__ void __launch_bounds__(64)
det_emit_kernel(const uint8_t* __restrict__ cand, int w, int h, const int32_t* __restrict__ cut, const uint32_t* __restrict__ rows,
                int max_keypoints, uint32_t* __restrict__ list)
{
    const int y = (int)blockIdx.x, img = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int c = cut[(size_t)img * 4];
    const uint32_t quota = (uint32_t)cut[(size_t)img * 4 + 1];
    uint32_t gt_run = rows[((size_t)img * h + y) * 2], eq_run = rows[((size_t)img * h + y) * 2 + 1];
    const uint8_t* __restrict__ row = cand + (size_t)img * w * h + (size_t)y * w;
    uint32_t* __restrict__ out = list + (size_t)img * max_keypoints * 2;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const int s = x < w ? row[x] : 0;
        const bool gt = s > c, eq = s == c && s != 0;
        const uint64_t mg = __ballot(gt), me = __ballot(eq);
        const uint32_t eq_rank = eq_run + (uint32_t)__popcll(me & below);
        const bool take = gt || (eq && eq_rank < quota);
        if (take) {
            const uint32_t eq_before = min(eq_run + (uint32_t)__popcll(me & below), quota);   // at-cut survivors before this one
            const uint32_t slot = gt_run + (uint32_t)__popcll(mg & below) + eq_before;
            if (slot < (uint32_t)max_keypoints) {
                out[2 * slot] = (uint32_t)x | ((uint32_t)y << 16);
                out[2 * slot + 1] = (uint32_t)s;
            }
        }
        gt_run += (uint32_t)__popcll(mg);
        eq_run += (uint32_t)__popcll(me);
    }
}

// ---- direction + descriptor: one wave per keypoint ---------------------------------------------------------------------------------------
// Where the keypoints come from and where the records go:
//   kAtRecords   from the caller's records (compute()); only the angle is written.
//   kFromList    from det_emit_kernel's list; record k of image img goes to slot img * max_keypoints + k.
//   kFromLevel   the same list, of pyramid level `level` (max_keypoints = the level's quota): the record goes behind the earlier levels'
//                survivors in the image's block of out_stride records, pt mapped to level 0, size and octave of the level.
//   kFromLevelRefined   kFromLevel behind the DoG detector's refining form: x, y and size of the record are moved by the offsets that
//                dog_maps_kernel<true> left in `codes` at the keypoint's pixel. Direction, response and
//                the row are those of the integer pixel.
enum { kAtRecords = 0, kFromList = 1, kFromLevel = 2, kFromLevelRefined = 3 };
struct LevelOut {
    const int32_t* level_counts;   // [level][image]: survivors of the levels (this level's row is `counts`)
    int level, n_images, out_stride;
    float fx, fy;                  // (float)w_0 / (float)w_level, (float)h_0 / (float)h_level
    uint16_t* codes;               // kFromLevelRefined: the level's plane of dog_core.h's refinement codes, [image][h][w] (detect_level has
                                   // dog_maps_kernel<true> write it; the describe kernel only reads it)
};

template <int MODE>
__global__ void __launch_bounds__(256)
det_describe_kernel(const uint8_t* __restrict__ images, const uint16_t* __restrict__ box, int w, int h, const uint32_t* __restrict__ list,
                    const int32_t* __restrict__ counts, int max_keypoints, gms_keypoint* __restrict__ kp, uint8_t* __restrict__ desc,
                    int32_t* __restrict__ status, LevelOut lo)
{
    constexpr bool FROM_LIST = MODE != kAtRecords;
    const int lane = (int)threadIdx.x & 63, img = (int)blockIdx.y;
    const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int n = counts != nullptr ? min(counts[img], max_keypoints) : max_keypoints;
    if (k >= n) return;   // wave-uniform
    const size_t plane = (size_t)w * h;
    const uint8_t* __restrict__ im = images + (size_t)img * plane;
    const uint16_t* __restrict__ bx = box + (size_t)img * plane;
    size_t slot = (size_t)img * max_keypoints + k;
    if constexpr (MODE == kFromLevel || MODE == kFromLevelRefined) {
        int before = 0;   // (the levels' counts sum to at most out_stride: the quotas do)
        for (int j = 0; j < lo.level; ++j) before += lo.level_counts[(size_t)j * lo.n_images + img];
        slot = (size_t)img * lo.out_stride + before + k;
    }
    gms_keypoint* rec = kp + slot;
    int x, y, sc = 0;
    if constexpr (FROM_LIST) {
        const uint32_t xy = list[((size_t)img * max_keypoints + k) * 2];
        x = (int)(xy & 0xFFFFu); y = (int)(xy >> 16);
        sc = (int)list[((size_t)img * max_keypoints + k) * 2 + 1];
    } else {
        const float fx = rec->x, fy = rec->y;
        x = (int)fx; y = (int)fy;
        const bool ok = (float)x == fx && (float)y == fy && x >= kBorder && y >= kBorder && x < w - kBorder && y < h - kBorder;
        if (!ok) {   // wave-uniform; the caller sees the flag, the row stays as it was
            if (lane == 0) atomicMax(status, 1);
            return;
        }
    }
    // moments over the disc of radius 15: 31 x 31 positions, 64 at a time
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
    // the best of 32 directions: key = dot << 5 | (31 - k), so the maximum is the largest dot product, then the lowest k
    const int kk = lane & 31;
    long long key = (((long long)m10 * kDir.c[kk] + (long long)m01 * kDir.s[kk]) << 5) | (long long)(31 - kk);
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    const int bin = 31 - (int)(key & 31);
    const int c = kDir.c[bin], s = kDir.s[bin];
    uint64_t bits[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = 64 * j + lane;
        const int ax = kPattern.p[t][0], ay = kPattern.p[t][1], bxx = kPattern.p[t][2], by = kPattern.p[t][3];
        const int rax = (ax * c - ay * s + 2048) >> 12, ray = (ax * s + ay * c + 2048) >> 12;
        const int rbx = (bxx * c - by * s + 2048) >> 12, rby = (bxx * s + by * c + 2048) >> 12;
        const int va = bx[(size_t)(y + ray) * w + (x + rax)], vb = bx[(size_t)(y + rby) * w + (x + rbx)];
        bits[j] = __ballot(va < vb);
    }
    if (lane < 4) reinterpret_cast<uint64_t*>(desc + slot * 32)[lane] = bits[lane & 3];
    if (lane == 0) {
        if constexpr (MODE == kFromLevelRefined) {   // (the code is non-zero: the list holds candidates only)
            const dog::Offsets o = dog::offsets_of((int)lo.codes[(size_t)img * plane + (size_t)y * w + x]);
            gms_keypoint r;
            r.x = dog::refined_coord(x, o.ox, lo.fx); r.y = dog::refined_coord(y, o.oy, lo.fy); r.size = dog::refined_size(o.os, lo.fx);
            r.angle = 11.25f * (float)bin; r.response = (float)sc; r.octave = lo.level; r.class_id = -1;
            *rec = r;
        } else if constexpr (MODE == kFromLevel) {   // pixel centres aligned; every operation rounded once (-ffp-contract=off)
            gms_keypoint r;
            r.x = ((float)x + 0.5f) * lo.fx - 0.5f; r.y = ((float)y + 0.5f) * lo.fy - 0.5f; r.size = 31.0f * lo.fx;
            r.angle = 11.25f * (float)bin; r.response = (float)sc; r.octave = lo.level; r.class_id = -1;
            *rec = r;
        } else if constexpr (MODE == kFromList) {
            gms_keypoint r;
            r.x = (float)x; r.y = (float)y; r.size = 31.0f; r.angle = 11.25f * (float)bin; r.response = (float)sc; r.octave = 0; r.class_id = -1;
            *rec = r;
        } else {
            rec->angle = 11.25f * (float)bin;
        }
    }
}

// ---- pyramid: a level from the level below it -----------------------------------------------------------------------------------------
// Bilinear, pixel centres aligned, 8-bit fixed-point weights, all integer: for output column x
//   X = floor((2x + 1) * w_src * 128 / w_dst) - 128 (>= 0 because w_src >= w_dst), x0 = X >> 8, ax = X & 255, x1 = min(x0 + 1, w_src - 1),
// the same for rows, out = ((256 - ax)(256 - ay) p00 + ax (256 - ay) p01 + (256 - ax) ay p10 + ax ay p11 + 32768) >> 16.
// A workgroup makes 64 x 16 output pixels, a thread four of one row as one aligned 4-byte store: rows of pitch = width start at any
// address, so the tile of row y starts (address of the row's first pixel) & 3 pixels early and the bytes that fall outside the row at
// its two ends are stored one by one. The source rows come through LDS with aligned 4-byte loads in the same way: a row is loaded
// from the 4-byte boundary at or below its first pixel and remembered with that shift. The level rule keeps w_src / w_dst and
// h_src / h_dst at or below 1.2 + 0.4 / 33, so the 67 columns a tile can touch span at most 83 source pixels (+ 3 of shift) and its 16
// rows at most 21 source rows.
constexpr int kRzCols = 64 + 3, kRzRows = 16, kRzSrcRows = 22, kRzPitch = 96;

__global__ void __launch_bounds__(256)
pyr_resize_kernel(const uint8_t* __restrict__ src, int ws, int hs, uint8_t* __restrict__ dst, int wd, int hd, size_t src_bytes)
{
    __shared__ uint32_t tile[kRzSrcRows][kRzPitch / 4];
    __shared__ int col_x[kRzCols], row_y[kRzRows];
    const int tid = (int)threadIdx.x;
    const int xo0 = (int)blockIdx.x * 64 - 3, yo0 = (int)blockIdx.y * kRzRows;   // first output column / row this tile may hold
    if (tid < kRzCols) {
        const int x = min(max(xo0 + tid, 0), wd - 1);
        col_x[tid] = (int)((uint64_t)(2 * x + 1) * (uint64_t)ws * 128u / (uint64_t)wd) - 128;
    } else if (tid >= 128 && tid < 128 + kRzRows) {
        const int y = min(yo0 + tid - 128, hd - 1);
        row_y[tid - 128] = (int)((uint64_t)(2 * y + 1) * (uint64_t)hs * 128u / (uint64_t)hd) - 128;
    }
    __syncthreads();
    const int xs0 = col_x[0] >> 8, ys0 = row_y[0] >> 8;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(src), hi = lo + src_bytes;
    const uintptr_t im = lo + (size_t)blockIdx.z * ws * hs;
    for (int i = tid; i < kRzSrcRows * (kRzPitch / 4); i += 256) {
        const int r = i / (kRzPitch / 4), j = i - r * (kRzPitch / 4);
        const uintptr_t a = ((im + (size_t)min(ys0 + r, hs - 1) * ws + xs0) & ~(uintptr_t)3) + 4u * (unsigned)j;
        uint32_t v = 0;
        if (a >= lo && a + 4 <= hi) {
            v = *reinterpret_cast<const uint32_t*>(a);
        } else {   // the 4 bytes straddle an end of the batch: the ones inside it, one by one
            for (int b = 0; b < 4; ++b)
                if (a + b >= lo && a + b < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + b) << (8 * b);
        }
        tile[r][j] = v;
    }
    __syncthreads();
    const int y = yo0 + (tid >> 4);
    if (y >= hd) return;
    uint8_t* __restrict__ out_row = dst + (size_t)blockIdx.z * wd * hd + (size_t)y * wd;
    const int xf = (int)blockIdx.x * 64 + 4 * (tid & 15) - (int)(reinterpret_cast<uintptr_t>(out_row) & 3);   // out_row + xf is 4-byte aligned
    const int Y = row_y[tid >> 4], y0 = Y >> 8, ay = Y & 255, y1 = min(y0 + 1, hs - 1);
    const uint8_t* r0 = reinterpret_cast<const uint8_t*>(tile[y0 - ys0]);   // source pixel x of a row sits at byte x + o of its LDS row
    const uint8_t* r1 = reinterpret_cast<const uint8_t*>(tile[y1 - ys0]);
    const int o0 = (int)((im + (size_t)y0 * ws + xs0) & 3) - xs0, o1 = (int)((im + (size_t)y1 * ws + xs0) & 3) - xs0;
    uint32_t packed = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int X = col_x[xf + q - xo0], x0 = X >> 8, ax = X & 255, x1 = min(x0 + 1, ws - 1);
        const uint32_t top = (uint32_t)(256 - ax) * r0[o0 + x0] + (uint32_t)ax * r0[o0 + x1];
        const uint32_t bot = (uint32_t)(256 - ax) * r1[o1 + x0] + (uint32_t)ax * r1[o1 + x1];
        packed |= (((uint32_t)(256 - ay) * top + (uint32_t)ay * bot + 32768u) >> 16) << (8 * q);
    }
    if (xf >= 0 && xf + 3 < wd) {
        *reinterpret_cast<uint32_t*>(out_row + xf) = packed;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (xf + q >= 0 && xf + q < wd) out_row[xf + q] = (uint8_t)(packed >> (8 * q));
    }
}

// zeroes the levels' counts and score histograms at the head of a call (a kernel, not a memset: the call is one chain of kernel launches,
// which is what the other graph-captured batch calls of this library are)
__global__ void __launch_bounds__(256)
pyr_clear_kernel(uint32_t* __restrict__ words, size_t n_words)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (size_t)gridDim.x * 256) words[i] = 0;
}

// the caller's counts from the levels' [level][image] counts: counts[img] = the sum, level_counts[img][l] (0 for levels not used)
__global__ void __launch_bounds__(256)
pyr_counts_kernel(const int32_t* __restrict__ lvl, int n_images, int n_used, int n_levels, int32_t* __restrict__ counts, int32_t* __restrict__ level_counts)
{
    const int img = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (img >= n_images) return;
    int sum = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int v = l < n_used ? lvl[(size_t)l * n_images + img] : 0;
        level_counts[(size_t)img * n_levels + l] = v;
        sum += v;
    }
    counts[img] = sum;
}

}  // namespace

size_t detect_workspace_bytes(int w, int h, int n_images, int max_keypoints)
{
    if (w <= 0 || h <= 0 || n_images <= 0 || max_keypoints < 0) return 0;
    return detect_layout(w, h, n_images, max_keypoints).total;
}

namespace {
struct DetWs { uint8_t* score; uint8_t* cand; uint16_t* box; uint32_t* hist; int32_t* cut; uint32_t* rows; uint32_t* list; size_t hist_bytes; };
DetWs carve(void* ws, int w, int h, int n_images, int max_keypoints)
{
    const DetectLayout L = detect_layout(w, h, n_images, max_keypoints);
    return {ws_ptr<uint8_t>(ws, L.score), ws_ptr<uint8_t>(ws, L.cand), ws_ptr<uint16_t>(ws, L.box), ws_ptr<uint32_t>(ws, L.hist),
            ws_ptr<int32_t>(ws, L.cut), ws_ptr<uint32_t>(ws, L.rows), ws_ptr<uint32_t>(ws, L.list), L.cut - L.hist};
}

// FAST scores and box sums of a batch
void launch_maps(const uint8_t* d_images, int n_images, int w, int h, const DetWs& ws, hipStream_t stream)
{
    hipLaunchKernelGGL(det_maps_kernel, dim3((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, n_images), dim3(256), 0, stream, d_images, w, h,
                       ws.score, ws.box);
}

// the detector on one set of equally sized images: the single-scale call (lo == nullptr; clears its histogram itself; never refined) or one
// level of the pyramid (lo and the level's histogram, already cleared; refined records go through lo->codes). With the DoG detector the
// candidates are dog_kernels.hip's; what follows the candidate plane is the same.
hipError_t detect_level(const PyramidRun& run, const uint8_t* d_images, int n_images, int w, int h, int max_keypoints, void* d_ws, gms_keypoint* d_kp,
                        uint8_t* d_desc, int32_t* d_counts, const LevelOut* lo, uint32_t* level_hist, hipStream_t stream)
{
    DetWs ws = carve(d_ws, w, h, n_images, max_keypoints);
    if (level_hist != nullptr) {
        ws.hist = level_hist;
    } else {
        hipError_t e = hipMemsetAsync(ws.hist, 0, ws.hist_bytes, stream);
        if (e != hipSuccess) return e;
    }
    const bool refined = run.refined && lo != nullptr;
    if (run.detector == PyramidRun::kDog) {
        hipError_t e = launch_dog_maps(d_images, n_images, w, h, run.strength, ws.cand, ws.box, ws.hist, refined ? lo->codes : nullptr, stream);
        if (e != hipSuccess) return e;
    } else {
        launch_maps(d_images, n_images, w, h, ws, stream);
        hipLaunchKernelGGL(det_nms_kernel, dim3((w + 63) / 64, (h + 3) / 4, n_images), dim3(256), 0, stream, ws.score, w, h, run.strength, ws.cand, ws.hist);
    }
    hipLaunchKernelGGL(det_cut_kernel, dim3(n_images), dim3(256), 0, stream, ws.hist, max_keypoints, ws.cut, d_counts);
    hipLaunchKernelGGL(det_rows_kernel, dim3(h, n_images), dim3(64), 0, stream, ws.cand, w, h, ws.cut, ws.rows);
    hipLaunchKernelGGL(det_scan_kernel, dim3(n_images), dim3(1024), 0, stream, ws.rows, h);
    hipLaunchKernelGGL(det_emit_kernel, dim3(h, n_images), dim3(64), 0, stream, ws.cand, w, h, ws.cut, ws.rows, max_keypoints, ws.list);
    if (max_keypoints > 0) {
        const dim3 grid((max_keypoints + 3) / 4, n_images);
        if (refined)
            hipLaunchKernelGGL(det_describe_kernel<kFromLevelRefined>, grid, dim3(256), 0, stream, d_images, ws.box, w, h, ws.list, d_counts,
                               max_keypoints, d_kp, d_desc, (int32_t*)nullptr, *lo);
        else if (lo != nullptr)
            hipLaunchKernelGGL(det_describe_kernel<kFromLevel>, grid, dim3(256), 0, stream, d_images, ws.box, w, h, ws.list, d_counts, max_keypoints,
                               d_kp, d_desc, (int32_t*)nullptr, *lo);
        else
            hipLaunchKernelGGL(det_describe_kernel<kFromList>, grid, dim3(256), 0, stream, d_images, ws.box, w, h, ws.list, d_counts, max_keypoints,
                               d_kp, d_desc, (int32_t*)nullptr, LevelOut{});
    }
    return hipGetLastError();
}
}  // namespace

hipError_t launch_detect(const uint8_t* d_images, int n_images, int w, int h, int threshold, int max_keypoints, void* d_ws,
                         gms_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts, hipStream_t stream)
{
    if (n_images <= 0) return hipSuccess;
    return detect_level({PyramidRun::kFast, threshold, false}, d_images, n_images, w, h, max_keypoints, d_ws, d_kp, d_desc, d_counts, nullptr, nullptr,
                        stream);
}

// FAST scores and box sums of a batch alone, into a detect_layout workspace (what the gradient descriptor's compute() starts from)
hipError_t launch_detect_maps(const uint8_t* d_images, int n_images, int w, int h, void* d_ws, hipStream_t stream)
{
    if (n_images <= 0) return hipSuccess;
    launch_maps(d_images, n_images, w, h, carve(d_ws, w, h, n_images, 0), stream);
    return hipGetLastError();
}

// compute(): directions and rows at the caller's keypoints of ONE image; *d_status = 1 when a keypoint is off the pixel grid or outside the
// keypoint region (its row is left alone)
hipError_t launch_describe(const uint8_t* d_image, int w, int h, gms_keypoint* d_kp, int n, void* d_ws, uint8_t* d_desc, int32_t* d_status,
                           hipStream_t stream)
{
    const DetWs ws = carve(d_ws, w, h, 1, 0);
    hipError_t e = hipMemsetAsync(d_status, 0, 4, stream);
    if (e != hipSuccess) return e;
    launch_maps(d_image, 1, w, h, ws, stream);
    if (n > 0)
        hipLaunchKernelGGL(det_describe_kernel<kAtRecords>, dim3((n + 3) / 4, 1), dim3(256), 0, stream, d_image, ws.box, w, h, (const uint32_t*)nullptr,
                           (const int32_t*)nullptr, n, d_kp, d_desc, d_status, LevelOut{});
    return hipGetLastError();
}

// ---- the pyramid keypoint source --------------------------------------------------------------------------------
// (the levels' sizes, pyramid_level_sizes, are part of the workspace's layout: ws_layout.h)
// q_l = max_keypoints * area_l / (sum of the areas) in 64-bit integers; what the division leaves goes to level 0
void pyramid_quotas(const int* widths, const int* heights, int n, int max_keypoints, int* quotas)
{
    int64_t total = 0, given = 0;
    for (int l = 0; l < n; ++l) total += (int64_t)widths[l] * heights[l];
    for (int l = 1; l < n; ++l) {
        quotas[l] = (int)((int64_t)max_keypoints * widths[l] * heights[l] / total);
        given += quotas[l];
    }
    if (n > 0) quotas[0] = (int)(max_keypoints - given);
}

hipError_t launch_pyramid_build(const uint8_t* d_images, int n_images, int w, int h, int n_levels, uint8_t* d_levels, hipStream_t stream)
{
    int ww[kPyramidMaxLevels], hh[kPyramidMaxLevels];
    const int n = pyramid_level_sizes(w, h, n_levels, ww, hh);
    if (n_images <= 0) return hipSuccess;
    const uint8_t* src = d_images;
    uint8_t* dst = d_levels;
    for (int l = 1; l < n; ++l) {
        const size_t src_bytes = (size_t)ww[l - 1] * hh[l - 1] * n_images;
        hipLaunchKernelGGL(pyr_resize_kernel, dim3((ww[l] + 3 + 63) / 64, (hh[l] + kRzRows - 1) / kRzRows, n_images), dim3(256), 0, stream, src, ww[l - 1],
                           hh[l - 1], dst, ww[l], hh[l], src_bytes);
        src = dst;
        dst += (size_t)ww[l] * hh[l] * n_images;
    }
    return hipGetLastError();
}

size_t detect_pyramid_workspace_bytes(int w, int h, int n_images, int max_keypoints, int n_levels, bool refined)
{
    if (detect_workspace_bytes(w, h, n_images, max_keypoints) == 0 || n_levels < 1 || n_levels > kPyramidMaxLevels) return 0;
    return pyramid_layout(w, h, n_images, max_keypoints, n_levels, refined).total;
}

hipError_t launch_detect_pyramid(const PyramidRun& run, const uint8_t* d_images, int n_images, int w, int h, int max_keypoints, int n_levels, void* d_ws,
                                 gms_keypoint* d_kp, uint8_t* d_desc, float* d_rows128, int32_t* d_counts, int32_t* d_level_counts, hipStream_t stream)
{
    if (n_images <= 0) return hipSuccess;
    int ww[kPyramidMaxLevels], hh[kPyramidMaxLevels], quota[kPyramidMaxLevels];
    const int n = pyramid_level_sizes(w, h, n_levels, ww, hh);
    pyramid_quotas(ww, hh, n, max_keypoints, quota);
    const PyramidLayout L = pyramid_layout(w, h, n_images, max_keypoints, n_levels, run.refined);
    uint8_t* levels = ws_ptr<uint8_t>(d_ws, L.levels);
    int32_t* lvl_counts = ws_ptr<int32_t>(d_ws, L.counts);
    uint32_t* hists = ws_ptr<uint32_t>(d_ws, L.hists);
    void* det_ws = ws_ptr<char>(d_ws, L.detect);
    uint16_t* codes = run.refined ? ws_ptr<uint16_t>(d_ws, L.codes) : nullptr;
    const size_t clear_words = (L.detect - L.counts) / 4;
    hipLaunchKernelGGL(pyr_clear_kernel, dim3((unsigned)((clear_words + 255) / 256 < 1024 ? (clear_words + 255) / 256 : 1024)), dim3(256), 0, stream,
                       reinterpret_cast<uint32_t*>(lvl_counts), clear_words);
    hipError_t e = launch_pyramid_build(d_images, n_images, w, h, n_levels, levels, stream);
    if (e != hipSuccess) return e;
    const uint8_t* img = d_images;
    for (int l = 0; l < n; ++l) {
        if (quota[l] > 0) {
            const LevelOut lo = {lvl_counts, l, n_images, max_keypoints, (float)w / (float)ww[l], (float)h / (float)hh[l], codes};
            e = detect_level(run, img, n_images, ww[l], hh[l], quota[l], det_ws, d_kp, d_desc, lvl_counts + (size_t)l * n_images, &lo,
                             hists + (size_t)l * n_images * 256, stream);
            if (e != hipSuccess) return e;
            if (d_rows128 != nullptr) {   // while the level's box sums and list are still in the workspace
                e = launch_grad_level(n_images, ww[l], hh[l], quota[l], det_ws, lvl_counts, l, max_keypoints, d_kp, d_rows128, stream);
                if (e != hipSuccess) return e;
            }
        }
        img = l == 0 ? levels : img + (size_t)ww[l] * hh[l] * n_images;
    }
    hipLaunchKernelGGL(pyr_counts_kernel, dim3((n_images + 255) / 256), dim3(256), 0, stream, lvl_counts, n_images, n, n_levels, d_counts, d_level_counts);
    return hipGetLastError();
}

}  // namespace gms
