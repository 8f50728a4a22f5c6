// gms_kernels.hip -- hand-written HIP kernels for gfx950 (CDNA4): the GMS match filter. Read this first: the overview of the
// per-pair kernels (each form in a file of its own, named below), then the small kernels around them and the public launchers.
//
// What the reference does per pair (cv::xfeatures2d::matchGMS, opencv_xfeatures2d452.dll; SURVEY.md
// section 8a) is a dense 400 x N_right int32 "motion" matrix that is zeroed, filled and scanned 4 times
// per hypothesis. One 1024-thread workgroup owns one image pair and keeps the pair's whole state in
// registers and in the CU's 160 KB LDS, in one of two forms:
//
//   filter_kernel_dense / dense_pair_plain(), dense_pair_rot()   [gms_kernel_dense.hip; layout and shared blocks: gms_kernel_dense.h]
//               no scale hypotheses (right grid 20 x 20) and no left cell above 255
//               matches: the 400 x 400 matrix itself, one BYTE per entry, fills the LDS; binning is one
//               returning atomic per match, verification reads neighbour counts directly, the DMatch records
//               stay in registers from load to copy-out. dense_pair_plain() is the default-flags body (the headline: written
//               around its instruction count, touches the next workgroup's records ahead, non-temporal record traffic),
//               dense_pair_rot() the one with rotation hypotheses; both are described in front of them there. Pairs that
//               do not qualify are handed to hash_pair() by the same workgroup before anything is written.
//   filter_kernel_dense_scales / dense_scales_pair()   [gms_kernel_scales.hip]
//               scale hypotheses on the same byte matrix with a runtime row stride:
//               scales 0..3 evaluated (scale 1 first), every later one -- and scale 4 -- bounded first by a probe that bins
//               without verifying and lets a scale skip when it cannot win; leaves a per-pair record for
//   filter_kernel / hash_pair()          [gms_kernel_hash.hip; the body and its table helpers: gms_kernel_hash.h]
//               everything else (scale 4 when it has to be evaluated, crowded cells, the fallback of
//               both kernels above): the matrix has at most M non-zeros and is kept as a hash table --
//
//   code[KPT]   (registers) one dword per match: right cell of the current scale, half-cell index of the
//               left point (it carries the left cell under all four grid types), 8 per-rotation inlier bits
//   nfine       40 x 40 half-cell histogram of the left points: nLeft of any cell of any grid type is a
//               sum of at most four entries, so there is no counting pass per grid type
//   tab         the non-zeros of the motion matrix of the current (scale, grid type): every left cell owns
//               a region = 1 header bucket + data buckets of four [right cell : 11 | count : 21] slots
//               (one ds_read_b128 sees a bucket); built with LDS atomics, the header keeps the running
//               arg-max of the row (highest count, lowest right cell) via atomicMin on the inverted key
//   nleft4 / desc4 / fdesc4   per grid type: nLeft and region of every cell, and the same region seen from
//               every half-cell (a match finds its region with one LDS read, no left-cell arithmetic)
//   fres        per half-cell: (j*, rotation bits that pass the threshold) of the cell it falls in
//
// Rotation only changes which neighbour counts are summed, so one table build serves all 8 rotations;
// the right cell only depends on the scale, the left cell only on the grid type. No MFMA: integer
// histogramming. Measured on MI355X both forms are bound by VALU issue (16 cycles of a SIMD per instruction
// of the 16-wave workgroup) and by the wait for the pair's records, not by HBM bandwidth: the hot loops are
// written branch-free and staged (all of a thread's independent LDS operations are issued before the first
// result is consumed).
//
// Bit-exactness notes (vs the DLL): fp32 multiply then floor for unshifted axes; widen the fp32
// product to fp64, add 0.5, floor for shifted axes (DLL@0x180047bc0) -- both read off floor(2 * fl32(20 n));
// fp64 div -> sqrt -> mul -> '>' for the threshold (DLL@0x180049171), decided by an exact squared form
// unless it is a near-tie; arg-max keeps the LOWEST right cell among maxima; hypotheses are compared
// scale-outer / rotation-inner with strict '>' (DLL@0x180047dc0). Built with -ffp-contract=off and
// HIP's default correctly rounded fp32 divide.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernel_dense.h"

namespace gms {

// ------------------------------------------------------------------------------------------------
// normalizePoints (DLL@0x180048420): one thread per keypoint; frame found by binary search.
// A -0.0 result is stored as +0.0 (adding +0.0f): every later use is floor(n * W), which is 0 for
// both, and it lets the filter test "finite, non-negative" on the bit pattern alone.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void keypoint_codes(float2 n, uint16_t& lcode, uint16_t& rcode, uint32_t& scode)
{
    const bool bad = max(__float_as_uint(n.x), __float_as_uint(n.y)) >= 0x49800000u;
    const float x = bad ? 0.0f : n.x, y = bad ? 0.0f : n.y;
    const float fx = 20.0f * x, fy = 20.0f * y;                                  // mulss, rounded to fp32 (DLL@0x180047bc0)
    const uint32_t hx = (uint32_t)(int)(fx + fx), hy = (uint32_t)(int)(fy + fy);  // floor(2 f): carries all four grid types
    const uint32_t q = (hx & 1u) + 20u * (hy & 1u);
    const uint32_t edge = (hx == 39u ? 1u << 5 : 0u) | (hy == 39u ? 1u << 6 : 0u);
    const uint32_t l1 = (hy >> 1) * (uint32_t)kLeftW + (hx >> 1);
    const bool never = max(hx, hy) >= 40u;
    lcode = (uint16_t)(bad ? kLCellBad << kLCellShift : (never ? kLCellNever << kLCellShift : (q | edge | (l1 << kLCellShift))));
    const uint32_t r0x = (uint32_t)(int)fx, r0y = (uint32_t)(int)fy;              // getGridIndexRight, 20 x 20 (DLL@0x180047d60)
    const uint32_t e0 = (r0x < 20u && r0y < 20u) ? 403u - (r0y * 20u + r0x) : 0u;
    rcode = (uint16_t)(e0 | (bad ? kRCodeBad : 0u));
    const uint32_t r3x = (uint32_t)(int)(28.0f * x), r3y = (uint32_t)(int)(28.0f * y);
    const uint32_t odd40 = ((uint32_t)(int)(40.0f * x) & 1u) | (((uint32_t)(int)(40.0f * y) & 1u) << 1);
    const bool in_grids = r0x < 20u && r0y < 20u && r3x < 28u && r3y < 28u;
    scode = (bad || !in_grids) ? kSCodeBad : ((r0y * 20u + r0x) | ((r3y * 28u + r3x) << 9) | (odd40 << 19));
}

__global__ void __launch_bounds__(256)
normalize_kernel(const char* __restrict__ kp, int kp_stride, const int64_t* __restrict__ frame_off,
                 const int32_t* __restrict__ wh, int n_frames, int64_t total, float2* __restrict__ pts, uint64_t stamp)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the table's header (gms_kernels.h): the kernels read the keypoint count from here
        uint32_t* h = reinterpret_cast<uint32_t*>(pts) - kTableHeaderBytes / 4;
        h[0] = kTableMagic0;
        h[1] = kTableMagic1;
        *reinterpret_cast<int64_t*>(h + 2) = total;
        // the stamp of the side records that go with this build, in the spare bytes behind the code arrays: 0 = none, until
        // table_stamp_kernel has worked it out from the finished table
        uint64_t* tail = reinterpret_cast<uint64_t*>(pts + 2 * total);
        tail[0] = stamp;
        tail[1] = 0;
    }
    uint16_t* __restrict__ lcode = reinterpret_cast<uint16_t*>(pts + total);
    uint16_t* __restrict__ rcode = lcode + total;
    uint32_t* __restrict__ scode = reinterpret_cast<uint32_t*>(rcode + total);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        int lo = 0, hi = n_frames - 1;  // last frame f with frame_off[f] <= i
        while (lo < hi) {
            int mid = (lo + hi + 1) >> 1;
            if (frame_off[mid] <= i) lo = mid; else hi = mid - 1;
        }
        float w = (float)wh[2 * lo], h = (float)wh[2 * lo + 1];
        const float* p = reinterpret_cast<const float*>(kp + i * kp_stride);  // pt.x at +0, pt.y at +4 (DLL@0x1800485d4)
        float2 o;
        o.x = p[0] / w + 0.0f;  // IEEE fp32 divide (divss)
        o.y = p[1] / h + 0.0f;
        pts[i] = o;
        uint16_t lc, rc;
        uint32_t sc;
        keypoint_codes(o, lc, rc, sc);
        lcode[i] = lc;
        rcode[i] = rc;
        scode[i] = sc;
    }
}

// The side record of one frame (gms_kernels.h), one workgroup per frame behind normalize_kernel: the half-cell histogram of the
// frame's keypoints as LEFT points -- counted the way dense_pair_plain counts a pair's matches, a returning LDS atomic per
// keypoint whose result catches a byte passing 255 -- and whether some keypoint lies outside the parity domain. What a pair
// whose match k has queryIdx k for every keypoint of frame A would build for itself, once instead of once per pair.
__device__ __forceinline__ uint64_t mix64(uint64_t x)  // (splitmix64's finaliser)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void __launch_bounds__(1024)
side_records_kernel(const int64_t* __restrict__ frame_off, int64_t total, const float2* __restrict__ pts, uint64_t stamp,
                    SideRecord* __restrict__ side)
{
    __shared__ uint32_t s_hist[kLeftN];
    __shared__ uint32_t s_flags;
    __shared__ unsigned long long s_sum;
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x;
    if (tid < kLeftN) s_hist[tid] = 0;
    if (tid == 0) s_flags = 0;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    const int64_t off = frame_off[f], end = frame_off[f + 1];
    const bool inside = off >= 0 && end >= off && end <= total && end - off <= (int64_t)0x7FFFFFFF;
    const int n = inside ? (int)(end - off) : 0;
    const uint16_t* __restrict__ lcode = reinterpret_cast<const uint16_t*>(pts + total) + (inside ? off : 0);
    uint32_t flags = 0;
    uint64_t sum = 0;  // of a 64-bit mix of every (position, left code) of the frame: whatever the order of the additions
    for (int i = tid; i < n; i += 1024) {
        const uint32_t c = lcode[i];
        sum += mix64(((uint64_t)(uint32_t)i << 16) | c);
        const uint32_t cell = c >> kLCellShift;
        if (cell == kLCellBad) flags |= kSideBadLeft;
        if (cell < (uint32_t)kLeftN) {  // (a cell below kLCellNever is a cell of the grid: keypoint_codes writes no other)
            const uint32_t sh = ((c & 1u) << 3) | ((c & 4u) << 2);
            const uint32_t old = atomicAdd(&s_hist[cell], 1u << sh);
            if (((old >> sh) & 255u) == 255u) flags |= kSideSpill;
        }
    }
    if (flags) atomicOr(&s_flags, flags);
    if (sum) atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();
    SideRecord* __restrict__ r = side + f;
    if (tid < kLeftN) r->hist[tid] = s_hist[tid];
    if (tid == 0) {
        r->off = off;
        r->n = inside ? n : -1;  // (a frame outside the table equals no pair's frame A)
        r->flags = s_flags;
        r->stamp = stamp != 0 ? (uint64_t)s_sum : 0;  // the frame's share; table_stamp_kernel replaces it by the table's stamp
        r->pad[0] = r->pad[1] = 0;
    }
}

// The stamp that ties a table to its side records is a 64-bit digest of what the records were built from -- every frame's left codes,
// first keypoint and count, and the table's keypoint count --, written behind the table's code arrays and into every record: equal
// tables carry equal bytes whichever context built them and when, and a table rebuilt from other keypoints, at the same address or
// not, no longer matches records of the build before (two different tables share a stamp with probability 2^-64). One workgroup.
__global__ void __launch_bounds__(1024)
table_stamp_kernel(SideRecord* __restrict__ side, int n_frames, int64_t total, float2* __restrict__ pts)
{
    __shared__ unsigned long long s_sum;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    uint64_t sum = 0;
    for (int f = tid; f < n_frames; f += 1024) {
        const SideRecord& r = side[f];
        sum += mix64(r.stamp ^ mix64(((uint64_t)(uint32_t)f << 32) ^ (uint64_t)r.off) ^ mix64(0x5157ull + (uint64_t)(uint32_t)r.n));
    }
    if (sum) atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();  // (every frame's share has been read: the field is written below)
    const uint64_t stamp = mix64((uint64_t)s_sum ^ (uint64_t)total) | 1ull;  // never 0
    for (int f = tid; f < n_frames; f += 1024) side[f].stamp = stamp;
    if (tid == 0) *reinterpret_cast<uint64_t*>(pts + 2 * total) = stamp;
}

// Are a batch's matches in spatial order? One small workgroup, launched now and then behind a byte-matrix launch (gms_capi.cpp):
// sixteen waves look at 64 consecutive matches in the middle of sixteen pairs spread over the batch and count neighbours in the list
// whose left points share the cell of grid type 1 (random order: 1 in 400; a row-scanning detector or a per-pixel grid: most of them).
// More than a quarter -> *flag = 1 (a word in pinned host memory the host reads, without waiting, when it picks the DEALT
// instantiation for later launches). Speed only: either mapping gives the same result.
// The same samples answer a second question: are these identity-query pairs -- match k of the list is query k, and the list has one
// match per keypoint of frame A (what a brute-force matcher without cross-check returns)? All of the sampled pairs -> *ident_flag = 1:
// later launches take the IDENT instantiation, which checks every pair completely itself.
__global__ void __launch_bounds__(1024)
order_probe_kernel(FilterParams p, uint32_t* __restrict__ flag, uint32_t* __restrict__ ident_flag)
{
    __shared__ uint32_t s_same, s_seen, s_not_ident;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_same = s_seen = s_not_ident = 0;
    __syncthreads();
    const int pi = (int)(((long long)wave * p.n_pairs) >> 4);
    const gms_pair pr = p.pairs[pi];
    if (pr.m >= 128 && pr.frame_a >= 0 && pr.frame_a < p.n_frames) {
        const int64_t offA = p.frame_off[pr.frame_a];
        const int nA = (int)(p.frame_off[pr.frame_a + 1] - offA);
        const int64_t total_kp = table_total_kp(p);
        const bool table_ok = total_kp >= 0 && nA > 0 && offA + nA <= total_kp;
        const uint16_t* __restrict__ lcode = reinterpret_cast<const uint16_t*>(p.pts + (table_ok ? total_kp : 0)) + offA;
        const int start = (pr.m >> 1) & ~63;
        const uint32_t q = (uint32_t)p.matches[pr.match_off + start + lane].queryIdx;
        const uint32_t lc = table_ok ? (uint32_t)lcode[min(q, (uint32_t)(nA - 1))] >> kLCellShift : kLCellNever;
        const uint32_t cell = lc >= kLCellNever ? 0x10000u + (uint32_t)lane : lc;  // never binned: equals nobody
        const uint32_t next = (uint32_t)__shfl_down((int)cell, 1);
        const unsigned long long same = __ballot(lane < 63 && cell == next);
        const unsigned long long moved = __ballot(q != (uint32_t)(start + lane));
        if (lane == 0) {
            atomicAdd(&s_same, (uint32_t)__popcll(same));
            atomicAdd(&s_seen, 63u);
            if (moved != 0ull || pr.m != nA) atomicAdd(&s_not_ident, 1u);
        }
    }
    __syncthreads();
    if (tid == 0 && s_seen != 0) {
        *flag = 4u * s_same > s_seen ? 1u : 0u;
        *ident_flag = s_not_ident == 0u ? 1u : 0u;
    }
}

// ------------------------------------------------------------------------------------------------
// launch helpers (called from gms_capi.cpp through gms_kernels.h)
// ------------------------------------------------------------------------------------------------
size_t filter_lds_bytes(int kpt, uint32_t table_slots)
{
    const size_t mcap = (size_t)kpt * kThreads;
    size_t dwords = table_slots + 5 * 1664 + 8 * kLeftN + (mcap >> 5) + (mcap >> 6) + 1 + 48 + 4 + 132 + 12;
    return dwords * 4;
}

int filter_region_shift(int kpt) { return kpt <= 10 ? 0 : 2; }  // ~2 slots per match while the LDS allows it

uint32_t filter_table_slots(int kpt)
{
    // sum over cells of 4 * (region_buckets(n) + 1 header) <= M + (M >> sh) + 3 * 400 + 4 * 400
    const uint32_t mcap = (uint32_t)kpt * kThreads;
    return (mcap + (mcap >> filter_region_shift(kpt)) + 7 * kLeftN + 3u) & ~3u;
}

int filter_pick_kpt(int max_m)
{
    static const int kKpt[] = {4, 10, 16};
    for (int k : kKpt)
        if (max_m <= k * kThreads && filter_lds_bytes(k, filter_table_slots(k)) <= kLdsBytes) return k;
    return 0;
}

// ---- pair-table validation (every sixteenth launch of a context, gms_capi.cpp) ----------------------------------------------
// The pairs of a batch own disjoint ranges [match_off, match_off + m) of the match / output arrays (include/gms.h): a pair's
// survivors are written over the head of its own range, so overlapping ranges would let one pair overwrite what another still
// reads. Tables are almost always laid out in order, so: one pass tests "every range ends before the next one starts"; only when
// that fails a second kernel compares every pair with every other (tiles of 256 through LDS; 67 M comparisons for 8192 pairs)
// and marks both partners of every overlap GMS_ERR_BAD_ARG in the results, behind the filter that wrote them. Empty ranges
// overlap nothing.
__global__ void __launch_bounds__(256)
pairs_in_order_kernel(const gms_pair* __restrict__ pairs, int n_pairs, uint32_t* __restrict__ flag)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    bool bad = false;
    if (i + 1 < n_pairs) {
        const gms_pair a = pairs[i], b = pairs[i + 1];
        bad = a.match_off + (int64_t)max(a.m, 0) > b.match_off;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(256)
pairs_overlap_kernel(const gms_pair* __restrict__ pairs, int n_pairs, const uint32_t* __restrict__ flag,
                     gms_pair_result* __restrict__ results)
{
    if (*flag == 0u) return;  // the table is in order: nothing overlaps
    __shared__ int64_t s_lo[256], s_hi[256];
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    int64_t lo = 0, hi = 0;  // an empty range
    if (i < n_pairs) {
        const gms_pair a = pairs[i];
        lo = a.match_off;
        hi = a.match_off + (int64_t)max(a.m, 0);
    }
    bool clash = false;
    for (int base = 0; base < n_pairs; base += 256) {
        const int j = base + (int)threadIdx.x;
        int64_t l = 0, h = 0;
        if (j < n_pairs) {
            const gms_pair b = pairs[j];
            l = b.match_off;
            h = b.match_off + (int64_t)max(b.m, 0);
        }
        __syncthreads();
        s_lo[threadIdx.x] = l;
        s_hi[threadIdx.x] = h;
        __syncthreads();
        const int n_tile = min(256, n_pairs - base);
        for (int t = 0; t < n_tile; ++t) {
            const int64_t tl = s_lo[t], th = s_hi[t];
            clash |= (base + t != i) & (tl < hi) & (lo < th) & (tl < th) & (lo < hi);
        }
    }
    if (i < n_pairs && clash) results[i].status = GMS_ERR_BAD_ARG;
}

hipError_t launch_check_pairs(const gms_pair* d_pairs, int n_pairs, gms_pair_result* d_results, uint32_t* d_flag, hipStream_t stream)
{
    if (n_pairs < 2) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_flag, 0, 4, stream);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)((n_pairs + 255) / 256);
    hipLaunchKernelGGL(pairs_in_order_kernel, dim3(blocks), dim3(256), 0, stream, d_pairs, n_pairs, d_flag);
    hipLaunchKernelGGL(pairs_overlap_kernel, dim3(blocks), dim3(256), 0, stream, d_pairs, n_pairs, d_flag, d_results);
    return hipGetLastError();
}

// ---- gms_filter_host_batch: the survivors of a chunk packed back to back (what travels to the host is K records, not m slots).
// One workgroup per pair: its offset is the sum of the pairs' counts in front of it (a chunk has at most 8192 pairs: every
// workgroup adds them up itself), its K records are copied 16 bytes per lane; the last workgroup leaves the chunk's total.
__global__ void __launch_bounds__(256)
compact_survivors_kernel(const gms_pair* __restrict__ pairs, const gms_pair_result* __restrict__ results, int n_pairs,
                         const gms_dmatch* __restrict__ out, gms_dmatch* __restrict__ packed, int64_t* __restrict__ total)
{
    __shared__ unsigned long long s_part[4];
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    unsigned long long sum = 0;
    for (int j = tid; j < i; j += 256) {
        const gms_pair_result r = results[j];
        sum += (r.status == GMS_OK && r.n_inliers > 0) ? (unsigned long long)r.n_inliers : 0ull;
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
    if ((tid & 63) == 0) s_part[tid >> 6] = sum;
    __syncthreads();
    const unsigned long long off = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    const gms_pair_result r = results[i];
    const int k = (r.status == GMS_OK && r.n_inliers > 0) ? r.n_inliers : 0;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(out + pairs[i].match_off);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(packed + off);
    for (int j = tid; j < k; j += 256) dst[j] = src[j];
    if (i == n_pairs - 1 && tid == 0) *total = (int64_t)(off + (unsigned long long)k);
}

hipError_t launch_compact_survivors(const gms_pair* d_pairs, const gms_pair_result* d_results, int n_pairs, const gms_dmatch* d_out,
                                    gms_dmatch* d_packed, int64_t* d_total, hipStream_t stream)
{
    if (n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(compact_survivors_kernel, dim3((unsigned)n_pairs), dim3(256), 0, stream, d_pairs, d_results, n_pairs, d_out, d_packed, d_total);
    return hipGetLastError();
}

// Scale probes of the launches so far, per scale hypothesis s: stats[2 s] probed and evaluated anyway, stats[2 s + 1] probed and
// skipped; the same for the four-bit first attempts of scales 3 and 4 at stats[10 + 2 (s - 3)]. A probe costs about 45 % of a scale
// and saves the rest when it lets the scale skip: it pays from a skip rate of one half (a four-bit attempt costs half a byte probe
// and saves a whole one: the same rule is on the safe side). *flag: bit s = probe scale s, bit 8 + s = try four-bit entries first;
// a scale that was not probed often enough since the last verdict keeps its bit.
__global__ void probe_verdict_kernel(uint32_t* stats, uint32_t* flag)
{
    uint32_t mask = *flag;
    for (int s = 0; s < 5; ++s) {
        const uint32_t kept = stats[2 * s], skipped = stats[2 * s + 1];
        if (kept + skipped >= 8u) mask = (mask & ~(1u << s)) | (skipped >= kept ? 1u << s : 0u);
        stats[2 * s] = stats[2 * s + 1] = 0u;
    }
    for (int s = 3; s < 5; ++s) {
        const uint32_t kept = stats[4 + 2 * s], skipped = stats[5 + 2 * s];
        if (kept + skipped >= 8u) mask = (mask & ~(1u << (8 + s))) | (skipped >= kept ? 1u << (8 + s) : 0u);
        stats[4 + 2 * s] = stats[5 + 2 * s] = 0u;
    }
    *flag = mask;
}

hipError_t launch_probe_verdict(uint32_t* stats, uint32_t* flag, hipStream_t stream)
{
    hipLaunchKernelGGL(probe_verdict_kernel, dim3(1), dim3(1), 0, stream, stats, flag);
    return hipGetLastError();
}

hipError_t launch_order_probe(const FilterParams& p, uint32_t* flag, uint32_t* ident_flag, hipStream_t stream)
{
    if (p.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(order_probe_kernel, dim3(1), dim3(1024), 0, stream, p, flag, ident_flag);
    return hipGetLastError();
}

hipError_t launch_normalize(const void* d_kp, int kp_stride_bytes, const int64_t* d_frame_off, const int32_t* d_wh,
                            int n_frames, int64_t total_kp, float* d_pts, SideRecord* d_side, uint64_t stamp, hipStream_t stream)
{
    if (total_kp <= 0) return hipSuccess;
    int64_t blocks = (total_kp + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    float2* pts = reinterpret_cast<float2*>(reinterpret_cast<char*>(d_pts) + kTableHeaderBytes);
    if (d_side == nullptr || n_frames <= 0) stamp = 0;
    hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const char*>(d_kp),
                       kp_stride_bytes, d_frame_off, d_wh, n_frames, total_kp, pts, (uint64_t)0);
    if (stamp != 0) {
        hipLaunchKernelGGL(side_records_kernel, dim3((unsigned)n_frames), dim3(1024), 0, stream, d_frame_off, total_kp, pts, stamp, d_side);
        hipLaunchKernelGGL(table_stamp_kernel, dim3(1), dim3(1024), 0, stream, d_side, n_frames, total_kp, pts);
    }
    return hipGetLastError();
}

// Once per context (device), before the first launch: every per-pair kernel may ask for the CU's whole LDS. Done up front so
// that a launch is nothing but a launch (stream capture of gms_filter_device sees no attribute call).
hipError_t init_filter_kernels()
{
    hipError_t e = init_hash_kernels();
    if (e == hipSuccess) e = init_dense_kernels();
    if (e == hipSuccess) e = init_scales_kernels();
    return e;
}

// kpt = matches per thread of the 1024-thread workgroup (filter_pick_kpt).
// p.dense selects the kernel that tries the byte-matrix path first (only meaningful without scale hypotheses).
hipError_t launch_filter(const FilterParams& p, int kpt, int n_pairs, hipStream_t stream)
{
    if (n_pairs <= 0) return hipSuccess;
    const size_t lds = filter_lds_bytes(kpt, p.table_slots);
    return p.dense ? launch_filter_dense(p, kpt, n_pairs, lds, stream) : launch_filter_hash(p, kpt, n_pairs, lds, stream);
}

}  // namespace gms

