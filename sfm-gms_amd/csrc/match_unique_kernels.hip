// match_unique_kernels.hip -- one-to-one matches per pair (the rule is match_unique_core.h, the workspace
// MatchUniqueLayout in ws_layout.h). Stream-ordered launches, nothing else:
//
//   mu_init_kernel   both tables empty, the counts 0
//   mu_min_kernel    pairs x chunks of 256 matches: a live match puts its key into the slot of its query keypoint and into the slot
//                    of its train keypoint (64-bit atomicMin). The tables are the pair's own -- 2 m slots each at 2 match_off, open
//                    addressing with linear probing --, so neither a frame that is frame_a of many pairs (a star) nor a frame that is
//                    frame_b of many, nor a pair of frames listed twice, shares a slot with another pair. A slot is claimed by a
//                    compare-and-swap on the empty pattern; after that it belongs to one keypoint for the rest of the call (the
//                    keypoint is read off the key's match), and only minima of that keypoint's keys go in. Which slot a keypoint
//                    gets depends on the order of arrival; the minimum it ends with does not.
//   mu_mark_kernel   pairs x chunks: keep = live and the key stands in both slots; one byte for every slot below m; the pair's live
//                    and kept counts by one integer add per wave
//
// Many matches on one keypoint (a repeated structure: hundreds of queries whose nearest neighbour is one train keypoint) all aim at one
// 8-byte word. A key that cannot lower the word is not sent: the slot is read first (a plain load; the word only ever falls, so a stale
// value costs one atomic that changes nothing and never drops one that would). An LDS stage was weighed for pairs that fit one
// workgroup and left out: with the read in front, the word takes the first arrivals and then only lower keys, and the tables of a
// 10 000-match pair (320 KB) do not fit LDS anyway.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "match_unique_core.h"

namespace gms {
namespace {

constexpr int kB = 256;

struct MuIn {
    const int64_t* frame_off;
    const gms_pair* pairs;
    const gms_dmatch* matches;
    const uint8_t* mask;      // null: every byte counts as set
    const gms_two_view* tv;   // null: n = m
    int64_t total_kp, total_m;
    int n_frames, n_pairs;
};

// What a kernel needs of pair i, with everything that indexes memory checked (sfr::pair_fits): a pair that does not fit has m = 0.
struct MuPair {
    sfr::PairRanges fr;
    int64_t off;
    int m, n;
};
__device__ __forceinline__ MuPair mu_pair(const MuIn& in, int i)
{
    MuPair p = {};
    const gms_pair pr = in.pairs[i];
    if (!sfr::pair_fits(pr, in.frame_off, in.n_frames, in.total_kp, in.total_m, &p.fr)) return MuPair{};
    p.off = pr.match_off;
    p.m = pr.m;
    p.n = mu::live_count(pr, in.tv, i);
    return p;
}
__device__ __forceinline__ bool mu_live(const MuIn& in, const MuPair& p, int k, gms_dmatch& m)
{
    if (k >= p.n) return false;  // (n <= m: the slot is the pair's)
    m = in.matches[p.off + k];
    return mu::live(m, k, p.n, in.mask ? in.mask + p.off : nullptr, p.fr);
}

__device__ __forceinline__ uint32_t mu_home(uint32_t idx, uint32_t slots)  // slots = 2 m < 2^25
{
    return (uint32_t)(((uint64_t)(idx * 0x9E3779B1u) * slots) >> 32);
}
// the keypoint a slot's key belongs to: read off the key's match. side 0: the query keypoint, 1: the train keypoint. A key whose match
// index is not the pair's (only where two pairs' match ranges overlap, which the interface rules out) names none: -1.
__device__ __forceinline__ int mu_owner(const MuIn& in, const MuPair& p, unsigned long long key, int side)
{
    const uint32_t k = (uint32_t)key;
    if (k >= (uint32_t)p.m) return -1;
    const gms_dmatch m = in.matches[p.off + k];
    return side ? m.trainIdx : m.queryIdx;
}

__device__ __forceinline__ void mu_insert(const MuIn& in, const MuPair& p, unsigned long long* __restrict__ table, int side, int idx,
                                          unsigned long long key)
{
    const uint32_t slots = 2u * (uint32_t)p.m;
    uint32_t h = mu_home((uint32_t)idx, slots);
    for (uint32_t step = 0; step < slots; ++step) {  // at most m keypoints in 2 m slots
        unsigned long long cur = table[h];
        if (cur == mu::kEmpty) {
            cur = atomicCAS(&table[h], mu::kEmpty, key);
            if (cur == mu::kEmpty) return;
        }
        if (mu_owner(in, p, cur, side) == idx) {
            if (key < cur) atomicMin(&table[h], key);
            return;
        }
        h = h + 1 == slots ? 0 : h + 1;
    }
}
__device__ __forceinline__ unsigned long long mu_lookup(const MuIn& in, const MuPair& p, const unsigned long long* __restrict__ table, int side,
                                                        int idx)
{
    const uint32_t slots = 2u * (uint32_t)p.m;
    uint32_t h = mu_home((uint32_t)idx, slots);
    for (uint32_t step = 0; step < slots; ++step) {
        const unsigned long long cur = table[h];
        if (cur == mu::kEmpty) break;
        if (mu_owner(in, p, cur, side) == idx) return cur;
        h = h + 1 == slots ? 0 : h + 1;
    }
    return mu::kEmpty;
}

__global__ void __launch_bounds__(kB)
mu_init_kernel(unsigned long long* __restrict__ by_query, unsigned long long* __restrict__ by_train, int64_t slots, int32_t* __restrict__ counts,
               int n_pairs)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g < slots) {
        by_query[g] = mu::kEmpty;
        by_train[g] = mu::kEmpty;
    }
    if (g < 2 * (int64_t)n_pairs) counts[g] = 0;
}

// grid: pairs x chunks of kB matches
__global__ void __launch_bounds__(kB)
mu_min_kernel(MuIn in, unsigned long long* __restrict__ by_query, unsigned long long* __restrict__ by_train)
{
    const MuPair p = mu_pair(in, (int)blockIdx.x);
    const int k = (int)(blockIdx.y * kB + threadIdx.x);
    gms_dmatch m;
    if (!mu_live(in, p, k, m)) return;
    const unsigned long long key = mu::key(m.distance, k);
    mu_insert(in, p, by_query + 2 * p.off, 0, m.queryIdx, key);
    mu_insert(in, p, by_train + 2 * p.off, 1, m.trainIdx, key);
}

__global__ void __launch_bounds__(kB)
mu_mark_kernel(MuIn in, const unsigned long long* __restrict__ by_query, const unsigned long long* __restrict__ by_train,
               uint8_t* __restrict__ keep, int32_t* __restrict__ counts)
{
    const int i = (int)blockIdx.x;
    const MuPair p = mu_pair(in, i);
    const int k = (int)(blockIdx.y * kB + threadIdx.x);
    if ((int)(blockIdx.y * kB) >= p.m) return;  // (uniform over the workgroup)
    gms_dmatch m;
    const bool live = mu_live(in, p, k, m);
    bool kept = false;
    if (live) {
        const unsigned long long key = mu::key(m.distance, k);
        kept = mu_lookup(in, p, by_train + 2 * p.off, 1, m.trainIdx) == key && mu_lookup(in, p, by_query + 2 * p.off, 0, m.queryIdx) == key;
    }
    if (k < p.m) keep[p.off + k] = kept ? 1 : 0;
    const unsigned long long bl = __ballot(live), bk = __ballot(kept);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicAdd(&counts[2 * i], (int)__popcll(bl));
        if (bk) atomicAdd(&counts[2 * i + 1], (int)__popcll(bk));
    }
}

}  // namespace

size_t match_unique_ws_bytes(int64_t total_m) { return match_unique_layout(total_m).total; }

hipError_t launch_match_unique(const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs, int max_m,
                               int64_t total_m, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_two_view* d_tv, void* d_ws,
                               uint8_t* d_keep, int32_t* d_counts, hipStream_t stream)
{
    const MatchUniqueLayout L = match_unique_layout(total_m);
    unsigned long long* by_query = ws_ptr<unsigned long long>(d_ws, L.by_query);
    unsigned long long* by_train = ws_ptr<unsigned long long>(d_ws, L.by_train);
    const MuIn in = {d_frame_off, d_pairs, d_filtered, d_mask, d_tv, total_kp, total_m, n_frames, n_pairs};
    const int64_t slots = 2 * total_m, init_n = slots > 2 * (int64_t)n_pairs ? slots : 2 * (int64_t)n_pairs;
    hipError_t e = hipSuccess;
#define MU_STAGE(...)                    \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        e = hipGetLastError();           \
        if (e != hipSuccess) return e;   \
    } while (0)
    if (init_n > 0)
        MU_STAGE(mu_init_kernel, dim3((uint32_t)((init_n + kB - 1) / kB)), dim3(kB), 0, stream, by_query, by_train, slots, d_counts, n_pairs);
    if (n_pairs > 0 && max_m > 0) {
        const dim3 per_match((uint32_t)n_pairs, (uint32_t)((max_m + kB - 1) / kB));
        MU_STAGE(mu_min_kernel, per_match, dim3(kB), 0, stream, in, by_query, by_train);
        MU_STAGE(mu_mark_kernel, per_match, dim3(kB), 0, stream, in, by_query, by_train, d_keep, d_counts);
    }
#undef MU_STAGE
    return hipSuccess;
}

}  // namespace gms
