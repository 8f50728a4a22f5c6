// bf_select_core.h -- the arithmetic of the reference's bruteForceMatch after the matcher (FeatureMatchUtil.cpp:20-31; DESIGN.md
// §4.5b): the cross-check merge rule, the ratio prune and the general-K prefix of MSVC's std::sort.
//
// Plain functions of their arguments, so that the SAME source is what bf_select_kernels.hip runs and what tests/cpp/bf_select_host.cpp
// compiles with g++ for the CPU tests. The sort's steps (insertion sort, partition, heap sort) are logos_core.h's, which
// tests/golden/refdll_logos.npz pins against the reference DLL's own std::sort instance with the same predicate shape (a.d < b.d on
// a float alone, as DMatch::operator<).
#pragma once
#include "logos_core.h"

namespace gms {
namespace bfsel {

using logos::f2u;
using logos::kIsortMax;

// One pending range (f, l, ideal) per partition level; ideal starts at n and goes (ideal >> 1) + (ideal >> 2) per level, so no
// chain of partitions is deeper than 57 levels for n < 2^24 before heap sort takes over.
constexpr int kSortStack = 64;
constexpr long kMaxRows = 1L << 22;  // the matcher's limit on a frame's rows

// Cross-check slot key: (float bits of d) << 32 | train row. Distances are non-negative, so their bits order as the values; a 64-bit
// minimum keeps the smallest distance and, among equal ones, the lowest train row -- what OpenCV's sequential loop keeps
// (`if (tdist[i] < dist[tidx[i]])`, i ascending).
constexpr uint64_t kEmptySlot = ~0ull;
GMS_HD uint64_t slot_key(float d, int32_t i) { return ((uint64_t)f2u(d) << 32) | (uint32_t)i; }
GMS_HD float slot_dist(uint64_t k) { return logos::u2f((uint32_t)(k >> 32)); }
GMS_HD int32_t slot_row(uint64_t k) { return (int32_t)(uint32_t)k; }

// The prune's keep test: `while (front.distance * kDistanceCoef < back.distance) pop_back` evaluates the product in double
// (float * double constant), so d survives iff !((double)d_min * coef < (double)d).
GMS_HD bool within_ratio(float d, float d_min, double coef) { return !((double)d_min * coef < (double)d); }

// The first k places of MSVC std::sort over the n records (d[i], ix[i]), ordered by d alone, for any k. Ranges that lie wholly at
// or beyond position k are never touched: elements do not cross a partition's boundaries, and the two sides of a partition are sorted
// with the same `ideal`, independently of each other, so the order in which they are worked on does not change the permutation.
// stk: room for 3 * kSortStack ints (LDS on the device, so that the kernel keeps no array in private memory).
GMS_HD void msvc_sort_prefix(float* d, int32_t* ix, long n, long k, int32_t* stk)
{
    int sp = 0;
    long f = 0, l = n, ideal = n;
    for (;;) {
        if (f < k) {
            if (l - f <= kIsortMax) {
                logos::sort_insertion(d, ix, f, l);
            } else if (ideal <= 0) {
                logos::sort_heap(d, ix, f, l);
            } else {
                long pf, pl;
                logos::sort_partition(d, ix, f, l, &pf, &pl);
                ideal = (ideal >> 1) + (ideal >> 2);
                if (pl < k && l - pl > 1) {  // the upper part reaches into [0, k): later, with this level's ideal
                    stk[3 * sp] = (int32_t)pl;
                    stk[3 * sp + 1] = (int32_t)l;
                    stk[3 * sp + 2] = (int32_t)ideal;
                    sp++;
                }
                l = pf;  // the lower part always starts below k
                continue;
            }
        }
        if (sp == 0) return;
        sp--;
        f = stk[3 * sp];
        l = stk[3 * sp + 1];
        ideal = stk[3 * sp + 2];
    }
}

}  // namespace bfsel
}  // namespace gms
