// match_unique_core.h -- one-to-one matches per pair: the order key of a match, when a match is live, and the keep
// rule as a sequential statement. What the kernels (match_unique_kernels.hip), the C ABI (capi_sfm.cpp) and the host build
// (tests/cpp/match_unique_host.cpp) share; tests/match_unique_ref.py states the same in numpy. The library's own definition.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gms.h"
#include "sfm_register_core.h"

namespace mu {

constexpr uint64_t kEmpty = ~0ull;  // no key: a key's low word is a match index below 2^24

// ord(d) from the bit pattern alone (no floating-point compare: denormals order as they are stored): the pattern for finite d > 0,
// 0 for +0 and -0, 0xFFFFFFFF for anything else -- negative, infinite or no number. Positive floats order as their patterns.
SFR_HD uint32_t ord_bits(uint32_t u)
{
    if ((u << 1) == 0u) return 0u;
    if (u >= 0x7F800000u) return 0xFFFFFFFFu;  // the sign bit, or an exponent of all ones
    return u;
}
SFR_HD uint32_t float_bits(float d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(d);
#else
    uint32_t u;
    memcpy(&u, &d, 4);
    return u;
#endif
}
SFR_HD uint64_t key(float distance, int k) { return ((uint64_t)ord_bits(float_bits(distance)) << 32) | (uint32_t)k; }

// the matches of pair i that can be live: the registration's n_i with a two-view record, every slot without
SFR_HD int live_count(const gms_pair& pr, const gms_two_view* tv, int i) { return tv ? sfr::pair_count(pr, tv[i]) : pr.m; }

// match k of a fitting pair (fr: its ranges) is live: k < n, a non-zero mask byte (none: every byte counts as set), both indices inside
SFR_HD bool live(const gms_dmatch& m, int k, int n, const uint8_t* mask_of_pair, const sfr::PairRanges& fr)
{
    if (k >= n || (mask_of_pair && mask_of_pair[k] == 0)) return false;
    return (uint32_t)m.queryIdx < (uint64_t)fr.na && (uint32_t)m.trainIdx < (uint64_t)fr.nb;
}

// The statement, one pair after the other: keep [total_m] gets one byte per slot of every fitting pair's [match_off, match_off + m)
// (1: live, and the least key among the live matches of its pair that share its trainIdx, and among those that share its queryIdx);
// counts [n_pairs][2] = {live, kept}. Slots of no fitting pair are not written. Not a maximum matching: a match may lose on one side
// to a match that loses on the other, and then neither is kept.
inline void unique_sequential(const int64_t* frame_off, int n_frames, int64_t total_kp, const gms_pair* pairs, int n_pairs, int64_t total_m,
                              const gms_dmatch* matches, const uint8_t* mask, const gms_two_view* tv, uint8_t* keep, int32_t* counts)
{
    std::vector<uint64_t> best_q, best_t;
    for (int i = 0; i < n_pairs; i++) {
        counts[2 * i] = counts[2 * i + 1] = 0;
        sfr::PairRanges fr = {};
        if (!sfr::pair_fits(pairs[i], frame_off, n_frames, total_kp, total_m, &fr)) continue;
        const gms_pair& pr = pairs[i];
        const int n = live_count(pr, tv, i);
        const gms_dmatch* mm = matches + pr.match_off;
        const uint8_t* mk = mask ? mask + pr.match_off : nullptr;
        best_q.assign((size_t)fr.na, kEmpty);
        best_t.assign((size_t)fr.nb, kEmpty);
        for (int k = 0; k < pr.m; k++) {
            if (!live(mm[k], k, n, mk, fr)) continue;
            const uint64_t key_k = key(mm[k].distance, k);
            if (key_k < best_q[mm[k].queryIdx]) best_q[mm[k].queryIdx] = key_k;
            if (key_k < best_t[mm[k].trainIdx]) best_t[mm[k].trainIdx] = key_k;
        }
        for (int k = 0; k < pr.m; k++) {
            const bool lv = live(mm[k], k, n, mk, fr);
            const uint64_t key_k = lv ? key(mm[k].distance, k) : 0;
            const bool kept = lv && best_q[mm[k].queryIdx] == key_k && best_t[mm[k].trainIdx] == key_k;
            keep[pr.match_off + k] = kept ? 1 : 0;
            counts[2 * i] += lv ? 1 : 0;
            counts[2 * i + 1] += kept ? 1 : 0;
        }
    }
}

}  // namespace mu
