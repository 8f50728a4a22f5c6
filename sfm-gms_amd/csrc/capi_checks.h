// capi_checks.h -- the argument checks that several sections of the host ABI (gms_capi.cpp, capi_*.cpp) apply, each stated once.
//
// Plain arithmetic and no HIP header, so that a host compiler builds it alone: tests/cpp/capi_checks_check.cpp pins the edges.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gms.h"

// p is no multiple of a bytes. A null pointer is aligned: whether it may be null is each call's own rule.
inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

// A caller's device workspace: 256-byte aligned (ws_layout.h counts its offsets from there) and at least `need` bytes, the call's own
// *_ws_bytes for its arguments -- which is 0 where it refuses them.
inline bool ws_ok(const void* d_ws, size_t ws_bytes, size_t need) { return !misaligned(d_ws, 256) && need != 0 && ws_bytes >= need; }

// host frame offsets never decrease (the host batches; each looks at the ends itself) ...
inline bool frame_offsets_ascend(const int64_t* frame_off, int n_frames)
{
    for (int f = 0; f < n_frames; f++)
        if (frame_off[f + 1] < frame_off[f]) return false;
    return true;
}
// ... and none of them is negative (the host one-shots behind the registration)
inline bool frame_offsets_ok(const int64_t* frame_off, int n_frames)
{
    return (n_frames < 1 || frame_off[0] >= 0) && frame_offsets_ascend(frame_off, n_frames);
}

// a pair's match range as the host one-shots take it: m >= 0, match_off >= 0 and an end within the 2^40 that sfm_register_sizes_ok
// allows -- match_off is held against 2^40 - m, so that match_off + m is formed only where it fits
inline bool sfm_match_range_ok(const gms_pair& pr)
{
    return pr.m >= 0 && pr.match_off >= 0 && pr.match_off <= ((int64_t)1 << 40) - (int64_t)pr.m;
}

// One walk over a host pair table: ok when every pair's range passes sfm_match_range_ok and, where bound_frames asks for it, both of
// its frames lie in [0, n_frames). total_m = the largest end of a range, max_m = the longest range (both only where ok).
struct PairRanges {
    bool ok;
    int64_t total_m;
    int max_m;
};
inline PairRanges pair_ranges(const gms_pair* pairs, int n_pairs, int n_frames, bool bound_frames)
{
    PairRanges r = {false, 0, 0};
    for (int p = 0; p < n_pairs; p++) {
        const gms_pair& q = pairs[p];
        if (bound_frames && (q.frame_a < 0 || q.frame_a >= n_frames || q.frame_b < 0 || q.frame_b >= n_frames)) return r;
        if (!sfm_match_range_ok(q)) return r;
        if (q.match_off + (int64_t)q.m > r.total_m) r.total_m = q.match_off + (int64_t)q.m;
        if (q.m > r.max_m) r.max_m = q.m;
    }
    r.ok = true;
    return r;
}

// [a, a + a_span) and [b, b + b_span) share a byte: a destination may not overlap its source
inline bool ranges_overlap(const void* a, uintptr_t a_span, const void* b, uintptr_t b_span)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_span && b0 < a0 + a_span;
}

// the dense entry points take the registration's three arrays together or not at all, and with them at least one frame
inline bool reg_group_ok(const void* d_pairs, const void* d_reg, const void* d_views, int n_frames)
{
    const bool any_reg = d_pairs || d_reg || d_views, all_reg = d_pairs && d_reg && d_views;
    return any_reg == all_reg && (!all_reg || n_frames >= 1);
}
