// capi_checks_check.cpp -- CPU check of the argument checks the host ABI sources share (sfm-gms_amd/csrc/capi_checks.h).
// tests/test_capi_checks.py builds it with g++ (plain and under the address / undefined-behaviour sanitizers) and runs it.
//
// Every case is an edge that the written-out copies of these checks handled in the entry points: frame offsets that decrease, start
// below zero or stay equal; match ranges with a negative length or start and ranges that end at and one past 2^40; a frame index equal
// to the number of frames with and without the frame bound; workspaces 0, 255 and 256 bytes past an aligned address, of size 0 and
// one byte short; byte ranges that abut and that share one byte; the registration's arrays given in part.
//
//   capi_checks_check      exit 0: every case holds; 1: one did not (it is printed)
#include <cstdint>
#include <cstdio>

#include "capi_checks.h"

static int bad = 0;
static void expect(bool cond, const char* what)
{
    if (cond) return;
    ++bad;
    std::printf("does not hold: %s\n", what);
}
#define EXPECT(cond) expect((cond), #cond)

static gms_pair pair_of(int a, int b, int m, int64_t match_off)
{
    gms_pair p = {};
    p.frame_a = a;
    p.frame_b = b;
    p.m = m;
    p.match_off = match_off;
    return p;
}

int main()
{
    const int64_t two40 = (int64_t)1 << 40;
    {   // frame offsets
        const int64_t up[4] = {0, 5, 5, 9}, down[4] = {0, 5, 4, 9}, neg[3] = {-1, 0, 3}, flat[2] = {7, 7}, last_down[3] = {0, 2, 1};
        EXPECT(frame_offsets_ok(up, 3) && frame_offsets_ascend(up, 3));
        EXPECT(!frame_offsets_ok(down, 3) && !frame_offsets_ascend(down, 3));
        EXPECT(frame_offsets_ok(down, 1));                                     // only n_frames + 1 offsets are looked at
        EXPECT(!frame_offsets_ok(neg, 2) && frame_offsets_ascend(neg, 2));     // a negative first offset: the host batches let it pass
        EXPECT(frame_offsets_ok(flat, 1) && frame_offsets_ascend(flat, 1));    // an empty frame
        EXPECT(!frame_offsets_ok(last_down, 2));
        EXPECT(frame_offsets_ok(neg, 0) && frame_offsets_ascend(neg, 0));      // no frame: nothing is read
    }
    {   // one pair's match range
        EXPECT(sfm_match_range_ok(pair_of(0, 1, 0, 0)));
        EXPECT(!sfm_match_range_ok(pair_of(0, 1, -1, 0)));
        EXPECT(!sfm_match_range_ok(pair_of(0, 1, 3, -1)));
        EXPECT(sfm_match_range_ok(pair_of(0, 1, 7, two40 - 7)));
        EXPECT(!sfm_match_range_ok(pair_of(0, 1, 7, two40 - 6)));
        EXPECT(!sfm_match_range_ok(pair_of(0, 1, INT32_MAX, INT64_MAX)));      // match_off + m is never formed
        EXPECT(sfm_match_range_ok(pair_of(0, 1, INT32_MAX, two40 - INT32_MAX)));
    }
    {   // the walk over a pair table
        const gms_pair tab[3] = {pair_of(0, 1, 4, 10), pair_of(1, 2, 9, 0), pair_of(2, 0, 0, 40)};
        PairRanges r = pair_ranges(tab, 3, 3, true);
        EXPECT(r.ok && r.total_m == 40 && r.max_m == 9);
        r = pair_ranges(tab, 3, 3, false);
        EXPECT(r.ok && r.total_m == 40 && r.max_m == 9);
        r = pair_ranges(tab, 0, 3, true);
        EXPECT(r.ok && r.total_m == 0 && r.max_m == 0);
        r = pair_ranges(nullptr, 0, 1, false);
        EXPECT(r.ok && r.total_m == 0 && r.max_m == 0);
        const gms_pair neg_m[2] = {pair_of(0, 1, 4, 0), pair_of(0, 1, -1, 4)};
        EXPECT(!pair_ranges(neg_m, 2, 2, false).ok && pair_ranges(neg_m, 1, 2, false).ok);
        const gms_pair neg_off[1] = {pair_of(0, 1, 4, -1)};
        EXPECT(!pair_ranges(neg_off, 1, 2, false).ok);
        const gms_pair at_end[1] = {pair_of(0, 1, 5, two40 - 5)}, past_end[1] = {pair_of(0, 1, 5, two40 - 4)};
        r = pair_ranges(at_end, 1, 2, false);
        EXPECT(r.ok && r.total_m == two40 && r.max_m == 5);
        EXPECT(!pair_ranges(past_end, 1, 2, false).ok);
        // frame_b == n_frames: refused only where the frames are bounded
        const gms_pair b_out[1] = {pair_of(0, 2, 1, 0)}, a_out[1] = {pair_of(2, 0, 1, 0)}, a_neg[1] = {pair_of(-1, 0, 1, 0)};
        EXPECT(!pair_ranges(b_out, 1, 2, true).ok && pair_ranges(b_out, 1, 2, false).ok);
        EXPECT(pair_ranges(b_out, 1, 3, true).ok);
        EXPECT(!pair_ranges(a_out, 1, 2, true).ok && pair_ranges(a_out, 1, 2, false).ok);
        EXPECT(!pair_ranges(a_neg, 1, 2, true).ok && pair_ranges(a_neg, 1, 2, false).ok);
    }
    {   // alignment and the workspace
        alignas(256) static unsigned char block[1024];
        EXPECT(!misaligned(block, 256) && !misaligned(nullptr, 256) && !misaligned(nullptr, 8));
        EXPECT(misaligned(block + 4, 8) && !misaligned(block + 8, 8) && misaligned(block + 1, 2) && !misaligned(block + 2, 2));
        EXPECT(misaligned(block + 2, 4) && !misaligned(block + 4, 4) && misaligned(block + 8, 16) && !misaligned(block + 16, 16));
        EXPECT(ws_ok(block, 512, 512));
        EXPECT(!ws_ok(block + 255, 512, 512) && !ws_ok(block + 1, 512, 512) && !ws_ok(block + 128, 512, 512));
        EXPECT(ws_ok(block + 256, 512, 512));
        EXPECT(!ws_ok(block, 512, 0) && !ws_ok(block, 0, 0));                  // need == 0: the size function refused the arguments
        EXPECT(!ws_ok(block, 511, 512) && ws_ok(block, 513, 512));
    }
    {   // overlap
        static unsigned char bytes[64];
        EXPECT(!ranges_overlap(bytes, 16, bytes + 16, 16) && !ranges_overlap(bytes + 16, 16, bytes, 16));   // abutting
        EXPECT(ranges_overlap(bytes, 17, bytes + 16, 16) && ranges_overlap(bytes + 16, 16, bytes, 17));     // one byte shared
        EXPECT(ranges_overlap(bytes, 16, bytes, 16) && ranges_overlap(bytes, 64, bytes + 20, 1));
        EXPECT(!ranges_overlap(bytes, 8, bytes + 32, 40) && ranges_overlap(bytes + 32, 8, bytes, 33));      // spans of different lengths
    }
    {   // the registration's arrays: all three and a frame, or none
        const int x = 0;
        EXPECT(reg_group_ok(nullptr, nullptr, nullptr, 0) && reg_group_ok(nullptr, nullptr, nullptr, -3));
        EXPECT(reg_group_ok(&x, &x, &x, 1) && !reg_group_ok(&x, &x, &x, 0));
        EXPECT(!reg_group_ok(&x, nullptr, nullptr, 1) && !reg_group_ok(nullptr, &x, nullptr, 1) && !reg_group_ok(nullptr, nullptr, &x, 1));
        EXPECT(!reg_group_ok(&x, &x, nullptr, 1) && !reg_group_ok(nullptr, &x, &x, 1));
    }
    std::printf("capi_checks_check: %d bad\n", bad);
    return bad ? 1 : 0;
}
