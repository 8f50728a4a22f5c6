// ws_layout.h -- the device workspaces the launchers work in: for each one, ONE list of its regions in order, which gives both the
// workspace's size (`total`) and the offset of every region. The size functions return the total; the launchers take every pointer
// they hand to a kernel, and every span they clear, from the same struct. Offsets count from the workspace's start, which is 256-byte
// aligned (the C ABI refuses other caller workspaces; the context's own come from hipMalloc).
//
// Plain arithmetic and no HIP header, so that a host compiler builds it alone: tests/cpp/ws_layout_check.cpp sweeps the layouts of
// the keypoint source (both forms of the pyramid's), the large pairs, StereoBM, portrait mode and bruteForceMatch's selection for order,
// overlap, alignment and size.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "calib_core.h"
#include "gms.h"
#include "portrait_core.h"

namespace gms {

constexpr int kLeftW = 20, kLeftH = 20, kLeftN = 400;  // DLL@0x180046ac6: fixed 20 x 20 left grid
constexpr int kFineW = 40, kFineN = 1600;                  // half-cell grid: carries all four grid types

constexpr size_t round_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }  // a: a power of two

template <typename T>
T* ws_ptr(void* ws, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(ws) + offset); }

// Hands out the consecutive regions of a workspace, in call order, and keeps count of the bytes that only round something up.
struct WsCursor {
    size_t end = 0, padding = 0;
    // the offset of a new region of `bytes` bytes whose length is rounded up to a multiple of `pad`
    size_t take(size_t bytes, size_t pad = 1)
    {
        const size_t at = end;
        end += round_up(bytes, pad);
        padding += round_up(bytes, pad) - bytes;
        return at;
    }
    // the next region starts on a multiple of `a`
    void align(size_t a)
    {
        padding += round_up(end, a) - end;
        end = round_up(end, a);
    }
};

// ---- the keypoint source (detect_kernels.hip) ---------------------------------------------------------------------------------------
struct DetectLayout {
    size_t score;  // uint8 [n][h][w]
    size_t cand;   // uint8 [n][h][w]
    size_t box;    // uint16 [n][h][w]: box sums
    size_t hist;   // uint32 [n][256]: score histogram
    size_t cut;    // int32 [n][4]. The single-scale call zeroes [hist, cut) first
    size_t rows;   // [n][h], 8 bytes each: row counts
    size_t list;   // [n][max_keypoints], 8 bytes each
    size_t total;
};
inline DetectLayout detect_layout(int w, int h, int n_images, int max_keypoints)
{
    const size_t n = (size_t)n_images, plane = (size_t)w * h;
    WsCursor c;
    return {c.take(plane * n, 256), c.take(plane * n, 256), c.take(plane * n * 2, 256), c.take(n * 256 * 4), c.take(n * 16),
            c.take(n * h * 8, 256), c.take(n * max_keypoints * 8, 256), c.end};
}

// The pyramid: level 0 is the image; w_l = (5 w_{l-1} + 3) / 6, the same for h; the levels end at n_levels or before the first one the
// detector refuses (width or height <= 32). Returns the number of levels (0: level 0 itself is refused).
constexpr int kPyramidMaxLevels = 16;
constexpr int kBorder = 16;  // the detector keeps this far from the image's edge
inline int pyramid_level_sizes(int w, int h, int n_levels, int* widths, int* heights)
{
    int n = 0;
    while (n < n_levels && n < kPyramidMaxLevels && w > 2 * kBorder && h > 2 * kBorder && w <= 65535 && h <= 65535) {
        widths[n] = w; heights[n] = h;
        ++n;
        w = (5 * w + 3) / 6; h = (5 * h + 3) / 6;
    }
    return n;
}
// bytes of levels 1 .. n - 1 of n_images images, level after level, the images of a level back to back, nothing between them
inline size_t pyramid_bytes(int w, int h, int n_images, int n_levels)
{
    int ww[kPyramidMaxLevels], hh[kPyramidMaxLevels];
    const int n = pyramid_level_sizes(w, h, n_levels, ww, hh);
    size_t b = 0;
    for (int l = 1; l < n; ++l) b += (size_t)ww[l] * hh[l] * (size_t)(n_images > 0 ? n_images : 0);
    return b;
}
// Every call zeroes [counts, detect) first (the counts too: a level with quota 0 is not run).
// `refined` (the DoG call with refinement; dog_kernels.hip, detect_kernels.hip) adds, behind the other regions, the plane of refinement
// codes that a level's candidate kernel leaves for its describe kernel. Never cleared: a code is read only where the level's candidate
// plane is non-zero, and the kernel that wrote that plane wrote the code. Not refined: `codes` is empty and `total` ends at `detect`'s end.
struct PyramidLayout {
    size_t levels;  // uint8: the level images 1 .., pyramid_bytes of them
    size_t counts;  // int32 [kPyramidMaxLevels][n]: keypoints per level and image
    size_t hists;   // uint32 [kPyramidMaxLevels][n][256]: the levels' score histograms
    size_t detect;  // the single-scale workspace of level 0: every level fits into it in its turn
    size_t codes;   // refined only: uint16 [n][h][w] of level 0, on a 256-byte boundary: every level fits into it in its turn
    size_t total;
};
inline PyramidLayout pyramid_layout(int w, int h, int n_images, int max_keypoints, int n_levels, bool refined)
{
    const size_t n = (size_t)n_images;
    WsCursor c;
    const size_t levels = c.take(pyramid_bytes(w, h, n_images, n_levels), 256), counts = c.take(kPyramidMaxLevels * n * 4, 256),
                 hists = c.take(kPyramidMaxLevels * n * 256 * 4), detect = c.take(detect_layout(w, h, n_images, max_keypoints).total);
    if (!refined) return {levels, counts, hists, detect, c.end, c.end};
    c.align(256);
    return {levels, counts, hists, detect, c.take((size_t)w * h * n * 2, 256), c.end};
}

// ---- large pairs, per slice of n pairs of the context's own workspace (gms_kernel_band.hip, gms_kernel_stream.hip) ------------------
// plan_workspace sizes a slice as n * bytes per pair: the regions of one pair, plus a slack that covers what the layout of n pairs
// rounds up (`padding`; every round-up here is to 16 bytes, so it adds less than 16).
constexpr size_t kAlignPadMax = 15;

// default flags: three-band lists
struct BandLayout {
    size_t lists;     // uint2 [n][3][mcap]
    size_t nfine;     // uint32 [n][1600]: half-cell histogram. Every launch zeroes [nfine, mask) first
    size_t list_len;  // uint32 [n][3]
    size_t flags;     // uint32 [n]
    size_t mask;      // uint8 [n][mcap], when the caller gives no mask
    size_t total, padding;
};
inline BandLayout band_layout(size_t n, size_t mcap, bool need_mask)
{
    WsCursor c;
    return {c.take(n * 3 * mcap * 8), c.take(n * kFineN * 4), c.take(n * 3 * 4), c.take(n * 4), c.take(need_mask ? n * mcap : 0), c.end, c.padding};
}
inline size_t band_bytes_per_pair(size_t mcap, bool need_mask) { return band_layout(1, mcap, need_mask).total; }  // (nothing is rounded)

// rotation / scale hypotheses: tiled lists; max_tiles = the most tiles of any scale's TileGeom
constexpr int kMaxTiles = 32;
struct TileLayout {
    size_t lists;     // uint2 [n][max_tiles][mcap]
    size_t nfine;     // uint32 [n][1600]. Every scale zeroes [nfine, flags) first: histogram, list lengths, counts
    size_t list_len;  // uint32 [n][kMaxTiles]
    size_t cnt;       // uint32 [n][8]: inliers per rotation
    size_t flags;     // uint32 [n]. Every launch zeroes [flags, state_end) first: the flags and both states
    size_t state;     // uint32 [2][n][4], the two used alternately
    size_t state_end;
    size_t rotmask;   // uint8 [n][mcap], on a 16-byte boundary: read 16 bytes at a time
    size_t bestmask;  // uint8 [n][mcap], when the caller gives no mask
    size_t total, padding;
};
inline TileLayout tile_layout(size_t n, size_t max_tiles, size_t mcap, bool need_mask)
{
    WsCursor c;
    const size_t lists = c.take(n * max_tiles * mcap * 8), nfine = c.take(n * kFineN * 4), list_len = c.take(n * kMaxTiles * 4), cnt = c.take(n * 8 * 4),
                 flags = c.take(n * 4), state = c.take(2 * n * 4 * 4), state_end = c.end;
    c.align(16);
    return {lists, nfine, list_len, cnt, flags, state, state_end, c.take(n * mcap), c.take(need_mask ? n * mcap : 0), c.end, c.padding};
}
constexpr size_t kTileSlack = 64;
static_assert(kTileSlack >= 1 * kAlignPadMax, "the slack covers the tile layout's one round-up");
inline size_t tile_bytes_per_pair(size_t max_tiles, size_t mcap, bool need_mask)
{
    const TileLayout one = tile_layout(1, max_tiles, mcap, need_mask);
    return one.total - one.padding + kTileSlack;
}

// pairs up to 65 536 matches, every flag combination: the streamed byte matrix
constexpr int kSRowWords = 192;  // per pair: [h] matches per bucket; [64 + h] fill cursors; [128 + h] first entry of bucket h
constexpr int kSTilesMax = 8;    // tiles of the marking / compacting kernels per pair
// Every launch zeroes [nfine, tile_cnt) first: the histograms, counters and flags start at zero (tables and tile counts need not:
// every word has one writer).
struct StreamLayout {
    size_t entries;   // uint2 [n][mcap], sorted by left row
    size_t codes;     // uint2 [n][mcap], the same words in the matches' original order
    size_t nfine;     // uint32 [n][1600]: half-cell histogram
    size_t row_cnt;   // uint32 [n][kSRowWords]
    size_t counts;    // uint32 [n][5][8]
    size_t flags;     // uint32 [n]
    size_t tile_cnt;  // uint32 [n][kSTilesMax][5][8]
    size_t tables;    // uint32 [n][scales][4][400]
    size_t nleft;     // uint16 [n][4][400]
    size_t total, padding;
};
inline StreamLayout stream_layout(size_t n, size_t mcap, size_t n_scales)
{
    WsCursor c;  // (the regions rounded to 16 keep every region of a slice 16-byte aligned)
    return {c.take(n * mcap * 8, 16), c.take(n * mcap * 8, 16), c.take(n * kFineN * 4), c.take(n * kSRowWords * 4), c.take(n * 5 * 8 * 4),
            c.take(n * 4, 16), c.take(n * kSTilesMax * 5 * 8 * 4), c.take(n * n_scales * 4 * kLeftN * 4, 16), c.take(n * 4 * kLeftN * 2), c.end,
            c.padding};
}
constexpr size_t kStreamSlack = 128;
static_assert(kStreamSlack >= 4 * kAlignPadMax, "the slack covers the stream layout's four round-ups");
inline size_t stream_bytes_per_pair(size_t mcap, size_t n_scales)
{
    const StreamLayout one = stream_layout(1, mcap, n_scales);
    return one.total - one.padding + kStreamSlack;
}

// the same size class without scale hypotheses: one workgroup per pair
struct StreamDenseLayout {
    size_t codes;  // uint32 [n][mcap]
    size_t nleft;  // uint16 [n][4][400]
    size_t flags;  // uint32 [n], zeroed by every launch
    size_t total, padding;
};
inline StreamDenseLayout stream_dense_layout(size_t n, size_t mcap)
{
    WsCursor c;
    return {c.take(n * mcap * 4, 16), c.take(n * 4 * kLeftN * 2, 16), c.take(n * 4), c.end, c.padding};
}
constexpr size_t kStreamDenseSlack = 64;
static_assert(kStreamDenseSlack >= 2 * kAlignPadMax, "the slack covers the dense stream layout's two round-ups");
inline size_t stream_dense_bytes_per_pair(size_t mcap)
{
    const StreamDenseLayout one = stream_dense_layout(1, mcap);
    return one.total - one.padding + kStreamDenseSlack;
}

// ---- StereoBM (stereo_bm_kernels.hip) -----------------------------------------------------------------------------------------------
struct StereoBmLayout {
    size_t pre;   // uint8 [n][2][H][W]: the pre-filtered images (left, right)
    size_t cost;  // int32 [n][H][W]: costs of the winner-take-all step
    size_t total;
};
inline StereoBmLayout stereo_bm_layout(int n, int W, int H)
{
    const size_t px = (size_t)n * (size_t)W * (size_t)H;
    WsCursor c;
    return {c.take(2 * px, 256), c.take(4 * px, 256), c.end};
}

// ---- semi-global matching (stereo_sgm_kernels.hip) ----------------------------------------------------------------------------------
// ny x wx: the region StereoBM computes (rows [w2, H - w2), wx output columns; 0 x 0 when it computes nothing). The volumes take
// 4 nd bytes per pixel of the region. total = 0: more than 2^50 pixels, so that no sum below can wrap.
struct StereoSgmLayout {
    StereoBmLayout bm;  // StereoBM's regions, unchanged: pre, and cost as the winner's S for the left-right check
    size_t tex;         // int32 [n][ny][wx]: StereoBM's texture sums
    size_t C;           // uint16 [n][ny][wx][nd]: the matching costs
    size_t S;           // uint16 [n][ny][wx][nd]: the sum of the path costs. The first direction's launch writes it, the others add
    size_t total;
};
inline StereoSgmLayout stereo_sgm_layout(int n, int W, int H, int ny, int wx, int nd)
{
    const StereoBmLayout B = stereo_bm_layout(n, W, H);
    const size_t px = (size_t)n * (size_t)ny * (size_t)wx;  // n <= 65535, ny <= H < 2^31, wx <= 8192: below 2^60, no wrap in 64 bits
    const bool fits = sizeof(size_t) >= 8 && px <= (SIZE_MAX >> 14) && B.total <= (SIZE_MAX >> 2);
    const size_t vol = fits ? 2 * (size_t)nd * px : 0;      // nd <= 512: at most 2^10 px < 2^60
    WsCursor c;
    c.take(B.total, 256);
    const size_t tex = c.take(4 * px, 256), C = c.take(vol, 256), S = c.take(vol, 256);
    return {B, tex, C, S, fits ? c.end : 0};
}

// ---- portrait mode (portrait_kernels.hip) -------------------------------------------------------------------------------------------
// Two pixels side by side are never both the root of a border, so a row holds at most (W + 1) / 2 of them. With equal values the two
// are one component. Otherwise one is a hole's first pixel: the pixel above it is set (a zero there would be an earlier pixel of the
// hole), and that pixel is 8-connected to the set pixel on either side of the hole's first pixel, so the set neighbour is not its
// component's first pixel. tests/test_portrait_ref.py checks the bound on random masks.
inline size_t pm_key_cap(int W, int H) { return (size_t)H * (size_t)((W + 1) / 2); }
constexpr int kChosenStride = 2 + pm::kMaxContours;
struct PortraitLayout {
    size_t mask, nb, flag, sel;  // uint8 [n][H][W] each: mask, neighbour codes, frame flags, selected
    size_t label;                // int32 [n][H][W]
    size_t tog;                  // uint64 [n][H][W]: toggles
    size_t keys;                 // uint64 [n][pm_key_cap]: the borders' rank keys
    size_t chosen;               // int32 [n][kChosenStride]: [0] chosen count, [1..64] chosen roots, [65] borders
    size_t total;
};
inline PortraitLayout portrait_layout(int n, int W, int H)
{
    const size_t px = (size_t)n * (size_t)W * (size_t)H;
    WsCursor c;
    return {c.take(px, 256), c.take(px, 256), c.take(px, 256), c.take(px, 256), c.take(4 * px, 256), c.take(8 * px, 256),
            c.take(8 * (size_t)n * pm_key_cap(W, H), 256), c.take((size_t)n * kChosenStride * 4, 256), c.end};
}

// ---- chessboard corner candidates (calib_kernels.hip) -------------------------------------------------------------------------------
// Every call zeroes n_list first.
struct ChessLayout {
    size_t R;       // uint32 [n][h][w]: the response
    size_t list;    // uint64 [n][calib::peak_capacity(w, h)]: the peaks' rank keys, in no fixed order
    size_t n_list;  // uint32 [n]: peaks per image
    size_t total;
};
inline ChessLayout chess_layout(int n, int w, int h)
{
    const size_t px = (size_t)n * (size_t)w * (size_t)h;
    WsCursor c;
    return {c.take(4 * px, 256), c.take(8 * (size_t)n * (size_t)calib::peak_capacity(w, h), 256), c.take(4 * (size_t)n, 256), c.end};
}

// ---- bruteForceMatch's selection (bf_select_kernels.hip) ----------------------------------------------------------------------------
struct BfSelectLayout {
    size_t pairs2;  // gms_pair [n_pairs]: the matcher's pair table
    size_t back;    // gms_dmatch [total_back]: the matcher's output
    size_t qt;      // uint64 [n_pairs][max_rows]: (q, t) / slots
    size_t cd;      // float [n_pairs][max_rows]: d
    size_t cix;     // int32 [n_pairs][max_rows]: ix
    size_t total;
};
inline BfSelectLayout bf_select_layout(int n_pairs, int64_t max_rows, int64_t total_back)
{
    const size_t rows = (size_t)n_pairs * (size_t)max_rows;
    WsCursor c;
    return {c.take(sizeof(gms_pair) * (size_t)n_pairs, 256), c.take(sizeof(gms_dmatch) * (size_t)total_back, 256), c.take(8 * rows, 256),
            c.take(4 * rows, 256), c.take(4 * rows, 256), c.end};
}

// ---- registering many views (sfm_register_kernels.hip) ------------------------------------------------------------------------------
// K global keypoints, M match slots, P pairs. Every call writes every word it later reads: nothing is carried from call to call.
constexpr int kSfrScanTile = 4096;  // keypoints per workgroup of the ordered compaction
inline size_t sfr_hash_slots(size_t total_kp)  // a power of two of at least 2 K: a probe always meets an empty slot
{
    size_t s = 64;
    while (s < 2 * total_kp) s <<= 1;
    return s;
}
struct SfmRegisterLayout {
    size_t rank;     // int32 [M]: non-zero mask bytes before the match, within its pair
    size_t rho;      // uint64 [M]: the pair's valid link ratios, as bit patterns, packed at its match_off
    size_t slot;     // int32 [K]: per keypoint of a registered frame, the lowest match of the registering pair that names it
    size_t parent;   // int32 [K]: union-find; after the flatten kernel the track id
    size_t member;   // int32 [K]: 1 when the keypoint is an end of an edge
    size_t obs;      // uint32 [K]: per root, its keypoints
    size_t est;      // uint32 [K]: per root, its estimates
    size_t multi;    // uint32 [K]: per root, 1 when two of its keypoints share a frame
    size_t repkey;  // uint64 [K]: per root, the least (pair << 32 | rank) of its estimates
    size_t spread;   // uint64 [K]: per root, the bit pattern of the largest distance
    size_t hash;     // uint64 [sfr_hash_slots(K)]: (root, frame) keys seen
    size_t tiles;    // int32 [ceil(K / kSfrScanTile) + 1]: roots per tile, then their exclusive prefix
    size_t npts;     // int32 [P]: non-zero mask bytes of the pair
    size_t ok;       // int32 [P]
    size_t total;
};
inline SfmRegisterLayout sfm_register_layout(int n_pairs, int64_t total_kp, int64_t total_matches)
{
    const size_t K = (size_t)total_kp, M = (size_t)total_matches, P = (size_t)n_pairs;
    WsCursor c;
    return {c.take(4 * M, 256), c.take(8 * M, 256), c.take(4 * K, 256), c.take(4 * K, 256), c.take(4 * K, 256), c.take(4 * K, 256),
            c.take(4 * K, 256), c.take(4 * K, 256), c.take(8 * K, 256), c.take(8 * K, 256),
            c.take(8 * sfr_hash_slots(K), 256), c.take(4 * ((K + kSfrScanTile - 1) / kSfrScanTile + 1), 256), c.take(4 * P, 256),
            c.take(4 * P, 256), c.end};
}

// ---- one-to-one matches per pair (match_unique_kernels.hip) --------------------------------------------------------------------------
// M match slots. A pair of m slots at match_off owns slots [2 match_off, 2 match_off + 2 m) of each table: open addressing over the
// keypoints its live matches name, at most m of them in 2 m slots, so a probe always meets an empty slot. A slot holds the least key
// (match_unique_core.h) of one keypoint; which keypoint, the key's match says. 32 bytes per match slot, whatever the frames' sizes
// and however often a frame appears in the pair list. Every call writes every word it later reads.
struct MatchUniqueLayout {
    size_t by_query;  // uint64 [2 M]
    size_t by_train;  // uint64 [2 M]
    size_t total;
};
inline MatchUniqueLayout match_unique_layout(int64_t total_matches)
{
    const size_t M = (size_t)total_matches;
    WsCursor c;
    return {c.take(16 * M, 256), c.take(16 * M, 256), c.take(0) + (M == 0 ? 256 : 0)};
}

// ---- bundle adjustment behind the registration (sfm_ba_kernels.hip) -----------------------------------------------------------------
// K global keypoints, C cloud entries, F frames. Everything an observation owns sits at its keypoint's index: a keypoint is an
// observation of at most one track, so no compaction is needed and the observations of a frame are a range. Every call writes every
// word it later reads.
constexpr int kSbaScanTile = 4096;  // cloud entries per workgroup of the prefix sum over the tracks' counts
struct SfmBaLayout {
    size_t kp_track;  // int32 [K]: the cloud entry the keypoint observes, -1: none
    size_t kp_frame;  // int32 [K]: its frame
    size_t list;      // int32 [K]: the tracks' keypoints, ascending within a track, track c at t_off[c]
    size_t uv;        // double [K][2]: the undistorted measurement
    size_t jc;        // double [K][12]: sqrt(w) Jc, zeros when inactive or the frame is not free
    size_t jp;        // double [K][6]: sqrt(w) Jp
    size_t res;       // double [K][2]: sqrt(w) r
    size_t t_cnt;     // int32 [C]: observations of the track
    size_t t_off;     // int32 [C]: their exclusive prefix
    size_t t_fill;    // int32 [C]: the fill cursor
    size_t t_used;    // int32 [C]: 1 when the track takes part
    size_t tiles;     // int32 [ceil(C / kSbaScanTile) + 1]
    size_t xc;        // double [C][3]: the candidate points
    size_t vinv;      // double [C][9]: (V + lambda diag V)^-1
    size_t gp;        // double [C][3]: -sum Jp^T r
    size_t qt;        // double [C][3]: the per-track pass of S p
    size_t cand;      // gms_sfm_view [F]: the candidate views
    size_t U;         // double [F][36]: damped
    size_t L;         // double [F][36]: the preconditioner's Cholesky factor
    size_t lok;       // int32 [F]: 1 when it has one
    size_t free_;     // int32 [F]: 1 when the frame is a parameter
    size_t vec;       // double [6][F][6]: b, x, r, z, p, q
    size_t part;      // double [F]: per-frame shares of a dot product
    size_t costp;     // double [F][2]: per-frame Huber cost and sum of squares
    size_t actp;      // int64 [F]: per-frame active observations
    size_t scal;      // double [16]
    size_t flags;     // int32 [16]
    size_t total;
};
inline SfmBaLayout sfm_ba_layout(int n_frames, int64_t total_kp, int64_t cloud_cap)
{
    const size_t K = (size_t)total_kp, Cc = (size_t)cloud_cap, F = (size_t)n_frames;
    WsCursor c;
    return {c.take(4 * K, 256), c.take(4 * K, 256), c.take(4 * K, 256), c.take(16 * K, 256), c.take(96 * K, 256), c.take(48 * K, 256),
            c.take(16 * K, 256), c.take(4 * Cc, 256), c.take(4 * Cc, 256), c.take(4 * Cc, 256), c.take(4 * Cc, 256),
            c.take(4 * ((Cc + kSbaScanTile - 1) / kSbaScanTile + 1), 256), c.take(24 * Cc, 256), c.take(72 * Cc, 256), c.take(24 * Cc, 256),
            c.take(24 * Cc, 256), c.take(sizeof(gms_sfm_view) * F, 256), c.take(288 * F, 256), c.take(288 * F, 256), c.take(4 * F, 256),
            c.take(4 * F, 256), c.take(288 * F, 256), c.take(8 * F, 256), c.take(16 * F, 256), c.take(8 * F, 256), c.take(128, 256),
            c.take(64, 256), c.end};
}

// ---- the points of disparity maps (rectify_kernels.hip) -----------------------------------------------------------------------------
// Every call writes every word it later reads.
constexpr int kDenseScanBlock = 1024;  // pixels per workgroup of the ordered compaction
inline int dense_cloud_blocks(int W, int H) { return (int)(((size_t)W * (size_t)H + kDenseScanBlock - 1) / kDenseScanBlock); }
struct DenseCloudLayout {
    size_t blocks;  // int32 [n][dense_cloud_blocks]: points per block, then in place their exclusive prefix within the pair
    size_t total;
};
inline DenseCloudLayout dense_cloud_layout(int n, int W, int H)
{
    WsCursor c;
    return {c.take(4 * (size_t)n * (size_t)dense_cloud_blocks(W, H), 256), c.end};
}


// ---- the dense stage of a batch of posed pairs (gms_dense_pairs_device) -----------------------------------------------------------------
// sgm_bytes: gms_stereo_sgm_workspace_bytes for the rectified size. Every call writes every word it later reads.
struct DensePairsLayout {
    size_t grey;   // uint8 [2][n][sh][sw]: the grey images of both cameras, for BGR input only
    size_t sgm;    // the matcher's workspace
    size_t cloud;  // DenseCloudLayout
    size_t total;
};
inline DensePairsLayout dense_pairs_layout(int n, int sw, int sh, int channels, int ow, int oh, size_t sgm_bytes)
{
    WsCursor c;
    return {c.take(channels == 3 ? 2 * (size_t)n * (size_t)sw * (size_t)sh : 0, 256), c.take(sgm_bytes, 256),
            c.take(dense_cloud_layout(n, ow, oh).total, 256), c.end};
}

// ---- the clouds of several pairs fused into one (dense_fuse_kernels.hip) -------------------------------------------------------------------
// Every source gets the blocks of max_cap points, source after source: block b of source i is word i * blocks_per_src + b. Every call
// writes every word it later reads.
constexpr int kFuseBlockPoints = 1024;  // points per workgroup of the mark and write kernels
inline int dense_fuse_blocks(int max_cap) { return (int)(((size_t)max_cap + kFuseBlockPoints - 1) / kFuseBlockPoints); }
struct DenseFuseLayout {
    size_t blocks;  // int32 [n_src][blocks_per_src]: kept points per block, then in place their exclusive prefix over all blocks
    size_t marks;   // uint8 [n_src][blocks_per_src * 1024][2]: per point its support byte (0x80: kept) and its conflict count
    size_t total;
};
inline DenseFuseLayout dense_fuse_layout(int n_src, int max_cap)
{
    const size_t nb = (size_t)n_src * (size_t)dense_fuse_blocks(max_cap);
    WsCursor c;
    return {c.take(4 * nb, 256), c.take(2 * nb * kFuseBlockPoints, 256), c.end};
}

// ---- the speckle filter (speckle_kernels.hip) ---------------------------------------------------------------------------------------
// Every call writes every word it later reads: the tile kernel writes both planes whole.
struct SpeckleLayout {
    size_t label;  // int32 [n][H][W]: union-find over pixel indices within the image; -1 where the pixel is new_val
    size_t size;   // int32 [n][H][W]: at a tile-local root the pixels of its tile-local component, at a global root the component's
    size_t total;
};
inline SpeckleLayout speckle_layout(int n, int W, int H)
{
    const size_t px = (size_t)n * (size_t)W * (size_t)H;  // n <= 65535, W, H <= 8192: below 2^42
    WsCursor c;
    return {c.take(4 * px, 256), c.take(4 * px, 256), c.end};
}

// ---- the dense stage with the speckle filter behind the matcher (gms_dense_pairs_filtered_device) -------------------------------------
// DensePairsLayout's regions unchanged, then the filter's own: it aliases none of the matcher's volumes.
struct DensePairsFilteredLayout {
    DensePairsLayout pairs;
    size_t speckle;  // SpeckleLayout of the rectified size
    size_t total;
};
inline DensePairsFilteredLayout dense_pairs_filtered_layout(int n, int sw, int sh, int channels, int ow, int oh, size_t sgm_bytes)
{
    const DensePairsLayout P = dense_pairs_layout(n, sw, sh, channels, ow, oh, sgm_bytes);
    WsCursor c;
    c.take(P.total, 256);
    const size_t speckle = c.take(speckle_layout(n, ow, oh).total, 256);
    return {P, speckle, c.end};
}

}  // namespace gms
