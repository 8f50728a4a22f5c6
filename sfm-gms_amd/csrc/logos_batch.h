// logos_batch.h -- layouts shared by the batched LOGOS path (logos_batch_kernels.hip) and its C ABI (capi_logos.cpp): the per-frame
// table gms_logos_prepare_device builds and the workspace of gms_logos_prepare_device / gms_logos_filter_device. Both are opaque to
// callers, who only size them (gms_logos_table_bytes, gms_logos_workspace_bytes).
#pragma once
#include <stdint.h>

#include "logos_core.h"

namespace gms {
namespace logos {

// ---- the table: a 64-byte header, then sections at 16-byte aligned offsets that follow from the header alone, so the kernels
// find them without the host knowing anything beyond the pointer ----------------------------------------------------------------
constexpr int64_t kTableMagic = 0x3130534f474f4c47ll;  // "GLOGOS01"
struct TableHeader {
    int64_t magic, total_kp;
    int32_t n_frames, n_words;
    int32_t reserved[10];
};
static_assert(sizeof(TableHeader) == 64, "table header");

struct TableLayout {
    int64_t frame_off;  // int64 [n_frames + 1]: the caller's keypoint offsets, copied
    int64_t status;     // int32 [n_frames]: GMS_OK, GMS_ERR_DOMAIN (a word out of range), GMS_ERR_BAD_ARG (workspace too small)
    int64_t items;      // int32 [n_frames + 1]: prefix of the five-nearest pass's workgroups per frame
    int64_t ties;       // int32 [1 + total_kp]: count, then the keypoints (global index) whose fifth neighbour is tied
    int64_t pts;        // Pt [total_kp]: x, y, orientation, log scale
    int64_t word;       // int32 [total_kp]
    int64_t nb;         // int32 [5 total_kp]: the five nearest, frame-local indices (-1 pads)
    int64_t sorted;     // int32 [total_kp]: per frame, its local indices by word (stable)
    int64_t bucket;     // int32 [n_frames (n_words + 1)]: per frame, where each word's run starts in `sorted`
    int64_t total;
};

GMS_HD int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

GMS_HD TableLayout table_layout(int64_t total_kp, int n_frames, int n_words)
{
    TableLayout L;
    int64_t o = (int64_t)sizeof(TableHeader);
    L.frame_off = o;
    o = align16(o + 8 * ((int64_t)n_frames + 1));
    L.status = o;
    o = align16(o + 4 * (int64_t)n_frames);
    L.items = o;
    o = align16(o + 4 * ((int64_t)n_frames + 1));
    L.ties = o;
    o = align16(o + 4 * (total_kp + 1));
    L.pts = o;
    o = align16(o + (int64_t)sizeof(Pt) * total_kp);
    L.word = o;
    o = align16(o + 4 * total_kp);
    L.nb = o;
    o = align16(o + 4 * (int64_t)kNum * total_kp);
    L.sorted = o;
    o = align16(o + 4 * total_kp);
    L.bucket = o;
    o = align16(o + 4 * (int64_t)n_frames * ((int64_t)n_words + 1));
    L.total = o;
    return L;
}

// ---- the workspace ----------------------------------------------------------------------------------------------------------------
// prepare: kTieLanes slices, one per lane of the tie pass, each of 2 (n - 1) words for a tied point of an n-point frame
constexpr int kTieBlock = 64;
constexpr int kTieLanes = 512;
GMS_HD int64_t tie_slice_records(int64_t ws_bytes) { return ws_bytes / kTieLanes / 8; }

// filter: a 64-byte header (the batch's query count), one PairWork per pair, then one int64 per query keypoint of the batch
struct PairWork {
    int64_t q_start;         // first query of the pair in the batch's query numbering
    int64_t n_cand, n_supp;  // pass 1
    int64_t total;           // survivors (scan)
    int64_t base_a, base_b;  // global index of the frames' first keypoints
    int32_t n1, n2;          // keypoints of frame_a / frame_b (n1 = 0 unless the pair is valid)
    int32_t status;
    int32_t peak_bin;
    float peak;
    int32_t frame_b;         // for its word buckets
    int32_t reserved[2];
    int32_t bins[kBins];
    int32_t pad[3];
};
static_assert(sizeof(PairWork) % 16 == 0, "PairWork is an array element of 16-byte alignment");
constexpr int64_t kFilterHeaderBytes = 64;

GMS_HD int64_t filter_fixed_bytes(int n_pairs) { return kFilterHeaderBytes + (int64_t)sizeof(PairWork) * n_pairs; }

GMS_HD int64_t workspace_bytes(int64_t max_frame_kp, int n_pairs, int64_t max_query_kp)
{
    const int64_t m = max_frame_kp > 1 ? max_frame_kp - 1 : 1;
    const int64_t prep = (int64_t)kTieLanes * 8 * m;
    const int64_t filt = filter_fixed_bytes(n_pairs) + 8 * (int64_t)n_pairs * (max_query_kp > 0 ? max_query_kp : 0);
    return prep > filt ? prep : filt;
}

}  // namespace logos
}  // namespace gms
