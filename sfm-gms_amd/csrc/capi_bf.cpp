// capi_bf.cpp -- the C ABI of the brute-force matcher and bruteForceMatch's selection (bf_kernels.hip, bf_select_kernels.hip).
#include <algorithm>
#include <cmath>

#include "capi_common.h"
#include "gms_kernels.h"

extern "C" {

int64_t gms_bf_prepared_bytes(int desc_kind, int64_t total_desc, int n_frames)
{
    return (int64_t)gms::bf_prepared_bytes(desc_kind, total_desc, n_frames);
}

int gms_bf_prepare_device(gms_ctx* c, int desc_kind, const void* d_desc, const int64_t* d_frame_off, int n_frames,
                          int64_t total_desc, void* d_prepared)
{
    if (!c || n_frames < 0 || total_desc < 0) return GMS_ERR_BAD_ARG;
    if (!desc_kind_ok(desc_kind)) return GMS_ERR_BAD_ARG;
    if (total_desc == 0 || n_frames == 0) return GMS_OK;
    if (!d_desc || !d_frame_off || !d_prepared) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_bf_prepare(desc_kind, d_desc, d_frame_off, n_frames, total_desc, d_prepared, c->stream); });
}

int gms_bfmatch_device(gms_ctx* c, int desc_kind, const void* d_desc, const void* d_prepared, int64_t total_desc,
                       const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_query,
                       gms_dmatch* d_matches)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_query < 0 || total_desc < 0) return GMS_ERR_BAD_ARG;
    if (!desc_kind_ok(desc_kind)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0 || max_query == 0) return GMS_OK;
    if (!d_desc || !d_frame_off || !d_pairs || !d_matches) return GMS_ERR_BAD_ARG;
    if (desc_kind == GMS_DESC_L2_F32X128 && !d_prepared) return GMS_ERR_BAD_ARG;
    if (max_query > (1 << 22)) return GMS_ERR_CAPACITY;
    return on_ctx(c, [&] {
        return gms::launch_bf_match(desc_kind, d_desc, d_prepared, total_desc, d_frame_off, n_frames, d_pairs, n_pairs, max_query, d_matches,
                                    c->stream);
    });
}

size_t gms_bf_select_workspace_bytes(int n_pairs, int max_rows, int64_t total_backward_rows)
{
    if (n_pairs < 0 || max_rows < 0 || max_rows > (1 << 22) || total_backward_rows < 0) return 0;
    return gms::bf_select_ws_bytes(n_pairs, max_rows, total_backward_rows);
}

static bool bf_select_args_ok(int desc_kind, int cross_check, double coef, int max_size)
{
    return desc_kind_ok(desc_kind) && (cross_check == 0 || cross_check == 1) &&
           std::isfinite(coef) && coef >= 1.0 && max_size >= 0;
}

int gms_bf_select_device(gms_ctx* c, int desc_kind, const void* d_desc, const void* d_prepared, int64_t total_desc,
                         const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_rows, int cross_check,
                         double distance_coef, int max_size, void* d_ws, size_t ws_bytes, gms_dmatch* d_out, gms_bf_result* d_bf_results,
                         gms_pair_result* d_pair_results)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_rows < 0 || max_rows > (1 << 22) || total_desc < 0) return GMS_ERR_BAD_ARG;
    if (!bf_select_args_ok(desc_kind, cross_check, distance_coef, max_size)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_pairs || !d_ws || !d_out || !d_bf_results || (total_desc > 0 && !d_desc)) return GMS_ERR_BAD_ARG;
    if (desc_kind == GMS_DESC_L2_F32X128 && total_desc > 0 && !d_prepared) return GMS_ERR_BAD_ARG;
    // the workspace's size fixes how many matcher rows it holds (total_backward_rows of gms_bf_select_workspace_bytes)
    const size_t fixed = gms::bf_select_ws_bytes(n_pairs, max_rows, 0);
    if (!ws_ok(d_ws, ws_bytes, fixed)) return GMS_ERR_BAD_ARG;
    const int64_t total_back = (int64_t)((ws_bytes - fixed) / 256) * 16;  // whole 256-byte blocks, as the layout aligns them
    return on_ctx(c, [&] {
        return gms::launch_bf_select(desc_kind, d_desc, d_prepared, total_desc, d_frame_off, n_frames, d_pairs, n_pairs, max_rows, total_back,
                                     cross_check, distance_coef, max_size, d_ws, d_out, d_bf_results, d_pair_results, c->stream);
    });
}

int gms_bf_match_select(int desc_kind, const void* desc1, int n1, const void* desc2, int n2, int cross_check, double distance_coef,
                        int max_size, gms_dmatch* out, int64_t out_cap, int64_t* n_out, gms_bf_result* result)
{
    if (n_out) *n_out = 0;
    if (result) *result = gms_bf_result{0, 0, 0, 0.0f, GMS_OK};
    if (n1 < 0 || n2 < 0 || n1 > (1 << 22) || n2 > (1 << 22) || out_cap < 0 || out_cap > INT32_MAX || !n_out) return GMS_ERR_BAD_ARG;
    if (!bf_select_args_ok(desc_kind, cross_check, distance_coef, max_size)) return GMS_ERR_BAD_ARG;
    if ((n1 > 0 && !desc1) || (n2 > 0 && !desc2) || (out_cap > 0 && !out)) return GMS_ERR_BAD_ARG;
    const size_t row = desc_row_bytes(desc_kind);
    const int64_t total = (int64_t)n1 + n2;
    const int max_rows = std::max(n1, n2);
    const int64_t back_rows = cross_check ? n2 : n1;
    gms::BlockLayout lay;
    const size_t o_desc = lay.add(row * (size_t)total, 16), o_off = lay.add(3 * 8), o_pair = lay.add(sizeof(gms_pair));
    const size_t o_res = lay.add(sizeof(gms_bf_result)), o_prep = lay.add((size_t)gms::bf_prepared_bytes(desc_kind, total, 2), 16);
    const size_t o_ws = lay.add(gms::bf_select_ws_bytes(1, max_rows, back_rows)), o_out = lay.add(sizeof(gms_dmatch) * (size_t)out_cap, 16);
    DevBlock blk(lay, nullptr);
    const int64_t off[3] = {0, n1, total};
    const gms_pair pr{0, 1, (int32_t)out_cap, 0, 0};
    if (n1 > 0) blk.in(o_desc, desc1, row * (size_t)n1);
    if (n2 > 0) blk.in(o_desc + row * (size_t)n1, desc2, row * (size_t)n2);
    blk.in(o_off, off, sizeof(off));
    blk.in(o_pair, &pr, sizeof(pr));
    if (total > 0)
        blk.run([&](hipStream_t st) { return gms::launch_bf_prepare(desc_kind, blk.at(o_desc), blk.at<int64_t>(o_off), 2, total, blk.at(o_prep), st); });
    blk.run([&](hipStream_t st) {
        return gms::launch_bf_select(desc_kind, blk.at(o_desc), blk.at(o_prep), total, blk.at<int64_t>(o_off), 2, blk.at<gms_pair>(o_pair), 1,
                                     max_rows, back_rows, cross_check, distance_coef, max_size, blk.at(o_ws), blk.at<gms_dmatch>(o_out),
                                     blk.at<gms_bf_result>(o_res), nullptr, st);
    });
    // the result record first, then exactly the matches it counts
    gms_bf_result r{0, 0, 0, 0.0f, GMS_OK};
    blk.out(&r, o_res, sizeof(r));
    blk.sync();
    if (blk.ok() && r.status == GMS_OK && r.n_out > 0) blk.out_now(out, o_out, sizeof(gms_dmatch) * (size_t)r.n_out);
    GMS_TRY(blk.finish());
    *n_out = r.n_out;
    if (result) *result = r;
    return r.status;
}

int gms_bf_select_host_batch(gms_ctx* c, int desc_kind, const void* desc, const int64_t* frame_off, int n_frames, const gms_pair* pairs,
                             int n_pairs, int cross_check, double distance_coef, int max_size, gms_dmatch* out, gms_bf_result* results)
{
    if (!c || n_frames < 0 || n_pairs < 0 || !frame_off) return GMS_ERR_BAD_ARG;
    if (!bf_select_args_ok(desc_kind, cross_check, distance_coef, max_size)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!pairs || !results) return GMS_ERR_BAD_ARG;
    const int64_t total = frame_off[n_frames];
    if (total < 0 || (total > 0 && !desc)) return GMS_ERR_BAD_ARG;
    int64_t max_rows = 0, back = 0, out_len = 0;
    if (!frame_offsets_ascend(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    for (int p = 0; p < n_pairs; p++) {
        const gms_pair& q = pairs[p];
        if (q.frame_a < 0 || q.frame_a >= n_frames || q.frame_b < 0 || q.frame_b >= n_frames) continue;  // reported per pair
        const int64_t na = frame_off[q.frame_a + 1] - frame_off[q.frame_a], nb = frame_off[q.frame_b + 1] - frame_off[q.frame_b];
        max_rows = std::max(max_rows, std::max(na, nb));
        back += cross_check ? nb : na;
        if (q.m > 0 && q.match_off >= 0) out_len = std::max(out_len, q.match_off + (int64_t)q.m);
    }
    if (max_rows > (1 << 22)) return GMS_ERR_CAPACITY;
    if (out_len > 0 && !out) return GMS_ERR_BAD_ARG;
    const size_t row = desc_row_bytes(desc_kind), b_off = 8 * ((size_t)n_frames + 1), b_pairs = sizeof(gms_pair) * (size_t)n_pairs;
    const size_t b_res = sizeof(gms_bf_result) * (size_t)n_pairs, b_out = sizeof(gms_dmatch) * (size_t)out_len;
    gms::BlockLayout lay;
    const size_t o_desc = lay.add(row * (size_t)total, 16), o_off = lay.add(b_off), o_pairs = lay.add(b_pairs), o_res = lay.add(b_res);
    const size_t o_prep = lay.add((size_t)gms::bf_prepared_bytes(desc_kind, total, n_frames), 16);
    const size_t o_ws = lay.add(gms::bf_select_ws_bytes(n_pairs, max_rows, back)), o_out = lay.add(b_out, 16);
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    DevBlock blk(lay, c->stream);
    if (total > 0) blk.in(o_desc, desc, row * (size_t)total);
    blk.in(o_off, frame_off, b_off);
    blk.in(o_pairs, pairs, b_pairs);
    if (total > 0)
        blk.run([&](hipStream_t st) {
            return gms::launch_bf_prepare(desc_kind, blk.at(o_desc), blk.at<int64_t>(o_off), n_frames, total, blk.at(o_prep), st);
        });
    blk.run([&](hipStream_t st) {
        return gms::launch_bf_select(desc_kind, blk.at(o_desc), blk.at(o_prep), total, blk.at<int64_t>(o_off), n_frames, blk.at<gms_pair>(o_pairs),
                                     n_pairs, (int)max_rows, back, cross_check, distance_coef, max_size, blk.at(o_ws), blk.at<gms_dmatch>(o_out),
                                     blk.at<gms_bf_result>(o_res), nullptr, st);
    });
    blk.out(results, o_res, b_res);
    if (out_len > 0) blk.out(out, o_out, b_out);
    return blk.finish();
}

}  // extern "C"
