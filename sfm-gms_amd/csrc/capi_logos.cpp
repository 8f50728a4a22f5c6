// capi_logos.cpp -- the C ABI of the LOGOS match filter on resident frames, of its host batch, and of the dictionary trainer.
#include <algorithm>

#include "capi_common.h"
#include "gms_kernels.h"
#include "logos_batch.h"
#include "logos_dict_core.h"

extern "C" {

// ---- LOGOS on resident frames (logos_batch_kernels.hip) ----------------------------------------------------------------------
int64_t gms_logos_table_bytes(int64_t total_kp, int n_frames, int n_words)
{
    if (total_kp < 0 || n_frames < 0 || n_words < 1 || n_words > 65535) return 0;
    return gms::logos::table_layout(total_kp, n_frames, n_words).total;
}

size_t gms_logos_workspace_bytes(int64_t max_frame_kp, int n_pairs, int64_t max_query_kp)
{
    if (max_frame_kp < 0 || n_pairs < 0 || max_query_kp < 0) return 0;
    return (size_t)gms::logos::workspace_bytes(max_frame_kp, n_pairs, max_query_kp);
}

int gms_logos_prepare_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, int64_t total_kp,
                             const int32_t* d_words, int n_words, void* d_workspace, size_t ws_bytes, void* d_table)
{
    if (!c || n_frames < 0 || total_kp < 0 || n_words < 1 || n_words > 65535 || !d_table || !d_frame_off) return GMS_ERR_BAD_ARG;
    if (total_kp > 0 && (!d_kp || !d_words)) return GMS_ERR_BAD_ARG;
    if (ws_bytes > 0 && !d_workspace) return GMS_ERR_BAD_ARG;
    if (total_kp > INT32_MAX || misaligned(d_table, 16)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_logos_prepare(d_kp, d_frame_off, n_frames, total_kp, d_words, n_words, d_workspace, ws_bytes, d_table, c->n_cus,
                                         c->stream);
    });
}

int gms_logos_filter_device(gms_ctx* c, const void* d_table, const gms_pair* d_pairs, int n_pairs, void* d_workspace, size_t ws_bytes,
                            gms_dmatch* d_out, gms_logos_result* d_logos_results, gms_pair_result* d_pair_results)
{
    if (!c || n_pairs < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_table || !d_pairs || !d_workspace || !d_out || !d_logos_results) return GMS_ERR_BAD_ARG;
    if ((int64_t)ws_bytes < gms::logos::filter_fixed_bytes(n_pairs) || misaligned(d_workspace, 16)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_logos_filter(d_table, d_pairs, n_pairs, d_workspace, ws_bytes, d_out, d_logos_results, d_pair_results, c->n_cus,
                                        c->stream);
    });
}

int gms_logos_words_device(gms_ctx* c, int desc_kind, const void* d_desc, int64_t total_desc, const void* d_dict, int n_words,
                           int32_t* d_words)
{
    if (!c || total_desc < 0 || n_words < 1 || n_words > 65535 || !d_dict) return GMS_ERR_BAD_ARG;
    if (!desc_kind_ok(desc_kind)) return GMS_ERR_BAD_ARG;
    if (total_desc == 0) return GMS_OK;
    if (!d_desc || !d_words) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_logos_words(desc_kind, d_desc, total_desc, d_dict, n_words, d_words, c->n_cus, c->stream); });
}

int gms_logos_host_batch(gms_ctx* c, const gms_keypoint* kp, const int64_t* frame_off, int n_frames, const int32_t* words, int n_words,
                         const gms_pair* pairs, int n_pairs, gms_dmatch* out, gms_logos_result* results)
{
    if (!c || n_frames < 0 || n_pairs < 0 || n_words < 1 || n_words > 65535 || !frame_off) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!pairs || !results) return GMS_ERR_BAD_ARG;
    const int64_t total_kp = frame_off[n_frames];
    if (total_kp < 0 || total_kp > INT32_MAX || (total_kp > 0 && (!kp || !words))) return GMS_ERR_BAD_ARG;
    int64_t max_kp = 0, max_q = 0, out_len = 0;
    if (!frame_offsets_ascend(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    for (int f = 0; f < n_frames; f++) max_kp = std::max(max_kp, frame_off[f + 1] - frame_off[f]);
    for (int p = 0; p < n_pairs; p++) {
        const gms_pair& q = pairs[p];
        if (q.frame_a >= 0 && q.frame_a < n_frames) max_q = std::max(max_q, frame_off[q.frame_a + 1] - frame_off[q.frame_a]);
        if (q.m > 0 && q.match_off >= 0) out_len = std::max(out_len, q.match_off + (int64_t)q.m);
    }
    if (out_len > 0 && !out) return GMS_ERR_BAD_ARG;
    const size_t table = (size_t)gms_logos_table_bytes(total_kp, n_frames, n_words);
    const size_t ws = gms_logos_workspace_bytes(max_kp, n_pairs, max_q);
    const size_t b_kp = sizeof(gms_keypoint) * (size_t)total_kp, b_off = 8 * ((size_t)n_frames + 1), b_words = 4 * (size_t)total_kp;
    const size_t b_pairs = sizeof(gms_pair) * (size_t)n_pairs, b_res = sizeof(gms_logos_result) * (size_t)n_pairs;
    const size_t b_out = sizeof(gms_dmatch) * (size_t)out_len;
    gms::BlockLayout lay;
    const size_t o_kp = lay.add(b_kp), o_off = lay.add(b_off), o_w = lay.add(b_words), o_pairs = lay.add(b_pairs), o_res = lay.add(b_res);
    const size_t o_tab = lay.add(table), o_ws = lay.add(ws), o_out = lay.add(b_out, 16);
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    DevBlock blk(lay, c->stream);
    if (total_kp > 0) blk.in(o_kp, kp, b_kp);
    blk.in(o_off, frame_off, b_off);
    if (total_kp > 0) blk.in(o_w, words, b_words);
    blk.in(o_pairs, pairs, b_pairs);
    blk.run([&](hipStream_t st) {
        return gms::launch_logos_prepare(blk.at<gms_keypoint>(o_kp), blk.at<int64_t>(o_off), n_frames, total_kp, blk.at<int32_t>(o_w), n_words,
                                         blk.at(o_ws), ws, blk.at(o_tab), c->n_cus, st);
    });
    blk.run([&](hipStream_t st) {
        return gms::launch_logos_filter(blk.at(o_tab), blk.at<gms_pair>(o_pairs), n_pairs, blk.at(o_ws), ws, blk.at<gms_dmatch>(o_out),
                                        blk.at<gms_logos_result>(o_res), nullptr, c->n_cus, st);
    });
    blk.out(results, o_res, b_res);
    if (out_len > 0) blk.out(out, o_out, b_out);
    return blk.finish();
}

// ---- LOGOS dictionary training (logos_dict_kernels.hip) --------------------------------------------------------------------------
static bool logos_dict_params(int desc_kind, int64_t total_rows, int n_sets, int n_words, int attempts, int max_iters, uint64_t seed,
                              gms::logos_dict::Params* p)
{
    p->kind = desc_kind;
    p->n_sets = n_sets;
    p->n_words = n_words;
    p->attempts = attempts;
    p->max_iters = max_iters;
    p->row_bytes = (int)desc_row_bytes(desc_kind);
    p->total_rows = total_rows;
    p->seed = seed;
    return desc_kind_ok(desc_kind) && gms::logos_dict::params_ok(*p);
}

size_t gms_logos_dict_workspace_bytes(int desc_kind, int64_t total_rows, int n_sets, int n_words, int attempts, int max_iters)
{
    gms::logos_dict::Params p;
    if (!logos_dict_params(desc_kind, total_rows, n_sets, n_words, attempts, max_iters, 0, &p)) return 0;
    return gms::logos_dict_ws_bytes(p);
}

int gms_logos_dict_train_device(gms_ctx* c, int desc_kind, const void* d_desc, const int64_t* d_set_off, int n_sets, int64_t total_rows,
                                int n_words, int attempts, int max_iters, uint64_t seed, void* d_workspace, size_t ws_bytes, void* d_dict,
                                gms_logos_dict_result* d_results, int32_t* d_labels)
{
    gms::logos_dict::Params p;
    if (!c || !logos_dict_params(desc_kind, total_rows, n_sets, n_words, attempts, max_iters, seed, &p)) return GMS_ERR_BAD_ARG;
    if (n_sets == 0) return GMS_OK;
    if (!d_set_off || !d_workspace || !d_dict || !d_results || (total_rows > 0 && !d_desc)) return GMS_ERR_BAD_ARG;
    if (ws_bytes < gms::logos_dict_ws_bytes(p) || misaligned(d_workspace, 16)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_logos_dict_train(p, d_desc, d_set_off, d_workspace, d_dict, d_results, d_labels, c->stream); });
}

int gms_logos_dict_train(int desc_kind, const void* desc, const int64_t* set_off, int n_sets, int n_words, int attempts, int max_iters,
                         uint64_t seed, void* dict, gms_logos_dict_result* results, int32_t* labels)
{
    if (n_sets < 0 || !set_off) return GMS_ERR_BAD_ARG;
    const int64_t total = set_off[n_sets];
    gms::logos_dict::Params p;
    if (!logos_dict_params(desc_kind, total, n_sets, n_words, attempts, max_iters, seed, &p)) return GMS_ERR_BAD_ARG;
    if (n_sets == 0) return GMS_OK;
    if (!dict || !results || (total > 0 && !desc)) return GMS_ERR_BAD_ARG;
    const size_t b_desc = (size_t)p.row_bytes * (size_t)total, b_off = 8 * ((size_t)n_sets + 1);
    const size_t b_dict = (size_t)p.row_bytes * (size_t)n_words * (size_t)n_sets, b_res = sizeof(gms_logos_dict_result) * (size_t)n_sets;
    const size_t b_lab = 4 * (size_t)total;
    gms::BlockLayout lay;
    const size_t o_desc = lay.add(b_desc, 16), o_off = lay.add(b_off), o_dict = lay.add(b_dict), o_res = lay.add(b_res);
    const size_t o_lab = lay.add(b_lab, 16), o_ws = lay.add(gms::logos_dict_ws_bytes(p));
    GMS_HIP(hipSetDevice(0));
    DevBlock blk(lay, nullptr);
    const bool with_labels = labels && total > 0;
    if (total > 0) blk.in(o_desc, desc, b_desc);
    blk.in(o_off, set_off, b_off);
    if (with_labels) blk.in(o_lab, labels, b_lab);  // rows outside every set keep theirs
    blk.run([&](hipStream_t st) {
        return gms::launch_logos_dict_train(p, blk.at(o_desc), blk.at<int64_t>(o_off), blk.at(o_ws), blk.at(o_dict), blk.at<gms_logos_dict_result>(o_res),
                                            labels ? blk.at<int32_t>(o_lab) : nullptr, st);
    });
    blk.out(dict, o_dict, b_dict);
    blk.out(results, o_res, b_res);
    if (with_labels) blk.out(labels, o_lab, b_lab);
    return blk.finish();
}

}  // extern "C"
