// gms_capi.cpp -- the C ABI declared in include/gms.h, on top of the HIP kernels.
//
// Host side of the drop-in for cv::xfeatures2d::matchGMS (FeatureMatchUtil.cpp:69,
// DisparityUtil.cpp:149,299 of the reference). There is deliberately no CPU implementation of the
// filter in this library: without a working HIP device every compute entry point returns an error.
//
// This file owns the context (capi_common.h) and holds the filter and its host-pointer paths; the other families of entry points
// are the capi_*.cpp beside it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "capi_common.h"
#include "copy_pool.h"
#include "gms_kernels.h"

static_assert(sizeof(gms_keypoint) == 28, "gms_keypoint must match cv::KeyPoint (stride 0x1c)");
static_assert(sizeof(gms_dmatch) == 16, "gms_dmatch must match cv::DMatch (stride 0x10)");
static_assert(sizeof(gms_pair) == 24, "gms_pair layout");
static_assert(sizeof(gms_pair_result) == 16, "gms_pair_result layout");

static thread_local int t_last_hip = 0;
// for the other translation units of the library (capi_*.cpp through GMS_HIP, logos_kernels.hip): what gms_last_hip_error() reports
namespace gms {
void record_hip_error(int e) { t_last_hip = e; }
}
#ifdef GMS_PHASE_TIMING
static unsigned long long* g_diag = nullptr;
extern "C" int gms_diag_set_buffer(void* d_buf) { g_diag = (unsigned long long*)d_buf; return 0; }
#endif

namespace {

// Diagnostic switches, read from the environment ONCE per process (never on the call path):
//   GMS_DENSE=0          keep every pair on the hashed path
//   GMS_BAND=0           keep large pairs on the HBM-slab kernel alone
//   GMS_STREAM=0         pairs of 16 385 .. 65 536 matches: the 16-bit band / tile kernels instead of the streamed byte-matrix kernels
//   GMS_PROBE_NIBBLE=m   which scale probes try four-bit entries first: 8 = the 28 x 28 grid, 16 = the 40 x 40 grid (default), 24 = both, 0 = none
//   GMS_STAGGER_US=n     spread of the first dispatch round's start times at 10k matches per pair (0 = off)
//   GMS_BAND_WS_BYTES=n  budget of the large-pair workspace (default 4 GiB); a batch is filtered in slices that fit it
//   GMS_DEAL=0|1         never / always deal the matches to the lanes of the byte-matrix kernel (default: what the probe saw)
//   GMS_IDENT=0|1        never / always try the byte-matrix kernel's identity-query instantiation under the default flags (default: what the probe saw)
//   GMS_SCALE_PROBE=0|1  never / always bound the finer scale hypotheses' inlier counts first (default: while it pays, see below)
//   GMS_CHECK_PAIRS=0|1  never / always validate the pair table behind a launch (default: the first launch and every sixteenth)
//   GMS_PREFETCH=t[,a]   byte-matrix kernel: before grid type t (0..3, default 3; -1 = never) a workgroup touches the match records of
//                        the pair a places ahead (default: the number of CUs = the pair its CU's next workgroup takes)
struct Knobs {
    bool dense_on = true, band_on = true, stream_on = true;
    int probe_nibble = 16;  // which fine right grids (bit 3: 28 x 28, bit 4: 40 x 40) a scale probe tries with four-bit entries first when the probe is forced on
    bool probe_nibble_set = false;  // GMS_PROBE_NIBBLE given: also a limit on what the library chooses by itself
    int stagger_us = -1, deal = -1, scale_probe = -1, check_pairs = -1, ident = -1;
    int prefetch_type = 3, prefetch_ahead = 0;
    size_t band_ws_budget = (size_t)4 << 30;
};
const Knobs& knobs()
{
    static const Knobs k = [] {
        Knobs v;
        if (const char* e = std::getenv("GMS_DENSE")) v.dense_on = std::atoi(e) != 0;
        if (const char* e = std::getenv("GMS_BAND")) v.band_on = std::atoi(e) != 0;
        if (const char* e = std::getenv("GMS_STREAM")) v.stream_on = std::atoi(e) != 0;
        if (const char* e = std::getenv("GMS_PROBE_NIBBLE")) { v.probe_nibble = (int)std::strtol(e, nullptr, 0) & 24; v.probe_nibble_set = true; }
        if (const char* e = std::getenv("GMS_STAGGER_US")) v.stagger_us = std::atoi(e);
        if (const char* e = std::getenv("GMS_DEAL")) v.deal = std::atoi(e) != 0 ? 1 : 0;
        if (const char* e = std::getenv("GMS_IDENT")) v.ident = std::atoi(e) != 0 ? 1 : 0;
        if (const char* e = std::getenv("GMS_SCALE_PROBE")) v.scale_probe = std::atoi(e) != 0 ? 1 : 0;
        if (const char* e = std::getenv("GMS_CHECK_PAIRS")) v.check_pairs = std::atoi(e) != 0 ? 1 : 0;
        if (const char* e = std::getenv("GMS_PREFETCH")) {
            v.prefetch_type = std::atoi(e);
            if (const char* comma = std::strchr(e, ',')) v.prefetch_ahead = std::atoi(comma + 1);
        }
        if (const char* e = std::getenv("GMS_BAND_WS_BYTES")) {
            const long long b = std::atoll(e);
            if (b > 0) v.band_ws_budget = (size_t)b;
        }
        return v;
    }();
    return k;
}

// mScaleRatios (DLL .data 0x1802c5008) and setScale's cvRound (DLL@0x180048c10, cvtsd2si = lrint).
void right_grids(int rw[5], int rh[5])
{
    const double ratio[5] = {1.0, 1.0 / 2, 1.0 / std::sqrt(2.0), std::sqrt(2.0), 2.0};
    for (int s = 0; s < 5; ++s) {
        rw[s] = (int)std::lrint(gms::kLeftW * ratio[s]);
        rh[s] = (int)std::lrint(gms::kLeftH * ratio[s]);
    }
}

// What one gms_filter_device call needs beyond its arguments.
struct WsNeed {
    size_t partial = 0, big = 0, band = 0;
    size_t slice = 0, per_pair = 0;  // large pairs: pairs per slice of the batch, workspace bytes per pair
    int kpt = 0, mcap = 0;
    bool stream = false;             // large pairs up to 65 536 matches: the streamed byte-matrix kernels
};

int plan_workspace(const gms_ctx* c, int n_pairs, int max_m, bool rot, bool scale, bool need_mask_ws, bool allow_stream, WsNeed* w)
{
    *w = WsNeed();
    w->kpt = gms::filter_pick_kpt(max_m);  // 0: too large for the register + LDS kernel
    if (w->kpt) {
        if (scale && knobs().dense_on) w->partial = (size_t)n_pairs * gms::kPartialStrideDw * 4;
        return GMS_OK;
    }
    if (max_m > gms::kBigMaxMatches) return GMS_ERR_CAPACITY;
    w->mcap = gms::big_mcap(max_m);
    const int n_wg = n_pairs < c->n_cus ? n_pairs : c->n_cus;  // one persistent workgroup per CU at most
    w->big = (size_t)n_wg * gms::big_ws_stride_dwords(w->mcap) * 4;
    if (knobs().band_on) {
        gms::FilterParams p{};
        p.with_rotation = rot;
        p.with_scale = scale;
        right_grids(p.right_w, p.right_h);
        // pairs up to 65 536 matches: the streamed byte-matrix kernels -- one workgroup per (pair, scale, grid type, band) with scale
        // hypotheses, one per pair without (tools/config4_bench.py has both against the 16-bit band / tile kernels)
        w->stream = knobs().stream_on && max_m <= gms::stream_max_matches() && allow_stream;
        w->per_pair = w->stream ? std::max(gms::stream_ws_bytes_per_pair(p, w->mcap, need_mask_ws), scale ? (size_t)0 : gms::stream_dense_ws_bytes_per_pair(w->mcap))
                                : (!rot && !scale) ? gms::band_ws_bytes_per_pair(w->mcap, need_mask_ws)
                                                   : gms::tile_ws_bytes_per_pair(p, w->mcap, need_mask_ws);
        size_t slice = knobs().band_ws_budget / w->per_pair;
        if (slice < 1) slice = 1;
        if (slice > (size_t)n_pairs) slice = (size_t)n_pairs;
        w->slice = slice;
        w->band = slice * w->per_pair;
    }
    return GMS_OK;
}

// Grows the context's workspaces to `w`. Growing frees the old block, so everything that may still use it is waited for first;
// inside a stream capture that is impossible (and so is the allocation): GMS_ERR_NOT_RESERVED.
int grow_workspace(gms_ctx* c, const WsNeed& w, hipStream_t st)
{
    if (w.partial <= c->partial_ws.cap && w.big <= c->big_ws.cap && w.band <= c->band_ws.cap) return GMS_OK;
    if (stream_is_capturing(st)) return GMS_ERR_NOT_RESERVED;
    GMS_HIP(hipStreamSynchronize(st));
    if (c->ws_pending) {
        GMS_HIP(hipEventSynchronize(c->ws_event));
        c->ws_pending = false;
    }
    GMS_HIP(c->partial_ws.reserve(w.partial));
    GMS_HIP(c->big_ws.reserve(w.big));
    GMS_HIP(c->band_ws.reserve(w.band));
    return GMS_OK;
}

// A frame table build on stream `st`: normalize_kernel and, behind it, the context's per-frame side records and the stamp that ties them to the table. The records' buffer grows like the filter's workspaces -- never inside a stream capture, and only after everything that may
// still read the old block has finished; a build that cannot have records (a capture that would have to allocate, more frames than
// kSideMaxBytes holds) stamps its table 0, and the filter then never takes the identity path on it. The caller holds c->mu.
int build_frame_table(gms_ctx* c, hipStream_t st, const void* d_kp, int kp_stride_bytes, const int64_t* d_frame_off, const int32_t* d_wh,
                      int n_frames, int64_t total_kp, float* d_pts)
{
    if (total_kp <= 0) return GMS_OK;
    const size_t need = (size_t)(n_frames > 0 ? n_frames : 0) * sizeof(gms::SideRecord);
    bool with_side = n_frames > 0 && need <= gms::kSideMaxBytes;
    if (with_side && need > c->side.cap) {
        if (stream_is_capturing(st)) {
            with_side = false;
        } else {
            GMS_HIP(hipDeviceSynchronize());  // (earlier filter launches of any stream may still read the old records)
            GMS_HIP(c->side.reserve(need));
        }
    }
    const uint64_t stamp = with_side ? 1 : 0;  // (records wanted; the stamp itself is worked out on the device: table_stamp_kernel)
    c->side_stamp = 0;  // (a failed launch leaves no records to use)
    c->side_frames = 0;
    GMS_HIP(gms::launch_normalize(d_kp, kp_stride_bytes, d_frame_off, d_wh, n_frames, total_kp, d_pts,
                                  with_side ? (gms::SideRecord*)c->side.p : nullptr, stamp, st));
    c->side_stamp = stamp;
    c->side_frames = with_side ? n_frames : 0;
    return GMS_OK;
}

// A verdict kernel behind a launch on `st`: launch(v) -> hipError_t gets the device pointer of the verdict words, and the event behind
// it is what a later launch finds complete before it adopts them.
template <class Launch>
int launch_verdict(gms_ctx* c, hipStream_t st, Launch&& launch)
{
    void* dflag = nullptr;
    GMS_HIP(hipHostGetDevicePointer(&dflag, c->verdict, 0));
    GMS_HIP(launch((uint32_t*)dflag));
    GMS_HIP(hipEventRecord(c->verdict_event, st));
    c->verdict_pending = true;
    return GMS_OK;
}

// The filter launches of one call on stream `st`. The caller holds c->mu and has selected the device.
int filter_launch(gms_ctx* c, hipStream_t st, const float* d_pts, const int64_t* d_frame_off, int n_frames,
                  const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_matches,
                  int with_rotation, int with_scale, double threshold_factor,
                  gms_dmatch* d_out, gms_pair_result* d_results, uint8_t* d_mask, bool validate_pairs = true)
{
    if (n_pairs < 0 || max_m < 0 || n_frames < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_pairs || !d_results) return GMS_ERR_BAD_ARG;
    if (max_m > 0 && (!d_matches || !d_out || !d_pts)) return GMS_ERR_BAD_ARG;
    const bool capturing = stream_is_capturing(st);
    if (gms::filter_pick_kpt(max_m) == 0 && !capturing) {
        // large pairs: the streamed kernels' report of pairs they could not keep (read without waiting: it only steers which of two
        // bit-identical paths runs)
        const uint32_t now = ((volatile uint32_t*)c->verdict)[2];
        if (now != c->overflow_seen) {
            c->overflow_seen = now;
            c->stream_penalty = 64;
        } else if (c->stream_penalty > 0) {
            --c->stream_penalty;
        }
    }
    WsNeed w;
    GMS_TRY(plan_workspace(c, n_pairs, max_m, with_rotation != 0, with_scale != 0, d_mask == nullptr, c->stream_penalty == 0, &w));
    GMS_TRY(grow_workspace(c, w, st));
    const bool uses_ws = w.partial || w.big || w.band;
    if (uses_ws && !capturing && c->ws_pending && c->ws_stream != st) GMS_HIP(hipStreamWaitEvent(st, c->ws_event, 0));

    gms::FilterParams p{};
    const int kpt = w.kpt;
    p.table_slots = kpt ? gms::filter_table_slots(kpt) : 0;
    p.region_shift = kpt ? gms::filter_region_shift(kpt) : 0;
    p.pts = reinterpret_cast<const float2*>(reinterpret_cast<const char*>(d_pts) + gms::kTableHeaderBytes);  // behind the table's header
    p.frame_off = d_frame_off;
    p.n_frames = n_frames;
    p.pairs = d_pairs;
    p.n_pairs = n_pairs;
    p.stagger_blocks = c->n_cus;
    p.prefetch_type = knobs().prefetch_type;
    p.prefetch_ahead = knobs().prefetch_ahead > 0 ? knobs().prefetch_ahead : c->n_cus;
    p.matches = d_matches;
    p.out = d_out;
    p.results = d_results;
    p.mask = d_mask;
    p.with_rotation = with_rotation ? 1 : 0;
    p.with_scale = with_scale ? 1 : 0;
    p.threshold_factor = threshold_factor;
    p.pair_flags = nullptr;
    p.partial = nullptr;
    p.dealt = 0;
    right_grids(p.right_w, p.right_h);
    // the byte-matrix path is tried first whenever there are no scale hypotheses (the reference's default flags,
    // DisparityUtil.cpp:149,299)
    p.dense = (knobs().dense_on && !with_scale) ? 1 : 0;
    if (c->verdict_pending && !capturing && hipEventQuery(c->verdict_event) == hipSuccess) {
        c->use_dealt = c->verdict[0] != 0u ? 1 : 0;
        c->use_probe = (int)c->verdict[1];
        c->use_ident = c->verdict[3] != 0u ? 1 : 0;
        c->verdict_pending = false;
    }
    if (!capturing) {
        // pairs an IDENT launch had to hand to the generic body (read without waiting: it only steers which of two bit-identical
        // instantiations runs): off until a later probe says otherwise
        const uint32_t now = ((volatile uint32_t*)c->verdict)[4];
        if (now != c->ident_misses_seen) {
            c->ident_misses_seen = now;
            c->use_ident = 0;
        }
    }
    const int force_ident = c->opt_ident >= 0 ? c->opt_ident : knobs().ident;
    // (only where the context's side records are current; the kernel checks table and records pair by pair whatever is asked for here)
    p.side = (const gms::SideRecord*)c->side.p;
    p.side_frames = c->side_frames;
    p.side_stamp = c->side_stamp;
    p.ident = (p.dense && kpt && !with_rotation && c->side.p != nullptr && c->side_frames >= 1 && c->side_stamp != 0 &&
               (force_ident >= 0 ? force_ident != 0 : c->use_ident != 0)) ? 1 : 0;
    const int force_deal = c->opt_deal >= 0 ? c->opt_deal : knobs().deal, force_probe = c->opt_probe >= 0 ? c->opt_probe : knobs().scale_probe;
    const bool scales_matrix = kpt && with_scale && knobs().dense_on;  // (the byte-matrix kernel of the scale hypotheses deals too)
    p.dealt = ((p.dense || scales_matrix) && kpt && (force_deal >= 0 ? force_deal != 0 : c->use_dealt != 0)) ? 1 : 0;
    // First-round stagger: the spread is about two thirds of a pair's duration on the path the launch will mostly take -- 16 us (byte
    // matrix) / 72 us (hashed) at 10k matches, in proportion to max_m -- in ticks of the 100 MHz wall clock. Only launches of
    // at least four dispatch rounds are staggered, and none with scale hypotheses on the byte matrix: a pair takes ten times as
    // long there and its loads are a small share of it, so the spread only delays (1.12 ms against 1.18 per 2048 pairs without).
    const bool scales_on_matrix = with_scale && knobs().dense_on;
    p.stagger_ticks = 0;
    if (n_pairs >= 4 * p.stagger_blocks && kpt && max_m >= 2048) {  // (measured neutral at 4k matches, -1 % at 500: tools/measure_misc.py)
        const double us10k = knobs().stagger_us >= 0 ? (double)knobs().stagger_us : (scales_on_matrix ? 0.0 : p.dense ? 16.0 : 72.0);
        p.stagger_ticks = (int)(us10k * 100.0 * max_m / 10000.0);
    }
#ifdef GMS_PHASE_TIMING
    p.diag = g_diag;
#endif
    p.probe_scales = 0;
    p.probe_stats = nullptr;
    {
        void* dflag = nullptr;
        p.overflow_events = hipHostGetDevicePointer(&dflag, c->verdict, 0) == hipSuccess ? (uint32_t*)dflag + 2 : nullptr;
        p.ident_misses = p.overflow_events ? p.overflow_events + 2 : nullptr;
    }
    if (kpt && with_scale) {
        // the scales finer than 20 x 20 and the 14 x 14 one are probed (2, 3, 4); the measuring launches are left out of stream captures
        const bool measuring = force_probe < 0 && !capturing && (c->scale_launches++ & 15u) == 0u;
        // which scales are probed (every scale but 1, which the byte-matrix kernel evaluates first) and which of the two fine ones try
        // four-bit entries first: forced, or everything in a measuring launch, or what the last verdict said paid -- scale by scale
        const int all = 0x1D | (24 << 8);
        const int mask = force_probe >= 0 ? (force_probe != 0 ? 0x1D | (knobs().probe_nibble << 8) : 0) : (measuring ? all : c->use_probe);
        p.probe_scales = mask & 0x1D;
        p.probe_nibble = (mask >> 8) & 24 & (knobs().probe_nibble_set ? knobs().probe_nibble : 24);
        p.probe_stats = measuring ? (uint32_t*)c->probe_stats.p : nullptr;
    }
    if (kpt && with_scale && knobs().dense_on) {
        // scale hypotheses: scales 0..3 on the byte matrix, the last on the hashed path (two launches, one record per pair)
        p.partial = (uint32_t*)c->partial_ws.p;
        GMS_HIP(gms::launch_filter_scales(p, kpt, n_pairs, st));
        if (!capturing && p.probe_stats == nullptr && (c->dense_launches++ & 15u) == 0u)  // the spatial-order probe of this batch, for later launches (one verdict event: not beside a measuring launch)
            GMS_TRY(launch_verdict(c, st, [&](uint32_t* v) { return gms::launch_order_probe(p, v, v + 3, st); }));
        if (p.probe_stats != nullptr)
            GMS_TRY(launch_verdict(c, st, [&](uint32_t* v) { return gms::launch_probe_verdict(p.probe_stats, v + 1, st); }));
    } else if (kpt) {
        GMS_HIP(gms::launch_filter(p, kpt, n_pairs, st));
        // every sixteenth byte-matrix launch (and the first) is followed by the spatial-order probe of its batch, for later launches
        if (p.dense && !capturing && (c->dense_launches++ & 15u) == 0u)
            GMS_TRY(launch_verdict(c, st, [&](uint32_t* v) { return gms::launch_order_probe(p, v, v + 3, st); }));
    } else if (knobs().band_on) {
        // Large pairs on the LDS kernels, a slice of the batch at a time so that the per-pair workspace (lists, histogram,
        // masks) stays bounded: three bands of rows for the default flags, tiles of left cells with three launches per
        // scale hypothesis otherwise. Pairs they flag (a cell above 65 535 matches) fall through to the HBM-slab kernel (a
        // fixed crew of persistent workgroups), which looks at flagged pairs only.
        const bool plain = !with_rotation && !with_scale;
        for (int s0 = 0; s0 < n_pairs; s0 += (int)w.slice) {
            gms::FilterParams ps = p;
            ps.pairs = d_pairs + s0;
            ps.results = d_results + s0;
            ps.n_pairs = (n_pairs - s0 < (int)w.slice) ? n_pairs - s0 : (int)w.slice;
            const uint32_t* flags = nullptr;
            // streamed byte matrix: one workgroup per (pair, scale, grid type, band) with scale hypotheses -- and without them when the
            // slice has fewer pairs than the chip has CUs (four workgroups per pair then) --, else one workgroup per pair
            if (w.stream && (with_scale || ps.n_pairs < c->n_cus)) GMS_HIP(gms::launch_filter_stream(ps, w.mcap, c->band_ws.p, &flags, st));
            else if (w.stream) GMS_HIP(gms::launch_filter_stream_dense(ps, w.mcap, c->band_ws.p, &flags, st));
            else if (plain) GMS_HIP(gms::launch_filter_band(ps, w.mcap, c->band_ws.p, &flags, st));
            else GMS_HIP(gms::launch_filter_tiles(ps, w.mcap, c->band_ws.p, &flags, st));
            ps.pair_flags = flags;
            const int wg = ps.n_pairs < c->n_cus ? ps.n_pairs : c->n_cus;
            GMS_HIP(gms::launch_filter_big(ps, w.mcap, wg, (uint32_t*)c->big_ws.p, st));
        }
    } else {
        const int n_wg = n_pairs < c->n_cus ? n_pairs : c->n_cus;
        GMS_HIP(gms::launch_filter_big(p, w.mcap, n_wg, (uint32_t*)c->big_ws.p, st));
    }
    c->last_dealt = p.dealt;
    c->last_ident = p.ident;
    c->last_probe = p.probe_scales | (p.probe_scales ? p.probe_nibble << 8 : 0);
    c->last_kpt = kpt;
    c->last_stagger_ticks = p.stagger_ticks;
    // pair-table validation (ranges [match_off, match_off + m) must be disjoint: include/gms.h), behind the filter: offenders'
    // status becomes GMS_ERR_BAD_ARG. The first launch of a context and every sixteenth; never inside a stream capture.
    if (validate_pairs && n_pairs > 1 && !capturing && knobs().check_pairs != 0 && (knobs().check_pairs == 1 || (c->filter_launches & 15u) == 0u))
        GMS_HIP(gms::launch_check_pairs(d_pairs, n_pairs, d_results, (uint32_t*)c->probe_stats.p + 16 + (c->filter_launches & 7u), st));  // (a flag word of its own per launch: launches of one context may run on different streams)
    if (!capturing) ++c->filter_launches;
    if (uses_ws && !capturing) {
        GMS_HIP(hipEventRecord(c->ws_event, st));
        c->ws_stream = st;
        c->ws_pending = true;
    }
    return GMS_OK;
}

// ---- the host-pointer paths --------------------------------------------------------------------------------------------
// Staging block of a chunk, host (pinned) and device alike:  [ pairs (24 B each, 16-aligned) | matches (16 B each) ]
// and coming back:                                            [ results (16 B each) | out (16 B each) ]
size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// Host-side staging: copy_pool.h (CopyJob, pack_xy, CopyPool)
using gms::CopyJob;
using gms::CopyPool;
using gms::pack_xy;

}  // namespace

extern "C" {

const char* gms_version(void) { return "mi355-gms 0.2 (gfx950)"; }

int gms_last_hip_error(void) { return t_last_hip; }

const char* gms_error_string(int code)
{
    switch (code) {
    case GMS_OK: return "ok";
    case GMS_ERR_BAD_ARG: return "bad argument";
    case GMS_ERR_DOMAIN: return "input outside the domain on which the reference is defined";
    case GMS_ERR_HIP: return "HIP runtime error";
    case GMS_ERR_NO_DEVICE: return "no usable HIP device";
    case GMS_ERR_CAPACITY: return "too many matches per pair for this build";
    case GMS_ERR_IO: return "dataset file: cannot open, truncated, or not a GMSFRM01 file";
    case GMS_ERR_NO_MODEL: return "two-view stage: too few correspondences, or no essential matrix / pose found";
    case GMS_ERR_NOT_RESERVED: return "workspace not reserved for this shape (stream capture in progress)";
    default: return "unknown error";
    }
}

int gms_max_matches(void) { return gms::kBigMaxMatches; }

int gms_ctx_create(int device, gms_ctx** out_ctx)
{
    if (!out_ctx) return GMS_ERR_BAD_ARG;
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        t_last_hip = (int)e;
        return GMS_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return GMS_ERR_BAD_ARG;
    GMS_HIP(hipSetDevice(device));
    gms_ctx* c = new (std::nothrow) gms_ctx;
    if (!c) return GMS_ERR_BAD_ARG;
    c->device = device;
    const int rc = [c] {  // (what a failed step leaves behind is destroyed below)
        GMS_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        GMS_HIP(hipStreamCreateWithFlags(&c->lane[1].stream, hipStreamNonBlocking));
        GMS_HIP(hipStreamCreateWithFlags(&c->lane[2].stream, hipStreamNonBlocking));
        for (Lane& l : c->lane) {
            GMS_HIP(hipEventCreateWithFlags(&l.ev_res, hipEventDisableTiming));
            GMS_HIP(hipEventCreateWithFlags(&l.ev_out, hipEventDisableTiming));
        }
        GMS_HIP(hipEventCreateWithFlags(&c->ws_event, hipEventDisableTiming));
        GMS_HIP(hipEventCreateWithFlags(&c->verdict_event, hipEventDisableTiming));
        GMS_HIP(hipHostMalloc((void**)&c->verdict, 64, hipHostMallocDefault));
        c->verdict[0] = 0;
        c->verdict[1] = 0x1D | (16 << 8);
        c->verdict[2] = 0;
        c->verdict[3] = 0;
        c->verdict[4] = 0;
        GMS_HIP(c->probe_stats.reserve(128));  // [0..13] probe counters (probe_verdict_kernel), [16..23] flag words of the pair-table check
        GMS_HIP(hipMemset(c->probe_stats.p, 0, 128));
        GMS_HIP(c->side.reserve(2048 * sizeof(gms::SideRecord)));  // (tables of up to 2048 frames are built without growing it)
        GMS_HIP(gms::init_filter_kernels());
        GMS_HIP(gms::init_band_kernels());
        GMS_HIP(gms::init_stream_kernels());
        GMS_HIP(gms::init_big_kernels());
        return GMS_OK;
    }();
    if (rc != GMS_OK) {
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        if (c->lane[1].stream) (void)hipStreamDestroy(c->lane[1].stream);
        if (c->lane[2].stream) (void)hipStreamDestroy(c->lane[2].stream);
        for (Lane& l : c->lane) {
            if (l.ev_res) (void)hipEventDestroy(l.ev_res);
            if (l.ev_out) (void)hipEventDestroy(l.ev_out);
        }
        if (c->ws_event) (void)hipEventDestroy(c->ws_event);
        if (c->verdict_event) (void)hipEventDestroy(c->verdict_event);
        if (c->verdict) (void)hipHostFree(c->verdict);
        c->probe_stats.release();
        c->side.release();
        delete c;
        return rc;
    }
    c->stream = c->own_stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cus = prop.multiProcessorCount;
    *out_ctx = c;
    return GMS_OK;
}

int gms_ctx_destroy(gms_ctx* c)
{
    if (!c) return GMS_OK;
    {
        std::lock_guard<std::mutex> lock(c->mu);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->own_stream);
        (void)hipStreamSynchronize(c->lane[1].stream);
        (void)hipStreamSynchronize(c->lane[2].stream);
        if (c->ws_pending) (void)hipEventSynchronize(c->ws_event);
        DevBuf* bufs[] = {&c->aux, &c->big_ws, &c->band_ws, &c->partial_ws, &c->pose_ws, &c->probe_stats, &c->tab_kp, &c->tab_pts, &c->tab_small, &c->side};
        if (c->verdict) (void)hipHostFree(c->verdict);
        for (DevBuf* b : bufs) b->release();
        for (Lane& l : c->lane) {
            l.hin.release();
            l.hout.release();
            l.din.release();
            l.dout.release();
            (void)hipEventDestroy(l.ev_res);
            (void)hipEventDestroy(l.ev_out);
        }
        delete c->pool;
        c->pool = nullptr;
        (void)hipStreamDestroy(c->lane[1].stream);
        (void)hipStreamDestroy(c->lane[2].stream);
        (void)hipStreamDestroy(c->own_stream);
        (void)hipEventDestroy(c->ws_event);
        (void)hipEventDestroy(c->verdict_event);
    }
    delete c;
    return GMS_OK;
}

int gms_ctx_set_stream(gms_ctx* c, void* hip_stream)
{
    if (!c) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return GMS_OK;
}

int gms_ctx_synchronize(gms_ctx* c)
{
    if (!c) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    GMS_HIP(hipStreamSynchronize(c->stream));
    if (c->verdict_pending && hipEventQuery(c->verdict_event) == hipSuccess) {  // (recorded on another stream: maybe not yet)
        c->use_dealt = c->verdict[0] != 0u ? 1 : 0;
        c->use_probe = (int)c->verdict[1];
        c->use_ident = c->verdict[3] != 0u ? 1 : 0;
        c->verdict_pending = false;
    }
    return GMS_OK;
}

int gms_ctx_set_option(gms_ctx* c, int option, int value)
{
    if (!c || value < -1 || value > 1) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    switch (option) {
    case GMS_OPTION_DEAL: c->opt_deal = value; return GMS_OK;
    case GMS_OPTION_SCALE_PROBE: c->opt_probe = value; return GMS_OK;
    case GMS_OPTION_IDENT: c->opt_ident = value; return GMS_OK;
    default: return GMS_ERR_BAD_ARG;
    }
}

int gms_ctx_query(gms_ctx* c, int what, int64_t* value)
{
    if (!c || !value) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    switch (what) {
    case GMS_QUERY_LAST_DEALT: *value = c->last_dealt; return GMS_OK;
    case GMS_QUERY_LAST_SCALE_PROBE: *value = c->last_probe; return GMS_OK;
    case GMS_QUERY_LAST_KPT: *value = c->last_kpt; return GMS_OK;
    case GMS_QUERY_LAUNCHES: *value = (int64_t)c->filter_launches; return GMS_OK;
    case GMS_QUERY_CUS: *value = c->n_cus; return GMS_OK;
    case GMS_QUERY_PREFETCH_TYPE: *value = knobs().prefetch_type; return GMS_OK;
    case GMS_QUERY_PREFETCH_AHEAD: *value = knobs().prefetch_ahead > 0 ? knobs().prefetch_ahead : c->n_cus; return GMS_OK;
    case GMS_QUERY_STAGGER_TICKS: *value = c->last_stagger_ticks; return GMS_OK;
    case GMS_QUERY_LAST_IDENT: *value = c->last_ident; return GMS_OK;
    case GMS_QUERY_IDENT_MISSES: *value = (int64_t)((volatile uint32_t*)c->verdict)[4]; return GMS_OK;
    default: return GMS_ERR_BAD_ARG;
    }
}

int gms_ctx_reserve(gms_ctx* c, int n_pairs, int max_m, int with_rotation, int with_scale)
{
    if (!c || n_pairs < 0 || max_m < 0) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    WsNeed w;
    // with and without a caller-provided mask array, on the streamed and on the band / tile kernels (the library picks per launch): the largest
    GMS_TRY(plan_workspace(c, n_pairs, max_m, with_rotation != 0, with_scale != 0, true, true, &w));
    for (int variant = 1; variant < 4; ++variant) {
        WsNeed w2;
        GMS_TRY(plan_workspace(c, n_pairs, max_m, with_rotation != 0, with_scale != 0, (variant & 1) == 0, (variant & 2) == 0, &w2));
        w.band = std::max(w.band, w2.band);
    }
    GMS_TRY(grow_workspace(c, w, c->stream));
    return gms::grow_pose_ws(c, (size_t)max_m + 48, c->stream);  // gms_recover_pose_device on a pair of this size
}

// header (16) | points (8 each) | lcode, rcode (2 each) | scode (4 each) | 16 spare bytes (the staging copies read whole uint4s)
int64_t gms_frame_table_bytes(int64_t total_kp) { return total_kp < 0 ? 0 : gms::kTableHeaderBytes + total_kp * 16 + 16; }

int gms_normalize_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off,
                         const int32_t* d_wh, int n_frames, int64_t total_kp, float* d_pts)
{
    if (!c || n_frames < 0 || total_kp < 0) return GMS_ERR_BAD_ARG;
    if (total_kp == 0 || n_frames == 0) return GMS_OK;
    if (!d_kp || !d_frame_off || !d_wh || !d_pts) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    return build_frame_table(c, c->stream, d_kp, (int)sizeof(gms_keypoint), d_frame_off, d_wh, n_frames, total_kp, d_pts);
}

int gms_ctx_read_side_records(gms_ctx* c, void* dst, size_t dst_bytes, int* n_frames)
{
    static_assert(sizeof(gms::SideRecord) == GMS_SIDE_RECORD_BYTES, "the public size of a side record");
    if (!c || !n_frames || (dst_bytes && !dst)) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    GMS_HIP(hipStreamSynchronize(c->stream));
    *n_frames = c->side_stamp != 0 ? c->side_frames : 0;
    const size_t bytes = std::min(dst_bytes, (size_t)*n_frames * sizeof(gms::SideRecord));
    if (bytes) GMS_HIP(hipMemcpy(dst, c->side.p, bytes, hipMemcpyDeviceToHost));
    return GMS_OK;
}

int gms_filter_device(gms_ctx* c, const float* d_pts, const int64_t* d_frame_off, int n_frames,
                      const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_matches,
                      int with_rotation, int with_scale, double threshold_factor,
                      gms_dmatch* d_out, gms_pair_result* d_results, uint8_t* d_mask)
{
    if (!c) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    return filter_launch(c, c->stream, d_pts, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_matches, with_rotation,
                         with_scale, threshold_factor, d_out, d_results, d_mask);
}

int gms_match_ctx(gms_ctx* c, const gms_keypoint* kp1, int n1, int w1, int h1,
                  const gms_keypoint* kp2, int n2, int w2, int h2, const gms_dmatch* matches, int m,
                  int with_rotation, int with_scale, double threshold_factor,
                  gms_dmatch* out, int* n_out, gms_pair_result* result)
{
    if (n_out) *n_out = 0;
    if (result) *result = gms_pair_result{0, -1, -1, GMS_OK};
    if (!c || !n_out) return GMS_ERR_BAD_ARG;
    if (n1 < 0 || n2 < 0 || m < 0 || w1 <= 0 || h1 <= 0 || w2 <= 0 || h2 <= 0) return GMS_ERR_BAD_ARG;
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2) || (m > 0 && (!matches || !out))) return GMS_ERR_BAD_ARG;
    if (m > gms_max_matches()) return GMS_ERR_CAPACITY;

    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    Lane& L = c->lane[0];
    // Everything the call sends travels as ONE block through pinned memory (one copy-engine transfer, no bounce through the
    // runtime's pageable staging):  header (64 B) | matches (16 B each) | (pt.x, pt.y) of both frames (8 B each)
    struct alignas(8) CallHeader {
        int64_t foff[3];
        int32_t wh[4];
        gms_pair pair;
    };
    static_assert(sizeof(CallHeader) == 64 && offsetof(CallHeader, wh) == 24 && offsetof(CallHeader, pair) == 40, "header layout");
    const size_t nkp = (size_t)n1 + (size_t)n2;
    const size_t off_m = sizeof(CallHeader), off_xy = off_m + (size_t)m * sizeof(gms_dmatch);
    const size_t in_bytes = off_xy + nkp * 8;
    const size_t out_bytes = sizeof(gms_pair_result) + (size_t)m * sizeof(gms_dmatch);  // result | out
    GMS_HIP(L.hin.reserve(in_bytes));
    GMS_HIP(L.hout.reserve(out_bytes));
    // (a DevBuf that grows frees its old block: earlier work of this lane is complete -- every host-pointer call ends
    // synchronised -- unless the caller switched streams in between, which the synchronize below covers)
    if (in_bytes > L.din.cap || out_bytes > L.dout.cap || (size_t)gms_frame_table_bytes((int64_t)nkp) > c->tab_pts.cap) GMS_HIP(hipDeviceSynchronize());
    GMS_HIP(L.din.reserve(in_bytes));
    GMS_HIP(L.dout.reserve(out_bytes));
    GMS_HIP(c->tab_pts.reserve((size_t)gms_frame_table_bytes((int64_t)nkp)));
    char* hin = (char*)L.hin.p;
    const CallHeader hdr = {{0, n1, (int64_t)n1 + n2}, {w1, h1, w2, h2}, {0, 1, m, 0, 0}};
    std::memcpy(hin, &hdr, sizeof hdr);
    if (m) std::memcpy(hin + off_m, matches, (size_t)m * sizeof(gms_dmatch));
    pack_xy(kp1, (size_t)n1, (float*)(hin + off_xy));
    pack_xy(kp2, (size_t)n2, (float*)(hin + off_xy) + 2 * (size_t)n1);
    // Small calls (up to 16k matches) skip the copy engines altogether: the kernels read the pinned block and write the pinned
    // result block directly over PCIe (every input byte is read once -- the records stay in registers -- and every output byte
    // written once), which saves the fixed cost of two DMA operations. Larger calls stage through device memory.
    const bool zero_copy = m <= 16384;
    const char* din = (const char*)L.din.p;
    char* dout = (char*)L.dout.p;
    if (zero_copy) {
        void *dev_in = nullptr, *dev_out = nullptr;
        GMS_HIP(hipHostGetDevicePointer(&dev_in, L.hin.p, 0));
        GMS_HIP(hipHostGetDevicePointer(&dev_out, L.hout.p, 0));
        din = (const char*)dev_in;
        dout = (char*)dev_out;
    } else {
        GMS_HIP(hipMemcpyAsync(L.din.p, hin, in_bytes, hipMemcpyHostToDevice, st));
    }
    const int64_t* d_foff = (const int64_t*)din;
    const int32_t* d_wh = (const int32_t*)(din + offsetof(CallHeader, wh));
    const gms_pair* d_pair = (const gms_pair*)(din + offsetof(CallHeader, pair));
    gms_pair_result* d_res = (gms_pair_result*)dout;
    gms_dmatch* d_out = (gms_dmatch*)(dout + sizeof(gms_pair_result));
    if (nkp) GMS_TRY(build_frame_table(c, st, din + off_xy, 8, d_foff, d_wh, 2, (int64_t)nkp, (float*)c->tab_pts.p));
    GMS_TRY(filter_launch(c, st, (const float*)c->tab_pts.p, d_foff, 2, d_pair, 1, m, (const gms_dmatch*)(din + off_m),
                          with_rotation, with_scale, threshold_factor, d_out, d_res, nullptr));
    // Staged calls fetch the result record first and then exactly the survivors.
    if (!zero_copy) GMS_HIP(hipMemcpyAsync(L.hout.p, L.dout.p, sizeof(gms_pair_result), hipMemcpyDeviceToHost, st));
    GMS_HIP(hipStreamSynchronize(st));
    const gms_pair_result r = *(const gms_pair_result*)L.hout.p;
    if (result) *result = r;
    if (r.status != GMS_OK) return r.status;
    if (r.n_inliers < 0 || r.n_inliers > m) return GMS_ERR_HIP;  // (cannot happen: the kernels count what they wrote)
    const size_t keep_bytes = (size_t)r.n_inliers * sizeof(gms_dmatch);
    if (!zero_copy && keep_bytes) {
        GMS_HIP(hipMemcpyAsync((char*)L.hout.p + sizeof(gms_pair_result), d_out, keep_bytes, hipMemcpyDeviceToHost, st));
        GMS_HIP(hipStreamSynchronize(st));
    }
    // only the survivors reach the caller's array: what lies beyond *n_out is left untouched
    if (keep_bytes) std::memcpy(out, (const char*)L.hout.p + sizeof(gms_pair_result), keep_bytes);
    *n_out = r.n_inliers;
    return GMS_OK;
}

int gms_match(const gms_keypoint* kp1, int n1, int w1, int h1, const gms_keypoint* kp2, int n2, int w2, int h2,
              const gms_dmatch* matches, int m, int with_rotation, int with_scale, double threshold_factor,
              gms_dmatch* out, int* n_out)
{
    static std::mutex mu;
    static gms_ctx* def = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!def) {
            int rc = gms_ctx_create(0, &def);
            if (rc != GMS_OK) {
                if (n_out) *n_out = 0;
                return rc;
            }
        }
    }
    return gms_match_ctx(def, kp1, n1, w1, h1, kp2, n2, w2, h2, matches, m, with_rotation, with_scale,
                         threshold_factor, out, n_out, nullptr);
}

int gms_filter_host_batch(gms_ctx* c, const gms_keypoint* kp, const int64_t* frame_off, const int32_t* wh, int n_frames,
                          const gms_pair* pairs, int n_pairs, const gms_dmatch* matches,
                          int with_rotation, int with_scale, double threshold_factor,
                          gms_dmatch* out, gms_pair_result* results)
{
    if (!c || n_frames < 0 || n_pairs < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!frame_off || !wh || !pairs || !results || n_frames == 0) return GMS_ERR_BAD_ARG;
    // the frame table starts at keypoint 0 and never decreases (whether kp holds frame_off[n_frames] records is the caller's word)
    if (frame_off[0] != 0 || !frame_offsets_ascend(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    const int64_t total_kp = frame_off[n_frames];
    if (total_kp < 0 || (total_kp > 0 && !kp)) return GMS_ERR_BAD_ARG;
    int max_m = 0;
    bool in_order = true;
    for (int i = 0; i < n_pairs; ++i) {
        if (pairs[i].m < 0 || pairs[i].match_off < 0) return GMS_ERR_BAD_ARG;
        if (pairs[i].m > gms_max_matches()) return GMS_ERR_CAPACITY;
        max_m = std::max(max_m, pairs[i].m);
        if (i + 1 < n_pairs && pairs[i].match_off + pairs[i].m > pairs[i + 1].match_off) in_order = false;
    }
    if (max_m > 0 && (!matches || !out)) return GMS_ERR_BAD_ARG;
    if (!in_order) {  // the pairs' match ranges must be disjoint (include/gms.h): sort the non-empty ones by start and look at the neighbours
        std::vector<std::pair<int64_t, int64_t>> r;
        r.reserve((size_t)n_pairs);
        for (int i = 0; i < n_pairs; ++i)
            if (pairs[i].m > 0) r.emplace_back(pairs[i].match_off, pairs[i].match_off + pairs[i].m);
        std::sort(r.begin(), r.end());
        for (size_t i = 1; i < r.size(); ++i)
            if (r[i - 1].second > r[i].first) return GMS_ERR_BAD_ARG;
    }

    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    c->lane[0].stream = c->own_stream;
    // everything earlier on the context's streams and workspaces is complete before buffers are regrown and reused
    GMS_HIP(hipStreamSynchronize(c->stream));
    GMS_HIP(hipStreamSynchronize(c->lane[0].stream));
    GMS_HIP(hipStreamSynchronize(c->lane[1].stream));
    GMS_HIP(hipStreamSynchronize(c->lane[2].stream));

    // ---- chunks: runs of consecutive pairs of at most kChunkMatches matches (a pair larger than that is a chunk of its own)
    const size_t kChunkMatches = (size_t)2 << 20;  // 32 MB of match records per chunk
    const int kChunkPairs = 8192;
    struct Chunk { int first, count; size_t matches; int max_m; };
    std::vector<Chunk> chunks;
    for (int i = 0; i < n_pairs;) {
        Chunk ch{i, 0, 0, 0};
        while (i < n_pairs && ch.count < kChunkPairs && (ch.count == 0 || ch.matches + (size_t)pairs[i].m <= kChunkMatches)) {
            ch.matches += (size_t)pairs[i].m;
            ch.max_m = std::max(ch.max_m, pairs[i].m);
            ++ch.count;
            ++i;
        }
        chunks.push_back(ch);
    }
    size_t cap_m = 0, cap_p = 0;
    for (const Chunk& ch : chunks) {
        cap_m = std::max(cap_m, ch.matches);
        cap_p = std::max(cap_p, (size_t)ch.count);
    }
    // a lane's blocks, host (pinned) and device alike:   in  [ pairs (24 B each, 16-aligned) | matches (16 B each) ]
    //                                                    out [ results (16 B each) | survivor total (16 B) | out (16 B each) ]
    // and, once a chunk is filtered, its survivors packed back to back over the chunk's own match records in the device's in-block
    const size_t in_pairs_bytes = align16(cap_p * sizeof(gms_pair));
    const size_t in_bytes = std::max(in_pairs_bytes + cap_m * sizeof(gms_dmatch), (size_t)total_kp * 8);
    const size_t out_res_bytes = cap_p * sizeof(gms_pair_result) + 16;
    const size_t out_bytes = out_res_bytes + cap_m * sizeof(gms_dmatch);
    for (Lane& L : c->lane) {
        GMS_HIP(L.hin.reserve(&L == &c->lane[0] ? in_bytes : in_pairs_bytes + cap_m * sizeof(gms_dmatch)));
        GMS_HIP(L.hout.reserve(out_bytes));
        GMS_HIP(L.din.reserve(in_pairs_bytes + cap_m * sizeof(gms_dmatch)));
        GMS_HIP(L.dout.reserve(out_bytes));
    }
    {   // the workspaces for the largest chunk, once, so that no launch below has to grow them mid-pipeline
        WsNeed w;
        GMS_TRY(plan_workspace(c, (int)cap_p, max_m, with_rotation != 0, with_scale != 0, true, true, &w));
        WsNeed w2;
        GMS_TRY(plan_workspace(c, (int)cap_p, max_m, with_rotation != 0, with_scale != 0, true, false, &w2));
        w.band = std::max(w.band, w2.band);
        GMS_TRY(grow_workspace(c, w, c->lane[0].stream));
    }
    if (!c->pool) c->pool = new (std::nothrow) CopyPool;
    if (!c->pool) return GMS_ERR_BAD_ARG;
    CopyPool& pool = *c->pool;
    std::vector<CopyJob> jobs;

    // ---- the frame table: (pt.x, pt.y) of every keypoint packed into pinned memory by the pool, one transfer, normalizePoints on the GPU
    const size_t small_bytes = align16((size_t)(n_frames + 1) * 8) + (size_t)n_frames * 8;
    GMS_HIP(c->tab_kp.reserve((size_t)total_kp * 8));
    GMS_HIP(c->tab_pts.reserve((size_t)gms_frame_table_bytes(total_kp)));
    GMS_HIP(c->tab_small.reserve(small_bytes));
    {
        hipStream_t st = c->lane[0].stream;
        GMS_HIP(hipMemcpyAsync(c->tab_small.p, frame_off, (size_t)(n_frames + 1) * 8, hipMemcpyHostToDevice, st));
        GMS_HIP(hipMemcpyAsync((char*)c->tab_small.p + align16((size_t)(n_frames + 1) * 8), wh, (size_t)n_frames * 8,
                               hipMemcpyHostToDevice, st));
        if (total_kp) {
            jobs.push_back(CopyJob{c->lane[0].hin.p, kp, (size_t)total_kp * 8, 1});
            pool.run(jobs);
            jobs.clear();
            GMS_HIP(hipMemcpyAsync(c->tab_kp.p, c->lane[0].hin.p, (size_t)total_kp * 8, hipMemcpyHostToDevice, st));
            GMS_TRY(build_frame_table(c, st, c->tab_kp.p, 8, (const int64_t*)c->tab_small.p,
                                      (const int32_t*)((char*)c->tab_small.p + align16((size_t)(n_frames + 1) * 8)),
                                      n_frames, total_kp, (float*)c->tab_pts.p));
        }
        GMS_HIP(hipStreamSynchronize(st));  // (frame_off / wh are the caller's pageable memory; lane 0's pinned block is reused below)
    }
    const int64_t* d_foff = (const int64_t*)c->tab_small.p;

    // ---- the pipeline, three chunks deep. Chunk k rides lane k % 3:
    //        iteration k     the pool copies chunk k into the lane's pinned block (and chunk k - 2's survivors out of its lane's:
    //                        one batch of jobs), then: upload, filter, pack the survivors back to back on the device
    //                        (compact_survivors_kernel), download the result records + the survivor total
    //        iteration k + 1 the records are on the host: download exactly the survivors (K records, not the m slots)
    //        iteration k + 2 the survivors are on the host: copy them to the caller's array at the pairs' offsets
    //      so that the copy engines (both directions) and the GPU work on chunks k - 1 and k while the host threads stage k + 1.
    auto in_matches = [&](Lane& L) { return (gms_dmatch*)((char*)L.din.p + in_pairs_bytes); };
    const size_t n_chunks = chunks.size();
    for (size_t k = 0; k < n_chunks + 2; ++k) {
        jobs.clear();
        if (k >= 2) {  // chunk k - 2: its survivors are (about to be) in the lane's pinned block
            const Chunk& ch = chunks[k - 2];
            Lane& L = c->lane[(k - 2) % 3];
            GMS_HIP(hipEventSynchronize(L.ev_out));
            const gms_pair_result* res = (const gms_pair_result*)L.hout.p;
            const gms_dmatch* o = (const gms_dmatch*)((const char*)L.hout.p + out_res_bytes);
            std::memcpy(results + ch.first, res, (size_t)ch.count * sizeof(gms_pair_result));
            size_t at = 0;
            for (int i = 0; i < ch.count; ++i) {
                if (res[i].status != GMS_OK || res[i].n_inliers <= 0) continue;
                jobs.push_back(CopyJob{out + pairs[ch.first + i].match_off, o + at, (size_t)res[i].n_inliers * sizeof(gms_dmatch), 0});
                at += (size_t)res[i].n_inliers;
            }
        }
        if (k < n_chunks) {  // chunk k: pair table rebased to the chunk, match records gathered
            const Chunk& ch = chunks[k];
            Lane& L = c->lane[k % 3];
            gms_pair* hp = (gms_pair*)L.hin.p;
            gms_dmatch* hm = (gms_dmatch*)((char*)L.hin.p + in_pairs_bytes);
            size_t local = 0;
            for (int i = 0; i < ch.count; ++i) {
                const gms_pair& pr = pairs[ch.first + i];
                hp[i] = gms_pair{pr.frame_a, pr.frame_b, pr.m, 0, (int64_t)local};
                if (pr.m) jobs.push_back(CopyJob{hm + local, matches + pr.match_off, (size_t)pr.m * sizeof(gms_dmatch), 0});
                local += (size_t)pr.m;
            }
        }
        pool.run(jobs);
        if (k < n_chunks) {
            const Chunk& ch = chunks[k];
            Lane& L = c->lane[k % 3];
            gms_pair_result* d_res = (gms_pair_result*)L.dout.p;
            int64_t* d_total = (int64_t*)((char*)L.dout.p + out_res_bytes - 16);
            gms_dmatch* d_out = (gms_dmatch*)((char*)L.dout.p + out_res_bytes);
            GMS_HIP(hipMemcpyAsync(L.din.p, L.hin.p, in_pairs_bytes + ch.matches * sizeof(gms_dmatch), hipMemcpyHostToDevice, L.stream));
            GMS_TRY(filter_launch(c, L.stream, (const float*)c->tab_pts.p, d_foff, n_frames, (const gms_pair*)L.din.p, ch.count, ch.max_m,
                                  in_matches(L), with_rotation, with_scale, threshold_factor, d_out, d_res, nullptr,
                                  false /* the ranges were validated on the host above; the device check's scratch word is per context, not per lane */));
            GMS_HIP(gms::launch_compact_survivors((const gms_pair*)L.din.p, d_res, ch.count, d_out, in_matches(L), d_total, L.stream));
            GMS_HIP(hipMemcpyAsync(L.hout.p, L.dout.p, out_res_bytes, hipMemcpyDeviceToHost, L.stream));
            GMS_HIP(hipEventRecord(L.ev_res, L.stream));
        }
        if (k >= 1 && k - 1 < n_chunks) {  // chunk k - 1: its records are (about to be) on the host; fetch its survivors
            const Chunk& ch = chunks[k - 1];
            Lane& L = c->lane[(k - 1) % 3];
            GMS_HIP(hipEventSynchronize(L.ev_res));
            const int64_t kept = *(const int64_t*)((const char*)L.hout.p + out_res_bytes - 16);
            if (kept < 0 || (size_t)kept > ch.matches) return GMS_ERR_HIP;  // (cannot happen: the kernels count what they wrote)
            if (kept)
                GMS_HIP(hipMemcpyAsync((char*)L.hout.p + out_res_bytes, in_matches(L), (size_t)kept * sizeof(gms_dmatch), hipMemcpyDeviceToHost, L.stream));
            GMS_HIP(hipEventRecord(L.ev_out, L.stream));
        }
    }
    return GMS_OK;
}

}  // extern "C"
