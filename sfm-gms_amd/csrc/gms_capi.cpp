// gms_capi.cpp -- the C ABI declared in include/gms.h, on top of the HIP kernels.
//
// Host side of the drop-in for cv::xfeatures2d::matchGMS (FeatureMatchUtil.cpp:69,
// DisparityUtil.cpp:149,299 of the reference). There is deliberately no CPU implementation of the
// filter in this library: without a working HIP device every compute entry point returns an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "block_layout.h"
#include "copy_pool.h"
#include "gms.h"
#include "gms_kernels.h"
#include "logos_batch.h"
#include "logos_dict_core.h"
#include "portrait_core.h"
#include "stereo_bm_core.h"
#include "sfm_ba_core.h"
#include "sfm_register_core.h"
#include "stereo_sgm_core.h"
#include "twoview_core.h"
#include "rectify_core.h"
#include "dense_fuse_core.h"
#include "sfm_pair_pose_core.h"
#include "speckle_core.h"
#include "warp_core.h"
#include "calib_core.h"

static_assert(sizeof(gms_keypoint) == 28, "gms_keypoint must match cv::KeyPoint (stride 0x1c)");
static_assert(sizeof(gms_dmatch) == 16, "gms_dmatch must match cv::DMatch (stride 0x10)");
static_assert(sizeof(gms_pair) == 24, "gms_pair layout");
static_assert(sizeof(gms_pair_result) == 16, "gms_pair_result layout");
static_assert(sizeof(gms_two_view) == 232 && sizeof(gms_camera) == 72, "two-view records");

static thread_local int t_last_hip = 0;
// for the other translation units of the library (logos_kernels.hip): what gms_last_hip_error() reports
namespace gms {
void record_hip_error(int e) { t_last_hip = e; }
}
#ifdef GMS_PHASE_TIMING
static unsigned long long* g_diag = nullptr;
extern "C" int gms_diag_set_buffer(void* d_buf) { g_diag = (unsigned long long*)d_buf; return 0; }
#endif

#define GMS_HIP(call)                         \
    do {                                      \
        hipError_t e_ = (call);               \
        if (e_ != hipSuccess) {               \
            t_last_hip = (int)e_;             \
            return GMS_ERR_HIP;               \
        }                                     \
    } while (0)
#define GMS_TRY(call)                \
    do {                             \
        const int rc_ = (call);      \
        if (rc_ != GMS_OK) return rc_; \
    } while (0)

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

inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// A buffer that only grows: a request above the capacity frees the block and allocates one a quarter larger (at least kMin bytes).
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*), size_t kMin>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes < kMin ? kMin : bytes + bytes / 4;
        const hipError_t e = Alloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)Free(p);
        p = nullptr;
        cap = 0;
    }
};
using DevBuf = GrowBuf<device_alloc, hipFree, 4096>;
// page-locked host memory: what the copy engines read and write without a bounce through the runtime's own staging
using PinBuf = GrowBuf<pinned_alloc, hipHostFree, 65536>;

// What one gms_filter_device call needs beyond its arguments.
struct WsNeed {
    size_t partial = 0, big = 0, band = 0;
    size_t slice = 0, per_pair = 0;  // large pairs: pairs per slice of the batch, workspace bytes per pair
    int kpt = 0, mcap = 0;
    bool stream = false;             // large pairs up to 65 536 matches: the streamed byte-matrix kernels
};

}  // namespace

// One lane of the host-pointer paths: pinned staging in both directions, the device arenas they mirror, a stream.
struct Lane {
    hipStream_t stream = nullptr;
    PinBuf hin, hout;
    DevBuf din, dout;
    hipEvent_t ev_res = nullptr, ev_out = nullptr;  // gms_filter_host_batch: a chunk's results are on the host / its survivors are
};

struct gms_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;  // every entry point that touches the context's buffers holds it
    DevBuf aux, big_ws, band_ws, partial_ws, pose_ws;
    // What recent launches saw, as words in pinned host memory that small kernels write now and then and the host reads without
    // waiting: verdict[0] "recent batches came in spatial order" (order_probe_kernel; picks the byte-matrix kernel's instantiation),
    // verdict[1] "probing scale hypotheses pays" (probe_verdict_kernel, below)
    uint32_t* verdict = nullptr;
    unsigned dense_launches = 0;
    // verdict[0] and verdict[1] are never read while a kernel may be writing them: a verdict kernel is followed by an event, and the
    // first launch (or gms_ctx_synchronize) that finds the event complete ADOPTS the words; launches run on the adopted values in
    // between. verdict[2] (below) is different: a counter the streamed kernels add to, read without waiting -- it only steers which of
    // two bit-identical paths the next launches of large pairs take (and with it which workspace such a launch asks for).
    // last_* = what the most recent launch ran with (gms_ctx_query).
    int use_dealt = 0, use_probe = 0x1D | (16 << 8), last_dealt = 0, last_probe = 0, last_kpt = 0, last_stagger_ticks = 0;
    hipEvent_t verdict_event = nullptr;
    bool verdict_pending = false;
    unsigned filter_launches = 0;  // every launch of the context (pair-table validation every sixteenth)
    // verdict[2] counts the pairs the streamed byte-matrix kernels had to hand on (an entry above 255, a cell above 65 535): when it has
    // moved since the last look, the next 64 launches of large pairs take the 16-bit band / tile kernels instead, then the streamed ones get another try
    uint32_t overflow_seen = 0;
    int stream_penalty = 0;
    int opt_deal = -1, opt_probe = -1, opt_ident = -1;  // gms_ctx_set_option: -1 = the library's own choice (and the environment switches), 0 / 1 = forced
    // Identity-query pairs (match k of a pair is query k, one match per keypoint of frame A): the byte-matrix kernel's IDENT instantiation
    // works from per-frame side records (gms_kernels.h) that every table build of this context fills in `side`; side_stamp says
    // whether the latest build left any (the stamp that ties them to their table is worked out and compared on the device).
    // verdict[3]: what the spatial-order probe saw of its sampled pairs (adopted with verdict[0]); verdict[4]: a counter of the pairs
    // an IDENT launch had to filter with the generic body, read without waiting like verdict[2] -- when it has moved, IDENT is off
    // until a later probe says otherwise.
    DevBuf side;
    int side_frames = 0;
    uint64_t side_stamp = 0;
    int use_ident = 0, last_ident = 0;
    uint32_t ident_misses_seen = 0;
    // Scale hypotheses: the kernels can bound a scale's inlier count before evaluating it (gms_kernel_scales.hip, PROBE) and skip the
    // scale when it cannot win -- a gain when at least half of the probes let a scale skip, a loss otherwise. The kernels count
    // both in probe_stats (device); every sixteenth launch with scale hypotheses probes whatever the verdict and is followed by a
    // one-thread kernel that turns the counts into verdict[1], which the launches in between follow.
    DevBuf probe_stats;
    unsigned scale_launches = 0;
    // the workspaces above are shared by every launch of the context: the last launch that used them, and where
    hipEvent_t ws_event = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    Lane lane[3];     // one-shot calls use lane 0 (on the context's stream); gms_filter_host_batch rotates through all three
    gms::CopyPool* pool = nullptr;  // gms_filter_host_batch: the threads that stage its chunks (created with the first call)
    DevBuf tab_kp, tab_pts, tab_small;  // gms_filter_host_batch: the call's frame table
    int n_cus = 256;  // multiProcessorCount of the device
};

namespace {

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
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return GMS_ERR_NOT_RESERVED;
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

// The scratch of gms_recover_pose_device (vote bytes + counters): grown like the filter's workspaces -- never inside a stream
// capture, and only after everything that may still use the old block has finished.
int grow_pose_ws(gms_ctx* c, size_t bytes, hipStream_t st)
{
    if (bytes <= c->pose_ws.cap) return GMS_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return GMS_ERR_NOT_RESERVED;
    GMS_HIP(hipStreamSynchronize(st));
    GMS_HIP(hipDeviceSynchronize());  // (an earlier call may have run on another stream of the caller's)
    GMS_HIP(c->pose_ws.reserve(bytes));
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
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
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
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
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
        if (!capturing && p.probe_stats == nullptr && (c->dense_launches++ & 15u) == 0u) {  // the spatial-order probe of this batch, for later launches (one verdict event: not beside a measuring launch)
            void* dflag = nullptr;
            GMS_HIP(hipHostGetDevicePointer(&dflag, c->verdict, 0));
            GMS_HIP(gms::launch_order_probe(p, (uint32_t*)dflag, (uint32_t*)dflag + 3, st));
            GMS_HIP(hipEventRecord(c->verdict_event, st));
            c->verdict_pending = true;
        }
        if (p.probe_stats != nullptr) {
            void* dflag = nullptr;
            GMS_HIP(hipHostGetDevicePointer(&dflag, c->verdict, 0));
            GMS_HIP(gms::launch_probe_verdict(p.probe_stats, (uint32_t*)dflag + 1, st));
            GMS_HIP(hipEventRecord(c->verdict_event, st));
            c->verdict_pending = true;
        }
    } else if (kpt) {
        GMS_HIP(gms::launch_filter(p, kpt, n_pairs, st));
        // every sixteenth byte-matrix launch (and the first) is followed by the spatial-order probe of its batch, for later launches
        if (p.dense && !capturing && (c->dense_launches++ & 15u) == 0u) {
            void* dflag = nullptr;
            GMS_HIP(hipHostGetDevicePointer(&dflag, c->verdict, 0));
            GMS_HIP(gms::launch_order_probe(p, (uint32_t*)dflag, (uint32_t*)dflag + 3, st));
            GMS_HIP(hipEventRecord(c->verdict_event, st));
            c->verdict_pending = true;
        }
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

bool desc_kind_ok(int kind) { return kind == GMS_DESC_HAMMING256 || kind == GMS_DESC_L2_F32X128; }
size_t desc_row_bytes(int kind) { return kind == GMS_DESC_HAMMING256 ? 32 : 512; }

// The body of an entry point that is one launch on the context's stream: launch() -> hipError_t, run with the context locked and
// its device selected.
template <class Launch>
int on_ctx(gms_ctx* c, Launch&& launch)
{
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    GMS_HIP(launch());
    return GMS_OK;
}

// ---- the one-shot host entry points ------------------------------------------------------------------------------------
// Such a call keeps everything it needs in one device block (gms::BlockLayout says where), allocated on the current device and
// freed when the call returns. DevBlock owns the block and the call's sticky HIP error: once a step has failed the later ones
// are skipped, and the block is freed only after the stream has been waited for -- also on failure and on an early return, so
// that nothing in flight still uses it.
class DevBlock {
public:
    DevBlock(const gms::BlockLayout& layout, hipStream_t stream) : st_(stream) { err_ = hipMalloc(&p_, layout.total()); }
    ~DevBlock() { release(); }
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;

    template <class T = void>
    T* at(size_t offset) const { return reinterpret_cast<T*>(static_cast<char*>(p_) + offset); }
    bool ok() const { return err_ == hipSuccess; }
    // the steps: launch(stream) -> hipError_t, and copies between host memory and a region
    template <class Launch>
    void run(Launch&& launch)
    {
        if (!ok()) return;
        busy_ = true;
        err_ = launch(st_);
    }
    void in(size_t offset, const void* src, size_t bytes) { run([&](hipStream_t st) { return hipMemcpyAsync(at(offset), src, bytes, hipMemcpyHostToDevice, st); }); }
    void out(void* dst, size_t offset, size_t bytes) { run([&](hipStream_t st) { return hipMemcpyAsync(dst, at(offset), bytes, hipMemcpyDeviceToHost, st); }); }
    // for a call that reads what it copied out before it goes on: wait for the steps so far / copy out and wait, in one blocking copy
    void sync() { wait([&] { return hipStreamSynchronize(st_); }); }
    void out_now(void* dst, size_t offset, size_t bytes) { wait([&] { return hipMemcpy(dst, at(offset), bytes, hipMemcpyDeviceToHost); }); }
    // The end of the call: waits, frees the block, records the error for gms_last_hip_error() -> GMS_OK or GMS_ERR_HIP.
    int finish()
    {
        release();
        GMS_HIP(err_);
        return GMS_OK;
    }

private:
    template <class Wait>
    void wait(Wait&& w)
    {
        if (ok()) err_ = w();
        busy_ = !ok();
    }
    void release()
    {
        if (!p_) return;
        if (busy_) {  // (also behind a failed step: earlier ones may still be running)
            const hipError_t e = hipStreamSynchronize(st_);
            if (ok()) err_ = e;
        }
        (void)hipFree(p_);
        p_ = nullptr;
    }
    void* p_ = nullptr;
    hipStream_t st_;
    hipError_t err_;
    bool busy_ = false;  // steps were enqueued since the stream was last waited for
};

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
    return grow_pose_ws(c, (size_t)max_m + 48, c->stream);  // gms_recover_pose_device on a pair of this size
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
    if (frame_off[0] != 0) return GMS_ERR_BAD_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
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
    if (reinterpret_cast<uintptr_t>(d_ws) & 255u) return GMS_ERR_BAD_ARG;
    // the workspace's size fixes how many matcher rows it holds (total_backward_rows of gms_bf_select_workspace_bytes)
    const size_t fixed = gms::bf_select_ws_bytes(n_pairs, max_rows, 0);
    if (ws_bytes < fixed) return GMS_ERR_BAD_ARG;
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
    for (int f = 0; f < n_frames; f++) {
        if (frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
    }
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

// ---- StereoBM (stereo_bm_kernels.hip) ----------------------------------------------------------------------------
static const gms_stereo_bm_params& sbm_params(const gms_stereo_bm_params* p)
{
    static const gms_stereo_bm_params ref = GMS_STEREO_BM_PARAMS_REFERENCE;
    return p ? *p : ref;
}

size_t gms_stereo_bm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_bm_params* params)
{
    if (n_pairs < 0 || n_pairs > 65535 || !sbm::params_ok(sbm_params(params), width, height)) return 0;
    return gms::stereo_bm_ws_bytes(n_pairs, width, height);
}

int gms_stereo_bm_device(gms_ctx* c, const gms_stereo_bm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                         int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost)
{
    const gms_stereo_bm_params& p = sbm_params(params);
    if (!c || n_pairs < 0 || n_pairs > 65535 || !sbm::params_ok(p, width, height) || pitch < width) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_left || !d_right || !d_ws || !d_disp16) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_disp16) & 1u) ||
        (reinterpret_cast<uintptr_t>(d_cost) & 3u) || ws_bytes < gms::stereo_bm_ws_bytes(n_pairs, width, height))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_bm(p, d_left, d_right, n_pairs, width, height, pitch, d_ws, d_disp16, d_cost, c->stream); });
}

int gms_stereo_bm_normalize_device(gms_ctx* c, const int16_t* d_disp16, int n, int width, int height, uint8_t* d_out8)
{
    if (!c || n < 0 || width <= 0 || height <= 0) return GMS_ERR_BAD_ARG;
    if (n == 0) return GMS_OK;
    if (!d_disp16 || !d_out8 || (reinterpret_cast<uintptr_t>(d_disp16) & 1u)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_bm_normalize(d_disp16, n, width, height, d_out8, c->stream); });
}

int gms_stereo_bm(const gms_stereo_bm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                  int16_t* disp16, int32_t* cost, uint8_t* disp8)
{
    const gms_stereo_bm_params& p = sbm_params(params);
    if (!sbm::params_ok(p, width, height) || pitch < width || !left || !right) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height, img = (size_t)pitch * (size_t)(height - 1) + (size_t)width;
    gms::BlockLayout lay;  // the images keep the caller's pitch
    const size_t o_l = lay.add(img), o_r = lay.add(img), o_ws = lay.add(gms::stereo_bm_ws_bytes(1, width, height));
    const size_t o_d = lay.add(2 * px), o_c = lay.add(4 * px), o_8 = lay.add(px);
    DevBlock blk(lay, nullptr);
    blk.in(o_l, left, img);
    blk.in(o_r, right, img);
    blk.run([&](hipStream_t st) {
        return gms::launch_stereo_bm(p, blk.at<uint8_t>(o_l), blk.at<uint8_t>(o_r), 1, width, height, pitch, blk.at(o_ws), blk.at<int16_t>(o_d),
                                     cost ? blk.at<int32_t>(o_c) : nullptr, st);
    });
    if (disp8) blk.run([&](hipStream_t st) { return gms::launch_stereo_bm_normalize(blk.at<int16_t>(o_d), 1, width, height, blk.at<uint8_t>(o_8), st); });
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (cost) blk.out(cost, o_c, 4 * px);
    if (disp8) blk.out(disp8, o_8, px);
    return blk.finish();
}

// ---- semi-global matching (stereo_sgm_kernels.hip) ------------------------------------------------------------------
static const gms_stereo_sgm_params& sgm_params(const gms_stereo_sgm_params* p)
{
    static const gms_stereo_sgm_params ref = GMS_STEREO_SGM_PARAMS_REFERENCE;
    return p ? *p : ref;
}

size_t gms_stereo_sgm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_sgm_params* params)
{
    if (n_pairs < 0 || n_pairs > 65535 || !sgm::params_ok(sgm_params(params), width, height)) return 0;
    return gms::stereo_sgm_ws_bytes(sgm_params(params), n_pairs, width, height);
}

int gms_stereo_sgm_device(gms_ctx* c, const gms_stereo_sgm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                          int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost)
{
    const gms_stereo_sgm_params& p = sgm_params(params);
    if (!c || n_pairs < 0 || n_pairs > 65535 || !sgm::params_ok(p, width, height) || pitch < width) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_left || !d_right || !d_ws || !d_disp16) return GMS_ERR_BAD_ARG;
    const size_t need = gms::stereo_sgm_ws_bytes(p, n_pairs, width, height);
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_disp16) & 1u) ||
        (reinterpret_cast<uintptr_t>(d_cost) & 3u) || need == 0 || ws_bytes < need)
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_sgm(p, d_left, d_right, n_pairs, width, height, pitch, d_ws, d_disp16, d_cost, c->stream); });
}

int gms_stereo_sgm(const gms_stereo_sgm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                   int16_t* disp16, int32_t* cost, uint8_t* disp8)
{
    const gms_stereo_sgm_params& p = sgm_params(params);
    if (!sgm::params_ok(p, width, height) || pitch < width || !left || !right) return GMS_ERR_BAD_ARG;
    const size_t ws = gms::stereo_sgm_ws_bytes(p, 1, width, height);
    if (ws == 0) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height, img = (size_t)pitch * (size_t)(height - 1) + (size_t)width;
    gms::BlockLayout lay;  // the images keep the caller's pitch
    const size_t o_l = lay.add(img), o_r = lay.add(img), o_ws = lay.add(ws);
    const size_t o_d = lay.add(2 * px), o_c = lay.add(4 * px), o_8 = lay.add(px);
    DevBlock blk(lay, nullptr);
    blk.in(o_l, left, img);
    blk.in(o_r, right, img);
    blk.run([&](hipStream_t st) {
        return gms::launch_stereo_sgm(p, blk.at<uint8_t>(o_l), blk.at<uint8_t>(o_r), 1, width, height, pitch, blk.at(o_ws), blk.at<int16_t>(o_d),
                                      cost ? blk.at<int32_t>(o_c) : nullptr, st);
    });
    if (disp8) blk.run([&](hipStream_t st) { return gms::launch_stereo_bm_normalize(blk.at<int16_t>(o_d), 1, width, height, blk.at<uint8_t>(o_8), st); });
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (cost) blk.out(cost, o_c, 4 * px);
    if (disp8) blk.out(disp8, o_8, px);
    return blk.finish();
}

// ---- portrait mode (portrait_kernels.hip) --------------------------------------------------------------------------
static const gms_portrait_params& pm_params(const gms_portrait_params* p)
{
    static const gms_portrait_params ref = GMS_PORTRAIT_PARAMS_REFERENCE;
    return p ? *p : ref;
}

size_t gms_portrait_workspace_bytes(int width, int height, int n, const gms_portrait_params* params)
{
    if (n < 1 || n > 65535 || !pm::params_ok(pm_params(params), width, height)) return 0;
    return gms::portrait_ws_bytes(n, width, height);
}

int gms_portrait_device(gms_ctx* c, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n, int width,
                        int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr, uint8_t* d_mask,
                        uint8_t* d_selected, uint8_t* d_blurred)
{
    const gms_portrait_params& p = pm_params(params);
    if (!c || n < 1 || n > 65535 || !pm::params_ok(p, width, height) || pitch_bgr < 3 * width || pitch_disp < width) return GMS_ERR_BAD_ARG;
    if (!d_bgr || !d_disparity || !d_ws || !d_out_bgr || (reinterpret_cast<uintptr_t>(d_ws) & 255u) ||
        ws_bytes < gms::portrait_ws_bytes(n, width, height))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_portrait(p, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, d_out_bgr, d_mask, d_selected, d_blurred,
                                    c->stream);
    });
}

int gms_portrait_profile_device(gms_ctx* c, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n,
                                int width, int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr,
                                uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred, float* stage_ms)
{
    const gms_portrait_params& p = pm_params(params);
    if (!c || !stage_ms || n < 1 || n > 65535 || !pm::params_ok(p, width, height) || pitch_bgr < 3 * width || pitch_disp < width)
        return GMS_ERR_BAD_ARG;
    if (!d_bgr || !d_disparity || !d_ws || !d_out_bgr || (reinterpret_cast<uintptr_t>(d_ws) & 255u) ||
        ws_bytes < gms::portrait_ws_bytes(n, width, height))
        return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    hipEvent_t ev[GMS_PORTRAIT_STAGES + 1] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i <= GMS_PORTRAIT_STAGES && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess)
        e = gms::launch_portrait(p, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, d_out_bgr, d_mask, d_selected,
                                 d_blurred, c->stream, ev);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    for (int i = 0; i < GMS_PORTRAIT_STAGES && e == hipSuccess; i++) e = hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]);
    for (int i = 0; i <= GMS_PORTRAIT_STAGES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    GMS_HIP(e);
    return GMS_OK;
}

int gms_median_blur_device(gms_ctx* c, const uint8_t* d_src, int n, int width, int height, int channels, int pitch, int ksize,
                           uint8_t* d_dst)
{
    if (!c || n < 1 || n > 65535 || !pm::median_ok(width, height, channels, ksize) || pitch < channels * width || !d_src || !d_dst)
        return GMS_ERR_BAD_ARG;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    const uintptr_t span = (uintptr_t)n * (uintptr_t)height * (uintptr_t)pitch;
    if (s0 < d0 + span && d0 < s0 + span) return GMS_ERR_BAD_ARG;  // the destination may not overlap the source
    return on_ctx(c, [&] { return gms::launch_median_blur(d_src, n, width, height, channels, pitch, ksize, d_dst, c->stream); });
}

int gms_median_blur(const uint8_t* src, int width, int height, int channels, int ksize, uint8_t* dst)
{
    if (!pm::median_ok(width, height, channels, ksize) || !src || !dst) return GMS_ERR_BAD_ARG;
    const size_t bytes = (size_t)width * (size_t)height * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(bytes), o_dst = lay.add(bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_median_blur(blk.at<uint8_t>(o_src), 1, width, height, channels, width * channels, ksize, blk.at<uint8_t>(o_dst), st);
    });
    blk.out(dst, o_dst, bytes);
    return blk.finish();
}

int gms_portrait(const gms_portrait_params* params, const uint8_t* bgr, const uint8_t* disparity, int width, int height, uint8_t* out_bgr,
                 uint8_t* mask, uint8_t* selected, uint8_t* blurred)
{
    const gms_portrait_params& p = pm_params(params);
    if (!pm::params_ok(p, width, height) || !bgr || !disparity || !out_bgr) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_img = lay.add(3 * px), o_d = lay.add(px), o_ws = lay.add(gms::portrait_ws_bytes(1, width, height)), o_out = lay.add(3 * px);
    const size_t o_m = lay.add(px), o_s = lay.add(px), o_b = lay.add(3 * px);
    DevBlock blk(lay, nullptr);
    blk.in(o_img, bgr, 3 * px);
    blk.in(o_d, disparity, px);
    blk.run([&](hipStream_t st) {
        return gms::launch_portrait(p, blk.at<uint8_t>(o_img), blk.at<uint8_t>(o_d), 1, width, height, 3 * width, width, blk.at(o_ws),
                                    blk.at<uint8_t>(o_out), mask ? blk.at<uint8_t>(o_m) : nullptr, selected ? blk.at<uint8_t>(o_s) : nullptr,
                                    blurred ? blk.at<uint8_t>(o_b) : nullptr, st);
    });
    blk.out(out_bgr, o_out, 3 * px);
    if (mask) blk.out(mask, o_m, px);
    if (selected) blk.out(selected, o_s, px);
    if (blurred) blk.out(blurred, o_b, 3 * px);
    return blk.finish();
}

// ---- resize and warpAffine (warp_kernels.hip) ----------------------------------------------------------------------
static bool warp_ranges_ok(const uint8_t* d_src, int n, int sh, int src_pitch, const uint8_t* d_dst, int dh, int dst_pitch)
{
    if (!d_src || !d_dst) return false;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    const uintptr_t s_span = (uintptr_t)n * (uintptr_t)sh * (uintptr_t)src_pitch, d_span = (uintptr_t)n * (uintptr_t)dh * (uintptr_t)dst_pitch;
    return !(s0 < d0 + d_span && d0 < s0 + s_span);  // the destination may not overlap the source
}

int gms_resize_device(gms_ctx* c, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, uint8_t* d_dst, int dw, int dh,
                      int dst_pitch)
{
    if (!c || !warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) || !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_resize(d_src, n, sw, sh, channels, src_pitch, d_dst, dw, dh, dst_pitch, c->stream); });
}

int gms_warp_affine_device(gms_ctx* c, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, const double* d_M,
                           int n_matrices, uint8_t* d_dst, int dw, int dh, int dst_pitch)
{
    if (!c || !d_M || (n_matrices != 1 && n_matrices != n) || !warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) ||
        !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_warp_affine(d_src, n, sw, sh, channels, src_pitch, d_M, n_matrices, d_dst, dw, dh, dst_pitch, c->stream);
    });
}

int gms_rotation_matrix_2d(double center_x, double center_y, double angle, double scale, double* M)
{
    if (!M) return GMS_ERR_BAD_ARG;
    warp::rotation_matrix_2d(center_x, center_y, angle, scale, M);
    return GMS_OK;
}

int gms_resize(const uint8_t* src, int sw, int sh, int channels, uint8_t* dst, int dw, int dh)
{
    if (!src || !dst || !warp::args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw)) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_bytes = (size_t)dw * (size_t)dh * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_dst = lay.add(d_bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_resize(blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<uint8_t>(o_dst), dw, dh, dw * channels, st);
    });
    blk.out(dst, o_dst, d_bytes);
    return blk.finish();
}

int gms_warp_affine(const uint8_t* src, int sw, int sh, int channels, const double* M, uint8_t* dst, int dw, int dh)
{
    if (!src || !dst || !M || !warp::args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw))
        return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_bytes = (size_t)dw * (size_t)dh * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_M = lay.add(6 * sizeof(double)), o_dst = lay.add(d_bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.in(o_M, M, 6 * sizeof(double));
    blk.run([&](hipStream_t st) {
        return gms::launch_warp_affine(blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<double>(o_M), 1, blk.at<uint8_t>(o_dst),
                                       dw, dh, dw * channels, st);
    });
    blk.out(dst, o_dst, d_bytes);
    return blk.finish();
}

int gms_img_rotate(const uint8_t* src, int width, int height, int channels, double angle, uint8_t* dst)
{
    double M[6];
    warp::rotation_matrix_2d(width / 2., height / 2., angle, 1.0, M);
    return gms_warp_affine(src, width, height, channels, M, dst, width, height);
}

// ---- a dense cloud from a posed pair (rectify_kernels.hip, rectify_core.h) ------------------------------------------
static_assert(sizeof(gms_rectify_plan) == 200, "gms_rectify_plan: 23 doubles and four 32-bit words");

int gms_rectify_plan_host(const gms_camera* camera, const double* R, const double* t, int width, int height, int out_w, int out_h,
                          gms_rectify_plan* plan)
{
    if (!camera || !R || !t || !plan || !warp::side_ok(width) || !warp::side_ok(height) || out_w > warp::kMaxSide || out_h > warp::kMaxSide)
        return GMS_ERR_BAD_ARG;
    rect::make_plan(rect::camera_of(*camera), R, t, width, height, out_w, out_h, *plan);
    return GMS_OK;
}

int gms_rectify_plan_device(gms_ctx* c, const gms_camera* camera, const gms_two_view* d_tv, int n_pairs, int width, int height, int out_w,
                            int out_h, gms_rectify_plan* d_plans)
{
    if (!c || !camera || n_pairs < 0 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height) || out_w > warp::kMaxSide ||
        out_h > warp::kMaxSide)
        return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_tv || !d_plans) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_rectify_plan(*camera, d_tv, n_pairs, width, height, out_w, out_h, d_plans, c->stream); });
}

int gms_rectify_q(const gms_rectify_plan* plan, double* Q)
{
    if (!plan || !Q) return GMS_ERR_BAD_ARG;
    rect::plan_q(*plan, Q);
    return GMS_OK;
}

int gms_rectify_device(gms_ctx* c, const gms_camera* camera, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch,
                       const gms_rectify_plan* d_plans, int n_plans, int which, uint8_t* d_dst, int dw, int dh, int dst_pitch,
                       uint8_t* d_valid)
{
    if (!c || !camera || !d_plans || (reinterpret_cast<uintptr_t>(d_plans) & 7u) || (n_plans != 1 && n_plans != n) || (which != 1 && which != 2) ||
        !rect::image_args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) || !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_rectify(*camera, d_src, n, sw, sh, channels, src_pitch, d_plans, n_plans, which, d_dst, dw, dh, dst_pitch, d_valid,
                                   c->stream);
    });
}

int gms_rectify(const gms_camera* camera, const gms_rectify_plan* plan, int which, const uint8_t* src, int sw, int sh, int channels,
                uint8_t* dst, uint8_t* valid)
{
    if (!camera || !plan || !src || !dst || (which != 1 && which != 2)) return GMS_ERR_BAD_ARG;
    const int dw = plan->out_w, dh = plan->out_h;
    if (!rect::image_args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw)) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_px = (size_t)dw * (size_t)dh;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_plan = lay.add(sizeof(gms_rectify_plan)), o_dst = lay.add(d_px * channels), o_valid = lay.add(d_px);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.in(o_plan, plan, sizeof(gms_rectify_plan));
    blk.run([&](hipStream_t st) {
        return gms::launch_rectify(*camera, blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<gms_rectify_plan>(o_plan), 1, which,
                                   blk.at<uint8_t>(o_dst), dw, dh, dw * channels, valid ? blk.at<uint8_t>(o_valid) : nullptr, st);
    });
    blk.out(dst, o_dst, d_px * channels);
    if (valid) blk.out(valid, o_valid, d_px);
    return blk.finish();
}

int gms_undistort(const gms_camera* camera, const uint8_t* src, int width, int height, int channels, uint8_t* dst)
{
    if (!camera || !warp::side_ok(width) || !warp::side_ok(height)) return GMS_ERR_BAD_ARG;
    gms_rectify_plan plan;
    rect::identity_plan(rect::camera_of(*camera), width, height, plan);
    return gms_rectify(camera, &plan, 1, src, width, height, channels, dst, nullptr);
}

size_t gms_dense_cloud_workspace_bytes(int width, int height, int n_pairs)
{
    if (n_pairs < 1 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height)) return 0;
    return gms::dense_cloud_ws_bytes(n_pairs, width, height);
}

int gms_dense_cloud_device(gms_ctx* c, const int16_t* d_disp16, const uint8_t* d_valid, const uint8_t* d_image, int channels,
                           int image_pitch, int n_pairs, int width, int height, const gms_rectify_plan* d_plans, int filtered16,
                           int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames,
                           void* d_ws, size_t ws_bytes, int cap, float* d_xyz, uint8_t* d_color, int32_t* d_pixel, int32_t* d_count)
{
    if (!c || n_pairs < 0 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height) || min_disp16 < 1 || cap < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    const bool any_reg = d_pairs || d_reg || d_views, all_reg = d_pairs && d_reg && d_views;
    if (!d_disp16 || !d_valid || !d_plans || !d_ws || !d_count || (cap > 0 && (!d_xyz || !d_pixel)) || any_reg != all_reg ||
        (all_reg && n_frames < 1))
        return GMS_ERR_BAD_ARG;
    if (d_image && ((channels != 1 && channels != 3) || (long long)image_pitch < (long long)channels * width)) return GMS_ERR_BAD_ARG;
    if (d_color && !d_image) return GMS_ERR_BAD_ARG;
    const size_t need = gms::dense_cloud_ws_bytes(n_pairs, width, height);
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_plans) & 7u) || (reinterpret_cast<uintptr_t>(d_disp16) & 1u) ||
        (reinterpret_cast<uintptr_t>(d_xyz) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_pixel) & 3u) || (reinterpret_cast<uintptr_t>(d_count) & 3u) || ws_bytes < need)
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_dense_cloud(d_disp16, d_valid, d_image, channels, image_pitch, n_pairs, width, height, d_plans, filtered16, min_disp16,
                                       d_pairs, d_reg, d_views, n_frames, d_ws, cap, d_xyz, d_color, d_pixel, d_count, c->stream);
    });
}

static const gms_stereo_sgm_params& dense_sgm_params(const gms_stereo_sgm_params* p)
{
    static const gms_stereo_sgm_params ref = GMS_STEREO_SGM_PARAMS_DENSE;
    return p ? *p : ref;
}

static bool dense_shape_ok(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params& p)
{
    return n_pairs >= 1 && n_pairs <= 65535 && (channels == 1 || channels == 3) && warp::side_ok(sw) && warp::side_ok(sh) && warp::side_ok(ow) &&
           warp::side_ok(oh) && sgm::params_ok(p, ow, oh);
}

size_t gms_dense_pairs_workspace_bytes(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params* params)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p)) return 0;
    const size_t sgm_bytes = gms::stereo_sgm_ws_bytes(p, n_pairs, ow, oh);
    return sgm_bytes ? gms::dense_pairs_layout(n_pairs, sw, sh, channels, ow, oh, sgm_bytes).total : 0;
}

// everything behind the plans, in stream order: grey, the three rectified images, the matcher, the cloud
static hipError_t dense_pairs_launch(const gms_camera& cam, const gms_stereo_sgm_params& p, const uint8_t* d_img1, const uint8_t* d_img2, int n,
                                     int sw, int sh, int channels, int ow, int oh, int min_disp16, const gms_pair* d_pairs,
                                     const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                                     const gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                                     int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count,
                                     int speckle_size, int speckle_diff16, int32_t* d_removed, hipStream_t st)
{
    // speckle_size > 0: the workspace is DensePairsFilteredLayout's, whose first regions are DensePairsLayout's
    const gms::DensePairsFilteredLayout F = gms::dense_pairs_filtered_layout(n, sw, sh, channels, ow, oh, gms::stereo_sgm_ws_bytes(p, n, ow, oh));
    const gms::DensePairsLayout& L = F.pairs;
    const uint8_t *g1 = d_img1, *g2 = d_img2;
    hipError_t e;
    if (channels == 3) {
        uint8_t* grey = gms::ws_ptr<uint8_t>(d_ws, L.grey);
        const size_t plane = (size_t)n * (size_t)sw * (size_t)sh;
        if ((e = gms::launch_bgr_to_gray(d_img1, n, sw, sh, grey, st)) != hipSuccess) return e;
        if ((e = gms::launch_bgr_to_gray(d_img2, n, sw, sh, grey + plane, st)) != hipSuccess) return e;
        g1 = grey;
        g2 = grey + plane;
        if ((e = gms::launch_rectify(cam, d_img1, n, sw, sh, 3, 3 * sw, d_plans, n, 1, d_color, ow, oh, 3 * ow, nullptr, st)) != hipSuccess) return e;
    }
    if ((e = gms::launch_rectify(cam, g1, n, sw, sh, 1, sw, d_plans, n, 1, d_rect1, ow, oh, ow, d_valid, st)) != hipSuccess) return e;
    if ((e = gms::launch_rectify(cam, g2, n, sw, sh, 1, sw, d_plans, n, 2, d_rect2, ow, oh, ow, nullptr, st)) != hipSuccess) return e;
    if ((e = gms::launch_stereo_sgm(p, d_rect1, d_rect2, n, ow, oh, ow, gms::ws_ptr<void>(d_ws, L.sgm), d_disp16, nullptr, st)) != hipSuccess) return e;
    if (speckle_size > 0)
        e = gms::launch_filter_speckles(d_disp16, n, ow, oh, (p.bm.min_disparity - 1) * 16, speckle_size, speckle_diff16,
                                        gms::ws_ptr<void>(d_ws, F.speckle), d_removed, st);
    else if (d_removed)
        e = hipMemsetAsync(d_removed, 0, sizeof(int32_t) * (size_t)n, st);
    if (e != hipSuccess) return e;
    return gms::launch_dense_cloud(d_disp16, d_valid, channels == 3 ? d_color : d_rect1, channels, channels * ow, n, ow, oh, d_plans,
                                   (p.bm.min_disparity - 1) * 16, min_disp16, d_pairs, d_reg, d_views, n_frames, gms::ws_ptr<void>(d_ws, L.cloud), cap,
                                   d_xyz, d_cloud_color, d_pixel, d_count, st);
}

size_t gms_dense_pairs_filtered_workspace_bytes(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params* params)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p)) return 0;
    const size_t sgm_bytes = gms::stereo_sgm_ws_bytes(p, n_pairs, ow, oh);
    return sgm_bytes ? gms::dense_pairs_filtered_layout(n_pairs, sw, sh, channels, ow, oh, sgm_bytes).total : 0;
}

// filtered: the workspace also holds the filter's region (also with speckle_size 0, so that one size serves every call)
static int dense_pairs_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1, const uint8_t* d_img2,
                              int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh, int min_disp16,
                              const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                              size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                              int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count, bool filtered,
                              int speckle_size, int speckle_diff16, int32_t* d_removed)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!c || !camera || !dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p) || min_disp16 < 1 || cap < 0) return GMS_ERR_BAD_ARG;
    if (speckle_size < 0 || speckle_diff16 < 0 || (reinterpret_cast<uintptr_t>(d_removed) & 3u)) return GMS_ERR_BAD_ARG;
    const bool any_reg = d_pairs || d_reg || d_views, all_reg = d_pairs && d_reg && d_views;
    if (!d_img1 || !d_img2 || !d_tv || !d_ws || !d_plans || !d_rect1 || !d_rect2 || !d_valid || (channels == 3 && !d_color) || !d_disp16 ||
        !d_count || (cap > 0 && (!d_xyz || !d_pixel)) || any_reg != all_reg || (all_reg && n_frames < 1))
        return GMS_ERR_BAD_ARG;
    const size_t need = filtered ? gms_dense_pairs_filtered_workspace_bytes(sw, sh, channels, ow, oh, n_pairs, &p)
                                 : gms_dense_pairs_workspace_bytes(sw, sh, channels, ow, oh, n_pairs, &p);
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_plans) & 7u) || (reinterpret_cast<uintptr_t>(d_disp16) & 1u) ||
        (reinterpret_cast<uintptr_t>(d_xyz) & 3u) || (reinterpret_cast<uintptr_t>(d_pixel) & 3u) || (reinterpret_cast<uintptr_t>(d_count) & 3u) ||
        need == 0 || ws_bytes < need)
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        const hipError_t e = gms::launch_rectify_plan(*camera, d_tv, n_pairs, sw, sh, ow, oh, d_plans, c->stream);
        if (e != hipSuccess) return e;
        return dense_pairs_launch(*camera, p, d_img1, d_img2, n_pairs, sw, sh, channels, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames, d_ws,
                                  d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, speckle_size,
                                  speckle_diff16, d_removed, c->stream);
    });
}

int gms_dense_pairs_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1, const uint8_t* d_img2,
                           int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh, int min_disp16,
                           const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                           size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                           int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count)
{
    return dense_pairs_device(c, camera, params, d_img1, d_img2, n_pairs, sw, sh, channels, d_tv, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames,
                              d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, false,
                              0, 0, nullptr);
}

int gms_dense_pairs_filtered_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1,
                                    const uint8_t* d_img2, int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh,
                                    int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames,
                                    void* d_ws, size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid,
                                    uint8_t* d_color, int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel,
                                    int32_t* d_count, int speckle_size, int speckle_diff16, int32_t* d_removed)
{
    return dense_pairs_device(c, camera, params, d_img1, d_img2, n_pairs, sw, sh, channels, d_tv, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames,
                              d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, true,
                              speckle_size, speckle_diff16, d_removed);
}

int gms_dense_pair_filtered(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2, int width,
                            int height, int channels, const double* R, const double* t, int out_w, int out_h, int min_disp16, gms_rectify_plan* plan,
                            uint8_t* rect1, uint8_t* rect2, uint8_t* valid, uint8_t* color, int16_t* disp16, int cap, float* xyz,
                            uint8_t* cloud_color, int32_t* pixel, int32_t* count, int speckle_size, int speckle_diff16, int32_t* removed)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!camera || !img1 || !img2 || !R || !t || !plan || !count || min_disp16 < 1 || cap < 0 || (cap > 0 && (!xyz || !pixel))) return GMS_ERR_BAD_ARG;
    if (speckle_size < 0 || speckle_diff16 < 0) return GMS_ERR_BAD_ARG;
    const int rc = gms_rectify_plan_host(camera, R, t, width, height, out_w, out_h, plan);
    if (rc != GMS_OK) return rc;
    if (plan->status != GMS_OK) return GMS_ERR_NO_MODEL;
    const int ow = plan->out_w, oh = plan->out_h;
    const size_t ws = speckle_size > 0 ? gms_dense_pairs_filtered_workspace_bytes(width, height, channels, ow, oh, 1, &p)
                                       : gms_dense_pairs_workspace_bytes(width, height, channels, ow, oh, 1, &p);
    if (ws == 0) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)width * (size_t)height * (size_t)channels, px = (size_t)ow * (size_t)oh, ucap = (size_t)cap;
    gms::BlockLayout lay;
    const size_t o_1 = lay.add(s_bytes), o_2 = lay.add(s_bytes), o_plan = lay.add(sizeof(gms_rectify_plan)), o_ws = lay.add(ws), o_r1 = lay.add(px),
                 o_r2 = lay.add(px), o_v = lay.add(px), o_c = lay.add(3 * px), o_d = lay.add(2 * px), o_xyz = lay.add(12 * ucap + 4),
                 o_cc = lay.add(3 * ucap + 4), o_pix = lay.add(4 * ucap + 4), o_n = lay.add(4), o_rm = lay.add(4);
    DevBlock blk(lay, nullptr);
    blk.in(o_1, img1, s_bytes);
    blk.in(o_2, img2, s_bytes);
    blk.in(o_plan, plan, sizeof(gms_rectify_plan));
    blk.run([&](hipStream_t st) {
        return dense_pairs_launch(*camera, p, blk.at<uint8_t>(o_1), blk.at<uint8_t>(o_2), 1, width, height, channels, ow, oh, min_disp16, nullptr, nullptr,
                                  nullptr, 0, blk.at(o_ws), blk.at<gms_rectify_plan>(o_plan), blk.at<uint8_t>(o_r1), blk.at<uint8_t>(o_r2),
                                  blk.at<uint8_t>(o_v), blk.at<uint8_t>(o_c), blk.at<int16_t>(o_d), cap, blk.at<float>(o_xyz),
                                  cloud_color ? blk.at<uint8_t>(o_cc) : nullptr, blk.at<int32_t>(o_pix), blk.at<int32_t>(o_n), speckle_size,
                                  speckle_diff16, removed ? blk.at<int32_t>(o_rm) : nullptr, st);
    });
    int32_t n = 0;
    blk.out_now(&n, o_n, 4);
    *count = n;
    if (removed) blk.out(removed, o_rm, 4);
    const size_t k = (size_t)(n < cap ? n : cap);
    if (rect1) blk.out(rect1, o_r1, px);
    if (rect2) blk.out(rect2, o_r2, px);
    if (valid) blk.out(valid, o_v, px);
    if (color && channels == 3) blk.out(color, o_c, 3 * px);
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (k && blk.ok()) {
        blk.out(xyz, o_xyz, 12 * k);
        blk.out(pixel, o_pix, 4 * k);
        if (cloud_color) blk.out(cloud_color, o_cc, (size_t)channels * k);
    }
    return blk.finish();
}

int gms_dense_pair(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2, int width, int height,
                   int channels, const double* R, const double* t, int out_w, int out_h, int min_disp16, gms_rectify_plan* plan, uint8_t* rect1,
                   uint8_t* rect2, uint8_t* valid, uint8_t* color, int16_t* disp16, int cap, float* xyz, uint8_t* cloud_color, int32_t* pixel,
                   int32_t* count)
{
    return gms_dense_pair_filtered(camera, params, img1, img2, width, height, channels, R, t, out_w, out_h, min_disp16, plan, rect1, rect2, valid, color,
                                   disp16, cap, xyz, cloud_color, pixel, count, 0, 0, nullptr);
}

// ---- the speckle filter (speckle_kernels.hip, speckle_core.h) ------------------------------------------------------
size_t gms_filter_speckles_workspace_bytes(int width, int height, int n)
{
    if (!spk::args_ok(width, height, n, 0, 0, 0)) return 0;
    return gms::speckle_ws_bytes(n, width, height);
}

int gms_filter_speckles_device(gms_ctx* c, int16_t* d_disp16, int n, int width, int height, int new_val, int max_speckle_size, int max_diff,
                               void* d_ws, size_t ws_bytes, int32_t* d_removed)
{
    if (!c || !spk::args_ok(width, height, n, new_val, max_speckle_size, max_diff) || !d_disp16 || !d_ws) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_disp16) & 1u) || (reinterpret_cast<uintptr_t>(d_removed) & 3u) ||
        ws_bytes < gms::speckle_ws_bytes(n, width, height))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_filter_speckles(d_disp16, n, width, height, new_val, max_speckle_size, max_diff, d_ws, d_removed, c->stream);
    });
}

int gms_filter_speckles(int16_t* disp16, int width, int height, int new_val, int max_speckle_size, int max_diff, int32_t* removed)
{
    if (!spk::args_ok(width, height, 1, new_val, max_speckle_size, max_diff) || !disp16) return GMS_ERR_BAD_ARG;
    const size_t bytes = 2 * (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_d = lay.add(bytes), o_ws = lay.add(gms::speckle_ws_bytes(1, width, height)), o_rm = lay.add(4);
    DevBlock blk(lay, nullptr);
    blk.in(o_d, disp16, bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_filter_speckles(blk.at<int16_t>(o_d), 1, width, height, new_val, max_speckle_size, max_diff, blk.at(o_ws),
                                           blk.at<int32_t>(o_rm), st);
    });
    blk.out(disp16, o_d, bytes);
    if (removed) blk.out(removed, o_rm, 4);
    return blk.finish();
}

// ---- the clouds of several pairs fused into one (dense_fuse_kernels.hip, dense_fuse_core.h) ----------------------
static_assert(sizeof(gms_dense_fuse_src) == 88, "gms_dense_fuse_src: eight pointers and six 32-bit words");

size_t gms_dense_fuse_workspace_bytes(int n_src, int max_cap)
{
    if (!fuse::call_args_ok(n_src, max_cap, 1, 1, 0, 1, 0)) return 0;
    return gms::dense_fuse_ws_bytes(n_src, max_cap);
}

int gms_dense_fuse_device(gms_ctx* c, const gms_dense_fuse_src* d_src, int n_src, int max_cap, const int32_t* d_neighbors, int n_nb, int channels,
                          int tol16, int min_support, void* d_ws, size_t ws_bytes, int fused_cap, float* d_xyz, uint8_t* d_color, int32_t* d_source,
                          int32_t* d_index, uint8_t* d_support, uint8_t* d_conflict, int32_t* d_counts)
{
    if (!c || !fuse::call_args_ok(n_src, max_cap, n_nb, channels, tol16, min_support, fused_cap)) return GMS_ERR_BAD_ARG;
    if (!d_src || !d_neighbors || !d_ws || !d_counts || (fused_cap > 0 && (!d_xyz || !d_source || !d_index || !d_support || !d_conflict)))
        return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_src) & 7u) || (reinterpret_cast<uintptr_t>(d_neighbors) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_xyz) & 3u) || (reinterpret_cast<uintptr_t>(d_source) & 3u) || (reinterpret_cast<uintptr_t>(d_index) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_counts) & 3u) || ws_bytes < gms::dense_fuse_ws_bytes(n_src, max_cap))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_dense_fuse(d_src, n_src, max_cap, d_neighbors, n_nb, channels, tol16, min_support, d_ws, fused_cap, d_xyz, d_color, d_source,
                                      d_index, d_support, d_conflict, d_counts, c->stream);
    });
}

int gms_dense_fuse(const gms_dense_fuse_src* src, int n_src, const int32_t* neighbors, int n_nb, int channels, int tol16, int min_support,
                   int fused_cap, float* xyz, uint8_t* color, int32_t* source, int32_t* index, uint8_t* support, uint8_t* conflict, int32_t* counts)
{
    if (!src || n_src < 1 || n_src > 65535 || !neighbors || !counts || (fused_cap > 0 && (!xyz || !source || !index || !support || !conflict)))
        return GMS_ERR_BAD_ARG;
    long long max_cap = 1;
    for (int i = 0; i < n_src; ++i) {
        const gms_dense_fuse_src& s = src[i];
        if (!fuse::shape_ok(s, fuse::kMaxCap) || !s.d_disp16 || !s.d_valid || !s.d_plan || !s.d_count || (s.cap > 0 && !s.d_xyz)) return GMS_ERR_BAD_ARG;
        if (s.cap > max_cap) max_cap = s.cap;
    }
    if (!fuse::call_args_ok(n_src, max_cap, n_nb, channels, tol16, min_support, fused_cap)) return GMS_ERR_BAD_ARG;
    const size_t ws = gms::dense_fuse_ws_bytes(n_src, (int)max_cap), ucap = (size_t)fused_cap, un = (size_t)n_src;
    // one block: the table, the neighbours, the workspace, the outputs, then every source's arrays
    struct Off { size_t disp, valid, plan, xyz, color, count, view, reg; };
    std::vector<Off> off(un);
    gms::BlockLayout lay;
    const size_t o_tab = lay.add(sizeof(gms_dense_fuse_src) * un), o_nb = lay.add(4 * un * (size_t)n_nb), o_ws = lay.add(ws), o_xyz = lay.add(12 * ucap + 4),
                 o_col = lay.add(3 * ucap + 4), o_src = lay.add(4 * ucap + 4), o_idx = lay.add(4 * ucap + 4), o_sup = lay.add(ucap + 4),
                 o_con = lay.add(ucap + 4), o_cnt = lay.add(4 * (un + 1));
    for (size_t i = 0; i < un; ++i) {
        const gms_dense_fuse_src& s = src[i];
        const size_t px = (size_t)s.width * (size_t)s.height, cap = (size_t)s.cap;
        off[i] = {lay.add(2 * px), lay.add(px), lay.add(sizeof(gms_rectify_plan)), lay.add(12 * cap + 4), lay.add(s.d_color ? channels * cap + 4 : 4),
                  lay.add(4), lay.add(sizeof(gms_sfm_view)), lay.add(sizeof(gms_sfm_pair_reg))};
    }
    DevBlock blk(lay, nullptr);
    std::vector<gms_dense_fuse_src> tab(src, src + n_src);
    for (size_t i = 0; i < un; ++i) {
        const gms_dense_fuse_src& s = src[i];
        const size_t px = (size_t)s.width * (size_t)s.height, cap = (size_t)s.cap;
        blk.in(off[i].disp, s.d_disp16, 2 * px);
        blk.in(off[i].valid, s.d_valid, px);
        blk.in(off[i].plan, s.d_plan, sizeof(gms_rectify_plan));
        blk.in(off[i].count, s.d_count, 4);
        if (cap) blk.in(off[i].xyz, s.d_xyz, 12 * cap);
        if (cap && s.d_color) blk.in(off[i].color, s.d_color, channels * cap);
        if (s.d_view) blk.in(off[i].view, s.d_view, sizeof(gms_sfm_view));
        if (s.d_reg) blk.in(off[i].reg, s.d_reg, sizeof(gms_sfm_pair_reg));
        tab[i].d_disp16 = blk.at<int16_t>(off[i].disp);
        tab[i].d_valid = blk.at<uint8_t>(off[i].valid);
        tab[i].d_plan = blk.at<gms_rectify_plan>(off[i].plan);
        tab[i].d_xyz = blk.at<float>(off[i].xyz);
        tab[i].d_color = s.d_color ? blk.at<uint8_t>(off[i].color) : nullptr;
        tab[i].d_count = blk.at<int32_t>(off[i].count);
        tab[i].d_view = s.d_view ? blk.at<gms_sfm_view>(off[i].view) : nullptr;
        tab[i].d_reg = s.d_reg ? blk.at<gms_sfm_pair_reg>(off[i].reg) : nullptr;
    }
    blk.in(o_tab, tab.data(), sizeof(gms_dense_fuse_src) * un);
    blk.in(o_nb, neighbors, 4 * un * (size_t)n_nb);
    blk.run([&](hipStream_t st) {
        return gms::launch_dense_fuse(blk.at<gms_dense_fuse_src>(o_tab), n_src, (int)max_cap, blk.at<int32_t>(o_nb), n_nb, channels, tol16, min_support,
                                      blk.at(o_ws), fused_cap, blk.at<float>(o_xyz), color ? blk.at<uint8_t>(o_col) : nullptr, blk.at<int32_t>(o_src),
                                      blk.at<int32_t>(o_idx), blk.at<uint8_t>(o_sup), blk.at<uint8_t>(o_con), blk.at<int32_t>(o_cnt), st);
    });
    blk.out_now(counts, o_cnt, 4 * (un + 1));  // (also waits for the copies in: `tab` is read until then)
    const size_t k = blk.ok() ? (size_t)(counts[n_src] < fused_cap ? counts[n_src] : fused_cap) : 0;
    if (k) {
        blk.out(xyz, o_xyz, 12 * k);
        if (color) blk.out(color, o_col, (size_t)channels * k);
        blk.out(source, o_src, 4 * k);
        blk.out(index, o_idx, 4 * k);
        blk.out(support, o_sup, k);
        blk.out(conflict, o_con, k);
    }
    return blk.finish();
}

// ---- camera calibration from chessboard photographs (calib_kernels.hip, calib_core.h) -----------------------------
static_assert(sizeof(gms_chess_candidate) == 12 && sizeof(calib::Candidate) == 12, "candidate records are three 32-bit words");
static_assert(GMS_CHESS_MAX_CANDIDATES == calib::kMaxCandidates && GMS_WARP_MAX_SIDE == calib::kMaxSide && GMS_DETECT_BORDER == calib::kBorder,
              "gms.h and calib_core.h state the same limits");

size_t gms_chess_candidates_workspace_bytes(int width, int height, int n_images)
{
    if (!calib::batch_ok(n_images, width, height, 1)) return 0;
    return gms::chess_candidates_ws_bytes(n_images, width, height);
}

int gms_chess_candidates_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int max_candidates, void* d_ws,
                                size_t ws_bytes, gms_chess_candidate* d_out, int32_t* d_counts)
{
    if (!c || !calib::batch_ok(n_images, width, height, max_candidates) || !d_images || !d_ws || !d_out || !d_counts) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || (reinterpret_cast<uintptr_t>(d_out) & 3u) || (reinterpret_cast<uintptr_t>(d_counts) & 3u) ||
        ws_bytes < gms::chess_candidates_ws_bytes(n_images, width, height))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_chess_candidates(d_images, n_images, width, height, max_candidates, d_ws, d_out, d_counts, c->stream); });
}

int gms_corner_subpix_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, const int32_t* d_image_of,
                             double* d_corners, int n_corners, int win, int max_iter, double eps, int32_t* d_status)
{
    if (!c || n_images < 1 || n_images > 65535 || n_corners < 0 || !calib::subpix_args_ok(width, height, win, max_iter, eps)) return GMS_ERR_BAD_ARG;
    if (n_corners == 0) return GMS_OK;
    if (!d_images || !d_corners || (reinterpret_cast<uintptr_t>(d_corners) & 7u) || (reinterpret_cast<uintptr_t>(d_image_of) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_status) & 3u))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_corner_subpix(d_images, n_images, width, height, d_image_of, d_corners, n_corners, max_iter, eps, d_status, c->stream);
    });
}

int gms_find_chessboard_corners(const uint8_t* image, int width, int height, int nx, int ny, int* found, float* corners)
{
    if (!image || !found || !corners || nx < 2 || ny < 2 || nx == ny || (long long)nx * ny > calib::kMaxCandidates ||
        !calib::batch_ok(1, width, height, nx * ny))
        return GMS_ERR_BAD_ARG;
    *found = 0;
    const int n = nx * ny;
    const size_t px = (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_img = lay.add(px), o_ws = lay.add(gms::chess_candidates_ws_bytes(1, width, height)), o_out = lay.add((size_t)n * sizeof(gms_chess_candidate)),
                 o_cnt = lay.add(sizeof(int32_t));
    std::vector<gms_chess_candidate> cand((size_t)n);
    int32_t count = 0;
    DevBlock blk(lay, nullptr);
    blk.in(o_img, image, px);
    blk.run([&](hipStream_t st) {
        return gms::launch_chess_candidates(blk.at<uint8_t>(o_img), 1, width, height, n, blk.at(o_ws), blk.at<gms_chess_candidate>(o_out),
                                            blk.at<int32_t>(o_cnt), st);
    });
    blk.out(&count, o_cnt, sizeof(int32_t));
    blk.out(cand.data(), o_out, (size_t)n * sizeof(gms_chess_candidate));
    const int rc = blk.finish();
    if (rc != GMS_OK || count < n) return rc;
    std::vector<calib::P2> p((size_t)n), ordered;
    for (int i = 0; i < n; ++i) p[i] = {(double)cand[i].x, (double)cand[i].y};
    if (!calib::order_board(p, nx, ny, ordered)) return GMS_OK;
    for (int i = 0; i < n; ++i) {
        corners[2 * i] = (float)ordered[i].x;
        corners[2 * i + 1] = (float)ordered[i].y;
    }
    *found = 1;
    return GMS_OK;
}

int gms_order_chessboard(const double* points, int nx, int ny, int* found, double* ordered)
{
    if (!points || !found || !ordered || nx < 2 || ny < 2 || nx == ny || (long long)nx * ny > calib::kMaxCandidates) return GMS_ERR_BAD_ARG;
    const int n = nx * ny;
    std::vector<calib::P2> p((size_t)n), o;
    for (int i = 0; i < n; ++i) p[i] = {points[2 * i], points[2 * i + 1]};
    *found = calib::order_board(p, nx, ny, o) ? 1 : 0;
    if (*found)
        for (int i = 0; i < n; ++i) {
            ordered[2 * i] = o[i].x;
            ordered[2 * i + 1] = o[i].y;
        }
    return GMS_OK;
}

int gms_corner_subpix(const uint8_t* image, int width, int height, double* corners, int n_corners, int win, int max_iter, double eps,
                      int32_t* status)
{
    if (!image || n_corners < 0 || (n_corners > 0 && !corners) || !calib::subpix_args_ok(width, height, win, max_iter, eps)) return GMS_ERR_BAD_ARG;
    for (int i = 0; i < n_corners; ++i)
        if (!calib::subpix_window_ok(width, height, corners[2 * i], corners[2 * i + 1])) return GMS_ERR_BAD_ARG;
    if (n_corners == 0) return GMS_OK;
    const size_t px = (size_t)width * (size_t)height, cb = (size_t)n_corners * 2 * sizeof(double), sb = (size_t)n_corners * sizeof(int32_t);
    gms::BlockLayout lay;
    const size_t o_img = lay.add(px), o_c = lay.add(cb), o_s = lay.add(sb);
    DevBlock blk(lay, nullptr);
    blk.in(o_img, image, px);
    blk.in(o_c, corners, cb);
    blk.run([&](hipStream_t st) {
        return gms::launch_corner_subpix(blk.at<uint8_t>(o_img), 1, width, height, nullptr, blk.at<double>(o_c), n_corners, max_iter, eps,
                                         blk.at<int32_t>(o_s), st);
    });
    blk.out(corners, o_c, cb);
    if (status) blk.out(status, o_s, sb);
    return blk.finish();
}

int gms_calibrate_camera(const double* object_points, const double* image_points, const int32_t* counts, int n_views, int width, int height,
                         double* K, double* dist, double* rvecs, double* tvecs, double* rms)
{
    if (!object_points || !image_points || !counts || n_views < 1 || n_views > 4096 || width < 1 || height < 1 || !K || !dist || !rvecs ||
        !tvecs || !rms)
        return GMS_ERR_BAD_ARG;
    std::vector<int> off(1, 0);
    for (int v = 0; v < n_views; ++v) {
        if (counts[v] < 4 || counts[v] > (1 << 20)) return GMS_ERR_BAD_ARG;
        off.push_back(off.back() + counts[v]);
    }
    const size_t total = (size_t)off.back();
    std::vector<calib::P3> obj(total);
    std::vector<calib::P2> img(total);
    for (size_t i = 0; i < total; ++i) {
        obj[i] = {object_points[3 * i], object_points[3 * i + 1], object_points[3 * i + 2]};
        img[i] = {image_points[2 * i], image_points[2 * i + 1]};
    }
    calib::Calibration cal;
    if (!calib::calibrate_camera(obj, img, off, width, height, cal)) return GMS_ERR_DOMAIN;
    std::copy(cal.K, cal.K + 9, K);
    std::copy(cal.dist, cal.dist + 5, dist);
    std::copy(cal.rvecs.begin(), cal.rvecs.end(), rvecs);
    std::copy(cal.tvecs.begin(), cal.tvecs.end(), tvecs);
    *rms = cal.rms;
    return GMS_OK;
}

int gms_disparity_device(gms_ctx* c, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                         const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches, int width, int height,
                         const uint8_t* d_gt, int disp_ratio, uint8_t* d_disparity, uint32_t* d_work, gms_disparity_stats* d_stats)
{
    if (!c || n1 < 0 || n2 < 0 || max_matches < 0 || width <= 0 || height <= 0) return GMS_ERR_BAD_ARG;
    if (!d_n_matches || !d_disparity || !d_work || !d_stats || (d_gt && disp_ratio == 0)) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_kp1 || !d_kp2 || !d_matches)) return GMS_ERR_BAD_ARG;
    if (max_matches >= (1 << 24)) return GMS_ERR_CAPACITY;  // the scatter key keeps the match index in 24 bits
    return on_ctx(c, [&] {
        return gms::launch_disparity(d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, width, height, d_gt, disp_ratio, d_disparity, d_work,
                                     d_stats, c->stream);
    });
}

int gms_gather_points_device(gms_ctx* c, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                             const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches,
                             float* d_coords1, float* d_coords2, int32_t* d_status)
{
    if (!c || n1 < 0 || n2 < 0 || max_matches < 0 || !d_n_matches || !d_status) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_kp1 || !d_kp2 || !d_matches || !d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_gather_points(d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, d_coords1, d_coords2, d_status, c->stream);
    });
}

int gms_triangulate_device(gms_ctx* c, const double camera[4], const double dist[5], const double P1[12], const double P2[12],
                           const float* d_coords1, const float* d_coords2, const int32_t* d_n_matches, int max_matches,
                           double* d_points3d, gms_triangulation_stats* d_stats)
{
    if (!c || !camera || !P1 || !P2 || !d_n_matches || !d_stats || max_matches < 0) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_coords1 || !d_coords2 || !d_points3d)) return GMS_ERR_BAD_ARG;
    if (camera[0] == 0.0 || camera[1] == 0.0) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_triangulate(camera, dist, P1, P2, d_coords1, d_coords2, d_n_matches, max_matches, d_points3d, d_stats, c->stream);
    });
}

int gms_recover_pose_device(gms_ctx* c, const double E[9], const double camera[4], const float* d_coords1, const float* d_coords2,
                            const int32_t* d_n_matches, int max_matches, const uint8_t* d_in_mask, gms_pose* d_pose, uint8_t* d_out_mask)
{
    if (!c || !E || !camera || !d_n_matches || !d_pose || max_matches < 0) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    if (camera[0] == 0.0 || camera[1] == 0.0) return GMS_ERR_BAD_ARG;
    double R1[9], R2[9], t[3];
    if (!gms::tv::decompose_essential(E, R1, R2, t)) return GMS_ERR_BAD_ARG;  // cv::decomposeEssentialMat (twoview_core.h)
    double P[4][12];
    for (int h = 0; h < 4; ++h) {
        const double* R = (h & 1) ? R2 : R1;
        const double sg = h < 2 ? 1.0 : -1.0;
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) P[h][4 * r + k] = R[3 * r + k];
            P[h][4 * r + 3] = sg * t[r];
        }
    }
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    GMS_TRY(grow_pose_ws(c, (size_t)max_matches + 48, c->stream));
    GMS_HIP(gms::launch_recover_pose(camera, P, 50.0, d_coords1, d_coords2, d_n_matches, max_matches, d_in_mask, d_pose, d_out_mask,
                                     c->pose_ws.p, c->stream));
    return GMS_OK;
}

// ---- the batched consumers (twoview_kernels.hip): nothing but launches on the context's stream --------------------------------
static bool camera_ok(const gms_camera* cam) { return cam && cam->fx != 0.0 && cam->fy != 0.0; }

int gms_gather_points_batch_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs,
                                   int n_pairs, int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1,
                                   float* d_coords2, gms_two_view* d_tv)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_m < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_pairs || !d_results || !d_tv) return GMS_ERR_BAD_ARG;
    if (max_m > 0 && (!d_kp || !d_filtered || !d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_gather_batch(d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1, d_coords2, d_tv,
                                        c->stream);
    });
}

int gms_find_essential_batch_device(gms_ctx* c, const gms_camera* camera, double prob, double threshold, int max_iters, const gms_pair* d_pairs,
                                    int n_pairs, const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (!(prob > 0.0 && prob < 1.0) || !(threshold > 0.0) || max_iters < 1) return GMS_ERR_BAD_ARG;  // (CV_Assert(confidence > 0 && confidence < 1))
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_mask || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_find_essential_batch(*camera, prob, threshold, max_iters, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, c->stream);
    });
}

int gms_recover_pose_batch_device(gms_ctx* c, const gms_camera* camera, int use_in_mask, const gms_pair* d_pairs, int n_pairs,
                                  const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_mask || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_recover_pose_batch(*camera, 50.0, use_in_mask ? 1 : 0, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, c->stream);
    });
}

int gms_triangulate_batch_device(gms_ctx* c, const gms_camera* camera, const gms_pair* d_pairs, int n_pairs, const float* d_coords1,
                                 const float* d_coords2, const uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_points3d || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_triangulate_batch(*camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_points3d, d_tv, c->stream);
    });
}

int gms_two_view_batch_device(gms_ctx* c, const gms_camera* camera, double prob, double threshold, int max_iters, const gms_keypoint* d_kp,
                              const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_m,
                              const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1, float* d_coords2,
                              uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv)
{
    GMS_TRY(gms_gather_points_batch_device(c, d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1, d_coords2, d_tv));
    GMS_TRY(gms_find_essential_batch_device(c, camera, prob, threshold, max_iters, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv));
    GMS_TRY(gms_recover_pose_batch_device(c, camera, 1, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv));
    return gms_triangulate_batch_device(c, camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_points3d, d_tv);
}

int gms_disparity_batch_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off, const int32_t* d_wh, int n_frames,
                               const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results,
                               const uint8_t* d_gt, int64_t gt_stride, int disp_ratio, uint8_t* d_disparity, int64_t map_stride, uint32_t* d_work,
                               gms_disparity_stats* d_stats)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_m < 0 || map_stride <= 0 || gt_stride < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_wh || !d_pairs || !d_results || !d_disparity || !d_work || !d_stats || (d_gt && disp_ratio == 0)) return GMS_ERR_BAD_ARG;
    if (max_m > 0 && (!d_kp || !d_filtered)) return GMS_ERR_BAD_ARG;
    if (max_m >= (1 << 24)) return GMS_ERR_CAPACITY;  // the scatter key keeps the match index in 24 bits
    return on_ctx(c, [&] {
        return gms::launch_disparity_batch(d_kp, d_frame_off, d_wh, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_gt, gt_stride,
                                           disp_ratio, d_disparity, map_stride, d_work, d_stats, c->stream);
    });
}

// ---- many views into one frame (sfm_register_kernels.hip; the plan and the arithmetic are sfm_register_core.h) ----------------------
int gms_sfm_plan(const gms_pair* pairs, int n_pairs, int n_frames, int root, gms_sfm_plan_entry* plan)
{
    if (n_pairs < 0 || n_frames < 1 || (n_pairs > 0 && (!pairs || !plan))) return GMS_ERR_BAD_ARG;
    std::vector<int32_t> reg_by((size_t)n_frames);
    return sfr::plan(pairs, n_pairs, n_frames, root, reg_by.data(), plan) ? GMS_OK : GMS_ERR_BAD_ARG;
}

static bool sfm_register_sizes_ok(int n_frames, int n_pairs, int64_t total_kp, int64_t total_matches)
{
    return n_frames >= 1 && n_pairs >= 0 && total_kp >= 0 && total_kp < INT32_MAX && total_matches >= 0 && total_matches < ((int64_t)1 << 40);
}

// a pair's match range as the host one-shots take it: m >= 0, match_off >= 0 and an end within the 2^40 that sfm_register_sizes_ok
// allows -- match_off is held against 2^40 - m, so that match_off + m is formed only where it fits
static bool sfm_match_range_ok(const gms_pair& pr)
{
    return pr.m >= 0 && pr.match_off >= 0 && pr.match_off <= ((int64_t)1 << 40) - (int64_t)pr.m;
}

size_t gms_sfm_register_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t total_matches)
{
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches)) return 0;
    return gms::sfm_register_ws_bytes(n_pairs, total_kp, total_matches);
}

int gms_sfm_register_keep_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                            const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                            const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links, void* d_ws,
                            size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world, int32_t* d_track,
                            int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                            double* d_cloud_spread, gms_sfm_summary* d_summary, const uint8_t* d_keep)
{
    if (!c || !sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches) || max_m < 0 || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (root < 0 || root >= n_frames || min_links < 1 || cloud_cap < 0) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_ws || !d_views || !d_summary) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_plan || !d_tv || !d_reg)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_mask || !d_points3d || !d_points_world || !d_track)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!d_cloud || !d_cloud_id || !d_cloud_obs || !d_cloud_est || !d_cloud_spread)) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || ws_bytes < gms::sfm_register_ws_bytes(n_pairs, total_kp, total_matches)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_sfm_register(d_frame_off, n_frames, total_kp, d_pairs, d_plan, n_pairs, max_m, total_matches, d_filtered, d_mask,
                                        d_points3d, d_tv, root, min_links, d_ws, d_views, d_reg, d_points_world, d_track, cloud_cap, d_cloud,
                                        d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary, c->stream, d_keep);
    });
}

int gms_sfm_register_keep(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                     gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                     int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary, const uint8_t* keep)
{
    if (n_frames < 1 || n_pairs < 0 || !frame_off || !views || !summary || root < 0 || root >= n_frames || min_links < 1 || cloud_cap < 0)
        return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !tv || !reg)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!cloud || !cloud_id || !cloud_obs || !cloud_est || !cloud_spread)) return GMS_ERR_BAD_ARG;
    for (int f = 0; f < n_frames; f++)
        if (frame_off[f] < 0 || frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
    std::vector<gms_sfm_plan_entry> plan((size_t)n_pairs);
    GMS_TRY(gms_sfm_plan(pairs, n_pairs, n_frames, root, plan.data()));
    int64_t total_m = 0;
    int max_m = 0;
    for (int p = 0; p < n_pairs; p++) {
        if (!sfm_match_range_ok(pairs[p])) return GMS_ERR_BAD_ARG;
        total_m = std::max(total_m, pairs[p].match_off + (int64_t)pairs[p].m);
        max_m = std::max(max_m, pairs[p].m);
    }
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_m) || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !mask || !points3d || !points_world || !track)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs, Cc = (size_t)cloud_cap;
    gms::BlockLayout lay;
    const size_t o_off = lay.add(8 * ((size_t)n_frames + 1)), o_pairs = lay.add(sizeof(gms_pair) * P), o_plan = lay.add(sizeof(gms_sfm_plan_entry) * P);
    const size_t o_m = lay.add(sizeof(gms_dmatch) * M), o_mask = lay.add(M), o_pts = lay.add(24 * M), o_tv = lay.add(sizeof(gms_two_view) * P);
    const size_t o_ws = lay.add(gms::sfm_register_ws_bytes(n_pairs, total_kp, total_m)), o_keep = lay.add(keep ? M : 0);
    // the outputs, back to back: cleared as one span
    const size_t o_views = lay.add(sizeof(gms_sfm_view) * (size_t)n_frames), o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P), o_world = lay.add(24 * M);
    const size_t o_track = lay.add(4 * M), o_cloud = lay.add(24 * Cc), o_id = lay.add(4 * Cc), o_obs = lay.add(4 * Cc), o_est = lay.add(4 * Cc);
    const size_t o_spread = lay.add(8 * Cc), o_sum = lay.add(sizeof(gms_sfm_summary));
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * ((size_t)n_frames + 1));
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        blk.in(o_plan, plan.data(), sizeof(gms_sfm_plan_entry) * P);
        blk.in(o_tv, tv, sizeof(gms_two_view) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        blk.in(o_mask, mask, M);
        blk.in(o_pts, points3d, 24 * M);
        if (keep) blk.in(o_keep, keep, M);
    }
    blk.run([&](hipStream_t st) { return hipMemsetAsync(blk.at(o_views), 0, lay.total() - o_views, st); });
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_register(blk.at<int64_t>(o_off), n_frames, total_kp, blk.at<gms_pair>(o_pairs), blk.at<gms_sfm_plan_entry>(o_plan),
                                        n_pairs, max_m, total_m, blk.at<gms_dmatch>(o_m), blk.at<uint8_t>(o_mask), blk.at<double>(o_pts),
                                        blk.at<gms_two_view>(o_tv), root, min_links, blk.at(o_ws), blk.at<gms_sfm_view>(o_views),
                                        blk.at<gms_sfm_pair_reg>(o_reg), blk.at<double>(o_world), blk.at<int32_t>(o_track), cloud_cap,
                                        blk.at<double>(o_cloud), blk.at<int32_t>(o_id), blk.at<int32_t>(o_obs), blk.at<int32_t>(o_est),
                                        blk.at<double>(o_spread), blk.at<gms_sfm_summary>(o_sum), st, keep && M ? blk.at<uint8_t>(o_keep) : nullptr);
    });
    blk.out(views, o_views, sizeof(gms_sfm_view) * (size_t)n_frames);
    if (P) blk.out(reg, o_reg, sizeof(gms_sfm_pair_reg) * P);
    if (M) {
        blk.out(points_world, o_world, 24 * M);
        blk.out(track, o_track, 4 * M);
    }
    if (Cc) {
        blk.out(cloud, o_cloud, 24 * Cc);
        blk.out(cloud_id, o_id, 4 * Cc);
        blk.out(cloud_obs, o_obs, 4 * Cc);
        blk.out(cloud_est, o_est, 4 * Cc);
        blk.out(cloud_spread, o_spread, 8 * Cc);
    }
    blk.out(summary, o_sum, sizeof(gms_sfm_summary));
    return blk.finish();
}

// the calls without a keep plane: the same launches with a null plane
int gms_sfm_register_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                            const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                            const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links, void* d_ws,
                            size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world, int32_t* d_track,
                            int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                            double* d_cloud_spread, gms_sfm_summary* d_summary)
{
    return gms_sfm_register_keep_device(c, d_frame_off, n_frames, total_kp, d_pairs, d_plan, n_pairs, max_m, total_matches, d_filtered, d_mask,
                                        d_points3d, d_tv, root, min_links, d_ws, ws_bytes, d_views, d_reg, d_points_world, d_track, cloud_cap,
                                        d_cloud, d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary, nullptr);
}

int gms_sfm_register(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                     gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                     int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary)
{
    return gms_sfm_register_keep(frame_off, n_frames, pairs, n_pairs, filtered, mask, points3d, tv, root, min_links, views, reg, points_world,
                                 track, cloud_cap, cloud, cloud_id, cloud_obs, cloud_est, cloud_spread, summary, nullptr);
}

// ---- one-to-one matches per pair (match_unique_kernels.hip; the rule is match_unique_core.h) ----------------------------------------
size_t gms_match_unique_workspace_bytes(int n_pairs, int64_t total_kp, int64_t total_matches)
{
    if (!sfm_register_sizes_ok(1, n_pairs, total_kp, total_matches)) return 0;
    return gms::match_unique_ws_bytes(total_matches);
}

int gms_match_unique_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                            int max_m, int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_two_view* d_tv,
                            void* d_ws, size_t ws_bytes, uint8_t* d_keep, int32_t* d_counts)
{
    if (!c || !sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches) || max_m < 0 || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_ws) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_counts)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_keep)) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || ws_bytes < gms::match_unique_ws_bytes(total_matches)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_match_unique(d_frame_off, n_frames, total_kp, d_pairs, n_pairs, max_m, total_matches, d_filtered, d_mask, d_tv, d_ws,
                                        d_keep, d_counts, c->stream);
    });
}

int gms_match_unique(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const gms_two_view* tv, uint8_t* keep, int32_t* counts)
{
    if (n_frames < 1 || n_pairs < 0 || !frame_off) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !counts)) return GMS_ERR_BAD_ARG;
    for (int f = 0; f < n_frames; f++)
        if (frame_off[f] < 0 || frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
    int64_t total_m = 0;
    int max_m = 0;
    for (int p = 0; p < n_pairs; p++) {
        if (pairs[p].frame_a < 0 || pairs[p].frame_a >= n_frames || pairs[p].frame_b < 0 || pairs[p].frame_b >= n_frames) return GMS_ERR_BAD_ARG;
        if (!sfm_match_range_ok(pairs[p])) return GMS_ERR_BAD_ARG;
        total_m = std::max(total_m, pairs[p].match_off + (int64_t)pairs[p].m);
        max_m = std::max(max_m, pairs[p].m);
    }
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_m) || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !keep)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs;
    gms::BlockLayout lay;
    const size_t o_off = lay.add(8 * ((size_t)n_frames + 1)), o_pairs = lay.add(sizeof(gms_pair) * P), o_m = lay.add(sizeof(gms_dmatch) * M);
    const size_t o_mask = lay.add(mask ? M : 0), o_tv = lay.add(tv ? sizeof(gms_two_view) * P : 0), o_ws = lay.add(gms::match_unique_ws_bytes(total_m));
    const size_t o_keep = lay.add(M), o_counts = lay.add(8 * P);  // the outputs, back to back: cleared as one span
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * ((size_t)n_frames + 1));
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        if (tv) blk.in(o_tv, tv, sizeof(gms_two_view) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        if (mask) blk.in(o_mask, mask, M);
    }
    if (lay.total() > o_keep) blk.run([&](hipStream_t st) { return hipMemsetAsync(blk.at(o_keep), 0, lay.total() - o_keep, st); });
    blk.run([&](hipStream_t st) {
        return gms::launch_match_unique(blk.at<int64_t>(o_off), n_frames, total_kp, blk.at<gms_pair>(o_pairs), n_pairs, max_m, total_m,
                                        blk.at<gms_dmatch>(o_m), mask && M ? blk.at<uint8_t>(o_mask) : nullptr,
                                        tv && P ? blk.at<gms_two_view>(o_tv) : nullptr, blk.at(o_ws), blk.at<uint8_t>(o_keep),
                                        blk.at<int32_t>(o_counts), st);
    });
    if (M) blk.out(keep, o_keep, M);
    if (P) blk.out(counts, o_counts, 8 * P);
    return blk.finish();
}

// ---- bundle adjustment behind the registration (sfm_ba_kernels.hip; the arithmetic is sfm_ba_core.h) --------------------------------
static bool sfm_ba_sizes_ok(int n_frames, int n_pairs, int64_t total_kp, int64_t cloud_cap)
{
    return n_frames >= 1 && n_frames <= (1 << 24) && n_pairs >= 0 && total_kp >= 0 && total_kp < INT32_MAX && cloud_cap >= 0 && cloud_cap < INT32_MAX;
}

size_t gms_sfm_ba_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t cloud_cap)
{
    if (!sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap)) return 0;
    return gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap);
}

int gms_sfm_ba_device(gms_ctx* c, const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* d_kp,
                      const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                      int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_sfm_view* d_views,
                      const gms_sfm_pair_reg* d_reg, const int32_t* d_track, int64_t cloud_cap, const double* d_cloud,
                      const int32_t* d_cloud_id, const gms_sfm_summary* d_reg_summary, void* d_ws, size_t ws_bytes,
                      gms_sfm_view* d_views_out, double* d_cloud_out, int32_t* d_track_status, gms_sfm_ba_summary* d_summary)
{
    if (!c || !camera || !params || !sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap) || !sba::params_ok(*params)) return GMS_ERR_BAD_ARG;
    if (total_matches < 0 || total_matches >= ((int64_t)1 << 40)) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_views || !d_reg_summary || !d_ws || !d_views_out || !d_summary) return GMS_ERR_BAD_ARG;
    if (total_kp > 0 && !d_kp) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_reg)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_mask || !d_track)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!d_cloud || !d_cloud_id || !d_cloud_out || !d_track_status)) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 255u) || ws_bytes < gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_sfm_ba(*camera, *params, d_kp, d_frame_off, n_frames, total_kp, d_pairs, n_pairs, total_matches, d_filtered, d_mask,
                                  d_views, d_reg, d_track, cloud_cap, d_cloud, d_cloud_id, d_reg_summary, d_ws, d_views_out, d_cloud_out,
                                  d_track_status, d_summary, c->stream);
    });
}

int gms_sfm_ba(const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* kp, const int64_t* frame_off, int n_frames,
               const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered, const uint8_t* mask, const gms_sfm_view* views,
               const gms_sfm_pair_reg* reg, const int32_t* track, int64_t cloud_cap, const double* cloud, const int32_t* cloud_id,
               int64_t n_tracks, gms_sfm_view* views_out, double* cloud_out, int32_t* track_status, gms_sfm_ba_summary* summary)
{
    if (!camera || !params || n_frames < 1 || n_pairs < 0 || !frame_off || !views || !views_out || !summary || cloud_cap < 0 || n_tracks < 0 ||
        !sba::params_ok(*params))
        return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !reg)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!cloud || !cloud_id || !cloud_out || !track_status)) return GMS_ERR_BAD_ARG;
    for (int f = 0; f < n_frames; f++)
        if (frame_off[f] < 0 || frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
    int64_t total_m = 0;
    for (int p = 0; p < n_pairs; p++) {
        if (!sfm_match_range_ok(pairs[p])) return GMS_ERR_BAD_ARG;
        total_m = std::max(total_m, pairs[p].match_off + (int64_t)pairs[p].m);
    }
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap) || total_m >= ((int64_t)1 << 40)) return GMS_ERR_BAD_ARG;
    if (total_kp > 0 && !kp) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !mask || !track)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs, Cc = (size_t)cloud_cap, K = (size_t)total_kp, F = (size_t)n_frames;
    gms_sfm_summary rs = {};
    rs.n_tracks = n_tracks;
    gms::BlockLayout lay;
    const size_t o_kp = lay.add(sizeof(gms_keypoint) * K), o_off = lay.add(8 * (F + 1)), o_pairs = lay.add(sizeof(gms_pair) * P);
    const size_t o_m = lay.add(sizeof(gms_dmatch) * M), o_mask = lay.add(M), o_views = lay.add(sizeof(gms_sfm_view) * F);
    const size_t o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P), o_track = lay.add(4 * M), o_cloud = lay.add(24 * Cc), o_id = lay.add(4 * Cc);
    const size_t o_rs = lay.add(sizeof(gms_sfm_summary)), o_ws = lay.add(gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap));
    const size_t o_vout = lay.add(sizeof(gms_sfm_view) * F), o_cout = lay.add(24 * Cc), o_st = lay.add(4 * Cc), o_sum = lay.add(sizeof(gms_sfm_ba_summary));
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * (F + 1));
    blk.in(o_views, views, sizeof(gms_sfm_view) * F);
    blk.in(o_rs, &rs, sizeof(rs));
    if (K) blk.in(o_kp, kp, sizeof(gms_keypoint) * K);
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        blk.in(o_reg, reg, sizeof(gms_sfm_pair_reg) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        blk.in(o_mask, mask, M);
        blk.in(o_track, track, 4 * M);
    }
    if (Cc) {
        blk.in(o_cloud, cloud, 24 * Cc);
        blk.in(o_id, cloud_id, 4 * Cc);
    }
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_ba(*camera, *params, blk.at<gms_keypoint>(o_kp), blk.at<int64_t>(o_off), n_frames, total_kp,
                                  blk.at<gms_pair>(o_pairs), n_pairs, total_m, blk.at<gms_dmatch>(o_m), blk.at<uint8_t>(o_mask),
                                  blk.at<gms_sfm_view>(o_views), blk.at<gms_sfm_pair_reg>(o_reg), blk.at<int32_t>(o_track), cloud_cap,
                                  blk.at<double>(o_cloud), blk.at<int32_t>(o_id), blk.at<gms_sfm_summary>(o_rs), blk.at(o_ws),
                                  blk.at<gms_sfm_view>(o_vout), blk.at<double>(o_cout), blk.at<int32_t>(o_st), blk.at<gms_sfm_ba_summary>(o_sum), st);
    });
    blk.out(views_out, o_vout, sizeof(gms_sfm_view) * F);
    if (Cc) {
        blk.out(cloud_out, o_cout, 24 * Cc);
        blk.out(track_status, o_st, 4 * Cc);
    }
    blk.out(summary, o_sum, sizeof(gms_sfm_ba_summary));
    return blk.finish();
}

// ---- pair records from a view array (sfm_pair_pose_kernels.hip; the arithmetic is sfm_pair_pose_core.h) -------------
int gms_sfm_pair_poses_device(gms_ctx* c, const gms_sfm_view* d_views, int n_frames, const gms_pair* d_pairs, int n_pairs, gms_two_view* d_tv_out,
                              gms_sfm_pair_reg* d_reg_out)
{
    if (!c || !ppose::call_args_ok(n_frames, n_pairs)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_views || !d_pairs || !d_tv_out || !d_reg_out) return GMS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(d_views) & 7u) || (reinterpret_cast<uintptr_t>(d_pairs) & 7u) || (reinterpret_cast<uintptr_t>(d_tv_out) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_reg_out) & 7u))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_sfm_pair_poses(d_views, n_frames, d_pairs, n_pairs, d_tv_out, d_reg_out, c->stream); });
}

int gms_sfm_pair_poses(const gms_sfm_view* views, int n_frames, const gms_pair* pairs, int n_pairs, gms_two_view* tv_out, gms_sfm_pair_reg* reg_out)
{
    if (!ppose::call_args_ok(n_frames, n_pairs)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!views || !pairs || !tv_out || !reg_out) return GMS_ERR_BAD_ARG;
    const size_t F = (size_t)n_frames, P = (size_t)n_pairs;
    gms::BlockLayout lay;
    const size_t o_views = lay.add(sizeof(gms_sfm_view) * F), o_pairs = lay.add(sizeof(gms_pair) * P), o_tv = lay.add(sizeof(gms_two_view) * P),
                 o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P);
    DevBlock blk(lay, nullptr);
    blk.in(o_views, views, sizeof(gms_sfm_view) * F);
    blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_pair_poses(blk.at<gms_sfm_view>(o_views), n_frames, blk.at<gms_pair>(o_pairs), n_pairs, blk.at<gms_two_view>(o_tv),
                                          blk.at<gms_sfm_pair_reg>(o_reg), st);
    });
    blk.out(tv_out, o_tv, sizeof(gms_two_view) * P);
    blk.out(reg_out, o_reg, sizeof(gms_sfm_pair_reg) * P);
    return blk.finish();
}

size_t gms_detect_workspace_bytes(int width, int height, int n_images, int max_keypoints)
{
    return gms::detect_workspace_bytes(width, height, n_images, max_keypoints);
}

static bool detect_image_ok(int width, int height)
{
    return width > 2 * GMS_DETECT_BORDER && height > 2 * GMS_DETECT_BORDER && width <= 65535 && height <= 65535;
}

int gms_detect_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                            void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors, int32_t* d_counts)
{
    if (!c || n_images < 0 || max_keypoints < 0 || threshold < 0 || threshold > 254 || !detect_image_ok(width, height)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_workspace || !d_counts || (max_keypoints > 0 && (!d_keypoints || !d_descriptors))) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, n_images, max_keypoints)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect(d_images, n_images, width, height, threshold, max_keypoints, d_workspace, d_keypoints, d_descriptors, d_counts,
                                  c->stream);
    });
}

int gms_describe_device(gms_ctx* c, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n,
                        void* d_workspace, size_t workspace_bytes, uint8_t* d_descriptors, int32_t* d_status)
{
    if (!c || n < 0 || !detect_image_ok(width, height) || !d_image || !d_workspace || !d_status) return GMS_ERR_BAD_ARG;
    if (n > 0 && (!d_keypoints || !d_descriptors)) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, 1, 0)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_describe(d_image, width, height, d_keypoints, n, d_workspace, d_descriptors, d_status, c->stream); });
}

// ---- pyramid keypoint source (detect_kernels.hip) -------------------------------------------------------------------------------
int gms_pyramid_level_sizes(int width, int height, int n_levels, int32_t* widths, int32_t* heights)
{
    if (n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS || !detect_image_ok(width, height) || !widths || !heights) return GMS_ERR_BAD_ARG;
    return gms::pyramid_level_sizes(width, height, n_levels, widths, heights);
}

int gms_pyramid_build_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int n_levels, uint8_t* d_levels,
                             size_t levels_bytes)
{
    if (!c || n_images < 0 || n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS || !detect_image_ok(width, height)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    const size_t need = gms::pyramid_bytes(width, height, n_images, n_levels);
    if (!d_images || levels_bytes < need || (need > 0 && !d_levels)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_pyramid_build(d_images, n_images, width, height, n_levels, d_levels, c->stream); });
}

// what the batch calls of the keypoint source check first: the context, the counts, the detector's strength and the image size
static bool detect_scalars_ok(const gms_ctx* c, int n_images, int width, int height, int strength, int max_strength)
{
    return c && n_images >= 0 && strength >= 0 && strength <= max_strength && detect_image_ok(width, height);
}

static bool misaligned8(const float* p) { return reinterpret_cast<uintptr_t>(p) % 8 != 0; }   // the 128-float rows are stored two floats at a time
static bool rows128_ok(const float* d_rows128) { return d_rows128 && !misaligned8(d_rows128); }

static size_t pyramid_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels, bool refined)
{
    return detect_image_ok(width, height) ? gms::detect_pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, refined) : 0;
}

// The four pyramid calls. max_strength: the bound of run.strength. rows128_bad: the caller's own rule for d_rows128 refuses it (looked at
// behind the early return of an empty batch, like every pointer).
static int detect_pyramid(gms_ctx* c, const gms::PyramidRun& run, int max_strength, const uint8_t* d_images, int n_images, int width, int height,
                          int max_keypoints, int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints,
                          uint8_t* d_descriptors, int32_t* d_counts, int32_t* d_level_counts, float* d_rows128, bool rows128_bad)
{
    if (!detect_scalars_ok(c, n_images, width, height, run.strength, max_strength) || max_keypoints < 0) return GMS_ERR_BAD_ARG;
    if (n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_workspace || !d_counts || !d_level_counts || rows128_bad) return GMS_ERR_BAD_ARG;
    if (max_keypoints > 0 && (!d_keypoints || !d_descriptors)) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, run.refined)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect_pyramid(run, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace, d_keypoints, d_descriptors,
                                          max_keypoints > 0 ? d_rows128 : nullptr, d_counts, d_level_counts, c->stream);
    });
}

size_t gms_detect_pyramid_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);
}

int gms_detect_pyramid_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                                    int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                    int32_t* d_counts, int32_t* d_level_counts)
{
    return detect_pyramid(c, {gms::PyramidRun::kFast, threshold, false}, 254, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace,
                          workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, nullptr, false);
}

// ---- gradient descriptor (grad_desc_kernels.hip): fused into the pyramid call, no workspace region of its own ----------------------
size_t gms_detect_pyramid_grad_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);
}

int gms_detect_pyramid_grad_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                                         int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                         int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    const bool rows128_bad = max_keypoints > 0 && !rows128_ok(d_rows128);   // required, but only where a row can be written
    return detect_pyramid(c, {gms::PyramidRun::kFast, threshold, false}, 254, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace,
                          workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, rows128_bad);
}

int gms_describe_grad_device(gms_ctx* c, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n, void* d_workspace,
                             size_t workspace_bytes, float* d_rows128, int32_t* d_status)
{
    if (!c || n < 0 || !detect_image_ok(width, height) || !d_image || !d_workspace || !d_status) return GMS_ERR_BAD_ARG;
    if (n > 0 && (!d_keypoints || !rows128_ok(d_rows128))) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, 1, 0)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_describe_grad(d_image, width, height, d_keypoints, n, d_workspace, d_rows128, d_status, c->stream); });
}

// ---- difference-of-Gaussians detector (dog_kernels.hip): d_rows128 is optional, but never misaligned -------------------------------
size_t gms_detect_dog_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);   // the kernel is fused: no region of its own
}

int gms_detect_dog_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, int max_keypoints,
                                int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    return detect_pyramid(c, {gms::PyramidRun::kDog, contrast, false}, GMS_DOG_MAX_CONTRAST, d_images, n_images, width, height, max_keypoints, n_levels,
                          d_workspace, workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, misaligned8(d_rows128));
}

size_t gms_detect_dog_refined_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, true);   // + the plane of refinement codes
}

int gms_detect_dog_refined_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, int max_keypoints,
                                        int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                        int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    return detect_pyramid(c, {gms::PyramidRun::kDog, contrast, true}, GMS_DOG_MAX_CONTRAST, d_images, n_images, width, height, max_keypoints, n_levels,
                          d_workspace, workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, misaligned8(d_rows128));
}

int gms_dog_offsets_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint16_t* d_codes)
{
    if (!detect_scalars_ok(c, n_images, width, height, contrast, GMS_DOG_MAX_CONTRAST)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_codes || reinterpret_cast<uintptr_t>(d_codes) % 2 != 0) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_dog_maps(d_images, n_images, width, height, contrast, nullptr, nullptr, nullptr, d_codes, c->stream); });
}

int gms_dog_candidates_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint8_t* d_cand)
{
    if (!detect_scalars_ok(c, n_images, width, height, contrast, GMS_DOG_MAX_CONTRAST)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_cand) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_dog_maps(d_images, n_images, width, height, contrast, d_cand, nullptr, nullptr, nullptr, c->stream); });
}

// ---- from photographs to the tables (ingest_kernels.hip) ----------------------------------------------------------------------------
int gms_bgr_to_gray_device(gms_ctx* c, const uint8_t* d_bgr, int n_images, int width, int height, uint8_t* d_gray)
{
    if (!c || n_images < 0 || width <= 0 || height <= 0 || width > 65535 || height > 65535) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_bgr || !d_gray) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_bgr_to_gray(d_bgr, n_images, width, height, d_gray, c->stream); });
}

int gms_detect_pack_device(gms_ctx* c, const gms_keypoint* d_keypoint_blocks, const uint8_t* d_rows32_blocks, const float* d_rows128_blocks,
                           const int32_t* d_counts, int n_images, int max_keypoints, gms_keypoint* d_keypoints, uint8_t* d_rows32,
                           float* d_rows128, int64_t* d_frame_off)
{
    if (!c || n_images < 1 || n_images > 65535 || max_keypoints < 0 || !d_counts || !d_frame_off) return GMS_ERR_BAD_ARG;
    if ((d_rows32_blocks == nullptr) != (d_rows32 == nullptr) || (d_rows128_blocks == nullptr) != (d_rows128 == nullptr)) return GMS_ERR_BAD_ARG;
    if (max_keypoints > 0 && (!d_keypoint_blocks || !d_keypoints)) return GMS_ERR_BAD_ARG;
    for (const void* p : {(const void*)d_keypoint_blocks, (const void*)d_rows32_blocks, (const void*)d_rows128_blocks, (const void*)d_counts,
                          (const void*)d_keypoints, (const void*)d_rows32, (const void*)d_rows128})
        if (reinterpret_cast<uintptr_t>(p) & 3u) return GMS_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(d_frame_off) & 7u) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect_pack(d_keypoint_blocks, d_rows32_blocks, d_rows128_blocks, d_counts, n_images, max_keypoints, d_keypoints, d_rows32,
                                       d_rows128, d_frame_off, c->stream);
    });
}

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
    if (total_kp > INT32_MAX || (reinterpret_cast<uintptr_t>(d_table) & 15u)) return GMS_ERR_BAD_ARG;
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
    if ((int64_t)ws_bytes < gms::logos::filter_fixed_bytes(n_pairs) || (reinterpret_cast<uintptr_t>(d_workspace) & 15u)) return GMS_ERR_BAD_ARG;
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
    for (int f = 0; f < n_frames; f++) {
        if (frame_off[f + 1] < frame_off[f]) return GMS_ERR_BAD_ARG;
        max_kp = std::max(max_kp, frame_off[f + 1] - frame_off[f]);
    }
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
    if (ws_bytes < gms::logos_dict_ws_bytes(p) || (reinterpret_cast<uintptr_t>(d_workspace) & 15u)) return GMS_ERR_BAD_ARG;
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

int gms_selftest_five_point(gms_ctx* c, const double* pts, int n_samples, double* models, int32_t* counts)
{
    if (!c || n_samples < 0 || (n_samples > 0 && (!pts || !models || !counts))) return GMS_ERR_BAD_ARG;
    if (n_samples == 0) return GMS_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    const size_t b_pts = (size_t)n_samples * 20 * 8, b_models = (size_t)n_samples * 90 * 8, b_counts = (size_t)n_samples * 4;
    GMS_HIP(hipStreamSynchronize(c->stream));
    GMS_HIP(c->aux.reserve(b_pts + b_models + b_counts));
    double* d_pts = (double*)c->aux.p;
    double* d_models = d_pts + (size_t)n_samples * 20;
    int* d_counts = (int*)(d_models + (size_t)n_samples * 90);
    GMS_HIP(hipMemcpyAsync(d_pts, pts, b_pts, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(gms::launch_five_point_selftest(d_pts, n_samples, d_models, d_counts, c->stream));
    GMS_HIP(hipMemcpyAsync(models, d_models, b_models, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipMemcpyAsync(counts, d_counts, b_counts, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipStreamSynchronize(c->stream));
    return GMS_OK;
}

int gms_selftest_threshold(gms_ctx* c, const int32_t* T, const int32_t* n, const int32_t* score, double factor,
                           int count, uint8_t* out)
{
    if (!c || count < 0 || (count > 0 && (!T || !n || !score || !out))) return GMS_ERR_BAD_ARG;
    if (count == 0) return GMS_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    const size_t nb = (size_t)count * 4;
    GMS_HIP(c->aux.reserve(3 * nb + (size_t)count));
    int32_t* dT = (int32_t*)c->aux.p;
    int32_t* dn = dT + count;
    int32_t* ds = dn + count;
    uint8_t* dout = (uint8_t*)(ds + count);
    GMS_HIP(hipMemcpyAsync(dT, T, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(hipMemcpyAsync(dn, n, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(hipMemcpyAsync(ds, score, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(gms::launch_threshold(dT, dn, ds, factor, count, dout, c->stream));
    GMS_HIP(hipMemcpyAsync(out, dout, (size_t)count, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipStreamSynchronize(c->stream));
    return GMS_OK;
}

}  // extern "C"
