// capi_common.h -- what the host ABI sources (gms_capi.cpp and the capi_*.cpp beside it) share: the error macros, the context, the
// body of a one-launch entry point and the one-shot calls' device block. Internal to csrc/, not installed.
//
// gms_capi.cpp owns the context: of its fields the feature files use mu, device and stream (through on_ctx), and beyond them only
// pose_ws (gms_recover_pose_device), n_cus (the LOGOS calls) and aux (the two self-tests). Everything else belongs to the filter and
// the host-batch pipeline of gms_capi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

#include "block_layout.h"
#include "capi_checks.h"
#include "gms.h"

namespace gms {
class CopyPool;                // copy_pool.h
void record_hip_error(int e);  // gms_capi.cpp: what gms_last_hip_error() reports
}

#define GMS_HIP(call)                             \
    do {                                          \
        hipError_t e_ = (call);                   \
        if (e_ != hipSuccess) {                   \
            gms::record_hip_error((int)e_);       \
            return GMS_ERR_HIP;                   \
        }                                         \
    } while (0)
#define GMS_TRY(call)                \
    do {                             \
        const int rc_ = (call);      \
        if (rc_ != GMS_OK) return rc_; \
    } while (0)

// name(params): the caller's parameters, or where it passes none the defaults of gms.h (`...`: one of its GMS_*_PARAMS_* initialisers)
#define GMS_PARAMS_OR(name, type, ...)        \
    static const type& name(const type* p)    \
    {                                         \
        static const type ref = __VA_ARGS__;  \
        return p ? *p : ref;                  \
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

// stream `st` is being captured into a graph: nothing may be allocated, freed or waited for
inline bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

namespace gms {
// capi_twoview.cpp: the scratch of gms_recover_pose_device, which gms_ctx_reserve also grows ahead of a capture
int grow_pose_ws(gms_ctx* c, size_t bytes, hipStream_t st);
}

inline bool desc_kind_ok(int kind) { return kind == GMS_DESC_HAMMING256 || kind == GMS_DESC_L2_F32X128; }
inline size_t desc_row_bytes(int kind) { return kind == GMS_DESC_HAMMING256 ? 32 : 512; }

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
