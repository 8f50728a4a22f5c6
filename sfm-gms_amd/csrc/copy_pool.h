// copy_pool.h -- host-side staging of gms_filter_host_batch: the copies between the caller's (pageable) arrays and the pinned
// blocks the copy engines work from. Host code only (no HIP): tests/cpp/copy_pool_stress.cpp builds it with g++ alone.
//
// One core moves 25-35 GB/s here, four move 65-110 (tools/ubench/host_copy_rate.cpp), the copy engines 30-55 GB/s per direction:
// the copies of a chunk are cut into parts of 1 MB that a PERSISTENT pool of threads (created with the context's first host batch,
// not per chunk) takes from a shared counter; the calling thread works along.
//
// Test seam: GMS_COPY_POOL_HOOK(site) expands to nothing unless it is defined before this header is included. The sites:
//   0  worker(), after it has taken a generation and released the lock, before its first ticket
//   1  worker(), before it publishes its count
//   2  run(), between publishing a generation and its own ticket loop
#ifndef GMS_COPY_POOL_H
#define GMS_COPY_POOL_H

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "gms.h"

#ifndef GMS_COPY_POOL_HOOK
#define GMS_COPY_POOL_HOOK(site) ((void)0)
#endif

namespace gms {

struct CopyJob {
    void* dst;
    const void* src;
    size_t bytes;   // of dst
    int pack_xy;    // 0: memcpy; 1: src = gms_keypoint records, dst = (pt.x, pt.y) float pairs, 8 bytes each (bytes % 8 == 0)
};

// (pt.x, pt.y) of n keypoints, 8 bytes each: all the filter reads of a cv::KeyPoint (DLL@0x1800485d4) and all that has to
// cross PCIe. Pure data movement; the divide by the image size happens on the GPU (normalize_kernel).
inline void pack_xy(const gms_keypoint* kp, size_t n, float* dst)
{
    for (size_t i = 0; i < n; ++i) {
        dst[2 * i] = kp[i].x;
        dst[2 * i + 1] = kp[i].y;
    }
}

class CopyPool {
public:
    // workers: threads besides the caller; 0 = min(hardware threads, 8) - 1
    explicit CopyPool(unsigned workers = 0) : workers_(workers) {}
    ~CopyPool() { shutdown(); }
    void shutdown()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_work_.notify_all();
        for (std::thread& t : threads_) t.join();
        threads_.clear();
        stop_ = false;
    }
    // Runs the jobs (disjoint destinations) and returns when every byte has landed.
    void run(const std::vector<CopyJob>& jobs)
    {
        if (jobs.empty()) return;
        starts_.resize(jobs.size() + 1);
        starts_[0] = 0;
        for (size_t i = 0; i < jobs.size(); ++i) starts_[i + 1] = starts_[i] + jobs[i].bytes;
        const size_t total = starts_.back();
        if (total == 0) return;
        const unsigned n_parts = (unsigned)((total + kPart - 1) / kPart);
        if (n_parts <= 1) {
            part(jobs, 0);
            return;
        }
        if (threads_.empty()) start();
        {
            std::lock_guard<std::mutex> lk(mu_);
            jobs_ = &jobs;
            n_parts_ = n_parts;
            next_.store(0, std::memory_order_relaxed);
            done_ = 0;
            ++gen_;
        }
        cv_work_.notify_all();
        GMS_COPY_POOL_HOOK(2);
        unsigned mine = 0;
        for (unsigned i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n_parts; ++mine) part(jobs, i);
        std::unique_lock<std::mutex> lk(mu_);
        done_ += mine;
        // no worker may still be in its ticket loop (or reading starts_ / the jobs) when the next run rewrites them
        cv_done_.wait(lk, [&] { return done_ == n_parts_ && active_ == 0; });
        jobs_ = nullptr;
    }

private:
    static constexpr size_t kPart = (size_t)1 << 20;
    void start()
    {
        unsigned hw = std::thread::hardware_concurrency();
        const unsigned n = workers_ ? workers_ : std::min(hw ? hw : 4u, 8u) - 1;   // plus the calling thread
        for (unsigned t = 0; t < n; ++t) threads_.emplace_back([this] { worker(); });
    }
    void worker()
    {
        uint64_t seen = 0;
        for (;;) {
            const std::vector<CopyJob>* jobs;
            unsigned n_parts;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                jobs = jobs_;
                n_parts = n_parts_;
                if (jobs) ++active_;  // counted out together with its parts: run() returns only when this worker is done
            }
            if (!jobs) continue;
            GMS_COPY_POOL_HOOK(0);
            unsigned mine = 0;
            for (unsigned i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n_parts; ++mine) part(*jobs, i);
            GMS_COPY_POOL_HOOK(1);
            std::lock_guard<std::mutex> lk(mu_);
            done_ += mine;
            --active_;
            if (done_ == n_parts_ && active_ == 0) cv_done_.notify_all();
        }
    }
    // bytes [i, i + 1) * kPart of the concatenated destinations
    void part(const std::vector<CopyJob>& jobs, unsigned i) const
    {
        const size_t lo = (size_t)i * kPart, hi = std::min(lo + kPart, starts_.back());
        size_t j = (size_t)(std::upper_bound(starts_.begin(), starts_.end(), lo) - starts_.begin()) - 1;
        for (; j < jobs.size() && starts_[j] < hi; ++j) {
            const size_t a = std::max(lo, starts_[j]) - starts_[j], b = std::min(hi, starts_[j + 1]) - starts_[j];
            if (a >= b) continue;
            if (jobs[j].pack_xy) pack_xy((const gms_keypoint*)jobs[j].src + a / 8, (b - a) / 8, (float*)((char*)jobs[j].dst + a));
            else std::memcpy((char*)jobs[j].dst + a, (const char*)jobs[j].src + a, b - a);
        }
    }
    const unsigned workers_;
    std::vector<std::thread> threads_;
    std::vector<size_t> starts_;
    std::mutex mu_;
    std::condition_variable cv_work_, cv_done_;
    const std::vector<CopyJob>* jobs_ = nullptr;
    unsigned n_parts_ = 0, done_ = 0, active_ = 0;  // active_: workers that took the current generation and have not counted out
    std::atomic<unsigned> next_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
};

}  // namespace gms

#endif
