// copy_pool_stress.cpp -- CPU stress test of gms::CopyPool (sfm-gms_amd/csrc/copy_pool.h), the host staging pool of
// gms_filter_host_batch. tests/test_copy_pool.py builds it with g++ (plain and under ThreadSanitizer) and runs it.
//
// The pool's hook sites sleep 0-3 ms on about one call in four (seeded per thread), so that workers are "descheduled" at the
// points where a generation hand-off can go wrong; the pool has more workers than the machine has cores. Job lists alternate
// between long (tens of 1 MB parts) and tiny ones (2-3 parts), with the early-return paths (no jobs, zero bytes, one part),
// memcpy and pack_xy jobs mixed, and one shutdown() + restart. Before each run every destination byte -- and the gaps between
// destinations -- holds a sentinel; after it every byte is checked.
//
//   copy_pool_stress [runs] [seed] [workers] [long_mb] [sleep_us]
//     long_mb: a long list holds long_mb / 2 .. long_mb MB (default 44); sleep_us: the longest sleep of a hook (default 3000).
//     Under ThreadSanitizer, where copies and checks are slow, shorter lists and longer sleeps keep the same overlap of runs.
//     exit 0: all runs correct; 1: a run left wrong bytes; 3: a run hung (watchdog)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "gms.h"

namespace {
std::atomic<unsigned> g_thread_seq{0};
unsigned g_seed = 1;

unsigned g_sleep_us = 3000;

void hook_sleep()
{
    thread_local std::mt19937 rng(g_seed * 7919u + g_thread_seq.fetch_add(1));
    if (rng() % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % g_sleep_us));
}
}  // namespace

#define GMS_COPY_POOL_HOOK(site) hook_sleep()
#include "copy_pool.h"

namespace {
constexpr size_t kMB = (size_t)1 << 20;
constexpr unsigned char kSentinel = 0xA5;
std::atomic<long> g_progress{0};

struct Check {
    size_t dst_off, bytes;
    size_t src_off;  // byte offset into the memcpy source, or keypoint index for pack_xy
    int pack_xy;
};

}  // namespace

int main(int argc, char** argv)
{
    const int runs = argc > 1 ? std::atoi(argv[1]) : 3000;
    g_seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    const unsigned workers = argc > 3 ? (unsigned)std::atoi(argv[3]) : 15u;
    const size_t long_mb = argc > 4 ? (size_t)std::max(std::atoi(argv[4]), 8) : 44u;
    g_sleep_us = argc > 5 ? (unsigned)std::max(std::atoi(argv[5]), 1) : 3000u;
    std::setvbuf(stdout, nullptr, _IOLBF, 0);

    std::thread([] {
        long last = -1;
        auto since = std::chrono::steady_clock::now();
        for (;;) {
            std::this_thread::sleep_for(std::chrono::milliseconds(250));
            const long p = g_progress.load();
            const auto now = std::chrono::steady_clock::now();
            if (p != last) {
                last = p;
                since = now;
            } else if (now - since > std::chrono::seconds(10)) {
                std::printf("HANG after %ld runs\n", p);
                std::fflush(stdout);
                std::_Exit(3);
            }
        }
    }).detach();

    // sources: bytes for memcpy jobs, keypoints for pack_xy jobs (distinct x / y per record)
    const size_t kSrcBytes = (long_mb + 4) * kMB, kDstBytes = (long_mb + 20) * kMB;
    std::vector<unsigned char> src(kSrcBytes);
    for (size_t i = 0; i < kSrcBytes; ++i) src[i] = (unsigned char)(i * 131u + (i >> 13) + 7u);
    const size_t kKp = 6 * kMB / 8;  // up to 6 MB of packed (x, y)
    std::vector<gms_keypoint> kp(kKp);
    std::vector<float> xy(2 * kKp);  // what pack_xy must make of them
    for (size_t i = 0; i < kKp; ++i) {
        kp[i] = gms_keypoint{(float)i + 0.25f, -(float)i - 0.5f, 1.f, 2.f, 3.f, 4, 5};
        xy[2 * i] = (float)i + 0.25f;
        xy[2 * i + 1] = -(float)i - 0.5f;
    }
    const std::vector<unsigned char> fill(kMB, kSentinel);
    std::vector<unsigned char> dst(kDstBytes);

    std::mt19937_64 rng(g_seed);
    auto uni = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };

    gms::CopyPool pool(workers);
    std::vector<gms::CopyJob> jobs;  // one list, cleared and refilled each run (as gms_filter_host_batch does)
    std::vector<Check> checks;
    long bad = 0, early = 0, parts_total = 0;
    for (int r = 0; r < runs; ++r) {
        if (r == runs / 2) pool.shutdown();  // the next run with parts starts the threads again
        jobs.clear();
        checks.clear();
        // the kind of list: mostly long and tiny in turn, now and then an early-return shape
        int kind = (r & 1) ? 1 : 0;              // 0 long, 1 tiny
        if (r % 7 == 3) kind = 2 + (int)(rng() % 3);  // 2 empty list, 3 zero bytes, 4 one part
        size_t target = 0;
        switch (kind) {
        case 0: target = uni(long_mb / 2, long_mb) * kMB + uni(0, kMB - 1); break;
        case 1: target = uni(kMB + 1, 3 * kMB); break;
        case 4: target = uni(1, kMB); break;
        default: break;
        }
        size_t at = 0, src_at = uni(0, 1024) * 8;
        if (kind == 3) {
            for (int j = 0; j < 3; ++j) jobs.push_back(gms::CopyJob{dst.data() + 64 * j, src.data(), 0, j & 1});
        }
        while (at < target) {
            at += uni(0, 3) * 8;                        // a gap the pool must not touch
            size_t bytes = std::min(target - at, (size_t)uni(1, 12) * kMB / uni(1, 8));
            bytes = (bytes + 7) & ~(size_t)7;
            if (rng() % 11 == 0) bytes = 0;             // empty jobs among the others
            if (at + bytes > kDstBytes) break;
            const bool pack = rng() % 3 == 0 && bytes <= kKp * 8;
            if (pack) {
                const size_t k0 = uni(0, kKp - bytes / 8);
                jobs.push_back(gms::CopyJob{dst.data() + at, kp.data() + k0, bytes, 1});
                checks.push_back(Check{at, bytes, k0, 1});
            } else {
                if (src_at + bytes > kSrcBytes) src_at = uni(0, 64) * 8;
                if (src_at + bytes > kSrcBytes) bytes = (kSrcBytes - src_at) & ~(size_t)7;
                jobs.push_back(gms::CopyJob{dst.data() + at, src.data() + src_at, bytes, 0});
                checks.push_back(Check{at, bytes, src_at, 0});
                src_at += bytes;
            }
            at += bytes;
        }
        const size_t span = std::min(at + 64, kDstBytes);
        std::memset(dst.data(), kSentinel, span);
        pool.run(jobs);
        size_t total = 0;
        for (const gms::CopyJob& j : jobs) total += j.bytes;
        if (total <= kMB) ++early;
        parts_total += (long)((total + kMB - 1) / kMB);

        // every byte: destinations hold their source, gaps the sentinel
        auto untouched = [&](size_t lo, size_t hi) {
            for (; lo < hi; lo += std::min(hi - lo, kMB))
                if (std::memcmp(dst.data() + lo, fill.data(), std::min(hi - lo, kMB)) != 0) return false;
            return true;
        };
        bool ok = true;
        size_t covered = 0;
        for (const Check& c : checks) {
            const unsigned char* want = c.pack_xy ? (const unsigned char*)(xy.data() + 2 * c.src_off) : src.data() + c.src_off;
            if (std::memcmp(dst.data() + c.dst_off, want, c.bytes) != 0) {
                size_t i = 0;
                while (dst[c.dst_off + i] == want[i]) ++i;
                std::printf("run %d: %s job at +%zu: byte %zu of %zu wrong\n", r, c.pack_xy ? "pack_xy" : "memcpy", c.dst_off, i, c.bytes);
                ok = false;
                break;
            }
            if (!untouched(covered, c.dst_off)) {
                std::printf("run %d: a byte in front of +%zu, outside every destination, was written\n", r, c.dst_off);
                ok = false;
                break;
            }
            covered = std::max(covered, c.dst_off + c.bytes);
        }
        if (ok && !untouched(covered, span)) {
            std::printf("run %d: a byte behind +%zu, outside every destination, was written\n", r, covered);
            ok = false;
        }
        if (!ok) ++bad;
        g_progress.fetch_add(1);
    }
    // the default worker count, a few runs
    {
        gms::CopyPool def;
        jobs.assign(1, gms::CopyJob{dst.data(), src.data(), 5 * kMB + 3, 0});
        for (int r = 0; r < 4; ++r) {
            std::memset(dst.data(), kSentinel, 6 * kMB);
            def.run(jobs);
            if (std::memcmp(dst.data(), src.data(), 5 * kMB + 3) != 0 || dst[5 * kMB + 3] != kSentinel) ++bad;
        }
    }
    std::printf("%d runs (%ld early-return shapes, %ld parts), %u workers, seed %u: %ld bad runs\n", runs, early, parts_total, workers,
                g_seed, bad);
    return bad ? 1 : 0;
}
