// logos_dict_core.h -- what the LOGOS dictionary trainer (logos_dict_kernels.hip, gms_logos_dict_train_device; DESIGN.md §6b,
// "Training the dictionary") shares between the device and a host build: the counter-based draws, the distances of the words call
// and their integer weights, the quantised mean, and the workspace layout. tests/cpp/logos_dict_host.cpp compiles this file with
// the host compiler and tests/logos_dict_ref.py states the same arithmetic in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef GMS_HD
#if defined(__HIPCC__)
#define GMS_HD __host__ __device__ __forceinline__
#else
#define GMS_HD inline
#endif
#endif

namespace gms {
namespace logos_dict {

constexpr int kChunk = 256;                 // rows of a set per workgroup of the row-parallel kernels
constexpr int kTrials = 3;                  // candidates per centre (cv::kmeans' k-means++)
constexpr int64_t kMaxSetRows = 1 << 20;    // the domain: with it every sum of weights stays below 2^63 and every S below 2^53
constexpr float kMaxAbs = 4096.0f;          // |x| of an L2 element
constexpr int kMaxAttempts = 16;
constexpr int kMaxIters = 1000;
constexpr int kMaxSets = 65535;
constexpr int kL2Dims = 128, kHammingWords = 8;

// ---- draws: u(seed, set, attempt, centre, trial), no state between calls -----------------------------------------------------------
GMS_HD uint64_t splitmix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

GMS_HD uint64_t draw(uint64_t seed, uint64_t set, uint64_t attempt, uint64_t centre, uint64_t trial)
{
    return splitmix64(splitmix64(splitmix64(splitmix64(splitmix64(seed) + set) + attempt) + centre) + trial);
}

GMS_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- distances (those of gms_logos_words_device) and their integer weights ---------------------------------------------------------
// fp32, per group of four dimensions ((d0 d0 + d1 d1) + d2 d2) + d3 d3, the groups added to the running sum in order; built without
// contraction, so no product is fused into a sum.
GMS_HD float l2_sq(const float* a, const float* b)
{
    float acc = 0.0f;
    for (int g = 0; g < kL2Dims; g += 4) {
        const float d0 = a[g] - b[g], d1 = a[g + 1] - b[g + 1], d2 = a[g + 2] - b[g + 2], d3 = a[g + 3] - b[g + 3];
        const float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
        const float grp = ((s0 + s1) + s2) + s3;
        acc = acc + grp;
    }
    return acc;
}

GMS_HD uint64_t l2_weight(float d) { return (uint64_t)floorf(d * 256.0f); }  // d 2^8 is exact; d <= 2^33 in the domain

GMS_HD int popcount32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

GMS_HD uint64_t hamming_weight(const uint32_t* a, const uint32_t* b)
{
    int s = 0;
    for (int k = 0; k < kHammingWords; k++) s += popcount32(a[k] ^ b[k]);
    return (uint64_t)s;
}

GMS_HD bool l2_in_domain(float x) { return fabsf(x) <= kMaxAbs; }  // false for NaN and +-inf

// ---- the update ----------------------------------------------------------------------------------------------------------------
GMS_HD int64_t quantise(float x) { return (int64_t)llrint((double)x * 1048576.0); }  // the product is exact in fp64; ties to even
GMS_HD float l2_mean(int64_t sum_q, int64_t count) { return (float)((double)sum_q / ((double)count * 1048576.0)); }
GMS_HD bool majority(int64_t ones, int64_t count) { return 2 * ones > count; }

// ---- workspace ------------------------------------------------------------------------------------------------------------------
struct Params {
    int32_t kind, n_sets, n_words, attempts, max_iters, row_bytes;
    int64_t total_rows;
    uint64_t seed;
};

struct SetInfo {      // [n_sets + 1]; entry n_sets holds the number of chunks of all sets
    int64_t off;      // first row
    int64_t chunk0;   // chunks of the sets before this one (a set that failed its row-count check has none)
    int32_t n;        // rows (0 when the set failed its row-count check)
    int32_t status;
    int32_t rows_given;  // rows between the set's offsets (0 when the offsets are unusable): what a failed set's labels cover
    int32_t usable;      // the offsets lie within [0, total_rows] and do not decrease
};
static_assert(sizeof(SetInfo) == 32, "SetInfo");

struct Seed {         // per (set, attempt): the three candidates of the centre being chosen
    uint64_t pot[kTrials];
    int32_t cand[kTrials];
    int32_t pad[3];
};
static_assert(sizeof(Seed) == 48, "Seed");

struct Layout {
    int64_t set, centres, minw, labels, bsum, seed, flags, comp, used, total;
    int64_t max_chunks, flag_bytes;
};

GMS_HD int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

GMS_HD Layout layout(const Params& p)
{
    Layout L;
    const int64_t units = (int64_t)p.n_sets * p.attempts;
    L.max_chunks = (p.total_rows + kChunk - 1) / kChunk + p.n_sets;
    int64_t o = 0;
    L.set = o;
    o = align16(o + (int64_t)sizeof(SetInfo) * ((int64_t)p.n_sets + 1));
    L.centres = o;
    o = align16(o + units * p.n_words * p.row_bytes);
    L.minw = o;
    o = align16(o + 8 * p.attempts * p.total_rows);
    L.labels = o;
    o = align16(o + 4 * p.attempts * p.total_rows);
    L.bsum = o;
    o = align16(o + 8 * p.attempts * L.max_chunks);
    L.seed = o;
    o = align16(o + (int64_t)sizeof(Seed) * units);
    L.flags = o;  // int32 [units][max_iters]: 1 when assignment `it` changed a label; cleared, with comp, at the start of a call
    o = align16(o + 4 * units * p.max_iters);
    L.comp = o;   // uint64 [units][max_iters]: the sum of the weights of assignment `it`
    o = align16(o + 8 * units * p.max_iters);
    L.flag_bytes = o - L.flags;
    L.used = o;   // int32 [n_sets][n_words]
    o = align16(o + 4 * (int64_t)p.n_sets * p.n_words);
    L.total = o;
    return L;
}

GMS_HD bool params_ok(const Params& p)
{
    return (p.kind == 0 || p.kind == 1) && p.n_sets >= 0 && p.n_sets <= kMaxSets && p.n_words >= 1 && p.n_words <= 65535 && p.attempts >= 1 &&
           p.attempts <= kMaxAttempts && p.max_iters >= 1 && p.max_iters <= kMaxIters && p.total_rows >= 0 &&
           p.total_rows <= ((int64_t)1 << 31) - 1;
}

}  // namespace logos_dict
}  // namespace gms
