// logos_dict_kernels.hip -- training the LOGOS visual-word dictionary (gms_logos_dict_train_device; DESIGN.md §6b, "Training the
// dictionary"): batched k-means of descriptor rows whose every order-dependent step is integer arithmetic, so that the result is
// the bytes of the numpy statement tests/logos_dict_ref.py. Stream-ordered, no allocation, no synchronisation, no host read-back:
// capturable. A work unit is (set, attempt); all units run in the same launches.
//
// plan      one workgroup: row counts, statuses and the chunk prefix of the sets; L2 rows are then checked against the domain
// seeding   per centre c = 1 .. k-1: update (minimum weight of every row against centre c-1, sums per chunk) -> pick (one workgroup
//           per unit: scan of the chunk sums, three draws, the row of each) -> potentials (the three candidates' potentials: LDS
//           partial per workgroup, one 64-bit atomic per candidate); the next update, or the final commit, keeps the best candidate
// iterate   assign (the words call's distances; label, weight, "a label changed" per unit and iteration) -> update (one workgroup per
//           (cluster, unit) gathers its members: an exact segmented sum, then the quantised mean / the bit majority). A unit whose
//           assignment changed nothing leaves its flag clear, and every later launch returns at once for it.
// finish    one workgroup per set: iterations and compactness of every attempt, the winner, its dictionary, empty clusters, labels
#include <hip/hip_runtime.h>

#include "gms.h"
#include "gms_kernels.h"
#include "logos_dict_core.h"
#include "logos_words_dist.h"

namespace {

using namespace gms::logos_dict;
using gms::logos::kWordTile;
using gms::logos::l2_words_dist;
using gms::logos::wave_argmin;
constexpr int kBlock = kChunk;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kHammingTile = 512;  // centres per LDS tile of the Hamming assignment
typedef unsigned long long u64;

struct View {
    SetInfo* set;
    char* centres;
    u64* minw;
    int32_t* labels;
    u64* bsum;
    Seed* seed;
    int32_t* flags;
    u64* comp;
    int32_t* used;
    int64_t max_chunks;
};

__device__ __forceinline__ View view(void* ws, const Params& p)
{
    const Layout L = layout(p);
    char* b = static_cast<char*>(ws);
    View v;
    v.set = (SetInfo*)(b + L.set);
    v.centres = b + L.centres;
    v.minw = (u64*)(b + L.minw);
    v.labels = (int32_t*)(b + L.labels);
    v.bsum = (u64*)(b + L.bsum);
    v.seed = (Seed*)(b + L.seed);
    v.flags = (int32_t*)(b + L.flags);
    v.comp = (u64*)(b + L.comp);
    v.used = (int32_t*)(b + L.used);
    v.max_chunks = L.max_chunks;
    return v;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// the sum of v over the workgroup, to every thread
__device__ u64 block_sum(u64 v)
{
    __shared__ u64 part[kWaves];
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_down(v, s);
    __syncthreads();
    if (lane_id() == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    u64 t = 0;
    for (int w = 0; w < kWaves; w++) t += part[w];
    return t;
}

// the set of global chunk g (blockIdx.x of the row-parallel kernels) and the chunk's place in it; false past the last chunk or
// when the set has failed a check
struct Chunk {
    int s, n, rows;      // set, its rows, rows of this chunk
    int64_t off, first;  // the set's first row; this chunk's first row within the set
};

__device__ __forceinline__ bool locate(const View& v, const Params& p, int64_t g, Chunk& c)
{
    int lo = 0, hi = p.n_sets + 1;  // the last s with chunk0[s] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v.set[mid].chunk0 <= g) lo = mid;
        else hi = mid;
    }
    if (lo >= p.n_sets) return false;
    const SetInfo& si = v.set[lo];
    if (si.status != GMS_OK) return false;
    c.s = lo;
    c.n = si.n;
    c.off = si.off;
    c.first = (g - si.chunk0) * kChunk;
    c.rows = (int)min((int64_t)kChunk, (int64_t)si.n - c.first);
    return c.rows > 0;
}

__device__ __forceinline__ int64_t unit_of(const Params& p, int s, int a) { return (int64_t)s * p.attempts + a; }

// the row (within its set) that became centre c of unit (s, a): the first centre's draw, or the best of the three candidates
__device__ __forceinline__ int64_t centre_row(const View& v, const Params& p, int s, int a, int c)
{
    if (c == 0) return (int64_t)mulhi64(draw(p.seed, (uint64_t)s, (uint64_t)a, 0, 0), (uint64_t)v.set[s].n);
    const Seed& sd = v.seed[unit_of(p, s, a)];
    int best = 0;
    for (int t = 1; t < kTrials; t++)
        if (sd.pot[t] < sd.pot[best]) best = t;
    return sd.cand[best];
}

__device__ __forceinline__ u64 row_weight(int kind, const void* row, const void* centre)
{
    if (kind == GMS_DESC_L2_F32X128) return l2_weight(l2_sq(static_cast<const float*>(row), static_cast<const float*>(centre)));
    return hamming_weight(static_cast<const uint32_t*>(row), static_cast<const uint32_t*>(centre));
}

// ========================================================== plan ==========================================================
__global__ void __launch_bounds__(kBlock) plan_kernel(Params p, const int64_t* __restrict__ set_off, void* ws)
{
    const View v = view(ws, p);
    for (int s = threadIdx.x; s < p.n_sets; s += kBlock) {
        const int64_t a = set_off[s], b = set_off[s + 1];
        SetInfo si = {0, 0, 0, GMS_OK, 0, 0};
        if (a < 0 || b < a || b > p.total_rows) {
            si.status = GMS_ERR_BAD_ARG;
        } else {
            si.off = a;
            si.rows_given = (int32_t)(b - a);
            si.usable = 1;
            if (b - a > kMaxSetRows || b - a < p.n_words) si.status = GMS_ERR_BAD_ARG;
            else si.n = (int32_t)(b - a);
        }
        v.set[s] = si;
    }
    __syncthreads();
    // in set order: a set that starts before the end of an earlier set (the offsets decreased somewhere) is refused, so the sets that
    // run are disjoint, no two units share a row of minw / labels, and the chunks stay within max_chunks
    if (threadIdx.x == 0) {
        int64_t run = 0, end = 0;
        for (int s = 0; s < p.n_sets; s++) {
            SetInfo& si = v.set[s];
            if (si.usable) {
                if (si.off < end) {
                    si = SetInfo{0, 0, 0, GMS_ERR_BAD_ARG, 0, 0};
                } else {
                    end = si.off + si.rows_given;
                }
            }
            si.chunk0 = run;
            run += (si.n + kChunk - 1) / kChunk;
        }
        const SetInfo last = {0, run, 0, GMS_ERR_BAD_ARG, 0, 0};
        v.set[p.n_sets] = last;
    }
}

// L2: a row with an element that is not finite or lies outside [-4096, 4096] puts its set outside the domain
__global__ void __launch_bounds__(kBlock) check_l2_kernel(Params p, const float* __restrict__ desc, void* ws)
{
    const View v = view(ws, p);
    Chunk c;
    if (!locate(v, p, blockIdx.x, c)) return;
    const float* x = desc + (c.off + c.first) * kL2Dims;
    bool bad = false;
    for (int e = threadIdx.x; e < c.rows * kL2Dims; e += kBlock) bad |= !l2_in_domain(x[e]);
    if (bad) atomicMin(&v.set[c.s].status, GMS_ERR_DOMAIN);
}

// ========================================================= seeding =========================================================
// centre c-1 is settled here (every workgroup of the unit reads the same three potentials); the unit's first chunk stores it
__global__ void __launch_bounds__(kBlock) seed_update_kernel(Params p, const char* __restrict__ desc, void* ws, int c)
{
    __shared__ uint32_t centre[kL2Dims];
    const View v = view(ws, p);
    Chunk ch;
    if (!locate(v, p, blockIdx.x, ch)) return;
    const int a = blockIdx.y;
    const int64_t u = unit_of(p, ch.s, a);
    const int words = p.row_bytes / 4;
    const uint32_t* src = (const uint32_t*)(desc + (ch.off + centre_row(v, p, ch.s, a, c - 1)) * p.row_bytes);
    if ((int)threadIdx.x < words) {
        centre[threadIdx.x] = src[threadIdx.x];
        if (ch.first == 0) ((uint32_t*)(v.centres + (u * p.n_words + (c - 1)) * p.row_bytes))[threadIdx.x] = src[threadIdx.x];
    }
    __syncthreads();
    u64 w = 0;
    if ((int)threadIdx.x < ch.rows) {
        const int64_t row = ch.off + ch.first + threadIdx.x;
        w = row_weight(p.kind, desc + row * p.row_bytes, centre);
        u64* m = v.minw + (int64_t)a * p.total_rows + row;
        if (c > 1) w = min(w, *m);
        *m = w;
    }
    const u64 sum = block_sum(w);
    if (threadIdx.x == 0) v.bsum[(int64_t)a * v.max_chunks + blockIdx.x] = sum;
}

// one workgroup per unit: exclusive scan of the chunk sums (in place), then wave t draws candidate t: the first row whose inclusive
// prefix of minimum weights exceeds mulhi64(u, total) -- or row mulhi64(u, n) when every weight is zero
__global__ void __launch_bounds__(kBlock) seed_pick_kernel(Params p, void* ws, int c)
{
    __shared__ u64 part[kBlock];
    const View v = view(ws, p);
    const int s = blockIdx.x, a = blockIdx.y, t = threadIdx.x;
    const SetInfo si = v.set[s];
    if (si.status != GMS_OK) return;
    const int64_t nch = v.set[s + 1].chunk0 - si.chunk0;
    u64* E = v.bsum + (int64_t)a * v.max_chunks + si.chunk0;
    const int64_t per = (nch + kBlock - 1) / kBlock;
    const int64_t lo = min(nch, (int64_t)t * per), hi = min(nch, lo + per);
    u64 sum = 0;
    for (int64_t k = lo; k < hi; k++) sum += E[k];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const u64 x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    u64 run = part[t] - sum;
    for (int64_t k = lo; k < hi; k++) {
        const u64 x = E[k];
        E[k] = run;
        run += x;
    }
    const u64 total = part[kBlock - 1];
    __syncthreads();  // the prefix is read by other threads below

    const int trial = t / kWave, lane = lane_id();
    if (trial >= kTrials) return;
    Seed& sd = v.seed[unit_of(p, s, a)];
    const uint64_t draw_u = draw(p.seed, (uint64_t)s, (uint64_t)a, (uint64_t)c, (uint64_t)trial);
    if (lane == 0) sd.pot[trial] = 0;
    if (total == 0) {
        if (lane == 0) sd.cand[trial] = (int32_t)mulhi64(draw_u, (uint64_t)si.n);
        return;
    }
    const u64 r = mulhi64(draw_u, total);
    int64_t b = 0, top = nch;  // the last chunk whose exclusive prefix is <= r: its inclusive prefix exceeds r
    while (top - b > 1) {
        const int64_t mid = (b + top) >> 1;
        if (E[mid] <= r) b = mid;
        else top = mid;
    }
    constexpr int kPer = kChunk / kWave;
    const u64* m = v.minw + (int64_t)a * p.total_rows + si.off;
    const int64_t i0 = b * kChunk + (int64_t)lane * kPer;
    u64 w[kPer], mine = 0;
    for (int j = 0; j < kPer; j++) {
        w[j] = i0 + j < si.n ? m[i0 + j] : 0;
        mine += w[j];
    }
    u64 incl = mine;
    for (int d = 1; d < kWave; d <<= 1) {
        const u64 x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    const uint64_t over = __ballot(E[b] + incl > r);
    if (over == 0) return;  // cannot happen: the chunk's inclusive prefix exceeds r
    if (lane == __ffsll((long long)over) - 1) {
        u64 acc = E[b] + incl - mine;
        for (int j = 0; j < kPer; j++) {
            acc += w[j];
            if (acc > r) {
                sd.cand[trial] = (int32_t)(i0 + j);
                break;
            }
        }
    }
}

// the potential the unit would have with each candidate added
__global__ void __launch_bounds__(kBlock) seed_potential_kernel(Params p, const char* __restrict__ desc, void* ws)
{
    __shared__ uint32_t cand[kTrials][kL2Dims];
    const View v = view(ws, p);
    Chunk ch;
    if (!locate(v, p, blockIdx.x, ch)) return;
    const int a = blockIdx.y;
    Seed& sd = v.seed[unit_of(p, ch.s, a)];
    const int words = p.row_bytes / 4;
    for (int e = threadIdx.x; e < kTrials * words; e += kBlock) {
        const int t = e / words, k = e % words;
        cand[t][k] = ((const uint32_t*)(desc + (ch.off + sd.cand[t]) * p.row_bytes))[k];
    }
    __syncthreads();
    u64 w[kTrials] = {0, 0, 0};
    if ((int)threadIdx.x < ch.rows) {
        const int64_t row = ch.off + ch.first + threadIdx.x;
        const u64 m = v.minw[(int64_t)a * p.total_rows + row];
        for (int t = 0; t < kTrials; t++) w[t] = min(m, row_weight(p.kind, desc + row * p.row_bytes, cand[t]));
    }
    for (int t = 0; t < kTrials; t++) {
        const u64 sum = block_sum(w[t]);
        if (threadIdx.x == 0 && sum) atomicAdd((u64*)&sd.pot[t], sum);
    }
}

// the last centre (the only one when n_words = 1)
__global__ void __launch_bounds__(kL2Dims) seed_commit_kernel(Params p, const char* __restrict__ desc, void* ws, int c)
{
    const View v = view(ws, p);
    const int s = blockIdx.x, a = blockIdx.y;
    const SetInfo si = v.set[s];
    if (si.status != GMS_OK) return;
    const uint32_t* src = (const uint32_t*)(desc + (si.off + centre_row(v, p, s, a, c)) * p.row_bytes);
    if ((int)threadIdx.x < p.row_bytes / 4)
        ((uint32_t*)(v.centres + (unit_of(p, s, a) * p.n_words + c) * p.row_bytes))[threadIdx.x] = src[threadIdx.x];
}

// ======================================================== iterations ========================================================
__device__ __forceinline__ bool unit_active(const View& v, const Params& p, int64_t u, int it)
{
    return it == 0 || v.flags[u * p.max_iters + it - 1] != 0;
}

// what every assignment ends with: the row's label and weight; whether a label of the unit changed; the sum of the weights
__device__ __forceinline__ void assign_tail(const View& v, const Params& p, const Chunk& ch, int a, int it, int label, u64 weight)
{
    const int64_t u = unit_of(p, ch.s, a);
    u64 changed = 0;
    if ((int)threadIdx.x < ch.rows) {
        int32_t* l = v.labels + (int64_t)a * p.total_rows + ch.off + ch.first + threadIdx.x;
        changed = it == 0 || *l != label;
        *l = label;
    } else {
        weight = 0;
    }
    const u64 sum = block_sum(weight);
    const u64 any = block_sum(changed);
    if (threadIdx.x == 0) {
        if (sum) atomicAdd(&v.comp[u * p.max_iters + it], sum);
        if (any) v.flags[u * p.max_iters + it] = 1;
    }
}

// L2: the words kernel's shape -- a tile of 64 centres in LDS, lane l of a wave owns centre (tile + l) of the wave's current row
__global__ void __launch_bounds__(kBlock) assign_l2_kernel(Params p, const float* __restrict__ desc, void* ws, int it)
{
    __shared__ float tile[kL2Dims][kWordTile];
    __shared__ float best_d[kChunk];
    __shared__ int best_w[kChunk];
    const View v = view(ws, p);
    Chunk ch;
    if (!locate(v, p, blockIdx.x, ch)) return;
    const int a = blockIdx.y;
    const int64_t u = unit_of(p, ch.s, a);
    if (!unit_active(v, p, u, it)) return;
    const float* dict = (const float*)(v.centres + u * p.n_words * p.row_bytes);
    const float* rows = desc + (ch.off + ch.first) * kL2Dims;
    const int lane = lane_id(), wv = threadIdx.x / kWave;
    best_d[threadIdx.x] = INFINITY;
    best_w[threadIdx.x] = 0;
    const int n_tiles = (p.n_words + kWordTile - 1) / kWordTile;
    for (int tl = 0; tl < n_tiles; tl++) {
        __syncthreads();
        for (int e = threadIdx.x; e < kL2Dims * kWordTile; e += kBlock) {
            const int w = e / kL2Dims, k = e % kL2Dims;
            const int gw = tl * kWordTile + w;
            tile[k][w] = gw < p.n_words ? dict[(int64_t)gw * kL2Dims + k] : 0.0f;
        }
        __syncthreads();
        const int w = tl * kWordTile + lane;
        for (int r = 0; r < kWave; r++) {
            const int slot = wv * kWave + r;
            if (slot >= ch.rows) break;
            float d = w < p.n_words ? l2_words_dist(rows + (int64_t)slot * kL2Dims, tile, lane) : INFINITY;
            if (d != d) d = INFINITY;
            int wi = w < p.n_words ? w : 0x7fffffff;
            wave_argmin(d, wi);
            if (lane == 0 && d < best_d[slot]) {
                best_d[slot] = d;
                best_w[slot] = wi;
            }
        }
    }
    __syncthreads();
    assign_tail(v, p, ch, a, it, best_w[threadIdx.x], (int)threadIdx.x < ch.rows ? l2_weight(best_d[threadIdx.x]) : 0);
}

// Hamming: one row per thread, the centres in LDS tiles that every lane reads at the same address
__global__ void __launch_bounds__(kBlock) assign_hamming_kernel(Params p, const uint32_t* __restrict__ desc, void* ws, int it)
{
    __shared__ uint32_t tile[kHammingTile][kHammingWords];
    const View v = view(ws, p);
    Chunk ch;
    if (!locate(v, p, blockIdx.x, ch)) return;
    const int a = blockIdx.y;
    const int64_t u = unit_of(p, ch.s, a);
    if (!unit_active(v, p, u, it)) return;
    const uint32_t* dict = (const uint32_t*)(v.centres + u * p.n_words * p.row_bytes);
    const bool live = (int)threadIdx.x < ch.rows;
    uint32_t x[kHammingWords] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live)
        for (int k = 0; k < kHammingWords; k++) x[k] = desc[(ch.off + ch.first + threadIdx.x) * kHammingWords + k];
    u64 best = ~0ull;
    int label = 0;
    for (int w0 = 0; w0 < p.n_words; w0 += kHammingTile) {
        const int cnt = min(kHammingTile, p.n_words - w0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * kHammingWords; e += kBlock) (&tile[0][0])[e] = dict[(int64_t)w0 * kHammingWords + e];
        __syncthreads();
        for (int w = 0; w < cnt; w++) {
            const u64 d = hamming_weight(x, tile[w]);
            if (d < best) {
                best = d;
                label = w0 + w;
            }
        }
    }
    assign_tail(v, p, ch, a, it, label, best);
}

// one workgroup per (cluster, unit): the members of the cluster are gathered chunk by chunk into LDS (in any order: the sums are
// integers), then summed per dimension / per bit. An empty cluster keeps its centre.
__global__ void __launch_bounds__(kBlock) update_kernel(Params p, const char* __restrict__ desc, void* ws, int it)
{
    __shared__ int32_t list[kChunk];
    __shared__ int n_list;
    __shared__ long long half[kL2Dims];
    __shared__ uint32_t bits[kBlock];
    const View v = view(ws, p);
    const int c = blockIdx.x, a = blockIdx.y, s = blockIdx.z, t = threadIdx.x;
    const SetInfo si = v.set[s];
    const int64_t u = unit_of(p, s, a);
    if (si.status != GMS_OK || v.flags[u * p.max_iters + it] == 0) return;
    const int32_t* lab = v.labels + (int64_t)a * p.total_rows + si.off;
    const char* rows = desc + si.off * p.row_bytes;
    const bool l2 = p.kind == GMS_DESC_L2_F32X128;
    const int dim = t & (kL2Dims - 1), par = t / kL2Dims;  // L2: two threads per dimension, members of even / odd place
    long long acc = 0;                                     // L2: sum of q; Hamming: ones of bit t
    int64_t count = 0;
    for (int64_t i0 = 0; i0 < si.n; i0 += kChunk) {
        if (t == 0) n_list = 0;
        __syncthreads();
        if (i0 + t < si.n && lab[i0 + t] == c) list[atomicAdd(&n_list, 1)] = (int32_t)(i0 + t);
        __syncthreads();
        const int m = n_list;
        count += m;
        if (l2) {
            for (int j = par; j < m; j += 2) acc += quantise(((const float*)rows)[(int64_t)list[j] * kL2Dims + dim]);
        } else {
            for (int j = 0; j < m; j++) acc += ((uint8_t)rows[(int64_t)list[j] * 32 + (t >> 3)] >> (t & 7)) & 1;
        }
        __syncthreads();
    }
    if (count == 0) return;
    char* centre = v.centres + (u * p.n_words + c) * p.row_bytes;
    if (l2) {
        if (par == 1) half[dim] = acc;
        __syncthreads();
        if (par == 0) ((float*)centre)[dim] = l2_mean(acc + half[dim], count);
    } else {
        bits[t] = majority(acc, count) ? 1u : 0u;
        __syncthreads();
        if (t < 32) {
            uint32_t b = 0;
            for (int k = 0; k < 8; k++) b |= bits[t * 8 + k] << k;
            ((uint8_t*)centre)[t] = (uint8_t)b;
        }
    }
}

// ========================================================== finish ==========================================================
__global__ void __launch_bounds__(kBlock) finish_kernel(Params p, void* ws, char* __restrict__ dict_out, gms_logos_dict_result* __restrict__ res,
                                                        int32_t* __restrict__ labels_out)
{
    __shared__ int win, win_iters;
    __shared__ u64 win_comp;
    const View v = view(ws, p);
    const int s = blockIdx.x, t = threadIdx.x;
    const SetInfo si = v.set[s];
    const int64_t dict_bytes = (int64_t)p.n_words * p.row_bytes;
    uint32_t* out = (uint32_t*)(dict_out + s * dict_bytes);
    if (si.status != GMS_OK) {
        for (int64_t e = t; e < dict_bytes / 4; e += kBlock) out[e] = 0;
        if (t == 0) res[s] = gms_logos_dict_result{si.status, -1, 0, 0, 0};
        if (labels_out)
            for (int i = t; i < si.rows_given; i += kBlock) labels_out[si.off + i] = -1;
        return;
    }
    if (t == 0) {
        int best = 0, best_iters = 0;
        u64 best_comp = 0;
        for (int a = 0; a < p.attempts; a++) {
            const int64_t u = unit_of(p, s, a);
            int changed = 0;  // assignments that changed a label: 0 .. changed - 1; the next one ran too unless it was not allowed
            while (changed < p.max_iters && v.flags[u * p.max_iters + changed] != 0) changed++;
            const int iters = min(changed + 1, p.max_iters);
            const u64 comp = v.comp[u * p.max_iters + iters - 1];
            if (a == 0 || comp < best_comp) {
                best = a;
                best_iters = iters;
                best_comp = comp;
            }
        }
        win = best;
        win_iters = best_iters;
        win_comp = best_comp;
    }
    __syncthreads();
    const uint32_t* src = (const uint32_t*)(v.centres + unit_of(p, s, win) * dict_bytes);
    for (int64_t e = t; e < dict_bytes / 4; e += kBlock) out[e] = src[e];
    int32_t* used = v.used + (int64_t)s * p.n_words;
    for (int w = t; w < p.n_words; w += kBlock) used[w] = 0;
    __syncthreads();
    const int32_t* lab = v.labels + (int64_t)win * p.total_rows + si.off;
    for (int i = t; i < si.n; i += kBlock) {
        const int32_t l = lab[i];
        used[l] = 1;
        if (labels_out) labels_out[si.off + i] = l;
    }
    __syncthreads();
    u64 empty = 0;
    for (int w = t; w < p.n_words; w += kBlock) empty += used[w] == 0;
    empty = block_sum(empty);
    if (t == 0) res[s] = gms_logos_dict_result{GMS_OK, win, win_iters, (int32_t)empty, win_comp};
}

}  // namespace

namespace gms {

size_t logos_dict_ws_bytes(const logos_dict::Params& p) { return (size_t)logos_dict::layout(p).total + 16; }

hipError_t launch_logos_dict_train(const logos_dict::Params& p, const void* d_desc, const int64_t* d_set_off, void* d_ws, void* d_dict,
                                   gms_logos_dict_result* d_results, int32_t* d_labels, hipStream_t st)
{
    if (p.n_sets == 0) return hipSuccess;
    const Layout L = layout(p);
    const char* desc = static_cast<const char*>(d_desc);
    hipError_t e = hipMemsetAsync(static_cast<char*>(d_ws) + L.flags, 0, (size_t)L.flag_bytes, st);
    if (e != hipSuccess) return e;
    plan_kernel<<<1, kBlock, 0, st>>>(p, d_set_off, d_ws);
    const dim3 rows_grid((unsigned)L.max_chunks, (unsigned)p.attempts), units_grid((unsigned)p.n_sets, (unsigned)p.attempts);
    if (p.kind == GMS_DESC_L2_F32X128) check_l2_kernel<<<(unsigned)L.max_chunks, kBlock, 0, st>>>(p, static_cast<const float*>(d_desc), d_ws);
    for (int c = 1; c < p.n_words; c++) {
        seed_update_kernel<<<rows_grid, kBlock, 0, st>>>(p, desc, d_ws, c);
        seed_pick_kernel<<<units_grid, kBlock, 0, st>>>(p, d_ws, c);
        seed_potential_kernel<<<rows_grid, kBlock, 0, st>>>(p, desc, d_ws);
    }
    seed_commit_kernel<<<units_grid, kL2Dims, 0, st>>>(p, desc, d_ws, p.n_words - 1);
    const dim3 update_grid((unsigned)p.n_words, (unsigned)p.attempts, (unsigned)p.n_sets);
    for (int it = 0; it < p.max_iters; it++) {
        if (p.kind == GMS_DESC_L2_F32X128) assign_l2_kernel<<<rows_grid, kBlock, 0, st>>>(p, static_cast<const float*>(d_desc), d_ws, it);
        else assign_hamming_kernel<<<rows_grid, kBlock, 0, st>>>(p, static_cast<const uint32_t*>(d_desc), d_ws, it);
        // the centres are not moved after the last assignment allowed: the labels returned are those of the dictionary returned
        if (it + 1 < p.max_iters) update_kernel<<<update_grid, kBlock, 0, st>>>(p, desc, d_ws, it);
    }
    finish_kernel<<<p.n_sets, kBlock, 0, st>>>(p, d_ws, static_cast<char*>(d_dict), d_results, d_labels);
    return hipGetLastError();
}

}  // namespace gms
