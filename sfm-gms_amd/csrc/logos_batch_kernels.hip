// logos_batch_kernels.hip -- the batched LOGOS path: per-frame tables built once (gms_logos_prepare_device), then
// any number of pairs of resident frames filtered per launch sequence (gms_logos_filter_device), and the visual word of every
// descriptor (gms_logos_words_device). Stream-ordered, no allocation, no synchronisation, no host read-back: capturable.
//
// prepare   plan (one workgroup)  -> points + word check -> five nearest per frame (LDS tiles) -> tied points redone by the
//           reference's sort on a fixed grid striding over the device-side tie list -> per frame a stable counting sort by word
// filter    plan (one workgroup: pair checks, query numbering) -> pass 1 (support of every candidate, histogram) -> peak (one wave
//           per pair) -> pass 2 (survivors per query) -> segmented scan + capacity check + records (one workgroup per pair) ->
//           pass 3 (survivors written in order)
// Passes 1-3 give one wave to one query keypoint i at a time: its candidates are frame b's bucket of word(i), already in ascending j,
// dealt to the 64 lanes; ballots keep the order. The arithmetic is logos_core.h's, so the bits are those of gms_logos_match.
#include <hip/hip_runtime.h>

#include "gms.h"
#include "gms_kernels.h"
#include "logos_batch.h"
#include "logos_core.h"
#include "logos_words_dist.h"

namespace {

using gms::logos::PairWork;
using gms::logos::Pt;
using gms::logos::TableHeader;
using gms::logos::TableLayout;
constexpr int kNum = gms::logos::kNum;
constexpr int kBins = gms::logos::kBins;
constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kScanBlock = 1024;

// where everything of a table is, from its header
struct Table {
    const TableHeader* h;
    int64_t* frame_off;
    int32_t *status, *items, *ties;
    Pt* pts;
    int32_t *word, *nb, *sorted, *bucket;
};

__device__ __forceinline__ Table table_view(const void* base)
{
    const TableHeader* h = static_cast<const TableHeader*>(base);
    const TableLayout L = gms::logos::table_layout(h->total_kp, h->n_frames, h->n_words);
    char* b = (char*)base;
    Table t;
    t.h = h;
    t.frame_off = (int64_t*)(b + L.frame_off);
    t.status = (int32_t*)(b + L.status);
    t.items = (int32_t*)(b + L.items);
    t.ties = (int32_t*)(b + L.ties);
    t.pts = (Pt*)(b + L.pts);
    t.word = (int32_t*)(b + L.word);
    t.nb = (int32_t*)(b + L.nb);
    t.sorted = (int32_t*)(b + L.sorted);
    t.bucket = (int32_t*)(b + L.bucket);
    return t;
}

// the last index k of a[0..n] with a[k] <= v (a ascending, a[0] <= v)
template <typename T>
__device__ __forceinline__ int last_le(const T* a, int n, int64_t v)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// exclusive scan of get(k), k in [0, n), by one workgroup of kScanBlock threads: put(k, offset); returns the total to every thread.
// Thread t reads the contiguous chunk [t per, (t + 1) per), which other threads of the workgroup may have just written (the callers
// fill their records with a stride of kScanBlock): the barrier in front makes those writes visible before the first get().
template <typename Get, typename Put>
__device__ int64_t block_scan(int64_t n, Get get, Put put)
{
    __shared__ int64_t part[kScanBlock];
    const int t = threadIdx.x;
    const int64_t per = (n + kScanBlock - 1) / kScanBlock;
    const int64_t lo = min(n, (int64_t)t * per), hi = min(n, lo + per);
    __syncthreads();
    int64_t s = 0;
    for (int64_t k = lo; k < hi; k++) s += get(k);
    __syncthreads();
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t k = lo; k < hi; k++) {
        const int64_t v = get(k);
        put(k, run);
        run += v;
    }
    const int64_t total = part[kScanBlock - 1];
    __syncthreads();
    return total;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// ======================================================== prepare ========================================================

__global__ void __launch_bounds__(kScanBlock) prep_plan_kernel(const int64_t* __restrict__ frame_off, int n_frames, int64_t total_kp,
                                                                int n_words, void* table)
{
    TableHeader* h = static_cast<TableHeader*>(table);
    const TableLayout L = gms::logos::table_layout(total_kp, n_frames, n_words);
    char* b = (char*)table;
    int64_t* fo = (int64_t*)(b + L.frame_off);
    int32_t* status = (int32_t*)(b + L.status);
    int32_t* items = (int32_t*)(b + L.items);
    for (int f = threadIdx.x; f <= n_frames; f += kScanBlock) fo[f] = frame_off[f];
    for (int f = threadIdx.x; f < n_frames; f += kScanBlock) status[f] = GMS_OK;
    if (threadIdx.x == 0) {
        h->magic = gms::logos::kTableMagic;
        h->total_kp = total_kp;
        h->n_frames = n_frames;
        h->n_words = n_words;
        *(int32_t*)(b + L.ties) = 0;
    }
    const int64_t total = block_scan(
        n_frames, [&](int64_t f) { return (frame_off[f + 1] - frame_off[f] + kBlock - 1) / kBlock; },
        [&](int64_t f, int64_t o) { items[f] = (int32_t)o; });
    if (threadIdx.x == 0) items[n_frames] = (int32_t)total;
}

__global__ void __launch_bounds__(kBlock) prep_points_kernel(const gms_keypoint* __restrict__ kp, const int32_t* __restrict__ words,
                                                              void* table)
{
    const Table t = table_view(table);
    const int64_t n = t.h->total_kp;
    const int n_words = t.h->n_words;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) {
        const gms_keypoint p = kp[k];
        // a keypoint outside the domain (logos_core.h kp_ok) marks its frame as a word out of range does, and is stored as zeros, so
        // that no later prepare kernel sorts or compares a non-finite coordinate; the filter runs none of the frame's queries
        const bool ok = gms::logos::kp_ok(p.x, p.y, p.angle);
        t.pts[k] = ok ? Pt{p.x, p.y, gms::logos::orientation(p.angle), gms::logos::logf_(p.size)} : Pt{0.0f, 0.0f, 0.0f, 0.0f};
        const int32_t w = words[k];
        t.word[k] = w;
        if (!ok || w < 0 || w >= n_words) atomicMin(&t.status[last_le(t.frame_off, t.h->n_frames, k)], GMS_ERR_DOMAIN);
    }
}

// logos_kernels.hip's logos_knn_kernel, many frames per launch: workgroup b works on frame f's points [c * kBlock, (c + 1) * kBlock)
// where items[f] + c = b. Tied points go on the table's tie list (global index).
__global__ void __launch_bounds__(kBlock) prep_knn_kernel(void* table)
{
    __shared__ float sx[kBlock], sy[kBlock];
    const Table t = table_view(table);
    const int n_frames = t.h->n_frames;
    if ((int)blockIdx.x >= t.items[n_frames]) return;
    const int f = last_le(t.items, n_frames, blockIdx.x);
    const int64_t base = t.frame_off[f];
    const int n = (int)(t.frame_off[f + 1] - base);
    const Pt* pts = t.pts + base;
    const int i = ((int)blockIdx.x - t.items[f]) * kBlock + threadIdx.x;
    float x = 0.0f, y = 0.0f;
    if (i < n) {
        x = pts[i].x;
        y = pts[i].y;
    }
    float bd[kNum];
    int bi[kNum];
#pragma unroll
    for (int k = 0; k < kNum; k++) {
        bd[k] = INFINITY;
        bi[k] = -1;
    }
    for (int b0 = 0; b0 < n; b0 += kBlock) {
        __syncthreads();
        const int s = b0 + threadIdx.x;
        if (s < n) {
            sx[threadIdx.x] = pts[s].x;
            sy[threadIdx.x] = pts[s].y;
        }
        __syncthreads();
        const int cnt = min(kBlock, n - b0);
        if (i < n) {
            for (int u = 0; u < cnt; u++) {
                const int j = b0 + u;
                if (j == i) continue;
                const float d = gms::logos::dist2(x, y, sx[u], sy[u]);
                if (bi[kNum - 1] >= 0 && !(d < bd[kNum - 1])) continue;
                float cd = d;
                int ci = j;
#pragma unroll
                for (int k = 0; k < kNum; k++) {
                    const bool take = bi[k] < 0 || cd < bd[k];
                    const float td = bd[k];
                    const int ti = bi[k];
                    if (take) {
                        bd[k] = cd;
                        bi[k] = ci;
                        cd = td;
                        ci = ti;
                        if (ti < 0) break;
                    }
                }
            }
        }
    }
    const int kk = min(kNum, n - 1);
    const float dk = kk > 0 ? bd[kk - 1] : 0.0f;
    int within = 0;
    for (int b0 = 0; b0 < n; b0 += kBlock) {
        __syncthreads();
        const int s = b0 + threadIdx.x;
        if (s < n) {
            sx[threadIdx.x] = pts[s].x;
            sy[threadIdx.x] = pts[s].y;
        }
        __syncthreads();
        const int cnt = min(kBlock, n - b0);
        if (i < n && kk > 0) {
            for (int u = 0; u < cnt; u++) within += (b0 + u != i && !(dk < gms::logos::dist2(x, y, sx[u], sy[u]))) ? 1 : 0;
        }
    }
    if (i < n) {
        int32_t* nb = t.nb + (base + i) * kNum;
#pragma unroll
        for (int k = 0; k < kNum; k++) nb[k] = bi[k];
        if (within > kk) t.ties[1 + atomicAdd(&t.ties[0], 1)] = (int32_t)(base + i);
    }
}

// logos_kernels.hip's logos_knn_ties_kernel on a fixed grid of kTieLanes lanes striding over the tie list, whose length is read on
// the device. Lane l's slice of the workspace holds slice_recs (distance, index) records; a frame too large for it is marked.
__global__ void __launch_bounds__(gms::logos::kTieBlock) prep_ties_kernel(void* table, float* __restrict__ work, int64_t slice_recs)
{
    const Table t = table_view(table);
    const int lane = blockIdx.x * gms::logos::kTieBlock + threadIdx.x;
    float* d = work + (size_t)lane * 2 * (size_t)slice_recs;
    const int n_ties = t.ties[0];
    for (int k = lane; k < n_ties; k += gms::logos::kTieLanes) {
        const int64_t g = t.ties[1 + k];
        const int f = last_le(t.frame_off, t.h->n_frames, g);
        const int64_t base = t.frame_off[f];
        const int n = (int)(t.frame_off[f + 1] - base);
        const long m = n - 1;
        if (m > slice_recs) {
            atomicMin(&t.status[f], GMS_ERR_BAD_ARG);
            continue;
        }
        int32_t* ix = reinterpret_cast<int32_t*>(d + m);
        const Pt* pts = t.pts + base;
        const int i = (int)(g - base);
        const float x = pts[i].x, y = pts[i].y;
        long c = 0;
        for (int j = 0; j < n; j++) {
            if (j == i) continue;
            d[c] = gms::logos::dist2(x, y, pts[j].x, pts[j].y);
            ix[c] = j;
            c++;
        }
        gms::logos::msvc_sort_head(d, ix, m, kNum);
        for (int q = 0; q < kNum; q++) t.nb[g * kNum + q] = ix[q];
    }
}

// per frame (one wave): stable counting sort of the keypoints by word. bucket[w] = start of word w's run, bucket[n_words] = the
// frame's in-range keypoints. Words out of range (their frame is marked) are left out.
__global__ void __launch_bounds__(kWave) prep_sort_kernel(void* table)
{
    const Table t = table_view(table);
    const int f = blockIdx.x;
    const int n_words = t.h->n_words;
    const int64_t base = t.frame_off[f];
    const int n = (int)(t.frame_off[f + 1] - base);
    int32_t* B = t.bucket + (int64_t)f * (n_words + 1);
    const int32_t* word = t.word + base;
    int32_t* sorted = t.sorted + base;
    const int lane = threadIdx.x;
    // 64 keypoints at a time, in index order: this lane's word (-1 out of range or past the end), its rank among the equal words of
    // the lanes below, and how many lanes hold it
    auto chunk = [&](int c, int32_t* w_out, int* rank_out, int* cnt_out) {
        const int k = c + lane;
        int32_t w = k < n ? word[k] : -1;
        if (w >= n_words) w = -1;
        int rank = 0, cnt = 0;
        for (int s = 0; s < kWave; s++) {
            const int32_t ws = __shfl(w, s);
            if (ws == w) {
                cnt++;
                rank += s < lane ? 1 : 0;
            }
        }
        *w_out = w < 0 ? -1 : w;
        *rank_out = rank;
        *cnt_out = cnt;
    };
    for (int w = lane; w <= n_words; w += kWave) B[w] = 0;
    __syncthreads();
    for (int c = 0; c < n; c += kWave) {  // counts at B[w + 1]; one lane per word and chunk adds
        int32_t w;
        int rank, cnt;
        chunk(c, &w, &rank, &cnt);
        if (w >= 0 && rank == cnt - 1) B[w + 1] += cnt;
        __syncthreads();
    }
    int carry = 0;  // inclusive scan of B[1 .. n_words]: B[w] = start of word w
    for (int c = 1; c <= n_words; c += kWave) {
        const int w = c + lane;
        int v = w <= n_words ? B[w] : 0;
        for (int d = 1; d < kWave; d <<= 1) {
            const int u = __shfl_up(v, d);
            if (lane >= d) v += u;
        }
        if (w <= n_words) B[w] = v + carry;
        carry += __shfl(v, kWave - 1);
    }
    __syncthreads();
    for (int c = 0; c < n; c += kWave) {  // scatter, B[w] as the cursor of word w
        int32_t w;
        int rank, cnt;
        chunk(c, &w, &rank, &cnt);
        if (w >= 0) sorted[B[w] + rank] = c + lane;
        __syncthreads();
        if (w >= 0 && rank == cnt - 1) B[w] += cnt;
        __syncthreads();
    }
    // B[w] now ends word w's run: shift up by one (from the top down, every read before the write over it)
    for (int top = n_words; top >= 1; top -= kWave) {
        const int w = top - lane;
        const int v = w >= 1 ? B[w - 1] : 0;
        __syncthreads();
        if (w >= 1) B[w] = v;
        __syncthreads();
    }
    if (lane == 0) B[0] = 0;
}

// ========================================================= filter ========================================================

struct FilterWs {
    int64_t* total_q;
    PairWork* pw;
    int64_t* keep;
};

__device__ __forceinline__ FilterWs filter_ws(void* ws, int n_pairs)
{
    char* b = (char*)ws;
    FilterWs f;
    f.total_q = (int64_t*)b;
    f.pw = (PairWork*)(b + gms::logos::kFilterHeaderBytes);
    f.keep = (int64_t*)(b + gms::logos::filter_fixed_bytes(n_pairs));
    return f;
}

// pair checks and the batch's query numbering; zeroes the pairs' accumulators. A pair of a marked frame (a word out of range, a
// keypoint outside the domain, ties that did not fit the prepare workspace) takes the frame's status in either role and gets n1 = 0:
// it has no queries in the numbering, so passes 1-3 never read the frame's points, neighbours or buckets.
__global__ void __launch_bounds__(kScanBlock) filter_plan_kernel(const void* table, const gms_pair* __restrict__ pairs, int n_pairs,
                                                                  void* ws, int64_t keep_cap)
{
    const Table t = table_view(table);
    const FilterWs W = filter_ws(ws, n_pairs);
    const int n_frames = t.h->n_frames;
    for (int p = threadIdx.x; p < n_pairs; p += kScanBlock) {
        const gms_pair pr = pairs[p];
        PairWork& w = W.pw[p];
        int st = GMS_OK;
        if (pr.frame_a < 0 || pr.frame_a >= n_frames || pr.frame_b < 0 || pr.frame_b >= n_frames || pr.m < 0 || pr.match_off < 0)
            st = GMS_ERR_BAD_ARG;
        else if (t.status[pr.frame_a] != GMS_OK)
            st = t.status[pr.frame_a];
        else if (t.status[pr.frame_b] != GMS_OK)
            st = t.status[pr.frame_b];
        w.status = st;
        w.n_cand = w.n_supp = w.total = 0;
        w.peak = 0.0f;
        w.peak_bin = -1;
        w.base_a = st == GMS_OK ? t.frame_off[pr.frame_a] : 0;
        w.base_b = st == GMS_OK ? t.frame_off[pr.frame_b] : 0;
        w.n1 = st == GMS_OK ? (int32_t)(t.frame_off[pr.frame_a + 1] - w.base_a) : 0;
        w.n2 = st == GMS_OK ? (int32_t)(t.frame_off[pr.frame_b + 1] - w.base_b) : 0;
        w.frame_b = st == GMS_OK ? pr.frame_b : 0;
        for (int b = 0; b < kBins; b++) w.bins[b] = 0;
    }
    const int64_t total = block_scan(
        n_pairs, [&](int64_t p) { return (int64_t)W.pw[p].n1; }, [&](int64_t p, int64_t o) { W.pw[p].q_start = o; });
    for (int p = threadIdx.x; p < n_pairs; p += kScanBlock)
        if (W.pw[p].q_start + W.pw[p].n1 > keep_cap) W.pw[p].status = GMS_ERR_BAD_ARG;  // the workspace has no room for its queries
    if (threadIdx.x == 0) *W.total_q = total;
}

// the query keypoint, the same for every lane of the wave
struct Query {
    Pt p;
    int32_t word;
    int64_t g, base_a;
    int32_t la[kNum];  // word of neighbour u, -1 where there is none
};

__device__ __forceinline__ void load_query(const Table& t, int64_t base_a, int i, Query& Q)
{
    Q.g = base_a + i;
    Q.base_a = base_a;
    Q.p = t.pts[Q.g];
    Q.word = t.word[Q.g];
#pragma unroll
    for (int u = 0; u < kNum; u++) {
        const int a = t.nb[Q.g * kNum + u];
        Q.la[u] = a >= 0 ? t.word[base_a + a] : -1;
    }
}

// does candidate (i, j) have support: some neighbour pair (a, b) with equal words that is consistent (logos_core.h). The pairs with
// equal words are found first (bit 5 u + v), then tested one by one.
__device__ __forceinline__ bool supported(const Table& t, const Query& Q, int64_t base_b, int j, const Pt& q, float rel_o, float rel_s)
{
    const int64_t gj = base_b + j;
    uint32_t pairs = 0;
#pragma unroll
    for (int v = 0; v < kNum; v++) {
        const int b = t.nb[gj * kNum + v];
        const int32_t lb = b >= 0 ? t.word[base_b + b] : -2;
#pragma unroll
        for (int u = 0; u < kNum; u++) pairs |= (Q.la[u] == lb ? 1u : 0u) << (kNum * u + v);
    }
    while (pairs) {
        const int bit = __ffs(pairs) - 1;
        pairs &= pairs - 1;
        const int u = bit / kNum, v = bit - kNum * (bit / kNum);
        const Pt a = t.pts[Q.base_a + t.nb[Q.g * kNum + u]];
        const Pt b = t.pts[base_b + t.nb[gj * kNum + v]];
        if (gms::logos::consistent_early(Q.p, q, rel_o, rel_s, a, b)) return true;
    }
    return false;
}

// a wave's contiguous share of the batch's queries, and the pair of its first one
__device__ __forceinline__ bool wave_share(const FilterWs& W, int n_pairs, int64_t* q0, int64_t* q1, int* p0)
{
    const int64_t total = *W.total_q;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const int64_t per = (total + waves - 1) / waves;
    *q0 = gw * per;
    *q1 = min(total, *q0 + per);
    if (*q0 >= *q1) return false;
    int lo = 0, hi = n_pairs;  // last pair with q_start <= q0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (W.pw[mid].q_start <= *q0) lo = mid;
        else hi = mid;
    }
    *p0 = lo;
    return true;
}


// the candidates of query i: frame b's run of word(i), local indices in ascending order
__device__ __forceinline__ void bucket_of(const Table& t, const PairWork& w, int32_t word, const int32_t** js, int* cnt)
{
    const int32_t* B = t.bucket + (int64_t)w.frame_b * (t.h->n_words + 1);
    *js = t.sorted + w.base_b + B[word];
    *cnt = B[word + 1] - B[word];
}

// pass 1: per candidate its support; per pair the candidates, the supported ones (int64) and their histogram. A wave's histogram
// lives in LDS and goes to the pair's bins whenever the wave moves on to another pair.
__global__ void __launch_bounds__(kBlock) filter_support_kernel(const void* table, int n_pairs, void* ws)
{
    __shared__ int32_t hist[kBlock / kWave][kBins];
    const Table t = table_view(table);
    const FilterWs W = filter_ws(ws, n_pairs);
    const int lane = lane_id();
    int32_t* h = hist[threadIdx.x / kWave];
    for (int b = lane; b < kBins; b += kWave) h[b] = 0;
    int64_t q0, q1;
    int p = 0;
    if (!wave_share(W, n_pairs, &q0, &q1, &p)) return;
    int64_t nc = 0, ns = 0;
    auto flush = [&](int pp) {
        __threadfence_block();
        PairWork& w = W.pw[pp];
        for (int b = lane; b < kBins; b += kWave) {
            const int32_t v = h[b];
            if (v) {
                atomicAdd(&w.bins[b], v);
                h[b] = 0;
            }
        }
        if (lane == 0 && nc) atomicAdd((unsigned long long*)&w.n_cand, (unsigned long long)nc);
        if (lane == 0 && ns) atomicAdd((unsigned long long*)&w.n_supp, (unsigned long long)ns);
        nc = ns = 0;
        __threadfence_block();
    };
    for (int64_t qi = q0; qi < q1; qi++) {
        while (p < n_pairs - 1 && qi >= W.pw[p].q_start + W.pw[p].n1) {
            flush(p);
            p++;
        }
        const PairWork& w = W.pw[p];
        if (w.status != GMS_OK) continue;
        Query Q;
        load_query(t, w.base_a, (int)(qi - w.q_start), Q);
        const int32_t* js;
        int cnt;
        bucket_of(t, w, Q.word, &js, &cnt);
        nc += cnt;
        for (int c = 0; c < cnt; c += kWave) {
            const int k = c + lane;
            bool sup = false;
            float rel_o = 0.0f;
            if (k < cnt) {
                const int j = js[k];
                const Pt q = t.pts[w.base_b + j];
                rel_o = gms::logos::rel_ori(Q.p.ori, q.ori);
                const float rel_s = Q.p.logscale - q.logscale;
                sup = supported(t, Q, w.base_b, j, q, rel_o, rel_s);
            }
            ns += __popcll(__ballot(sup));
            if (sup) atomicAdd(&h[gms::logos::bin_of(rel_o)], 1);
        }
    }
    flush(p);
}

// the histogram's peak, one wave per pair
__global__ void __launch_bounds__(kWave) filter_peak_kernel(int n_pairs, void* ws)
{
    __shared__ int32_t bins[kBins];
    const FilterWs W = filter_ws(ws, n_pairs);
    PairWork& w = W.pw[blockIdx.x];
    if (w.status != GMS_OK) return;
    for (int b = threadIdx.x; b < kBins; b += kWave) bins[b] = w.bins[b];
    __syncthreads();
    if (threadIdx.x == 0) {
        int pb = 0;
        w.peak = gms::logos::peak_orientation(bins, &pb);
        w.peak_bin = pb;
    }
}

// pass 2 (kWrite = false): survivors per query -> keep[q]. Pass 3 (kWrite = true): the survivors of pairs that fit, at
// match_off + keep[q] (the scanned offsets), in ascending j by ballot.
template <bool kWrite>
__global__ void __launch_bounds__(kBlock) filter_select_kernel(const void* table, const gms_pair* __restrict__ pairs, int n_pairs,
                                                                void* ws, gms_dmatch* __restrict__ out)
{
    const Table t = table_view(table);
    const FilterWs W = filter_ws(ws, n_pairs);
    const int lane = lane_id();
    int64_t q0, q1;
    int p = 0;
    if (!wave_share(W, n_pairs, &q0, &q1, &p)) return;
    for (int64_t qi = q0; qi < q1; qi++) {
        while (p < n_pairs - 1 && qi >= W.pw[p].q_start + W.pw[p].n1) p++;
        const PairWork& w = W.pw[p];
        if (w.status != GMS_OK) continue;
        const int i = (int)(qi - w.q_start);
        Query Q;
        load_query(t, w.base_a, i, Q);
        const int32_t* js;
        int cnt;
        bucket_of(t, w, Q.word, &js, &cnt);
        const float g = w.peak;
        int64_t o = kWrite ? pairs[p].match_off + W.keep[qi] : 0;
        int64_t kept = 0;
        for (int c = 0; c < cnt; c += kWave) {
            const int k = c + lane;
            bool keep = false;
            int j = 0;
            if (k < cnt) {
                j = js[k];
                const Pt q = t.pts[w.base_b + j];
                const float rel_o = gms::logos::rel_ori(Q.p.ori, q.ori);
                if (gms::logos::globally_consistent(rel_o, g)) {
                    const float rel_s = Q.p.logscale - q.logscale;
                    keep = supported(t, Q, w.base_b, j, q, rel_o, rel_s);
                }
            }
            const uint64_t mask = __ballot(keep);
            if (kWrite && keep) out[o + __popcll(mask & lanes_below())] = gms_dmatch{i, j, -1, 0.0f};
            o += __popcll(mask);
            kept += __popcll(mask);
        }
        if (!kWrite && lane == 0) W.keep[qi] = kept;
    }
}

// one workgroup per pair: keep[] -> offsets within the pair, the capacity check, the result records
__global__ void __launch_bounds__(kScanBlock) filter_scan_kernel(const gms_pair* __restrict__ pairs, int n_pairs, void* ws,
                                                                  gms_logos_result* __restrict__ lres, gms_pair_result* __restrict__ pres)
{
    const FilterWs W = filter_ws(ws, n_pairs);
    PairWork& w = W.pw[blockIdx.x];
    const int st0 = w.status;
    int64_t total = 0;
    if (st0 == GMS_OK) {
        int64_t* keep = W.keep + w.q_start;
        total = block_scan(w.n1, [&](int64_t k) { return keep[k]; }, [&](int64_t k, int64_t o) { keep[k] = o; });
    }
    if (threadIdx.x != 0) return;
    int st = st0;
    if (st == GMS_OK && total > (int64_t)pairs[blockIdx.x].m) st = GMS_ERR_CAPACITY;
    w.status = st;
    w.total = total;
    const bool counted = st0 == GMS_OK;
    lres[blockIdx.x] = gms_logos_result{counted ? w.n_cand : 0, counted ? w.n_supp : 0, total,
                                        counted && w.n_supp ? w.peak_bin : -1, st};
    if (pres) pres[blockIdx.x] = gms_pair_result{st == GMS_OK ? (int32_t)total : 0, -1, -1, st};
}

// ========================================================= words ========================================================
// The exact nearest dictionary row of every descriptor row: lane l of a wave computes, alone and in the sequential
// order of the definition, the distance of the wave's current row to word (tile + l); a wave-wide (distance, index) minimum and a
// strict '<' across tiles leave the lowest index among equal distances. NaN distances count as +inf.
using gms::logos::kWordTile;
using gms::logos::l2_words_dist;
using gms::logos::wave_argmin;
constexpr int kRowsPerWave = 8;
constexpr int kRowsPerBlock = kRowsPerWave * (kBlock / kWave);

__global__ void __launch_bounds__(kBlock) words_l2_kernel(const float* __restrict__ desc, int64_t total, const float* __restrict__ dict,
                                                           int n_words, int32_t* __restrict__ out)
{
    __shared__ float tile[128][kWordTile];
    __shared__ float best_d[kRowsPerBlock];
    __shared__ int best_w[kRowsPerBlock];
    const int lane = lane_id(), wv = threadIdx.x / kWave;
    const int n_tiles = (n_words + kWordTile - 1) / kWordTile;
    for (int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock; r0 < total; r0 += (int64_t)gridDim.x * kRowsPerBlock) {
        if (threadIdx.x < kRowsPerBlock) {
            best_d[threadIdx.x] = INFINITY;
            best_w[threadIdx.x] = 0;
        }
        for (int tl = 0; tl < n_tiles; tl++) {
            if (n_tiles > 1 || r0 == (int64_t)blockIdx.x * kRowsPerBlock) {
                __syncthreads();
                for (int e = threadIdx.x; e < 128 * kWordTile; e += kBlock) {
                    const int w = e / 128, k = e % 128;
                    const int gw = tl * kWordTile + w;
                    tile[k][w] = gw < n_words ? dict[(int64_t)gw * 128 + k] : 0.0f;
                }
            }
            __syncthreads();
            for (int r = 0; r < kRowsPerWave; r++) {
                const int slot = wv * kRowsPerWave + r;
                const int64_t row = r0 + slot;
                if (row >= total) break;
                const int w = tl * kWordTile + lane;
                float d = w < n_words ? l2_words_dist(desc + row * 128, tile, lane) : INFINITY;
                if (d != d) d = INFINITY;
                int wi = w < n_words ? w : 0x7fffffff;
                wave_argmin(d, wi);
                if (lane == 0 && d < best_d[slot]) {
                    best_d[slot] = d;
                    best_w[slot] = wi;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < kRowsPerBlock && r0 + threadIdx.x < total) out[r0 + threadIdx.x] = best_w[threadIdx.x];
    }
}

__global__ void __launch_bounds__(kBlock) words_hamming_kernel(const uint32_t* __restrict__ desc, int64_t total,
                                                                const uint32_t* __restrict__ dict, int n_words, int32_t* __restrict__ out)
{
    const int lane = lane_id();
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
    const int n_tiles = (n_words + kWordTile - 1) / kWordTile;
    for (int64_t row = wave; row < total; row += waves) {
        const uint32_t* x = desc + row * 8;
        float bd = INFINITY;
        int bw = 0;
        for (int tl = 0; tl < n_tiles; tl++) {
            const int w = tl * kWordTile + lane;
            float d = INFINITY;
            if (w < n_words) {
                const uint32_t* y = dict + (int64_t)w * 8;
                int s = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += __popc(x[k] ^ y[k]);
                d = (float)s;
            }
            int wi = w < n_words ? w : 0x7fffffff;
            wave_argmin(d, wi);
            if (d < bd) {
                bd = d;
                bw = wi;
            }
        }
        if (lane == 0) out[row] = bw;
    }
}

int grid_for(int64_t items, int per_block, int cap)
{
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

namespace gms {

hipError_t launch_logos_prepare(const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const int32_t* d_words,
                                int n_words, void* d_ws, size_t ws_bytes, void* d_table, int n_cus, hipStream_t st)
{
    prep_plan_kernel<<<1, kScanBlock, 0, st>>>(d_frame_off, n_frames, total_kp, n_words, d_table);
    if (total_kp > 0) {
        prep_points_kernel<<<grid_for(total_kp, kBlock, 8 * n_cus), kBlock, 0, st>>>(d_kp, d_words, d_table);
        // the five-nearest pass: at most one partial workgroup per frame beyond total_kp / kBlock
        const int64_t knn_blocks = (total_kp + kBlock - 1) / kBlock + n_frames;
        prep_knn_kernel<<<(unsigned)knn_blocks, kBlock, 0, st>>>(d_table);
        prep_ties_kernel<<<logos::kTieLanes / logos::kTieBlock, logos::kTieBlock, 0, st>>>(
            d_table, static_cast<float*>(d_ws), logos::tie_slice_records((int64_t)ws_bytes));
    }
    if (n_frames > 0) prep_sort_kernel<<<n_frames, kWave, 0, st>>>(d_table);
    return hipGetLastError();
}

hipError_t launch_logos_filter(const void* d_table, const gms_pair* d_pairs, int n_pairs, void* d_ws, size_t ws_bytes, gms_dmatch* d_out,
                               gms_logos_result* d_lres, gms_pair_result* d_pres, int n_cus, hipStream_t st)
{
    const int64_t keep_cap = ((int64_t)ws_bytes - logos::filter_fixed_bytes(n_pairs)) / 8;
    const int waves_grid = 8 * n_cus;
    filter_plan_kernel<<<1, kScanBlock, 0, st>>>(d_table, d_pairs, n_pairs, d_ws, keep_cap);
    filter_support_kernel<<<waves_grid, kBlock, 0, st>>>(d_table, n_pairs, d_ws);
    filter_peak_kernel<<<n_pairs, kWave, 0, st>>>(n_pairs, d_ws);
    filter_select_kernel<false><<<waves_grid, kBlock, 0, st>>>(d_table, d_pairs, n_pairs, d_ws, d_out);
    filter_scan_kernel<<<n_pairs, kScanBlock, 0, st>>>(d_pairs, n_pairs, d_ws, d_lres, d_pres);
    filter_select_kernel<true><<<waves_grid, kBlock, 0, st>>>(d_table, d_pairs, n_pairs, d_ws, d_out);
    return hipGetLastError();
}

hipError_t launch_logos_words(int kind, const void* d_desc, int64_t total, const void* d_dict, int n_words, int32_t* d_words, int n_cus,
                              hipStream_t st)
{
    if (kind == GMS_DESC_L2_F32X128)
        words_l2_kernel<<<grid_for(total, kRowsPerBlock, 4 * n_cus), kBlock, 0, st>>>(static_cast<const float*>(d_desc), total,
                                                                                       static_cast<const float*>(d_dict), n_words, d_words);
    else
        words_hamming_kernel<<<grid_for(total, kBlock / kWave, 8 * n_cus), kBlock, 0, st>>>(
            static_cast<const uint32_t*>(d_desc), total, static_cast<const uint32_t*>(d_dict), n_words, d_words);
    return hipGetLastError();
}

}  // namespace gms
