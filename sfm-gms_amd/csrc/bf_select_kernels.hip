// bf_select_kernels.hip -- the reference's bruteForceMatch on resident frames (FeatureMatchUtil.cpp:20-31):
//
//     BFMatcher(norm, crossCheck = true).match(desc1, desc2, matches)
//     std::sort(matches)                                                   // by distance, MSVC introsort (not stable)
//     while (front.distance * 4.0 < back.distance) pop_back; while (size > 500) pop_back
//
// Three stream-ordered launches per batch, no allocation, no synchronisation (graph-capturable):
//   bf_sel_plan_kernel      one workgroup: the matcher's pair table in the workspace -- per pair (frame_b, frame_a) with cross-check
//                           (OpenCV's batchDistance computes only the backward direction), (frame_a, frame_b) without -- and each
//                           pair's row range in the matcher output (an exclusive scan of the matcher's query rows).
//   the matcher             launch_bf_match, unchanged (bf_kernels.hip), on that table, into the workspace.
//   bf_select_kernel        one workgroup per pair: the cross-check merge (a 64-bit minimum per query row of frame_a on
//                           (distance bits, train row): bf_select_core.h), compaction in query order into (d, q, t) candidates,
//                           d_min and the count within the ratio (K), the first K places of MSVC's sort by one lane, the survivors.
// Slots and sort records live in LDS while a pair's query rows fit (kLdsRecs), in the workspace otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf_select_core.h"
#include "gms_kernels.h"

namespace gms {
namespace {

using bfsel::kEmptySlot;
using bfsel::kSortStack;

constexpr int kSelBlock = 512;
constexpr int kSelWaves = kSelBlock / 64;
constexpr int kPlanBlock = 1024;
constexpr int kLdsRecs = 10240;  // 80 KiB: 8 bytes per slot, or per sort record (float d + int32 ix); two workgroups per CU

// the workspace's typed pointers (its regions: BfSelectLayout in ws_layout.h); per pair, stride max_rows: (q, t) / slots, d, ix
struct SelWs {
    gms_pair* pairs2;
    gms_dmatch* back;
    uint64_t* qt;
    float* cd;
    int32_t* cix;
};

struct PairCheck {
    int64_t offA, offB;
    int nA, nB, status;
};

// GMS_ERR_BAD_ARG: a frame index out of range, m < 0, a frame larger than max_rows; GMS_ERR_DOMAIN: an empty frame
__device__ __forceinline__ PairCheck check_pair(const gms_pair& pr, const int64_t* __restrict__ frame_off, int n_frames, int max_rows)
{
    PairCheck c{0, 0, 0, 0, GMS_OK};
    if (pr.frame_a < 0 || pr.frame_a >= n_frames || pr.frame_b < 0 || pr.frame_b >= n_frames || pr.m < 0) {
        c.status = GMS_ERR_BAD_ARG;
        return c;
    }
    c.offA = frame_off[pr.frame_a];
    c.offB = frame_off[pr.frame_b];
    const int64_t nA = frame_off[pr.frame_a + 1] - c.offA, nB = frame_off[pr.frame_b + 1] - c.offB;
    if (nA < 0 || nB < 0 || nA > max_rows || nB > max_rows) {
        c.status = GMS_ERR_BAD_ARG;
        return c;
    }
    c.nA = (int)nA;
    c.nB = (int)nB;
    if (c.nA == 0 || c.nB == 0) c.status = GMS_ERR_DOMAIN;
    return c;
}

// one workgroup: the matcher's table and each pair's place in its output; a pair that does not fit in total_back rows gets m = -1
// (the matcher skips it; bf_select_kernel reports GMS_ERR_BAD_ARG)
__global__ void __launch_bounds__(kPlanBlock)
bf_sel_plan_kernel(const gms_pair* __restrict__ pairs, int n_pairs, const int64_t* __restrict__ frame_off, int n_frames, int max_rows,
                   int cross, int64_t total_back, gms_pair* __restrict__ pairs2)
{
    __shared__ int64_t s_wave[kPlanBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int p0 = 0; p0 < n_pairs; p0 += kPlanBlock) {
        const int p = p0 + tid;
        gms_pair pr{0, 0, -1, 0, 0};
        int64_t rows = 0;
        if (p < n_pairs) {
            pr = pairs[p];
            const PairCheck c = check_pair(pr, frame_off, n_frames, max_rows);
            if (c.status == GMS_OK) rows = cross ? c.nB : c.nA;
        }
        // inclusive scan of rows: within the wave by shuffles, across waves through LDS
        int64_t x = rows;
        for (int s = 1; s < 64; s <<= 1) {
            const int64_t y = __shfl_up(x, s);
            if (lane >= s) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        int64_t total = carry;
        for (int w = 0; w < kPlanBlock / 64; w++) total += s_wave[w];
        const int64_t off = before + x - rows;
        if (p < n_pairs) {
            gms_pair q;
            q.frame_a = cross ? pr.frame_b : pr.frame_a;
            q.frame_b = cross ? pr.frame_a : pr.frame_b;
            q.m = (rows > 0 && off + rows <= total_back) ? (int)rows : (rows > 0 ? -1 : 0);
            q.reserved = 0;
            q.match_off = rows > 0 && off + rows <= total_back ? off : 0;
            pairs2[p] = q;
        }
        carry = total;
        __syncthreads();
    }
}

struct SelStats {
    int64_t n_cand, n_ratio, n_out;
    float d_min;
    int32_t status;
};

__device__ __forceinline__ void write_results(int p, const SelStats& s, gms_bf_result* res, gms_pair_result* pres)
{
    gms_bf_result r;
    r.n_candidates = s.n_cand;
    r.n_ratio = s.n_ratio;
    r.n_out = s.n_out;
    r.d_min = s.d_min;
    r.status = s.status;
    res[p] = r;
    if (pres) pres[p] = gms_pair_result{s.status == GMS_OK ? (int32_t)s.n_out : 0, -1, -1, s.status};
}

// exclusive prefix of `flag` over the workgroup; *total: the workgroup's count. Ends with a barrier.
__device__ __forceinline__ int block_prefix(bool flag, int* s_cnt, int* total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t b = __ballot(flag);
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kSelWaves; w++) {
        before += w < wave ? s_cnt[w] : 0;
        all += s_cnt[w];
    }
    *total = all;
    __syncthreads();
    return before + in_wave;
}

__global__ void __launch_bounds__(kSelBlock)
bf_select_kernel(const gms_pair* __restrict__ pairs, const int64_t* __restrict__ frame_off, int n_frames, int max_rows,
                 int cross, double coef, int max_size, SelWs ws, gms_dmatch* __restrict__ out, gms_bf_result* __restrict__ res,
                 gms_pair_result* __restrict__ pres)
{
    __shared__ uint64_t s_buf[kLdsRecs];  // slots (u64), then sort records: d in the first half, ix in the second
    __shared__ int32_t s_stack[3 * kSortStack];
    __shared__ int s_cnt[kSelWaves];
    __shared__ float s_min[kSelWaves];
    __shared__ int64_t s_n[kSelWaves];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gms_pair pr = pairs[p];
    const PairCheck c = check_pair(pr, frame_off, n_frames, max_rows);
    SelStats st{0, 0, 0, 0.0f, c.status};
    if (st.status == GMS_OK && ws.pairs2[p].m < 0) st.status = GMS_ERR_BAD_ARG;  // beyond the matcher rows the workspace holds
    if (st.status != GMS_OK) {
        if (tid == 0) write_results(p, st, res, pres);
        return;  // workgroup-uniform
    }
    const int nA = c.nA, nB = c.nB;
    const int64_t base = (int64_t)p * max_rows;
    const gms_dmatch* __restrict__ back = ws.back + ws.pairs2[p].match_off;
    uint64_t* __restrict__ g_qt = ws.qt + base;
    float* __restrict__ g_d = ws.cd + base;
    int32_t* __restrict__ g_ix = ws.cix + base;
    const bool lds = nA <= kLdsRecs;

    // ---- cross-check merge: slot[q] = min over the backward matches i with tidx[i] == q of (d_i bits, i) ----------------------
    // (without cross-check the forward match of q is its only entry). Keys hold (distance bits, train row of frame_b) either way.
    uint64_t* slot = lds ? s_buf : g_qt;
    if (cross) {
        for (int q = tid; q < nA; q += kSelBlock) slot[q] = kEmptySlot;
        __threadfence();  // the slots may live in the workspace: other waves' atomics follow
        __syncthreads();
        for (int i = tid; i < nB; i += kSelBlock) {
            const gms_dmatch m = back[i];
            if ((unsigned)m.trainIdx < (unsigned)nA) atomicMin((unsigned long long*)&slot[m.trainIdx], (unsigned long long)bfsel::slot_key(m.distance, i));
        }
    } else {
        for (int q = tid; q < nA; q += kSelBlock) {
            const gms_dmatch m = back[q];
            slot[q] = bfsel::slot_key(m.distance, m.trainIdx);
        }
    }
    __threadfence();
    __syncthreads();

    // ---- compaction in query order: candidate k = (d, q, t); in place in the workspace when the slots live there -----------------
    int n_cand = 0;
    float dmin = INFINITY;
    for (int q0 = 0; q0 < nA; q0 += kSelBlock) {
        const int q = q0 + tid;
        const uint64_t k = q < nA ? slot[q] : kEmptySlot;
        const bool keep = k != kEmptySlot;
        int cnt;
        const int pos = n_cand + block_prefix(keep, s_cnt, &cnt);  // (its barrier orders this chunk's reads before the writes)
        if (keep) {
            const float d = bfsel::slot_dist(k);
            g_qt[pos] = (uint64_t)(uint32_t)q | ((uint64_t)(uint32_t)bfsel::slot_row(k) << 32);
            g_d[pos] = d;
            dmin = fminf(dmin, d);
        }
        n_cand += cnt;
    }
    __threadfence();  // candidates in the workspace, read by other waves below
    __syncthreads();
    // d_min over the workgroup
    for (int s = 32; s > 0; s >>= 1) dmin = fminf(dmin, __shfl_xor(dmin, s));
    if (lane == 0) s_min[wave] = dmin;
    __syncthreads();
    dmin = s_min[0];
    for (int w = 1; w < kSelWaves; w++) dmin = fminf(dmin, s_min[w]);

    // ---- K = min(max_size, #{d : !(d_min * coef < d)}) ---------------------------------------------------------------------------
    int64_t n_in = 0;
    for (int k = tid; k < n_cand; k += kSelBlock) n_in += bfsel::within_ratio(g_d[k], dmin, coef) ? 1 : 0;
    for (int s = 32; s > 0; s >>= 1) n_in += __shfl_xor(n_in, s);
    if (lane == 0) s_n[wave] = n_in;
    __syncthreads();
    n_in = 0;
    for (int w = 0; w < kSelWaves; w++) n_in += s_n[w];
    const int64_t K = n_in < (int64_t)max_size ? n_in : (int64_t)max_size;
    st.n_cand = n_cand;
    st.n_ratio = n_in;
    st.n_out = K;
    st.d_min = n_cand > 0 ? dmin : 0.0f;
    if (n_cand == 0) st.status = GMS_ERR_DOMAIN;
    else if (K > (int64_t)pr.m) st.status = GMS_ERR_CAPACITY;
    if (st.status != GMS_OK) {
        if (tid == 0) write_results(p, st, res, pres);
        return;  // workgroup-uniform
    }

    // ---- the first K places of MSVC std::sort over the candidates in query order, then the survivors ------------------------------
    gms_dmatch* __restrict__ o = out + pr.match_off;
    if (n_cand <= kLdsRecs) {
        float* sd = reinterpret_cast<float*>(s_buf);
        int32_t* six = reinterpret_cast<int32_t*>(s_buf) + kLdsRecs;
        for (int k = tid; k < n_cand; k += kSelBlock) {
            sd[k] = g_d[k];
            six[k] = k;
        }
        __syncthreads();
        if (tid == 0) bfsel::msvc_sort_prefix(sd, six, n_cand, K, s_stack);
        __syncthreads();
        for (int r = tid; r < K; r += kSelBlock) {
            const uint64_t v = g_qt[six[r]];
            o[r] = gms_dmatch{(int32_t)(uint32_t)v, (int32_t)(uint32_t)(v >> 32), 0, sd[r]};
        }
    } else {
        for (int k = tid; k < n_cand; k += kSelBlock) g_ix[k] = k;
        __threadfence();
        __syncthreads();
        if (tid == 0) bfsel::msvc_sort_prefix(g_d, g_ix, n_cand, K, s_stack);
        __threadfence();
        __syncthreads();
        for (int r = tid; r < K; r += kSelBlock) {
            const uint64_t v = g_qt[g_ix[r]];
            o[r] = gms_dmatch{(int32_t)(uint32_t)v, (int32_t)(uint32_t)(v >> 32), 0, g_d[r]};
        }
    }
    if (tid == 0) write_results(p, st, res, pres);
}

}  // namespace

size_t bf_select_ws_bytes(int n_pairs, int64_t max_rows, int64_t total_back) { return bf_select_layout(n_pairs, max_rows, total_back).total; }

hipError_t launch_bf_select(int kind, const void* d_desc, const void* d_prep, int64_t total, const int64_t* d_frame_off, int n_frames,
                            const gms_pair* d_pairs, int n_pairs, int max_rows, int64_t total_back, int cross, double coef, int max_size,
                            void* d_ws, gms_dmatch* d_out, gms_bf_result* d_res, gms_pair_result* d_pres, hipStream_t stream)
{
    if (n_pairs <= 0) return hipSuccess;
    const BfSelectLayout L = bf_select_layout(n_pairs, max_rows, total_back);
    const SelWs ws = {ws_ptr<gms_pair>(d_ws, L.pairs2), ws_ptr<gms_dmatch>(d_ws, L.back), ws_ptr<uint64_t>(d_ws, L.qt), ws_ptr<float>(d_ws, L.cd),
                      ws_ptr<int32_t>(d_ws, L.cix)};
    hipLaunchKernelGGL(bf_sel_plan_kernel, dim3(1), dim3(kPlanBlock), 0, stream, d_pairs, n_pairs, d_frame_off, n_frames, max_rows,
                       cross, total_back, ws.pairs2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (max_rows > 0 && total_back > 0) {
        e = launch_bf_match(kind, d_desc, d_prep, total, d_frame_off, n_frames, ws.pairs2, n_pairs, max_rows, ws.back, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bf_select_kernel, dim3((uint32_t)n_pairs), dim3(kSelBlock), 0, stream, d_pairs, d_frame_off, n_frames,
                       max_rows, cross, coef, max_size, ws, d_out, d_res, d_pres);
    return hipGetLastError();
}

}  // namespace gms
